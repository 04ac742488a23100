"""The batch-normalised advantage of the device learner (uavtrack_learner_set_advantage) on top of tests/learner_mirror.py,
which needs no change: `forward`, the standardised advantage in f.delta's place, `terms` / `backward` / `combine`, and the
raw sum w delta back in loss word 1.  The critic's terms come from f.v - f.target and never see the advantage.

The statistics are restated exactly as include/uavtrack.h orders them: the float32 delta widened to float64; rows in
chunks of 256 consecutive rows, the last chunk padded with zeros; inside a chunk the halving tree x[k] += x[k + h],
h = 128 .. 1; the chunk sums added in ascending chunk order from 0.0.  S = sum delta, mean64 = S / n;
Q = sum (delta - mean64)^2 (difference, product and adds as separate float64 operations); std64 = sqrt(Q / (n - 1));
inv64 = 1 / (std64 + eps); stats = float32 of (mean64, inv64, std64).  A_i = fl(fl(delta_i - mean32) * inv32) in float32.

The cases are learner_harness.host_case batches with the rewards shifted by +3 (a critic that is wrong by about 3, so most
raw TD errors share a sign that the standardised advantage does not), and for the clipped surrogate a log_mu of
log p -+ 0.4 (ratios of about 0.67 and 1.49: beyond [0.8, 1.2] on either side, never near a boundary)."""
import types

import numpy as np
import torch

import learner_harness as lh
import learner_mirror as mirror

GAMMA = lh.GAMMA
SHIFT = 3.0
CHUNK = 256
# (H, A, n, gathered): the smallest legal batch; one chunk plus one row, no multiple of the tile; the harness's teeth
# batch size; the largest LDS footprint with a last tile of one row (16 rows per tile at H = 256)
SHAPES = [(32, 12, 2, False), (33, 9, 257, True), (128, 12, 6007, False), (256, 48, 4097, True)]
EPS_CLIP = 0.2


# ---- the statistics --------------------------------------------------------------------------------------------------

def ordered_sum(x):
    """The documented order over float64 terms x [n]."""
    x = np.asarray(x, np.float64)
    chunks = -(-len(x) // CHUNK)
    c = np.zeros(chunks * CHUNK)
    c[:len(x)] = x
    c = c.reshape(chunks, CHUNK)
    h = CHUNK // 2
    while h >= 1:
        c[:, :h] = c[:, :h] + c[:, h:2 * h]
        h //= 2
    total = np.float64(0.0)
    for s in c[:, 0]:
        total = total + s
    return total


def stats(td32, eps=1e-8):
    """(mean64, inv64, std64) of the float32 TD errors td32 [n], n >= 2."""
    x = np.asarray(td32, np.float32).astype(np.float64)
    n = len(x)
    assert n >= 2
    mean = ordered_sum(x) / np.float64(n)
    d = x - mean
    std = np.sqrt(ordered_sum(d * d) / np.float64(n - 1))
    with np.errstate(divide="ignore"):
        inv = np.float64(1.0) / (std + np.float64(eps))
    return mean, inv, std


def stats32(td32, eps=1e-8):
    """What the library leaves in its three floats."""
    return np.array(stats(td32, eps), np.float64).astype(np.float32)


def standardise(td32, mean32, inv32):
    """A_i = fl(fl(delta_i - mean32) * inv32), float32."""
    d = np.subtract(np.asarray(td32, np.float32), np.float32(mean32), dtype=np.float32)
    return np.multiply(d, np.float32(inv32), dtype=np.float32)


def ulps(x, y):
    """Distance of two finite float32 values of one sign in units of the last place."""
    a, b = (int(np.float32(v).view(np.int32)) for v in (x, y))
    return abs(a - b)


# ---- rows and the update ---------------------------------------------------------------------------------------------

def shard_sums(blob, H, A, s, a, r, s2, discount, weights=None, entropy_coef=0.0, clip=None, theta=None, given=None,
               eps=1e-8):
    """One gradient row in float64 under a normalised advantage: learner_mirror.shard_sums' record plus "adv" [n] and
    "stats" (mean32, inv32).  given = (mean, inv_std), or None for the batch's own statistics (from delta rounded to
    float32, as the library's TD pass holds it)."""
    f = mirror.forward(blob, H, A, s, a, r, s2, discount, theta)
    delta = f.delta
    td32 = delta.astype(np.float32)
    mean32, inv32 = stats32(td32, eps)[:2] if given is None else (np.float32(given[0]), np.float32(given[1]))
    adv = standardise(td32, mean32, inv32).astype(np.float64)
    f.delta = adv
    gz, gv, lt, ratio = mirror.terms(f, "per_sample", weights, entropy_coef, clip)
    f.delta = delta
    iw = np.ones(f.n) if weights is None else np.asarray(weights, np.float64)
    lt[1] = delta * iw                                               # loss word 1 stays the raw sum w delta
    return {"g": mirror.backward(f, gz, gv), "loss": lt.sum(axis=1), "n": f.n, "td": delta, "entropy": f.entropy,
            "ratio": ratio, "adv": adv, "stats": (mean32, inv32)}


def losses_and_grads(blob, H, A, s, a, r, s2, discount, **options):
    """One update of the whole batch: (learner_mirror.Update, the row's record)."""
    row = shard_sums(blob, H, A, s, a, r, s2, discount, **options)
    al, cl, g = mirror.combine([row], H, A, "per_sample")
    return mirror.Update(al, cl, row["td"], g, row["entropy"], row["ratio"]), row


def autograd(blob, H, A, s, a, r, s2, gamma, adv, weights=None, entropy_coef=0.0, clip=None):
    """torch float64 autograd of mean(w (-A log p - c H)), or of the clipped form mean(w (-min(r A, clamp(r) A) - c H)),
    with the advantage `adv` [n] a constant, and of the critic's mean(w (V - y)^2): (actor_loss, critic_loss, grad [P])."""
    t = [torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in mirror.unpack(blob, H, A)]
    w1a, b1a, w2a, b2a, w1c, b1c, w2c, b2c = t
    S, S2, R = (torch.from_numpy(np.asarray(x, np.float64)) for x in (s, s2, r))
    n = len(a)
    W = torch.ones(n, dtype=torch.float64) if weights is None else torch.from_numpy(np.asarray(weights, np.float64))
    Adv = torch.from_numpy(np.asarray(adv, np.float64))
    critic = lambda x: (torch.relu(x @ w1c.T + b1c) @ w2c.T)[:, 0] + b2c[0]                            # noqa: E731
    logp = torch.log_softmax(torch.relu(S @ w1a.T + b1a) @ w2a.T + b2a, dim=1)
    ent = -(logp.exp() * logp).sum(dim=1)
    target = (R + gamma * critic(S2)).detach()
    v = critic(S)
    lpa = logp.gather(1, torch.from_numpy(np.asarray(a, np.int64)).view(-1, 1))[:, 0]
    if clip is None:
        al = torch.mean(W * (-lpa * Adv - entropy_coef * ent))
    else:
        ratio = torch.exp(lpa - torch.from_numpy(np.asarray(clip[0], np.float64)))
        lo, hi = mirror.bounds(clip[1])
        al = torch.mean(W * (-torch.min(ratio * Adv, ratio.clamp(lo, hi) * Adv) - entropy_coef * ent))
    cl = torch.mean(W * (v - target) ** 2)
    al.backward(); cl.backward()
    return float(al.detach()), float(cl.detach()), np.concatenate([x.grad.numpy().ravel() for x in t])


# ---- the cases, built without a GPU ----------------------------------------------------------------------------------

_cases = {}


def host_case(H, A, n, gather, shift=SHIFT):
    """learner_harness.host_case with the rewards shifted, and a per-slot float32 log_mu of log p -+ 0.4: the record
    blob, b (the store's four arrays), cap, idx, log_mu [cap]."""
    key = (H, A, n, gather, shift)
    if key not in _cases:
        blob, (s, a, r, s2), cap, idx = lh.host_case(H, A, n, gather)
        r = (r + np.float32(shift)).astype(np.float32)
        logp = mirror.policy(blob, H, A, s)[0][np.arange(cap), a.astype(np.int64)]
        sign = np.where(np.random.RandomState(H + n + 5).randint(0, 2, size=cap) == 1, 0.4, -0.4)
        log_mu = np.minimum(logp + sign, 0.0).astype(np.float32)
        _cases[key] = types.SimpleNamespace(blob=blob, b=(s, a, r, s2), cap=cap, idx=idx, log_mu=log_mu, H=H, A=A, n=n,
                                            gather=gather)
    return _cases[key]


def rows(c):
    """The batch rows of a case in batch order."""
    return lh.gathered(c.b, c.idx)


def weights(n):
    return lh.make_weights(np.random.RandomState(n + 23), n)


def census(c, eps=EPS_CLIP, theta=None):
    """Of a case's batch: (mean32, std32, rows whose advantage changes sign, rows whose gate outcome differs between
    delta_i and A_i, rows whose float64 ratio lies within a relative 1e-4 of a clip boundary)."""
    f = mirror.forward(c.blob, c.H, c.A, *rows(c), GAMMA, theta)
    td32 = f.delta.astype(np.float32)
    st = stats32(td32)
    adv = standardise(td32, st[0], st[1]).astype(np.float64)
    ratio = np.exp(f.logp[np.arange(f.n), f.a] - c.log_mu[c.idx].astype(np.float64))
    lo, hi = mirror.bounds(eps)
    near = (np.abs(ratio - lo) <= 1e-4 * lo) | (np.abs(ratio - hi) <= 1e-4 * hi)
    flips = (f.delta >= 0) != (adv >= 0)
    differ = mirror.gate(ratio, f.delta, eps) != mirror.gate(ratio, adv, eps)
    return float(st[0]), float(st[2]), int(flips.sum()), int(differ.sum()), int(near.sum())
