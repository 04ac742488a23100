"""float64 numpy mirror of the device learner (ActorCritic.update, actor_critic.py:150-179, + torch.optim.Adam, and what
include/uavtrack.h adds to it), the yardstick of the learner's tests.  One forward, one set of per-row terms, one
backward; every option of the update is an argument of those, and an option left at its default changes no bit.

Parameters travel as one flat blob in torch order (actor fc1.weight [H][12], fc1.bias, fc2.weight [A][H], fc2.bias, then
the critic's four tensors); a target critic theta is the critic's block, 14 H + 1 words.  With y_i = r_i + d_i V(s'_i)
(d a scalar gamma or one discount per row; V the target critic's where theta is given), delta_i = y_i - V(s_i), one
weight w_i >= 0 per row (None: ones) and means that divide by the row count n:
    critic_loss               = mean_i( w_i (V(s_i) - y_i)^2 )
    actor_loss, "reference"   = mean_i( -w_i log p_i(a_i) ) * mean_j( w_j delta_j )
    actor_loss, "per_sample"  = mean_i( w_i ( -log p_i(a_i) delta_i - c H_i ) ),   H_i = -sum_o p_io log p_io
    clip = (log_mu, eps)      : -log p_i(a_i) delta_i becomes -min(r_i delta_i, clamp(r_i, lo, hi) delta_i), with
                                r_i = exp(log p_i(a_i) - log_mu_i) and lo, hi = 1 -+ eps as float32 values; the row
                                passes (its gradient is r_i delta_i's) where r_i <= hi for delta_i >= 0, r_i >= lo for < 0
    dL/dz_io                  = -(1/n) w_i ( k_i (onehot - p_i)_o - c p_io (log p_io + H_i) ),  k_i = mean_j(w_j delta_j),
                                delta_i, or (pass_i ? r_i delta_i : 0)
td_delta stays the unweighted delta.  Every log p comes from the logits, (z - max) - log sum exp(z - max), so nothing
needs a probability to be representable: a probability of exactly 0 adds 0 to H and to its gradient.

The split update (uavtrack_learner_grad / _apply): `shard_sums` is a shard's UNSCALED gradient and loss sums, `combine`
adds rows in order and scales once by the global n; `losses_and_grads` is `combine` of the one row of a whole batch.
Gradient-norm clipping is torch.nn.utils.clip_grad_norm_ per network: coef = min(1, max_norm / (norm + 1e-6))."""
import collections
import types

import numpy as np

Update = collections.namedtuple("Update", "actor_loss critic_loss td grad entropy ratio")


# ---- layout ----------------------------------------------------------------------------------------------------------

def layout(H, A):
    sizes = [12 * H, H, A * H, A, 12 * H, H, H, 1]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return sizes, offs


def unpack(blob, H, A):
    sizes, o = layout(H, A)
    t = [np.asarray(blob[o[i]:o[i + 1]], np.float64) for i in range(8)]
    return t[0].reshape(H, 12), t[1], t[2].reshape(A, H), t[3], t[4].reshape(H, 12), t[5], t[6].reshape(1, H), t[7]


def critic_block(blob, H, A):
    """The critic's 14 H + 1 words of a parameter blob, as a copy."""
    return np.array(blob[layout(H, A)[1][4]:], copy=True)


def with_critic(blob, H, A, theta):
    """The blob with theta in the critic's place."""
    out = np.array(blob, copy=True)
    out[layout(H, A)[1][4]:] = theta
    return out


def _critic(theta, H, x):
    """(pre-activations, hidden, V [n], fc2.weight [1][H]) of the critic block theta on rows x."""
    theta = np.asarray(theta, np.float64)
    w1, b1, w2, b2 = theta[:12 * H].reshape(H, 12), theta[12 * H:13 * H], theta[13 * H:14 * H].reshape(1, H), theta[14 * H]
    pc = np.asarray(x, np.float64) @ w1.T + b1; hc = np.maximum(pc, 0)
    return pc, hc, (hc @ w2.T)[:, 0] + b2, w2


def values64(theta, H, x):
    """V(x) of the critic block theta in float64."""
    return _critic(theta, H, x)[2]


# ---- forward, terms, backward ----------------------------------------------------------------------------------------

def _actor(blob, H, A, s):
    w1a, b1a, w2a, b2a = unpack(blob, H, A)[:4]
    s = np.asarray(s, np.float64).reshape(-1, 12)
    pa = s @ w1a.T + b1a; ha = np.maximum(pa, 0)
    z = ha @ w2a.T + b2a
    d = z - z.max(axis=1, keepdims=True)
    logp = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    entropy = -np.where(p > 0, p * logp, 0.0).sum(axis=1)
    return types.SimpleNamespace(s=s, pa=pa, ha=ha, z=z, logp=logp, p=p, entropy=entropy, w2a=w2a)


def logits(blob, H, A, s):
    """z [n][A] of the actor on states s."""
    return _actor(blob, H, A, s).z


def policy(blob, H, A, s):
    """(log p [n][A], p, entropy [n]) of the actor on states s, from the logits."""
    f = _actor(blob, H, A, s)
    return f.logp, f.p, f.entropy


def forward(blob, H, A, s, a, r, s2, discount, theta=None):
    """Both networks on one batch: the record s, a, n, pa, ha, logp, p, entropy, pc, hc, v, target, delta, onehot, w2a,
    w2c.  discount: gamma or one value per row; theta: the block V(s') is taken from, None for the critic's own."""
    f = _actor(blob, H, A, s)
    own = critic_block(blob, H, A)
    f.a = np.asarray(a, np.int64)
    f.n = len(f.a)
    f.pc, f.hc, f.v, f.w2c = _critic(own, H, f.s)
    f.target = np.asarray(r, np.float64) + np.asarray(discount, np.float64) * values64(own if theta is None else theta, H, s2)
    f.delta = f.target - f.v
    f.onehot = np.zeros_like(f.p); f.onehot[np.arange(f.n), f.a] = 1
    return f


def terms(f, loss, weights=None, entropy_coef=0.0, clip=None):
    """The unscaled per-row pieces of forward record f: (logit weights gz [n][A], value weights gv [n], the four loss
    terms lt [4][n] -- -w log p, w delta, the per-sample actor term, w (V - y)^2 --, the ratios [n] or None)."""
    c = float(entropy_coef)
    if c != 0 and loss != "per_sample":
        raise ValueError("the entropy bonus exists for the per-sample loss only")
    if clip is not None and loss != "per_sample":
        raise ValueError("the clipped surrogate exists for the per-sample loss only")
    n, delta = f.n, f.delta
    iw = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    assert iw.shape == (n,)
    lp = f.logp[np.arange(n), f.a]
    if clip is None:
        ratio = None
        k = delta if loss == "per_sample" else np.ones(n)
        actor = -lp * delta
    else:
        log_mu, eps = clip
        lo, hi = bounds(eps)
        ratio = np.exp(lp - np.asarray(log_mu, np.float64))
        ok = gate(ratio, delta, eps)
        with np.errstate(invalid="ignore"):
            actor = -np.where(ok, ratio * delta, np.where(delta >= 0, hi, lo) * delta)
        k = np.where(ok, ratio * delta, 0.0)
    eg = np.where(f.p > 0, f.p * (f.logp + f.entropy[:, None]), 0.0)
    gz = iw[:, None] * (k[:, None] * (f.onehot - f.p) - c * eg)
    gv = (f.v - f.target) * iw
    lt = np.stack([-lp * iw, delta * iw, iw * (actor - c * f.entropy), (f.v - f.target) ** 2 * iw])
    return gz, gv, lt, ratio


def backward(f, gz, gv):
    """The flat sums [P] from the logit weights [n][A] and the value weights [n]."""
    g_w2a = gz.T @ f.ha; g_b2a = gz.sum(0)
    dha = (gz @ f.w2a) * (f.pa > 0)
    g_w1a = dha.T @ f.s; g_b1a = dha.sum(0)
    g_w2c = (gv[:, None] * f.hc).sum(0)[None, :]; g_b2c = np.array([gv.sum()])
    dhc = gv[:, None] * f.w2c * (f.pc > 0)
    g_w1c = dhc.T @ f.s; g_b1c = dhc.sum(0)
    return np.concatenate([g.ravel() for g in (g_w1a, g_b1a, g_w2a, g_b2a, g_w1c, g_b1c, g_w2c, g_b2c)])


def bounds(eps):
    """(lo, hi) of the clipped surrogate as float64 values of the float32 bounds the host folds from (float)eps."""
    e = np.float32(eps)
    with np.errstate(over="ignore"):
        return float(np.float32(1.0) - e), float(np.float32(1.0) + e)


def gate(ratio, delta, eps):
    """pass_i of every row, inclusive at the bound."""
    lo, hi = bounds(eps)
    return np.where(delta >= 0, ratio <= hi, ratio >= lo)


# ---- rows and the whole update ---------------------------------------------------------------------------------------

def shard_sums(blob, H, A, s, a, r, s2, discount, loss="reference", weights=None, entropy_coef=0.0, clip=None,
               theta=None):
    """One gradient row in float64: {"g": unscaled gradient sums [P], "loss": the four loss sums, "n": the row count
    (whatever the weights), "td", "entropy" [n], "ratio" [n] or None}."""
    f = forward(blob, H, A, s, a, r, s2, discount, theta)
    gz, gv, lt, ratio = terms(f, loss, weights, entropy_coef, clip)
    return {"g": backward(f, gz, gv), "loss": lt.sum(axis=1), "n": f.n, "td": f.delta, "entropy": f.entropy,
            "ratio": ratio}


def combine(rows, H, A, loss="reference"):
    """(actor_loss, critic_loss, gradient [P]) of the ONE update the rows make: sums added in row order, N = sum n, the
    actor scaled by the GLOBAL -mean(delta) / N (reference) or -1 / N (per_sample), the critic by 2 / N."""
    g = np.zeros_like(rows[0]["g"])
    ls = np.zeros(4)
    N = 0
    for row in rows:
        g = g + row["g"]; ls = ls + row["loss"]; N += row["n"]
    mean_delta = ls[1] / N
    actor_loss = (ls[0] / N) * mean_delta if loss == "reference" else ls[2] / N
    na = layout(H, A)[1][4]
    scale = np.concatenate([np.full(na, -mean_delta / N if loss == "reference" else -1.0 / N), np.full(g.size - na, 2.0 / N)])
    return actor_loss, ls[3] / N, g * scale


def losses_and_grads(blob, H, A, s, a, r, s2, discount, loss="reference", **options):
    """One update of the whole batch, before any gradient-norm clip: Update(actor_loss, critic_loss, td, grad, entropy,
    ratio); options as shard_sums'."""
    row = shard_sums(blob, H, A, s, a, r, s2, discount, loss, **options)
    al, cl, g = combine([row], H, A, loss)
    return Update(al, cl, row["td"], g, row["entropy"], row["ratio"])


def averaged_shard_gradients(blob, H, A, shards, gamma, loss="reference"):
    """The rule the split is NOT: every shard's own loss gradient (its own mean(delta) for the reference loss),
    averaged over the shards."""
    return np.mean([losses_and_grads(blob, H, A, s, a, r, s2, gamma, loss).grad for s, a, r, s2 in shards], axis=0)


# ---- gradient-norm clipping, Adam ------------------------------------------------------------------------------------

def norms(grad, H, A):
    """The actor's and the critic's gradient norm."""
    na = layout(H, A)[1][4]
    return np.array([np.sqrt((grad[:na] ** 2).sum()), np.sqrt((grad[na:] ** 2).sum())])


def clip_grad_norm(grad, H, A, max_norms):
    """clip_grad_norm_ per network: (coef [2], norms [2], clipped flat gradient); max_norms = (actor, critic), inf = off."""
    na = layout(H, A)[1][4]
    nr = norms(grad, H, A)
    coef = np.array([1.0 if np.isinf(m) else min(1.0, m / (x + 1e-6)) for m, x in zip(max_norms, nr)])
    out = np.array(grad, np.float64, copy=True)
    out[:na] *= coef[0]
    out[na:] *= coef[1]
    return coef, nr, out


def adam(blob, m, v, step, grad, lrs, H, A):
    """torch.optim.Adam defaults; step [8] per tensor (already advanced); lrs = (actor_lr, critic_lr)."""
    sizes, o = layout(H, A)
    blob, m, v = blob.astype(np.float64).copy(), m.astype(np.float64).copy(), v.astype(np.float64).copy()
    for t in range(8):
        sl = slice(o[t], o[t + 1])
        lr = lrs[0] if t < 4 else lrs[1]
        m[sl] = 0.9 * m[sl] + 0.1 * grad[sl]
        v[sl] = 0.999 * v[sl] + 0.001 * grad[sl] ** 2
        bc1, bc2 = 1 - 0.9 ** step[t], 1 - 0.999 ** step[t]
        blob[sl] -= lr / bc1 * m[sl] / (np.sqrt(v[sl]) / np.sqrt(bc2) + 1e-8)
    return blob, m, v


def _step(state, g, lrs, H, A, max_norms):
    if max_norms is not None:
        g = clip_grad_norm(g, H, A, max_norms)[2]
    step = np.asarray(state["step"], np.int64) + 1
    p, m, v = adam(state["params"], state["exp_avg"], state["exp_avg_sq"], step, g, lrs, H, A)
    return {"params": p, "exp_avg": m, "exp_avg_sq": v, "step": step}


def update(state, H, A, s, a, r, s2, discount, lrs, loss="reference", max_norms=None, **options):
    """state = dict(params, exp_avg, exp_avg_sq, step [8]) -> (new state, actor_loss, critic_loss, td_delta); options as
    shard_sums', max_norms as clip_grad_norm's.  A target critic's sync rule is not part of it (polyak / periodic)."""
    u = losses_and_grads(state["params"], H, A, s, a, r, s2, discount, loss, **options)
    return _step(state, u.grad, lrs, H, A, max_norms), u.actor_loss, u.critic_loss, u.td


def update_from_rows(state, rows, H, A, lrs, loss="reference", max_norms=None):
    """update with the gradient taken from rows: (new state, actor_loss, critic_loss)."""
    al, cl, g = combine(rows, H, A, loss)
    return _step(state, g, lrs, H, A, max_norms), al, cl


# ---- the target critic's two sync rules, in float32 ------------------------------------------------------------------

def polyak(t, w, tau):
    """t <- fl(fl(omt * t) + fl(tau32 * w)) per word, tau32 = (float)tau and omt = 1.0f - tau32: two float32 multiplies
    and one float32 add, each rounded on its own."""
    tau32 = np.float32(tau)
    omt = np.float32(np.float32(1.0) - tau32)
    t, w = np.asarray(t, np.float32), np.asarray(w, np.float32)
    a = np.multiply(omt, t, dtype=np.float32)
    b = np.multiply(tau32, w, dtype=np.float32)
    return np.add(a, b, dtype=np.float32)


def periodic(t, w, step, period):
    """t <- w when the critic's step count (already advanced by the update) is a multiple of period."""
    return np.array(w if int(step) % int(period) == 0 else t, np.float32, copy=True)


def last_wins(prio, idx, values):
    """PrioritizedReplayBuffer.update_priorities (train.py:136-138): a sequential loop, the last write wins."""
    out = np.array(prio, copy=True)
    for i, x in zip(idx, values):
        out[i] = x
    return out
