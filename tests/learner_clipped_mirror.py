"""float64 numpy mirror of the clipped-surrogate update (uavtrack_learner_update_clipped / _grad_clipped), built on
tests/learner_regularised_mirror.py.  Per-sample form only.  With r_i = exp(log p_i(a_i) - log_mu_i), A_i = delta_i (a
constant of the differentiation), lo = 1 - eps and hi = 1 + eps as the float32 values the host folds:
    pass_i     = r_i <= hi  where A_i >= 0,   r_i >= lo  where A_i < 0            (inclusive)
    surr_i     = min(r_i A_i, clip(r_i, lo, hi) A_i)  =  r_i A_i where pass_i, else (hi or lo) A_i
    actor_loss = mean_i( w_i ( -surr_i - c H_i ) )
    dL/dz_io   = -(1/n) w_i ( (pass_i ? r_i A_i : 0) (onehot - p_i)_o - c p_io (log p_io + H_i) )
The critic, td_delta and the entropy term are learner_regularised_mirror's.

The batches: log_mu is the float64 log p of the case's blob plus a seeded offset in [-1.5, 1.5], so the ratios lie in
[e^-1.5, e^1.5] and eps in {0.1, 0.2} clips a good share on both sides.  The gate is discontinuous at its boundary, where
float32 may decide otherwise than float64: a row whose float64 ratio lies within a relative 1e-4 of the boundary that
decides it is nudged away when the batch is built; nothing is set aside at run time."""
import numpy as np

import learner_regularised_mirror as rm
import learner_weighted_mirror as wm

NEAR = 1e-4          # relative distance from the deciding boundary inside which the builder moves a row
NUDGE = 1e-2         # how far (in log mu) it moves it


def bounds(eps):
    """(lo, hi) as float64 values of the float32 bounds the host folds from (float)eps."""
    e = np.float32(eps)
    with np.errstate(over="ignore"):
        return float(np.float32(1.0) - e), float(np.float32(1.0) + e)


def gate(ratio, delta, eps):
    """pass_i of every row."""
    lo, hi = bounds(eps)
    return np.where(delta >= 0, ratio <= hi, ratio >= lo)


def _terms(blob, H, A, s, a, r, s2, gamma, log_mu, eps, weights, c):
    """The unscaled per-row pieces: forward dict, logit weights [n][A], value weights [n], the four loss terms, entropy,
    ratios."""
    with np.errstate(divide="ignore"):
        f = wm._forward(blob, H, A, s, a, r, s2, gamma)
    n, delta, v, target = f["n"], f["delta"], f["v"], f["target"]
    iw = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    assert iw.shape == (n,)
    logp, p, ent = rm.policy(blob, H, A, s)
    lp = logp[np.arange(n), np.asarray(a, np.int64)]
    ratio = np.exp(lp - np.asarray(log_mu, np.float64))
    lo, hi = bounds(eps)
    ok = gate(ratio, delta, eps)
    with np.errstate(invalid="ignore"):
        surr = np.where(ok, ratio * delta, np.where(delta >= 0, hi, lo) * delta)
    pg = np.where(ok, ratio * delta, 0.0)[:, None] * (f["onehot"] - p)
    eg = np.where(p > 0, p * (logp + ent[:, None]), 0.0)
    gz = iw[:, None] * (pg - c * eg)
    gv = (v - target) * iw
    lt = np.stack([-lp * iw, delta * iw, iw * (-surr - c * ent), (v - target) ** 2 * iw])
    return f, gz, gv, lt, ent, ratio


def losses_and_grads(blob, H, A, s, a, r, s2, gamma, log_mu, eps, weights=None, entropy_coef=0.0):
    """(actor_loss, critic_loss, td_delta, flat gradient, entropy [n], ratios [n]) of one clipped update in float64."""
    f, gz, gv, lt, ent, ratio = _terms(blob, H, A, s, a, r, s2, gamma, log_mu, eps, weights, float(entropy_coef))
    n = f["n"]
    return lt[2].mean(), lt[3].mean(), f["delta"], wm._backward(f, -gz / n, 2 * gv / n), ent, ratio


def shard_sums(blob, H, A, s, a, r, s2, gamma, log_mu, eps, weights=None, entropy_coef=0.0):
    """One clipped gradient row in float64, in learner_dp_mirror.shard_sums' form: learner_dp_mirror.combine(rows, H, A,
    "per_sample") adds such rows, with plain per-sample rows if it is given some, and scales them once."""
    f, gz, gv, lt, ent, ratio = _terms(blob, H, A, s, a, r, s2, gamma, log_mu, eps, weights, float(entropy_coef))
    return {"g": wm._backward(f, gz, gv), "loss": lt.sum(axis=1), "n": f["n"], "td": f["delta"], "entropy": ent,
            "ratio": ratio}


def make_log_mu(blob, H, A, s, a, r, s2, gamma, seed, eps_list=(0.1, 0.2)):
    """float32 log_mu [n] in batch-row order for the rows (s, a, r, s2): the float64 log p of `blob` plus a seeded offset
    in [-1.5, 1.5], every row nudged until its float64 ratio (against the float32 log_mu) is farther than a relative
    NEAR from the boundary that decides it, for every eps of eps_list; clamped to <= 0 (a log-probability)."""
    n = len(a)
    logp = rm.policy(blob, H, A, s)[0][np.arange(n), np.asarray(a, np.int64)]
    delta = wm._forward(blob, H, A, s, a, r, s2, gamma)["delta"]
    off = np.random.RandomState(seed).uniform(-1.5, 1.5, size=n)
    mu = np.minimum(logp + off, 0.0).astype(np.float32)
    for _ in range(8):
        near = near_boundary(logp, mu, delta, eps_list)
        if not near.any():
            break
        mu[near] = (mu[near].astype(np.float64) - NUDGE).astype(np.float32)      # downwards: stays <= 0, the ratio grows
    assert not near_boundary(logp, mu, delta, eps_list).any()
    return mu


def near_boundary(logp, log_mu, delta, eps_list):
    """Rows whose float64 ratio lies within a relative NEAR of the boundary that decides them, for some eps of the list."""
    ratio = np.exp(logp - np.asarray(log_mu, np.float64))
    near = np.zeros(len(ratio), bool)
    for eps in eps_list:
        lo, hi = bounds(eps)
        edge = np.where(delta >= 0, hi, lo)
        near |= np.abs(ratio - edge) <= NEAR * edge
    return near


def census(ratio, delta, eps):
    """(rows gated where A >= 0, rows gated where A < 0, rows passing)."""
    ok = gate(ratio, delta, eps)
    return int((~ok & (delta >= 0)).sum()), int((~ok & (delta < 0)).sum()), int(ok.sum())


# ---- the cases of tests/test_hip_learner_clipped.py, built without a GPU -------------------------------------------------

GAMMA = 0.95
# (H, A, n, gathered): corners of learner_harness.SWEEP; at (256, 48, 4113) workgroups loop over tiles and LDS is at its largest
SHAPES = [(1, 2, 1, False), (33, 12, 63, True), (128, 48, 65, False), (128, 12, 4096, True), (256, 48, 4113, True)]
EPS = (0.1, 0.2)

_batches = {}


def host_case(H, A, n, gather):
    """The host half of learner_harness.case(H, A, n, gather), drawn the same way: (blob, store batch, capacity, indices).
    The GPU tests assert that it is that case's."""
    import learner_dp_mirror as dp
    rng = np.random.RandomState(H * 1000 + n + (7 if gather else 0))
    cap = n + 7 if gather else n
    b = dp.batch(rng, cap, A)
    idx = rng.randint(0, cap, size=n).astype(np.int64) if gather else np.arange(n)
    return dp.init_blob(H, A, H + n), b, cap, idx


def premises(blob, H, A, b, idx, log_mu, gamma=GAMMA, eps_list=EPS):
    """Per eps: census of the drawn rows, and whether any drawn row sits near its boundary."""
    rows = tuple(x[idx] for x in b)
    logp = rm.policy(blob, H, A, rows[0])[0][np.arange(len(idx)), rows[1].astype(np.int64)]
    delta = wm._forward(blob, H, A, *rows, gamma)["delta"]
    ratio = np.exp(logp - log_mu[idx].astype(np.float64))
    return {eps: census(ratio, delta, eps) for eps in eps_list}, bool(near_boundary(logp, log_mu[idx], delta, eps_list).any()), ratio


def decides(counts, n):
    """A case shows the gate: at least one row gated on each side and one passing; a batch of fewer than three rows cannot
    hold all three kinds, and must then hold a gated row."""
    return all((hi > 0 and lo > 0 and ok > 0) if n >= 3 else (hi + lo > 0) for hi, lo, ok in counts.values())


def clip_batch(H, A, n, gather, b=None, gamma=GAMMA):
    """The clipped case over learner_harness.case(H, A, n, gather): that case's host arrays and a per-SLOT float32 log_mu
    [capacity] by make_log_mu over the whole store, with the first offset seed (from the case's own) for which the drawn
    rows show the gate (decides).  b, gamma: the store batch and discount the deltas are formed from, where they are not
    the case's own (a target critic folded into the rewards with gamma = 0)."""
    key = (H, A, n, gather, None if b is None else b[2].tobytes(), gamma)
    if key not in _batches:
        blob, b0, cap, idx = host_case(H, A, n, gather)
        bb = b0 if b is None else b
        for seed in range(H + n, H + n + 64):
            log_mu = make_log_mu(blob, H, A, *bb, gamma, seed)
            counts, near, _ = premises(blob, H, A, bb, idx, log_mu, gamma)
            if decides(counts, n) and not near:
                break
        else:
            raise AssertionError(f"no offset seed makes the case {(H, A, n, gather)} decide anything")
        _batches[key] = dict(blob=blob, b=b0, cap=cap, idx=idx, log_mu=log_mu, seed=seed)
    return _batches[key]
