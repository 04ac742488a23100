"""The batches of the clipped-surrogate update's tests (uavtrack_learner_update_clipped / _grad_clipped); the update itself
is tests/learner_mirror.py's with clip=(log_mu, eps), whose `bounds` and `gate` are the ones named here.

log_mu is the float64 log p of the case's blob plus a seeded offset in [-1.5, 1.5], so the ratios lie in [e^-1.5, e^1.5]
and eps in {0.1, 0.2} clips a good share on both sides.  The gate is discontinuous at its boundary, where float32 may
decide otherwise than float64: a row whose float64 ratio lies within a relative 1e-4 of the boundary that decides it is
nudged away when the batch is built; nothing is set aside at run time."""
import numpy as np

import learner_harness as lh
import learner_mirror as mirror
from learner_mirror import bounds, gate                                                  # noqa: F401

NEAR = 1e-4          # relative distance from the deciding boundary inside which the builder moves a row
NUDGE = 1e-2         # how far (in log mu) it moves it


def _logp_and_delta(blob, H, A, s, a, r, s2, gamma, theta):
    f = mirror.forward(blob, H, A, s, a, r, s2, gamma, theta)
    return f.logp[np.arange(f.n), f.a], f.delta


def make_log_mu(blob, H, A, s, a, r, s2, gamma, seed, eps_list=(0.1, 0.2), theta=None):
    """float32 log_mu [n] in batch-row order for the rows (s, a, r, s2): the float64 log p of `blob` plus a seeded offset
    in [-1.5, 1.5], every row nudged until its float64 ratio (against the float32 log_mu) is farther than a relative
    NEAR from the boundary that decides it, for every eps of eps_list; clamped to <= 0 (a log-probability).  theta: the
    target critic the deltas bootstrap from."""
    logp, delta = _logp_and_delta(blob, H, A, s, a, r, s2, gamma, theta)
    off = np.random.RandomState(seed).uniform(-1.5, 1.5, size=len(a))
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


def premises(blob, H, A, b, idx, log_mu, gamma=GAMMA, eps_list=EPS, theta=None):
    """Per eps: census of the drawn rows, and whether any drawn row sits near its boundary."""
    rows = tuple(x[idx] for x in b)
    logp, delta = _logp_and_delta(blob, H, A, *rows, gamma, theta)
    ratio = np.exp(logp - log_mu[idx].astype(np.float64))
    return {eps: census(ratio, delta, eps) for eps in eps_list}, bool(near_boundary(logp, log_mu[idx], delta, eps_list).any()), ratio


def decides(counts, n):
    """A case shows the gate: at least one row gated on each side and one passing; a batch of fewer than three rows cannot
    hold all three kinds, and must then hold a gated row."""
    return all((hi > 0 and lo > 0 and ok > 0) if n >= 3 else (hi + lo > 0) for hi, lo, ok in counts.values())


def clip_batch(H, A, n, gather, theta=None):
    """The clipped case over learner_harness.case(H, A, n, gather): that case's host arrays and a per-SLOT float32 log_mu
    [capacity] by make_log_mu over the whole store, with the first offset seed (from the case's own) for which the drawn
    rows show the gate (decides).  theta: the target critic the deltas bootstrap from, where it is not the critic."""
    key = (H, A, n, gather, None if theta is None else theta.tobytes())
    if key not in _batches:
        blob, b, cap, idx = lh.host_case(H, A, n, gather)
        for seed in range(H + n, H + n + 64):
            log_mu = make_log_mu(blob, H, A, *b, GAMMA, seed, theta=theta)
            counts, near, _ = premises(blob, H, A, b, idx, log_mu, theta=theta)
            if decides(counts, n) and not near:
                break
        else:
            raise AssertionError(f"no offset seed makes the case {(H, A, n, gather)} decide anything")
        _batches[key] = dict(blob=blob, b=b, cap=cap, idx=idx, log_mu=log_mu, seed=seed)
    return _batches[key]
