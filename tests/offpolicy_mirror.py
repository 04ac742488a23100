"""float64 numpy mirror of the actor alone and of the truncated importance ratios (uavtrack_learner_log_probs,
_log_probs_window, _ratio_weights), the window an add of n rows writes, and the bounds the device is held to.  The
actor is tests/learner_mirror.py's; imports no uavtrack.

    log p_a = (z_a - max_o z_o) - log sum_o exp(z_o - max),   z = W2a relu(W1a s + b1a) + b2a
    rho_i   = min(float32(rho_bar), exp(log p_i - log_mu_i)),  NaN where log_mu_i is NaN or > 0, where the slot lies
              outside the store or the action outside [0, A)
    w_i     = w_in_i * rho_i   (w_in None: ones)
"""
import numpy as np

import learner_mirror as mirror


def log_probs(blob, H, A, s, a):
    """log pi(a_i | s_i) in float64 [n]; NaN where a_i is outside [0, A)."""
    logp = mirror.policy(blob, H, A, s)[0]
    a = np.asarray(a, np.int64).reshape(-1)
    ok = (a >= 0) & (a < A)
    return np.where(ok, logp[np.arange(len(a)), np.where(ok, a, 0)], np.nan)


def scale(blob, H, A, s):
    """max_o |z_o| + log A per row: the scale of the log-softmax's inputs, which the bound on log p is taken at."""
    return np.abs(mirror.logits(blob, H, A, s)).max(axis=1) + np.log(A)


def log_prob_bound(blob, H, A, s):
    """|device - mirror| of log p per row: the learner tests' 2e-5 at the scale of the log-softmax's inputs."""
    return 2e-5 * scale(blob, H, A, s)


def weights(blob, H, A, s, a, log_mu, rho_bar, w_in=None):
    """(weights [n], rho [n]) in float64 of rows (s_i, a_i) whose behaviour log-probabilities are log_mu_i.  rho_bar is
    rounded to float32 first, as the device takes it; +inf does not truncate."""
    lp = log_probs(blob, H, A, s, a)
    lm = np.asarray(log_mu, np.float64).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        rho = np.minimum(np.float64(np.float32(rho_bar)), np.exp(lp - lm))
    rho = np.where((lm <= 0) & ~np.isnan(lp), rho, np.nan)
    w = rho if w_in is None else np.asarray(w_in, np.float64).reshape(-1) * rho
    return w, rho


def ratio_bound(rho64, b):
    """|rho_dev - rho_64| where log p is within b of the mirror's and both sides read the same float32 log_mu: the
    exponent is off by at most b plus the rounding of one subtraction and of expf, together below 2 b."""
    return rho64 * np.expm1(2 * b) + 1e-37


def window_slots(pos, n, capacity):
    """(slots, rows): the slots an add of n rows into a ring at `pos` leaves written, in ring order from the first one,
    and the row of the add each holds.  Only the last min(n, capacity) rows are kept."""
    k = min(n, capacity)
    rows = np.arange(n - k, n)
    return (pos + rows) % capacity, rows
