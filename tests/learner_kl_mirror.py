"""The KL estimate of the device learner's early stop (uavtrack_learner_set_kl_stop), restated as include/uavtrack.h states
it: the float32 ratios r_i widened to float64; k_i = (r_i - 1) - log r_i, two subtractions and a log as written; the sum in
the order of the advantage statistics (learner_advantage_mirror.ordered_sum: chunks of 256 rows, the last padded with
zeros, the halving tree inside a chunk, chunk sums ascending from 0.0); kl = float32(sum / n).  The statistic is unweighted.
r == 1 gives exactly 0, r == 0 gives +inf."""
import numpy as np

from learner_advantage_mirror import ordered_sum


def terms(ratio32):
    """k_i in float64 of the float32 ratios."""
    r = np.asarray(ratio32, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return (r - 1.0) - np.log(r)


def kl64(ratio32):
    """sum / n before the rounding to float32."""
    k = terms(ratio32)
    return ordered_sum(k) / np.float64(len(k))


def kl(ratio32):
    """What the library leaves in kl_out."""
    return np.float32(kl64(ratio32))


def stops(ratio32, limit):
    """kl > (float)limit, compared in float32."""
    with np.errstate(over="ignore"):
        return bool(kl(ratio32) > np.float32(limit))


def ulps(x, y):
    """Distance of two finite non-negative float32 values in units of the last place."""
    a, b = (int(np.float32(v).view(np.int32)) for v in (x, y))
    return abs(a - b)
