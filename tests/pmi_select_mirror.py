"""uavtrack_pmi_trainer_select / _train_many's gather restated in numpy (include/uavtrack.h, "One observation history
among several"), and the recomposition DevicePMINetwork.train_pmi(group=...) trains from.

A group is n_uav consecutive rows; the timeline of a source list is the concatenation of the sources' groups in list
order.  locate() finds a group's source by the same binary search over the exclusive prefix sum of the group counts
that pmi_select_kernel runs; select() writes the two rows of every draw whose group lies in the list's span and leaves
the others alone; recompose() reads draw i out of the rank-major block of per-rank selected buffers at
t' = owner(i) * b2 + i."""
import numpy as np


def bases(group_counts, group_base=0):
    """base[k] of every source and the span's end: [K + 1] int64."""
    return group_base + np.concatenate([[0], np.cumsum(np.asarray(group_counts, np.int64))])


def locate(base, t):
    """The source whose span [base[k], base[k + 1]) holds group t (which lies in [base[0], base[-1]))."""
    lo, hi = 0, len(base) - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if t >= base[mid]:
            lo = mid
        else:
            hi = mid
    return lo


def select(sources, n_uav, t_idx, u_idx, selected, group_base=0, total_groups=None):
    """sources: list of [n_rows_k, 12] arrays holding groups [group_base, group_base + sum of their groups) of a
    timeline of total_groups; selected [b2, 2, 12] is written in place for the draws inside that span.  A draw outside
    [0, total_groups) x [0, n_uav) refuses the call: nothing is written and False comes back."""
    base = bases([s.shape[0] // n_uav for s in sources], group_base)
    if total_groups is None:
        total_groups = int(base[-1])
    t_idx, u_idx = np.asarray(t_idx), np.asarray(u_idx)
    if ((t_idx < 0) | (t_idx >= total_groups)).any() or ((u_idx < 0) | (u_idx >= n_uav)).any():
        return False
    for i, t in enumerate(t_idx):
        if t < base[0] or t >= base[-1]:
            continue
        k = locate(base, t)
        for side in range(2):
            selected[i, side] = sources[k][(t - base[k]) * n_uav + u_idx[i, side]]
    return True


def owner(group_counts, t_idx):
    """The rank whose span of the timeline holds each draw's group."""
    base = bases(group_counts)
    return np.array([locate(base, t) for t in np.asarray(t_idx)], np.int64)


def recompose(blocks, group_counts, t_idx):
    """blocks: one [b2, 2, 12] selected buffer per rank.  Their rank-major concatenation is a history of R * b2 groups
    of 2 rows; draw i reads group t' = owner(i) * b2 + i with u' = (0, 1).  Returns ([b2, 2, 12], t')."""
    b2 = len(t_idx)
    block = np.concatenate(blocks).reshape(-1, 12)
    t2 = owner(group_counts, t_idx) * b2 + np.arange(b2)
    return np.stack([block[t2 * 2], block[t2 * 2 + 1]], axis=1), t2
