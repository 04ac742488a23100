"""uavtrack_episode_stats_* restated in numpy (include/uavtrack.h, "per-episode results"): the same fp64 sums in the same
order, the same record order, the same overflow rule.  tests/test_episode_stats_cpu.py holds this mirror to the
reference's arithmetic (train.py:181-192 in Python floats) on recorded episodes; tests/test_hip_episode_stats.py holds
the kernels to the mirror, bit for bit.

Order of the sums: the N values of a step in ascending UAV index, starting from +0.0; the step sums into the episode's
accumulator in ascending t.  numpy's own reductions (pairwise) are never used on the values."""
import numpy as np

RECORD_DTYPE = np.dtype([("ret", "<f8"), ("tracking", "<f8"), ("boundary", "<f8"), ("duplicate", "<f8"),
                         ("average_covered", "<f8"), ("max_covered", "<f8"), ("env", "<i8"), ("steps", "<i4"),
                         ("ordinal", "<i4")])
FIELDS = ("ret", "tracking", "boundary", "duplicate")


def step_sums(reward, terms):
    """reward [T, B, N], terms [T, 3, B, N] (fp32) -> [T, 4, B] fp64: each step's sum over the UAVs, ascending index."""
    reward, terms = np.asarray(reward, np.float32), np.asarray(terms, np.float32)
    T, B, N = reward.shape
    planes = np.concatenate([reward[:, None], terms], axis=1)           # [T, 4, B, N]
    s = np.zeros((T, 4, B), np.float64)
    for i in range(N):
        s = s + planes[..., i].astype(np.float64)
    return s


class EpisodeStatsMirror:
    def __init__(self, n_envs, n_uav, log_capacity, env_offset=0):
        self.B, self.N, self.cap, self.env_offset = n_envs, n_uav, log_capacity, env_offset
        self.acc = np.zeros((4, n_envs), np.float64)
        self.cov_sum = np.zeros(n_envs, np.int64)
        self.cov_max = np.zeros(n_envs, np.int32)
        self.steps = np.zeros(n_envs, np.int32)
        self.ordinal = np.zeros(n_envs, np.int32)
        self.log = []
        self.dropped = 0

    def _close(self, b):
        if len(self.log) < self.cap:
            r = np.zeros((), RECORD_DTYPE)
            den = np.float64(int(self.steps[b]) * self.N)
            for p, f in enumerate(FIELDS):
                r[f] = self.acc[p, b] / den
            r["average_covered"] = np.float64(int(self.cov_sum[b])) / np.float64(int(self.steps[b]))
            r["max_covered"] = np.float64(int(self.cov_max[b]))
            r["env"], r["steps"], r["ordinal"] = self.env_offset + b, self.steps[b], self.ordinal[b]
            self.log.append(r)
        else:
            self.dropped += 1
        self.acc[:, b] = 0.0
        self.cov_sum[b] = 0
        self.cov_max[b] = 0
        self.steps[b] = 0
        self.ordinal[b] += 1

    def add(self, reward, terms, covered, done=None):
        s = step_sums(reward, terms)
        covered = np.asarray(covered, np.int32)
        T = s.shape[0]
        for t in range(T):
            self.acc = self.acc + s[t]                                   # every environment, ascending t
            self.cov_sum += covered[t]
            self.cov_max = np.where((self.steps == 0) | (covered[t] > self.cov_max), covered[t], self.cov_max).astype(np.int32)
            self.steps += 1
            if done is not None:
                for b in np.flatnonzero(np.asarray(done[t])):            # ascending b within the row
                    self._close(int(b))

    def close(self):
        for b in np.flatnonzero(self.steps > 0):
            self._close(int(b))

    def clear(self):
        self.log, self.dropped = [], 0

    def records(self):
        return np.array(self.log, RECORD_DTYPE) if self.log else np.zeros(0, RECORD_DTYPE)
