"""Integer numpy mirror of the uniform replay draw (uavtrack_replay_sample_uniform, uavtrack.ReplayRing), restated from
the stream documented in include/uavtrack.h: draw j of call c is pi_c(j), a balanced Feistel network on b bits keyed by
Philox4x32-10(seed, c), walked along its cycle until the value falls below count.  Every operation is an integer one,
so the device's indices are reproduced exactly."""
import numpy as np

from replay_mirror import M32, philox_np

DOMAIN = 0x554E4946          # "UNIF": Philox counter word 3 of the uniform draw's round keys
ROUNDS = 16                  # Feistel rounds (kUniformRounds, csrc/replay_kernel.hip)

_U32 = np.uint64(M32)


def width(count):
    """b: the even number of bits of the walk's domain [0, 2^b): count <= 2^b < 4 * count, b >= 2."""
    b = max(2, (int(count) - 1).bit_length())
    return b + (b & 1)


def round_keys(seed, calls, rounds=ROUNDS):
    """[len(calls), rounds] round keys: key 4 i + w is word w of Philox(counter = (i, c lo, c hi, "UNIF"), key = seed)."""
    calls = np.atleast_1d(np.asarray(calls, dtype=np.uint64))
    out = np.empty((len(calls), 4 * (-(-rounds // 4))), np.uint64)
    for i in range(out.shape[1] // 4):
        r = philox_np(i, calls & _U32, calls >> np.uint64(32), DOMAIN, seed & M32, (seed >> 32) & M32)
        for w in range(4):
            out[:, 4 * i + w] = r[w]
    return out[:, :rounds]


def fmix32(x):
    """murmur3's 32-bit finaliser, on uint64 arrays holding 32-bit values."""
    x = x & _U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & _U32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & _U32
    x ^= x >> np.uint64(16)
    return x


def permute(x, keys, b):
    """pi on [0, 2^b): x [calls, k] uint64, keys [calls, rounds].  (L, R) <- (R, L ^ (fmix32(R + key_r) mod 2^(b/2)))."""
    h = np.uint64(b // 2)
    mask = np.uint64((1 << (b // 2)) - 1)
    L, R = x >> h, x & mask
    for r in range(keys.shape[1]):
        L, R = R, L ^ (fmix32(R + keys[:, r:r + 1]) & mask)
    return (L << h) | R


def draw_calls(count, k, seed, calls, rounds=ROUNDS):
    """[len(calls), k] int64: the k indices of each of the given call numbers."""
    b = width(count)
    keys = round_keys(seed, calls, rounds)
    x = np.broadcast_to(np.arange(k, dtype=np.uint64), (keys.shape[0], k)).copy()
    x = permute(x, keys, b)
    while True:
        out = x >= np.uint64(count)
        if not out.any():
            return x.astype(np.int64)
        rows = np.flatnonzero(out.any(axis=1))
        sub = x[rows]
        x[rows] = np.where(out[rows], permute(sub, keys[rows], b), sub)


def draw(count, k, seed=0, call=0):
    """indices [k] of call number `call` on a ring of `count` valid slots keyed by seed."""
    return draw_calls(count, k, seed, [call])[0]
