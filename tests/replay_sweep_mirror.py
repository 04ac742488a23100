"""Integer numpy mirror of the sweep draw (uavtrack_replay_sample_sweep, uavtrack.RingSweep), restated from the stream
documented in include/uavtrack.h: call q over a window of W slots from `first` on is minibatch m = q mod M of epoch
e = q div M, M = W div n, and its entry j is (first + sigma_e(m n + j)) mod capacity, sigma_e the uniform draw's Feistel
network keyed by Philox4x32-10(seed, e) under the domain word "SWEP", walked along its cycle until the value falls
below W.  Every operation is an integer one, so the device's indices are reproduced exactly."""
import numpy as np

from replay_mirror import M32, philox_np
from replay_uniform_mirror import ROUNDS, permute, width

DOMAIN = 0x53574550          # "SWEP": Philox counter word 3 of the sweep's round keys

_U32 = np.uint64(M32)


def round_keys(seed, epochs, rounds=ROUNDS):
    """[len(epochs), rounds] round keys: key 4 i + w is word w of Philox(counter = (i, e lo, e hi, "SWEP"), key = seed)."""
    epochs = np.atleast_1d(np.asarray(epochs, dtype=np.uint64))
    out = np.empty((len(epochs), 4 * (-(-rounds // 4))), np.uint64)
    for i in range(out.shape[1] // 4):
        r = philox_np(i, epochs & _U32, epochs >> np.uint64(32), DOMAIN, seed & M32, (seed >> 32) & M32)
        for w in range(4):
            out[:, 4 * i + w] = r[w]
    return out[:, :rounds]


def walk(x, keys, W):
    """sigma on the starts x [rows, k] uint64 (all below W), keys [rows, rounds]: pi applied until the value is below W."""
    b = width(W)
    x = permute(x, keys, b)
    while True:
        out = x >= np.uint64(W)
        if not out.any():
            return x
        rows = np.flatnonzero(out.any(axis=1))
        sub = x[rows]
        x[rows] = np.where(out[rows], permute(sub, keys[rows], b), sub)


def sigma(W, seed, epoch):
    """[W] int64: sigma_e(0), ..., sigma_e(W - 1), the order in which epoch e goes through the window's offsets."""
    x = np.arange(W, dtype=np.uint64)[None, :].copy()
    return walk(x, round_keys(seed, [epoch]), W)[0].astype(np.int64)


def sweep_calls(capacity, first, W, n, seed, calls):
    """[len(calls), n] int64: the ring slots of each of the given call numbers."""
    calls = np.atleast_1d(np.asarray(calls, dtype=np.uint64))
    M = np.uint64(W // n)
    e, m = calls // M, calls % M
    x = (m * np.uint64(n))[:, None] + np.arange(n, dtype=np.uint64)[None, :]
    x = walk(x, round_keys(seed, e), W)
    return ((np.uint64(first) + x) % np.uint64(capacity)).astype(np.int64)


def sweep_call(capacity, first, W, n, seed=0, call=0):
    """indices [n] of call number `call`."""
    return sweep_calls(capacity, first, W, n, seed, [call])[0]
