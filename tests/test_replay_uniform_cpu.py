"""The uniform replay draw (uavtrack_replay_sample_uniform, uavtrack.ReplayRing) without a GPU: the new symbol in the
header, the library and the binding; the struct sizes; the argument errors that need no device; and the integer mirror
of the documented stream (tests/replay_uniform_mirror.py): every call a permutation of [0, count) whose prefixes are the
smaller draws, and the chi-square of its slot and ordered-pair frequencies over 200 000 calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import replay_uniform_mirror as mirror
from conftest import ROOT

COUNTS = [1, 2, 3, 5, 7, 16, 17, 64, 65, 2047, 2048, 2049, 4097]


# ---- symbols, ABI, argument errors -------------------------------------------------------------------------------------

def test_header_library_and_binding_declare_the_uniform_draw():
    from uavtrack import _lib
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    name = "uavtrack_replay_sample_uniform"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, name
    args = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert args == ["uavtrack_replay *replay", "const uavtrack_replay_ring *ring", "int64_t n", "int64_t *indices",
                    "void *stream"]
    assert hasattr(_lib.load(), name)
    res, bound = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert bound == [C.c_void_p, C.POINTER(_lib.ReplayRing), C.c_int64, C.c_void_p, C.c_void_p]
    # the prioritised draw without alpha, beta and weights
    pa = _lib.SIGNATURES["uavtrack_replay_sample"][1]
    assert bound == pa[:3] + [pa[5], pa[7]]
    assert "0x554E4946" in hdr and mirror.DOMAIN == 0x554E4946
    assert mirror.DOMAIN not in (0x52504C59, 0x55415631, 0x4143544F)          # "RPLY", "UAV1", "ACTO"


def test_struct_sizes_are_unchanged():
    from uavtrack import _lib
    assert C.sizeof(_lib.ReplayConfig) == 32
    assert C.sizeof(_lib.ReplayRing) == 64
    assert [f[0] for f in _lib.ReplayRing._fields_] == ["states", "actions", "rewards", "next_states", "priorities",
                                                        "capacity", "pos", "count"]


def test_python_interface():
    import inspect
    import uavtrack
    R, P = uavtrack.ReplayRing, uavtrack.PrioritizedReplayRing
    assert issubclass(P, R) and R.priorities is None
    assert list(inspect.signature(R.__init__).parameters)[1:] == ["capacity", "device", "seed", "max_batch", "obs_dim"]
    ps = inspect.signature(R.__init__).parameters
    assert ps["seed"].default == 0 and ps["max_batch"].default == 65536
    assert list(inspect.signature(P.__init__).parameters)[1:] == ["capacity", "device", "alpha", "seed", "max_batch",
                                                                  "obs_dim"]
    assert list(inspect.signature(R.draw).parameters) == ["self", "batch_size"]
    assert list(inspect.signature(R.sample).parameters) == ["self", "batch_size"]
    for name in ("add", "add_rollout", "size", "check"):
        assert getattr(P, name) is getattr(R, name), name                     # shared, not copied
    assert P.draw is not R.draw and P.sample is not R.sample and P._draw_batch is not R._draw_batch


def test_uniform_draw_refuses_without_a_gpu_handle():
    from uavtrack import _lib
    lib = _lib.load()
    ring = _lib.ReplayRing(capacity=4, pos=0, count=4)
    assert lib.uavtrack_replay_sample_uniform(None, C.byref(ring), 1, None, None) != 0
    assert b"uavtrack_replay_sample_uniform: null handle" in lib.uavtrack_last_error()


# ---- the mirror: a permutation per call ---------------------------------------------------------------------------------

def test_round_keys_follow_the_counter_layout():
    from oracle import philox4x32_10
    seed, call = 0x123456789ABCDEF0, (7 << 32) | 3
    keys = mirror.round_keys(seed, [call])[0]
    assert len(keys) == mirror.ROUNDS == 16
    for i in range(4):
        r = philox4x32_10([i, 3, 7, mirror.DOMAIN], [seed & 0xFFFFFFFF, seed >> 32])
        assert [int(v) for v in keys[4 * i:4 * i + 4]] == r


def test_width():
    assert [mirror.width(c) for c in (1, 2, 4, 5, 16, 17, 64, 65, 2048, 2049, 4097)] == [2, 2, 2, 4, 4, 6, 6, 8, 12, 12, 14]
    for c in COUNTS[1:] + [1 << 25, (1 << 25) + 1, 1 << 41]:
        b = mirror.width(c)
        assert b % 2 == 0 and c <= 1 << b < 4 * c


def test_fmix32_is_murmur3s_finaliser():
    # known values of MurmurHash3's fmix32
    got = mirror.fmix32(np.array([0, 1, 0xFFFFFFFF, 0x12345678], np.uint64))
    ref = []
    for x in (0, 1, 0xFFFFFFFF, 0x12345678):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 16
        ref.append(x)
    assert [int(v) for v in got] == ref and ref[0] == 0 and ref[1] == 0x514E28B7


@pytest.mark.parametrize("count", COUNTS)
def test_every_call_is_a_permutation_and_smaller_draws_are_its_prefix(count):
    calls = np.arange(200)
    full = mirror.draw_calls(count, count, 0, calls)
    assert full.shape == (200, count)
    assert np.array_equal(np.sort(full, axis=1), np.broadcast_to(np.arange(count), full.shape))
    for k in sorted({1, (count + 1) // 2, max(1, count - 1)}):
        assert np.array_equal(mirror.draw_calls(count, k, 0, calls), full[:, :k]), k
    assert np.array_equal(mirror.draw(count, count, 0, 7), full[7])
    if count > 16:
        assert len({tuple(r) for r in full}) == 200                             # every call another permutation


def test_call_numbers_beyond_2_32():
    c = (1 << 32) + 5
    a, b, z = mirror.draw(4097, 4097, 0, c), mirror.draw(4097, 4097, 0, 5), mirror.draw(4097, 4097, 0, c + 1)
    for d in (a, b, z):
        assert np.array_equal(np.sort(d), np.arange(4097))
    assert not np.array_equal(a, b) and not np.array_equal(a, z)
    assert not np.array_equal(mirror.draw(4097, 64, 1, 0), mirror.draw(4097, 64, 1 << 32, 0))    # both seed words key it


# ---- the mirror: statistics ---------------------------------------------------------------------------------------------

def _quantile_9999(dof):
    """The 99.99 % quantile of chi-square(dof), Wilson-Hilferty."""
    return dof * (1 - 2 / (9 * dof) + 3.719 * np.sqrt(2 / (9 * dof))) ** 3


@pytest.mark.parametrize("count,k", [(5, 2), (7, 3), (17, 5), (100, 30), (1000, 8)])
def test_slot_and_pair_frequencies(count, k):
    """Seed 0, calls 0 .. 199 999: the chi-square of the slot frequencies over all k draws (dof count - 1) and of the
    ordered pair of the first two draws (dof count (count - 1) - 1), each below its law's 99.99 % quantile.  Measured
    (slot, pair): (5, 2) 2.1, 11.7; (7, 3) 3.0, 24.5; (17, 5) 4.0, 257.5; (100, 30) 57.9, 9930.1; (1000, 8) 935.9,
    1000178.6."""
    calls = 200_000
    d = np.concatenate([mirror.draw_calls(count, k, 0, np.arange(lo, lo + 50_000)) for lo in range(0, calls, 50_000)])
    assert d.shape == (calls, k) and d.min() >= 0 and d.max() < count
    f = np.bincount(d.reshape(-1), minlength=count).astype(np.float64)
    e = calls * k / count
    slot = ((f - e) ** 2 / e).sum()
    pairs = np.bincount(d[:, 0] * count + d[:, 1], minlength=count * count).reshape(count, count).astype(np.float64)
    assert not np.diag(pairs).any()                                            # without replacement
    e2 = calls / (count * (count - 1))
    pair = ((pairs[~np.eye(count, dtype=bool)] - e2) ** 2 / e2).sum()
    print(f"count {count} k {k}: slot chi2 {slot:.1f} (dof {count - 1}, bound {_quantile_9999(count - 1):.1f}), "
          f"pair chi2 {pair:.1f} (dof {count * (count - 1) - 1}, bound {_quantile_9999(count * (count - 1) - 1):.1f})")
    assert slot < _quantile_9999(count - 1)
    assert pair < _quantile_9999(count * (count - 1) - 1)
