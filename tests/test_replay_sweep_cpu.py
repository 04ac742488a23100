"""The sweep draw (uavtrack_replay_sample_sweep, uavtrack.RingSweep) without a GPU: the new symbol in the header, the
library and the binding; the integer mirror of the documented stream (tests/replay_sweep_mirror.py): every epoch's
minibatches are disjoint and, where the minibatch divides the window, cover it; and the argument refusals of ring.sweep
that need no device."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import replay_sweep_mirror as mirror
import replay_uniform_mirror as umirror
from conftest import ROOT

WINDOWS = [1, 2, 5, 64, 65, 257, 2049, 4099]
EPOCHS = [0, 1, 7, (1 << 32) + 3]


# ---- symbols, ABI, argument errors -------------------------------------------------------------------------------------

def test_header_library_and_binding_declare_the_sweep():
    from uavtrack import _lib
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    name = "uavtrack_replay_sample_sweep"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, name
    args = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert args == ["uavtrack_replay *replay", "const uavtrack_replay_ring *ring", "int64_t first", "int64_t length",
                    "int64_t n", "uint64_t *cursor", "int64_t *indices", "void *stream"]
    assert hasattr(_lib.load(), name)
    res, bound = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert bound == [C.c_void_p, C.POINTER(_lib.ReplayRing), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                     C.c_void_p]
    assert "0x53574550" in hdr and mirror.DOMAIN == 0x53574550 == int.from_bytes(b"SWEP", "big")
    assert mirror.DOMAIN not in (umirror.DOMAIN, 0x52504C59, 0x55415631, 0x4143544F)     # "UNIF", "RPLY", "UAV1", "ACTO"
    # the uniform draw's declaration is what it was
    m = re.search(r"\bint\s+uavtrack_replay_sample_uniform\s*\(([^;]*)\)\s*;", hdr)
    assert [" ".join(x.split()) for x in m.group(1).split(",")] == [
        "uavtrack_replay *replay", "const uavtrack_replay_ring *ring", "int64_t n", "int64_t *indices", "void *stream"]


def test_sweep_refuses_without_a_gpu_handle():
    from uavtrack import _lib
    lib = _lib.load()
    ring = _lib.ReplayRing(capacity=4, pos=0, count=4)
    assert lib.uavtrack_replay_sample_sweep(None, C.byref(ring), 0, 4, 1, None, None, None) != 0
    assert b"uavtrack_replay_sample_sweep: null handle" in lib.uavtrack_last_error()


# ---- the mirror ---------------------------------------------------------------------------------------------------------

def test_round_keys_follow_the_counter_layout():
    from oracle import philox4x32_10
    seed, epoch = 0x123456789ABCDEF0, (7 << 32) | 3
    keys = mirror.round_keys(seed, [epoch])[0]
    assert len(keys) == 16
    for i in range(4):
        r = philox4x32_10([i, 3, 7, mirror.DOMAIN], [seed & 0xFFFFFFFF, seed >> 32])
        assert [int(v) for v in keys[4 * i:4 * i + 4]] == r
    assert not np.array_equal(keys, umirror.round_keys(seed, [epoch])[0])                # another domain word, other keys


def _batch_sizes(W):
    """Minibatch sizes for a window of W: the window itself, 1, a proper divisor where there is one, and sizes that do
    not divide W."""
    divisors = [d for d in range(2, W) if W % d == 0]
    return sorted({1, W, min(W, 16), max(1, W // 3), *(divisors[-1:])})


@pytest.mark.parametrize("W", WINDOWS)
def test_an_epochs_minibatches_are_disjoint_and_cover_the_window_when_n_divides_it(W):
    seed = 3
    for e in EPOCHS:
        perm = mirror.sigma(W, seed, e)
        assert np.array_equal(np.sort(perm), np.arange(W)), e                        # sigma_e permutes [0, W)
        for n in _batch_sizes(W):
            M = W // n
            got = mirror.sweep_calls(W, 0, W, n, seed, e * M + np.arange(M))
            assert got.shape == (M, n)
            assert np.array_equal(got.reshape(-1), perm[:M * n]), (e, n)             # the epoch's permutation, in chunks
            if W % n == 0:
                assert np.array_equal(np.sort(got.reshape(-1)), np.arange(W)), (e, n)
            else:
                assert len(np.unique(got)) == M * n and got.min() >= 0 and got.max() < W, (e, n)
    if W >= 64:
        orders = [tuple(mirror.sigma(W, seed, e)) for e in EPOCHS]
        assert len(set(orders)) == len(EPOCHS)                                       # every epoch another order
        assert not np.array_equal(mirror.sigma(W, seed, 0), mirror.sigma(W, seed + 1, 0))
        assert not np.array_equal(mirror.sigma(W, seed, 0), mirror.sigma(W, seed + (1 << 32), 0))
        assert not np.array_equal(mirror.sigma(W, seed, 0), umirror.draw(W, W, seed, 0))   # not the uniform draw's stream


def test_the_dropped_remainder_changes_from_epoch_to_epoch():
    W, n = 65, 16
    left = [tuple(sorted(set(range(W)) - set(mirror.sweep_calls(W, 0, W, n, 0, 4 * e + np.arange(4)).reshape(-1))))
            for e in range(8)]
    assert all(len(x) == 1 for x in left) and len(set(left)) > 1


@pytest.mark.parametrize("capacity,first,W,n", [(4097, 4000, 257, 64), (4097, 4096, 4097, 241), (65, 3, 65, 16),
                                                (4097, 100, 2049, 128), (5, 4, 1, 1)])
def test_a_wrapped_window_is_first_plus_the_offset_mod_capacity(capacity, first, W, n):
    window = (first + np.arange(W)) % capacity
    M = W // n
    for e in (0, 3, (1 << 32) + 3):
        got = mirror.sweep_calls(capacity, first, W, n, 11, e * M + np.arange(M))
        assert np.array_equal(got.reshape(-1), (first + mirror.sigma(W, 11, e)[:M * n]) % capacity)
        assert len(np.unique(got)) == M * n and np.isin(got, window).all()
        if W % n == 0:
            assert np.array_equal(np.sort(got.reshape(-1)), np.sort(window))
    assert np.array_equal(mirror.sweep_call(capacity, first, W, n, 11, M + 1),
                          mirror.sweep_calls(capacity, first, W, n, 11, [M + 1])[0])


# ---- ring.sweep's own refusals -------------------------------------------------------------------------------------------

def _ring(capacity=100, count=60, last=(40, 20), max_batch=32):
    """What RingSweep reads of a ring before its first library call."""
    return types.SimpleNamespace(capacity=capacity, count=count, _last=last, max_batch=max_batch,
                                 device=torch.device("cpu"))


def test_sweep_windows():
    import uavtrack
    sweep = uavtrack.ReplayRing.sweep
    assert uavtrack.PrioritizedReplayRing.sweep is sweep
    s = sweep(_ring(), 8)
    assert isinstance(s, uavtrack.RingSweep)
    assert s.window == (40, 20) and s.minibatches == 2 and s.count == 20 and s.batch_size == 8
    assert sweep(_ring(), 8, "all").window == (0, 60)
    assert sweep(_ring(), 8, (10, 50)).window == (10, 50)
    full = _ring(count=100, last=(90, 30))
    s = sweep(full, 8)
    assert s.window == (90, 30) and s.minibatches == 3                            # a full ring's window may wrap
    assert sweep(full, 32, "all").window == (0, 100)
    # pinned at creation: a later add does not move it, rebind does
    full._last = (20, 16)
    assert s.window == (90, 30)
    assert s.rebind().window == (20, 16) and s.minibatches == 2


@pytest.mark.parametrize("kwargs,batch,window,match", [
    ({}, 0, "last", "batch_size = 0 outside"),
    ({}, 33, "last", "batch_size = 33 outside .*max_batch = 32"),
    ({}, 21, "last", "batch_size = 21 exceeds the window's 20 slots"),
    ({"last": None}, 8, "last", "before any add"),
    ({"count": 0, "last": None}, 1, "all", "holds 0 slots"),
    ({}, 8, "recent", "window must be"),
    ({}, 8, (1, 2, 3), "window must be"),
    ({}, 8, 5, "window must be"),
    ({}, 8, (0, 0), "holds 0 slots"),
    ({}, 8, (-1, 10), "first = -1 outside"),
    ({}, 8, (100, 10), "first = 100 outside"),
    ({}, 8, (55, 10), "leaves the ring's 60 valid slots"),                        # beyond count on a ring that is not full
    ({}, 8, (0, 61), "leaves the ring's 60 valid slots"),
    ({"count": 100}, 8, (0, 101), "leaves the ring's 100 valid slots"),
])
def test_sweep_refusals(kwargs, batch, window, match):
    import uavtrack
    with pytest.raises(ValueError, match=match):
        uavtrack.ReplayRing.sweep(_ring(**kwargs), batch, window)


def test_rebind_refusal_keeps_the_window_and_seek_checks_its_argument():
    import uavtrack
    ring = _ring()
    s = uavtrack.ReplayRing.sweep(ring, 8)
    ring._last = (0, 4)
    with pytest.raises(ValueError, match="exceeds the window's 4 slots"):
        s.rebind()
    assert s.window == (40, 20)
    with pytest.raises(ValueError, match="seek"):
        s.seek(-1)
    s.seek(5)
    assert s.position() == 5
    s.rebind((0, 16))
    assert s.position() == 0 and s.minibatches == 2


def test_a_sweep_has_no_weights_and_one_batch_size():
    import uavtrack
    from uavtrack.replay import DrawSpec
    s = uavtrack.ReplayRing.sweep(_ring(), 8)
    with pytest.raises(ValueError, match="no importance weights"):
        s._draw_batch(8, DrawSpec(importance=True))
    with pytest.raises(ValueError, match="no importance weights"):
        s._draw_batch(8, DrawSpec(beta_final=1.0, anneal_calls=10))
    with pytest.raises(ValueError, match="batch_size = 4: this sweep was made for minibatches of 8"):
        s._draw_batch(4, DrawSpec())
    assert s.position() == 0
