"""The prioritised replay mirror (tests/replay_mirror.py) on the CPU: its selection against np.random.choice's rule
given the same uniforms, the tiled search of the device against the flat one, its u mapping, and the ring add."""
import ctypes as C

import numpy as np
import pytest

import replay_mirror as mirror


def _choice_rule(w, u):
    """np.random.choice's selection (numpy/random/mtrand.pyx): cdf = cumsum(p); cdf /= cdf[-1];
    searchsorted(cdf, u, side='right')."""
    cdf = np.cumsum(np.asarray(w, np.float64))
    cdf /= cdf[-1]
    return np.searchsorted(cdf, u, side="right")


def _exact_weights(rng, n, zero_frac=0.0, total_log2=40):
    """Integer weights whose sum is a power of two: every cdf entry, cdf / total and u * total is exact in fp64."""
    w = rng.randint(1, 1000, size=n).astype(np.float64)
    w[rng.rand(n) < zero_frac] = 0
    if w.sum() == 0:
        w[-1] = 1
    rest = 2.0 ** total_log2 - w.sum()
    nz = np.flatnonzero(w)
    w[nz[-1]] += rest
    assert np.cumsum(w)[-1] == 2.0 ** total_log2
    return w


@pytest.mark.parametrize("n,zero_frac", [(1, 0.0), (5, 0.0), (2048, 0.3), (3 * 2048 + 17, 0.5), (10007, 0.9)])
def test_select_equals_choice_rule(n, zero_frac):
    rng = np.random.RandomState(n)
    w = _exact_weights(rng, n, zero_frac)
    u = np.concatenate([rng.rand(5000), [0.0, 1.0 - 2.0 ** -53]])
    idx, _ = mirror.select(w, u)
    assert np.array_equal(idx, _choice_rule(w, u))
    assert (idx < n).all() and (w[idx] > 0).all()
    # the boundaries themselves: u exactly at cdf[i] / total goes to the next slot with w > 0 (side='right')
    cdf = np.cumsum(w)
    ub = cdf[:-1] / cdf[-1]
    ub = ub[ub < 1.0]                     # u never reaches 1
    idx_b, _ = mirror.select(w, ub)
    assert np.array_equal(idx_b, _choice_rule(w, ub))
    assert (w[idx_b] > 0).all()


def test_last_slot_and_count_one():
    w = np.array([0.0, 0.0, 3.0], np.float32)
    u = np.array([0.0, 0.5, 1.0 - 2.0 ** -53])
    assert mirror.select(w, u)[0].tolist() == [2, 2, 2]
    assert mirror.select(np.array([7.0], np.float32), u)[0].tolist() == [0, 0, 0]
    # u * total rounding up to total falls on the last slot with w > 0, never on count
    w = np.array([1.0, 0.0], np.float32)
    assert mirror.select(w, np.array([1.0 - 2.0 ** -53]))[0].tolist() == [0]


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 5 * 2048 + 1000])
def test_tiled_search_equals_flat_search(n):
    rng = np.random.RandomState(7 + n)
    w = _exact_weights(rng, n, zero_frac=0.4, total_log2=24).astype(np.float32)     # integers <= 2^24: exact in fp32
    ub = np.cumsum(w, dtype=np.float64)[:-1][:200] / 2.0 ** 24
    u = np.concatenate([rng.rand(2000), ub[ub < 1.0]])
    flat, _ = mirror.select(w, u)
    assert np.array_equal(mirror.select_tiled(w, u), flat)


def test_tiled_search_never_a_bad_slot_under_rounding():
    rng = np.random.RandomState(3)
    n = 3 * 2048 + 5
    p = np.where(rng.rand(n) < 0.95, 0.0, 2.0 ** rng.uniform(-40, 40, n)).astype(np.float32)
    w = mirror.weights_fp32(p, 0.6)
    u = np.concatenate([rng.rand(3000), [1.0 - 2.0 ** -53]])
    idx = mirror.select_tiled(w, u)
    assert (idx < n).all() and (w[idx] > 0).all()


def test_u_mapping_spans_unit_interval():
    assert mirror.u53(0, 0) == 0.0
    assert mirror.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert mirror.u53(0x80000000, 0) == 0.5
    assert mirror.u53(0, 1 << 11) == 2.0 ** -53                     # the lowest of r1's 21 kept bits
    assert mirror.u53(0, (1 << 11) - 1) == 0.0                       # r1's low 11 bits are dropped
    u = mirror.uniforms(seed=5, call=0, k=4000)
    assert (u >= 0).all() and (u < 1).all()
    assert abs(u.mean() - 0.5) < 0.02 and u.min() < 0.01 and u.max() > 0.99


def test_uniforms_follow_the_counter_layout():
    from oracle import philox4x32_10
    seed, call = 0x123456789ABCDEF0, (7 << 32) | 3
    r = philox4x32_10([4, 3, 7, mirror.DOMAIN], [seed & 0xFFFFFFFF, seed >> 32])
    assert mirror.uniforms(seed, call, 5)[4] == mirror.u53(r[0], r[1])
    assert not np.array_equal(mirror.uniforms(seed, 0, 16), mirror.uniforms(seed, 1, 16))
    assert not np.array_equal(mirror.uniforms(1, 0, 16), mirror.uniforms(2, 0, 16))


def test_importance_weights():
    w = np.array([1.0, 2.0, 4.0, 0.0], np.float32)
    idx = np.array([0, 2, 2, 1])
    got = mirror.importance(w, idx, 7.0, 4, 0.4)
    P = w[idx].astype(np.float64) / 7.0
    ref = (4 * P) ** -0.4
    assert np.allclose(got, ref / ref.max(), rtol=1e-15) and got.max() == 1.0


def test_ring_add_matches_the_reference_semantics():
    cap = 10
    store = {"states": np.zeros((cap, 12), np.float32), "actions": np.zeros(cap, np.int32),
             "rewards": np.zeros(cap, np.float32), "next_states": np.zeros((cap, 12), np.float32)}
    prio = np.zeros(cap, np.float32)

    def trans(n, base):
        return {"states": np.full((n, 12), base, np.float32) + np.arange(n)[:, None],
                "actions": (np.arange(n) + base).astype(np.int32), "rewards": np.arange(n, dtype=np.float32) + base,
                "next_states": np.full((n, 12), -base, np.float32) - np.arange(n)[:, None]}

    pos, count = mirror.ring_add(store, prio, 0, 0, cap, trans(4, 100))
    assert (pos, count) == (4, 4) and (prio[:4] == 1).all() and (prio[4:] == 0).all()
    prio[2] = 5.0
    pos, count = mirror.ring_add(store, prio, pos, count, cap, trans(8, 200))     # wraps
    assert (pos, count) == (2, 10)
    assert store["actions"].tolist() == [206, 207, 102, 103, 200, 201, 202, 203, 204, 205]
    assert prio.tolist() == [5, 5, 5, 1, 5, 5, 5, 5, 5, 5]
    pos, count = mirror.ring_add(store, prio, pos, count, cap, trans(23, 300))    # n > capacity: the last 10
    assert (pos, count) == (5, 10)
    assert sorted(store["actions"].tolist()) == list(range(313, 323))
    assert store["actions"][(2 + 13) % cap] == 313


def test_ring_structs_match_header_layout():
    from uavtrack import _lib
    assert C.sizeof(_lib.ReplayConfig) == 4 + 4 + 8 + 8 + 8
    assert C.sizeof(_lib.ReplayRing) == 5 * 8 + 3 * 8
    assert _lib.ReplayRing.capacity.offset == 40


def test_replay_abi_refuses_without_a_gpu_handle():
    from uavtrack import _lib
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.ReplayConfig(struct_size=C.sizeof(_lib.ReplayConfig) + 1, device_id=0, max_capacity=16, max_batch=4)
    assert lib.uavtrack_replay_create(C.byref(cfg), C.byref(h)) != 0
    assert b"struct_size" in lib.uavtrack_last_error()
    cfg = _lib.ReplayConfig(struct_size=C.sizeof(_lib.ReplayConfig), device_id=0, max_capacity=0, max_batch=4)
    assert lib.uavtrack_replay_create(C.byref(cfg), C.byref(h)) != 0
    assert b"max_capacity" in lib.uavtrack_last_error()
    ring = _lib.ReplayRing(capacity=4, pos=0, count=4)
    assert lib.uavtrack_replay_sample(None, C.byref(ring), 1, 0.6, 0.4, None, None, None) != 0
    assert b"null handle" in lib.uavtrack_last_error()
    assert lib.uavtrack_replay_destroy(None) == 0
