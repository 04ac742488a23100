"""The replay draw on the MI355X against the order-exact mirror (tests/replay_mirror.py, draw_device): indices bit for bit
and weights within one fp32 ulp at non-integer priorities, at the shapes where the kernels change path (one tile, the
1024-tile scan and the first chunked one, 2^25 slots, beyond 2^31), partly filled rings, batch sizes around the draw and
batch-minimum kernels' geometry, rounding gaps built on purpose (the zero-weight draw regression), and the add's
priority maximum at 2^25 slots."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x1_2345_6789                 # >= 2^32: both Philox key words in use
COUNTS = [1, 63, 2047, 2048, 2049, 1024 * 2048, 1024 * 2048 + 1, 3000 * 2048 + 17, 1 << 25, (1 << 25) + 1]


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Handle:
    """uavtrack_replay_* driven directly: only the priorities and count are given, as the sample reads nothing else."""

    def __init__(self, max_capacity, max_batch, seed=SEED):
        from uavtrack import _lib
        self._L, self.lib = _lib, _lib.load()
        cfg = _lib.ReplayConfig(struct_size=C.sizeof(_lib.ReplayConfig), device_id=0, max_capacity=max_capacity,
                                max_batch=max_batch, seed=seed)
        self.h = C.c_void_p()
        _lib.check(self.lib.uavtrack_replay_create(C.byref(cfg), C.byref(self.h)), "uavtrack_replay_create")
        self.calls = 0

    def draw(self, prio, count, k, alpha=1.0, beta=0.4, weights=True):
        """(indices, weights or None, call number) as numpy."""
        ring = self._L.ReplayRing(priorities=prio.data_ptr(), capacity=prio.numel(), pos=0, count=count)
        idx = torch.empty(k, dtype=torch.int64, device=DEV)
        w = torch.empty(k, dtype=torch.float32, device=DEV) if weights else None
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._L.check(self.lib.uavtrack_replay_sample(self.h, C.byref(ring), k, alpha, beta, self._L.ptr(idx),
                                                      self._L.ptr(w), st), "uavtrack_replay_sample")
        self._L.check(self.lib.uavtrack_replay_check(self.h, None, st), "uavtrack_replay_check")
        call, self.calls = self.calls, self.calls + 1
        return idx.cpu().numpy(), (w.cpu().numpy() if weights else None), call

    def close(self):
        self.lib.uavtrack_replay_destroy(self.h)


def _wide(rng, n):
    """Non-integer fp32 priorities over 2^-20 .. 2^20 (fp64 sums round), with zero slots, whole zero lanes and tiles."""
    p = (2.0 ** rng.uniform(-20, 20, n)).astype(np.float32)
    p[rng.rand(n) < 0.2] = 0
    for L in rng.choice(max(1, n // 32), max(1, n // 3000), replace=False):
        p[L * 32:(L + 1) * 32] = 0
    if n > 8 * 2048:
        p[5 * 2048:7 * 2048] = 0
    p[-1] = 1.5
    return p


def _assert_ulps(got, ref, ulps=1):
    """fp32 weights within `ulps` units in the last place (device pow is not correctly rounded)."""
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    d = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert d.max() <= ulps, (d.max(), np.flatnonzero(d > ulps)[:5])


def _check(h, p_dev, p, count, k, calls=1, beta=0.4):
    sums = mirror.tile_sums(mirror.padded(p, count))
    for _ in range(calls):
        idx, w, call = h.draw(p_dev, count, k, beta=beta)
        ref = mirror.draw_device(p, count, 1.0, beta, SEED, call, k, sums=sums)
        assert np.array_equal(idx, ref.indices), (count, call, np.flatnonzero(idx != ref.indices)[:5])
        assert (idx < count).all() and (p[idx] > 0).all()
        _assert_ulps(w, ref.weights)
        assert w.max() == 1.0


def test_bit_exact_non_integer_priorities():
    rng = np.random.RandomState(0)
    p = _wide(rng, COUNTS[-1])
    p_dev = torch.from_numpy(p).to(DEV)
    h = Handle(COUNTS[-1], 4096)
    for count in COUNTS:
        q = p[:count].copy()
        q[-1] = max(q[-1], np.float32(1.0))                 # never an all-zero ring
        p_dev[count - 1] = float(q[-1])
        _check(h, p_dev, q, count, 2048, calls=3 if count < (1 << 25) else 2)
        p_dev[count - 1] = float(p[count - 1])
    h.close()


@pytest.mark.parametrize("capacity,count", [(1 << 22, 3 * 2048 + 17), (1 << 22, 1024 * 2048 + 1), (1 << 22, 1000)])
def test_partly_filled_ring(capacity, count):
    rng = np.random.RandomState(count)
    p = np.full(capacity, 3e38, np.float32)                 # what lies beyond count must never be drawn or summed
    p[:count] = _wide(rng, count)
    h = Handle(capacity, 8192)
    _check(h, torch.from_numpy(p).to(DEV), p[:count], count, 8192, calls=2)
    h.close()


@pytest.mark.parametrize("k", [1, 3, 4097, 4194304 + 4097])
def test_batch_sizes(k):
    rng = np.random.RandomState(k % 1000)
    count = 3 * 2048 + 17
    p = _wide(rng, count)
    h = Handle(count, k)
    p_dev = torch.from_numpy(p).to(DEV)
    h.draw(p_dev, count, 1)                                 # call 0: the counter moves on before the checked call
    idx, w, call = h.draw(p_dev, count, k)
    ref = mirror.draw_device(p, count, 1.0, 0.4, SEED, call, k)
    assert np.array_equal(idx, ref.indices)
    _assert_ulps(w, ref.weights)                            # the batch minimum (across min workgroups) is the mirror's
    assert w.max() == 1.0 and (w[ref.pdraw == ref.pmin] == 1.0).all()
    h.close()


def test_beyond_2_31_slots():
    count = (1 << 31) + 4099
    rng = np.random.RandomState(31)
    special = np.array([0, (1 << 31) - 1, 1 << 31, (1 << 31) + 2048, (1 << 31) + 2047, count - 1], np.int64)
    pos = np.unique(np.concatenate([special, rng.randint(0, count, 300)]))
    val = rng.randint(1, 1000, len(pos)).astype(np.float32)
    val[np.isin(pos, special)] = 100000.0                   # drawn often: every special slot is seen
    prio = torch.zeros(count, dtype=torch.float32, device=DEV)     # 8.6 GB
    prio[torch.from_numpy(pos).to(DEV)] = torch.from_numpy(val).to(DEV)
    k = 8192
    h = Handle(count, k)
    cdf = np.cumsum(val, dtype=np.float64)                  # exact integers: the flat rule is the device's
    seen = set()
    for _ in range(2):
        idx, w, call = h.draw(prio, count, k)
        x = mirror.uniforms_np(SEED, call, k) * cdf[-1]
        ref = pos[np.searchsorted(cdf, x, side="right")]
        assert np.array_equal(idx, ref)
        P = val[np.searchsorted(pos, idx)].astype(np.float64) / cdf[-1]
        _assert_ulps(w, ((count * P) ** -0.4 / (count * P.min()) ** -0.4).astype(np.float32))
        seen |= set(idx.tolist())
    assert set(special.tolist()) <= seen
    h.close()
    del prio


@pytest.mark.parametrize("capacity,count", [(1 << 25, 1 << 25), (1 << 25, (1 << 25) - 12345)])
def test_fractional_alpha_away_from_boundaries(capacity, count):
    rng = np.random.RandomState(9)
    p = np.full(capacity, 1e30, np.float32)
    p[:count] = rng.exponential(1.0, count).astype(np.float32)
    h = Handle(capacity, 4000)
    p_dev = torch.from_numpy(p).to(DEV)
    for _ in range(2):
        idx, w, call = h.draw(p_dev, count, 4000, alpha=0.6, beta=0.7)
        ref_idx, ref_w, u, cdf = mirror.draw(p[:count], count, 0.6, 0.7, SEED, call, 4000)
        # a net 1-ulp powf difference in up to 4096 slots: the full sum (ulp_slots=None) would cover every draw here
        away = ~mirror.near_boundary(u, cdf, ref_idx, mirror.weights_fp32(p[:count], 0.6), ulp_slots=4096)
        assert away.mean() > 0.98
        assert np.array_equal(idx[away], ref_idx[away])
        assert (idx < count).all()
        if np.array_equal(idx, ref_idx):
            np.testing.assert_allclose(w, ref_w, rtol=1e-5)
    h.close()


@pytest.mark.parametrize("kind,nt", [("lane", 4), ("tile", 600), ("tile", 1100)],
                         ids=["lane-gap", "tile-gap", "tile-gap-chunked"])
def test_constructed_gap_draws_a_positive_slot(kind, nt):
    """The regression test: draw j of call 0 is sent, through rounding, to a lane or tile holding no w > 0; slot 0 weighs
    0.  The parent library returned slot 0 there, with weight NaN and every other weight 0."""
    p, count, j = mirror.gap_ring(kind, SEED, ntiles=nt)
    k = 256
    h = Handle(count, k)
    idx, w, call = h.draw(torch.from_numpy(p).to(DEV), count, k)
    assert call == 0
    ref = mirror.draw_device(p, count, 1.0, 0.4, SEED, 0, k)
    assert ref.branch[j] == (mirror.LANE_GAP if kind == "lane" else mirror.TILE_GAP)
    assert p[idx[j]] > 0, (j, idx[j], w[j])
    assert np.array_equal(idx, ref.indices)
    assert np.isfinite(w).all() and w.max() == 1.0
    _assert_ulps(w, ref.weights)
    h.close()


def test_add_priority_maximum_at_scale():
    import uavtrack as uav
    cap = 1 << 25
    ring = uav.PrioritizedReplayRing(cap, DEV, seed=3, max_batch=64)
    ring.count = cap
    gen = torch.Generator(device=DEV).manual_seed(0)
    base = torch.rand(cap, device=DEV, generator=gen)
    one = {"states": torch.zeros(1, 12, device=DEV), "actions": torch.zeros(1, dtype=torch.int32, device=DEV),
           "rewards": torch.zeros(1, device=DEV), "next_states": torch.zeros(1, 12, device=DEV)}
    stride = 1024 * 256                                     # replay_max_kernel: 1024 workgroups x 256 threads
    cases = [("first", 0, 2.0), ("last", cap - 1, 2.0), ("later pass", 5 * stride + 77, 1.5),
             ("nan", 7 * stride + 3, float("nan")), ("zero", None, 0.0)]
    for name, slot, v in cases:
        ring.priorities.copy_(base if name != "zero" else torch.zeros_like(base))
        if slot is not None:
            ring.priorities[slot] = v
        want = torch.max(ring.priorities).item()
        ring.pos = 12345
        ring.add(one)
        got = ring.priorities[12345].item()
        assert np.float32(got).view(np.int32) == np.float32(want).view(np.int32) or (np.isnan(got) and np.isnan(want)), \
            (name, got, want)
        if name == "nan":
            ring.draw(16)
            with pytest.raises(RuntimeError, match="refused"):
                ring.check()
    ring.check()
    ring.close()
