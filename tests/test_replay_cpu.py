"""The prioritised replay mirror (tests/replay_mirror.py) on the CPU: its selection against np.random.choice's rule
given the same uniforms, the tiled search of the device against the flat one, its u mapping, and the ring add; the
order-exact mirror of the kernels (draw_device) against kernel code transcribed line by line and against the flat rule,
the rounding gaps it builds on purpose, and the rule that no draw lands on a slot >= count or with w = 0."""
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


# ---- the order-exact mirror (draw_device) ---------------------------------------------------------------------------

def _literal_tile_sum(w):
    """replay_tile_kernel for one tile, transcribed line by line in Python floats (IEEE doubles)."""
    s = []
    for tid in range(256):
        v = 0.0
        for q in range(8):
            v += float(w[tid * 8 + q])
        s.append(v)
    wsum = []
    for wave in range(4):
        v = s[wave * 64:(wave + 1) * 64]
        o = 32
        while o:                                           # __shfl_down: lanes past the wave keep their own value
            v = [v[l] + (v[l + o] if l + o < 64 else v[l]) for l in range(64)]
            o >>= 1
        wsum.append(v[0])
    t = 0.0
    for x in wsum:
        t += x
    return t


def _literal_scan(sums):
    """replay_scan_kernel, transcribed line by line."""
    n = len(sums)
    chunk = (n + 1023) // 1024
    s = []
    for tid in range(1024):
        b, e = tid * chunk, min(n, tid * chunk + chunk)
        v = 0.0
        for t in range(b, e):
            v += sums[t]
        s.append(v)
    incl = []
    for wave in range(16):
        v = s[wave * 64:(wave + 1) * 64]
        o = 1
        while o < 64:
            v = [v[l] + v[l - o] if l >= o else v[l] for l in range(64)]
            o <<= 1
        incl.extend(v)
    out = [0.0] * n
    for tid in range(1024):
        wave, lane = tid >> 6, tid & 63
        off = 0.0
        for w in range(wave):
            off += incl[w * 64 + 63]
        run = off + (incl[tid - 1] if lane else 0.0)
        for t in range(tid * chunk, min(n, tid * chunk + chunk)):
            run += sums[t]
            out[t] = run
    return out


def _wide_weights(rng, n, zero_frac=0.3):
    """Non-integer fp32 weights over 2^-40 .. 2^40, some zero."""
    w = (2.0 ** rng.uniform(-40, 40, n)).astype(np.float32)
    w[rng.rand(n) < zero_frac] = 0
    return w


def test_philox_np_equals_the_oracle():
    seed, call = 0x123456789ABCDEF0, (7 << 32) | 3
    assert np.array_equal(mirror.uniforms_np(seed, call, 300), mirror.uniforms(seed, call, 300))
    assert np.array_equal(mirror.uniforms_np(5, 0, 64), mirror.uniforms(5, 0, 64))


@pytest.mark.parametrize("nt", [1, 3, 1024, 1025, 2051])
def test_tile_sums_and_scan_follow_the_kernels_order(nt):
    rng = np.random.RandomState(nt)
    w = np.zeros(nt * mirror.TILE)
    probe = min(nt, 3)                                     # the literal tile kernel is slow: a few tiles suffice
    w[:probe * mirror.TILE] = _wide_weights(rng, probe * mirror.TILE)
    sums, last = mirror.tile_sums(w)
    for t in range(probe):
        assert sums[t] == _literal_tile_sum(w[t * mirror.TILE:(t + 1) * mirror.TILE])
    assert last[0] == np.flatnonzero(w[:mirror.TILE])[-1]
    ts = (2.0 ** rng.uniform(-30, 30, nt)) * (rng.rand(nt) > 0.3)
    assert np.array_equal(mirror.scan(ts), np.array(_literal_scan(list(ts))))
    # the mirror's sums are not np.sum's or np.cumsum's: the association is the kernels'
    if nt >= 1024:
        assert not np.array_equal(mirror.scan(ts), np.cumsum(ts))


@pytest.mark.parametrize("count", [1, 63, 2047, 2048, 2049, 1024 * 2048, 1024 * 2048 + 1, 3000 * 2048 + 17])
def test_draw_device_equals_flat_rule_when_sums_are_exact(count):
    rng = np.random.RandomState(count % 100003)
    w = rng.randint(0, 1000, size=count).astype(np.float32)          # every fp64 partial sum is an exact integer
    w[rng.rand(count) < 0.3] = 0
    w[-1] = 1
    if count > 4 * 2048:
        w[2048:2 * 2048] = 0                                           # a whole zero tile
    w[64:96] = 0                                                       # a whole zero lane
    u = mirror.uniforms_np(0x1_0000_0005, 0, 4000)
    cdf = np.cumsum(w, dtype=np.float64)
    ub = cdf[rng.choice(count, min(count, 500), replace=False)] / cdf[-1]
    u = np.concatenate([u, ub[ub < 1.0], [0.0, 1.0 - 2.0 ** -53]])
    d = mirror.draw_device(w, count, 1.0, 0.4, 0, 0, 0, u=u)
    flat, _ = mirror.select(w, u)
    assert np.array_equal(d.indices, flat)
    assert (d.branch == mirror.HIT).all()
    assert (w[d.indices] > 0).all() and (d.indices < count).all()
    np.testing.assert_allclose(d.weights, mirror.importance(w, flat, cdf[-1], count, 0.4), rtol=1e-6)


def test_draw_device_literal_draw_kernel():
    """The vectorised draw against the draw kernel transcribed for one draw at a time (binary search, lane sums,
    Hillis-Steele lane scan, serial search, fallbacks) on wide-range weights."""
    rng = np.random.RandomState(11)
    count = 5 * 2048 + 77
    w = _wide_weights(rng, count, 0.5)
    w[3 * 2048 + 5 * 32:3 * 2048 + 9 * 32] = 0
    u = np.concatenate([rng.rand(300), [0.0, 1.0 - 2.0 ** -53]])
    d = mirror.draw_device(w, count, 1.0, 0.0, 0, 0, 0, u=u)
    wp = np.zeros(6 * 2048)
    wp[:count] = w
    sums, last = mirror.tile_sums(wp)
    prefix = _literal_scan(list(sums))
    assert list(mirror.scan(sums)) == prefix
    total = prefix[-1]
    assert d.total == total
    for j, uj in enumerate(u):
        x = uj * total
        lo, hi = 0, 6
        while lo < hi:
            mid = (lo + hi) >> 1
            if prefix[mid] > x:
                hi = mid
            else:
                lo = mid + 1
        rem = x - (prefix[lo - 1] if lo > 0 else 0.0)
        lanes = []
        for lane in range(64):
            s = 0.0
            for q in range(32):
                s += float(wp[lo * 2048 + lane * 32 + q])
            lanes.append(s)
        incl = lanes
        o = 1
        while o < 64:
            incl = [incl[l] + incl[l - o] if l >= o else incl[l] for l in range(64)]
            o <<= 1
        hits = [l for l in range(64) if incl[l] > rem]
        if not hits:
            slot = int(np.maximum.accumulate(last)[lo])
        else:
            L = hits[0]
            want = rem - (incl[L - 1] if L else 0.0)
            c, slot, lastnz = 0.0, -1, -1
            for q in range(32):
                i = lo * 2048 + L * 32 + q
                if wp[i] > 0:
                    lastnz = i
                c += float(wp[i])
                if c > want:
                    slot = i
                    break
            if slot < 0:
                slot = lastnz if lastnz >= 0 else int(np.flatnonzero(wp[lo * 2048:lo * 2048 + L * 32])[-1]) + lo * 2048
        assert d.indices[j] == slot, j


# kind, ntiles: a lane-level gap; tile-level gaps with a one-tile-per-thread scan and with the chunked scan (> 1024 tiles)
GAPS = [("lane", 4), ("tile", 600), ("tile", 1100)]


@pytest.mark.parametrize("kind,nt", GAPS, ids=["lane-fallback", "tile-fallback", "tile-fallback-chunked"])
def test_constructed_gap_takes_the_fallback(kind, nt):
    seed = 0x1_2345_6789
    p, count, j = mirror.gap_ring(kind, seed, ntiles=nt)
    assert count == (nt - 1) * mirror.TILE + 1 and p[0] == 0
    fixed = mirror.draw_device(p, count, 1.0, 0.4, seed, 0, 256)
    want = mirror.LANE_GAP if kind == "lane" else mirror.TILE_GAP
    assert fixed.branch[j] == want
    s = fixed.indices[j]
    # the documented rule: the last slot with w > 0 before the zero lane / tile the draw was sent to
    x = fixed.u[j] * fixed.total
    cdf = np.cumsum(p, dtype=np.float64)
    assert 0 < s < count and p[s] > 0
    g = mirror.PER_LANE if kind == "lane" else mirror.TILE
    assert not p[s + 1:(s // g + 1) * g].any()                      # the last slot with w > 0 of its lane / tile
    assert abs(cdf[s] - x) <= 1e-12 * fixed.total                   # the draw sits on the CDF boundary after s
    assert np.isfinite(fixed.weights).all() and fixed.weights.max() == 1.0
    # the parent library's kernels: the draw falls through to slot 0, whose weight is 0, and the weights break
    parent = mirror.draw_device(p, count, 1.0, 0.4, seed, 0, 256, parent=True)
    assert parent.indices[j] == 0 and p[0] == 0
    assert np.isnan(parent.weights[j]) and (np.nan_to_num(parent.weights) == 0).all()
    others = np.arange(256) != j
    assert np.array_equal(parent.indices[others], fixed.indices[others])


def test_draw_device_never_a_bad_slot_under_wide_range_weights():
    rng = np.random.RandomState(17)
    count = 40 * 2048 + 999
    # tile t's scale is 4^t * 2^-40 (so each tile outweighs the prefix before it, and x is fine-grained wherever it
    # lands), the last tile's FLT_MAX / count; within a tile the weights span 2^24
    scale = (2.0 ** (-40 + 2.0 * np.arange(count // 2048 + 1))).repeat(2048)[:count]
    scale[40 * 2048:] = np.float32(3.4e38) / count
    w = (scale * 2.0 ** rng.uniform(-24, 0, count)).astype(np.float32)
    w[rng.rand(count) < 0.2] = 0
    w[7 * 2048:9 * 2048] = 0                                          # whole zero tiles
    for L in rng.choice(count // 32, 200, replace=False):             # whole zero lanes
        w[L * 32:(L + 1) * 32] = 0
    w[11 * 2048:12 * 2048] = np.float32(2.0 ** -149) * rng.randint(0, 8, 2048)    # fp32 subnormals
    w[0] = 0
    # u at random, and u within a few ulps of every tile and lane boundary as the kernels sum them
    wp = np.zeros(-(-count // 2048) * 2048)
    wp[:count] = w
    prefix = mirror.scan(mirror.tile_sums(wp)[0])
    lanes = mirror._hillis_steele(mirror._serial(wp.reshape(-1, 64, 32)))
    b = np.concatenate([prefix, (np.concatenate([[0.0], prefix[:-1]])[:, None] + lanes).reshape(-1)]) / prefix[-1]
    u = [rng.rand(20000), [0.0, 1.0 - 2.0 ** -53]]
    for _ in range(3):
        u += [b]
        b = np.nextafter(b, 0)
    u = np.concatenate(u)
    u = u[(u >= 0) & (u < 1)]
    d = mirror.draw_device(w, count, 1.0, 0.4, 0, 0, 0, u=u)
    assert (d.indices >= 0).all() and (d.indices < count).all() and (w[d.indices] > 0).all()
    seen = np.bincount(d.branch, minlength=6)
    assert seen[mirror.LANE_FALLBACK] > 0 and seen[mirror.TILE_FALLBACK] > 0 and seen[mirror.OVER] == 0, seen
    assert np.isfinite(d.weights).all() and d.weights.max() == 1.0
    # and on the constructed gaps
    for kind, nt in GAPS:
        p, n, j = mirror.gap_ring(kind, 77 << 32, ntiles=nt)
        for parent in (False, True):
            g = mirror.draw_device(p, n, 1.0, 0.4, 77 << 32, 0, 256, parent=parent)
            if parent:
                assert g.indices[j] == 0 and p[0] == 0                     # the defect, modelled
            else:
                assert (g.indices < n).all() and (p[g.indices] > 0).all()
