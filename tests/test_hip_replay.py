"""The prioritised replay ring (uavtrack_replay_*, uavtrack.PrioritizedReplayRing) on the MI355X: draws against the
fp64 mirror (tests/replay_mirror.py), the distribution beyond torch.multinomial's 2^24 categories, refused priorities,
the fused add against transitions_from_rollout + PrioritizedDeviceReplayBuffer.add, the learner integration, graph
capture and the ABI's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _uav():
    import uavtrack
    return uavtrack


def _ring(capacity, prio=None, seed=11, alpha=0.6, max_batch=65536):
    """A ring whose priorities are set directly (draws need no stores); count = capacity."""
    r = _uav().PrioritizedReplayRing(capacity, DEV, alpha=alpha, seed=seed, max_batch=max_batch)
    if prio is not None:
        r.priorities.copy_(torch.as_tensor(np.asarray(prio, np.float32)))
        r.count = capacity
    return r


def test_draw_equals_mirror_exact_integer_priorities():
    rng = np.random.RandomState(0)
    n, k, seed = 3 * 2048 + 517, 4000, 1234
    p = rng.randint(0, 50, size=n).astype(np.float32)          # zeros included; every fp64 prefix sum is exact
    ring = _ring(n, p, seed=seed, alpha=1.0)
    for call in range(3):                                       # the device counter advances between calls
        idx, w = ring.draw(k, beta=0.4)
        ref_idx, ref_w, _, _ = mirror.draw(p, n, 1.0, 0.4, seed, call, k)
        assert np.array_equal(idx.cpu().numpy(), ref_idx), call
        np.testing.assert_allclose(w.cpu().numpy(), ref_w, rtol=1e-6)
        assert (p[idx.cpu().numpy()] > 0).all()
    ring.check()


def test_draw_equals_mirror_fractional_alpha():
    rng = np.random.RandomState(1)
    n, k, seed = 5000, 4000, 99
    p = rng.exponential(1.0, size=n).astype(np.float32)
    ring = _ring(n, p, seed=seed, alpha=0.6)
    for call in range(2):
        idx, w = ring.draw(k, beta=0.7)
        ref_idx, ref_w, u, cdf = mirror.draw(p, n, 0.6, 0.7, seed, call, k)
        away = ~mirror.near_boundary(u, cdf, ref_idx, mirror.weights_fp32(p, 0.6))
        assert away.mean() > 0.98
        got = idx.cpu().numpy()
        assert np.array_equal(got[away], ref_idx[away])
        # weights take the batch maximum over every draw: compare where the draws agree everywhere
        if np.array_equal(got, ref_idx):
            np.testing.assert_allclose(w.cpu().numpy(), ref_w, rtol=1e-5)
    ring.check()


def test_distribution_beyond_2_24_slots():
    count = 1 << 25
    half = count // 2
    p = torch.ones(count, device=DEV)
    p[half:] = 0.25
    ring = _uav().PrioritizedReplayRing(count, DEV, alpha=0.6, seed=5, max_batch=1 << 22)
    ring.priorities.copy_(p)
    ring.count = count
    N = 1 << 22
    idx, w = ring.draw(N)
    ring.check()
    idx = idx.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < count
    q = 0.25 ** 0.6
    share = q / (1 + q)                                         # 0.30327
    tail = (idx >= half).mean()
    se = np.sqrt(share * (1 - share) / N)
    assert abs(tail - share) < 6 * se, (tail, share, se)
    buckets = np.bincount(idx // (count // 64), minlength=64)
    expect = np.where(np.arange(64) < 32, (1 - share) / 32, share / 32) * N
    chi2 = ((buckets - expect) ** 2 / expect).sum()
    assert chi2 < 130, chi2                                     # 63 degrees of freedom; p < 1e-6 beyond 130
    # one hot slot at count - 1, drawn at its probability
    base = half * 1.0 + half * q
    hot_w = np.float32(base / 9.0)                              # P(hot) ~ 0.1
    ring.priorities[count - 1] = float(np.float32(hot_w) ** np.float32(1 / 0.6))
    w_hot = float(np.float32(ring.priorities[count - 1].item()) ** np.float32(0.6))
    P_hot = w_hot / (base - q + w_hot)
    idx, _ = ring.draw(N)
    ring.check()
    f = (idx == count - 1).float().mean().item()
    assert abs(f - P_hot) < 6 * np.sqrt(P_hot * (1 - P_hot) / N), (f, P_hot)
    ring.close()


def test_never_a_bad_slot():
    rng = np.random.RandomState(3)
    count = 3_000_017
    p = np.zeros(count, np.float32)
    nz = rng.choice(count, 2000, replace=False)
    p[nz] = (2.0 ** rng.uniform(-40, 40, nz.size)).astype(np.float32)
    ring = _ring(count, p, max_batch=1 << 20)
    idx, w = ring.draw(1 << 20)
    ring.check()
    got = idx.cpu().numpy()
    assert got.min() >= 0 and got.max() < count and (p[got] > 0).all()
    assert torch.isfinite(w).all() and w.max().item() == 1.0
    # all zero, a NaN, a negative: refused on the device, every index in range, check() raises
    for bad in ("zero", "nan", "neg"):
        q = np.zeros(count, np.float32) if bad == "zero" else p.copy()
        if bad == "nan":
            q[count // 2] = np.nan
        if bad == "neg":
            q[7] = -1.0
        ring.priorities.copy_(torch.from_numpy(q))
        idx, w = ring.draw(4096)
        got = idx.cpu().numpy()
        assert (got >= 0).all() and (got < count).all()
        assert torch.isnan(w).all()
        with pytest.raises(RuntimeError, match="refused"):
            ring.check()
    ring.check()                                                # the count restarted
    ring.close()


def _rollout(rng, T, B, N):
    obs_in = torch.from_numpy(rng.randn(B, N, 12).astype(np.float32)).to(DEV)
    out = {"obs": torch.from_numpy(rng.randn(T, B, N, 12).astype(np.float32)).to(DEV),
           "actions": torch.from_numpy(rng.randint(0, 12, (T, B, N)).astype(np.int32)).to(DEV),
           "reward": torch.from_numpy(rng.randn(T, B, N).astype(np.float32)).to(DEV)}
    return obs_in, out


def _assert_same_ring(ring, ref):
    assert (ring.pos, ring.count) == (ref.pos, ref.count)
    c = ref.count
    for key in ("states", "actions", "rewards", "next_states"):
        assert torch.equal(ring.store[key][:c], ref.store[key][:c]), key
    assert torch.equal(ring.priorities, ref.priorities)


def test_add_rollout_equals_reference_ring():
    uav = _uav()
    rng = np.random.RandomState(4)
    cap = 1000
    ring = uav.PrioritizedReplayRing(cap, DEV, seed=1)
    ref = uav.PrioritizedDeviceReplayBuffer(cap, DEV)
    for (T, B, N) in ((3, 4, 20), (12, 4, 20), (7, 9, 20)):     # first add, a wrap-around, n > capacity
        obs_in, out = _rollout(rng, T, B, N)
        ring.add_rollout(obs_in, out)
        ref.add(uav.transitions_from_rollout(obs_in, out))
        _assert_same_ring(ring, ref)
    # raise the maximum, add; lower it, add (flat add this time)
    for val in (7.5, 0.125):
        slots = torch.tensor([3, 500, 999], device=DEV)
        ring.update_priorities(slots, torch.full((3,), val))
        ref.update_priorities(slots, torch.full((3,), val))
        if val < 1:                                             # every slot below the old maximum
            ring.priorities.fill_(val)
            ref.priorities.fill_(val)
        obs_in, out = _rollout(rng, 2, 5, 20)
        trans = uav.transitions_from_rollout(obs_in, out)
        ring.add(trans)
        ref.add(trans)
        _assert_same_ring(ring, ref)


def test_update_priorities_last_write_wins():
    import learner_mirror
    ring = _ring(64, np.ones(64, np.float32))
    idx = torch.tensor([5, 9, 5, 5, 9, 1], device=DEV)
    val = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], device=DEV)
    ring.update_priorities(idx, val)
    ref = learner_mirror.last_wins(np.ones(64, np.float32), idx.cpu().numpy(), val.cpu().numpy())
    assert np.array_equal(ring.priorities.cpu().numpy(), ref)


def _twin_learners(seed=0):
    uav = _uav()
    torch.manual_seed(seed)
    a = uav.DeviceActorCritic(12, 64, 12, 1e-3, 5e-3, 0.95, DEV, max_batch=4096)
    torch.manual_seed(seed)
    b = uav.DeviceActorCritic(12, 64, 12, 1e-3, 5e-3, 0.95, DEV, max_batch=4096)
    return a, b


def _twin_rings(rng, cap=5000, seed=21):
    uav = _uav()
    ra, rb = uav.PrioritizedReplayRing(cap, DEV, seed=seed), uav.PrioritizedReplayRing(cap, DEV, seed=seed)
    obs_in, out = _rollout(rng, 10, 20, 20)
    ra.add_rollout(obs_in, out)
    rb.add_rollout(obs_in, out)
    p = torch.from_numpy(rng.exponential(1.0, cap).astype(np.float32)).to(DEV)
    ra.priorities[:ra.count] = p[:ra.count]
    rb.priorities[:rb.count] = p[:rb.count]
    return ra, rb


def test_update_from_ring_equals_draw_then_update():
    rng = np.random.RandomState(5)
    la, lb = _twin_learners()
    ra, rb = _twin_rings(rng)
    k = 2000
    for _ in range(3):
        a_loss, c_loss, td = la.update_from(ra, k)
        idx, _ = rb.draw(k)
        b_a, b_c, b_td = lb._run(k, rb.store, rb.capacity, idx, rb.priorities)
        assert torch.equal(a_loss, b_a) and torch.equal(c_loss, b_c) and torch.equal(td, b_td)
        assert torch.equal(ra._idx[:k], idx)
        assert torch.equal(ra.priorities, rb.priorities)
    la.check(); lb.check(); ra.check(); rb.check()


def test_capture_draw_and_update():
    rng = np.random.RandomState(6)
    la, lb = _twin_learners(1)
    ra, rb = _twin_rings(rng, seed=77)
    k = 2048
    # warm-up, eager, on both twins (counter 0 of both rings)
    la.update_from(ra, k)
    idx, _ = rb.draw(k)
    lb._run(k, rb.store, rb.capacity, idx, rb.priorities)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ga, gc, gtd = la.update_from(ra, k)
    seen = []
    for _ in range(2):
        g.replay()
        idx, _ = rb.draw(k)
        b_a, b_c, b_td = lb._run(k, rb.store, rb.capacity, idx, rb.priorities)
        torch.cuda.synchronize()
        assert torch.equal(ra._idx[:k], idx)
        assert torch.equal(ga, b_a) and torch.equal(gc, b_c) and torch.equal(gtd, b_td)
        assert torch.equal(ra.priorities, rb.priorities)
        seen.append(idx.clone())
    assert not torch.equal(seen[0], seen[1])
    la.check(); ra.check()


def test_same_seed_same_indices_and_abi_refusals():
    uav, lib = _uav(), _uav()._lib.load()
    rng = np.random.RandomState(8)
    p = rng.exponential(1.0, 3000).astype(np.float32)
    a, b, c = _ring(3000, p, seed=42, max_batch=512), _ring(3000, p, seed=42, max_batch=512), _ring(3000, p, seed=43)
    ia, _ = a.draw(500)
    ib, _ = b.draw(500)
    ic, _ = c.draw(500)
    assert torch.equal(ia, ib) and not torch.equal(ia, ic)
    # refusals: a message, and nothing enqueued (the next good call is call 1 of ring a, as of its twin b)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(1024, dtype=torch.int64, device=DEV)
    ring = a._ring()
    assert lib.uavtrack_replay_sample(a._h, C.byref(ring), 513, 0.6, 0.4, uav._lib.ptr(out), None, st) != 0
    assert b"max_batch" in lib.uavtrack_last_error()
    assert lib.uavtrack_replay_sample(a._h, C.byref(ring), 10, 0.6, 0.4, None, None, st) != 0
    assert b"indices" in lib.uavtrack_last_error()
    assert lib.uavtrack_replay_sample(a._h, None, 10, 0.6, 0.4, uav._lib.ptr(out), None, st) != 0
    big = a._ring()
    big.capacity, big.count = 3001, 3001
    assert lib.uavtrack_replay_sample(a._h, C.byref(big), 10, 0.6, 0.4, uav._lib.ptr(out), None, st) != 0
    assert b"max_capacity" in lib.uavtrack_last_error()
    over = a._ring()
    over.count = 3001
    assert lib.uavtrack_replay_sample(a._h, C.byref(over), 10, 0.6, 0.4, uav._lib.ptr(out), None, st) != 0
    assert b"count" in lib.uavtrack_last_error()
    assert lib.uavtrack_replay_sample(a._h, C.byref(ring), 10, 0.0, 0.4, uav._lib.ptr(out), None, st) != 0
    assert b"alpha" in lib.uavtrack_last_error()
    nul = a._ring()
    nul.states = None
    assert lib.uavtrack_replay_add(a._h, C.byref(nul), 1, uav._lib.ptr(a.store["states"]), uav._lib.ptr(a.store["actions"]),
                                   uav._lib.ptr(a.store["rewards"]), uav._lib.ptr(a.store["next_states"]), st) != 0
    assert b"null" in lib.uavtrack_last_error()
    assert lib.uavtrack_replay_add_rollout(a._h, C.byref(ring), 1, 1, None, None, None, None, st) != 0
    assert b"null" in lib.uavtrack_last_error()
    assert torch.equal(a.draw(500)[0], b.draw(500)[0])
    a.check()
    with pytest.raises(ValueError):
        uav.PrioritizedReplayRing(16, DEV, alpha=0.0)
    e = _ring(16)
    assert e.draw(4) == (None, None)
    d, i, w = e.sample(4)
    assert i is None and w is None and d["states"].shape == (0, 12)
