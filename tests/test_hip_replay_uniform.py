"""The uniform replay ring (uavtrack_replay_sample_uniform, uavtrack.ReplayRing) on the MI355X: draws bitwise against
the integer mirror (tests/replay_uniform_mirror.py), the call counter it shares with the prioritised draws, graph
capture, the adds of a ring without priorities against a prioritised ring's, the learner on uniform rings, and the
refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_mirror as pmirror
import replay_uniform_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCH = 128


def _uav():
    import uavtrack
    return uavtrack


def _transitions(rng, n):
    return {"states": torch.from_numpy(rng.randn(n, 12).astype(np.float32)).to(DEV),
            "actions": torch.from_numpy(rng.randint(0, 12, n).astype(np.int32)).to(DEV),
            "rewards": torch.from_numpy(rng.randn(n).astype(np.float32)).to(DEV),
            "next_states": torch.from_numpy(rng.randn(n, 12).astype(np.float32)).to(DEV)}


def _rollout(rng, T, B, N, episodes=False):
    obs_in = torch.from_numpy(rng.randn(B, N, 12).astype(np.float32)).to(DEV)
    out = {"obs": torch.from_numpy(rng.randn(T, B, N, 12).astype(np.float32)).to(DEV),
           "actions": torch.from_numpy(rng.randint(0, 12, (T, B, N)).astype(np.int32)).to(DEV),
           "reward": torch.from_numpy(rng.randn(T, B, N).astype(np.float32)).to(DEV)}
    if episodes:
        out["done"] = torch.from_numpy((rng.rand(T, B) < 0.5).astype(np.uint8)).to(DEV)
        out["start_obs"] = torch.from_numpy(rng.randn(T, B, N, 12).astype(np.float32)).to(DEV)
    return obs_in, out


def _filled(capacity, adds, seed, max_batch=None):
    """A ReplayRing after flat adds of the given sizes."""
    ring = _uav().ReplayRing(capacity, DEV, seed=seed, max_batch=max_batch or capacity)
    rng = np.random.RandomState(capacity)
    for n in adds:
        ring.add(_transitions(rng, n))
    return ring


# ---- device against mirror ------------------------------------------------------------------------------------------------

# capacity, the adds, count after them: both bit-width parities, the tile boundary and its neighbour, a ring not yet
# full, a ring that has wrapped
RINGS = [(5, [5], 5), (64, [64], 64), (65, [65], 65), (2049, [2049], 2049), (4097, [3000], 3000),
         (4097, [3000, 3000], 4097)]


@pytest.mark.parametrize("capacity,adds,count", RINGS, ids=[f"cap{c}-count{n}-{len(a)}adds" for c, a, n in RINGS])
def test_draw_equals_mirror(capacity, adds, count):
    seed = 1000 + capacity
    ring = _filled(capacity, adds, seed)
    assert ring.size() == count and ring.priorities is None
    for call, k in enumerate((1, count, min(BATCH, count))):
        idx = ring.draw(k)
        assert idx.dtype == torch.int64 and idx.shape == (k,)
        got = idx.cpu().numpy()
        assert np.array_equal(got, mirror.draw(count, k, seed, call)), (call, k)
        assert len(np.unique(got)) == k and got.min() >= 0 and got.max() < count
    batch = ring.sample(BATCH)                                      # call 3: ReplayBuffer.sample's dict
    ref = torch.from_numpy(mirror.draw(count, min(BATCH, count), seed, 3)).to(DEV)
    assert set(batch) == {"states", "actions", "rewards", "next_states"}
    for key in batch:
        assert torch.equal(batch[key], ring.store[key][ref]), key
    ring.check()


def test_empty_ring():
    ring = _uav().ReplayRing(8, DEV)
    assert ring.draw(4) is None and ring.size() == 0
    assert {k: tuple(v.shape) for k, v in ring.sample(4).items()} == {"states": (0, 12), "actions": (0,), "rewards": (0,),
                                                                      "next_states": (0, 12)}


# ---- counter and seed -----------------------------------------------------------------------------------------------------

def test_counter_and_seed():
    a, b, c = _filled(3000, [3000], 42), _filled(3000, [3000], 42), _filled(3000, [3000], 43)
    a0, a1, b0, c0 = a.draw(500), a.draw(500), b.draw(500), c.draw(500)
    assert not torch.equal(a0, a1)                                  # call c + 1 differs from call c
    assert torch.equal(a0, b0) and not torch.equal(a0, c0)          # the same seed agrees, another differs
    assert torch.equal(a1, b.draw(500))


def test_uniform_and_prioritised_draws_share_one_counter():
    rng = np.random.RandomState(2)
    n, k, seed = 2 * 2048 + 77, 300, 99
    p = rng.randint(0, 50, size=n).astype(np.float32)               # exact fp64 prefix sums: the mirror is bitwise
    ring = _uav().PrioritizedReplayRing(n, DEV, alpha=1.0, seed=seed, max_batch=k)
    ring.priorities.copy_(torch.from_numpy(p))
    ring.count = n
    uni = torch.empty(k, dtype=torch.int64, device=DEV)
    for call in range(6):
        if call % 2 == 0:
            ring._draw_uniform(k, uni)
            assert np.array_equal(uni.cpu().numpy(), mirror.draw(n, k, seed, call)), call
        else:
            idx, w = ring.draw(k, beta=0.4)
            ref_idx, ref_w, _, _ = pmirror.draw(p, n, 1.0, 0.4, seed, call, k)
            assert np.array_equal(idx.cpu().numpy(), ref_idx), call
            np.testing.assert_allclose(w.cpu().numpy(), ref_w, rtol=1e-6)
    ring.check()


# ---- the learner ----------------------------------------------------------------------------------------------------------

H, CAP, K = 128, 512, 128


def _twin_learners(seed=0):
    uav = _uav()
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        out.append(uav.DeviceActorCritic(12, H, 12, 1e-3, 5e-3, 0.95, DEV, max_batch=K))
    return out


def _learner_ring(rng, seed, T=4):
    ring = _uav().ReplayRing(CAP, DEV, seed=seed, max_batch=K)
    ring.add_rollout(*_rollout(rng, T, 8, 10))                      # T = 4: 320 of 512 slots; T = 8: full, wrapped
    return ring


def _gathered(ring, call, k=K):
    idx = torch.from_numpy(mirror.draw(ring.count, k, ring.seed, call)).to(DEV)
    return {key: ring.store[key][idx] for key in ring.store}, idx


def _assert_same_learner(la, lb):
    assert np.array_equal(la._get_params(), lb._get_params())


def test_update_from_equals_update_on_the_mirrors_rows():
    rng = np.random.RandomState(5)
    la, lb = _twin_learners()
    ring = _learner_ring(rng, seed=21)
    for call in range(3):
        if call == 2:
            ring.add_rollout(*_rollout(rng, 8, 8, 10))              # n > capacity: the ring is full now
        a_loss, c_loss, td = la.update_from(ring, K, importance=(call == 1))   # importance changes nothing here
        batch, idx = _gathered(ring, call)
        b_a, b_c, b_td = lb.update(batch)
        assert torch.equal(ring._idx[:K], idx)
        assert torch.equal(a_loss, b_a) and torch.equal(c_loss, b_c) and torch.equal(td, b_td)
        _assert_same_learner(la, lb)
    la.check(); lb.check(); ring.check()


def test_update_from_many_equals_the_grad_apply_chain():
    la, lb = _twin_learners(1)
    rings_a = [_learner_ring(np.random.RandomState(7 + r), seed=30 + r, T=4 + 4 * r) for r in range(2)]
    rings_b = [_learner_ring(np.random.RandomState(7 + r), seed=30 + r, T=4 + 4 * r) for r in range(2)]
    for call in range(2):
        al, cl, tds = la.update_from_many(rings_a, K)
        rows = lb.new_rows(2)
        ref_td = []
        for r, ring in enumerate(rings_b):
            _, td, idx = lb.grad_from(ring, K, rows[r])
            assert np.array_equal(idx.cpu().numpy(), mirror.draw(ring.count, K, ring.seed, call))
            ref_td.append(td)
        b_al, b_cl = lb.apply(rows)
        assert torch.equal(al, b_al) and torch.equal(cl, b_cl)
        assert all(torch.equal(x, y) for x, y in zip(tds, ref_td))
        _assert_same_learner(la, lb)
    la.check(); lb.check()


def test_capture_draw_and_update():
    rng = np.random.RandomState(6)
    la, lb = _twin_learners(2)
    ring = _learner_ring(rng, seed=77, T=8)
    la.update_from(ring, K)                                         # warm-up, eager: call 0
    lb.update(_gathered(ring, 0)[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ga, gc, gtd = la.update_from(ring, K)
    seen = []
    for call in (1, 2):                                             # the capture itself ran nothing
        g.replay()
        torch.cuda.synchronize()
        batch, idx = _gathered(ring, call)
        assert torch.equal(ring._idx[:K], idx), call
        b_a, b_c, b_td = lb.update(batch)
        assert torch.equal(ga, b_a) and torch.equal(gc, b_c) and torch.equal(gtd, b_td)
        _assert_same_learner(la, lb)
        seen.append(idx)
    assert not torch.equal(seen[0], seen[1])
    la.check(); ring.check()


# ---- adds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity", [17, 64])
def test_adds_write_the_stores_of_a_prioritised_ring(capacity):
    uav = _uav()
    rng = np.random.RandomState(capacity)
    uni, pri = uav.ReplayRing(capacity, DEV), uav.PrioritizedReplayRing(capacity, DEV)
    for ring in (uni, pri):
        for t in ring.store.values():
            t.zero_()

    def same():
        assert (uni.pos, uni.count) == (pri.pos, pri.count)
        for key in uni.store:
            assert torch.equal(uni.store[key], pri.store[key]), key

    T, B, N = 3, 2, 5                                               # 30 transitions: n > 17; 64 wraps at the third add
    for step in range(4):
        obs_in, out = _rollout(rng, T, B, N, episodes=(step % 2 == 1))
        for ring in (uni, pri):
            ring.add_rollout(obs_in, out)
        same()
        trans = uav.transitions_from_rollout(obs_in, out)
        part = {k: v[:10] for k, v in trans.items()} if step % 2 == 0 else trans    # 10 rows: a wrap within capacity 17
        for ring in (uni, pri):
            ring.add(part)
        same()
    assert uni.count == capacity and uni.priorities is None
    # and the content is the reference's: the last `capacity` transitions in ring order
    ref = uav.DeviceReplayBuffer(capacity, DEV)
    rng = np.random.RandomState(capacity)
    for step in range(4):
        obs_in, out = _rollout(rng, T, B, N, episodes=(step % 2 == 1))
        trans = uav.transitions_from_rollout(obs_in, out)
        ref.add(trans)
        ref.add({k: v[:10] for k, v in trans.items()} if step % 2 == 0 else trans)
    for key in uni.store:
        assert torch.equal(uni.store[key], ref.store[key]), key


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_refusals_enqueue_nothing():
    uav, lib = _uav(), _uav()._lib.load()
    ptr = uav._lib.ptr
    seed = 9
    a = _filled(300, [200], seed, max_batch=64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(512, dtype=torch.int64, device=DEV)
    ring = a._ring()
    fn = lib.uavtrack_replay_sample_uniform
    assert fn(a._h, C.byref(ring), 65, ptr(out), st) != 0
    assert b"n = 65 outside [1, max_batch = 64]" in lib.uavtrack_last_error()
    assert fn(a._h, C.byref(ring), 0, ptr(out), st) != 0
    assert b"n = 0 outside" in lib.uavtrack_last_error()
    few = a._ring()
    few.count = 10
    assert fn(a._h, C.byref(few), 11, ptr(out), st) != 0
    assert b"n = 11 exceeds count = 10" in lib.uavtrack_last_error()
    none = a._ring()
    none.count = 0
    assert fn(a._h, C.byref(none), 1, ptr(out), st) != 0
    assert b"empty" in lib.uavtrack_last_error()
    assert fn(a._h, C.byref(ring), 10, None, st) != 0
    assert b"indices must not be null" in lib.uavtrack_last_error()
    assert fn(a._h, None, 10, ptr(out), st) != 0
    assert b"ring is null" in lib.uavtrack_last_error()
    big = a._ring()
    big.capacity = 301
    assert fn(a._h, C.byref(big), 10, ptr(out), st) != 0
    assert b"max_capacity" in lib.uavtrack_last_error()
    over = a._ring()
    over.count = 301
    assert fn(a._h, C.byref(over), 10, ptr(out), st) != 0
    assert b"count" in lib.uavtrack_last_error()
    # the prioritised draws keep refusing a ring without priorities
    assert ring.priorities is None
    w = torch.empty(64, device=DEV)
    assert lib.uavtrack_replay_sample(a._h, C.byref(ring), 10, 0.6, 0.4, ptr(out), ptr(w), st) != 0
    assert b"uavtrack_replay_sample: ring->priorities is null" in lib.uavtrack_last_error()
    assert lib.uavtrack_replay_sample_annealed(a._h, C.byref(ring), 10, 0.6, 0.4, 1.0, 5, ptr(out), ptr(w), st) != 0
    assert b"uavtrack_replay_sample_annealed: ring->priorities is null" in lib.uavtrack_last_error()
    with pytest.raises(RuntimeError, match="uavtrack_replay_sample_uniform failed.*max_batch"):
        a._draw_uniform(201, out)
    # nothing was enqueued: the counter still stands at 0
    assert np.array_equal(a.draw(64).cpu().numpy(), mirror.draw(200, 64, seed, 0))
    a.check()
