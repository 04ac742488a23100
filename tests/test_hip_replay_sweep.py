"""The sweep over a ring window (uavtrack_replay_sample_sweep, uavtrack.RingSweep) on the MI355X: indices bitwise against
the integer mirror (tests/replay_sweep_mirror.py), an epoch's coverage of its window, the caller-owned cursor and the
handle counter it leaves alone, the "last" window of the adds, the learner on sweeps, graph capture, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_mirror as pmirror
import replay_sweep_mirror as mirror
import replay_uniform_mirror as umirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _uav():
    import uavtrack
    return uavtrack


def _transitions(rng, n):
    return {"states": torch.from_numpy(rng.randn(n, 12).astype(np.float32)).to(DEV),
            "actions": torch.from_numpy(rng.randint(0, 12, n).astype(np.int32)).to(DEV),
            "rewards": torch.from_numpy(rng.randn(n).astype(np.float32)).to(DEV),
            "next_states": torch.from_numpy(rng.randn(n, 12).astype(np.float32)).to(DEV)}


def _rollout(rng, T, B, N):
    obs_in = torch.from_numpy(rng.randn(B, N, 12).astype(np.float32)).to(DEV)
    out = {"obs": torch.from_numpy(rng.randn(T, B, N, 12).astype(np.float32)).to(DEV),
           "actions": torch.from_numpy(rng.randint(0, 12, (T, B, N)).astype(np.int32)).to(DEV),
           "reward": torch.from_numpy(rng.randn(T, B, N).astype(np.float32)).to(DEV)}
    return obs_in, out


def _filled(capacity, count, seed, max_batch=None, kind="ReplayRing"):
    """A ring holding `count` transitions behind one flat add."""
    ring = getattr(_uav(), kind)(capacity, DEV, seed=seed, max_batch=max_batch or capacity)
    ring.add(_transitions(np.random.RandomState(capacity), count))
    assert ring.size() == count
    return ring


# ---- device against mirror, coverage ---------------------------------------------------------------------------------------

# capacity, count, first, W, n: the smallest window with n = W, both bit-width parities, n not dividing W from a first
# slot that is not 0 (the window of a full ring wraps), a ring that is not full, a window across the capacity, W = 1
CASES = [(5, 5, 0, 5, 5), (64, 64, 0, 64, 16), (65, 65, 3, 65, 16), (4097, 3000, 100, 2049, 128),
         (4097, 4097, 4000, 257, 64), (5, 5, 4, 1, 1)]


@pytest.mark.parametrize("capacity,count,first,W,n", CASES, ids=[f"cap{c}-count{k}-first{f}-W{w}-n{n}" for c, k, f, w, n in CASES])
def test_sweep_equals_mirror_and_covers_its_window(capacity, count, first, W, n):
    seed = 2000 + capacity
    ring = _filled(capacity, count, seed)
    sweep = ring.sweep(n, (first, W))
    M = W // n
    assert sweep.window == (first, W) and sweep.minibatches == M and sweep.count == W
    calls = 2 * M + 1                                               # an epoch boundary is crossed twice
    drawn = [sweep.draw() for _ in range(calls)]
    assert all(d.dtype == torch.int64 and d.shape == (n,) for d in drawn)
    got = torch.stack(drawn).cpu().numpy()
    assert np.array_equal(got, mirror.sweep_calls(capacity, first, W, n, seed, np.arange(calls)))
    assert sweep.position() == calls
    window = (first + np.arange(W)) % capacity
    for e in range(2):
        epoch = got[e * M:(e + 1) * M].reshape(-1)
        if W % n == 0:
            assert np.array_equal(np.sort(epoch), np.sort(window)), e
        else:
            assert len(np.unique(epoch)) == M * n and np.isin(epoch, window).all(), e
    if W >= 64:
        assert not np.array_equal(got[:M], got[M:2 * M])            # another epoch, another order
    batch = sweep.sample()                                          # call 2 M + 1: ring.sample()'s dict at the sweep's slots
    ref = torch.from_numpy(mirror.sweep_call(capacity, first, W, n, seed, calls)).to(DEV)
    assert set(batch) == {"states", "actions", "rewards", "next_states"}
    for key in batch:
        assert torch.equal(batch[key], ring.store[key][ref]), key
    ring.check()


def test_named_windows_and_a_prioritised_ring():
    ring = _filled(300, 200, 5, kind="PrioritizedReplayRing")
    for window, (first, W) in (("all", (0, 200)), ("last", (0, 200)), ((50, 150), (50, 150))):
        sweep = ring.sweep(50, window)
        assert sweep.window == (first, W) and sweep.priorities is ring.priorities
        got = torch.stack([sweep.draw() for _ in range(W // 50)]).cpu().numpy()
        assert np.array_equal(got, mirror.sweep_calls(300, first, W, 50, 5, np.arange(W // 50)))
        assert np.array_equal(np.sort(got.reshape(-1)), first + np.arange(W))


# ---- the cursor ------------------------------------------------------------------------------------------------------------

def test_seek_reproduces_a_call():
    cap, first, W, n, seed = 4097, 4000, 257, 64, 31
    sweep = _filled(cap, cap, seed).sweep(n, (first, W))
    M = W // n
    for q in (7, 0, M, ((1 << 32) + 3) * M + 1):                    # an epoch number beyond 2^32 among them
        sweep.seek(q)
        a, b = sweep.draw(), sweep.draw()
        assert np.array_equal(a.cpu().numpy(), mirror.sweep_call(cap, first, W, n, seed, q)), q
        assert np.array_equal(b.cpu().numpy(), mirror.sweep_call(cap, first, W, n, seed, q + 1)), q
        assert sweep.position() == q + 2


def test_two_sweeps_agree_and_another_seed_differs():
    a, c = _filled(3000, 3000, 42), _filled(3000, 3000, 43)
    s1, s2, s3 = a.sweep(500, "all"), a.sweep(500, "all"), c.sweep(500, "all")
    for q in range(8):                                              # 6 minibatches an epoch
        x, y, z = s1.draw(), s2.draw(), s3.draw()
        assert torch.equal(x, y) and not torch.equal(x, z), q
    assert s1.position() == s2.position() == 8


def test_sweep_calls_leave_the_handle_counter_alone():
    count, k, seed = 3000, 500, 77
    ring = _filled(count, count, seed)
    sweep = ring.sweep(500)
    for call in range(3):
        sweep.draw(); sweep.draw()
        assert np.array_equal(ring.draw(k).cpu().numpy(), umirror.draw(count, k, seed, call)), call
    # a prioritised ring: uniform and prioritised draws between sweep calls are what they are without any sweep
    rng = np.random.RandomState(2)
    n = 2 * 2048 + 77
    p = rng.randint(0, 50, size=n).astype(np.float32)               # exact fp64 prefix sums: the mirror is bitwise
    ring = _uav().PrioritizedReplayRing(n, DEV, alpha=1.0, seed=seed, max_batch=300)
    ring.priorities.copy_(torch.from_numpy(p))
    ring.count = n
    sweep = ring.sweep(300, (n - 100, 1000))
    uni = torch.empty(300, dtype=torch.int64, device=DEV)
    for call in range(4):
        s = sweep.draw()
        assert np.array_equal(s.cpu().numpy(), mirror.sweep_call(n, n - 100, 1000, 300, seed, call))
        if call % 2 == 0:
            ring._draw_uniform(300, uni)
            assert np.array_equal(uni.cpu().numpy(), umirror.draw(n, 300, seed, call)), call
        else:
            idx, w = ring.draw(300, beta=0.4)
            ref_idx, ref_w, _, _ = pmirror.draw(p, n, 1.0, 0.4, seed, call, 300)
            assert np.array_equal(idx.cpu().numpy(), ref_idx), call
            np.testing.assert_allclose(w.cpu().numpy(), ref_w, rtol=1e-6)
    ring.check()


def test_the_last_window_is_what_the_add_wrote():
    SENTINEL = 12345.0
    ring = _uav().ReplayRing(512, DEV, seed=1, max_batch=64).with_behaviour()
    rng = np.random.RandomState(3)
    learner = _uav().DeviceActorCritic(12, 64, 12, 1e-3, 5e-3, 0.95, DEV, max_batch=64)
    # 320 into an empty ring; 160 behind them; 640 > capacity from pos 480; a flat add of 100; a behaviour add across the end
    for T, flat, want in ((4, 0, (0, 320)), (2, 0, (320, 160)), (8, 0, (96, 512)), (0, 100, (96, 100)), (5, 0, (196, 400))):
        ring.store["rewards"].fill_(SENTINEL)
        if flat:
            ring.add(_transitions(rng, flat))
        else:
            ring.add_rollout_behaviour(*_rollout(rng, T, 8, 10), behaviour=learner)
        sweep = ring.sweep(64)                                      # window="last"
        assert sweep.window == want
        written = np.flatnonzero(ring.store["rewards"].cpu().numpy() != SENTINEL)
        first, W = want
        assert np.array_equal(written, np.sort((first + np.arange(W)) % 512))
        epoch = torch.stack([sweep.draw() for _ in range(sweep.minibatches)]).cpu().numpy().reshape(-1)
        assert len(np.unique(epoch)) == (W // 64) * 64 and np.isin(epoch, written).all()
    # pinned at creation: a later add does not move it, rebind does, and rewinds the cursor
    ring.add(_transitions(rng, 70))
    assert sweep.window == (196, 400) and sweep.position() == 6
    assert sweep.rebind().window == (84, 70) and sweep.position() == 0 and sweep.minibatches == 1
    assert np.array_equal(sweep.draw().cpu().numpy(), mirror.sweep_call(512, 84, 70, 64, 1, 0))
    batch = sweep.sample()                                          # a behaviour ring's dict carries log_mu, as ring.sample()'s
    idx = torch.from_numpy(mirror.sweep_call(512, 84, 70, 64, 1, 1)).to(DEV)
    assert set(batch) == set(ring.sample(64)) == {"states", "actions", "rewards", "next_states", "log_mu"}
    assert torch.equal(batch["rewards"], ring.store["rewards"][idx])
    assert batch["log_mu"].shape == (64,) and torch.isnan(batch["log_mu"]).all()     # a flat add: unknown


# ---- the learner -----------------------------------------------------------------------------------------------------------

H, CAP, K = 128, 512, 128


def _twin_learners(seed=0, loss="reference"):
    uav = _uav()
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        out.append(uav.DeviceActorCritic(12, H, 12, 1e-3, 5e-3, 0.95, DEV, loss=loss, max_batch=K))
    return out


def _learner_ring(rng, seed, T=8, behaviour=None, kind="ReplayRing"):
    """512 slots behind a rollout of T * 80 transitions (T = 8: 640, full and wrapped; T = 4: 320 of them)."""
    ring = getattr(_uav(), kind)(CAP, DEV, seed=seed, max_batch=K)
    if behaviour is None:
        ring.add_rollout(*_rollout(rng, T, 8, 10))
    else:
        ring.with_behaviour().add_rollout_behaviour(*_rollout(rng, T, 8, 10), behaviour=behaviour)
    return ring


def _gathered(ring, sweep, call):
    first, W = sweep.window
    idx = torch.from_numpy(mirror.sweep_call(ring.capacity, first, W, K, ring.seed, call)).to(DEV)
    return {key: ring.store[key][idx] for key in ring.store}, idx


def _assert_same_learner(la, lb):
    assert np.array_equal(la._get_params(), lb._get_params())


def test_update_from_a_sweep_equals_update_on_the_mirrors_rows():
    la, lb = _twin_learners()
    ring = _learner_ring(np.random.RandomState(5), seed=21, kind="PrioritizedReplayRing")
    sweep = ring.sweep(K)
    assert sweep.window == (128, 512) and sweep.minibatches == 4
    seen = []
    for call in range(8):                                           # two whole epochs
        a_loss, c_loss, td = la.update_from(sweep, K)
        batch, idx = _gathered(ring, sweep, call)
        b_a, b_c, b_td = lb.update(batch)
        assert torch.equal(sweep._idx, idx)
        assert torch.equal(a_loss, b_a) and torch.equal(c_loss, b_c) and torch.equal(td, b_td)
        assert torch.equal(ring.priorities[idx], td.abs())          # a prioritised ring's priorities still receive |delta|
        _assert_same_learner(la, lb)
        seen.append(idx.cpu().numpy())
    for e in range(2):
        assert np.array_equal(np.sort(np.concatenate(seen[4 * e:4 * e + 4])), np.arange(CAP))
    assert sweep.position() == 8
    la.check(); lb.check(); ring.check()


def test_update_from_a_sweep_with_clip_eps_takes_the_rings_log_mu():
    la, lb = _twin_learners(3, loss="per_sample")
    ring = _learner_ring(np.random.RandomState(6), seed=22, behaviour=la)
    torch.manual_seed(4)                                            # the actor moves on; the ring's log_mu stays
    moved = 0.5 * (la._get_params() + _uav().DeviceActorCritic(12, H, 12, 1e-3, 5e-3, 0.95, DEV, max_batch=K)._get_params())
    la._set_params(moved); lb._set_params(moved)
    sweep = ring.sweep(K, "all")
    ra, rb = torch.empty(K, device=DEV), torch.empty(K, device=DEV)
    for call in range(8):
        a_loss, c_loss, td = la.update_from(sweep, K, clip_eps=0.2, ratio_out=ra)
        batch, idx = _gathered(ring, sweep, call)
        b_a, b_c, b_td = lb.update(batch, log_mu=ring.log_mu[idx], clip_eps=0.2, ratio_out=rb)
        assert torch.equal(a_loss, b_a) and torch.equal(c_loss, b_c) and torch.equal(td, b_td)
        assert torch.equal(ra, rb) and torch.isfinite(ra).all() and not (ra == 1.0).all()
        _assert_same_learner(la, lb)
    la.check(); lb.check()


def test_update_from_many_over_two_sweeps_equals_the_grad_apply_chain():
    la, lb = _twin_learners(1)
    sweeps_a = [_learner_ring(np.random.RandomState(7 + r), seed=30 + r, T=4 + 4 * r).sweep(K) for r in range(2)]
    sweeps_b = [_learner_ring(np.random.RandomState(7 + r), seed=30 + r, T=4 + 4 * r).sweep(K) for r in range(2)]
    assert [s.window for s in sweeps_a] == [(0, 320), (128, 512)]   # 2 and 4 minibatches an epoch
    for call in range(5):
        al, cl, tds = la.update_from_many(sweeps_a, K)
        rows = lb.new_rows(2)
        ref_td = []
        for r, sweep in enumerate(sweeps_b):
            _, td, idx = lb.grad_from(sweep, K, rows[r])
            first, W = sweep.window
            assert np.array_equal(idx.cpu().numpy(), mirror.sweep_call(CAP, first, W, K, 30 + r, call))
            ref_td.append(td)
        b_al, b_cl = lb.apply(rows)
        assert torch.equal(al, b_al) and torch.equal(cl, b_cl)
        assert all(torch.equal(x, y) for x, y in zip(tds, ref_td))
        _assert_same_learner(la, lb)
    la.check(); lb.check()


def test_capture_a_sweep_update_and_replay_it_through_an_epoch_boundary():
    la, lb = _twin_learners(2)
    ring = _learner_ring(np.random.RandomState(6), seed=77)
    sweep = ring.sweep(K)
    la.update_from(sweep, K)                                        # warm-up, eager: call 0
    lb.update(_gathered(ring, sweep, 0)[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ga, gc, gtd = la.update_from(sweep, K)
    assert sweep.position() == 1                                    # the capture itself ran nothing
    seen = []
    for call in range(1, 7):                                        # calls 1 .. 6: the boundary lies between 3 and 4
        g.replay()
        torch.cuda.synchronize()
        batch, idx = _gathered(ring, sweep, call)
        assert torch.equal(sweep._idx, idx), call
        b_a, b_c, b_td = lb.update(batch)
        assert torch.equal(ga, b_a) and torch.equal(gc, b_c) and torch.equal(gtd, b_td)
        _assert_same_learner(la, lb)
        seen.append(idx.cpu().numpy())
    assert sweep.position() == 7
    first_epoch = np.concatenate([mirror.sweep_call(CAP, *sweep.window, K, 77, 0)] + seen[:3])
    assert np.array_equal(np.sort(first_epoch), np.arange(CAP))
    la.check(); ring.check()


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_refusals_enqueue_nothing_and_leave_the_cursor_alone():
    uav, lib = _uav(), _uav()._lib.load()
    ptr = uav._lib.ptr
    seed = 9
    a = _filled(300, 200, seed, max_batch=64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(512, dtype=torch.int64, device=DEV)
    cur = torch.tensor([5, -1], dtype=torch.int64, device=DEV)
    ring = a._ring()
    fn = lib.uavtrack_replay_sample_sweep

    def refused(message, view, first, length, n, cursor=cur, indices=out, handle=a._h):
        assert fn(handle, None if view is None else C.byref(view), first, length, n, ptr(cursor), ptr(indices), st) != 0
        assert message in lib.uavtrack_last_error(), lib.uavtrack_last_error()

    refused(b"n = 11 exceeds length = 10", ring, 0, 10, 11)
    refused(b"leaves the ring's 200 valid slots", ring, 150, 51, 10)         # beyond count on a ring that is not full
    refused(b"leaves the ring's 200 valid slots", ring, 0, 201, 10)
    refused(b"n = 65 outside [1, max_batch = 64]", ring, 0, 200, 65)
    refused(b"n = 0 outside", ring, 0, 200, 0)
    refused(b"length = 0 < 1", ring, 0, 0, 1)
    refused(b"first = 300 outside [0, capacity = 300)", ring, 300, 10, 10)
    refused(b"first = -1 outside", ring, -1, 10, 10)
    refused(b"cursor must not be null", ring, 0, 200, 10, cursor=None)
    refused(b"indices must not be null", ring, 0, 200, 10, indices=None)
    refused(b"ring is null", None, 0, 200, 10)
    refused(b"null handle", ring, 0, 200, 10, handle=None)
    none = a._ring()
    none.count = 0
    refused(b"empty", none, 0, 1, 1)
    big = a._ring()
    big.capacity = 301
    refused(b"max_capacity", big, 0, 200, 10)
    full = a._ring()
    full.count = 300
    refused(b"leaves the ring's 300 valid slots", full, 0, 301, 10)
    assert fn(a._h, C.byref(full), 250, 100, 10, ptr(cur), ptr(out), st) == 0    # a full ring's window may wrap: call 5
    assert np.array_equal(out[:10].cpu().numpy(), mirror.sweep_call(300, 250, 100, 10, seed, 5))
    assert cur.tolist() == [6, 5]                                            # one call went through, the refused ones left no trace

    # the Python side: ValueError before any library call
    sweep = a.sweep(50, "all")
    with pytest.raises(ValueError, match="exceeds the window's 10 slots"):
        a.sweep(11, (0, 10))
    with pytest.raises(ValueError, match="leaves the ring's 200 valid slots"):
        a.sweep(10, (150, 51))
    learner = uav.DeviceActorCritic(12, 64, 12, 1e-3, 5e-3, 0.95, DEV, max_batch=64)
    with pytest.raises(ValueError, match="no importance weights"):
        learner.update_from(sweep, 50, importance=True)
    with pytest.raises(ValueError, match="no importance weights"):
        learner.grad_from(sweep, 50, beta_final=1.0, anneal_calls=4)
    with pytest.raises(ValueError, match="this sweep was made for minibatches of 50"):
        learner.update_from(sweep, 40)
    with pytest.raises(ValueError, match="rho_bar needs"):                   # no behaviour store: as on the ring itself
        learner.update_from(sweep, 50, rho_bar=1.0)
    fresh = uav.ReplayRing(64, DEV, seed=seed)
    with pytest.raises(ValueError, match="before any add"):
        fresh.sweep(8)
    fresh.count = 64                                                         # (valid slots without an add)
    pinned = fresh.sweep(8, (0, 64))
    with pytest.raises(ValueError, match="before any add"):
        pinned.rebind()
    assert pinned.window == (0, 64) and pinned.position() == 0
    with pytest.raises(RuntimeError, match="uavtrack_replay_sample_sweep failed.*leaves the ring's 10 valid slots"):
        fresh.count = 10                                                     # the ring shrank under the sweep: the library refuses
        pinned.draw()
    fresh.count = 64
    assert pinned.position() == 0
    assert sweep.position() == 1                                             # rho_bar's refusal came behind its draw
    assert np.array_equal(pinned.draw().cpu().numpy(), mirror.sweep_call(64, 0, 64, 8, seed, 0))
    # and the handle counter still stands at 0
    assert np.array_equal(a.draw(64).cpu().numpy(), umirror.draw(200, 64, seed, 0))
    a.check()
