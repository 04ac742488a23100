"""The importance-weighted learner update (uavtrack_learner_update_weighted / _grad_weighted, DeviceActorCritic's
`weights` / `importance` arguments) and the annealed ring draw (uavtrack_replay_sample_annealed) on the MI355X: ones
and NULL against the unweighted update to the bit, exact scaling by a power of two, random weights against the float64
mirror (tests/learner_mirror.py with weights) at test_sweep_against_fp64_mirror's tolerances, the split form,
refused weights, the ring end to end, and the device-side beta schedule, eager and under graph replay."""
import types

import numpy as np
import pytest
import torch

import learner_harness as lh
import learner_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA

# shapes that cross the tile (4096 / max(16, H) rows) and workgroup boundaries: one row, one partial tile, a tile less
# one row, two tiles and a row, 128 workgroups
SHAPES = [(1, 9, 1), (33, 12, 2), (64, 48, 63), (128, 12, 65), (128, 12, 4096)]
CASES = [(H, A, n, loss, gather) for H, A, n in SHAPES for loss in ("reference", "per_sample") for gather in (True, False)]


def _uav():
    import uavtrack
    return uavtrack


# ---- 1. ones are nothing -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,loss,gather", CASES)
def test_ones_and_null_are_the_unweighted_update_bitwise(H, A, n, loss, gather):
    """uavtrack_learner_update, uavtrack_learner_update_weighted with weights == NULL (called directly), and a device
    vector of ones."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    prio0 = torch.rand(cap, device=DEV) + 0.1
    modes = (dict(), dict(entry="weighted"), dict(w=torch.ones(n, device=DEV)))
    outs = []
    for mode in modes:
        L = lh.learner(H, A, loss, blob, max_batch=n)
        outs.append(lh.update(L, n, store, cap, it, prio0.clone(), **mode))
        L.check()
    assert np.isfinite(outs[0]["actor_loss"]) and np.array_equal(outs[0]["step"], np.ones(8))
    assert not np.array_equal(outs[0]["prio"], prio0.cpu().numpy())
    lh.same(outs[0], outs[1])
    lh.same(outs[0], outs[2])
    L = lh.learner(H, A, loss, blob, max_batch=n)
    rows = [lh.row(L, n, store, cap, it, **mode) for mode in modes]
    L.check()
    for row, td in rows[1:]:
        assert np.array_equal(row.view(np.int32), rows[0][0].view(np.int32)) and np.array_equal(td, rows[0][1])
    assert np.array_equal(rows[0][1], outs[0]["td"])


# ---- 2. powers of two scale exactly ------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,loss,gather", CASES)
def test_half_weights_scale_the_row_exactly(H, A, n, loss, gather):
    """Every weight 0.5: each term of every sum is halved exactly, and sums of halves are halves of the sums, so words
    [0, P + 4) of the row are 0.5 x the unweighted row's to the bit; td_delta is untouched."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    L = lh.learner(H, A, loss, blob, max_batch=n)
    P = L.num_params
    row_u, td_u = lh.row(L, n, store, cap, it)
    row_h, td_h = lh.row(L, n, store, cap, it, torch.full((n,), 0.5, device=DEV))
    L.check()
    assert np.abs(row_u[:P]).max() > 0 and np.isfinite(row_u[:P + 4]).all()
    assert np.array_equal(row_h[:P + 4], np.float32(0.5) * row_u[:P + 4])
    assert np.array_equal(row_h[P + 4:].view(np.int32), row_u[P + 4:].view(np.int32))     # n, status, tag
    assert np.array_equal(td_h, td_u)


# ---- 3. random weights against the fp64 weighted mirror ------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,loss,gather", CASES)
def test_random_weights_against_fp64_weighted_mirror(H, A, n, loss, gather):
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    w = lh.make_weights(np.random.RandomState(n + H), n)
    assert w.max() == 1.0 and w.min() >= 0.0 and (n < 2 or (w == 0).any())
    L = lh.learner(H, A, loss, blob, max_batch=n)
    out = lh.update(L, n, store, cap, it, None, lh.dev(w))
    L.check()
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), GAMMA, loss, weights=w)[:4]
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ral, rcl, rtd)
    lh.assert_step_from_zero(out, blob, g, n, H, A)
    if n >= 63:       # the weights are in the result: the unweighted gradient is far outside the bound
        gu = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), GAMMA, loss)[3]
        assert np.abs(out["exp_avg"] / 0.1 - gu).max() > 100 * lh.tol_g(n, g)


# ---- 4. the split form -------------------------------------------------------------------------------------------------

SPLIT = [(64, 48, 63), (128, 12, 65), (128, 12, 4096)]


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n", SPLIT)
def test_one_weighted_row_applied_alone_is_the_weighted_update(H, A, n, loss):
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    w = lh.dev(lh.make_weights(np.random.RandomState(n), n))
    closed = lh.learner(H, A, loss, blob, max_batch=n)
    want = lh.update(closed, n, store, cap, it, None, w)
    split = lh.learner(H, A, loss, blob, max_batch=n)
    row, td = split._grad(n, store, cap, it, None, None, w)
    al, cl = split.apply(row)
    split.check(); closed.check()
    lh.same(dict(lh.state(split), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy(), td=td.cpu().numpy(),
                 prio=None), want)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n", SPLIT)
def test_two_rows_over_the_halves_match_the_mirror_on_the_whole_batch(H, A, n, loss, mixed):
    """Two gradient rows over the two halves of a batch, applied together, against the weighted mirror on the whole
    batch; `mixed`: the second half goes through the unweighted uavtrack_learner_grad (weights of 1 in the mirror) and
    the apply accepts the pair."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    w = lh.make_weights(np.random.RandomState(n + 1), n)
    h = n // 2
    if mixed:
        w[h:] = 1.0
    L = lh.learner(H, A, loss, blob, max_batch=n)
    rows = L.new_rows(2)
    _, td0 = L._grad(h, store, cap, it[:h], rows[0], None, lh.dev(w[:h]))
    _, td1 = L._grad(n - h, store, cap, it[h:].contiguous(), rows[1], None, None if mixed else lh.dev(w[h:]))
    al, cl = L.apply(rows)
    L.check()
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), GAMMA, loss, weights=w)[:4]
    lh.assert_losses_and_td(al.cpu().numpy(), cl.cpu().numpy(), torch.cat([td0, td1]).cpu().numpy(), ral, rcl, rtd)
    lh.assert_step_from_zero(lh.state(L), blob, g, n, H, A)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("nan"), -1.0, float("inf")], ids=["nan", "negative", "inf"])
def test_a_bad_weight_refuses_the_update(bad):
    H, A, n = 128, 12, 65
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    L = lh.learner(H, A, "reference", blob, max_batch=n)
    good = lh.dev(lh.make_weights(np.random.RandomState(3), n))
    L._run(n, store, cap, it, None, good)
    L.check()
    before = lh.state(L)
    prio = torch.rand(cap, device=DEV) + 0.1
    prio0 = prio.clone()
    w = good.clone()
    w[40] = bad                                                        # in the second tile of the batch
    al, cl, _ = L._run(n, store, cap, it, prio, w)
    assert torch.isnan(al) and torch.isnan(cl)
    lh.same(lh.state(L), before)
    assert torch.equal(prio, prio0)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    L.check()                                                          # the count restarts
    # the split form: the row carries status bit 2, the apply of it changes nothing, the priority write is held back
    row, td = L._grad(n, store, cap, it, None, None, w)
    assert int(row.cpu().numpy().view(np.int32)[L.num_params + 6]) == 4
    al, cl = L.apply(row)
    L.write_priorities(types.SimpleNamespace(priorities=prio, capacity=cap), it, td)
    assert torch.isnan(al) and torch.isnan(cl)
    lh.same(lh.state(L), before)
    assert torch.equal(prio, prio0)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    # the next good update succeeds
    al, cl, _ = L._run(n, store, cap, it, prio, good)
    L.check()
    assert torch.isfinite(al) and torch.isfinite(cl) and not torch.equal(prio, prio0)
    assert np.array_equal(lh.state(L)["step"], before["step"] + 1)


def _ring(data, seed, max_batch, prio_seed=1, extra=50):
    n = len(data[1])
    r = _uav().PrioritizedReplayRing(n + extra, DEV, seed=seed, max_batch=max_batch)
    r.add({k: torch.from_numpy(x) for k, x in zip(("states", "actions", "rewards", "next_states"), data)})
    if prio_seed is not None:
        r.priorities[:n] = lh.dev(np.random.RandomState(prio_seed).uniform(0.1, 2.0, n).astype(np.float32))
    return r


def test_a_refused_draw_refuses_the_update_behind_it():
    """All priorities zero: the draw is refused on the device and writes NaN weights, which refuse the update behind it
    with no host involvement; both handles report it."""
    H, A, n, k = 64, 12, 500, 200
    data = lh.batch(np.random.RandomState(8), n, A)
    ring = _ring(data, 3, k, prio_seed=None)
    L = lh.learner(H, A, "reference", lh.init_blob(H, A, 8), max_batch=k)
    before = lh.state(L)
    ring.priorities.zero_()
    al, cl, _ = L.update_from(ring, k, beta=0.4, importance=True)
    assert torch.isnan(al) and torch.isnan(cl)
    lh.same(lh.state(L), before)
    assert not ring.priorities.any()
    with pytest.raises(RuntimeError, match="refused"):
        ring.check()
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    ring.priorities[:n] = 1.0
    al, cl, _ = L.update_from(ring, k, beta=0.4, importance=True)
    ring.check(); L.check()
    assert torch.isfinite(al) and np.array_equal(lh.state(L)["step"], np.ones(8))


# ---- 6. the ring, end to end -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_update_from_with_importance_is_draw_update_write(loss):
    H, A, n, k = 128, 12, 3000, 1000
    data = lh.batch(np.random.RandomState(21), n, A)
    blob = lh.init_blob(H, A, 21)
    one, ring = lh.learner(H, A, loss, blob, max_batch=k), _ring(data, 17, k)
    two, twin = lh.learner(H, A, loss, blob, max_batch=k), _ring(data, 17, k)
    for u in range(3):
        al, cl, td = one.update_from(ring, k, beta=0.4, importance=True)
        idx, w = twin.draw(k, 0.4)
        assert 0 < float(w.min()) < 1 and float(w.max()) == 1.0
        al2, cl2, td2 = two.update({key: twin.store[key][idx] for key in twin.store}, weights=w)
        two.write_priorities(twin, idx, td2)
        assert torch.equal(al, al2) and torch.equal(cl, cl2) and torch.equal(td, td2) and torch.isfinite(al), u
        assert torch.equal(ring._idx[:k], idx) and torch.equal(ring._w[:k], w)
        assert torch.equal(ring.priorities, twin.priorities)
    lh.same(lh.state(one), lh.state(two))
    for x in (one, two, ring, twin):
        x.check()
    # the weights are in the result: the same draws without them end elsewhere
    three, third = lh.learner(H, A, loss, blob, max_batch=k), _ring(data, 17, k)
    for u in range(3):
        three.update_from(third, k, beta=0.4)
    assert not np.array_equal(lh.state(three)["params"], lh.state(one)["params"])


def test_beta_zero_with_importance_is_importance_off():
    H, A, n, k = 64, 12, 2000, 700
    data = lh.batch(np.random.RandomState(22), n, A)
    blob = lh.init_blob(H, A, 22)
    outs = []
    for kw in (dict(beta=0.0, importance=True), dict(importance=False), dict()):
        L, ring = lh.learner(H, A, "reference", blob, max_batch=k), _ring(data, 4, k)
        res = [tuple(t.cpu().numpy() for t in L.update_from(ring, k, **kw)) for _ in range(2)]
        L.check(); ring.check()
        outs.append((lh.state(L), res, ring.priorities.cpu().numpy()))
    idx, w = _ring(data, 4, k).draw(k, 0.0)
    assert torch.equal(w, torch.ones(k, device=DEV))                     # the weights are then exactly 1.0
    for other in outs[1:]:
        lh.same(outs[0][0], other[0])
        assert np.array_equal(outs[0][2], other[2])
        for ra, rb in zip(outs[0][1], other[1]):
            for x, y in zip(ra, rb):
                assert np.array_equal(x, y)


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_update_from_many_uses_each_rings_own_weights(loss):
    """Two rings, importance on: the update is the mirror's over both draws, each with its own weights -- normalised by
    its own draw's maximum, so both rows hold a weight of exactly 1."""
    H, A, k = 128, 12, 600
    blob = lh.init_blob(H, A, 23)
    datas = [lh.batch(np.random.RandomState(30 + j), 900 + 100 * j, A) for j in range(2)]
    rings = [_ring(d, 40 + j, k, prio_seed=j) for j, d in enumerate(datas)]
    twins = [_ring(d, 40 + j, k, prio_seed=j) for j, d in enumerate(datas)]
    L = lh.learner(H, A, loss, blob, max_batch=k)
    before = [ring.priorities.cpu().numpy() for ring in rings]
    al, cl, tds = L.update_from_many(rings, k, importance=True, beta=0.7)
    L.check()
    drawn = [t.draw(k, 0.7) for t in twins]
    rows, parts = [], []
    for d, (idx, w) in zip(datas, drawn):
        assert float(w.max()) == 1.0
        i, wn = idx.cpu().numpy(), w.cpu().numpy()
        parts.append((lh.gathered(d, i), wn))
        rows.append(mirror.shard_sums(blob, H, A, *lh.gathered(d, i), GAMMA, loss, wn))
    ral, rcl, g = mirror.combine(rows, H, A, loss)
    whole = tuple(np.concatenate([p[0][q] for p in parts]) for q in range(4))
    wal, wcl, rtd, wg = mirror.losses_and_grads(blob, H, A, *whole, GAMMA, loss, weights=np.concatenate([p[1] for p in parts]))[:4]
    assert abs(ral - wal) <= 1e-12 * abs(wal) and np.abs(g - wg).max() <= 1e-12 * np.abs(wg).max()
    lh.assert_losses_and_td(al.cpu().numpy(), cl.cpu().numpy(), torch.cat(tds).cpu().numpy(), ral, rcl, rtd)
    lh.assert_step_from_zero(lh.state(L), blob, g, 2 * k, H, A)
    for ring, p0, (idx, _), td in zip(rings, before, drawn, tds):        # each ring's priorities from its own draw
        want = mirror.last_wins(p0, idx.cpu().numpy(), np.abs(td.cpu().numpy()))
        assert np.array_equal(ring.priorities.cpu().numpy(), want.astype(np.float32))


# ---- 7. annealed beta ------------------------------------------------------------------------------------------------------

def _beta(c, beta0=0.4, beta1=1.0, calls=3):
    return beta0 + (beta1 - beta0) * min(1.0, c / calls)


def test_annealed_draws_equal_draws_at_the_schedules_beta():
    n, k = 5000, 777
    data = lh.batch(np.random.RandomState(41), n, 12)
    ring, twin = _ring(data, 9, k), _ring(data, 9, k)
    seen = []
    for c in range(5):
        idx, w = ring.draw(k, 0.4, beta_final=1.0, anneal_calls=3)
        idx2, w2 = twin.draw(k, _beta(c))
        assert torch.equal(idx, idx2) and torch.equal(w, w2), c
        assert float(w.max()) == 1.0 and float(w.min()) < 1.0
        seen.append(w.cpu().numpy())
    ring.check(); twin.check()
    assert _beta(0) == 0.4 and _beta(3) == _beta(4) == 1.0 and len({_beta(c) for c in range(5)}) == 4
    # beta does move the weights: the same draw at the first beta gives other weights than at the last
    third = _ring(data, 9, k)
    for c in range(5):
        _, w3 = third.draw(k, 0.4)
    assert not np.array_equal(w3.cpu().numpy(), seen[4])
    with pytest.raises(ValueError, match="anneal_calls"):
        ring.draw(k, 0.4, beta_final=1.0)
    with pytest.raises(RuntimeError, match="uavtrack_replay_sample_annealed: beta1"):
        ring.draw(k, 0.4, beta_final=-1.0, anneal_calls=3)


def test_a_replayed_graph_anneals():
    """One update_from(..., importance=True, beta_final=1.0, anneal_calls=3) captured once and replayed five times ==
    five eager updates at the schedule's beta, bitwise: parameters and priorities after every replay."""
    H, A, n, k = 128, 12, 5000, 2048
    data = lh.batch(np.random.RandomState(42), n, A)
    blob = lh.init_blob(H, A, 42)
    eager, re_ = lh.learner(H, A, "reference", blob, max_batch=k), _ring(data, 5, k)
    graphed, rg = lh.learner(H, A, "reference", blob, max_batch=k), _ring(data, 5, k)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = graphed.update_from(rg, k, beta=0.4, importance=True, beta_final=1.0, anneal_calls=3)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(graphed)["step"], np.zeros(8))           # capture ran nothing
    for c in range(5):
        e_out = eager.update_from(re_, k, beta=_beta(c), importance=True)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y), c
        assert np.array_equal(graphed._get_params(), eager._get_params()), c
        assert torch.equal(rg.priorities, re_.priorities), c
    lh.same(lh.state(graphed), lh.state(eager))
    assert np.array_equal(lh.state(graphed)["step"], np.full(8, 5))
    graphed.check(); eager.check(); re_.check(); rg.check()
