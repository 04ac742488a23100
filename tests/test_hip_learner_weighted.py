"""The importance-weighted learner update (uavtrack_learner_update_weighted / _grad_weighted, DeviceActorCritic's
`weights` / `importance` arguments) and the annealed ring draw (uavtrack_replay_sample_annealed) on the MI355X: ones
and NULL against the unweighted update to the bit, exact scaling by a power of two, random weights against the float64
weighted mirror (tests/learner_weighted_mirror.py) at test_sweep_against_fp64_mirror's tolerances, the split form,
refused weights, the ring end to end, and the device-side beta schedule, eager and under graph replay."""
import types

import numpy as np
import pytest
import torch

import learner_dp_mirror as dp
import learner_mirror as mirror
import learner_weighted_mirror as wm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = (1e-3, 5e-3)
GAMMA = 0.95

# shapes that cross the tile (4096 / max(16, H) rows) and workgroup boundaries: one row, one partial tile, a tile less
# one row, two tiles and a row, 128 workgroups
SHAPES = [(1, 9, 1), (33, 12, 2), (64, 48, 63), (128, 12, 65), (128, 12, 4096)]
CASES = [(H, A, n, loss, gather) for H, A, n in SHAPES for loss in ("reference", "per_sample") for gather in (True, False)]


def _uav():
    import uavtrack
    return uavtrack


def _learner(H, A, loss="reference", blob=None, max_batch=0):
    L = _uav().DeviceActorCritic(12, H, A, LR[0], LR[1], GAMMA, DEV, loss=loss, max_batch=max_batch)
    if blob is not None:
        L._set_params(np.ascontiguousarray(blob, np.float32))
    return L


def _state(L):
    m, v, st = L._optim_state()
    return {"params": L._get_params(), "exp_avg": m, "exp_avg_sq": v, "step": st}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


_cache = {}


def _case(H, A, n, gather):
    """(blob, host batch over the store, device store, capacity, host indices, device indices or None), built once."""
    key = (H, A, n, gather)
    if key not in _cache:
        rng = np.random.RandomState(H * 1000 + n + (7 if gather else 0))
        cap = n + 7 if gather else n
        b = dp.batch(rng, cap, A)
        idx = rng.randint(0, cap, size=n).astype(np.int64) if gather else np.arange(n)
        store = {k: _dev(x) for k, x in zip(("states", "actions", "rewards", "next_states"), b)}
        _cache[key] = (dp.init_blob(H, A, H + n), b, store, cap, idx, _dev(idx) if gather else None)
    return _cache[key]


def _gathered(b, idx):
    return tuple(x[idx] for x in b)


def _update(L, n, store, cap, it, prio, mode):
    """One update: mode "plain" = uavtrack_learner_update, "null" = uavtrack_learner_update_weighted with weights ==
    NULL (called directly), or a device weight tensor."""
    if mode == "plain":
        al, cl, td = L._run(n, store, cap, it, prio)
    elif mode == "null":
        from uavtrack import _lib
        losses, td = torch.empty(2, device=DEV), torch.empty(n, device=DEV)
        _lib.check(L._lib.uavtrack_learner_update_weighted(
            L._h, n, *L._batch_args(store, cap, it), None, _lib.ptr(losses[0:1]), _lib.ptr(losses[1:2]), _lib.ptr(td),
            _lib.ptr(prio), L._stream()), "uavtrack_learner_update_weighted")
        al, cl = losses[0], losses[1]
    else:
        al, cl, td = L._run(n, store, cap, it, prio, mode)
    return dict(_state(L), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy(), td=td.cpu().numpy(),
                prio=None if prio is None else prio.cpu().numpy())


def _row(L, n, store, cap, it, mode):
    if mode == "null":
        from uavtrack import _lib
        row, td = torch.empty(L.row_floats, device=DEV), torch.empty(n, device=DEV)
        _lib.check(L._lib.uavtrack_learner_grad_weighted(
            L._h, n, *L._batch_args(store, cap, it), None, _lib.ptr(td), _lib.ptr(row), L._stream()),
            "uavtrack_learner_grad_weighted")
    else:
        row, td = L._grad(n, store, cap, it, None, None, None if mode == "plain" else mode)
    return row.cpu().numpy(), td.cpu().numpy()


# ---- 1. ones are nothing -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,loss,gather", CASES)
def test_ones_and_null_are_the_unweighted_update_bitwise(H, A, n, loss, gather):
    blob, b, store, cap, idx, it = _case(H, A, n, gather)
    prio0 = torch.rand(cap, device=DEV) + 0.1
    ones = torch.ones(n, device=DEV)
    outs = []
    for mode in ("plain", "null", ones):
        L = _learner(H, A, loss, blob, max_batch=n)
        outs.append(_update(L, n, store, cap, it, prio0.clone(), mode))
        L.check()
    assert np.isfinite(outs[0]["actor_loss"]) and np.array_equal(outs[0]["step"], np.ones(8))
    assert not np.array_equal(outs[0]["prio"], prio0.cpu().numpy())
    _same(outs[0], outs[1])
    _same(outs[0], outs[2])
    L = _learner(H, A, loss, blob, max_batch=n)
    rows = [_row(L, n, store, cap, it, mode) for mode in ("plain", "null", ones)]
    L.check()
    for row, td in rows[1:]:
        assert np.array_equal(row.view(np.int32), rows[0][0].view(np.int32)) and np.array_equal(td, rows[0][1])
    assert np.array_equal(rows[0][1], outs[0]["td"])


# ---- 2. powers of two scale exactly ------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,loss,gather", CASES)
def test_half_weights_scale_the_row_exactly(H, A, n, loss, gather):
    """Every weight 0.5: each term of every sum is halved exactly, and sums of halves are halves of the sums, so words
    [0, P + 4) of the row are 0.5 x the unweighted row's to the bit; td_delta is untouched."""
    blob, b, store, cap, idx, it = _case(H, A, n, gather)
    L = _learner(H, A, loss, blob, max_batch=n)
    P = L.num_params
    row_u, td_u = _row(L, n, store, cap, it, "plain")
    row_h, td_h = _row(L, n, store, cap, it, torch.full((n,), 0.5, device=DEV))
    L.check()
    assert np.abs(row_u[:P]).max() > 0 and np.isfinite(row_u[:P + 4]).all()
    assert np.array_equal(row_h[:P + 4], np.float32(0.5) * row_u[:P + 4])
    assert np.array_equal(row_h[P + 4:].view(np.int32), row_u[P + 4:].view(np.int32))     # n, status, tag
    assert np.array_equal(td_h, td_u)


# ---- 3. random weights against the fp64 weighted mirror ------------------------------------------------------------------

def _assert_losses_and_td(al, cl, td, ral, rcl, rtd):
    """test_sweep_against_fp64_mirror's bounds: td_delta and the losses at 2e-5 of their scale."""
    tds = np.abs(rtd).max() + 1e-6
    np.testing.assert_allclose(td, rtd, rtol=0, atol=2e-5 * tds)
    assert abs(float(cl) - rcl) <= 2e-5 * (np.mean(rtd ** 2) + 1e-12) + 1e-12, (float(cl), rcl)
    nlp_scale = abs(ral) + np.mean(np.abs(rtd)) * 30
    assert abs(float(al) - ral) <= 2e-5 * nlp_scale, (float(al), ral)


def _assert_step_from_zero(st, blob, g, n, H, A):
    """test_sweep_against_fp64_mirror's bounds on the first Adam step: the gradient (exp_avg / 0.1) within
    2e-6 (1 + log2 n) of its largest element, the parameters within 1e-3 lr except where the fp64 gradient is within
    the gradient's rounding of 0 (Adam's first step may then take either sign: within 2 lr)."""
    gd = st["exp_avg"] / 0.1
    gmax = np.abs(g).max()
    tol_g = 2e-6 * (1 + np.log2(n)) * gmax
    print(f"gradient error {np.abs(gd - g).max():.3e} of bound {tol_g:.3e}")
    assert np.abs(gd - g).max() <= tol_g + 1e-30, (np.abs(gd - g).max(), tol_g)
    p64 = mirror.adam(blob.astype(np.float64), np.zeros(g.size), np.zeros(g.size), np.ones(8, np.int64), g, LR, H, A)[0]
    lr_of = np.concatenate([np.full(k, LR[0] if t < 4 else LR[1]) for t, k in enumerate(mirror.layout(H, A)[0])])
    near0 = np.abs(g) <= 4 * tol_g + 1e-8
    err = np.abs(st["params"] - p64)
    assert (err[~near0] <= 1e-3 * lr_of[~near0] + 1e-6 * np.abs(p64[~near0])).all(), err[~near0].max()
    assert (err[near0] <= 2 * lr_of[near0] + 1e-6).all()


@pytest.mark.parametrize("H,A,n,loss,gather", CASES)
def test_random_weights_against_fp64_weighted_mirror(H, A, n, loss, gather):
    blob, b, store, cap, idx, it = _case(H, A, n, gather)
    w = wm.make_weights(np.random.RandomState(n + H), n)
    assert w.max() == 1.0 and w.min() >= 0.0 and (n < 2 or (w == 0).any())
    L = _learner(H, A, loss, blob, max_batch=n)
    out = _update(L, n, store, cap, it, None, _dev(w))
    L.check()
    ral, rcl, rtd, g = wm.losses_and_grads(blob, H, A, *_gathered(b, idx), GAMMA, loss, w)
    _assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ral, rcl, rtd)
    _assert_step_from_zero(out, blob, g, n, H, A)
    if n >= 63:       # the weights are in the result: the unweighted gradient is far outside the bound
        gu = mirror.losses_and_grads(blob, H, A, *_gathered(b, idx), GAMMA, loss)[3]
        assert np.abs(out["exp_avg"] / 0.1 - gu).max() > 100 * 2e-6 * (1 + np.log2(n)) * np.abs(g).max()


# ---- 4. the split form -------------------------------------------------------------------------------------------------

SPLIT = [(64, 48, 63), (128, 12, 65), (128, 12, 4096)]


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n", SPLIT)
def test_one_weighted_row_applied_alone_is_the_weighted_update(H, A, n, loss):
    blob, b, store, cap, idx, it = _case(H, A, n, True)
    w = _dev(wm.make_weights(np.random.RandomState(n), n))
    closed = _learner(H, A, loss, blob, max_batch=n)
    want = _update(closed, n, store, cap, it, None, w)
    split = _learner(H, A, loss, blob, max_batch=n)
    row, td = split._grad(n, store, cap, it, None, None, w)
    al, cl = split.apply(row)
    split.check(); closed.check()
    _same(dict(_state(split), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy(), td=td.cpu().numpy(), prio=None),
          want)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n", SPLIT)
def test_two_rows_over_the_halves_match_the_mirror_on_the_whole_batch(H, A, n, loss, mixed):
    """Two gradient rows over the two halves of a batch, applied together, against the weighted mirror on the whole
    batch; `mixed`: the second half goes through the unweighted uavtrack_learner_grad (weights of 1 in the mirror) and
    the apply accepts the pair."""
    blob, b, store, cap, idx, it = _case(H, A, n, True)
    w = wm.make_weights(np.random.RandomState(n + 1), n)
    h = n // 2
    if mixed:
        w[h:] = 1.0
    L = _learner(H, A, loss, blob, max_batch=n)
    rows = L.new_rows(2)
    _, td0 = L._grad(h, store, cap, it[:h], rows[0], None, _dev(w[:h]))
    _, td1 = L._grad(n - h, store, cap, it[h:].contiguous(), rows[1], None, None if mixed else _dev(w[h:]))
    al, cl = L.apply(rows)
    L.check()
    ral, rcl, rtd, g = wm.losses_and_grads(blob, H, A, *_gathered(b, idx), GAMMA, loss, w)
    _assert_losses_and_td(al.cpu().numpy(), cl.cpu().numpy(), torch.cat([td0, td1]).cpu().numpy(), ral, rcl, rtd)
    _assert_step_from_zero(_state(L), blob, g, n, H, A)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("nan"), -1.0, float("inf")], ids=["nan", "negative", "inf"])
def test_a_bad_weight_refuses_the_update(bad):
    H, A, n = 128, 12, 65
    blob, b, store, cap, idx, it = _case(H, A, n, True)
    L = _learner(H, A, "reference", blob, max_batch=n)
    good = _dev(wm.make_weights(np.random.RandomState(3), n))
    L._run(n, store, cap, it, None, good)
    L.check()
    before = _state(L)
    prio = torch.rand(cap, device=DEV) + 0.1
    prio0 = prio.clone()
    w = good.clone()
    w[40] = bad                                                        # in the second tile of the batch
    al, cl, _ = L._run(n, store, cap, it, prio, w)
    assert torch.isnan(al) and torch.isnan(cl)
    _same(_state(L), before)
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
    _same(_state(L), before)
    assert torch.equal(prio, prio0)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    # the next good update succeeds
    al, cl, _ = L._run(n, store, cap, it, prio, good)
    L.check()
    assert torch.isfinite(al) and torch.isfinite(cl) and not torch.equal(prio, prio0)
    assert np.array_equal(_state(L)["step"], before["step"] + 1)


def _ring(data, seed, max_batch, prio_seed=1, extra=50):
    n = len(data[1])
    r = _uav().PrioritizedReplayRing(n + extra, DEV, seed=seed, max_batch=max_batch)
    r.add({k: torch.from_numpy(x) for k, x in zip(("states", "actions", "rewards", "next_states"), data)})
    if prio_seed is not None:
        r.priorities[:n] = _dev(np.random.RandomState(prio_seed).uniform(0.1, 2.0, n).astype(np.float32))
    return r


def test_a_refused_draw_refuses_the_update_behind_it():
    """All priorities zero: the draw is refused on the device and writes NaN weights, which refuse the update behind it
    with no host involvement; both handles report it."""
    H, A, n, k = 64, 12, 500, 200
    data = dp.batch(np.random.RandomState(8), n, A)
    ring = _ring(data, 3, k, prio_seed=None)
    L = _learner(H, A, "reference", dp.init_blob(H, A, 8), max_batch=k)
    before = _state(L)
    ring.priorities.zero_()
    al, cl, _ = L.update_from(ring, k, beta=0.4, importance=True)
    assert torch.isnan(al) and torch.isnan(cl)
    _same(_state(L), before)
    assert not ring.priorities.any()
    with pytest.raises(RuntimeError, match="refused"):
        ring.check()
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    ring.priorities[:n] = 1.0
    al, cl, _ = L.update_from(ring, k, beta=0.4, importance=True)
    ring.check(); L.check()
    assert torch.isfinite(al) and np.array_equal(_state(L)["step"], np.ones(8))


# ---- 6. the ring, end to end -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_update_from_with_importance_is_draw_update_write(loss):
    H, A, n, k = 128, 12, 3000, 1000
    data = dp.batch(np.random.RandomState(21), n, A)
    blob = dp.init_blob(H, A, 21)
    one, ring = _learner(H, A, loss, blob, max_batch=k), _ring(data, 17, k)
    two, twin = _learner(H, A, loss, blob, max_batch=k), _ring(data, 17, k)
    for u in range(3):
        al, cl, td = one.update_from(ring, k, beta=0.4, importance=True)
        idx, w = twin.draw(k, 0.4)
        assert 0 < float(w.min()) < 1 and float(w.max()) == 1.0
        al2, cl2, td2 = two.update({key: twin.store[key][idx] for key in twin.store}, weights=w)
        two.write_priorities(twin, idx, td2)
        assert torch.equal(al, al2) and torch.equal(cl, cl2) and torch.equal(td, td2) and torch.isfinite(al), u
        assert torch.equal(ring._idx[:k], idx) and torch.equal(ring._w[:k], w)
        assert torch.equal(ring.priorities, twin.priorities)
    _same(_state(one), _state(two))
    for x in (one, two, ring, twin):
        x.check()
    # the weights are in the result: the same draws without them end elsewhere
    three, third = _learner(H, A, loss, blob, max_batch=k), _ring(data, 17, k)
    for u in range(3):
        three.update_from(third, k, beta=0.4)
    assert not np.array_equal(_state(three)["params"], _state(one)["params"])


def test_beta_zero_with_importance_is_importance_off():
    H, A, n, k = 64, 12, 2000, 700
    data = dp.batch(np.random.RandomState(22), n, A)
    blob = dp.init_blob(H, A, 22)
    outs = []
    for kw in (dict(beta=0.0, importance=True), dict(importance=False), dict()):
        L, ring = _learner(H, A, "reference", blob, max_batch=k), _ring(data, 4, k)
        res = [tuple(t.cpu().numpy() for t in L.update_from(ring, k, **kw)) for _ in range(2)]
        L.check(); ring.check()
        outs.append((_state(L), res, ring.priorities.cpu().numpy()))
    idx, w = _ring(data, 4, k).draw(k, 0.0)
    assert torch.equal(w, torch.ones(k, device=DEV))                     # the weights are then exactly 1.0
    for other in outs[1:]:
        _same(outs[0][0], other[0])
        assert np.array_equal(outs[0][2], other[2])
        for ra, rb in zip(outs[0][1], other[1]):
            for x, y in zip(ra, rb):
                assert np.array_equal(x, y)


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_update_from_many_uses_each_rings_own_weights(loss):
    """Two rings, importance on: the update is the mirror's over both draws, each with its own weights -- normalised by
    its own draw's maximum, so both rows hold a weight of exactly 1."""
    H, A, k = 128, 12, 600
    blob = dp.init_blob(H, A, 23)
    datas = [dp.batch(np.random.RandomState(30 + j), 900 + 100 * j, A) for j in range(2)]
    rings = [_ring(d, 40 + j, k, prio_seed=j) for j, d in enumerate(datas)]
    twins = [_ring(d, 40 + j, k, prio_seed=j) for j, d in enumerate(datas)]
    L = _learner(H, A, loss, blob, max_batch=k)
    before = [ring.priorities.cpu().numpy() for ring in rings]
    al, cl, tds = L.update_from_many(rings, k, importance=True, beta=0.7)
    L.check()
    drawn = [t.draw(k, 0.7) for t in twins]
    rows, parts = [], []
    for d, (idx, w) in zip(datas, drawn):
        assert float(w.max()) == 1.0
        i, wn = idx.cpu().numpy(), w.cpu().numpy()
        parts.append((_gathered(d, i), wn))
        rows.append(wm.shard_sums(blob, H, A, *_gathered(d, i), GAMMA, loss, wn))
    ral, rcl, g = dp.combine(rows, H, A, loss)
    whole = tuple(np.concatenate([p[0][q] for p in parts]) for q in range(4))
    wal, wcl, rtd, wg = wm.losses_and_grads(blob, H, A, *whole, GAMMA, loss, np.concatenate([p[1] for p in parts]))
    assert abs(ral - wal) <= 1e-12 * abs(wal) and np.abs(g - wg).max() <= 1e-12 * np.abs(wg).max()
    _assert_losses_and_td(al.cpu().numpy(), cl.cpu().numpy(), torch.cat(tds).cpu().numpy(), ral, rcl, rtd)
    _assert_step_from_zero(_state(L), blob, g, 2 * k, H, A)
    for ring, p0, (idx, _), td in zip(rings, before, drawn, tds):        # each ring's priorities from its own draw
        want = mirror.last_wins(p0, idx.cpu().numpy(), np.abs(td.cpu().numpy()))
        assert np.array_equal(ring.priorities.cpu().numpy(), want.astype(np.float32))


# ---- 7. annealed beta ------------------------------------------------------------------------------------------------------

def _beta(c, beta0=0.4, beta1=1.0, calls=3):
    return beta0 + (beta1 - beta0) * min(1.0, c / calls)


def test_annealed_draws_equal_draws_at_the_schedules_beta():
    n, k = 5000, 777
    data = dp.batch(np.random.RandomState(41), n, 12)
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
    data = dp.batch(np.random.RandomState(42), n, A)
    blob = dp.init_blob(H, A, 42)
    eager, re_ = _learner(H, A, "reference", blob, max_batch=k), _ring(data, 5, k)
    graphed, rg = _learner(H, A, "reference", blob, max_batch=k), _ring(data, 5, k)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = graphed.update_from(rg, k, beta=0.4, importance=True, beta_final=1.0, anneal_calls=3)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(_state(graphed)["step"], np.zeros(8))           # capture ran nothing
    for c in range(5):
        e_out = eager.update_from(re_, k, beta=_beta(c), importance=True)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y), c
        assert np.array_equal(graphed._get_params(), eager._get_params()), c
        assert torch.equal(rg.priorities, re_.priorities), c
    _same(_state(graphed), _state(eager))
    assert np.array_equal(_state(graphed)["step"], np.full(8, 5))
    graphed.check(); eager.check(); re_.check(); rg.check()
