"""Multi-step targets on the MI355X: the n-step ring add (uavtrack_replay_add_rollout_nstep) against the numpy mirror
(tests/nstep_mirror.py), bitwise over all five stores and the priorities; n = 1 as today's adds; the learner's per-row
discounts (uavtrack_learner_update_discounted / _grad_discounted) with a store of float32(gamma) and with NULL as the
plain update to the bit, with random discounts against the float64 mirror at test_sweep_against_fp64_mirror's bounds;
the split form; refused discounts and host-side errors; the Python surface; graph capture; a real rollout end to end."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import learner_harness as lh
import learner_mirror as mirror
import nstep_mirror as nm
import ring_rollout_harness as rr
from ring_rollout_harness import B, DONES, N, NTR, RINGS, T

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA
G32 = np.float32(GAMMA)
INF = float("inf")
STORES = lh.STORES


def _uav():
    import uavtrack
    return uavtrack


# ---- 1. the add against the mirror ---------------------------------------------------------------------------------------

def _new_ring(kind, cap, **kw):
    u = _uav()
    ring = (u.PrioritizedReplayRing if kind == "prioritised" else u.ReplayRing)(cap, DEV, seed=1, max_batch=64)
    return ring.with_nstep(**kw)


@pytest.mark.parametrize("ringcase", sorted(RINGS))
@pytest.mark.parametrize("done_kind", DONES)
@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_add_against_the_mirror_bitwise(kind, done_kind, ringcase):
    r = rr.rollout()
    done = rr.done(done_kind)
    cap, pos, count = RINGS[ringcase]
    longest = 0
    for gamma in (0.95, 1.0, 0.0):
        for n_step in (1, 2, 3, 5, 7, 9):
            ring = _new_ring(kind, cap, n_step=n_step, gamma=gamma)
            rr.prefill(ring, pos, count)
            img = rr.image(ring)
            ring.add_rollout(r["dev"]["obs_in"], rr.out(done))
            tr, m = nm.transitions(r["obs_in"], r["obs"], r["actions"], r["reward"], n_step, gamma, done,
                                   None if done is None else r["start_obs"])
            longest = max(longest, int(m.max()))
            p2, c2 = nm.ring_add(img, pos, count, tr)
            assert (ring.pos, ring.count) == (p2, c2)
            rr.same_image(rr.image(ring), img)
            if kind == "prioritised":
                assert (img["priorities"] == np.float32(2.5)).sum() >= min(NTR, cap)
    assert longest == T                                                # the longest window ran the whole rollout


# ---- 2. n = 1 is today's add ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ringcase", sorted(RINGS))
@pytest.mark.parametrize("done_kind", ["null", "zeros", "mid", "every"])
@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_n1_is_todays_add(kind, done_kind, ringcase):
    r = rr.rollout()
    done = rr.done(done_kind)
    cap, pos, count = RINGS[ringcase]
    new, old = _new_ring(kind, cap, n_step=1, gamma=GAMMA), _new_ring(kind, cap)
    assert old.discounts is None and new.discounts is not None
    rr.prefill(new, pos, count); rr.prefill(old, pos, count)
    new.add_rollout(r["dev"]["obs_in"], rr.out(done))
    old.add_rollout(r["dev"]["obs_in"], rr.out(done))      # uavtrack_replay_add_rollout_episodes, or _add_rollout without done
    a, b = rr.image(new), rr.image(old)
    rr.same_image(a, b, STORES + ("priorities",))
    assert (new.pos, new.count) == (old.pos, old.count)
    k = min(NTR, cap)
    written = np.zeros(cap, bool)
    written[(new.pos - k + np.arange(k)) % cap] = True
    d = a["discounts"].view(np.int32)
    assert (d[written] == G32.view(np.int32)).all() and (d[~written] == np.float32(7.0).view(np.int32)).all()


# ---- the learner ---------------------------------------------------------------------------------------------------------

SHAPES = [(1, 9, 1), (33, 12, 2), (64, 48, 63), (128, 12, 65), (128, 12, 4096)]
CASES = [(H, A, n, loss, gather) for H, A, n in SHAPES for loss in ("reference", "per_sample") for gather in (True, False)]


def _discount_store(cap, seed):
    """A per-slot store in [0, 1] with exact zeros and an exact one (cap 1: a single zero)."""
    return lh.make_weights(np.random.RandomState(seed + 101), cap) if cap > 1 else np.zeros(1, np.float32)


# ---- 3. gamma everywhere is nothing --------------------------------------------------------------------------------------

VARIANTS = ("plain", "weighted", "regularised", "diagnostics")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H,A,n,loss,gather", CASES)
def test_a_store_of_gamma_and_null_are_the_plain_update_bitwise(H, A, n, loss, gather, variant):
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    prio0 = torch.rand(cap, device=DEV) + 0.1
    w = lh.dev(lh.make_weights(np.random.RandomState(n + H), n)) if variant == "weighted" else None
    kw = {}
    if variant == "regularised":                                       # (the entropy bonus exists for per_sample only)
        kw = dict(c=0.01 if loss == "per_sample" else 0.0, mgn=(0.05, 0.5))
    if variant == "diagnostics":
        kw = dict(diag=True, mgn=(1e30, 1e30))
    full = torch.full((cap,), GAMMA, device=DEV)
    assert full.cpu().numpy().view(np.int32)[0] == G32.view(np.int32)
    modes = (dict(), dict(entry="discounted"), dict(d=full), dict(d=full, entry="discounted"))
    outs = []
    for mode in modes:
        L = lh.learner(H, A, loss, blob, max_batch=n, **kw)
        outs.append(lh.update(L, n, store, cap, it, prio0.clone(), w, **mode))
        L.check()
    assert np.isfinite(outs[0]["actor_loss"]) and np.array_equal(outs[0]["step"], np.ones(8))
    assert not np.array_equal(outs[0]["prio"], prio0.cpu().numpy())
    for other in outs[1:]:
        lh.same(outs[0], other)
    L = lh.learner(H, A, loss, blob, max_batch=n, **kw)
    rows = [lh.row(L, n, store, cap, it, w, **mode) for mode in modes]
    L.check()
    for row, td in rows[1:]:
        assert np.array_equal(row.view(np.int32), rows[0][0].view(np.int32)) and np.array_equal(td, rows[0][1])
    assert np.array_equal(rows[0][1], outs[0]["td"])


# ---- 4. random discounts against the fp64 mirror ---------------------------------------------------------------------------

PATHS = [(loss, path) for loss in ("reference", "per_sample") for path in ("plain", "weighted", "regularised")
         if not (path == "regularised" and loss == "reference")]


@pytest.mark.parametrize("loss,path", PATHS)
@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("H,A,n", SHAPES)
def test_random_discounts_against_fp64_mirror(H, A, n, gather, loss, path):
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    ds = _discount_store(cap, n + H)
    d = ds[idx]                                                         # the per-row discounts, through the index vector
    w = lh.make_weights(np.random.RandomState(n + H + 5), n) if path != "plain" else None
    c = 0.01 if path == "regularised" else None
    L = lh.learner(H, A, loss, blob, max_batch=n, c=c or 0.0)
    out = lh.update(L, n, store, cap, it, None, None if w is None else lh.dev(w), lh.dev(ds))
    L.check()
    opts = dict(weights=w, entropy_coef=0.0 if c is None else np.float32(c))
    ref = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), d, loss, **opts)
    ral, rcl, rtd, g = ref[:4]
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ral, rcl, rtd)
    lh.assert_step_from_zero(out, blob, g, n, H, A)
    # rows with d = 0 do not bootstrap: td_delta = r - V(s), within the same bound
    zero = d == 0
    assert zero.any() or n < 63
    if zero.any():
        r0 = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), np.zeros(n), loss, **opts).td
        assert np.array_equal(r0[zero], rtd[zero])
        np.testing.assert_allclose(out["td"][zero], r0[zero], rtol=0, atol=2e-5 * (np.abs(rtd).max() + 1e-6))
    if n >= 63:       # the discounts are in the result: gamma for every row is far outside the bound
        gu = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), np.full(n, GAMMA), loss, **opts).grad
        assert np.abs(out["exp_avg"] / 0.1 - gu).max() > 100 * lh.tol_g(n, g)


def test_the_discount_is_per_slot_and_the_weight_per_batch_row():
    """A gathered batch whose index vector is a reversal: the discounts follow the slots, the weights the batch rows."""
    H, A, n = 64, 12, 63
    blob, b, store, cap, _, _ = lh.case(H, A, n, False)
    idx = np.arange(n)[::-1].copy()
    ds, w = _discount_store(cap, 3), lh.make_weights(np.random.RandomState(4), n)
    L = lh.learner(H, A, "per_sample", blob, max_batch=n)
    out = lh.update(L, n, store, cap, lh.dev(idx), None, lh.dev(w), lh.dev(ds))
    L.check()
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), ds[idx], "per_sample", weights=w)[:4]
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ral, rcl, rtd)
    lh.assert_step_from_zero(out, blob, g, n, H, A)


# ---- 5. the split form ---------------------------------------------------------------------------------------------------

SPLIT = [(64, 48, 63), (128, 12, 65), (128, 12, 4096)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n", SPLIT)
def test_grad_apply_write_is_the_discounted_update_bitwise(H, A, n, loss, weighted):
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    ds = lh.dev(_discount_store(cap, n))
    w = lh.dev(lh.make_weights(np.random.RandomState(n), n)) if weighted else None
    prio0 = torch.rand(cap, device=DEV) + 0.1
    closed = lh.learner(H, A, loss, blob, max_batch=n)
    want = lh.update(closed, n, store, cap, it, prio0.clone(), w, ds)
    split = lh.learner(H, A, loss, blob, max_batch=n)
    prio = prio0.clone()
    row, td = split._grad(n, store, cap, it, None, None, w, ds)
    al, cl = split.apply(row)
    split.write_priorities(types.SimpleNamespace(priorities=prio, capacity=cap), it, td)
    split.check(); closed.check()
    assert not np.array_equal(want["prio"], prio0.cpu().numpy())
    lh.same(dict(lh.state(split), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy(), td=td.cpu().numpy(),
               prio=prio.cpu().numpy()), want)


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n", SPLIT)
def test_a_row_with_discounts_and_a_row_without_apply_together(H, A, n, loss):
    """Two gradient rows over the two halves of a batch, the first with a discount store and the second through the
    plain uavtrack_learner_grad (gamma in the mirror), against the mirror on the whole batch."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    ds = _discount_store(cap, n + 1)
    h = n // 2
    L = lh.learner(H, A, loss, blob, max_batch=n)
    rows = L.new_rows(2)
    _, td0 = L._grad(h, store, cap, it[:h], rows[0], None, None, lh.dev(ds))
    _, td1 = L._grad(n - h, store, cap, it[h:].contiguous(), rows[1])
    al, cl = L.apply(rows)
    L.check()
    d = np.concatenate([ds[idx[:h]].astype(np.float64), np.full(n - h, float(G32))])
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), d, loss)[:4]
    lh.assert_losses_and_td(al.cpu().numpy(), cl.cpu().numpy(), torch.cat([td0, td1]).cpu().numpy(), ral, rcl, rtd)
    lh.assert_step_from_zero(lh.state(L), blob, g, n, H, A)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("nan"), -0.1, 1.5], ids=["nan", "negative", "above-one"])
def test_a_bad_discount_refuses_the_update(bad):
    H, A, n = 128, 12, 65
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    L = lh.learner(H, A, "reference", blob, max_batch=n)
    good = lh.dev(_discount_store(cap, 3))
    good[int(idx[0])], good[int(idx[1])] = 1.0, 0.0                     # both ends of the range are accepted
    L._run(n, store, cap, it, None, None, good)
    L.check()
    before = lh.state(L)
    prio = torch.rand(cap, device=DEV) + 0.1
    prio0 = prio.clone()
    d = good.clone()
    d[int(idx[40])] = bad                                               # a slot the second tile of the batch gathers
    al, cl, _ = L._run(n, store, cap, it, prio, None, d)
    assert torch.isnan(al) and torch.isnan(cl)
    lh.same(lh.state(L), before)
    assert torch.equal(prio, prio0)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    L.check()                                                          # the count restarts
    # the split form: the row carries status 8, the apply of it changes nothing, the priority write is held back
    row, td = L._grad(n, store, cap, it, None, None, None, d)
    assert int(row.cpu().numpy().view(np.int32)[L.num_params + 6]) == 8
    ok_row, _ = L._grad(n, store, cap, it)
    al, cl = L.apply(torch.stack([ok_row, row]))
    L.write_priorities(types.SimpleNamespace(priorities=prio, capacity=cap), it, td)
    assert torch.isnan(al) and torch.isnan(cl)
    lh.same(lh.state(L), before)
    assert torch.equal(prio, prio0)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    # a bad discount in a slot the batch does not gather is not read
    unused = np.setdiff1d(np.arange(cap), idx)
    d = good.clone()
    d[int(unused[0])] = bad
    al, cl, _ = L._run(n, store, cap, it, prio, None, d)
    L.check()
    assert torch.isfinite(al) and torch.isfinite(cl) and not torch.equal(prio, prio0)
    assert np.array_equal(lh.state(L)["step"], before["step"] + 1)


def test_a_row_with_the_wrong_tag_is_still_refused():
    """The finalize kernel's "another layout" flag moved from 8 to 16: a row whose tag is not P refuses the apply, alone
    and beside a good row, and so does a row whose n is 0."""
    H, A, n = 64, 12, 63
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    L = lh.learner(H, A, "reference", blob, max_batch=n)
    before = lh.state(L)
    good, _ = L._grad(n, store, cap, it, None, None, None, lh.dev(_discount_store(cap, 1)))
    P = L.num_params
    for word, value in ((P + 7, P + 1), (P + 4, 0)):
        bad = good.clone()
        bad.view(torch.int32)[word] = value
        for rows in (bad, torch.stack([good, bad])):
            al, cl = L.apply(rows)
            assert torch.isnan(al) and torch.isnan(cl)
            lh.same(lh.state(L), before)
            with pytest.raises(RuntimeError, match="1 update"):
                L.check()
    al, cl = L.apply(good)
    L.check()
    assert torch.isfinite(al) and np.array_equal(lh.state(L)["step"], np.ones(8))


def test_host_side_errors_of_the_add_enqueue_nothing():
    from uavtrack import _lib
    lib = _lib.load()
    r = rr.rollout()["dev"]
    done = lh.dev(rr.done("mid"))
    ring = _new_ring("prioritised", 100, n_step=3, gamma=GAMMA)
    rr.prefill(ring, 10, 10)
    torch.cuda.synchronize()
    img = rr.image(ring)
    p = _lib.ptr
    off = lambda t: C.c_void_p(t.data_ptr() + 4)                       # not 16-byte aligned

    def call(ring_struct=None, discounts=p(ring.discounts), obs_in=p(r["obs_in"]), obs=p(r["obs"]), act=p(r["actions"]),
             rew=p(r["reward"]), dn=p(done), so=p(r["start_obs"]), n_step=3, gamma=GAMMA, steps=T, envs=B, n_uav=N):
        rs = ring._ring() if ring_struct is None else ring_struct
        return lib.uavtrack_replay_add_rollout_nstep(ring._h, C.byref(rs), discounts, steps, envs, n_uav, obs_in, obs, act,
                                                     rew, dn, so, n_step, gamma, ring._stream())

    def ring_with(**kw):
        rs = ring._ring()
        for k, v in kw.items():
            setattr(rs, k, v)
        return rs

    bad_calls = {
        "discounts": dict(discounts=None), "obs_in, obs": dict(obs=None), "obs_in": dict(obs_in=None),
        "actions": dict(act=None), "reward": dict(rew=None),
        "n_step = 0": dict(n_step=0), "n_step = 65": dict(n_step=65),
        "gamma": dict(gamma=float("nan")), "gamma = -0.1": dict(gamma=-0.1), "gamma = 1.5": dict(gamma=1.5),
        "gamma = inf": dict(gamma=INF),
        "both": dict(dn=None), "both be": dict(so=None),
        "pos": dict(ring_struct=ring_with(pos=100)), "capacity": dict(ring_struct=ring_with(capacity=101)),
        "count": dict(ring_struct=ring_with(count=101)), "ring's": dict(ring_struct=ring_with(states=None)),
        "aligned": dict(obs=off(r["obs"])), "16-byte": dict(so=off(r["start_obs"])),
        "16-byte aligned": dict(ring_struct=ring_with(next_states=ring.store["next_states"].data_ptr() + 4)),
        "steps": dict(steps=0),
    }
    for word, kw in bad_calls.items():
        assert call(**kw) != 0, word
        msg = lib.uavtrack_last_error().decode()
        assert msg.startswith("uavtrack_replay_add_rollout_nstep: ") and word.split(" =")[0] in msg, (word, msg)
    torch.cuda.synchronize()
    rr.same_image(rr.image(ring), img)
    assert call() == 0                                                  # and the good call goes through
    torch.cuda.synchronize()
    assert rr.image(ring)["rewards"].tobytes() != img["rewards"].tobytes()


@pytest.mark.parametrize("fn", ["update", "grad"])
def test_host_side_errors_of_the_discounted_calls_enqueue_nothing(fn):
    from uavtrack import _lib
    H, A, n = 64, 12, 63
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    L = lh.learner(H, A, "reference", blob, max_batch=n)
    name = f"uavtrack_learner_{fn}_discounted"
    ds = lh.dev(_discount_store(cap, 2))
    losses, td, row = torch.empty(2, device=DEV), torch.zeros(n, device=DEV), torch.zeros(L.row_floats, device=DEV)
    prio = torch.rand(cap, device=DEV) + 0.1
    prio0 = prio.clone()
    before = lh.state(L)
    p = _lib.ptr

    def call(n_=n, states=p(store["states"]), cap_=cap, idx_=p(it), out0=p(losses[0:1]), td_=p(td), row_=p(row)):
        head = (L._h, n_, states, p(store["actions"]), p(store["rewards"]), p(store["next_states"]), cap_, idx_, None, p(ds))
        if fn == "update":
            return L._lib.uavtrack_learner_update_discounted(*head, out0, p(losses[1:2]), td_, p(prio), L._stream())
        return L._lib.uavtrack_learner_grad_discounted(*head, td_, row_, L._stream())

    bad_calls = [dict(states=None), dict(n_=0), dict(n_=n + 1), dict(cap_=0), dict(n_=n, idx_=None, cap_=n - 1)]
    bad_calls += [dict(out0=None)] if fn == "update" else [dict(td_=None), dict(row_=None)]
    for kw in bad_calls:
        assert call(**kw) != 0, kw
        assert L._lib.uavtrack_last_error().decode().startswith(name + ": "), kw
    L.check()
    lh.same(lh.state(L), before)
    assert torch.equal(prio, prio0) and not td.any() and not row.any()
    assert call() == 0
    L.check()


# ---- 7. the Python surface -------------------------------------------------------------------------------------------------

def _filled_ring(kind, data, seed, k, n_step=3, gamma=GAMMA, dseed=1):
    """An n-step ring holding `data` through add(), with a random discount store, and (prioritised) random priorities."""
    n = len(data[1])
    ring = (_uav().PrioritizedReplayRing if kind == "prioritised" else _uav().ReplayRing)(
        n + 50, DEV, seed=seed, max_batch=k).with_nstep(n_step, gamma)
    tr = {key: torch.from_numpy(x) for key, x in zip(STORES, data)}
    tr["discounts"] = torch.from_numpy(_discount_store(n, dseed))
    ring.add(tr)
    if kind == "prioritised":
        ring.priorities[:n] = lh.dev(np.random.RandomState(dseed).uniform(0.1, 2.0, n).astype(np.float32))
    return ring


def test_ring_arguments_and_the_gamma_check():
    u = _uav()
    for cls in (u.ReplayRing, u.PrioritizedReplayRing):
        plain = cls(64, DEV)
        with pytest.raises(ValueError, match="gamma"):
            plain.with_nstep(3)
        with pytest.raises(ValueError, match="n_step"):
            plain.with_nstep(65, gamma=0.9)
        with pytest.raises(ValueError, match="gamma"):
            plain.with_nstep(1, gamma=1.5)
        assert plain.with_nstep() is plain
        assert plain.discounts is None and plain.n_step == 1 and plain.gamma is None
        assert "discounts" not in (plain.sample(4) if cls is u.ReplayRing else plain.sample(4)[0])
    data = lh.batch(np.random.RandomState(1), 300, 12)
    ring = _filled_ring("uniform", data, 3, 100, gamma=0.9)
    L = lh.learner(64, 12, "reference", lh.init_blob(64, 12, 1), max_batch=100)
    before = lh.state(L)
    for call in (lambda: L.update_from(ring, 100), lambda: L.grad_from(ring, 100), lambda: L.update_from_many([ring], 100)):
        with pytest.raises(ValueError, match=r"0\.9\b.*0\.95\b"):
            call()
    lh.same(lh.state(L), before)
    L9 = lh.learner(64, 12, "reference", lh.init_blob(64, 12, 1), max_batch=100, gamma=0.9)
    L9.update_from(ring, 100)
    L9.check()


@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_add_fills_the_discounts_and_sample_carries_them(kind):
    n = 300
    data = lh.batch(np.random.RandomState(2), n, 12)
    ring = _filled_ring(kind, data, 3, 100)
    ds = _discount_store(n, 1)
    assert np.array_equal(ring.discounts[:n].cpu().numpy(), ds)
    # without a "discounts" entry the slots get float32(gamma); a wrapping add fills both pieces
    more = {key: torch.from_numpy(x[:80]) for key, x in zip(STORES, data)}
    ring.add(more)
    got = ring.discounts.cpu().numpy()
    assert (got[n:n + 50] == G32).all() and (got[:30] == G32).all() and np.array_equal(got[30:n], ds[30:])
    assert ring.pos == 30 and ring.count == n + 50
    s = ring.sample(64)
    tr, idx = (s, None) if kind == "uniform" else (s[0], s[1])
    assert set(tr) == set(STORES) | {"discounts"} and tr["discounts"].shape == (64,)
    if idx is not None:
        assert torch.equal(tr["discounts"], ring.discounts[idx]) and torch.equal(tr["rewards"], ring.store["rewards"][idx])
    empty = _uav().ReplayRing(8, DEV).with_nstep(1, GAMMA).sample(4)
    assert empty["discounts"].numel() == 0


@pytest.mark.parametrize("importance", [False, True])
@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_update_from_and_grad_from_are_draw_discounted_call_write(kind, importance):
    H, A, n, k = 128, 12, 3000, 1000
    data = lh.batch(np.random.RandomState(21), n, A)
    blob = lh.init_blob(H, A, 21)
    one, ring = lh.learner(H, A, "per_sample", blob, max_batch=k), _filled_ring(kind, data, 17, k)
    two, twin = lh.learner(H, A, "per_sample", blob, max_batch=k), _filled_ring(kind, data, 17, k)
    imp = importance and kind == "prioritised"
    for u in range(3):
        if u < 2:
            al, cl, td = one.update_from(ring, k, beta=0.4, importance=importance)
        else:                                                           # the split path through grad_from
            row, td, gidx = one.grad_from(ring, k, importance=importance, beta=0.4)
            al, cl = one.apply(row)
            one.write_priorities(ring, gidx, td)
        if kind == "prioritised":
            idx, w = twin.draw(k, 0.4)
        else:
            idx, w = twin.draw(k), None
        out = lh.update(two, k, twin.store, twin.capacity, idx, twin.priorities, w if imp else None, twin.discounts,
                      entry="discounted")
        assert np.array_equal(al.cpu().numpy(), out["actor_loss"]) and np.array_equal(cl.cpu().numpy(), out["critic_loss"])
        assert np.array_equal(td.cpu().numpy(), out["td"]) and np.isfinite(out["actor_loss"]), u
        assert torch.equal(ring._idx[:k], idx)
        if kind == "prioritised":
            assert torch.equal(ring.priorities, twin.priorities)
    lh.same(lh.state(one), lh.state(two))
    for x in (one, two, ring, twin):
        x.check()
    # the discounts are in the result: the same draws from a ring without them end elsewhere
    three = lh.learner(H, A, "per_sample", blob, max_batch=k)
    third = _filled_ring(kind, data, 17, k)
    third.discounts = None
    for u in range(3):
        three.update_from(third, k, beta=0.4, importance=importance)
    assert not np.array_equal(lh.state(three)["params"], lh.state(one)["params"])


def test_update_from_many_over_two_nstep_rings():
    H, A, k = 128, 12, 600
    blob = lh.init_blob(H, A, 23)
    datas = [lh.batch(np.random.RandomState(30 + j), 900 + 100 * j, A) for j in range(2)]
    kinds = ("prioritised", "uniform")
    rings = [_filled_ring(kd, d, 40 + j, k, dseed=j) for j, (kd, d) in enumerate(zip(kinds, datas))]
    twins = [_filled_ring(kd, d, 40 + j, k, dseed=j) for j, (kd, d) in enumerate(zip(kinds, datas))]
    L, M = lh.learner(H, A, "reference", blob, max_batch=k), lh.learner(H, A, "reference", blob, max_batch=k)
    al, cl, tds = L.update_from_many(rings, k)
    rows = M.new_rows(2)
    drawn = []
    for j, t in enumerate(twins):
        idx = t.draw(k, 0.4)[0] if kinds[j] == "prioritised" else t.draw(k)
        from uavtrack import _lib
        td = torch.empty(k, device=DEV)
        _lib.check(M._lib.uavtrack_learner_grad_discounted(
            M._h, k, *M._batch_args(t.store, t.capacity, idx), None, _lib.ptr(t.discounts), _lib.ptr(td),
            _lib.ptr(rows[j]), M._stream()), "uavtrack_learner_grad_discounted")
        drawn.append((idx, td))
    al2, cl2 = M.apply(rows)
    for t, (idx, td) in zip(twins, drawn):
        M.write_priorities(t, idx, td)
    L.check(); M.check()
    assert torch.equal(al, al2) and torch.equal(cl, cl2) and torch.isfinite(al)
    for a, (_, td) in zip(tds, drawn):
        assert torch.equal(a, td)
    lh.same(lh.state(L), lh.state(M))
    assert torch.equal(rings[0].priorities, twins[0].priorities)


# ---- 8. graph --------------------------------------------------------------------------------------------------------------

def test_add_and_update_captured_and_replayed_equal_eager():
    """add_rollout (n_step = 3) + update_from on one linear stream, captured once and replayed three times == three eager
    iterations, bitwise.  The ring's host-side pos and count are frozen into the capture, so every eager iteration
    starts its add from the same pos and count as the captured one."""
    H, A, k = 64, 12, 32
    r = rr.rollout()
    out = rr.out(rr.done("mid"))
    blob = lh.init_blob(H, A, 42)

    def fresh():
        ring = _new_ring("prioritised", 100, n_step=3, gamma=GAMMA)      # empty: every drawn slot is one the add wrote
        return lh.learner(H, A, "reference", blob, max_batch=k), ring

    eager, re_ = fresh()
    graphed, rg = fresh()

    def iteration(L, ring):
        ring.pos, ring.count = 0, 0                                     # every iteration enqueues the same add
        ring.add_rollout(r["dev"]["obs_in"], out)
        return L.update_from(ring, k, importance=True, beta=0.4)

    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = iteration(graphed, rg)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(graphed)["step"], np.zeros(8))           # capture ran nothing
    for c in range(3):
        e_out = iteration(eager, re_)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y) and torch.isfinite(x).all(), c
        assert np.array_equal(graphed._get_params(), eager._get_params()), c
        a, b = rr.image(rg), rr.image(re_)
        for key in a:                                                   # the written slots: the rest was never initialised
            assert a[key][:NTR].tobytes() == b[key][:NTR].tobytes(), key
    lh.same(lh.state(graphed), lh.state(eager))
    assert np.array_equal(lh.state(graphed)["step"], np.full(8, 3))
    for x in (graphed, eager, re_, rg):
        x.check()


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_a_real_rollout_across_episode_ends(kind):
    """3 envs x 5 UAVs x 3 targets, horizon 4, one fused launch of 10 steps with automatic reset: episode ends at t = 3 and
    t = 7, and the rollout's tail cuts the third episode.  add_rollout with n_step = 3 equals the mirror on the launch's
    own tensors, bitwise."""
    u = _uav()
    cfg = u.EnvConfig(n_envs=3, n_uav=5, m_targets=3, horizon=4)
    env = u.BatchedUavEnv(cfg, DEV)
    torch.manual_seed(3)
    actor = u.ActorMLP(hidden_dim=32, action_dim=cfg.na_total)
    ro = u.BatchedRollout(env, actor, device_actor=True, seed=3, auto_reset_seed=11)
    ro.reset(seed=5)
    obs_in = ro.obs.clone()
    res = ro.run_fused(10)
    host = {key: res[key].cpu().numpy() for key in ("obs", "actions", "reward", "done", "start_obs")}
    assert host["done"][3].all() and host["done"][7].all() and host["done"].sum() == 6
    ring = _new_ring(kind, 400, n_step=3, gamma=GAMMA)
    rr.prefill(ring, 20, 20)
    img = rr.image(ring)
    ring.add_rollout(obs_in, res)
    tr, m = nm.transitions(obs_in.cpu().numpy(), host["obs"], host["actions"], host["reward"], 3, GAMMA, host["done"],
                           host["start_obs"])
    assert m[:, 0].tolist() == [3, 3, 2, 1, 3, 3, 2, 1, 2, 1]
    p2, c2 = nm.ring_add(img, 20, 20, tr)
    assert (ring.pos, ring.count) == (p2, c2) == (170, 170)
    rr.same_image(rr.image(ring), img)
    # the learner trains from it (a ring of its own: the prefilled slots above hold sentinels, no transitions)
    fresh = _new_ring(kind, 400, n_step=3, gamma=GAMMA)
    fresh.add_rollout(obs_in, res)
    assert fresh.count == 150 and torch.equal(fresh.discounts[:150], ring.discounts[20:170])
    L = lh.learner(32, cfg.na_total, "reference", max_batch=64)
    al, cl, _ = L.update_from(fresh, 64)
    L.check()
    assert torch.isfinite(al) and torch.isfinite(cl)
    env.close()


# ---- 10. the example -------------------------------------------------------------------------------------------------------

def test_example_trains_on_n_step_targets(capsys):
    """examples/train_maac.py --n-step 3: both learners, both device rings and --shards train; with the PyTorch buffer of
    --replay uniform it exits with a message naming the two ring options."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_maac
    common = ["--envs", "64", "--steps", "20", "--iters", "2", "--batch", "4096", "--updates", "2", "--n-step", "3"]
    for extra in (["--replay", "prioritized", "--learner", "device", "--publish", "device"],
                  ["--replay", "uniform-device", "--learner", "torch"],
                  ["--replay", "prioritized", "--learner", "torch", "--importance"],
                  ["--replay", "uniform-device", "--learner", "device", "--shards", "2"]):
        hist = train_maac.main(common + extra)
        assert len(hist) == 2 and np.isfinite(hist).all(), extra
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == 2 and all(np.isfinite(float(ln.split("critic loss")[1].split()[0])) for ln in lines), extra
    with pytest.raises(SystemExit):
        train_maac.main(common + ["--replay", "uniform"])
    err = capsys.readouterr().err
    assert "--replay prioritized" in err and "uniform-device" in err
