"""Off-policy correction on the MI355X: the actor alone (uavtrack_learner_log_probs, _log_probs_window) against the
float64 mirror (tests/offpolicy_mirror.py) and bitwise against itself wherever a row is placed; the truncated ratios
(uavtrack_learner_ratio_weights) against the mirror; update_from(ring, k, rho_bar=) on-policy as the plain update to the
bit, off-policy as draw + ratio weights + the weighted update called one by one; the behaviour store behind every add
form; refusals; the split update; one captured graph; and everything unchanged while rho_bar is None.  Built on
tests/learner_harness.py; every bound holds for every row."""
import numpy as np
import pytest
import torch

import learner_harness as lh
import offpolicy_mirror as om
from uavtrack.replay import DrawSpec

pytestmark = pytest.mark.gpu

DEV = lh.DEV
CASES = [(1, 9, 1), (33, 12, 2), (128, 12, 513), (256, 48, 4097)]        # (H, A, n)
CAP = 257                                                                # the rings of tests 4 to 10
T, B, N = 3, 4, 5                                                        # their rollouts: 60 transitions an add


def _uav():
    import uavtrack
    return uavtrack


def _sharp(blob, H, A):
    """The same blob with the actor's fc2.weight x 30: logits near +-35, log p down to -60."""
    b = np.array(blob, np.float32)
    b[13 * H:13 * H + A * H] *= np.float32(30)
    return b


_stores = {}


def _store(H, A, n):
    """(blob, host states, host actions, device store, capacity, host indices, device indices): a store 7 slots larger
    than the batch, shared by the tests."""
    key = (H, A, n)
    if key not in _stores:
        rng = np.random.RandomState(31 * H + n)
        cap = n + 7
        s, a, r, s2 = lh.batch(rng, cap, A)
        idx = rng.randint(0, cap, size=n).astype(np.int64)
        store = {k: lh.dev(x) for k, x in zip(lh.STORES, (s, a, r, s2))}
        _stores[key] = (lh.init_blob(H, A, H + n), s, a, store, cap, idx, lh.dev(idx))
    return _stores[key]


def _log_probs_at(L, store, cap, n, idx):
    """uavtrack_learner_log_probs itself, with an index vector."""
    from uavtrack import _lib
    out = torch.full((n,), 7.0, device=DEV)
    _lib.check(L._lib.uavtrack_learner_log_probs(L._h, n, _lib.ptr(store["states"]), _lib.ptr(store["actions"]), cap,
                                                 _lib.ptr(idx), _lib.ptr(out), L._stream()), "uavtrack_learner_log_probs")
    return out


def _ratio(L, n, store, log_mu, cap, idx, rho_bar, w_in, w_out, rho_out):
    """uavtrack_learner_ratio_weights itself."""
    from uavtrack import _lib
    _lib.check(L._lib.uavtrack_learner_ratio_weights(
        L._h, n, _lib.ptr(store["states"]), _lib.ptr(store["actions"]), _lib.ptr(log_mu), cap, _lib.ptr(idx),
        float(rho_bar), _lib.ptr(w_in), _lib.ptr(w_out), _lib.ptr(rho_out), L._stream()), "uavtrack_learner_ratio_weights")


def _bits(t):
    return t.cpu().numpy().tobytes()


# ---- 1. log_probs against the mirror -----------------------------------------------------------------------------------

@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("H,A,n", CASES)
def test_log_probs_against_the_fp64_mirror_in_both_addressing_modes(H, A, n, sharp):
    blob, s, a, store, cap, idx, idx_d = _store(H, A, n)
    if sharp:
        blob = _sharp(blob, H, A)
    L = lh.learner(H, A, "per_sample", blob, max_batch=64)                 # n is not limited by max_batch
    before = lh.state(L)
    want_all = om.log_probs(blob, H, A, s, a)
    bound_all = om.log_prob_bound(blob, H, A, s)
    got = {"batch order, no indices": (L.log_probs(store["states"][:n], store["actions"][:n]).cpu().numpy(), np.arange(n)),
           "batch order, indices": (_log_probs_at(L, store, cap, n, idx_d).cpu().numpy(), idx)}
    first = cap - 3                                                        # the window wraps (where n > 3)
    log_mu = torch.full((cap,), float("nan"), device=DEV)
    L.log_probs_window(store["states"], store["actions"], first, n, log_mu)
    slots = (first + np.arange(n)) % cap
    lm = log_mu.cpu().numpy()
    assert np.isnan(np.delete(lm, slots)).all()                            # nothing outside the window is written
    got["ring window"] = (lm[slots], slots)
    lh.same(lh.state(L), before)
    if sharp and n > 100:
        assert want_all.min() < -30
    for what, (dev, rows) in got.items():
        assert dev.dtype == np.float32 and np.isfinite(dev).all() and (dev <= 0).all()
        err, bound = np.abs(dev.astype(np.float64) - want_all[rows]), bound_all[rows]
        print(f"H = {H}, A = {A}, n = {n}, {'sharp' if sharp else 'default'} actor, {what}: share of the bound "
              f"{(err / bound).max():.3f}")
        assert (err <= bound).all(), (what, (err / bound).max())


def test_log_probs_takes_any_leading_shape_and_writes_out_in_place():
    H, A, n = 33, 12, 2
    blob, s, a, store, cap, _, _ = _store(H, A, n)
    L = lh.learner(H, A, "per_sample", blob)
    st, ac = store["states"][:6].contiguous(), store["actions"][:6].contiguous()
    flat = L.log_probs(st, ac)
    assert flat.shape == (6,) and flat.dtype == torch.float32
    out = torch.full((2, 3), 7.0, device=DEV)
    assert L.log_probs(st.reshape(2, 3, 12), ac.reshape(2, 3), out=out) is out and _bits(out) == _bits(flat)
    bad = ac.clone()
    bad[1], bad[4] = -1, A                                                 # an action outside [0, A): NaN for that row alone
    got = L.log_probs(st, bad).cpu().numpy()
    assert np.isnan(got[[1, 4]]).all() and got[[0, 2, 3, 5]].tobytes() == flat.cpu().numpy()[[0, 2, 3, 5]].tobytes()
    far = lh.dev(np.array([0, cap, -1, 2], np.int64))                      # a slot outside the store: NaN likewise
    got = _log_probs_at(L, store, cap, 4, far).cpu().numpy()
    assert np.isnan(got[[1, 2]]).all() and np.isfinite(got[[0, 3]]).all()
    with pytest.raises(ValueError, match="actions must be"):
        L.log_probs(st, ac.to(torch.int64))
    with pytest.raises(ValueError, match="states must be"):
        L.log_probs(st.double(), ac)
    with pytest.raises(RuntimeError, match="window"):
        L.log_probs_window(st, ac, 0, 7, torch.empty(6, device=DEV))        # n > capacity
    with pytest.raises(RuntimeError, match="first"):
        L.log_probs_window(st, ac, 6, 1, torch.empty(6, device=DEV))


# ---- 2. placement independence -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A", [(128, 12), (256, 48)])
def test_a_rows_bits_do_not_depend_on_the_launch_that_carries_it(H, A):
    n = 4097
    blob, s, a, store, cap, _, _ = _store(H, A, n)
    L = lh.learner(H, A, "per_sample", _sharp(blob, H, A))
    st, ac = store["states"], store["actions"]
    whole = L.log_probs(st[:n], ac[:n])
    parts = torch.empty(n, device=DEV)
    q = n // 4
    for lo, hi in ((0, q), (q, 2 * q), (2 * q, 3 * q), (3 * q, 4 * q), (4 * q, n)):      # four quarters and the ragged tail
        L.log_probs(st[lo:hi], ac[lo:hi], out=parts[lo:hi])
    assert _bits(parts) == _bits(whole)
    single = torch.stack([L.log_probs(st[i:i + 1], ac[i:i + 1])[0] for i in (0, 255, 256, 511, 512, 4096)])
    assert _bits(single) == _bits(whole[[0, 255, 256, 511, 512, 4096]])
    for first in (0, 1000):                                                 # the window mode over the whole store
        log_mu = torch.full((cap,), float("nan"), device=DEV)
        L.log_probs_window(st, ac, first, cap, log_mu)
        assert _bits(log_mu[:n]) == _bits(whole), first


# ---- 3. the ratios ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("H,A,n", CASES[1:])
def test_ratio_weights_against_the_mirror(H, A, n, sharp):
    blob, s, a, store, cap, idx, idx_d = _store(H, A, n)
    if sharp:
        blob = _sharp(blob, H, A)
    L = lh.learner(H, A, "per_sample", blob)
    rng = np.random.RandomState(n)
    lp_all = om.log_probs(blob, H, A, s, a)
    log_mu = np.minimum(lp_all + rng.uniform(-1.5, 1.5, size=cap), 0.0).astype(np.float32)
    log_mu[::5] = -80.0
    log_mu_d = lh.dev(log_mu)
    b = om.log_prob_bound(blob, H, A, s)[idx]
    w_in = rng.uniform(0, 1, size=n).astype(np.float32)
    w_in_d = lh.dev(w_in)
    for rho_bar in (1.0, 2.5, float("inf")):
        _, rho64 = om.weights(blob, H, A, s[idx], a[idx], log_mu[idx], rho_bar)
        w_out, rho = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        _ratio(L, n, store, log_mu_d, cap, idx_d, rho_bar, w_in_d, w_out, rho)
        got = rho.cpu().numpy()
        err, bound = np.abs(got.astype(np.float64) - rho64), om.ratio_bound(rho64, b)
        print(f"H = {H}, A = {A}, n = {n}, {'sharp' if sharp else 'default'} actor, rho_bar = {rho_bar}: share of the "
              f"bound {(err / bound).max():.3f}, {np.mean(got == np.float32(rho_bar)):.2f} of the rows at the cap")
        assert np.isfinite(got).all() and (err <= bound).all(), (err / bound).max()
        far = log_mu[idx] == -80.0
        assert n < 100 or (far.any() and not far.all())
        if np.isfinite(rho_bar):
            assert (got[far] == np.float32(rho_bar)).all()
        assert _bits(w_out) == _bits(w_in_d * rho)                          # out of place
        in_place = w_in_d.clone()
        _ratio(L, n, store, log_mu_d, cap, idx_d, rho_bar, in_place, in_place, None)
        assert _bits(in_place) == _bits(w_out)
        ones = torch.empty(n, device=DEV)
        _ratio(L, n, store, log_mu_d, cap, idx_d, rho_bar, None, ones, None)          # no weights_in: the factor 1.0f
        assert _bits(ones) == _bits(rho)


# ---- the rings of tests 4 to 10 ------------------------------------------------------------------------------------------

_rolls = {}


def _rollout(seed, steps=T, episodes=False, A=12):
    key = (seed, steps, episodes)
    if key not in _rolls:
        rng = np.random.default_rng(1000 + seed)
        obs_in = lh.dev(rng.uniform(-1, 1, (B, N, 12)).astype(np.float32))
        out = {"obs": lh.dev(rng.uniform(-1, 1, (steps, B, N, 12)).astype(np.float32)),
               "actions": lh.dev(rng.integers(0, A, (steps, B, N)).astype(np.int32)),
               "reward": lh.dev(rng.uniform(-2, 2, (steps, B, N)).astype(np.float32))}
        if episodes:
            out["done"] = lh.dev((rng.random((steps, B)) < 0.3).astype(np.uint8))
            out["start_obs"] = lh.dev(rng.uniform(-1, 1, (steps, B, N, 12)).astype(np.float32))
        _rolls[key] = (obs_in, out)
    return _rolls[key]


def _ring(kind, behaviour, lam=None, cap=CAP, max_batch=64, seed=3):
    u = _uav()
    ring = (u.PrioritizedReplayRing if kind == "prioritised" else u.ReplayRing)(cap, DEV, seed=seed, max_batch=max_batch)
    if lam is not None:
        ring.with_lambda(*lam)
    return ring.with_behaviour() if behaviour else ring


def _fill(ring, L, adds=5):
    """`adds` rollouts of 60 transitions: past the ring's 257 slots from the fifth on."""
    for k in range(adds):
        obs_in, out = _rollout(k)
        kw = dict(critic=L) if ring.lam is not None else {}
        if ring.log_mu is not None:
            ring.add_rollout_behaviour(obs_in, out, behaviour=L, **kw)
        else:
            ring.add_rollout(obs_in, out, **kw)
    assert ring.count == min(ring.capacity, adds * T * B * N)


def _outcome(L, ring, res):
    al, cl, td = res
    return dict(lh.state(L), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy(), td=td.cpu().numpy(),
                prio=None if ring.priorities is None else ring.priorities.cpu().numpy())


H0, A0 = 64, 12


def _twins(loss="per_sample"):
    blob = lh.init_blob(H0, A0, 77)
    return lh.learner(H0, A0, loss, blob, max_batch=64), lh.learner(H0, A0, loss, blob, max_batch=64), blob


# ---- 4. on-policy: rho = 1 exactly, the plain update's bits --------------------------------------------------------------

@pytest.mark.parametrize("kind,importance,lam,loss", [("uniform", False, None, "per_sample"),
                                                      ("prioritised", True, None, "per_sample"),
                                                      ("prioritised", False, None, "reference"),
                                                      ("uniform", False, (0.9, 0.95), "per_sample")])
def test_on_policy_the_corrected_update_is_the_plain_update_bit_for_bit(kind, importance, lam, loss):
    L1, L2, _ = _twins(loss)
    r1, r2 = _ring(kind, True, lam), _ring(kind, False, lam)
    assert r2.log_mu is None
    _fill(r1, L1)
    _fill(r2, L2)
    assert torch.isfinite(r1.log_mu).all()
    rho = torch.empty(63, device=DEV)
    for rho_bar in (1.0, float("inf")):
        got = _outcome(L1, r1, L1.update_from(r1, 63, importance=importance, rho_bar=rho_bar, rho_out=rho))
        want = _outcome(L2, r2, L2.update_from(r2, 63, importance=importance))
        L1.check(); L2.check()
        assert (rho == 1.0).all()
        lh.same(got, want, rho_bar)
        assert np.isfinite(got["td"]).all() and got["step"][0] >= 1
        # the next round is on-policy again only if the store is refreshed with the new actor
        L1.log_probs_window(r1.store["states"], r1.store["actions"], 0, CAP, r1.log_mu)


# ---- 5. stale data: draw + ratio weights + the weighted update, one by one ------------------------------------------------

@pytest.mark.parametrize("kind,importance", [("uniform", False), ("prioritised", True)])
def test_off_policy_update_from_is_draw_then_ratio_weights_then_the_weighted_update(kind, importance):
    L1, L2, _ = _twins()
    r1, r2 = _ring(kind, True), _ring(kind, True)
    _fill(r1, L1)
    _fill(r2, L2)
    for _ in range(2):
        L1.update_from(r1, 63, importance=importance, rho_bar=2.0)
        L2.update_from(r2, 63, importance=importance, rho_bar=2.0)
    blob = L1._get_params()
    r = torch.empty(63, device=DEV)
    got = _outcome(L1, r1, L1.update_from(r1, 63, importance=importance, rho_bar=2.0, rho_out=r))
    idx, w = r2._draw_batch(63, DrawSpec(importance=importance, beta=0.4))
    w_out, rho = torch.empty(63, device=DEV), torch.empty(63, device=DEV)
    _ratio(L2, 63, r2.store, r2.log_mu, CAP, idx, 2.0, w, w_out, rho)
    want = lh.update(L2, 63, r2.store, CAP, idx, r2.priorities, w_out)
    want.pop("entropy", None)
    L1.check(); L2.check()
    lh.same(got, want)
    assert _bits(r) == _bits(rho)
    # the ratios against the mirror, with the parameters the third update started from
    i = idx.cpu().numpy()
    s, a, lm = (x.cpu().numpy()[i] for x in (r2.store["states"], r2.store["actions"], r2.log_mu))
    _, rho64 = om.weights(blob, H0, A0, s, a, lm, 2.0)
    got_r = r.cpu().numpy()
    err, bound = np.abs(got_r - rho64), om.ratio_bound(rho64, om.log_prob_bound(blob, H0, A0, s))
    print(f"{kind}: rho in [{got_r.min():.4f}, {got_r.max():.4f}], share of the bound {(err / bound).max():.3f}")
    assert (err <= bound).all() and not (got_r == 1.0).all() and (got_r > 0).all() and (got_r <= 2.0).all()


# ---- 6. the store behind every add form ----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["plain", "episodes", "nstep", "lambda"])
def test_every_add_form_leaves_the_actors_log_probs_in_the_slots_it_wrote(form):
    L, _, _ = _twins()
    ring = _ring("prioritised" if form == "nstep" else "uniform", False, (0.9, 0.95) if form == "lambda" else None)
    if form == "nstep":
        ring.with_nstep(3, 0.95)
    assert ring.with_behaviour() is ring
    kw = dict(critic=L) if form == "lambda" else {}

    def check(count):
        assert ring.count == count
        lm = ring.log_mu.cpu().numpy()
        want = L.log_probs(ring.store["states"], ring.store["actions"]).cpu().numpy()
        assert np.isfinite(want[:count]).all()
        assert lm[:count].tobytes() == want[:count].tobytes()
        assert np.isnan(lm[count:]).all()                                  # slots never written stay unknown

    for k in range(5):                                                     # 300 rows: the fifth add wraps
        obs_in, out = _rollout(k, episodes=form == "episodes")
        ring.add_rollout_behaviour(obs_in, out, behaviour=L, **kw)
        check(min(CAP, 60 * (k + 1)))
    assert ring.pos == 300 - CAP
    obs_in, out = _rollout(9, steps=14, episodes=form == "episodes")       # 280 rows > 257 slots: the last 257 are kept
    ring.add_rollout_behaviour(obs_in, out, behaviour=L, **kw)
    check(CAP)
    # log_mu= in add order lands where the rows land; a torch module as the behaviour gives the same store to fp32 accuracy
    given = lh.dev(-np.arange(1, 281, dtype=np.float32))
    pos = ring.pos
    ring.add_rollout_behaviour(obs_in, out, log_mu=given, **kw)
    slots, rows = om.window_slots(pos, 280, CAP)
    assert np.array_equal(ring.log_mu.cpu().numpy()[slots], given.cpu().numpy()[rows])
    actor = _uav().ActorMLP(12, H0, A0).to(DEV)
    actor.load_state_dict(L.actor_state_dict())
    obs_in, out = _rollout(0, episodes=form == "episodes")
    ring.add_rollout_behaviour(obs_in, out, behaviour=actor, **kw)
    want = L.log_probs(ring.store["states"], ring.store["actions"])
    slots, _ = om.window_slots((ring.pos - 60) % CAP, 60, CAP)
    assert torch.allclose(ring.log_mu[slots], want[slots], rtol=0, atol=1e-4)
    assert set(ring.sample(8)[0] if form == "nstep" else ring.sample(8)) >= {"states", "actions", "log_mu"}


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------

def _flat(n, seed, log_mu=None):
    rng = np.random.RandomState(seed)
    s, a, r, s2 = lh.batch(rng, n, A0)
    d = {"states": lh.dev(s), "actions": lh.dev(a), "rewards": lh.dev(r), "next_states": lh.dev(s2)}
    if log_mu is not None:
        d["log_mu"] = lh.dev(np.asarray(log_mu, np.float32))
    return d


@pytest.mark.parametrize("what", ["unknown", "positive", "overflow"])
def test_an_unknown_or_impossible_behaviour_policy_refuses_the_update_on_the_device(what):
    L, _, _ = _twins()
    ring = _ring("prioritised", True, cap=64)
    ring.add(_flat(20, 1, np.full(20, -2.0)))
    if what == "unknown":
        ring.add(_flat(20, 2))                                              # no "log_mu": NaN
        assert torch.isnan(ring.log_mu[20:40]).all() and (ring.log_mu[:20] == -2.0).all()
    else:
        ring.add(_flat(20, 2, np.full(20, 0.5 if what == "positive" else -200.0)))
    assert ring.sample(4)[0]["log_mu"].shape == (4,)
    before = _outcome(L, ring, (torch.zeros(()), torch.zeros(()), torch.zeros(1)))
    rho = torch.empty(40, device=DEV)
    al, cl, _ = L.update_from(ring, 40, rho_bar=float("inf") if what == "overflow" else 1.0, rho_out=rho)
    with pytest.raises(RuntimeError, match="refused"):
        L.check()
    r = rho.cpu().numpy()
    assert (np.isinf(r) if what == "overflow" else np.isnan(r)).any()       # 40 draws of 40 slots with equal priorities
    assert np.isnan(float(al)) and np.isnan(float(cl))
    after = _outcome(L, ring, (torch.zeros(()), torch.zeros(()), torch.zeros(1)))
    lh.same(after, before)                                                  # parameters, moments, steps, priorities
    # the learner is none the worse: rows whose behaviour is known train
    ok = _ring("uniform", True, cap=64)
    ok.add(_flat(20, 1, np.full(20, -2.0)))
    L.update_from(ok, 20, rho_bar=1.0)
    L.check()
    assert lh.state(L)["step"][0] == 1


def test_the_host_refuses_a_rho_bar_that_is_not_positive_and_enqueues_nothing():
    L, _, _ = _twins()
    ring = _ring("uniform", True, cap=64)
    ring.add(_flat(20, 1, np.full(20, -2.0)))
    before = lh.state(L)
    w = torch.full((20,), 7.0, device=DEV)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="rho_bar"):
            _ratio(L, 20, ring.store, ring.log_mu, 64, None, bad, None, w, None)
        with pytest.raises(RuntimeError, match="rho_bar"):
            L.update_from(ring, 20, rho_bar=bad)
    from uavtrack import _lib
    for args in ((None, ring.log_mu, w), (ring.store["states"], None, w), (ring.store["states"], ring.log_mu, None)):
        rc = L._lib.uavtrack_learner_ratio_weights(L._h, 20, _lib.ptr(args[0]), _lib.ptr(ring.store["actions"]),
                                                   _lib.ptr(args[1]), 64, None, 1.0, None, _lib.ptr(args[2]), None, L._stream())
        assert rc != 0
    assert L._lib.uavtrack_learner_ratio_weights(L._h, 0, _lib.ptr(ring.store["states"]), _lib.ptr(ring.store["actions"]),
                                                 _lib.ptr(ring.log_mu), 64, None, 1.0, None, _lib.ptr(w), None,
                                                 L._stream()) != 0
    L.check()
    assert (w == 7.0).all()
    lh.same(lh.state(L), before)
    plain = _ring("uniform", False, cap=64)
    plain.add(_flat(20, 1))
    with pytest.raises(ValueError, match="with_behaviour"):
        L.update_from(plain, 20, rho_bar=1.0)
    with pytest.raises(ValueError, match="behaviour ring"):
        plain.add_rollout_behaviour(*_rollout(0), behaviour=L)
    with pytest.raises(ValueError, match="exactly one"):
        ring.add_rollout(*_rollout(0))


# ---- 8. the split update -----------------------------------------------------------------------------------------------

def test_update_from_many_is_the_apply_of_the_explicit_weighted_rows():
    L1, L2, _ = _twins()
    rings1 = [_ring("uniform", True, seed=3), _ring("prioritised", True, seed=4)]
    rings2 = [_ring("uniform", True, seed=3), _ring("prioritised", True, seed=4)]
    for r1, r2 in zip(rings1, rings2):
        _fill(r1, L1)
        _fill(r2, L2)
    stale = lh.init_blob(H0, A0, 78)                                        # the actor moves on; the stores stay
    L1._set_params(0.5 * (L1._get_params() + stale))
    L2._set_params(0.5 * (L2._get_params() + stale))
    before = lh.state(L1)
    row, td, idx = L1.grad_from(rings1[0], 40, rho_bar=2.0)
    L2.grad_from(rings2[0], 40, rho_bar=2.0)                                # (keeps the twins' draw counters equal)
    lh.same(lh.state(L1), before)                                           # grad_from changes nothing in the learner
    rhos = [torch.empty(40, device=DEV) for _ in rings1]
    al, cl, tds = L1.update_from_many(rings1, 40, importance=True, rho_bar=2.0, rho_out=rhos)
    rows = L2.new_rows(2)
    want_td = []
    for k, ring in enumerate(rings2):
        i, w = ring._draw_batch(40, DrawSpec(importance=True, beta=0.4))    # a uniform ring: no weights
        w_out = torch.empty(40, device=DEV)
        _ratio(L2, 40, ring.store, ring.log_mu, CAP, i, 2.0, w, w_out, None)
        _, t = L2._grad(40, ring.store, CAP, i, rows[k], None, w_out)
        want_td.append((i, t))
    al2, cl2 = L2.apply(rows)
    for ring, (i, t) in zip(rings2, want_td):
        L2.write_priorities(ring, i, t)
    L1.check(); L2.check()
    lh.same(lh.state(L1), lh.state(L2))
    assert _bits(al) == _bits(al2) and _bits(cl) == _bits(cl2)
    for a, (_, b) in zip(tds, want_td):
        assert _bits(a) == _bits(b)
    assert _bits(rings1[1].priorities) == _bits(rings2[1].priorities)
    assert all(not (r == 1.0).all() and (r > 0).all() and (r <= 2.0).all() for r in rhos)


# ---- 9. one captured graph -------------------------------------------------------------------------------------------------

def test_draw_weights_and_update_capture_into_one_graph():
    L1, L2, _ = _twins()
    r1, r2 = _ring("prioritised", True), _ring("prioritised", True)
    _fill(r1, L1)
    _fill(r2, L2)
    stale = lh.init_blob(H0, A0, 78)
    L1._set_params(0.5 * (L1._get_params() + stale))
    L2._set_params(0.5 * (L2._get_params() + stale))
    rho1, rho2 = torch.empty(63, device=DEV), torch.empty(63, device=DEV)

    def iteration(L, ring, rho):
        return L.update_from(ring, 63, importance=True, rho_bar=2.0, rho_out=rho)

    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = iteration(L2, r2, rho2)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(L2)["step"], np.zeros(8))                # capture ran nothing
    for c in range(2):
        e_out = iteration(L1, r1, rho1)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y) and torch.isfinite(x).all(), c
        assert _bits(rho1) == _bits(rho2) and not (rho1 == 1.0).all()
        lh.same(lh.state(L1), lh.state(L2), c)
        assert _bits(r1.priorities) == _bits(r2.priorities)
    L1.check(); L2.check()
    assert lh.state(L1)["step"][0] == 2


# ---- 10. unchanged when off ------------------------------------------------------------------------------------------------

def test_without_rho_bar_every_call_is_what_it_was():
    L1, L2, _ = _twins()
    rings1 = [_ring("uniform", False, seed=3), _ring("prioritised", False, seed=4)]
    rings2 = [_ring("uniform", False, seed=3), _ring("prioritised", False, seed=4)]
    for r1, r2 in zip(rings1, rings2):
        assert r1.log_mu is None and r1._rho_w is None
        _fill(r1, L1)
        _fill(r2, L2)
    assert "log_mu" not in rings1[0]._gather(slice(0, 2))
    batch = _flat(50, 5)
    a = L1.update(batch, log_mu=None, rho_bar=None)
    b = L2.update(batch)
    assert all(_bits(x) == _bits(y) for x, y in zip(a, b))
    for r1, r2 in zip(rings1, rings2):
        got = _outcome(L1, r1, L1.update_from(r1, 63, importance=True, rho_bar=None, rho_out=None))
        lh.same(got, _outcome(L2, r2, L2.update_from(r2, 63, importance=True)))
        x = L1.grad_from(r1, 63, rho_bar=None)
        y = L2.grad_from(r2, 63)
        assert all(_bits(p) == _bits(q) for p, q in zip(x, y))
    x = L1.update_from_many(rings1, 40, rho_bar=None)
    y = L2.update_from_many(rings2, 40)
    assert _bits(x[0]) == _bits(y[0]) and _bits(x[1]) == _bits(y[1])
    assert all(_bits(p) == _bits(q) for p, q in zip(x[2], y[2]))
    L1.check(); L2.check()
    lh.same(lh.state(L1), lh.state(L2))
    assert _bits(rings1[1].priorities) == _bits(rings2[1].priorities)
    with pytest.raises(ValueError, match="come together"):
        L1.update(batch, rho_bar=1.0)
    # update(log_mu=, rho_bar=): on-policy it is the plain update, to the bit
    lp = L1.log_probs(batch["states"], batch["actions"])
    a = L1.update(batch, log_mu=lp, rho_bar=1.0)
    b = L2.update(batch)
    assert all(_bits(p) == _bits(q) for p, q in zip(a, b))
    lh.same(lh.state(L1), lh.state(L2))


# ---- the example ---------------------------------------------------------------------------------------------------------

def test_example_trains_with_truncated_ratios_and_prints_them(capsys):
    """examples/train_maac.py --rho-bar 1.0: the device learner (prioritised ring, device publish, one printed line per two
    iterations), two shards over uniform rings, and the torch learner train; every printed line carries the mean ratio
    and the share of rows at the cap; --replay uniform is refused with a message."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_maac
    common = ["--envs", "64", "--steps", "20", "--iters", "2", "--batch", "4096", "--updates", "2", "--rho-bar", "1.0"]
    for extra, printed in ((["--replay", "prioritized", "--learner", "device", "--actor-loss", "per_sample", "--publish",
                             "device", "--log-every", "2", "--importance"], 1),
                           (["--replay", "uniform-device", "--learner", "device", "--shards", "2", "--td-lambda", "0.9"], 2),
                           (["--replay", "prioritized", "--learner", "torch"], 2)):
        hist = train_maac.main(common + extra)                               # learner.check() inside: nothing was refused
        assert len(hist) == 2 and np.isfinite(hist).all(), extra
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == printed, extra
        for ln in lines:
            mean, cap = float(ln.split("rho mean")[1].split()[0]), float(ln.split("at cap")[1].split()[0])
            assert 0.5 < mean <= 1.0 and 0.0 <= cap <= 1.0, ln
            assert np.isfinite(float(ln.split("critic loss")[1].split()[0])), ln
    with pytest.raises(SystemExit):
        train_maac.main(common + ["--replay", "uniform"])
    assert "--rho-bar" in capsys.readouterr().err
