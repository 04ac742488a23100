"""KL early stopping of the device learner (uavtrack_learner_set_kl_stop, DeviceActorCritic.set_kl_stop) on the MI355X,
loss="per_sample": the estimate against tests/learner_kl_mirror.py formed from the same call's ratio_out; an update that
does not trip the latch is the stop-off update bit for bit; one that does changes nothing, and neither does any update
behind it until kl_reset; a refused update is not a stopped one; and E epochs of M minibatches as 12 replays of one
captured update stop where the eager stop-off run's own KLs say they must.

Cases are learner_harness's; the behaviour store is log_mu = min(log_probs(now) + noise, 0) with noise of +-0.3 per slot
(k_i of about 0.04 to 0.05 per row), and every test asserts the mirror's KL >= 1e-3, so limits of half and double it sit
far from any rounding.

The value is asserted EQUAL to the mirror's.  The ratios are the same float32 bits on both sides and every float64
subtraction and add is the same operation in the one stated order, so the only freedom is two float64 log implementations
(each within an ulp of float64) moving sum / n across one float32 rounding boundary, 2^29 float64 steps apart.  The device
came out exact (0 ulp) on every shape here, so the bound of 1 float32 ulp that this freedom would allow was tightened to
equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import learner_harness as lh
import learner_kl_mirror as klm

pytestmark = pytest.mark.gpu

DEV = lh.DEV
INF = float("inf")
EPS = 0.2
SHAPES = [(32, 12, 1, False), (33, 9, 257, True), (128, 12, 6007, False)]   # one row; a chunk plus a row; 24 chunks, many tiles
IDS = [f"H{H}-A{A}-n{n}" for H, A, n, _ in SHAPES]
ONE = SHAPES[1]
TD_SENTINEL, RATIO_SENTINEL = 12345.0, -7.0
KEYS = ("params", "exp_avg", "exp_avg_sq", "step", "actor_loss", "critic_loss", "td", "ratio", "prio")


def _uav():
    import uavtrack
    return uavtrack


_setups = {}


def _setup(H, A, n, gather):
    """learner_harness.case plus, per slot of the store, the log-probabilities of the case's own actor (on-policy) and
    those shifted by +-0.3 (off-policy), and the first priorities; built once."""
    key = (H, A, n, gather)
    if key not in _setups:
        blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
        lp = lh.learner(H, A, "per_sample", blob, n).log_probs(store["states"], store["actions"])
        sign = np.where(np.random.RandomState(H + n + 3).randint(0, 2, size=cap) == 1, 0.3, -0.3).astype(np.float32)
        off = torch.minimum(lp + lh.dev(sign), torch.zeros_like(lp))
        prio0 = lh.dev(np.random.RandomState(n).uniform(0.1, 1.1, cap).astype(np.float32))
        _setups[key] = dict(blob=blob, store=store, cap=cap, it=it, n=n, H=H, A=A, on=lp, off=off, prio0=prio0)
    return _setups[key]


def _learner(case, limit="off", **kw):
    L = lh.learner(case["H"], case["A"], "per_sample", case["blob"], max(case["n"], 2), **kw)
    if limit != "off":
        L.set_kl_stop(limit)
    return L


def _run(L, c, mu, prio=None, w=None, adv=None, store=None):
    """One closed clipped update into sentinel-filled td_delta and ratio_out: the learner's state after it, the outputs
    and, while the stop is on, kl and kl_state."""
    n = c["n"]
    td = torch.full((n,), TD_SENTINEL, device=DEV)
    ratio = torch.full((n,), RATIO_SENTINEL, device=DEV)
    losses = torch.empty(2, device=DEV)
    L._launch("update", L._Batch(n, store or c["store"], c["cap"], c["it"], prio, w, None, mu, EPS, ratio, adv),
              losses[0:1], losses[1:2], td, prio)
    out = dict(lh._result(L, n, losses[0], losses[1], td, prio), ratio=ratio.cpu().numpy())
    if L.kl is not None:
        out["kl"], out["kl_state"] = L.kl.cpu().numpy()[0], L.kl_state.cpu().numpy().tolist()
    return out


def _refused(L):
    """uavtrack_learner_check itself: (return code, the count)."""
    count = C.c_int64(-1)
    rc = L._lib.uavtrack_learner_check(L._h, C.byref(count), L._stream())
    return rc, count.value


_refs = {}


def _reference(shape):
    """The stop-off update of a shape with a prioritised ring's priorities, and the mirror's KL of its ratios; once."""
    if shape not in _refs:
        c = _setup(*shape)
        out = _run(_learner(c), c, c["off"], c["prio0"].clone())
        kl = klm.kl(out["ratio"])
        assert kl >= 1e-3, kl
        _refs[shape] = (out, kl)
    return _refs[shape]


# ---- 1. the value ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kl_is_the_mirror_of_the_calls_own_ratios(shape):
    c = _setup(*shape)
    L = _learner(c, INF)
    assert L.get_kl_stop() == INF and np.isnan(L.kl.cpu().numpy()[0])
    out = _run(L, c, c["off"])
    want = klm.kl(out["ratio"])
    print(f"kl: device {out['kl']!r}, mirror {want!r} (float64 {klm.kl64(out['ratio'])!r}), {klm.ulps(out['kl'], want)} ulp")
    assert want >= 1e-3
    assert out["kl"] == want
    assert out["kl_state"] == [0, 0] and np.array_equal(out["step"], np.full(8, 1))
    L.check()
    # without a ratio_out the ratios go through the handle's scratch: the same value
    L2 = _learner(c, INF)
    n = c["n"]
    losses, td = torch.empty(2, device=DEV), torch.empty(n, device=DEV)
    L2._launch("update", L2._Batch(n, c["store"], c["cap"], c["it"], None, None, None, c["off"], EPS, None),
               losses[0:1], losses[1:2], td, None)
    assert L2.kl.cpu().numpy()[0] == out["kl"]
    L2.check()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_on_policy_the_kl_is_exactly_zero_and_never_stops(shape):
    c = _setup(*shape)
    L = _learner(c, 0.0)
    out = _run(L, c, c["on"])
    assert np.array_equal(out["ratio"], np.ones(c["n"], np.float32))
    assert out["kl"] == 0.0 and not np.signbit(out["kl"])
    assert out["kl_state"] == [0, 0] and np.array_equal(out["step"], np.full(8, 1)) and np.isfinite(out["actor_loss"])
    out = _run(L, c, L.log_probs(c["store"]["states"], c["store"]["actions"]))       # the actor moved; so did log_mu
    assert out["kl"] == 0.0 and out["kl_state"] == [0, 0] and np.array_equal(out["step"], np.full(8, 2))
    L.check()


# ---- 2. not tripped: the stop-off update, bit for bit ----------------------------------------------------------------------

@pytest.mark.parametrize("limit", ["2kl", "inf"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_an_update_within_the_limit_is_the_stop_off_update(shape, limit):
    c = _setup(*shape)
    ref, kl = _reference(shape)
    out = _run(_learner(c, INF if limit == "inf" else 2.0 * float(kl)), c, c["off"], c["prio0"].clone())
    lh.same({k: out[k] for k in KEYS}, {k: ref[k] for k in KEYS})
    assert out["kl_state"] == [0, 0] and out["kl"] == kl
    assert np.array_equal(out["step"], np.full(8, 1)) and not np.array_equal(out["prio"], c["prio0"].cpu().numpy())


@pytest.mark.parametrize("option", ["batch", "target", "stored", "weights"])
def test_within_the_limit_with_the_other_settings_on(option):
    """set_advantage("batch"), a target critic, stored advantages and importance weights, each on the one-chunk-plus-a-row
    shape: stop on (limit 2 kl) against stop off, every output and the setting's own state."""
    c = _setup(*ONE)
    w = lh.dev(lh.make_weights(np.random.RandomState(5), c["n"])) if option == "weights" else None
    adv = lh.dev(np.random.RandomState(6).randn(c["cap"]).astype(np.float32)) if option == "stored" else None
    outs = []
    for limit in ("off", None):
        L = _learner(c, "off", c=0.01, mgn=0.5, diag=True)
        if option == "batch":
            L.set_advantage("batch")
        if option == "target":
            L.set_target(tau=0.5)
            L._set_target_params(np.ascontiguousarray(L._get_target_params() * np.float32(0.5)))
        if limit is None:
            L.set_kl_stop(2.0 * float(klm.kl(outs[0]["ratio"])))
        out = _run(L, c, c["off"], c["prio0"].clone(), w, adv)
        if option == "batch":
            out["stats"] = L.advantage_stats.cpu().numpy()
        if option == "target":
            out["theta"] = L._get_target_params()
        L.check()
        outs.append(out)
    off, on = outs
    assert klm.kl(off["ratio"]) >= 1e-3 and on["kl_state"] == [0, 0]
    keys = KEYS + ("entropy", "grad_norm") + (("stats",) if option == "batch" else ()) + (("theta",) if option == "target" else ())
    lh.same({k: on[k] for k in keys}, {k: off[k] for k in keys})
    assert np.array_equal(on["step"], np.full(8, 1))


# ---- 3. tripped ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_tripped_update_changes_nothing_and_latches_until_reset(shape):
    c = _setup(*shape)
    _, kl = _reference(shape)
    limit = 0.5 * float(kl)
    L = _learner(c, limit, mgn=0.5, diag=True)
    L.set_target(period=1)
    theta0 = np.ascontiguousarray(L._get_target_params() * np.float32(0.5))
    L._set_target_params(theta0)
    before = lh.state(L)
    prio = c["prio0"].clone()
    out = _run(L, c, c["off"], prio)
    lh.same({k: out[k] for k in before}, before, "tripped")
    assert np.array_equal(L._get_target_params(), theta0) and torch.equal(prio, c["prio0"])
    assert np.isnan(out["actor_loss"]) and np.isnan(out["critic_loss"]) and np.isnan(out["grad_norm"]).all()
    assert out["kl_state"] == [1, 1] and out["kl"] == kl
    assert not (out["td"] == TD_SENTINEL).any() and klm.kl(out["ratio"]) == kl    # the tripping update's rows were formed
    assert _refused(L) == (0, 0)
    # a following on-policy update (its own kl would be 0) is skipped too, before its first tile
    out2 = _run(L, c, c["on"], prio)
    lh.same({k: out2[k] for k in before}, before, "skipped")
    assert np.array_equal(L._get_target_params(), theta0) and torch.equal(prio, c["prio0"])
    assert np.isnan(out2["actor_loss"]) and np.isnan(out2["critic_loss"])
    assert out2["kl_state"] == [1, 2] and out2["kl"] == out["kl"]
    assert (out2["td"] == TD_SENTINEL).all() and (out2["ratio"] == RATIO_SENTINEL).all()
    assert _refused(L) == (0, 0)
    # after the reset: the update of a never-latched learner in the same state
    L.kl_reset()
    assert L.kl_state.cpu().numpy().tolist() == [0, 0]
    F = _learner(c, limit, mgn=0.5, diag=True)
    F.set_target(period=1)
    F._set_target_params(theta0)
    prio_f = c["prio0"].clone()
    got, want = _run(L, c, c["on"], prio), _run(F, c, c["on"], prio_f)
    lh.same({k: got[k] for k in KEYS + ("grad_norm", "entropy")}, {k: want[k] for k in KEYS + ("grad_norm", "entropy")}, "reset")
    assert np.array_equal(L._get_target_params(), F._get_target_params())
    assert got["kl"] == 0.0 and got["kl_state"] == [0, 0] and np.array_equal(got["step"], np.full(8, 1))
    assert not np.array_equal(L._get_target_params(), theta0) and not torch.equal(prio, c["prio0"])
    L.check(); F.check()


def test_a_tripped_update_under_batch_advantages_leaves_what_a_refused_one_leaves():
    c = _setup(*ONE)
    _, kl = _reference(ONE)
    L = _learner(c, 0.5 * float(kl))
    L.set_advantage("batch")
    before = lh.state(L)
    out = _run(L, c, c["off"])
    lh.same({k: out[k] for k in before}, before)
    assert out["kl_state"] == [1, 1] and np.isnan(L.advantage_stats.cpu().numpy()).all()
    assert _refused(L) == (0, 0)


# ---- 4. refused is not stopped ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("limit", [0.0, INF])
def test_a_refused_update_never_sets_the_latch(limit):
    c = _setup(*ONE)
    L = _learner(c, limit)
    bad = dict(c["store"], actions=c["store"]["actions"].clone())
    bad["actions"][c["it"][0]] = c["A"]                             # the first batch row's action: out of range
    before = lh.state(L)
    out = _run(L, c, c["off"], store=bad)
    lh.same({k: out[k] for k in before}, before)
    assert np.isnan(out["kl"]) and out["kl_state"] == [0, 0] and np.isnan(out["actor_loss"])
    rc, count = _refused(L)
    assert rc != 0 and count == 1
    out = _run(L, c, c["on"])                                       # and the learner goes on
    assert out["kl"] == 0.0 and np.array_equal(out["step"], np.full(8, 1))
    L.check()


def test_the_library_refuses_what_brings_no_ratios_while_on():
    c = _setup(*ONE)
    L = _learner(c, 0.02)
    lib, ptr = L._lib, _uav()._lib.ptr
    n, store, cap, it = c["n"], c["store"], c["cap"], c["it"]
    losses, td, row = torch.empty(2, device=DEV), torch.empty(n, device=DEV), torch.empty(L.row_floats, device=DEV)
    args = (L._h, n, *L._batch_args(store, cap, it))
    outs = (ptr(losses[0:1]), ptr(losses[1:2]), ptr(td), None, L._stream())
    mu = ptr(c["off"])

    def refused(rc, message):
        assert rc != 0 and message in lib.uavtrack_last_error(), lib.uavtrack_last_error()

    refused(lib.uavtrack_learner_update(*args, *outs), b"brings none")
    refused(lib.uavtrack_learner_update_weighted(*args, None, *outs), b"brings none")
    refused(lib.uavtrack_learner_update_discounted(*args, None, None, *outs), b"brings none")
    refused(lib.uavtrack_learner_update_stored(*args, None, None, mu, None, 0.2, None, *outs), b"brings none")
    refused(lib.uavtrack_learner_grad(*args, ptr(td), ptr(row), L._stream()), b"nowhere to carry a KL sum")
    refused(lib.uavtrack_learner_grad_clipped(*args, None, None, mu, 0.2, None, ptr(td), ptr(row), L._stream()),
            b"nowhere to carry a KL sum")
    refused(lib.uavtrack_learner_apply(L._h, ptr(row), 1, ptr(losses[0:1]), ptr(losses[1:2]), L._stream()), b"no KL sum")
    kl, state = ptr(L.kl), ptr(L.kl_state)
    refused(lib.uavtrack_learner_set_kl_stop(L._h, 1, float("nan"), kl, state), b"must be >= 0")
    refused(lib.uavtrack_learner_set_kl_stop(L._h, 1, -1.0, kl, state), b"must be >= 0")
    refused(lib.uavtrack_learner_set_kl_stop(L._h, 1, 0.02, None, state), b"must not be null")
    refused(lib.uavtrack_learner_set_kl_stop(L._h, 1, 0.02, kl, None), b"must not be null")
    assert L.get_kl_stop() == 0.02                                  # the refused calls changed nothing
    before = lh.state(L)
    torch.cuda.synchronize()
    lh.same(lh.state(L), before)
    assert L.kl_state.cpu().numpy().tolist() == [0, 0] and _refused(L) == (0, 0)
    L.set_kl_stop(None)
    assert L.get_kl_stop() is None
    refused(lib.uavtrack_learner_kl_reset(L._h, L._stream()), b"is off")
    R = lh.learner(c["H"], c["A"], "reference", c["blob"], n)
    k2, s2 = torch.zeros(1, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    refused(lib.uavtrack_learner_set_kl_stop(R._h, 1, 0.02, ptr(k2), ptr(s2)), b"UAVTRACK_LOSS_REFERENCE")


# ---- 5. an iteration under a graph -----------------------------------------------------------------------------------------

def test_twelve_replays_of_one_captured_update_stop_where_the_eager_run_says():
    uav = _uav()
    H, A, CAP, K, M, E = 32, 12, 1024, 256, 4, 3
    calls = M * E
    lr = (1e-2, 5e-3)                                               # an actor rate at which the policy leaves mu within an epoch

    def fresh(limit="off"):
        torch.manual_seed(11)
        L = uav.DeviceActorCritic(12, H, A, lr[0], lr[1], 0.95, DEV, loss="per_sample", max_batch=K)
        if limit != "off":
            L.set_kl_stop(limit)
        return L

    rng = np.random.RandomState(12)
    ring = uav.ReplayRing(CAP, DEV, seed=5, max_batch=K).with_behaviour()
    obs_in = lh.dev(rng.randn(8, 8, 12).astype(np.float32))
    rollout = {"obs": lh.dev(rng.randn(16, 8, 8, 12).astype(np.float32)),
               "actions": lh.dev(rng.randint(0, A, (16, 8, 8)).astype(np.int32)),
               "reward": lh.dev(rng.randn(16, 8, 8).astype(np.float32))}
    ring.add_rollout_behaviour(obs_in, rollout, behaviour=fresh())  # log_mu of the initial actor: call 0 is on-policy
    sweep = ring.sweep(K)
    assert sweep.window == (0, CAP) and sweep.minibatches == M

    # the stop-off run: the state before each update and the mirror's KL of each
    off = fresh()
    ratio = torch.empty(K, device=DEV)
    snaps, kls = [], []
    for q in range(calls):
        snaps.append(lh.state(off))
        off.update_from(sweep, K, clip_eps=EPS, ratio_out=ratio)
        kls.append(float(klm.kl(ratio.cpu().numpy())))
    snaps.append(lh.state(off))
    off.check()
    print("stop-off KLs:", " ".join(f"{k:.3e}" for k in kls))
    assert kls[0] == 0.0
    # the limit: between two successive KLs of which the later is the first above everything before it
    rising = [q for q in range(2, 11) if kls[q - 1] == max(kls[:q]) and kls[q] > kls[q - 1] > 0]
    assert rising, kls
    q_star = rising[len(rising) // 2]
    limit = float(np.sqrt(kls[q_star - 1] * kls[q_star]))
    assert all(k < limit for k in kls[:q_star]) and kls[q_star] > limit and 1 <= q_star <= 10
    assert all(abs(k - limit) >= 1e-3 * limit for k in kls[:q_star + 1]), (limit, kls)
    print(f"limit {limit:.3e}: the first crossing is update {q_star}")

    def iteration(L, step):
        L.kl_reset()
        sweep.rebind()
        for _ in range(calls):
            step()
        torch.cuda.synchronize()
        assert sweep.position() == calls                            # the draws went on under the stopped updates
        lh.same(lh.state(L), snaps[q_star])
        assert L.kl_state.cpu().numpy().tolist() == [1, calls - q_star]
        assert L.kl.cpu().numpy()[0] == np.float32(kls[q_star])
        L.check()

    eager = fresh(limit)
    iteration(eager, lambda: eager.update_from(sweep, K, clip_eps=EPS))

    G = fresh(limit)
    G.update_from(sweep, K, clip_eps=EPS)                           # warm-up, eager; then back to the initial state
    G._set_params(snaps[0]["params"])
    P = G.num_params
    G._set_optim_state(np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(8, np.int64))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = G.update_from(sweep, K, clip_eps=EPS)
    iteration(G, g.replay)
    assert torch.isnan(held[0]).all() and torch.isnan(held[1]).all()   # the last replay was a stopped update
