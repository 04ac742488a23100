"""The device learner's target critic (uavtrack_learner_set_target, DeviceActorCritic.set_target) on the MI355X: off is
off; the bootstrap substituted bit for bit against a plain learner that is handed V_target(s') as its rewards; the update
against the float64 mirror (tests/learner_mirror.py with theta=) at the harness's bounds; the Polyak and the periodic rule
against their float32 mirrors; the split update and several rings; the target's values and a lambda ring's add; graph
capture; checkpoints and pack / unpack.

Shapes (H, A, n): the narrowest and the widest hidden width, a width that is a multiple of nothing, the LDS-heavy
instantiation, a partial tile, and (256 wide: 16 rows per tile) more tiles than one workgroup; each with and without an
index vector."""
import numpy as np
import pytest
import torch

import learner_harness as lh
import learner_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA
SHAPES = [(1, 9, 1), (33, 12, 65), (128, 12, 63), (256, 48, 4097)]
LOSSES = ["reference", "per_sample"]
GATHER = pytest.mark.parametrize("gather", [False, True], ids=["rows", "indexed"])
NEVER = 10 ** 9            # a period no test reaches: a target that stays what it was given


def _uav():
    import uavtrack
    return uavtrack


def _other(H, A, seed=0):
    """A critic block that is not the case's: theta- != theta."""
    return mirror.critic_block(lh.init_blob(H, A, 5000 + H + seed), H, A)


def _weights(n):
    return lh.make_weights(np.random.RandomState(n + 11), n)


def _prio(cap):
    return (torch.arange(cap, device=DEV, dtype=torch.float32) % 7) * 0.25 + 0.1


def _full(L):
    """The learner's state with theta- (None while off)."""
    return dict(lh.state(L), target=L._get_target_params() if L._target_on() else None)


# ---- 1. off is off -------------------------------------------------------------------------------------------------------

@GATHER
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("H,A,n", SHAPES)
def test_off_is_off_and_a_fresh_target_is_the_critic(H, A, n, loss, gather):
    """A learner that enabled a target (with another theta-) and disabled it again updates bit for bit like one that
    never did, twice in a row; with a target freshly enabled (theta- = the critic) the first update's td_delta, losses,
    moments, parameters and priorities are the plain learner's bits, under either rule."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    plain = lh.learner(H, A, loss, blob, n)
    toggled = lh.learner(H, A, loss, blob, n)
    toggled.set_target(tau=0.3)
    toggled._set_target_params(_other(H, A))
    toggled.set_target()
    assert toggled.get_target() == {"tau": None, "period": None} == plain.get_target()
    pp, pt = _prio(cap), _prio(cap)
    first = None
    for k in range(2):
        want = lh.update(plain, n, store, cap, it, pp)
        lh.same(lh.update(toggled, n, store, cap, it, pt), want, k)
        first = first or want
    for kw in (dict(tau=0.3), dict(period=NEVER)):
        fresh = lh.learner(H, A, loss, blob, n)
        fresh.set_target(**kw)
        assert fresh._get_target_params().tobytes() == mirror.critic_block(blob, H, A).tobytes()
        lh.same(lh.update(fresh, n, store, cap, it, _prio(cap)), first, kw)
    for L in (plain, toggled, fresh):
        L.check()


# ---- 2. substitution, bitwise ----------------------------------------------------------------------------------------------

@GATHER
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("H,A,n", SHAPES)
def test_bootstrap_is_the_target_critics_value_bitwise(H, A, n, loss, weighted, gather):
    """A bootstraps from theta- != theta over rewards 0 and discounts 1.0: y = V_target(s') exactly.  B is a plain
    learner with the same theta whose rewards ARE V_target(s') -- values(next_states) of a third, plain learner whose
    critic is theta- -- and whose discounts are 0.0.  Every output and the whole state after the update are bit-equal."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    theta = _other(H, A)
    w = lh.dev(_weights(n)) if weighted else None
    A_ = lh.learner(H, A, loss, blob, n)
    A_.set_target(period=NEVER)
    A_._set_target_params(theta)
    B_ = lh.learner(H, A, loss, blob, n)
    C_ = lh.learner(H, A, loss, mirror.with_critic(blob, H, A, theta), n)
    v_next = C_.values(store["next_states"])
    assert v_next.shape == (cap,)
    assert torch.equal(A_.target.values(store["next_states"]), v_next)
    assert not torch.equal(B_.values(store["next_states"]), v_next)             # theta- != theta shows
    store_a = dict(store, rewards=torch.zeros(cap, device=DEV))
    store_b = dict(store, rewards=v_next)
    ones, zeros = torch.ones(cap, device=DEV), torch.zeros(cap, device=DEV)
    pa, pb = (_prio(cap), _prio(cap)) if gather else (None, None)
    got = lh.update(A_, n, store_a, cap, it, pa, w, ones)
    want = lh.update(B_, n, store_b, cap, it, pb, w, zeros)
    lh.same(got, want)
    assert np.isfinite(got["td"]).all() and np.array_equal(got["step"], np.ones(8))
    assert A_._get_target_params().tobytes() == theta.tobytes()               # step 1 is no multiple of the period
    for L in (A_, B_):
        L.check()


@GATHER
@pytest.mark.parametrize("H,A,n", SHAPES)
def test_bootstrap_substitution_holds_under_the_entropy_bonus_and_clipping(H, A, n, gather):
    """The same substitution through learner_grad_reg_target_kernel (an entropy bonus, diagnostics installed) with the
    gradient-norm clip on: the regularised instantiation takes V(s') from theta- and nothing else changes; the Polyak
    step behind the clipped Adam step is the mirror's."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    theta = _other(H, A)
    kw = dict(c=0.3, mgn=(1e-3, 1e-3), diag=True)
    A_ = lh.learner(H, A, "per_sample", blob, n, **kw)
    A_.set_target(tau=0.5)
    A_._set_target_params(theta)
    B_ = lh.learner(H, A, "per_sample", blob, n, **kw)
    v_next = lh.learner(H, A, "per_sample", mirror.with_critic(blob, H, A, theta), n).values(store["next_states"])
    ones, zeros = torch.ones(cap, device=DEV), torch.zeros(cap, device=DEV)
    got = lh.update(A_, n, dict(store, rewards=zeros), cap, it, _prio(cap), None, ones)
    want = lh.update(B_, n, dict(store, rewards=v_next), cap, it, _prio(cap), None, zeros)
    lh.same(got, want)
    assert np.isfinite(got["grad_norm"]).all() and (got["grad_norm"] > 0).all() and (got["entropy"] > 0).all()
    assert A_._get_target_params().tobytes() == mirror.polyak(theta, mirror.critic_block(got["params"], H, A), 0.5).tobytes()
    for L in (A_, B_):
        L.check()


# ---- 3. against fp64 -------------------------------------------------------------------------------------------------------

U = 2.0 ** -24
_clear = {}


def _on_a_kink(blob, H, A, s):
    """The rows of s with a hidden pre-activation of the actor or of the critic within the float32 chain's rounding of
    0: 13 fused operations, each within 2^-24 of the running magnitude |b| + sum |w_k| |x_k| (16 for a margin).  Formed
    in float64 from the inputs alone."""
    w1a, b1a, _, _, w1c, b1c, _, _ = mirror.unpack(blob, H, A)
    s = np.asarray(s, np.float64)
    bad = np.zeros(len(s), bool)
    for W, bias in ((w1a, b1a), (w1c, b1c)):
        bad |= (np.abs(s @ W.T + bias) <= 16 * U * (np.abs(s) @ np.abs(W).T + np.abs(bias))).any(axis=1)
    return bad


def _clear_case(H, A, n, gather):
    """learner_harness.case's recipe with every row of `states` away from the ReLU kinks of the two networks that are
    differentiated.  The backward pass gates on h > 0; where a pre-activation is 0 to within float32 rounding, the gate
    the float32 chain takes and the one float64 takes are both right and the gradients differ by a whole row's term, so
    a float64 mirror is no reference there.  (learner_harness.case(256, 48, 4097, False) has such a row: the actor's
    unit 188 on row 887 is +2.0e-9 in float64 and -7.8e-9 along the float32 chain; on that batch the per-sample update
    of this test was 1.12 tol_g away from the mirror, against 0.012 on the indexed batch of the same shape.)  Rows on a
    kink are drawn again from the same generator; next_states need no care: V(s') is not differentiated and ReLU itself
    is continuous."""
    key = (H, A, n, gather)
    if key not in _clear:
        rng = np.random.RandomState(H * 1000 + n + (7 if gather else 0))
        cap = n + 7 if gather else n
        blob = lh.init_blob(H, A, H + n)
        s, a, r, s2 = lh.batch(rng, cap, A)
        bad = _on_a_kink(blob, H, A, s)
        while bad.any():
            s[bad] = lh.batch(rng, int(bad.sum()), A)[0]
            bad = _on_a_kink(blob, H, A, s)
        b = (s, a, r, s2)
        idx = rng.randint(0, cap, size=n).astype(np.int64) if gather else np.arange(n)
        _clear[key] = (blob, b, {k: lh.dev(x) for k, x in zip(lh.STORES, b)}, cap, idx, lh.dev(idx) if gather else None)
    return _clear[key]


@GATHER
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("H,A,n", SHAPES)
def test_update_with_a_target_against_the_fp64_mirror(H, A, n, loss, gather):
    """theta- != theta, ordinary rewards and gamma: the harness's bounds of a single update from zero moments, on
    batches whose states keep clear of the ReLU kinks (_clear_case)."""
    blob, b, store, cap, idx, it = _clear_case(H, A, n, gather)
    theta = _other(H, A)
    L = lh.learner(H, A, loss, blob, n)
    L.set_target(tau=0.01)
    L._set_target_params(theta)
    out = lh.update(L, n, store, cap, it, None)
    L.check()
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), GAMMA, loss, theta=theta)[:4]
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ral, rcl, rtd)
    lh.assert_step_from_zero(out, blob, g, n, H, A)
    # the target moved the targets: the plain mirror's td_delta is another one
    plain_td = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), GAMMA, loss).td
    assert np.abs(plain_td - rtd).max() > 1e-6


# ---- 4. the Polyak chain -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tau", [0.005, 0.3, 1.0])
@pytest.mark.parametrize("H,A,n,gather", [(1, 9, 1, False), (33, 12, 65, True), (256, 48, 4097, True)])
def test_polyak_chain_is_the_float32_mirror(H, A, n, gather, tau):
    """Five updates: after each, theta- is the float32 mirror applied to the previous theta- and the critic just stepped."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    L = lh.learner(H, A, "per_sample", blob, n)
    L.set_target(tau=tau)
    assert L.get_target() == {"tau": tau, "period": None}
    t = _other(H, A)
    L._set_target_params(t)
    for k in range(5):
        L._run(n, store, cap, it, None)
        w = mirror.critic_block(L._get_params(), H, A)
        t = mirror.polyak(t, w, tau)
        got = L._get_target_params()
        assert got.tobytes() == t.tobytes(), (k, np.flatnonzero(got.view(np.int32) != t.view(np.int32))[:5])
        if tau == 1.0:
            assert got.tobytes() == w.tobytes()
    L.check()
    assert np.array_equal(lh.state(L)["step"], np.full(8, 5))


# ---- 5. the periodic rule ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,gather", [(33, 12, 65, True), (128, 12, 63, False)])
def test_periodic_copy_counts_successful_updates_on_the_device(H, A, n, gather):
    """period = 3 over seven updates, the fourth refused (an action out of range): theta- changes exactly after the 3rd
    and the 6th successful update, to the critic's bits of that moment; the refused one changes nothing and does not
    count."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    bad_actions = store["actions"].clone()
    bad_actions[int(idx[0])] = A
    bad = dict(store, actions=bad_actions)
    L = lh.learner(H, A, "reference", blob, n)
    L.set_target(period=3)
    assert L.get_target() == {"tau": None, "period": 3}
    t = mirror.critic_block(blob, H, A)
    good = 0
    for k in range(1, 8):
        before = _full(L)
        al, cl, td = L._run(n, bad if k == 4 else store, cap, it, None)
        if k == 4:
            assert torch.isnan(al) and torch.isnan(cl)
            lh.same(_full(L), before, "a refused update changes nothing")
            continue
        good += 1
        st = _full(L)
        assert np.array_equal(st["step"], np.full(8, good))
        w = mirror.critic_block(st["params"], H, A)
        assert w.tobytes() != t.tobytes()
        t = mirror.periodic(t, w, st["step"][4], 3)
        assert st["target"].tobytes() == t.tobytes(), k
        assert (t.tobytes() == w.tobytes()) == (good in (3, 6)), k
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()


def test_period_one_is_tau_one():
    H, A, n = 33, 12, 65
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    a, c = lh.learner(H, A, "per_sample", blob, n), lh.learner(H, A, "per_sample", blob, n)
    a.set_target(period=1)
    c.set_target(tau=1.0)
    for L in (a, c):
        L._set_target_params(_other(H, A))
    for k in range(3):
        lh.same(lh.update(a, n, store, cap, it, None), lh.update(c, n, store, cap, it, None), k)
        lh.same(_full(a), _full(c), k)
        assert a._get_target_params().tobytes() == mirror.critic_block(a._get_params(), H, A).tobytes()


# ---- 6. the split update and several rings -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(tau=0.3), dict(period=2)], ids=["polyak", "periodic"])
@pytest.mark.parametrize("H,A,n,gather", [(33, 12, 65, True), (256, 48, 4097, True), (128, 12, 63, False)])
def test_grad_apply_write_priorities_is_the_closed_update(H, A, n, gather, kw):
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    closed, split = lh.learner(H, A, "reference", blob, n), lh.learner(H, A, "reference", blob, n)
    for L in (closed, split):
        L.set_target(**kw)
        L._set_target_params(_other(H, A))
    pc, ps = _prio(cap), _prio(cap)
    for k in range(2):
        lh.same(lh.split_update(split, n, store, cap, it, ps), lh.update(closed, n, store, cap, it, pc), k)
        lh.same(_full(split), _full(closed), k)
    assert closed._get_target_params().tobytes() != _other(H, A).tobytes()
    # a plain learner's row of the same batch is another row: grad bootstraps from theta-
    plain = lh.learner(H, A, "reference", blob, n)
    fresh = lh.learner(H, A, "reference", blob, n)
    fresh.set_target(**kw)
    fresh._set_target_params(_other(H, A))
    assert lh.row(fresh, n, store, cap, it)[1].tobytes() != lh.row(plain, n, store, cap, it)[1].tobytes()


def test_update_from_many_is_the_rows_applied_by_hand():
    H, A, counts, k = 33, 12, (65, 40), 48
    blob = lh.init_blob(H, A, 77)

    def rings():
        out = []
        for r, cnt in enumerate(counts):
            s, a, rew, s2 = lh.batch(np.random.RandomState(100 + r), cnt, A)
            ring = _uav().PrioritizedReplayRing(cnt + 5, DEV, seed=60 + r, max_batch=64)
            ring.add({"states": torch.from_numpy(s), "actions": torch.from_numpy(a), "rewards": torch.from_numpy(rew),
                      "next_states": torch.from_numpy(s2)})
            out.append(ring)
        return out
    many, hand = lh.learner(H, A, "per_sample", blob, 64), lh.learner(H, A, "per_sample", blob, 64)
    for L in (many, hand):
        L.set_target(tau=0.25)
        L._set_target_params(_other(H, A))
    ra, rb = rings(), rings()
    for u in range(2):
        al, cl, tds = many.update_from_many(ra, k)
        drawn = [hand.grad_from(ring, k) for ring in rb]
        al2, cl2 = hand.apply([row for row, _, _ in drawn])
        for ring, (_, td, idx) in zip(rb, drawn):
            hand.write_priorities(ring, idx, td)
        assert torch.equal(al, al2) and torch.equal(cl, cl2) and torch.isfinite(al)
        for x, (_, y, _) in zip(tds, drawn):
            assert torch.equal(x, y)
        for x, y in zip(ra, rb):
            assert torch.equal(x.priorities, y.priorities)
        lh.same(_full(many), _full(hand), u)
    t = mirror.critic_block(blob, H, A)
    assert many._get_target_params().tobytes() not in (t.tobytes(), _other(H, A).tobytes())
    for x in (many, hand, *ra, *rb):
        x.check()


# ---- 7. values -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n", SHAPES)
def test_target_values_are_the_values_of_a_learner_whose_critic_is_theta(H, A, n):
    blob = lh.init_blob(H, A, 9)
    theta = _other(H, A)
    L = lh.learner(H, A, "reference", blob, 64)
    with pytest.raises(RuntimeError, match="uavtrack_learner_values_target: no target"):
        L.target.values(torch.zeros(1, 12, device=DEV))
    L.set_target(tau=0.5)
    L._set_target_params(theta)
    ref = lh.learner(H, A, "reference", mirror.with_critic(blob, H, A, theta), 64)
    x = lh.dev(np.random.RandomState(n).uniform(-3, 3, (n, 12)).astype(np.float32))
    want = ref.values(x)
    got = L.target.values(x)
    assert got.shape == (n,) and torch.equal(got, want)
    out = torch.full((n,), 7.0, device=DEV)
    assert L.target.values(x.reshape(n, 1, 12), out=out) is out and torch.equal(out, want)
    assert torch.equal(L.values(x), lh.learner(H, A, "reference", blob, 64).values(x))     # the online critic's stay
    want64 = mirror.values64(theta, H, x.cpu().numpy())
    assert np.abs(got.cpu().numpy() - want64).max() <= 1e-4 * (1 + np.abs(want64).max())


@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_lambda_ring_add_with_the_target_critic_stores_what_its_values_store(kind):
    """add_rollout(critic=learner.target) on a lambda ring == add_rollout(values=) of the target's values; T B N = 3 2 2."""
    T, B, N, H, A = 3, 2, 2, 33, 12
    rng = np.random.default_rng(8)
    obs_in = lh.dev(rng.standard_normal((B, N, 12)).astype(np.float32))
    out = {"obs": lh.dev(rng.standard_normal((T, B, N, 12)).astype(np.float32)),
           "actions": lh.dev(rng.integers(0, A, (T, B, N)).astype(np.int32)),
           "reward": lh.dev(rng.standard_normal((T, B, N)).astype(np.float32))}
    L = lh.learner(H, A, "reference", lh.init_blob(H, A, 10), 64)
    L.set_target(period=NEVER)
    L._set_target_params(_other(H, A))
    u = _uav()
    cls = u.PrioritizedReplayRing if kind == "prioritised" else u.ReplayRing

    def ring():
        return cls(40, DEV, seed=1, max_batch=16).with_lambda(0.9, GAMMA)
    a, b, c = ring(), ring(), ring()
    a.add_rollout(obs_in, out, critic=L.target)
    b.add_rollout(obs_in, out, values=L.target.values(out["obs"]))
    c.add_rollout(obs_in, out, critic=L)
    ntr = T * B * N
    assert (a.pos, a.count) == (b.pos, b.count) == (ntr, ntr)
    for key in lh.STORES:
        assert torch.equal(a.store[key][:ntr], b.store[key][:ntr]), key
    assert torch.equal(a.discounts[:ntr], b.discounts[:ntr])
    assert not torch.equal(a.store["rewards"][:ntr], c.store["rewards"][:ntr])   # the online critic folds other returns


# ---- 8. capture ------------------------------------------------------------------------------------------------------------------

def test_captured_update_from_keeps_the_periodic_schedule_across_replays():
    """update_from with period = 2, captured once on one stream and replayed four times == the eager chain, bitwise; the
    target changed on replays 2 and 4 only: the schedule runs on the device step counter."""
    H, A, cnt, k = 128, 12, 90, 64
    blob = lh.init_blob(H, A, 12)
    s, a, rew, s2 = lh.batch(np.random.RandomState(4), cnt, A)

    def fresh():
        ring = _uav().PrioritizedReplayRing(100, DEV, seed=3, max_batch=k)
        ring.add({"states": torch.from_numpy(s), "actions": torch.from_numpy(a), "rewards": torch.from_numpy(rew),
                  "next_states": torch.from_numpy(s2)})
        L = lh.learner(H, A, "per_sample", blob, k)
        L.set_target(period=2)
        return L, ring
    eager, re_ = fresh()
    graphed, rg = fresh()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(DEV)
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            g_out = graphed.update_from(rg, k, importance=True, beta=0.4)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(graphed)["step"], np.zeros(8))              # capture ran nothing
    graphed.set_target(period=NEVER)                                            # the graph keeps period = 2
    t = mirror.critic_block(blob, H, A)
    for c in range(1, 5):
        e_out = eager.update_from(re_, k, importance=True, beta=0.4)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y) and torch.isfinite(x).all(), c
        lh.same(lh.state(graphed), lh.state(eager), c)
        assert torch.equal(re_.priorities, rg.priorities)
        got = graphed._get_target_params()
        assert got.tobytes() == eager._get_target_params().tobytes(), c
        assert (got.tobytes() != t.tobytes()) == (c % 2 == 0), c
        if c % 2 == 0:
            assert got.tobytes() == mirror.critic_block(graphed._get_params(), H, A).tobytes()
        t = got
    for x in (eager, graphed, re_, rg):
        x.check()


# ---- 9. checkpoints, pack / unpack, host-side errors -------------------------------------------------------------------------------

def _trained(H, A, n, kw, loss="per_sample"):
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    L = lh.learner(H, A, loss, blob, n)
    L.set_target(**kw)
    L._set_target_params(_other(H, A))
    for _ in range(2):
        L._run(n, store, cap, it, None)
    return L, (n, store, cap, it)


@pytest.mark.parametrize("kw", [dict(tau=0.005), dict(period=3)], ids=["polyak", "periodic"])
def test_checkpoints_restore_the_target_and_its_settings(kw, tmp_path):
    H, A, n = 33, 12, 65
    src, batch = _trained(H, A, n, kw)
    assert src._get_target_params().tobytes() != mirror.critic_block(src._get_params(), H, A).tobytes()
    sd = src.state_dict()
    assert set(sd) == {"actor", "critic", "actor_optimizer", "critic_optimizer", "target_critic", "target"}
    assert list(sd["target_critic"]) == list(sd["critic"]) and sd["target"] == src.get_target() == {**dict(tau=None, period=None), **kw}
    src.save(str(tmp_path), 7)
    ck = torch.load(str(tmp_path / "critic" / "critic_weights_7.pth"), map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "target_state_dict", "target"}
    assert set(torch.load(str(tmp_path / "actor" / "actor_weights_7.pth"), map_location="cpu")) == {
        "model_state_dict", "optimizer_state_dict"}
    a = lh.learner(H, A, "per_sample", None, n)
    a.load_state_dict(sd)
    c = lh.learner(H, A, "per_sample", None, n)
    c.load(str(tmp_path / "actor" / "actor_weights_7.pth"), str(tmp_path / "critic" / "critic_weights_7.pth"))
    want = _full(src)
    for L in (a, c):
        assert L.get_target() == src.get_target()
        lh.same(_full(L), want)
    want = lh.update(src, *batch, None)
    for L in (a, c):
        lh.same(lh.update(L, *batch, None), want)
        lh.same(_full(L), _full(src))


def test_checkpoint_without_a_target_hard_syncs_and_off_keeps_todays_keys(tmp_path):
    H, A, n = 33, 12, 65
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    off = lh.learner(H, A, "reference", blob, n)
    off._run(n, store, cap, it, None)
    sd = off.state_dict()
    assert set(sd) == {"actor", "critic", "actor_optimizer", "critic_optimizer"}
    off.save(str(tmp_path), 1)
    paths = (str(tmp_path / "actor" / "actor_weights_1.pth"), str(tmp_path / "critic" / "critic_weights_1.pth"))
    assert set(torch.load(paths[1], map_location="cpu")) == {"model_state_dict", "optimizer_state_dict"}
    critic = mirror.critic_block(off._get_params(), H, A)
    for load in (lambda L: L.load_state_dict(sd), lambda L: L.load(*paths)):
        on = lh.learner(H, A, "reference", None, n)
        on.set_target(tau=0.1)
        on._set_target_params(_other(H, A))
        load(on)
        assert on.get_target() == {"tau": 0.1, "period": None}
        assert on._get_target_params().tobytes() == critic.tobytes()
        lh.same(lh.state(on), lh.state(off))
    # and a learner without a target loads it and stays without one
    plain = lh.learner(H, A, "reference", None, n)
    plain.load_state_dict(sd)
    assert plain.get_target() == {"tau": None, "period": None}


@pytest.mark.parametrize("kw", [dict(tau=0.3), dict(period=2), dict()], ids=["polyak", "periodic", "off"])
def test_pack_and_unpack_make_two_live_learners_update_identically(kw):
    from uavtrack import sharding
    H, A, n = 33, 12, 65
    if kw:
        src, batch = _trained(H, A, n, kw)
    else:
        blob, b, store, cap, idx, it = lh.case(H, A, n, True)
        src, batch = lh.learner(H, A, "per_sample", blob, n), (n, store, cap, it)
        src._run(*batch, None)
    src.set_regularisation(0.01, (0.5, None))
    dst = lh.learner(H, A, "per_sample", None, n)
    dst.set_target(tau=0.9)                                                     # settings of its own, to be replaced
    sharding.unpack_learner_state(dst, sharding.pack_learner_state(src))
    assert dst.get_target() == src.get_target() and dst.get_regularisation() == src.get_regularisation()
    lh.same(_full(dst), _full(src))
    for k in range(3):
        lh.same(lh.update(dst, *batch, None), lh.update(src, *batch, None), k)
        lh.same(_full(dst), _full(src), k)


def test_settings_and_host_side_errors():
    H, A, n = 33, 12, 65
    blob, b, store, cap, idx, it = lh.case(H, A, n, False)
    L = lh.learner(H, A, "reference", blob, n)
    lib = L._lib
    for fn in (L.sync_target, L._get_target_params, lambda: L._set_target_params(_other(H, A)), L.target_state_dict):
        with pytest.raises(RuntimeError, match="no target critic is enabled"):
            fn()
    # the library's own argument tests (Python refuses these before it calls)
    for mode, tau, period, word in ((1, 0.0, 0, "tau"), (1, 1.5, 0, "tau"), (1, float("nan"), 0, "tau"), (2, 0.0, 0, "period"),
                                    (3, 0.5, 1, "mode")):
        assert lib.uavtrack_learner_set_target(L._h, mode, tau, period, L._stream()) != 0
        msg = lib.uavtrack_last_error().decode()
        assert msg.startswith("uavtrack_learner_set_target: ") and word in msg, msg
        assert L.get_target() == {"tau": None, "period": None}
    L.set_target(tau=0.3)
    theta = _other(H, A)
    L._set_target_params(theta)
    with pytest.raises(RuntimeError, match="floats"):
        L._set_target_params(theta[:-1])
    # changing tau, the period or the rule keeps theta-; off and on again hard-copies
    for kw in (dict(tau=0.7), dict(period=4), dict(tau=0.2)):
        L.set_target(**kw)
        assert L._get_target_params().tobytes() == theta.tobytes()
    sd = L.target_state_dict()
    assert [tuple(v.shape) for v in sd.values()] == [(H, 12), (H,), (1, H), (1,)]
    assert np.concatenate([v.numpy().ravel() for v in sd.values()]).tobytes() == theta.tobytes()
    L.set_target()
    L.set_target(tau=0.2)
    assert L._get_target_params().tobytes() == mirror.critic_block(blob, H, A).tobytes()
    L._set_target_params(theta)
    L._run(n, store, cap, it, None)
    L.sync_target()
    assert L._get_target_params().tobytes() == mirror.critic_block(L._get_params(), H, A).tobytes()
    L.check()


# ---- 10. the example ---------------------------------------------------------------------------------------------------------------

def test_example_trains_with_a_target_critic(capsys):
    """examples/train_maac.py --target-tau / --target-period: the device learner over two shards with --td-lambda (the add
    folding with the target's values, and with the online critic's under --lambda-critic online) and the torch learner
    train; both flags at once, a bad value and --lambda-critic without a target are refused with a message."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_maac
    common = ["--envs", "64", "--steps", "20", "--iters", "2", "--batch", "4096", "--updates", "2"]
    for extra in (["--replay", "prioritized", "--learner", "device", "--shards", "2", "--td-lambda", "0.9", "--target-period", "3"],
                  ["--replay", "prioritized", "--learner", "device", "--td-lambda", "0.9", "--target-tau", "0.05",
                   "--lambda-critic", "online"],
                  ["--replay", "uniform-device", "--learner", "torch", "--td-lambda", "0.9", "--target-tau", "0.05"],
                  ["--replay", "prioritized", "--learner", "torch", "--target-period", "3"]):
        hist = train_maac.main(common + extra)
        assert len(hist) == 2 and np.isfinite(hist).all(), extra
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == 2 and all(np.isfinite(float(ln.split("critic loss")[1].split()[0])) for ln in lines), extra
    for extra, word in ((["--target-tau", "0.1", "--target-period", "3"], "not allowed with"), (["--target-tau", "1.5"], "(0, 1]"),
                        (["--target-period", "0"], ">= 1"), (["--lambda-critic", "online", "--target-tau", "0.1"], "--td-lambda")):
        with pytest.raises(SystemExit):
            train_maac.main(common + extra)
        assert word in capsys.readouterr().err, extra
