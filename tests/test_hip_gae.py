"""Fixed GAE advantages on the MI355X: the GAE ring add (uavtrack_replay_add_rollout_gae) bitwise against the numpy mirror
(tests/replay_gae_mirror.py) over all seven stores and the priorities, and against the lambda add on the same inputs; the
learner on stored advantages (uavtrack_learner_update_stored / _grad_stored) bitwise against the plain per-sample update
where the store holds that update's td_delta, and against the float64 mirror where it does not; the device refusal; the
sweep under graph capture and update_from_many."""
import numpy as np
import pytest
import torch

import learner_advantage_mirror as lam
import learner_harness as lh
import learner_mirror as mirror
import replay_gae_mirror as gm
import replay_sweep_mirror as smirror
import ring_rollout_harness as rr

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA
SENTINEL_ADV = np.float32(-55.5)


def _uav():
    import uavtrack
    return uavtrack


# ---- 1. the add against the mirror ---------------------------------------------------------------------------------------

# T either side of the scan's load group of 8 (1 and 7: the one-at-a-time steps alone; 8: one group alone; 9 and 17: both,
# one and two groups); 3 x 2 chains: below one wavefront, 33 x 2 = 66: across one.
STEPS = (1, 7, 8, 9, 17)
AGENTS = ((3, 2), (33, 2))
LAM_GAMMA = ((0.0, 0.95), (0.9, 0.95), (1.0, 0.95), (0.9, 0.0))

_rollouts = {}


def _rollout(T, B, N):
    if (T, B, N) not in _rollouts:
        rng = np.random.default_rng(T * 100 + B)
        r = dict(obs_in=rng.standard_normal((B, N, 12)).astype(np.float32),
                 obs=rng.standard_normal((T, B, N, 12)).astype(np.float32),
                 actions=rng.integers(0, 12, (T, B, N)).astype(np.int32),
                 reward=(rng.standard_normal((T, B, N)) * 3).astype(np.float32),
                 start_obs=rng.standard_normal((T, B, N, 12)).astype(np.float32),
                 values=(rng.standard_normal((T, B, N)) * 4).astype(np.float32),
                 values_in=(rng.standard_normal((B, N)) * 4).astype(np.float32),
                 values_start=(rng.standard_normal((T, B, N)) * 4).astype(np.float32))
        r["dev"] = {k: lh.dev(v) for k, v in r.items()}
        _rollouts[T, B, N] = r
    return _rollouts[T, B, N]


def _dones(T, B):
    """name -> done [T][B] or None.  "mixed": environment 0 fires at t = 0, environment 1 at T - 2 and at T - 1 (two
    consecutive steps, the second the rollout's last), environment 2 at two consecutive steps in the middle."""
    mixed = np.zeros((T, B), np.uint8)
    mixed[0, 0] = 1
    mixed[max(T - 2, 0):, 1] = 1
    if T >= 5:
        mixed[2:4, 2] = 1
    last = np.zeros((T, B), np.uint8)
    last[T - 1, 1] = 1
    return {"null": None, "zeros": np.zeros((T, B), np.uint8), "mixed": mixed, "last": last}


def _rings(n):
    """name -> (capacity, pos, count): roomy; a window that wraps; a ring smaller than the rollout (the skip path), its
    window wrapping too."""
    return {"roomy": (n + 50, 10, 10), "wrap": (n + 50, n + 47, n + 50), "small": (n // 2 + 1, n // 4 + 1, n // 2 + 1)}


def _image(ring):
    img = rr.image(ring)
    img["advantages"] = ring.advantages.cpu().numpy().copy()
    return img


def _same_image(a, b):
    rr.same_image(a, b)
    assert a["advantages"].tobytes() == b["advantages"].tobytes(), "advantages"


def _out(r, done):
    d = r["dev"]
    out = {k: d[k] for k in ("obs", "actions", "reward")}
    if done is not None:
        out.update(done=lh.dev(done), start_obs=d["start_obs"])
    return out


@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
@pytest.mark.parametrize("B,N", AGENTS)
@pytest.mark.parametrize("T", STEPS)
def test_add_against_the_mirror_bitwise(T, B, N, kind):
    u = _uav()
    r = _rollout(T, B, N)
    n = T * B * N
    carried = 0
    for ringcase, (cap, pos, count) in _rings(n).items():
        ring = (u.PrioritizedReplayRing if kind == "prioritised" else u.ReplayRing)(cap, DEV, seed=1, max_batch=8)
        for done_kind, done in _dones(T, B).items():
            for lam, gamma in LAM_GAMMA:
                ring.with_gae(lam, gamma)
                rr.prefill(ring, pos, count)
                ring.advantages.fill_(float(SENTINEL_ADV))
                img = _image(ring)
                d = r["dev"]
                ring.add_rollout_gae(d["obs_in"], _out(r, done), values=d["values"], values_in=d["values_in"],
                                     values_start=None if done is None else d["values_start"])
                tr = gm.transitions(r["obs_in"], r["obs"], r["actions"], r["reward"], r["values"], r["values_in"],
                                    None if done is None else r["values_start"], lam, gamma, done,
                                    None if done is None else r["start_obs"])
                p2, c2 = gm.ring_add(img, pos, count, tr)
                assert (ring.pos, ring.count) == (p2, c2)
                _same_image(_image(ring), img)
                assert ring._last == ((pos + max(0, n - cap)) % cap, min(n, cap)), (ringcase, done_kind)
                written = img["advantages"] != SENTINEL_ADV
                assert written.sum() == min(n, cap)
                assert (img["discounts"][written].view(np.int32) == 0).all()       # +0.0, never -0.0
                carried += int((tr["rewards"] != (r["reward"] + np.float32(gamma) * r["values"]).reshape(-1)).sum())
    assert carried > 0 or T == 1                                          # some return carried a tail


def test_states_and_priorities_are_the_lambda_adds_and_the_reward_is_its_pair_folded_once():
    u = _uav()
    T, B, N = 9, 33, 2
    r = _rollout(T, B, N)
    n = T * B * N
    done = _dones(T, B)["mixed"]
    d = r["dev"]
    for cap, pos, count in (_rings(n)["roomy"], _rings(n)["small"]):
        a = u.PrioritizedReplayRing(cap, DEV, seed=1, max_batch=8).with_gae(0.9, GAMMA)
        b = u.PrioritizedReplayRing(cap, DEV, seed=1, max_batch=8).with_lambda(0.9, GAMMA)
        for ring in (a, b):
            rr.prefill(ring, pos, count)
        a.add_rollout_gae(d["obs_in"], _out(r, done), values=d["values"], values_in=d["values_in"],
                          values_start=d["values_start"])
        b.add_rollout(d["obs_in"], _out(r, done), values=d["values"])
        ia, ib = rr.image(a), rr.image(b)
        rr.same_image(ia, ib, ("states", "actions", "next_states", "priorities"))
        k = min(n, cap)
        slots = torch.from_numpy((a._last[0] + np.arange(k)) % cap).to(DEV)
        v = d["values"].reshape(-1)[n - k:]                                # the window holds the rollout's last k rows
        want = b.store["rewards"][slots] + b.discounts[slots] * v           # two torch kernels: each rounded on its own
        assert torch.equal(a.store["rewards"][slots], want)
        assert (a.discounts[slots].view(torch.int32) == 0).all()


def test_critic_form_runs_the_three_value_passes_into_buffers_the_ring_keeps():
    u = _uav()
    T, B, N = 9, 3, 2
    r = _rollout(T, B, N)
    done = _dones(T, B)["mixed"]
    d = r["dev"]
    L = lh.learner(32, 12, "per_sample", lh.init_blob(32, 12, 3), max_batch=64)
    a = u.ReplayRing(200, DEV, seed=1, max_batch=8).with_gae(0.9, GAMMA)
    b = u.ReplayRing(200, DEV, seed=1, max_batch=8).with_gae(0.9, GAMMA)
    for ring in (a, b):
        rr.prefill(ring, 0, 0)                                           # the same sentinels outside the window
    a.add_rollout(d["obs_in"], _out(r, done), critic=L)
    held = [a._values.data_ptr(), a._values_in.data_ptr(), a._values_start.data_ptr()]
    b.add_rollout_gae(d["obs_in"], _out(r, done), values=L.values(d["obs"]).reshape(-1),
                      values_in=L.values(d["obs_in"]).reshape(-1), values_start=L.values(d["start_obs"]).reshape(-1))
    _same_image(_image(a), _image(b))
    a.add_rollout(d["obs_in"], _out(r, done), critic=L)                   # the buffers are kept, not allocated again
    assert held == [a._values.data_ptr(), a._values_in.data_ptr(), a._values_start.data_ptr()]
    batch = a.sample(8)
    assert set(batch) == {"states", "actions", "rewards", "next_states", "discounts", "advantages"}
    assert set(a.sweep(8).sample()) == set(batch)
    assert torch.isfinite(batch["advantages"]).all()
    a.add({k: batch[k] for k in lh.STORES})                              # a flat add: advantages unknown
    assert torch.isnan(a.advantages[a._last[0]:a._last[0] + 8]).all()


# ---- 2. the learner on stored advantages, bitwise --------------------------------------------------------------------------

H, A = 32, 12
MODES = ("raw", "clip0", "clip0.2", "weights", "target", "batch")


def _configured(mode, blob, n):
    L = lh.learner(H, A, "per_sample", blob, max_batch=n)
    if mode == "target":
        L.set_target(tau=0.25)
        L._set_target_params(mirror.critic_block(lh.init_blob(H, A, 77), H, A))   # a target that is not the critic
    if mode == "batch":
        L.set_advantage("batch")
    return L


def _options(mode, c, n):
    """(weights, log_mu, clip_eps) of a mode, device tensors."""
    w = lh.dev(lam.weights(n)) if mode == "weights" else None
    if mode.startswith("clip"):
        return w, lh.dev(c.log_mu), float(mode[4:])
    return w, None, None


@pytest.mark.parametrize("n", [2, 255, 256, 257])
@pytest.mark.parametrize("mode", MODES)
def test_a_store_of_td_delta_leaves_the_plain_update_and_grad_apply_equals_the_closed_form(mode, n):
    c = lam.host_case(H, A, n, True)
    store = {k: lh.dev(x) for k, x in zip(lh.STORES, c.b)}
    it = lh.dev(c.idx)
    w, log_mu, eps = _options(mode, c, n)
    plain = _configured(mode, c.blob, n)
    prio = torch.ones(c.cap, device=DEV)
    al, cl, td = plain._run(n, store, c.cap, it, prio, w, None, log_mu, eps)
    plain.check()
    want = lh._result(plain, n, al, cl, td, prio)
    # the store: NaN (unknown) everywhere but the drawn slots, which hold the bits of that update's td_delta
    x = np.full(c.cap, np.nan, np.float32)
    x[c.idx] = want["td"]
    adv = lh.dev(x)
    stored = _configured(mode, c.blob, n)
    prio2 = torch.ones(c.cap, device=DEV)
    al2, cl2, td2 = stored._run(n, store, c.cap, it, prio2, w, None, log_mu, eps, None, adv)
    stored.check()
    got = lh._result(stored, n, al2, cl2, td2, prio2)
    keys = ("params", "exp_avg", "exp_avg_sq", "step", "td", "critic_loss", "prio")
    lh.same({k: got[k] for k in keys}, {k: want[k] for k in keys}, mode)
    assert not np.array_equal(got["params"], c.blob)
    if mode == "batch":
        s_plain, s_stored = plain.advantage_stats.cpu().numpy(), stored.advantage_stats.cpu().numpy()
        ref = lam.stats32(want["td"][np.arange(n)])                       # the gathered values, in batch order
        assert s_stored[0] == ref[0], (s_stored, ref)                      # the existing contract: mean exact,
        assert lam.ulps(s_stored[1], ref[1]) <= 1 and lam.ulps(s_stored[2], ref[2]) <= 1   # inv_std and std one ulp
        assert s_stored.tobytes() == s_plain.tobytes()
    # the split form of the same stored update
    split = _configured(mode, c.blob, n)
    prio3 = torch.ones(c.cap, device=DEV)
    row, td3 = split._grad(n, store, c.cap, it, None, None, w, None, log_mu, eps, None, adv)
    assert row.numel() == split.num_params + 8
    al3, cl3 = split.apply(row)
    import types
    split.write_priorities(types.SimpleNamespace(priorities=prio3, capacity=c.cap), it, td3)
    split.check()
    lh.same(lh._result(split, n, al3, cl3, td3, prio3), got, mode + " split")


# ---- 3. the learner on stored advantages against float64 -------------------------------------------------------------------

def _stored_row64(c, x, weights=None, clip=None, theta=None, critic_fed_x=False, actor_fed_delta=False):
    """One gradient row in float64 with the actor's advantage x [n] (batch order) in delta's place: learner_mirror's
    forward, terms, backward.  The two flags are the two miswirings the comparison must see."""
    f = mirror.forward(c.blob, c.H, c.A, *lam.rows(c), GAMMA, theta)
    delta = f.delta
    f.delta = delta if actor_fed_delta else np.asarray(x, np.float64)
    gz, gv, lt, ratio = mirror.terms(f, "per_sample", weights, 0.0, clip)
    f.delta = delta
    iw = np.ones(f.n) if weights is None else np.asarray(weights, np.float64)
    lt[1] = delta * iw
    if critic_fed_x:
        gv = -np.asarray(x, np.float64) * iw
    return {"g": mirror.backward(f, gz, gv), "loss": lt.sum(axis=1), "n": f.n, "td": delta}


@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clip0.2"])
@pytest.mark.parametrize("Hc,Ac,n,gather", lam.SHAPES)
def test_gradient_row_against_fp64_with_advantages_unrelated_to_delta(Hc, Ac, n, gather, clipped):
    c = lam.host_case(Hc, Ac, n, gather)
    rng = np.random.RandomState(n + 91)
    x_store = (rng.standard_normal(c.cap) * 2).astype(np.float32)         # nothing to do with delta
    x = x_store[c.idx]
    w = lam.weights(n)
    clip = (c.log_mu[c.idx], lam.EPS_CLIP) if clipped else None
    store = {k: lh.dev(v) for k, v in zip(lh.STORES, c.b)}
    it = lh.dev(c.idx) if gather else None
    L = lh.learner(Hc, Ac, "per_sample", c.blob, max_batch=n)
    row, td = L._grad(n, store, c.cap, it, None, None, lh.dev(w), None, lh.dev(c.log_mu) if clipped else None,
                      lam.EPS_CLIP if clipped else None, None, lh.dev(x_store))
    L.check()
    row, td = row.cpu().numpy(), td.cpu().numpy()
    P = L.num_params
    assert int(row[P + 6:P + 7].view(np.int32)[0]) == 0 and int(row[P + 7:P + 8].view(np.int32)[0]) == P
    ref = _stored_row64(c, x, w, clip)
    ral, rcl, rg = mirror.combine([ref], Hc, Ac, "per_sample")
    dev_row = {"g": row[:P].astype(np.float64), "loss": row[P:P + 4].astype(np.float64), "n": n}
    al, cl, g = mirror.combine([dev_row], Hc, Ac, "per_sample")
    # learner_harness's bounds as they are; the actor-loss scale is that of |x| here, so it is given mean |x| as its delta
    lh.assert_losses_and_td(al, cl, td, ral, rcl, ref["td"])
    tol = lh.tol_g(n, rg)
    err = np.abs(g - rg)
    print(f"share of the gradient bound: {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), float((err / tol).max())
    # teeth: either miswiring is far outside the bound, on the block it touches
    na = mirror.layout(Hc, Ac)[1][4]
    bad_critic = mirror.combine([_stored_row64(c, x, w, clip, critic_fed_x=True)], Hc, Ac, "per_sample")[2]
    bad_actor = mirror.combine([_stored_row64(c, x, w, clip, actor_fed_delta=True)], Hc, Ac, "per_sample")[2]
    assert np.abs(g - bad_critic)[na:].max() > 100 * tol and np.array_equal(bad_critic[:na], rg[:na])
    assert np.abs(g - bad_actor)[:na].max() > 100 * tol and np.array_equal(bad_actor[na:], rg[na:])


# ---- 4. the refusal --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_one_bad_advantage_in_a_drawn_slot_refuses_the_update(bad):
    n = 257
    c = lam.host_case(H, A, n, True)
    store = {k: lh.dev(x) for k, x in zip(lh.STORES, c.b)}
    it = lh.dev(c.idx)
    x = np.ones(c.cap, np.float32)
    x[c.idx[200]] = bad
    L = lh.learner(H, A, "per_sample", c.blob, max_batch=n)
    before = lh.state(L)
    row, _ = L._grad(n, store, c.cap, it, None, None, None, None, None, None, None, lh.dev(x))
    P = L.num_params
    assert int(row.cpu().numpy()[P + 6:P + 7].view(np.int32)[0]) == 128
    al, cl = L.apply(row)
    assert torch.isnan(al) and torch.isnan(cl)
    prio = torch.ones(c.cap, device=DEV)
    al, cl, td = L._run(n, store, c.cap, it, prio, None, None, None, None, None, lh.dev(x))
    assert torch.isnan(al) and torch.isnan(cl) and (prio == 1).all()
    lh.same(lh.state(L), before)
    with pytest.raises(RuntimeError, match="2 update"):
        L.check()
    L.check()                                                            # the count restarts
    x[c.idx[200]] = 1.0                                                  # an unknown advantage in a slot NOT drawn is fine
    x[np.setdiff1d(np.arange(c.cap), c.idx)[0]] = np.nan
    L._run(n, store, c.cap, it, prio, None, None, None, None, None, lh.dev(x))
    L.check()
    assert not np.array_equal(L._get_params(), before["params"])


# ---- 5. sweep, graph capture, update_from_many -----------------------------------------------------------------------------

HS, CAP, K = 64, 512, 128


def _twins(seed):
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        out.append(_uav().DeviceActorCritic(12, HS, 12, 1e-3, 5e-3, 0.95, DEV, loss="per_sample", max_batch=K))
    return out


def _gae_ring(rng, seed, learner, T=8):
    """512 slots behind a rollout of T * 64 transitions with episode ends, log_mu and advantages from `learner`."""
    B, N = 8, 8
    obs_in = lh.dev(rng.randn(B, N, 12).astype(np.float32))
    out = {"obs": lh.dev(rng.randn(T, B, N, 12).astype(np.float32)),
           "actions": lh.dev(rng.randint(0, 12, (T, B, N)).astype(np.int32)),
           "reward": lh.dev(rng.randn(T, B, N).astype(np.float32)),
           "done": lh.dev((rng.rand(T, B) < 0.2).astype(np.uint8)),
           "start_obs": lh.dev(rng.randn(T, B, N, 12).astype(np.float32))}
    ring = _uav().ReplayRing(CAP, DEV, seed=seed, max_batch=K).with_gae(0.9, 0.95).with_behaviour()
    ring.add_rollout_behaviour(obs_in, out, behaviour=learner, critic=learner)
    return ring


def test_captured_sweep_update_over_a_gae_ring_equals_the_eager_calls():
    la, lb = _twins(5)
    ra, rb = (_gae_ring(np.random.RandomState(9), 31, L) for L in (la, lb))
    assert torch.equal(ra.advantages, rb.advantages) and torch.isfinite(ra.advantages).all()
    sa, sb = ra.sweep(K, window="last"), rb.sweep(K, window="last")
    E, M = 2, sa.minibatches
    assert M == 4
    la.update_from(sa, K, clip_eps=0.2)                                   # warm-up, eager: call 0
    lb.update_from(sb, K, clip_eps=0.2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ga, gc, gtd = la.update_from(sa, K, clip_eps=0.2)
    for call in range(1, E * M):
        g.replay()
        b_a, b_c, b_td = lb.update_from(sb, K, clip_eps=0.2)
        torch.cuda.synchronize()
        assert torch.equal(sa._idx, sb._idx), call
        assert torch.equal(ga, b_a) and torch.equal(gc, b_c) and torch.equal(gtd, b_td), call
        # and the eager call is the stored update of the mirror's rows: the ring's advantages, not delta, reach the actor
        first, W = sb.window
        idx = smirror.sweep_call(CAP, first, W, K, 31, call)
        assert np.array_equal(sb._idx.cpu().numpy(), idx)
    assert np.array_equal(la._get_params(), lb._get_params())
    la.check(); lb.check()
    # advantages that were NOT picked up would leave another learner: the same calls on a ring without the store
    lc, _ = _twins(5)
    rc = _gae_ring(np.random.RandomState(9), 31, lc)
    rc.advantages = None
    sc = rc.sweep(K, window="last")
    for _ in range(E * M):
        lc.update_from(sc, K, clip_eps=0.2)
    assert not np.array_equal(lc._get_params(), lb._get_params())


def test_update_from_many_over_two_gae_rings_equals_the_two_rows_applied_by_hand():
    la, lb = _twins(6)
    rings_a = [_gae_ring(np.random.RandomState(11 + r), 40 + r, la, T=4 + 4 * r) for r in range(2)]
    rings_b = [_gae_ring(np.random.RandomState(11 + r), 40 + r, lb, T=4 + 4 * r) for r in range(2)]
    for call in range(3):
        al, cl, tds = la.update_from_many(rings_a, K, clip_eps=0.2)
        rows = lb.new_rows(2)
        ref = [lb.grad_from(ring, K, rows[r], clip_eps=0.2)[1] for r, ring in enumerate(rings_b)]
        b_al, b_cl = lb.apply(rows)
        assert torch.equal(al, b_al) and torch.equal(cl, b_cl)
        assert all(torch.equal(x, y) for x, y in zip(tds, ref))
        assert np.array_equal(la._get_params(), lb._get_params())
    la.check(); lb.check()


# ---- 6. the example --------------------------------------------------------------------------------------------------------

def test_example_trains_on_fixed_gae_advantages(capsys):
    """examples/train_maac.py --gae-lambda 0.95 --ppo-epochs 2: the device learner over two shards with the clipped
    surrogate and standardised advantages, and the torch learner (its critic module passed to the add) train; without
    --ppo-epochs, with --td-lambda and with the reference loss on the device it is refused with a message."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_maac
    common = ["--envs", "64", "--steps", "20", "--iters", "2", "--gae-lambda", "0.95", "--ppo-clip", "0.2"]
    epochs = ["--ppo-epochs", "2", "--minibatch", "4096"]
    for extra in (["--replay", "prioritized", "--learner", "device", "--actor-loss", "per_sample", "--shards", "2",
                   "--normalise-advantage"],
                  ["--replay", "uniform-device", "--learner", "torch"]):
        hist = train_maac.main(common + epochs + extra)
        assert len(hist) == 2 and np.isfinite(hist).all(), extra
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == 2 and all(np.isfinite(float(ln.split("critic loss")[1].split()[0])) for ln in lines), extra
    for extra, words in ((["--replay", "prioritized", "--batch", "4096"], ("--ppo-epochs",)),
                         (epochs + ["--replay", "prioritized", "--td-lambda", "0.9"], ("--td-lambda", "one of the three")),
                         (epochs + ["--replay", "prioritized", "--learner", "device"], ("per_sample",))):
        with pytest.raises(SystemExit):
            train_maac.main(common + extra)
        err = capsys.readouterr().err
        assert all(w in err for w in words), err
