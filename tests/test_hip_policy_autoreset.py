"""The fused policy rollouts across episode ends (uavtrack_run_actor_autoreset, uavtrack_run_greedy_autoreset), their
start_obs output, the episodes add of the replay ring, and the drivers above them.

Shapes: 5 x 3 (specialised kernel) and 7 x 4 (generic), B = 37 (the last workgroup is partly filled), horizon 4, T = 11
with the step counts staggered over the environments (resets fire at different t inside one workgroup; every
environment turns over at least twice and the launch ends mid-episode), actor widths 128 and 32.  The policy seed is
2^64 - 6 and the episodes start at 5, so seed + e wraps inside every launch.

Every comparison is bitwise.  One exception is stated where it is made: in MAAC-R the chain test compares the return
column of ep_sums through the given-actions launch of the anchor test (the mix stage sums it), not through the
restated register sums."""
import numpy as np
import pytest
import torch

import episode_stats_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H, T, EP0 = 37, 4, 11, 5
SEED, RESET = 2 ** 64 - 6, 99
SENTINEL = -777.25
OUT_KEYS = ("actions", "obs", "reward", "terms", "covered", "done")

# (policy, N, M, mode, dim, hidden): every actor mode in 2-D and 3-D on both shapes, the two widths alternating so each
# meets both shapes and both dimensions; the greedy baseline where it exists (2-D, RAW / MEAN)
CASES = [("actor", N, M, mode, dim, (128, 32)[(k + j + (dim == 3)) % 2])
         for k, (N, M) in enumerate(((5, 3), (7, 4))) for j, mode in enumerate(("RAW", "MEAN", "PMI")) for dim in (2, 3)]
CASES += [("greedy", N, M, mode, 2, 0) for N, M in ((5, 3), (7, 4)) for mode in ("RAW", "MEAN")]
IDS = ["-".join(str(v) for v in c) for c in CASES]
_cache = {}


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def make_cfg(N, M, mode, dim, horizon=H, n_envs=B):
    import uavtrack
    return uavtrack.EnvConfig(n_envs=n_envs, n_uav=N, m_targets=M, cooperative=0.0 if mode == "RAW" else 0.3,
                              reward_mode=getattr(uavtrack.RewardMode, mode), horizon=horizon, env_offset=500, dim=dim,
                              nc=3 if dim == 3 else 1)


def make_actor(cfg, hidden):
    import uavtrack
    torch.manual_seed(hidden + cfg.n_uav)
    actor = uavtrack.ActorMLP(hidden_dim=hidden, action_dim=cfg.na_total)
    with torch.no_grad():
        actor.fc2.weight.mul_(5.0)      # (probabilities away from uniform)
    return actor


def make_env(case, pmi_sd, **kw):
    import uavtrack
    policy, N, M, mode, dim, hidden = case
    cfg = make_cfg(N, M, mode, dim, **kw)
    env = uavtrack.BatchedUavEnv(cfg, DEV)
    if mode == "PMI":
        env.set_pmi(pmi_sd)
    if policy == "actor":
        env.set_actor(make_actor(cfg, hidden))
    return env


def stagger(env, h=H):
    """reset(3, episode 5), then step counts b % h; returns the reset's observation (what the policy sees first)."""
    obs = env.reset(seed=3, episode=EP0)
    st = env.get_state()
    st["step_count"] = torch.arange(env.B, dtype=torch.int32, device=DEV) % h
    env.set_state(**st)
    return obs


def run(env, case, T_, obs_in, seed, **kw):
    if case[0] == "actor":
        return env.run_actor(T_, obs_in, seed=seed, want_terms=True, **kw)
    return env.run_greedy(T_, seed=seed, **kw)


def sentinel_start_obs(env, T_=T):
    return torch.full((T_, env.B, env.N, 12), SENTINEL, device=DEV)


def launch(case, pmi_sd):
    """The automatic-reset launch of a case, its hand-built chain, and what both started from -- computed once."""
    if case in _cache:
        return _cache[case]
    a, b, c = (make_env(case, pmi_sd) for _ in range(3))
    obs0 = stagger(a)
    assert torch.equal(stagger(b), obs0)
    fused = run(a, case, T, obs0, SEED, auto_reset_seed=RESET, want_start_obs=True, out=dict(start_obs=sentinel_start_obs(a)))
    fused = {k: v.clone() for k, v in fused.items()}
    final_a = a.get_state()

    # the chain: per step, per episode number present in the batch, one T = 1 call of the existing entry point with
    # seed + e on the whole batch, of which the environments in episode e are kept; a finished environment becomes
    # reset(RESET, e + 1) and goes on from that call's observation
    chain = {k: torch.empty_like(fused[k]) for k in OUT_KEYS}
    want_start = sentinel_start_obs(b)
    cur = obs0.clone()
    episode = torch.full((B,), EP0, dtype=torch.int64)
    first_of_episode = []                                    # (t, environments mask, e): step t is the first of episode e
    for t in range(T):
        st = b.get_state()
        new = {k: v.clone() for k, v in st.items()}
        for e in episode.unique().tolist():
            b.set_state(**st)
            r = run(b, case, 1, cur, SEED + e)
            pick = (episode == e).to(DEV)
            for k in OUT_KEYS:
                if k == "terms":
                    chain[k][t][:, pick] = r[k][0][:, pick]
                else:
                    chain[k][t][pick] = r[k][0][pick]
            after = b.get_state()
            for k in new:
                new[k][pick] = after[k][pick]
        cur = chain["obs"][t].clone()
        d = chain["done"][t].bool().cpu()
        if d.any():
            episode[d] += 1
            for e in episode[d].unique().tolist():
                fresh_obs = c.reset(seed=RESET, episode=int(e))
                fresh = c.get_state()
                pick = (d & (episode == e)).to(DEV)
                for k in new:
                    new[k][pick] = fresh[k][pick]
                cur[pick] = fresh_obs[pick]
                want_start[t][pick] = fresh_obs[pick]
                first_of_episode.append((t + 1, pick, int(e)))
        b.set_state(**new)
    res = dict(case=case, fused=fused, chain=chain, want_start=want_start, obs0=obs0, final_a=final_a,
               final_b=b.get_state(), first_of_episode=first_of_episode, scratch=c)
    for e in (a, b):
        e.close()
    _cache[case] = res
    return res


def ep_sums_restated(out, N, pmi):
    """ep_sums [B, 5] as the rollout kernel forms it, from per-step outputs: each UAV's fp32 running sum over the steps,
    those added in ascending UAV index in fp32, times fl32(1 / N); the covered counts as an integer.  (MAAC-R: column 0
    is the mix stage's and is left NaN here.)"""
    rew = out["reward"].cpu().numpy()
    terms = out["terms"].cpu().numpy()
    planes = [rew, terms[:, 0], terms[:, 1], terms[:, 2]]
    ep = np.full((rew.shape[1], 5), np.nan, np.float32)
    inv_n = np.float32(1.0) / np.float32(N)
    for k, p in enumerate(planes):
        if k == 0 and pmi:
            continue
        acc = np.zeros(p.shape[1:], np.float32)
        for t in range(p.shape[0]):
            acc = acc + p[t]
        s = np.zeros(p.shape[1], np.float32)
        for i in range(N):
            s = s + acc[:, i]
        ep[:, k] = s * inv_n
    ep[:, 4] = out["covered"].cpu().numpy().sum(axis=0).astype(np.float32)
    return ep


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_launch_equals_chain_of_existing_calls(case, pmi_state_dict):
    """Test 1.  actions, obs, reward, terms, covered, done, the final state (with every environment's episode number)
    and ep_sums; start_obs rows at fired steps are the reset call's observation, the others keep the sentinel."""
    r = launch(case, pmi_state_dict)
    fused, chain = r["fused"], r["chain"]
    done = fused["done"].bool()
    assert int(done.sum(dim=0).min()) >= 2 and not bool(done[-1].all())        # everyone turned over twice; the launch ends mid-episode
    assert len({int(t) for t in done.any(dim=1).nonzero().flatten()}) >= H     # ... at different steps
    for k in OUT_KEYS:
        assert torch.equal(fused[k], chain[k]), (case, k, (fused[k] != chain[k]).nonzero()[:4].tolist())
    for k in r["final_a"]:
        assert torch.equal(r["final_a"][k], r["final_b"][k]), (case, k)
    assert torch.equal(r["final_a"]["episode"].cpu(), (EP0 + done.sum(dim=0)).to(torch.int32).cpu())
    assert torch.equal(fused["start_obs"], r["want_start"]), case
    fired = done[:, :, None, None].expand_as(fused["start_obs"])
    assert bool((fused["start_obs"][~fired] == SENTINEL).all()) and not bool((fused["start_obs"][fired] == SENTINEL).any())
    pmi = case[3] == "PMI"
    want = ep_sums_restated(chain, case[1], pmi)
    got = fused["ep_sums"].cpu().numpy()
    cols = slice(1, 5) if pmi else slice(0, 5)
    assert got[:, cols].tobytes() == want[:, cols].tobytes(), (case, got[:2], want[:2])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_anchored_to_the_given_actions_path(case, pmi_state_dict):
    """Test 2.  The launch's own actions through step_many(auto_reset_seed) from the same start reproduce every output,
    ep_sums and the final state; the first action of each new episode is the stand-alone actor kernel's on the
    start_obs row with seed + e."""
    r = launch(case, pmi_state_dict)
    fused = r["fused"]
    g = make_env(case, pmi_state_dict)
    stagger(g)
    given = g.step_many(fused["actions"], auto_reset_seed=RESET)
    for k in ("obs", "reward", "terms", "covered", "done", "ep_sums"):
        assert torch.equal(given[k], fused[k]), (case, k)
    final = g.get_state()
    for k in final:
        assert torch.equal(final[k], r["final_a"][k]), (case, k)
    g.close()
    if case[0] != "actor":
        return
    c = r["scratch"]
    seen = 0
    for t, pick, e in r["first_of_episode"]:
        if t >= T:
            continue
        c.reset(seed=1, episode=0)                            # step counts 0, as behind the in-launch reset
        rows = torch.where(pick[:, None, None], fused["start_obs"][t - 1], torch.zeros_like(r["obs0"]))
        acts = c.actor_actions(rows.contiguous(), seed=SEED + e)
        assert torch.equal(acts[pick], fused["actions"][t][pick]), (case, t, e)
        seen += int(pick.sum())
    assert seen >= B


@pytest.mark.parametrize("case", [CASES[0], CASES[9], CASES[-1]], ids=[IDS[0], IDS[9], IDS[-1]])
def test_plain_launches_ignore_an_installed_buffer(case, pmi_state_dict):
    """Test 3.  run_actor / run_greedy without the automatic reset: the same bytes with and without a start_obs buffer
    installed, and the buffer is never written -- also through want_start_obs."""
    outs = []
    for installed in (False, True, "want"):
        env = make_env(case, pmi_state_dict)
        obs0 = stagger(env)
        buf = sentinel_start_obs(env)
        kw = {}
        if installed is True:
            env.set_start_obs_output(buf)
        elif installed == "want":
            kw = dict(want_start_obs=True, out=dict(start_obs=buf))
        res = run(env, case, T, obs0, SEED, **kw)
        assert ("start_obs" in res) == (installed == "want")
        assert bool((buf == SENTINEL).all())
        outs.append(({k: res[k].clone() for k in OUT_KEYS + ("ep_sums",)}, env.get_state(), env.variant_info()))
        env.close()
    for other in outs[1:]:
        for k in outs[0][0]:
            assert torch.equal(outs[0][0][k], other[0][k]), (case, k)
        for k in outs[0][1]:
            assert torch.equal(outs[0][1][k], other[1][k]), (case, k)
        assert outs[0][2] == other[2]                          # ... on the same kernel variant


def _rings(capacity, prefill):
    import uavtrack
    rings = [uavtrack.PrioritizedReplayRing(capacity, DEV, seed=1) for _ in range(2)]
    g = torch.Generator(DEV).manual_seed(7)
    pre = dict(states=torch.randn(prefill, 12, device=DEV, generator=g), next_states=torch.randn(prefill, 12, device=DEV, generator=g),
               actions=torch.randint(0, 12, (prefill,), dtype=torch.int32, device=DEV, generator=g),
               rewards=torch.randn(prefill, device=DEV, generator=g))
    for r in rings:
        for v in r.store.values():
            v.zero_()
        r.add(pre)
        r.priorities[:min(prefill, capacity)] = torch.linspace(0.5, 3.0, min(prefill, capacity), device=DEV)
    return rings


def _same_ring(x, y):
    assert (x.pos, x.count) == (y.pos, y.count)
    for k in x.store:
        assert torch.equal(x.store[k], y.store[k]), k
    assert torch.equal(x.priorities, y.priorities)


# n = 11 * 37 * 5 = 2035 transitions, 185 agents per step: a ring that holds them all; one smaller than n and no multiple
# of the agents, entered at slot 300 (the window starts mid-step and wraps); one of a single step and a bit
@pytest.mark.parametrize("capacity,prefill", [(4096, 300), (1000, 300), (191, 50)])
def test_replay_add_across_episodes(capacity, prefill, pmi_state_dict):
    """Test 4.  add_rollout on the launch's result == add(transitions_from_rollout(...)), byte for byte over the whole
    ring; with done zeroed it equals the add_rollout of a result without start_obs."""
    import uavtrack
    r = launch(CASES[0], pmi_state_dict)
    fused, obs0 = r["fused"], r["obs0"]
    dev, ref = _rings(capacity, prefill)
    dev.add_rollout(obs0, fused)
    tr = uavtrack.transitions_from_rollout(obs0, fused)
    plain = uavtrack.transitions_from_rollout(obs0, {k: fused[k] for k in ("obs", "actions", "reward")})
    assert not torch.equal(tr["states"], plain["states"]) and not bool((tr["states"] == SENTINEL).any())
    ref.add(tr)
    _same_ring(dev, ref)
    dev, old = _rings(capacity, prefill)
    dev.add_rollout(obs0, dict(fused, done=torch.zeros_like(fused["done"])))
    old.add_rollout(obs0, {k: fused[k] for k in ("obs", "actions", "reward")})
    _same_ring(dev, old)


def test_episode_stats_on_the_launch(pmi_state_dict):
    """Test 5a.  EpisodeStats.add on the launch: the records of the numpy mirror applied to the launch's own outputs, in
    (t, b) order -- environment by environment within a step, an environment's episodes in order."""
    import uavtrack
    case = CASES[2]
    r = launch(case, pmi_state_dict)
    fused = r["fused"]
    stats = uavtrack.EpisodeStats((B, case[1]), log_capacity=4 * B, max_steps=T, env_offset=500, device=DEV)
    stats.add(fused)
    m = mirror.EpisodeStatsMirror(B, case[1], 4 * B, env_offset=500)
    m.add(*(fused[k].cpu().numpy() for k in ("reward", "terms", "covered", "done")))
    rec, dropped = stats.read_records()
    assert dropped == 0 and rec.tobytes() == m.records().tobytes()
    done = fused["done"].cpu().numpy()
    tb = np.argwhere(done)                                  # (t, b) ascending: the documented order
    assert rec["env"].tolist() == (500 + tb[:, 1]).tolist()
    first = np.array([H - b % H for b in range(B)])          # steps of each environment's first (staggered) episode
    want_steps = [int(first[b]) if t < H and t + 1 == first[b] else H for t, b in tb]
    assert rec["steps"].tolist() == want_steps
    assert rec["ordinal"].tolist() == [int(done[:t, b].sum()) for t, b in tb]
    stats.destroy()


@pytest.mark.parametrize("case", [CASES[2], CASES[-1]], ids=[IDS[2], IDS[-1]])
def test_evaluate_in_one_launch(case, pmi_state_dict):
    """Test 5b.  evaluate(auto_reset=True): the records of the hand-reset chain -- reset(seed, e), run with seed + e --
    fed through EpisodeStats."""
    import uavtrack
    policy, N, M, mode, dim, hidden = case
    E, S = 3, 21
    cfg = make_cfg(N, M, mode, dim)
    pol = "greedy" if policy == "greedy" else make_actor(cfg, hidden)
    env = uavtrack.BatchedUavEnv(cfg, DEV)
    res = uavtrack.evaluate(env, pol, num_steps=H, episodes=E, seed=S, auto_reset=True)
    assert res["path"] == "auto_reset" and res["dropped"] == 0 and len(res["return_list"]) == E * B
    assert res["env"].tolist() == list(range(500, 500 + B)) * E and res["steps"].tolist() == [H] * (E * B)
    hand = uavtrack.BatchedUavEnv(cfg, DEV)
    if policy == "actor":
        hand.set_actor(pol)
    stats = uavtrack.EpisodeStats(hand, log_capacity=E * B, max_steps=H)
    for e in range(E):
        obs = hand.reset(seed=S, episode=e)
        stats.add(run(hand, case, H, obs, S + e))
    want = stats.read()
    for key, _ in uavtrack.episode_stats.RESULT_KEYS:
        assert res[key].tobytes() == want[key].tobytes(), key
    for key in ("env", "steps", "ordinal"):
        assert res[key].tolist() == want[key].tolist(), key
    with pytest.raises(ValueError, match="horizon"):
        uavtrack.evaluate(env, pol, num_steps=H + 1, episodes=E, seed=S, auto_reset=True)
    stats.destroy(); env.close(); hand.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[-2]], ids=[IDS[1], IDS[4], IDS[-2]])
def test_captured_launch_replays_like_eager_calls(case, pmi_state_dict):
    """Test 6.  The launch captured in a graph (which refuses an allocation or a synchronisation) and replayed twice
    equals two eager calls.  The eager side goes through bind_run (arguments built once, on the stream current then),
    the captured side through run_actor / run_greedy into the same kind of buffers (the stream current at the call: the
    capture's)."""
    a, b = make_env(case, pmi_state_dict), make_env(case, pmi_state_dict)
    obs0 = stagger(a)
    stagger(b)
    policy = case[0]
    keys = OUT_KEYS + ("ep_sums", "start_obs")

    def bound(env):
        first = run(env, case, T, obs0, SEED, auto_reset_seed=RESET, want_start_obs=True)      # (also sizes the MAAC-R scratch)
        out = {k: torch.empty_like(v) for k, v in first.items()}
        out["start_obs"].fill_(SENTINEL)
        return out, env.bind_run(T, out, policy, obs_in=obs0, seed=SEED, auto_reset_seed=RESET, want_start_obs=True)
    out_a, call_a = bound(a)
    out_b, _ = bound(b)
    want = []
    for _ in range(2):
        call_a()
        want.append({k: out_a[k].clone() for k in keys})
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = run(b, case, T, obs0, SEED, auto_reset_seed=RESET, want_start_obs=True, out=out_b)
    assert all(res[k] is out_b[k] for k in keys)              # every buffer was reused: nothing was allocated
    torch.cuda.synchronize()
    for k in range(2):
        g.replay()
        for key in keys:
            assert torch.equal(out_b[key], want[k][key]), (case, k, key)
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    a.close(); b.close()


def test_refusals_enqueue_nothing(pmi_state_dict):
    """Test 7.  horizon == 0; a start_obs capacity below T; the greedy baseline in 3-D and under MAAC-R (the combinations
    without a rollout kernel, named in the message): an error, the state and the outputs untouched.  want_start_obs
    without the automatic reset is accepted (test 3)."""
    import uavtrack

    def refused(env, match, fn):
        before = env.get_state()
        out = dict(reward=torch.full((T, env.B, env.N), SENTINEL, device=DEV),
                   obs=torch.full((T, env.B, env.N, 12), SENTINEL, device=DEV))
        with pytest.raises(RuntimeError, match=match):
            fn(env, out)
        torch.cuda.synchronize()
        after = env.get_state()
        for k in before:
            assert torch.equal(before[k], after[k]), k
        assert bool((out["reward"] == SENTINEL).all()) and bool((out["obs"] == SENTINEL).all())
        env.close()

    actor_case = CASES[0]
    env = make_env(actor_case, pmi_state_dict, horizon=0)
    obs = env.reset(seed=1)
    refused(env, "no horizon", lambda e, out: e.run_actor(T, obs, auto_reset_seed=RESET, out=out))
    env = make_env(("greedy", 5, 3, "RAW", 2, 0), pmi_state_dict, horizon=0)
    env.reset(seed=1)
    refused(env, "no horizon", lambda e, out: e.run_greedy(T, auto_reset_seed=RESET, out=out))

    env = make_env(actor_case, pmi_state_dict)
    obs2 = env.reset(seed=1)
    small = sentinel_start_obs(env, T - 1)
    def too_small(e, out):
        e.set_start_obs_output(small)
        e.run_actor(T, obs2, auto_reset_seed=RESET, out=out)
    refused(env, "start-observation buffer", too_small)
    assert bool((small == SENTINEL).all())

    for mode, dim, match in (("RAW", 3, r"policy greedy, reward mode MAAC, 3-D"), ("PMI", 2, r"policy greedy, reward mode MAAC-R, 2-D")):
        env = make_env(("greedy", 5, 3, mode, dim, 0), pmi_state_dict)
        env.reset(seed=1)
        refused(env, match, lambda e, out: e.run_greedy(T, auto_reset_seed=RESET, out=out))


def test_chunked_maacr_launch_equals_the_single_chunk(pmi_state_dict, monkeypatch):
    """Test 8.  An automatic-reset MAAC-R launch split into several chunks (UAVTRACK_PMI_SCRATCH_MB=1: two to four steps
    per chunk at 70 x 20 x 10) against the same launch in one chunk: run_actor with start_obs and the target trace,
    step_many with the target trace and the raw rewards.  Horizon 5, T = 19, step counts b % 5: a done flag fires at every
    step, chunk edges included.  Everything bitwise, the final state with it, but ep_sums: the chunks add their float
    sums in another order (rtol = atol = 1e-6, as the chunked comparison of tests/test_hip_parity.py)."""
    case, Hc, Tc = ("actor", 20, 10, "PMI", 2, 128), 5, 19
    g = torch.Generator(DEV).manual_seed(4)
    given = torch.randint(0, 12, (Tc, 70, 20), dtype=torch.int32, device=DEV, generator=g)

    def play(scratch_mb):
        # (the library reads the variable whenever it sizes the scratch: at set_pmi and at a launch longer than it holds)
        if scratch_mb is None:
            monkeypatch.delenv("UAVTRACK_PMI_SCRATCH_MB", raising=False)
        else:
            monkeypatch.setenv("UAVTRACK_PMI_SCRATCH_MB", str(scratch_mb))
        env = make_env(case, pmi_state_dict, horizon=Hc, n_envs=70)
        env.set_profiling(True)
        res = []
        for form in ("run_actor", "step_many"):
            obs0 = stagger(env, Hc)
            env.profile()
            if form == "run_actor":
                r = env.run_actor(Tc, obs0, seed=SEED, auto_reset_seed=RESET, want_start_obs=True, want_targets=True,
                                  out=dict(start_obs=sentinel_start_obs(env, Tc)))
            else:
                r = env.step_many(given, auto_reset_seed=RESET, want_targets=True, want_raw=True)
            launches = env.profile()["rollout"]["launches"]
            res.append(({k: v.clone() for k, v in r.items()}, env.get_state(), launches))
        env.close()
        return res

    chunked, whole = play(1), play(None)
    keys = (("actions", "obs", "reward", "terms", "covered", "done", "start_obs", "targets", "ep_sums"),
            ("obs", "reward", "terms", "covered", "done", "targets", "raw", "ep_sums"))
    for form, (a, sa, la), (b, sb, lb), want_keys in zip(("run_actor", "step_many"), chunked, whole, keys):
        assert la >= 3 and lb == 1, (form, la, lb)            # a chunk behind the second ran: kAutoResetContinued
        assert set(a) == set(b) == set(want_keys), (form, sorted(a), sorted(b))
        done = a["done"].bool()
        assert bool(done.any(dim=1).all()), form               # a reset at every step of the launch
        for k in want_keys:
            if k == "ep_sums":
                torch.testing.assert_close(a[k], b[k], rtol=1e-6, atol=1e-6, msg=lambda m: f"{form} ep_sums: {m}")
            else:
                assert torch.equal(a[k], b[k]), (form, k, (a[k] != b[k]).nonzero()[:4].tolist())
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (form, k)
        if form == "run_actor":
            fired = done[:, :, None, None].expand_as(a["start_obs"])
            assert bool((a["start_obs"][~fired] == SENTINEL).all()) and not bool((a["start_obs"][fired] == SENTINEL).any())
