"""The MAAC-R mix on the device (pmi_mix_kernel<WS>, ep_reward_kernel, and the pair slots the rollout hands it) against
fp64, across score spreads.  Scenes, bounds and the ladder: maacr_mix_mirror.py; that the scenes keep their margins, show
their graphs and reach the pool's branches: test_maacr_mix_cpu.py.  Nothing is set aside by margin here.

Leg A: one teacher-forced step per scene against the oracle inside leg_a_bound, on the rungs where the scorer's own
allowance stays small (c = 0, 1).
Leg B: the device's reward against mix_fp64 of the device's OWN scores -- float32(la_i) * float32(la_j) of the launch's
obs rows, the single IEEE multiply the scorer does, through env.pmi_inference, which runs the same launch_pmi_score as
the chunk (pmi_kernel.hip: every scorer takes one pair per matrix row, the products are its only input and the reduction
over hidden units has a fixed order, so a pair's score depends on its twelve products alone) -- and the device's own raw
rewards, inside leg_b_bound on every rung.  A mix without the max shift, with a wrong log2(e), or reading the score of
another pair of the same UAV fails it from c = 64 up.
"""
import os

import numpy as np
import pytest
import torch

import maacr_mix_mirror as mm
from conftest import GOLDEN, pmi_forward_fp64
from oracle import OracleConfig, OracleEnv, OraclePmi
from test_hip_parity import ATOL, host

pytestmark = pytest.mark.gpu

REPORT = bool(os.environ.get("UAVTRACK_TEST_REPORT"))


@pytest.fixture(scope="module")
def uavtrack():
    import uavtrack
    return uavtrack


@pytest.fixture(scope="module")
def sd0():
    z = np.load(os.path.join(GOLDEN, "pmi_h64.npz"))
    return {k: z[k] for k in z.files if k != "meta"}


def make_env(uavtrack, kw, st=None):
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(reward_mode=uavtrack.RewardMode.PMI, **kw))
    if st is not None:
        env.set_state(**st)
    return env


def device_scores(env, obs, nbs_per_env):
    """Device scores of every ordered neighbour pair of every environment: {(i, j): score} per environment."""
    keys, xs = zip(*(mm.pair_inputs(obs[b], nbs) for b, nbs in enumerate(nbs_per_env)))
    x = np.concatenate(xs)
    s = env.pmi_inference(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64) if len(x) else np.zeros(0)
    out, at = [], 0
    for k in keys:
        out.append(dict(zip(k, s[at:at + len(k)])))
        at += len(k)
    return out


def leg_b(poses, nbs, scores, raw, reward, coop):
    """One environment -> (worst err / bound over its rows, the mirror's rewards)."""
    want, _ = mm.mix_fp64(poses, raw, scores, coop=coop)
    return float((np.abs(reward.astype(np.float64) - want) / mm.leg_b_bound(nbs, raw)).max()), want


@pytest.mark.parametrize("N,M,dim", mm.SHAPES)
def test_mix_against_oracle_and_against_own_scores(uavtrack, sd0, N, M, dim):
    worst_a, worst_b = 0.0, {c: 0.0 for c in mm.RUNGS}
    for kind in mm.KINDS:
        names, st, _ = mm.scenes_of(N, M, dim, kind)
        B = len(names)
        act = mm.rigid_actions(1, B, N, dim)
        geo = None            # poses, neighbour sets and obs rows do not depend on coop or the rung: formed once
        for coop in mm.COOPS:
            kw = mm.config_kwargs(N, M, dim, kind, coop, B)
            env = make_env(uavtrack, kw)
            orc = OracleEnv(OracleConfig(**kw), n_threads=4)
            scores = {}
            for c in mm.RUNGS:
                sd = mm.spread_ladder(sd0, c)
                env.set_pmi(sd)
                env.set_state(**st)
                before = env.pmi_info()["rescored_chunks"]
                out = env.step_many(torch.from_numpy(act), want_raw=True)
                rew, raw, obs = (out[k][0].cpu().numpy() for k in ("reward", "raw", "obs"))
                if geo is None:
                    pos = host(env.get_state())
                    poses = [mm.poses_of(pos, b, dim) for b in range(B)]
                    geo = (poses, [mm.neighbour_sets(p) for p in poses], obs)
                poses, nbs, obs0 = geo
                assert np.array_equal(obs, obs0)
                if c not in scores:
                    scores[c] = device_scores(env, obs, nbs)
                assert env.pmi_info()["rescored_chunks"] == before
                assert np.isfinite(rew).all()
                for b in range(B):
                    ratio, _ = leg_b(poses[b], nbs[b], scores[c][b], raw[b], rew[b], coop)
                    worst_b[c] = max(worst_b[c], ratio)
                    assert ratio <= 1.0, ("leg B", kind, names[b], coop, c, ratio)
                mean = out["ep_sums"][:, 0].cpu().numpy().astype(np.float64)
                for b in range(B):
                    assert abs(mean[b] - rew[b].astype(np.float64).mean()) <= mm.sum_bound(rew[b], N), (kind, names[b], coop, c)
                if c in mm.LEG_A_RUNGS:
                    orc.pmi = OraclePmi.from_state_dict(sd)
                    orc.set_state(**st)
                    ref = orc.step(act[0])
                    opos = orc.get_state()
                    for b in range(B):
                        onb = mm.neighbour_sets(mm.poses_of(opos, b, dim))
                        assert all(np.array_equal(p, q) for p, q in zip(onb, nbs[b])), (kind, names[b])
                        keys, x = mm.pair_inputs(ref["obs"][b], onb, np.float64)
                        mag = pmi_forward_fp64(sd, x, want_scale=True)[1] if keys else np.zeros(0)
                        bound = mm.leg_a_bound(onb, ref["raw"][b], dict(zip(keys, mag)), coop, ATOL)
                        ratio = float((np.abs(rew[b] - ref["reward"][b]) / bound).max())
                        worst_a = max(worst_a, ratio)
                        assert ratio <= 1.0, ("leg A", kind, names[b], coop, c, ratio)
            env.close()
    if REPORT:
        print(f"[maacr-mix] N{N} M{M} dim{dim}: worst err / bound leg A {worst_a:.3f}, leg B "
              + ", ".join(f"c={c}: {v:.3f}" for c, v in worst_b.items()), flush=True)


@pytest.mark.parametrize("T,B", [(1, 1), (1, 12), (1, 13), (3, 5)])
def test_instance_groups_at_the_edges_of_a_workgroup(uavtrack, sd0, T, B):
    """20 x 10: E = 3 instances per group, 4 groups per workgroup -- S * B below, equal to and one above E * 4, and not a
    multiple of it.  Every row inside leg B on the top rung; rows of instances without neighbours are bit for bit what
    the rollout left there, clip((1 - a) raw) in fp32."""
    N, M, coop = 20, 10, 0.3
    assert mm.mix_geometry(N)[1:3] == (3, 4)
    names, st, _ = mm.build_scenes(N, M)
    pick = [(names.index("empty") + b) % len(names) for b in range(B)]       # the empty scene first, then around the batch
    st = {k: np.ascontiguousarray(v[pick]) for k, v in st.items()}
    kw = mm.config_kwargs(N, M, 2, "open", coop, B)
    env = make_env(uavtrack, kw, st)
    env.set_pmi(mm.spread_ladder(sd0, mm.TOP_RUNG))
    out = env.step_many(torch.from_numpy(mm.rigid_actions(T, B, N)), want_raw=True)
    pos = host(env.get_state())
    rew, raw, obs = (out[k].cpu().numpy() for k in ("reward", "raw", "obs"))
    lonely = 0
    for b in range(B):
        poses = mm.poses_of(pos, b, 2)
        nbs = mm.neighbour_sets(poses)          # (the swarm is rigid: the final poses' graph is every step's)
        for t in range(T):
            scores = device_scores(env, obs[t, b:b + 1], [nbs])[0]
            ratio, _ = leg_b(poses, nbs, scores, raw[t, b], rew[t, b], coop)
            assert ratio <= 1.0, (T, B, b, t, ratio)
            alone = np.array([len(nb) == 0 for nb in nbs])
            left = np.clip((np.float32(1.0) - np.float32(coop)) * raw[t, b], np.float32(-1.0), np.float32(1.0))
            assert rew[t, b][alone].tobytes() == left[alone].tobytes(), (T, B, b, t)
            lonely += int(alone.sum())
    assert lonely >= T * N                      # the empty scene at least
    want = rew.astype(np.float64).mean(axis=2).sum(axis=0)
    got = out["ep_sums"][:, 0].cpu().numpy().astype(np.float64)
    for b in range(B):
        assert abs(got[b] - want[b]) <= mm.sum_bound(rew[:, b], N), (T, B, b)
    env.close()


@pytest.mark.parametrize("N,M,E", mm.POOL_SHAPES)
def test_pooled_launches_equal_single_steps_and_pass_leg_b(uavtrack, sd0, N, M, E):
    """The LONE variant's pooled pair slots on the scenes that reach every branch of the pool (test_maacr_mix_cpu.py): a
    launch of T = 16, 17, 32, 36 steps equals T single steps bit for bit; the single steps pass leg B on the top rung; the
    pairs scored are the oracle's non-isolated ones."""
    coop, Tmax = 0.3, max(mm.POOL_LAUNCHES)
    sd = mm.spread_ladder(sd0, mm.TOP_RUNG)
    kw = mm.config_kwargs(N, M, 2, "open", coop, E)
    for name, st in mm.pool_scenes(N, M, E).items():
        act = mm.rigid_actions(Tmax, E, N)
        orc = OracleEnv(OracleConfig(**kw), n_threads=4)
        orc.set_state(**st)
        pairs = []
        for t in range(Tmax):
            orc.step(act[t])
            pos = orc.get_state()
            pairs.append(sum(mm.wave_runs([mm.poses_of(pos, e, 2) for e in range(E)])))
        single = make_env(uavtrack, kw, st)
        single.set_pmi(sd)
        assert single.kernel_info()["envs_per_workgroup"] == E
        p0 = single.pmi_pairs_scored()
        steps = []
        for t in range(Tmax):
            out = single.step_many(torch.from_numpy(act[t:t + 1]), want_raw=True)
            pos = host(single.get_state())
            rew, raw, obs = (out[k][0].cpu().numpy() for k in ("reward", "raw", "obs"))
            poses = [mm.poses_of(pos, e, 2) for e in range(E)]
            nbs = [mm.neighbour_sets(p) for p in poses]
            scores = device_scores(single, obs, nbs)      # (stand-alone scoring: not in the rollout's pair count)
            for e in range(E):
                ratio, _ = leg_b(poses[e], nbs[e], scores[e], raw[e], rew[e], coop)
                assert ratio <= 1.0, (name, t, e, ratio)
            steps.append((out["reward"][0].clone(), out["obs"][0].clone()))
        assert single.pmi_pairs_scored() - p0 == sum(pairs), name
        single.close()
        for T in mm.POOL_LAUNCHES:
            env = make_env(uavtrack, kw, st)
            env.set_pmi(sd)
            q0 = env.pmi_pairs_scored()
            fused = env.step_many(torch.from_numpy(act[:T]))
            assert env.variant_info()[-1] == 1 and env.launch_info()["single_wavefront_variant"] == 1, (name, T)
            assert env.pmi_pairs_scored() - q0 == sum(pairs[:T]), (name, T)
            for t in range(T):
                assert torch.equal(fused["reward"][t], steps[t][0]) and torch.equal(fused["obs"][t], steps[t][1]), (name, T, t)
            env.close()


@pytest.mark.parametrize("B", [1, 15, 17])
def test_episode_return_against_fp64_of_the_final_rewards(uavtrack, sd0, monkeypatch, B):
    """ep_sums[:, 0] against the fp64 sum over the steps of the fp64 mean of the device's own final rewards, inside
    sum_bound: through one call, through a call scored in several chunks (a 1 MiB scratch budget, B > 1: one more addition
    per chunk, counted by the library's own profile of mix launches and asserted above 1 at S = 33) and through step(..., ep_sums=) accumulation (one more per step).  test_hip_parity holds the three
    routes to each other and to torch's fp32 sums at 1e-5; this holds each to fp64 at the bound of its own arithmetic."""
    N, M, coop = 20, 10, 0.3
    _, st, _ = mm.dense_scenes(N, M, B=B, seed=7)
    kw = mm.config_kwargs(N, M, 2, "dense", coop, B)
    sd = mm.spread_ladder(sd0, 64)
    rng = np.random.RandomState(B)
    for S in (1, 15, 16, 17, 33):
        act = rng.randint(0, 12, size=(S, B, N)).astype(np.int32)
        env = make_env(uavtrack, kw, st)
        env.set_pmi(sd)
        many = env.step_many(torch.from_numpy(act))
        rew = many["reward"].cpu().numpy()
        want = rew.astype(np.float64).mean(axis=2).sum(axis=0)

        def check(got, extra, route):
            got = got.cpu().numpy().astype(np.float64)
            for b in range(B):
                bound = mm.sum_bound(rew[:, b], N, extra)
                assert abs(got[b] - want[b]) <= bound, (route, S, b, abs(got[b] - want[b]) / bound)
        check(many["ep_sums"][:, 0], 0, "one call")
        env.close()
        if B > 1:     # (one environment's steps all fit 1 MiB: that would be the one-call route again)
            with monkeypatch.context() as mp:
                mp.setenv("UAVTRACK_PMI_SCRATCH_MB", "1")
                env = make_env(uavtrack, kw, st)
                env.set_pmi(sd)
                env.set_profiling(True)
                env.profile()
                chunked = env.step_many(torch.from_numpy(act))
                prof = env.profile()
            chunks = prof["mix"]["launches"]                   # one mix launch per chunk: the library's own count
            assert prof["ep_sums"]["launches"] == chunks and 1 <= chunks <= S, prof
            if S == 33:
                assert chunks >= 2, (B, S, chunks)             # the route really is chunked where it is meant to be
            assert torch.equal(chunked["reward"], many["reward"])
            check(chunked["ep_sums"][:, 0], chunks, "chunked")
            env.close()
        env = make_env(uavtrack, kw, st)
        env.set_pmi(sd)
        acc = torch.zeros(B, 5, device="cuda")
        for t in range(S):
            _, r, _ = env.step(torch.from_numpy(act[t]), ep_sums=acc)
            assert torch.equal(r, many["reward"][t])
        check(acc[:, 0], S, "accumulated")
        env.close()
