"""The greedy baseline policy on the device -- the stand-alone greedy_policy_kernel (csrc/policy_kernel.hip), csrc/greedy.h
and the POLICY = greedy rollout variants -- against the fp64 oracle on the shape cases and the hand-made scenes of
tests/greedy_scenes.py, and the fused launches against the stand-alone kernel, bit for bit.

What is set aside: only scoring-branch decisions the oracle's per-UAV verdict (uav_oracle.h, `robust`) calls uncertain,
at most 10 % per case (greedy_scenes.CAP; tests/test_greedy_cpu.py holds the same cap on the oracle's own states).  The
hand-made scenes are compared without any set-aside.
"""
import numpy as np
import pytest
import torch

import greedy_scenes as gs
from oracle import OracleConfig, OracleEnv, greedy_actions
from test_hip_parity import host, inject

pytestmark = pytest.mark.gpu

GREEDY = 1                       # kPolicyGreedy, slot 4 of variant_info()
T = 3


@pytest.fixture(scope="module")
def uavtrack():
    import uavtrack
    return uavtrack


def make_env(uavtrack, s, coop=0.0, **over):
    return uavtrack.BatchedUavEnv(uavtrack.EnvConfig(env_offset=s.env_offset, cooperative=coop, **{**gs.shape_config(s), **over}))


def advance(env, s):
    """reset and the case's random-action steps (step_count > 0)."""
    env.reset(seed=s.seed)
    for act in gs.shape_actions(s):
        env.step(torch.from_numpy(act))


# ---- the stand-alone kernel against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("s", gs.SHAPES, ids=gs.SHAPE_IDS)
def test_standalone_kernel_vs_oracle(uavtrack, s):
    env = make_env(uavtrack, s)
    try:
        advance(env, s)
        st = host(env.get_state())
        assert (st["step_count"] == s.steps).all()
        orc = OracleEnv(OracleConfig(**gs.shape_config(s)))
        inject(orc, st)
        got = env.greedy_actions(seed=gs.POLICY_SEED).cpu().numpy()
        want, aid = greedy_actions(orc, gs.POLICY_SEED, st["step_count"], env_offset=s.env_offset)
        bad, scoring = gs.set_aside(aid)
        print(f"\n[greedy set-aside, device state] {s.name}: {bad} / {scoring} = {bad / max(scoring, 1):.4f}")
        assert bad <= gs.CAP * scoring, (s.name, bad, scoring)
        assert got.min() >= 0 and got.max() < s.na
        rnd = aid["branch"] == 0
        assert rnd.any() and (aid["branch"] == 1).any()
        np.testing.assert_array_equal(got[rnd], want[rnd], err_msg=f"{s.name}: random actions are pure Philox")
        ok = aid["robust"]
        assert aid["robust"][aid["branch"] != 2].all()
        np.testing.assert_array_equal(got[ok], want[ok], err_msg=f"{s.name}: robust decisions")
    finally:
        env.close()


# ---- the hand-made scenes: exact, nothing set aside ----------------------------------------------------------------------
@pytest.mark.parametrize("sc", gs.SCENES + [gs.NEAR_DC], ids=gs.SCENE_IDS + [gs.NEAR_DC.name])
def test_constructed_scene(uavtrack, sc):
    B = 6
    kw = gs.scene_config(sc, B)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(env_offset=3, **kw))
    try:
        env.reset(seed=1)
        sc_count = np.arange(B, dtype=np.int32)
        env.set_state(**gs.scene_state(sc, B), step_count=sc_count)
        orc = OracleEnv(OracleConfig(**kw))
        inject(orc, host(env.get_state()))
        steered = 0
        for seed in range(5):
            got = env.greedy_actions(seed=seed).cpu().numpy()
            ref, aid = greedy_actions(orc, seed, sc_count, env_offset=3)
            steer = aid["branch"] == 2
            np.testing.assert_array_equal(got[steer], gs.scene_want(sc, ref)[steer], err_msg=f"{sc.name} seed {seed}: hand-written answer")
            np.testing.assert_array_equal(got, ref, err_msg=f"{sc.name} seed {seed}: oracle")
            steered += int(steer[:, [w is not None for w in sc.want]].sum())
        assert steered >= 5, (sc.name, steered)
    finally:
        env.close()


# ---- fused == stand-alone, bit for bit ------------------------------------------------------------------------------------
# Rollout families (csrc/step_kernel.hip): specialised kernels (20 x 10, 50 x 25, 5 x 3), the generic kernel (every other
# shape), and a single environment whose tables exceed the 64 KiB a launch gets without asking -- 3 x 4096: the target
# table alone is 16 M bytes, the per-target words 8 M more, 98 304 B (lds_bytes_for) -- which asks for the CU's larger limit.
SPECIALISED = {(20, 10), (50, 25), (10, 10), (5, 3)}
FUSED = [(s, mode, 0) for s in gs.SHAPES for mode in ("raw", "mean")]
# forced workgroup sizes (UAVTRACK_WGS) on one shape of each family; plan_geometry honours a size that holds a whole environment
FUSED += [(s, mode, w) for s in gs.SHAPES if s.name in ("dense_20x10", "na9", "n3_m4096")
          for mode, w in (("raw", 64), ("mean", 512))]
FUSED += [(s, "raw", 512) for s in gs.SHAPES if s.name == "n256"]
FUSED_IDS = [f"{s.name}-{mode}-wgs{w or 'own'}" for s, mode, w in FUSED]


def _assert_family(env, s, wgs):
    v, li = env.variant_info(), env.launch_info()
    assert v[4] == GREEDY and v[3] == 0, v
    assert v[:2] == ((s.N, s.M) if (s.N, s.M) in SPECIALISED else (0, 0)), (s.name, v)
    if wgs:
        assert li["workgroup"] == wgs, f"{s.name}: UAVTRACK_WGS={wgs} was ignored ({li})"
    ki = env.kernel_info()
    assert bool(ki["specialised"]) == ((s.N, s.M) in SPECIALISED)
    if s.name == "n3_m4096":
        assert li["envs_per_workgroup"] == 1 and ki["lds_bytes"] > 64 * 1024, (li, ki)
    return li


@pytest.mark.parametrize("s,mode,wgs", FUSED, ids=FUSED_IDS)
def test_fused_rollout_equals_standalone_steps(uavtrack, monkeypatch, s, mode, wgs):
    """run_greedy(T = 3) == T x (greedy_actions, step): actions, observations, rewards, coverage, final state."""
    if wgs:
        monkeypatch.setenv("UAVTRACK_WGS", str(wgs))
    else:
        monkeypatch.delenv("UAVTRACK_WGS", raising=False)
    coop = 0.0 if mode == "raw" else 0.3
    a, b = make_env(uavtrack, s, coop), make_env(uavtrack, s, coop)
    try:
        advance(a, s); advance(b, s)
        fused = a.run_greedy(T, seed=gs.POLICY_SEED)
        _assert_family(a, s, wgs)
        for t in range(T):
            act = b.greedy_actions(seed=gs.POLICY_SEED)
            assert torch.equal(act, fused["actions"][t]), f"{s.name}: actions of step {t}"
            obs, rew, _ = b.step(act)
            assert torch.equal(obs, fused["obs"][t]) and torch.equal(rew, fused["reward"][t]), (s.name, t)
            assert torch.equal(b.info["covered"], fused["covered"][t]), (s.name, t)
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (s.name, k)
        assert int(sa["step_count"][0]) == s.steps + T
    finally:
        a.close(); b.close()


AUTORESET = [(s, mode) for s, mode in zip([x for x in gs.SHAPES if x.name in ("dense_20x10", "na9", "n3_m4096", "n257", "offset_2p32")],
                                          ("raw", "mean", "raw", "mean", "mean"))]


@pytest.mark.parametrize("s,mode", AUTORESET, ids=[f"{s.name}-{m}" for s, m in AUTORESET])
def test_autoreset_rollout_crosses_a_reset_like_the_standalone_chain(uavtrack, monkeypatch, s, mode):
    """run_greedy_autoreset, horizon 2, T = 3, every environment at step 0 of episode 0: steps 0 and 1 draw with the key
    seed + 0, the second ends the episode, the state becomes reset(reset_seed, episode 1), and step 2 draws with seed + 1
    at step_count 0 (include/uavtrack.h).  The chain of stand-alone calls says the same, bit for bit."""
    monkeypatch.delenv("UAVTRACK_WGS", raising=False)
    coop = 0.0 if mode == "raw" else 0.3
    seed, reset_seed = 2 ** 64 - 1, 41                       # seed + 1 wraps to key 0
    a, b = make_env(uavtrack, s, coop, horizon=2), make_env(uavtrack, s, coop, horizon=2)
    try:
        a.reset(seed=s.seed, episode=0); b.reset(seed=s.seed, episode=0)
        fused = a.run_greedy(T, seed=seed, auto_reset_seed=reset_seed)
        v = a.variant_info()
        assert v[4] == GREEDY and v[6] == 1, v
        done = fused["done"].bool().cpu().numpy()
        assert not done[0].any() and done[1].all() and not done[2].any()
        for t in range(T):
            act = b.greedy_actions(seed=(seed + (t == 2)) % 2 ** 64)
            assert torch.equal(act, fused["actions"][t]), f"{s.name}: actions of step {t}"
            obs, rew, _ = b.step(act)
            assert torch.equal(obs, fused["obs"][t]) and torch.equal(rew, fused["reward"][t]), (s.name, t)
            if t == 1:
                b.reset(seed=reset_seed, episode=1)
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (s.name, k)
        assert (sa["episode"] == 1).all() and (sa["step_count"] == 1).all()
    finally:
        a.close(); b.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_enqueue_nothing(uavtrack):
    """The baseline is planar and runs with the MAAC / MAAC-G rewards.  uavtrack_greedy_actions and uavtrack_run_greedy
    refuse a 3-D handle, uavtrack_run_greedy a MAAC-R handle, each naming the reason; the state and the caller's buffers
    stay as they were.  (uavtrack_run_greedy_autoreset: tests/test_hip_policy_autoreset.py, test_refusals_enqueue_nothing.)
    The stand-alone policy does not read the reward mode: include/uavtrack.h documents uavtrack_greedy_actions as
    "2-D only", and on a MAAC-R handle it gives the actions of the MAAC handle."""
    SENT = -7
    kw = dict(n_envs=9, n_uav=5, m_targets=3)

    def refused(env, match, fn):
        env.reset(seed=2)
        before = env.get_state()
        acts = torch.full((T, env.B, env.N), SENT, dtype=torch.int32, device="cuda")
        rew = torch.full((T, env.B, env.N), float(SENT), device="cuda")
        with pytest.raises(RuntimeError, match=match):
            fn(env, acts, rew)
        torch.cuda.synchronize()
        after = env.get_state()
        for k in before:
            assert torch.equal(before[k], after[k]), k
        assert bool((acts == SENT).all()) and bool((rew == SENT).all())
        env.close()

    e3 = lambda: uavtrack.BatchedUavEnv(uavtrack.EnvConfig(dim=3, nc=3, **kw))
    refused(e3(), "uavtrack_greedy_actions.*planar", lambda e, acts, rew: e.greedy_actions(seed=1, out=acts[0]))
    refused(e3(), "uavtrack_run_greedy.*planar", lambda e, acts, rew: e.run_greedy(T, seed=1, out=dict(actions=acts, reward=rew)))
    pmi = lambda: uavtrack.BatchedUavEnv(uavtrack.EnvConfig(cooperative=0.3, reward_mode=uavtrack.RewardMode.PMI, **kw))
    refused(pmi(), "uavtrack_run_greedy.*MAAC / MAAC-G", lambda e, acts, rew: e.run_greedy(T, seed=1, out=dict(actions=acts, reward=rew)))
    r, p = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw)), pmi()
    r.reset(seed=2); p.reset(seed=2)
    assert torch.equal(r.greedy_actions(seed=1), p.greedy_actions(seed=1))
    r.close(); p.close()
