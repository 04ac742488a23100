"""GPU census: every rollout kernel variant of tests/variant_census.py, at the library's own geometry and at every forced
workgroup size plan_geometry accepts, against the fp64 oracle -- and the x-z-plane restriction of the 3-D kernel against
the 2-D kernel.

Each case first asserts that `variant_info()` after the launch IS the table entry's template tuple and that
`launch_info()` shows the intended workgroup size: a case that cannot reach its kernel fails, it does not pass on another
one.  tests/test_variant_census_cpu.py holds the table against the library's symbols, so "every case green" means every
instantiated kernel met the oracle.

The scene (variant_census.SCENE): swarm and targets uniform over a dense 600 x 500 (x 400) box with non-default constants,
headings uniform, the state rounded to fp32 and injected; every launch is one teacher-forced step from a state the oracle
is given too, three steps per case, B = 37 (prime: the last workgroup is partly filled at every geometry).  The comparison
and its numbers are test_hip_parity's (ATOL, RTOL_POSE, MARGIN, Tally).  Knife-edge rates of the fp64 oracle alone on this
scene (6 steps, B = 64, fp32 state re-injected each step): rows 0 / 7 680 (20x10 2-D), 2 / 7 680 (20x10 3-D), 0 / 19 200
(50x25 2-D), 1 / 19 200 (50x25 3-D), 0 elsewhere; environments at most 2 / 384 (0.0052, 50x25 2-D) -- far inside Tally's
caps of 0.003 and 0.03, which are applied here per shape family over all its cases (test_census_knife_edge_rates).
"""
import time

import numpy as np
import pytest
import torch

import variant_census as vc
from greedy_scenes import CAP
from oracle import OracleConfig, OracleEnv, OraclePmi, actor_actions, greedy_actions
from test_hip_parity import (ATOL, MARGIN, RTOL_POSE, Tally, check_outputs, check_state, host, inject, knife_masks,
                             random_pmi_state_dict)

pytestmark = pytest.mark.gpu

STEPS = 3
RESET_SEED = 99
TALLIES = {}                      # shape family -> Tally over every case of the family
REPORT = dict(cases=0, ignored_sizes=[], t0=None, seconds=0.0)
_CASES = vc.cases()


@pytest.fixture(scope="module")
def uavtrack():
    import uavtrack
    return uavtrack


def _merge(fam, tally):
    t = TALLIES.setdefault(fam, Tally())
    t.excluded += tally.excluded; t.total += tally.total
    t.env_excluded += tally.env_excluded; t.env_total += tally.env_total


def _np(t):
    return None if t is None else t.cpu().numpy()


def _make(uavtrack, e, pmi_sd, actor, **over):
    kw = vc.scene_config(e, **over)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(reward_mode=uavtrack.RewardMode(e.mode), **kw))
    if e.mode == vc.PMI:
        env.set_pmi({k: torch.from_numpy(v) for k, v in pmi_sd.items()})
    if actor is not None:
        env.set_actor(actor)
    env.reset(seed=5)
    env.set_state(**vc.scene_state(kw, seed=1000 + e.N), step_count=np.zeros(e.B, np.int32))
    return env, kw


def _oracle(kw, e, pmi_sd):
    orc = OracleEnv(OracleConfig(**{k: v for k, v in kw.items() if k != "horizon"}), n_threads=8)
    if e.mode == vc.PMI:
        orc.pmi = OraclePmi.from_state_dict(pmi_sd)
    return orc


def _actor(uavtrack, e):
    if e.entry != "run_actor":
        return None
    torch.manual_seed(e.N)
    actor = uavtrack.ActorMLP(hidden_dim=e.hidden, action_dim=12 * (3 if e.dim == 3 else 1))
    with torch.no_grad():
        actor.fc2.weight.mul_(5.0)      # (probabilities away from uniform)
    return actor


def _assert_launch(env, e, wgs, what):
    """The kernel that ran is the entry's, on the intended workgroup size, with a partly filled last workgroup."""
    got, li = env.variant_info(), env.launch_info()
    assert got == e.key, f"{what}: launched rollout_kernel<{got}>, the census entry is <{e.key}>"
    assert li["single_wavefront_variant"] == e.key[7], (what, li)
    if wgs:
        assert li["workgroup"] == wgs, f"{what}: UAVTRACK_WGS={wgs} was ignored (launch {li}); the table lists it as feasible"
    elif e.key[7]:
        assert li["workgroup"] == 64, (what, li)
    E = li["envs_per_workgroup"]
    assert E == 1 or e.B % E, f"{what}: B = {e.B} fills every workgroup of {E} environments"


def _launch(env, e, act, obs_in, seed):
    """One step through the entry's own entry point -> dict of host arrays for step 0 of the launch (None: not asked for)."""
    if e.entry == "step":
        obs, rew, done = env.step(torch.from_numpy(act))
        return dict(obs=_np(obs), reward=_np(rew), terms=_np(env.info["terms"]), covered=_np(env.info["covered"]), done=_np(done))
    if e.entry == "step_host":
        v = env.step_host(act)
        return {k: (None if a is None else np.array(a)) for k, a in v.items()}
    if e.entry == "step_many":
        res = env.step_many(torch.from_numpy(act[None]), **e.flags)
    elif e.entry == "run_greedy":
        res = env.run_greedy(1, seed=seed, **e.flags)
    else:
        res = env.run_actor(1, obs_in, seed=seed, **e.flags)
    return {k: (None if v is None else _np(v if k == "ep_sums" else v[0])) for k, v in res.items()}


def _check_policy(e, orc, kw, out, obs_in, seed, step_count, actor, pre, what):
    """The launch's own actions against the oracle's policy, outside its margins (tests/fuzz_api.py steps 2 and 3)."""
    if e.key[4] == vc.GREEDY:
        want, mg = greedy_actions(orc, seed, step_count)
        # the oracle's per-UAV verdict and whatever the per-environment margins used here before accepted; at most 10 % of
        # the scoring-branch decisions left out (greedy_scenes.CAP; the census scene leaves out about 1 %)
        okg = mg["robust"] | ((mg["score"] > 2e-5) & (mg["angle"] > 1e-4) & (mg["dist"][:, None] > 1e-2))
        steer = mg["branch"] == 2
        assert okg.any(), what
        assert (steer & ~okg).sum() <= CAP * steer.sum() and okg[~steer].all(), (what, int((steer & ~okg).sum()), int(steer.sum()))
        np.testing.assert_array_equal(out["actions"][okg], want[okg], err_msg=f"{what} greedy actions")
    elif e.key[4] == vc.ACTOR:
        aa, probs = pre           # actor_actions on the same observation and step count, taken before the launch
        assert np.array_equal(_np(aa), out["actions"]), f"{what}: the rollout's actor and actor_actions disagree"
        want, wp, mg = actor_actions(OracleConfig(n_envs=e.B, n_uav=e.N, m_targets=e.M, na=12, dim=e.dim, nc=kw.get("nc", 1)),
                                     _np(obs_in), actor.state_dict(), seed, step_count)
        assert np.abs(_np(probs) - wp).max() < 1e-5, f"{what} actor probabilities"
        oka = mg > 1e-5
        assert oka.any(), what
        np.testing.assert_array_equal(out["actions"][oka], want[oka], err_msg=f"{what} actor actions")


def _check_extra(env, e, orc, kw, out, ok, okr, ref, st_after, t, what):
    """The EXTRAS variant's own output."""
    if e.extra == "raw":
        np.testing.assert_allclose(out["raw"][okr], ref["raw"][okr], rtol=0, atol=ATOL, err_msg=f"{what} raw")
    elif e.extra == "targets":
        rs = orc.get_state()
        for c, k in enumerate(("tx", "ty")):
            assert np.array_equal(out["targets"][..., c], st_after[k]), f"{what}: target trace {k} is not the state"
            np.testing.assert_allclose(out["targets"][..., c], rs[k], rtol=RTOL_POSE, atol=1e-4, err_msg=f"{what} trace {k}")
    elif e.extra == "state_copy":
        np.testing.assert_allclose(out["raw"][okr], ref["raw"][okr], rtol=0, atol=ATOL, err_msg=f"{what} raw (step_host)")
        for k, v in st_after.items():
            if k != "episode":
                assert np.array_equal(out[k], v), f"{what}: step_host's state copy {k} is not get_state()"
    elif e.extra == "auto_reset":
        done = out["done"] != 0
        assert done.all() if t == kw["horizon"] - 1 else not done.any(), (what, out["done"])


def _run_single_steps(uavtrack, e, wgs, what):
    pmi_sd = random_pmi_state_dict(128, 7) if e.mode == vc.PMI else None
    actor = _actor(uavtrack, e)
    over = dict(horizon=2) if e.extra == "auto_reset" else {}
    env, kw = _make(uavtrack, e, pmi_sd, actor, **over)
    orc = _oracle(kw, e, pmi_sd)
    tally = Tally()
    rng = np.random.RandomState(e.N * 31 + e.dim)
    na = 12 * kw.get("nc", 1)
    obs_in = torch.from_numpy(rng.uniform(-1.0, 1.0, (e.B, e.N, 12)).astype(np.float32)).cuda()
    try:
        for t in range(STEPS):
            st = host(env.get_state())
            inject(orc, st)
            act = rng.randint(0, na, size=(e.B, e.N)).astype(np.int32)
            pre = env.actor_actions(obs_in, seed=11 + t, want_probs=True) if e.key[4] == vc.ACTOR else None
            out = _launch(env, e, act, obs_in, seed=11 + t)
            _assert_launch(env, e, wgs, what)
            if e.key[4] != vc.GIVEN:
                _check_policy(e, orc, kw, out, obs_in, 11 + t, st["step_count"], actor, pre, f"{what} t{t}")
                act = out["actions"]              # the launch's own actions teacher-force the oracle
            ref = orc.step(act)
            ok, okr = knife_masks(ref, f"{what} t{t}", MARGIN, tally=tally)
            check_outputs(ref, ok, okr, kw["cooperative"], f"{what} t{t}", obs=out.get("obs"), rew=out.get("reward"),
                          terms=out.get("terms"), cov=out.get("covered"))
            if e.key[5]:
                assert all(out.get(k) is not None for k in ("obs", "reward", "terms", "covered", "done")), what
            st_after = host(env.get_state())
            if e.extra == "auto_reset" and t == kw["horizon"] - 1:
                # every environment reached its horizon in this step: the state behind it is reset(seed, next episode)
                orc.reset_philox(seed=RESET_SEED, episode=1)
                rs = orc.get_state()
                for k in rs:
                    np.testing.assert_array_equal(st_after[k].astype(np.float64) if k != "ua" else st_after[k], rs[k],
                                                  err_msg=f"{what} t{t}: automatic reset {k}")
                assert (st_after["step_count"] == 0).all() and (st_after["episode"] == 1).all(), what
            else:
                check_state(st_after, orc.get_state(), ok, f"{what} t{t}")
            _check_extra(env, e, orc, kw, out, ok, okr, ref, st_after, t, f"{what} t{t}")
            if out.get("obs") is not None:
                obs_in = torch.from_numpy(out["obs"]).cuda()
        tally.check(what)             # (a single case is too few rows to bound: Tally's own min_total rule)
    finally:
        _merge(vc.family(e), tally)
        env.close()


def _run_pmi_long_launch(uavtrack, e, what):
    """The MAAC-R LONE variants need launches of at least kPmiShortLaunch = 16 steps, whose intermediate state is not
    visible -- the ONE indirect route of the census.  The 16-step launch must equal, bit for bit, 16 single steps from the
    same state (what test_pmi_long_launch_pooled_slots_equals_single_steps and fuzz_api step 1 assert), and each of those
    single steps is compared with the oracle here, in the same test."""
    pmi_sd = random_pmi_state_dict(128, 7)
    actor = _actor(uavtrack, e)
    a, kw = _make(uavtrack, e, pmi_sd, actor)
    b, _ = _make(uavtrack, e, pmi_sd, actor)
    orc = _oracle(kw, e, pmi_sd)
    tally = Tally()
    rng = np.random.RandomState(e.N)
    T = e.T
    try:
        if e.key[4] == vc.ACTOR:
            obs0 = torch.from_numpy(rng.uniform(-1.0, 1.0, (e.B, e.N, 12)).astype(np.float32)).cuda()
            fused = a.run_actor(T, obs0, seed=4)
        else:
            acts = torch.from_numpy(rng.randint(0, 12, size=(T, e.B, e.N)).astype(np.int32)).cuda()
            fused = a.step_many(acts)
        _assert_launch(a, e, 0, what)
        obs = obs0 if e.key[4] == vc.ACTOR else None
        for t in range(T):
            if e.key[4] == vc.ACTOR:
                sc = _np(b.get_state()["step_count"])
                aa, probs = b.actor_actions(obs, seed=4, want_probs=True)
                assert torch.equal(aa, fused["actions"][t]), f"{what}: actor actions t{t}"
                want, wp, mg = actor_actions(OracleConfig(n_envs=e.B, n_uav=e.N, m_targets=e.M, na=12), _np(obs),
                                             actor.state_dict(), 4, sc)
                assert np.abs(_np(probs) - wp).max() < 1e-5, f"{what} actor probabilities t{t}"
                oka = mg > 1e-5
                np.testing.assert_array_equal(_np(aa)[oka], want[oka], err_msg=f"{what} actor actions t{t}")
                act = _np(aa)
            else:
                act = _np(acts[t])
            inject(orc, host(b.get_state()))
            o, r, _ = b.step(torch.from_numpy(act))
            ref = orc.step(act)
            ok, okr = knife_masks(ref, f"{what} single step t{t}", MARGIN, tally=tally)
            check_outputs(ref, ok, okr, kw["cooperative"], f"{what} single step t{t}", obs=_np(o), rew=_np(r),
                          terms=_np(b.info["terms"]), cov=_np(b.info["covered"]))
            check_state(host(b.get_state()), orc.get_state(), ok, f"{what} single step t{t}")
            for k, v in (("obs", o), ("reward", r), ("terms", b.info["terms"]), ("covered", b.info["covered"])):
                assert torch.equal(v, fused[k][t]), f"{what}: {k} of step {t} of the long launch != the single step"
            obs = o
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"{what}: state {k} behind the long launch"
        tally.check(what)
    finally:
        _merge(vc.family(e), tally)
        a.close(); b.close()


@pytest.mark.parametrize("e,wgs", _CASES, ids=[vc.case_id(e, w) for e, w in _CASES])
def test_variant_against_oracle(uavtrack, monkeypatch, e, wgs):
    if REPORT["t0"] is None:
        REPORT["t0"] = time.perf_counter()
    if wgs:
        monkeypatch.setenv("UAVTRACK_WGS", str(wgs))      # read by plan_geometry when the handle is created
    else:
        monkeypatch.delenv("UAVTRACK_WGS", raising=False)
    what = vc.case_id(e, wgs)
    if e.T > 1:
        _run_pmi_long_launch(uavtrack, e, what)
    else:
        _run_single_steps(uavtrack, e, wgs, what)
    REPORT["cases"] += 1
    REPORT["seconds"] = time.perf_counter() - REPORT["t0"]


def test_forced_size_the_library_ignores_is_detected(uavtrack, monkeypatch):
    """A forced workgroup size plan_geometry turns away (fewer lanes than one environment has UAVs) is visible through
    launch_info(): such a (variant, size) pair is infeasible, not a case that ran.  The census shapes have none
    (variant_census.feasible_sizes: every forced size holds a whole environment of at most 50 UAVs); a 70-UAV swarm on
    64 lanes shows the detection."""
    for e in vc.CENSUS:
        assert not e.infeasible, e
    monkeypatch.setenv("UAVTRACK_WGS", "64")
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=5, n_uav=70, m_targets=5))
    env.reset(seed=1)
    assert env.variant_info() == (-1,) * 8 and env.launch_info()["workgroup"] == 0       # none yet
    env.step(torch.zeros(5, 70, dtype=torch.int32))
    assert env.launch_info()["workgroup"] != 64
    assert env.variant_info() == (0, 0, vc.RAW, 0, vc.GIVEN, 1, 0, 0)
    REPORT["ignored_sizes"].append((70, 5, 64))
    env.close()


def test_census_knife_edge_rates():
    """Tally's caps (0.003 of rows, 0.03 of environments) per shape family, summed over every case of the family that ran
    in this session; prints the device's rates and the census's size and wall time for DESIGN.md."""
    print(f"\n[census] {REPORT['cases']} (variant, workgroup size) cases of {len(_CASES)} ran in {REPORT['seconds']:.1f} s; "
          f"forced sizes the library ignored: {REPORT['ignored_sizes']}")
    for fam in sorted(TALLIES):
        t = TALLIES[fam]
        print(f"[census] {fam[0]}x{fam[1]} {fam[2]}-D: rows set aside {t.excluded} / {t.total} "
              f"({t.excluded / max(t.total, 1):.5f}), environments {t.env_excluded} / {t.env_total} "
              f"({t.env_excluded / max(t.env_total, 1):.5f})")
        t.check(f"census {fam}")


# ---- the x-z-plane restriction on the device --------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(20, 10), (50, 25), (7, 4)])
@pytest.mark.parametrize("coop", [0.0, 0.3], ids=["raw", "mean"])
def test_3d_restricted_to_the_xz_plane_equals_2d_kernel(uavtrack, N, M, coop):
    """The 3-D HIP kernel against the 2-D HIP kernel (pinned by the reference's recordings g1-g5) under the x-z-plane
    restriction of tests/test_variant_census_cpu.py, which lists what the mapping makes equal and why: the three terms,
    the reward (RAW and MAAC-G: the neighbour sets enter), the coverage count and observation columns 0, 2-5, 7-9, 11.
    Within ATOL, counts exactly, knife edges by the 2-D oracle's margins under Tally's caps; not bitwise --
    dx^2 + 0 + dz^2 and dx^2 + dy^2 need not round alike.  The scene has pairs within dp in x alone and outside it in
    (x, z): a kernel that dropped the altitude term would put them in range."""
    from test_variant_census_cpu import XZ_OBS_EQUAL, xz_configs, xz_scene, xz_separates
    B = 48
    k3, k2 = xz_configs(N, M, B, coop)
    e3, e2 = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**k3)), uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**k2))
    orc = OracleEnv(OracleConfig(**k2), n_threads=8)
    e3.reset(seed=1); e2.reset(seed=1)
    act = np.full((B, N), 4, np.int32)
    tally, separated = Tally(), 0
    cols = list(XZ_OBS_EQUAL)
    try:
        for t in range(4):
            s3, s2 = xz_scene(N, M, B, 200 + t)
            separated += xz_separates(s3, k3["dp"])
            e3.set_state(**s3); e2.set_state(**s2)
            orc.set_state(**s2)
            ref = orc.step(act)
            ok, okr = knife_masks(ref, f"xz N{N} t{t}", MARGIN, tally=tally)
            o3, r3, _ = e3.step(torch.from_numpy(act))
            o2, r2, _ = e2.step(torch.from_numpy(act))
            assert e3.variant_info()[3] == 1 and e2.variant_info()[3] == 0
            assert e3.variant_info()[:2] == e2.variant_info()[:2] == ((N, M) if (N, M) != (7, 4) else (0, 0))
            t3, t2 = _np(e3.info["terms"]), _np(e2.info["terms"])
            np.testing.assert_allclose(t3[:, okr], t2[:, okr], rtol=0, atol=ATOL, err_msg=f"xz terms t{t}")
            np.testing.assert_allclose(_np(o3)[okr][:, cols], _np(o2)[okr][:, cols], rtol=0, atol=ATOL, err_msg=f"xz obs t{t}")
            m = okr if coop == 0 else ok
            np.testing.assert_allclose(_np(r3)[m], _np(r2)[m], rtol=0, atol=ATOL, err_msg=f"xz reward t{t}")
            np.testing.assert_array_equal(_np(e3.info["covered"])[ok], _np(e2.info["covered"])[ok], err_msg=f"xz covered t{t}")
            # ... and both against the 2-D oracle, so "equal" cannot mean "equally wrong"
            check_outputs(ref, ok, okr, coop, f"xz 2-D vs oracle t{t}", rew=_np(r2), terms=t2, cov=_np(e2.info["covered"]))
            if coop:
                assert np.abs(_np(r3) - (k3["alpha"] * t3[0] + k3["beta"] * t3[1] + k3["gamma"] * t3[2])).max() > 1e-3
        assert separated > 50, separated
        tally.check(f"xz N{N} M{M}")
    finally:
        e3.close(); e2.close()
