"""GPU: every differently written range test of the rollout kernels, one fp32 ulp inside, exactly on and one ulp outside
its threshold, across constants sets -- against the fp64 oracle with NO margin filter.

The scenes are tests/range_edge_scenes.py's (premises and oracle pinned on the CPU by tests/test_range_edges_cpu.py; the
2-D scenes of g10 are the reference's own recordings).  One environment per scene, all scenes of a (constants set,
shape, dim) in one batch, one launch per case; compared: obs, reward, the three terms, raw, covered -- every
environment, every row.  Tolerances are test_hip_parity's: ATOL = 1e-5; the observation rows of UAVs within 2.5 m of
the origin at g7's 2e-4 (the uav.py:165 weight multiplies fp32 rounding by 1 / w).

The nine forms (csrc/step_kernel.hip) and what reaches them -- each case asserts through variant_info() / launch_info()
the template tuple and workgroup size it ran on, derives the forms from that tuple with `forms_of` below, and
test_every_form_was_reached fails the file if one of them never launched:

  form                                               reached by (variant tuple; geometry)
  1s sweep_fast targets, scalar-constant mask        every non-LONE variant (forced sizes, 3-D, (50,25), generic, EXTRAS)
  1v sweep_fast targets, vector-constant mask (VC)   LONE = 1: (20,10) (10,10) (5,3) planar, own geometry, every output
  2  sweep_fast peers: le_dc2; le_two_dp2 in MEAN    every variant (le_two_dp2: MODE = MEAN)
  3  neighbour mask NBF (base-4 digits, __brev)      MODE != RAW, N_ in {20, 10, 5}, not form 5
  4  neighbour mask, scalar compare                  MODE != RAW, N_ = 50
  5  NBSEQ (sequential view + LDS hand-over)         LONE = 1, MODE = PMI, planar: step_many with T = 16
  6  sym_dup (mask inside the fixed-point FMA)       MODE = RAW or PMI, any shape
  7  sweep_weighted (+ its mask loop, N_ > 0)        a probe within 2.5 m of the origin (group d)
  8  MEAN without a mask: neighbours re-derived      MODE = MEAN, generic kernel (N_ = 0)
  9  MAAC-R generic emit is_neighbour; mse           MODE = PMI, generic kernel; mse: every sweep_fast lane

Groups: a. every constants set x {(20,10), (7,4)} x three modes, planar, own geometry;  b. default / pow2 /
dc-below-step x six shapes x three modes x 2-D / 3-D (3-D adds the z-only family: a dropped altitude term puts those
pairs at distance 0);  c. the LONE shapes: RAW with two moves in one launch (the odd-step copy of the LONE RAW loop, the
table-copy parity of every variant), MAAC-R through step_many with T = 16 (step 0 compared), then every feasible forced
workgroup size for the non-LONE siblings;  d. near-origin probes;  e. the integer-in-mantissa bounds fold_constants and
uavtrack_create promise;  and the 2-D scenes of g10 against the reference's own recordings.  The 3-D goldens are the
oracle's alone (the reference is planar), anchored by test_3d_restricted_to_the_xz_plane_equals_2d_kernel.
"""
import numpy as np
import pytest
import torch

import range_edge_scenes as res
from conftest import load_golden
from oracle import OracleConfig, OracleEnv, OraclePmi
from test_hip_parity import ATOL

pytestmark = pytest.mark.gpu

RAW, MEAN, PMI = 0, 1, 2
MODE_NAMES = {RAW: "raw", MEAN: "mean", PMI: "pmi"}
NEAR_ORIGIN_OBS_ATOL = 2e-4            # test_edge_cases_exact_thresholds: near_origin_weight
PMI_LONG_T = 16                        # kPmiShortLaunch
FORCED_SIZES = (64, 128, 256, 512)
FORMS = ("1s", "1v", "2", "2-two_dp2", "3", "4", "5", "6", "7", "7-mask", "8", "9", "9-mse")
REACHED = {f: set() for f in FORMS}    # form -> ids of the cases that launched it and passed


def forms_of(variant, near0):
    """The forms a launch of `variant` = (N_, M_, MODE, Z3, POLICY, ALLOUT, EXTRAS, LONE) takes its decisions in."""
    n_, _, mode, z3, _, _, _, lone = variant
    f = {"1v" if lone else "1s", "2", "9-mse"}
    if mode == MEAN:
        f.add("2-two_dp2")
    else:
        f.add("6")
    if mode != RAW and 0 < n_ <= 64:
        if lone and mode == PMI and n_ <= 24 and not z3:
            f.add("5")
        elif n_ <= 24:
            f.add("3")
        else:
            f.add("4")
    if mode == MEAN and n_ == 0:
        f.add("8")
    if mode == PMI and n_ == 0:
        f.add("9")
    if near0:
        f.add("7")
        if mode != RAW and 0 < n_ <= 64:
            f.add("7-mask")
    return f


@pytest.fixture(scope="module")
def uavtrack():
    import uavtrack
    return uavtrack


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for b in res.gpu_batches():
        if b.group in ("a", "b"):
            out += [(b, m, 0) for m in (RAW, MEAN, PMI)]
        elif b.group == "d":
            out += [(b, m, 0) for m in (MEAN, PMI)]
        elif b.moves == 2:                       # c, two moves: RAW
            out += [(b, RAW, w) for w in (0,) + FORCED_SIZES if w == 0 or w // b.N >= 1]
        else:                                    # c, one move: MAAC-R's long launch on the own geometry, then the forced sizes
            out.append((b, PMI, 0))
            out += [(b, m, w) for w in FORCED_SIZES if w // b.N >= 1 for m in (RAW, MEAN, PMI)]
    return out


_CASES = _cases()


def _case_id(b, mode, wgs):
    return f"{res.batch_id(b)}-{MODE_NAMES[mode]}-wgs{wgs or 'own'}"


_REFS = {}


def _reference(b, mode, pmi_sd):
    """The oracle's outputs of every move of the batch (computed once per (batch, mode), never modified)."""
    key = (tuple(b)[1:], mode)
    if key not in _REFS:
        scenes, _ = res.batch_scenes(b)
        pmi = OraclePmi.from_state_dict(pmi_sd) if mode == PMI else None
        _REFS[key] = res.oracle_steps(scenes, 0.0 if mode == RAW else 0.3, pmi)
        for r in _REFS[key]:
            for v in r.values():
                v.setflags(write=False)
    return _REFS[key]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _report(bad_env, scenes):
    names = [scenes[n].name for n in np.nonzero(bad_env)[0]]
    return f"{len(names)} of {len(scenes)} scenes, e.g. {names[:6]}"


def _compare(out, ref, scenes, near_rows, what):
    """Every environment and row of one step's outputs against the oracle -- nothing set aside."""
    B, N = ref["reward"].shape
    worst = {}
    tol = np.full((B, N, 1), ATOL)
    tol[near_rows] = NEAR_ORIGIN_OBS_ATOL
    for k, got, want, t in (("obs", out["obs"], ref["obs"], tol), ("reward", out["reward"], ref["reward"], ATOL),
                            ("terms", out["terms"], ref["terms"], ATOL), ("raw", out.get("raw"), ref["raw"], ATOL)):
        if got is None:
            continue
        d = np.abs(got.astype(np.float64) - want)
        worst[k] = float(d.max())
        bad = d > t
        if bad.any():
            env_axis = 1 if k == "terms" else 0
            bad_env = bad.any(axis=tuple(a for a in range(bad.ndim) if a != env_axis))
            raise AssertionError(f"{what}: {k} differs from the oracle by up to {d.max():.3g} in {_report(bad_env, scenes)}")
    bad = out["covered"] != ref["covered"]
    assert not bad.any(), f"{what}: covered differs from the oracle in {_report(bad, scenes)}"
    return worst


def _expected_variant(b, mode, lone, extras):
    spec = (b.N, b.M) in res.SPEC_SHAPES
    return (b.N if spec else 0, b.M if spec else 0, mode, int(b.dim == 3), 0, int(not extras), int(extras), int(lone))


def _assert_launch(env, want, wgs, what):
    got, li = env.variant_info(), env.launch_info()
    assert got == want, f"{what}: launched rollout_kernel<{got}>, the case is written for <{want}>"
    assert li["single_wavefront_variant"] == want[7], (what, li)
    if wgs:
        assert li["workgroup"] == wgs, f"{what}: UAVTRACK_WGS={wgs} was ignored (launch {li})"
    elif want[7]:
        assert li["workgroup"] == 64, (what, li)


def _near_rows(scenes, t):
    post = res.exact_state(scenes, t + 1)
    return np.maximum(np.abs(post["ux"]), np.abs(post["uy"])) < 2.5


@pytest.mark.parametrize("b,mode,wgs", _CASES, ids=[_case_id(*c) for c in _CASES])
def test_range_edges_against_oracle(uavtrack, monkeypatch, pmi_state_dict_h64, b, mode, wgs):
    if wgs:
        monkeypatch.setenv("UAVTRACK_WGS", str(wgs))      # read by plan_geometry when the handle is created
    else:
        monkeypatch.delenv("UAVTRACK_WGS", raising=False)
    what = _case_id(b, mode, wgs)
    scenes, _ = res.batch_scenes(b)
    B = len(scenes)
    refs = _reference(b, mode, pmi_state_dict_h64)
    kw = res.config(b.cs, b.N, b.M, b.dim, b.moves, B, 0.0 if mode == RAW else 0.3)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(reward_mode=uavtrack.RewardMode(mode), **kw))
    lone_shape = (b.N, b.M) in res.LONE_SHAPES and b.dim == 2 and not wgs
    launched = set()
    try:
        if mode == PMI:
            env.set_pmi(pmi_state_dict_h64)
        env.reset(seed=3)
        _, acts = res.batch(scenes)
        zeros = np.zeros(B, np.int32)
        state0 = {k: v.astype(np.int32 if k == "ua" else np.float32) for k, v in res.exact_state(scenes, 0).items()}
        long_pmi = b.group == "c" and mode == PMI and not wgs
        if b.moves == 2 or long_pmi:
            # ONE launch of T steps through step_many with every output
            T = PMI_LONG_T if long_pmi else b.moves
            a = np.zeros((T, B, b.N), np.int32)
            a[:b.moves] = acts
            env.set_state(**state0, step_count=zeros)
            r = env.step_many(torch.from_numpy(a))
            want = _expected_variant(b, mode, lone_shape and (mode != PMI or T >= PMI_LONG_T), False)
            _assert_launch(env, want, wgs, what)
            launched |= forms_of(want, b.near0)
            for t in range(b.moves):
                out = {k: _np(r[k][t]) for k in ("obs", "reward", "terms", "covered")}
                _compare(out, refs[t], scenes, _near_rows(scenes, t), f"{what} step {t} of one {T}-step launch")
        else:
            # the single step with every output ...
            env.set_state(**state0, step_count=zeros)
            obs, rew, _ = env.step(torch.from_numpy(acts[0]))
            want = _expected_variant(b, mode, lone_shape and mode != PMI, False)
            _assert_launch(env, want, wgs, what)
            launched |= forms_of(want, b.near0)
            out = dict(obs=_np(obs), reward=_np(rew), terms=_np(env.info["terms"]), covered=_np(env.info["covered"]))
            _compare(out, refs[0], scenes, _near_rows(scenes, 0), what)
            # ... and the same step with the raw rewards attached: the EXTRAS sibling, never LONE
            env.set_state(**state0, step_count=zeros)
            r = env.step_many(torch.from_numpy(acts[:1]), want_raw=True)
            want = _expected_variant(b, mode, False, True)
            _assert_launch(env, want, wgs, what + " (raw attached)")
            launched |= forms_of(want, b.near0)
            out = {k: _np(r[k][0]) for k in ("obs", "reward", "terms", "covered", "raw")}
            _compare(out, refs[0], scenes, _near_rows(scenes, 0), what + " (raw attached)")
    finally:
        env.close()
    for f in launched:
        REACHED[f].add(what)


_G10 = res.g10_groups()


@pytest.mark.parametrize("name,cs,N,M,use_pmi", _G10, ids=[g[0] for g in _G10])
def test_reference_recordings_of_the_scenes(uavtrack, pmi_state_dict_h64, name, cs, N, M, use_pmi):
    """g10: the 2-D scenes as the unmodified reference stepped them (MAAC-G at all ten constants sets, MAAC-R H = 64 at
    three) -- the kernels against the recordings themselves, every scene, every row, no margin filter."""
    z, meta = load_golden("g10_ulp_edges_constants")
    case = next(c for c in meta["cases"] if c["name"] == name)
    scenes = res.all_scenes(cs, N, M, 2, moves=1)
    assert [s.name for s in scenes] == case["scenes"]
    B = len(scenes)
    g = lambda k: z[f"{name}__{k}"]      # noqa: E731
    ref = dict(obs=g("obs")[:, 0], reward=g("reward")[:, 0], terms=np.moveaxis(g("terms")[:, 0], 0, 1), raw=g("raw")[:, 0],
               covered=g("covered")[:, 0])
    mode = PMI if use_pmi else MEAN
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(reward_mode=uavtrack.RewardMode(mode), **res.config(cs, N, M, 2, 1, B, 0.3)))
    try:
        if use_pmi:
            env.set_pmi(pmi_state_dict_h64)
        env.reset(seed=3)
        env.set_state(**{k: g(k)[:, 0] for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th")}, step_count=np.zeros(B, np.int32))
        r = env.step_many(torch.from_numpy(g("actions")[:, 0].astype(np.int32)[None]), want_raw=True)
        out = {k: _np(r[k][0]) for k in ("obs", "reward", "terms", "covered", "raw")}
        _compare(out, ref, scenes, np.zeros((B, N), bool), f"g10 {name}")
    finally:
        env.close()


def test_every_form_was_reached():
    """Each of the nine forms was launched by at least one case that passed, and every batch holds all three sides of
    every threshold (tests/test_range_edges_cpu.py asserts that per batch), so each form met inside / on / outside."""
    missing = [f for f in FORMS if not REACHED[f]]
    print("\n[range edges] cases per form: " + ", ".join(f"{f}: {len(REACHED[f])}" for f in FORMS))
    assert not missing, f"forms no passing case launched: {missing}"


# ---- e. integer-in-mantissa bounds --------------------------------------------------------------------------------------
def test_act_bias_packing_at_the_largest_action_count(uavtrack):
    """e1.  Specialised swarms of up to 64 UAVs carry the peer count in the high part and the action sum in the low part
    of ONE fp32 sum (act_bias_shape); uavtrack_create accepts n_uav^2 * na * nc * 4 < 2^24.  N = 50 at the largest na it
    accepts (1677), every peer within dc, every previous action na - 1 -- the largest sum the packing meets: the mean
    action difference obs[..., 4] (count and sum both enter it) must match the oracle.  Positions are random inside a 100 m
    square (every distance below 162 m against dp = 200, 2 dp = 400, dc = 500: no range test near its threshold), so
    nothing is set aside.  One more action is refused with a message."""
    N, M, B = 50, 25, 6
    na = ((1 << 24) - 1) // (N * N * 4)
    assert N * N * na * 4 < (1 << 24) <= N * N * (na + 1) * 4 and na == 1677
    kw = dict(n_envs=B, n_uav=N, m_targets=M, na=na, x_max=2000.0, y_max=2000.0)
    r = np.random.RandomState(5)
    st = dict(ux=r.uniform(900, 1000, (B, N)).astype(np.float32), uy=r.uniform(900, 1000, (B, N)).astype(np.float32),
              uh=r.uniform(-np.pi, np.pi, (B, N)).astype(np.float32), ua=np.full((B, N), na - 1, np.int32),
              tx=r.uniform(900, 1000, (B, M)).astype(np.float32), ty=r.uniform(900, 1000, (B, M)).astype(np.float32),
              th=r.uniform(-np.pi, np.pi, (B, M)).astype(np.float32))
    act = r.randint(0, na, size=(B, N)).astype(np.int32)
    act[0] = na - 1                                    # one environment with every current action at the top as well
    act[1] = 0
    orc = OracleEnv(OracleConfig(**kw))
    orc.set_state(**st)
    ref = orc.step(act)
    assert ref["margin"].min() > 1.0                   # metres: nothing near a threshold
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw))
    try:
        env.reset(seed=1)
        env.set_state(**st, step_count=np.zeros(B, np.int32))
        obs, rew, _ = env.step(torch.from_numpy(act))
        assert env.variant_info()[:2] == (N, M)
        obs = _np(obs)
        # N - 1 peers in range for everyone: the oracle's mean is over 49 rows; a wrong count or a sum that lost a bit shows here
        assert np.abs(ref["obs"][..., 4]).max() > 0.3
        np.testing.assert_allclose(obs[..., 4], ref["obs"][..., 4], rtol=0, atol=ATOL, err_msg="mean action difference")
        np.testing.assert_allclose(obs, ref["obs"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(rew), ref["reward"], rtol=0, atol=ATOL)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="beyond what the specialised kernel"):
        uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**dict(kw, na=na + 1)))


@pytest.mark.parametrize("N,M", [(50, 25), (512, 4)])
def test_fixed_point_duplicate_sum_of_a_coincident_swarm(uavtrack, N, M):
    """e2.  sym_dup accumulates the duplicate term as integers (g * 2^kSymBits, N - 1 terms of at most e * 2^kSymBits
    each, below 2^32 in sum).  A fully coincident swarm is the largest sum there is: every term is e.  With norm_n_uav = N
    the clip does not saturate (-(N - 1) / N), so a lost carry or a wrapped sum shows in the term.  Specialised N = 50 and
    the generic kernel at its largest swarm."""
    B = 3
    kw = dict(n_envs=B, n_uav=N, m_targets=M, norm_n_uav=N)
    st = dict(ux=np.full((B, N), 1000.0, np.float32), uy=np.full((B, N), 700.0, np.float32),
              uh=np.full((B, N), 0.5, np.float32), ua=np.zeros((B, N), np.int32),
              tx=np.full((B, M), 300.0, np.float32), ty=np.full((B, M), 300.0, np.float32), th=np.zeros((B, M), np.float32))
    st["ux"][1] = 1234.5; st["uh"][2] = -2.0
    act = np.full((B, N), 7, np.int32)                 # one action: the swarm stays coincident
    orc = OracleEnv(OracleConfig(**kw), n_threads=4)
    orc.set_state(**st)
    ref = orc.step(act)
    np.testing.assert_allclose(ref["terms"][2], -(N - 1) / N, rtol=0, atol=1e-12)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw))
    try:
        env.reset(seed=1)
        env.set_state(**st, step_count=np.zeros(B, np.int32))
        _, rew, _ = env.step(torch.from_numpy(act))
        assert env.variant_info()[:3] == ((N, M) if N == 50 else (0, 0)) + (RAW,)
        np.testing.assert_allclose(_np(env.info["terms"])[2], ref["terms"][2], rtol=0, atol=ATOL, err_msg="duplicate term")
        np.testing.assert_allclose(_np(env.info["terms"]), ref["terms"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(rew), ref["reward"], rtol=0, atol=ATOL)
    finally:
        env.close()
