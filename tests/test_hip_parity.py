"""GPU parity: the HIP path, called through the C ABI, against the fp64 CPU oracle and
against golden vectors recorded from the unmodified reference.

Tolerances (BASELINE.json north_star): indices (actions, covered counts) bit-exact;
fp32 observations / rewards within 1e-5 absolute (they are normalised to O(1)); poses
within 1e-5 relative (fp32 ulp at 2000 m is 1.2e-4 m, so an absolute 1e-5 on metres is
not representable).  Range tests (d <= dp, d <= dc, d <= 2dp, d < dp, wall crossings)
are discontinuous: a result whose fp64 margin |d - threshold| is below MARGIN (2.5e-4 m,
about two fp32 ulps of a pose at 2000 m) may legitimately flip in fp32, so it is set aside
for that step and counted -- per ROW (one UAV's own range tests: oracle margin_row) for the
observation row, the three reward terms, the raw reward and the MAAC reward; per ENVIRONMENT
(every test of the environment: oracle margin) only for what couples the UAVs: the coverage
count and the cooperative (MAAC-G / MAAC-R) rewards.  Both rates are bounded from above.
"""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import OracleConfig, OracleEnv

pytestmark = pytest.mark.gpu

ATOL = 1e-5
RTOL_POSE = 1e-5
MARGIN = 2.5e-4


@pytest.fixture(scope="module")
def uavtrack():
    import uavtrack
    return uavtrack


def ang_diff(a, b):
    return np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi) % (2 * np.pi) - np.pi)


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def inject(orc, st):
    orc.set_state(st["ux"], st["uy"], st["uh"], st["ua"], st["tx"], st["ty"], st["th"],
                  uz=st.get("uz"), tz=st.get("tz"))


class Tally:
    """Knife-edge bookkeeping of one test: results set aside (fp64 margin below MARGIN) over results compared -- rows (one
    UAV-step each) and environments (one env-step each).  `check()` bounds both rates from ABOVE: an exclusion that grew
    would hide real differences."""

    def __init__(self):
        self.excluded = self.total = 0              # rows
        self.env_excluded = self.env_total = 0

    def add(self, ok_row, ok_env=None):
        self.excluded += int((~ok_row).sum())
        self.total += int(ok_row.size)
        if ok_env is not None:
            self.env_excluded += int((~ok_env).sum())
            self.env_total += int(ok_env.size)

    def check(self, what, max_rate=0.003, max_env_rate=0.03, min_total=150):
        if self.total >= 20 * min_total:     # (a handful of rows quantises the rate too coarsely to bound)
            assert self.excluded <= max_rate * self.total, f"{what}: {self.excluded} of {self.total} UAV-steps on a knife edge"
        if self.env_total >= min_total:
            assert self.env_excluded <= max_env_rate * self.env_total, \
                f"{what}: {self.env_excluded} of {self.env_total} env-steps on a knife edge"


def knife_masks(ref, what, margin=MARGIN, min_ok_frac=0.9, tally=None):
    """The knife-edge masks of one oracle step `ref` -> (ok [B], okr [B, N]): results whose fp64 margin is below `margin`
    are set aside, counted in `tally`, and bounded per step (at least `min_ok_frac` of a batch of 30 or more compared)."""
    ok = ref["margin"] > margin               # [B]    every range / wall test of the environment
    okr = ref["margin_row"] > margin          # [B, N] the tests one UAV's own row depends on
    if os.environ.get("UAVTRACK_TEST_REPORT"):
        print(f"[knife-edge] {what}: rows {int((~okr).sum())}/{okr.size} = {1 - okr.mean():.5f}, "
              f"envs {int((~ok).sum())}/{len(ok)} = {1 - ok.mean():.4f}", flush=True)
    if tally is not None:
        tally.add(okr, ok)
    if len(ok) >= 30:
        assert ok.mean() >= min_ok_frac, f"{what}: too many knife-edge envs ({ok.mean():.3f})"
    assert ok.any(), what
    return ok, okr


def check_outputs(ref, ok, okr, cooperative, what, obs=None, rew=None, terms=None, cov=None):
    """The outputs of one step (host arrays; None: not requested by the launch, not compared) against the oracle's `ref`
    outside the knife edges: observations, terms and rewards within ATOL, the coverage count exactly."""
    if obs is not None:
        np.testing.assert_allclose(obs[okr], ref["obs"][okr], rtol=0, atol=ATOL, err_msg=f"{what} obs")
    if terms is not None:
        np.testing.assert_allclose(terms[:, okr], ref["terms"][:, okr], rtol=0, atol=ATOL, err_msg=f"{what} terms")
    if rew is not None:
        if cooperative == 0:                  # MAAC: the reward is the UAV's own raw reward (uav.py:270)
            np.testing.assert_allclose(rew[okr], ref["reward"][okr], rtol=0, atol=ATOL, err_msg=f"{what} reward")
        else:                                 # MAAC-G / MAAC-R: neighbours' raw rewards and the neighbour test enter
            np.testing.assert_allclose(rew[ok], ref["reward"][ok], rtol=0, atol=ATOL, err_msg=f"{what} reward")
    if cov is not None:
        np.testing.assert_array_equal(cov[ok], ref["covered"][ok], err_msg=f"{what} covered")


def check_state(st, rs, ok, what):
    """The state behind a step (host arrays `st`) against the oracle's `rs`: poses within RTOL_POSE, headings within 1e-5
    (the targets' outside wall knife edges), actions exactly."""
    for k in ("ux", "uy", "tx", "ty") + (("uz",) if "uz" in st else ()):
        np.testing.assert_allclose(st[k], rs[k], rtol=RTOL_POSE, atol=1e-4, err_msg=f"{what} {k}")
    assert ang_diff(st["uh"], rs["uh"]).max() < 1e-5, what
    assert ang_diff(st["th"][ok], rs["th"][ok]).max() < 1e-5, what
    np.testing.assert_array_equal(st["ua"], rs["ua"])


def compare_step(env, orc, act, what, margin=MARGIN, min_ok_frac=0.9, tally=None):
    """One teacher-forced step: oracle starts from the device's fp32 state.  Returns the per-environment mask."""
    inject(orc, host(env.get_state()))
    obs, rew, _ = env.step(torch.from_numpy(act))
    ref = orc.step(act)
    ok, okr = knife_masks(ref, what, margin, min_ok_frac, tally)
    check_outputs(ref, ok, okr, orc.cfg.cooperative, what, obs=obs.cpu().numpy(), rew=rew.cpu().numpy(),
                  terms=env.info["terms"].cpu().numpy(), cov=env.info["covered"].cpu().numpy())
    check_state(host(env.get_state()), orc.get_state(), ok, what)
    return ok


CASES = [
    # (N, M, cooperative, B)          specialised kernels: (5,3) (10,10) (20,10) (50,25); others generic
    (5, 3, 0.0, 200), (10, 10, 0.3, 150), (20, 10, 0.0, 256), (20, 10, 0.3, 256),
    (50, 25, 0.0, 64), (50, 25, 0.3, 64), (7, 4, 0.3, 99), (33, 40, 0.0, 31), (64, 1, 0.3, 9), (1, 5, 0.3, 70),
    (130, 70, 0.3, 5), (1, 70, 0.3, 300), (2, 65, 0.0, 90),     # few UAVs, many targets: LDS caps the envs per workgroup
]


@pytest.mark.parametrize("N,M,coop,B", CASES)
def test_step_teacher_forced_vs_oracle(uavtrack, N, M, coop, B):
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=coop)
    env = uavtrack.BatchedUavEnv(cfg)
    env.reset(seed=1234)
    orc = OracleEnv(OracleConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=coop), n_threads=8)
    rng = np.random.RandomState(N * 100 + M)
    tally = Tally()
    for t in range(6):
        act = rng.randint(0, 12, size=(B, N)).astype(np.int32)
        compare_step(env, orc, act, f"N{N} M{M} coop{coop} t{t}", tally=tally)
    tally.check(f"N{N} M{M} coop{coop}")
    env.close()


@pytest.mark.parametrize("N,M,coop,B", [(50, 25, 0.0, 64), (50, 25, 0.3, 48), (20, 10, 0.3, 128), (9, 6, 0.0, 77)])
def test_3d_step_teacher_forced_vs_oracle(uavtrack, N, M, coop, B):
    """BASELINE configs[3] path: 3-D kinematics (our own spec, DESIGN.md -- the reference has no
    3-D code): z state, climb-angle action factor (action = a_turn + na * a_climb), 3-D ranges."""
    kw = dict(n_envs=B, n_uav=N, m_targets=M, cooperative=coop, dim=3, nc=3, z_max=300.0)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw))
    env.reset(seed=99)
    orc = OracleEnv(OracleConfig(**kw), n_threads=8)
    st, ref = host(env.get_state()), None
    orc.reset_philox(seed=99)
    rs = orc.get_state()
    for k in ("ux", "uy", "uz", "uh", "tx", "ty", "tz", "th"):
        np.testing.assert_array_equal(st[k].astype(np.float64), rs[k], err_msg=f"3-D reset {k}")
    rng = np.random.RandomState(5)
    tally = Tally()
    for t in range(8):
        act = rng.randint(0, 36, size=(B, N)).astype(np.int32)
        compare_step(env, orc, act, f"3D N{N} M{M} t{t}", tally=tally)
    tally.check(f"3D N{N} M{M}")
    assert np.abs(host(env.get_state())["uz"] - 150.0).max() > 1.0      # climbing really happened


def test_3d_restricted_to_plane_equals_2d_bitwise(uavtrack):
    """With one climb level (level flight) and all z equal, the 3-D kernel is the 2-D model."""
    B, N, M, T = 64, 20, 10, 40
    c2 = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=0.3, x_max=900.0, y_max=900.0)
    c3 = c2.with_(dim=3, nc=1, z_max=1000.0)
    e2, e3 = uavtrack.BatchedUavEnv(c2), uavtrack.BatchedUavEnv(c3)
    e2.reset(seed=3)
    s = e2.get_state()
    z = torch.full((B, N), 500.0, device="cuda"); tz = torch.full((B, M), 500.0, device="cuda")
    e3.set_state(s["ux"], s["uy"], s["uh"], s["ua"], s["tx"], s["ty"], s["th"], uz=z, tz=tz)
    act = torch.randint(0, 12, (T, B, N), dtype=torch.int32, device="cuda")
    o2, o3 = e2.step_many(act), e3.step_many(act)
    for k in ("obs", "reward", "terms", "covered"):
        assert torch.equal(o2[k], o3[k]), k


def random_pmi_state_dict(hidden, seed):
    """A PMINetwork-shaped state_dict (PMINet.py:29-38) with non-trivial BatchNorm statistics."""
    r = np.random.RandomState(seed)
    sd = {}
    for lin, bn, fan_in in (("fc_comm", "bn_comm", 5), ("fc_obs", "bn_obs", 4),
                            ("fc_boundary_state", "bn_boundary_state", 3), ("fc1", "bn1", 3 * hidden)):
        k = 1.0 / np.sqrt(fan_in)
        sd[lin + ".weight"] = r.uniform(-k, k, (hidden, fan_in)).astype(np.float32)
        sd[lin + ".bias"] = r.uniform(-k, k, hidden).astype(np.float32)
        sd[bn + ".weight"] = r.uniform(0.5, 1.5, hidden).astype(np.float32)
        sd[bn + ".bias"] = (r.randn(hidden) * 0.2).astype(np.float32)
        sd[bn + ".running_mean"] = (r.randn(hidden) * 0.3).astype(np.float32)
        sd[bn + ".running_var"] = r.uniform(0.5, 2.0, hidden).astype(np.float32)
    k = 1.0 / np.sqrt(hidden)
    sd["fc2.weight"] = r.uniform(-k, k, (1, hidden)).astype(np.float32)
    sd["fc2.bias"] = r.uniform(-k, k, 1).astype(np.float32)
    return sd


@pytest.mark.parametrize("N,M,B,hidden,box", [(20, 10, 128, 128, 2000.0), (20, 10, 96, 128, 500.0), (50, 25, 24, 128, 2000.0),
                                              (20, 10, 64, 64, 700.0), (7, 4, 50, 128, 600.0), (5, 3, 40, 64, 2000.0),
                                              # PMINetwork takes any hidden_dim (PMINet.py:19): other multiples of 32, a width
                                              # that is padded (100 -> 128), one past the register-stationary limit, and
                                              # more than 64 UAVs (multi-word neighbour records)
                                              (20, 10, 64, 96, 700.0), (20, 10, 48, 100, 700.0), (10, 10, 40, 32, 600.0),
                                              (20, 10, 32, 200, 600.0), (70, 5, 6, 64, 900.0)])
def test_pmi_reward_teacher_forced_vs_oracle(uavtrack, pmi_state_dict, N, M, B, hidden, box):
    """MAAC-R (BASELINE configs[2]): PMI-softmax weighted neighbour rewards (uav.py:262-291) with the
    BatchNorm-folded PMINetwork on the matrix cores, against the unfolded fp64 oracle."""
    from oracle import OraclePmi
    sd = pmi_state_dict if hidden == 128 else random_pmi_state_dict(hidden, 3)
    kw = dict(n_envs=B, n_uav=N, m_targets=M, cooperative=0.3, x_max=box, y_max=box)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(reward_mode=uavtrack.RewardMode.PMI, **kw))
    env.set_pmi(sd)
    env.reset(seed=21)
    orc = OracleEnv(OracleConfig(**kw), n_threads=8)
    orc.pmi = OraclePmi.from_state_dict(sd)
    rng = np.random.RandomState(8)
    saw_pairs = 0
    tally = Tally()
    for t in range(5):
        act = rng.randint(0, 12, size=(B, N)).astype(np.int32)
        compare_step(env, orc, act, f"PMI N{N} H{hidden} t{t}", tally=tally)
        saw_pairs += int((np.abs(env.info["terms"].cpu().numpy()[2]) > 0.04).sum())
    tally.check(f"PMI N{N} H{hidden}")
    assert saw_pairs > 0       # neighbours existed, so the network really ran


def test_pmi_against_reference_goldens(uavtrack, pmi_state_dict, pmi_state_dict_h64):
    """HIP MAAC-R reward vs the REAL reference's recorded rewards (g4: N20 M10 H128, g5b: N50 M25 H128, g4b: N20 M10 at
    PMINetwork's default hidden_dim 64)."""
    for name in ("g4_n20m10_pmi", "g5b_n50m25_pmi", "g4b_n20m10_pmi_h64"):
        z, meta = load_golden(name)
        sd = pmi_state_dict_h64 if name.endswith("h64") else pmi_state_dict
        N, M = meta["n_uav"], meta["m_targets"]
        E, T = len(meta["seeds"]), meta["steps"]
        B = E * T
        pick = lambda k: z[k][:, :T].reshape(B, -1)
        kw = dict(n_envs=B, n_uav=N, m_targets=M, cooperative=0.3)
        env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(reward_mode=uavtrack.RewardMode.PMI, **kw))
        env.set_pmi(sd)
        env.set_state(**{k: pick(k) for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th")})
        act = z["actions"].reshape(B, N).astype(np.int32)
        orc = OracleEnv(OracleConfig(**kw), n_threads=8)
        inject(orc, host(env.get_state()))
        ok = orc.step(act)["margin"] > 5e-3
        obs, rew, _ = env.step(torch.from_numpy(act))
        np.testing.assert_allclose(rew.cpu().numpy()[ok], z["reward"].reshape(B, N)[ok], rtol=0, atol=2e-5, err_msg=name)
        np.testing.assert_allclose(obs.cpu().numpy()[ok], z["obs"].reshape(B, N, 12)[ok], rtol=0, atol=2e-5, err_msg=name)
        # the cooperative term really moved the reward away from the raw one somewhere
        assert np.abs(z["reward"] - z["raw"]).max() > 1e-3


def test_pmi_edge_cases_and_step_many(uavtrack, pmi_state_dict):
    z, meta = load_golden("g7_edges")
    for case in meta["cases"]:
        if not case["pmi"]:
            continue
        name, N, M = case["name"], case["n_uav"], case["m_targets"]
        cfg = uavtrack.EnvConfig(n_envs=1, n_uav=N, m_targets=M, cooperative=0.3, reward_mode=uavtrack.RewardMode.PMI)
        env = uavtrack.BatchedUavEnv(cfg)
        env.set_pmi(pmi_state_dict)
        g = lambda k: z[f"{name}__{k}"]
        for t in range(case["steps"]):
            env.set_state(**{k: g(k)[t][None] for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th")})
            obs, rew, _ = env.step(torch.from_numpy(g("actions")[t][None].astype(np.int32)))
            np.testing.assert_allclose(rew[0].cpu().numpy(), g("reward")[t], rtol=0, atol=2e-5, err_msg=f"{name} t{t}")
    # fused-call form: T steps == T single steps, bit for bit, including the episode accumulators
    cfg = uavtrack.EnvConfig(n_envs=40, n_uav=20, m_targets=10, cooperative=0.3, x_max=600.0, y_max=600.0,
                             reward_mode=uavtrack.RewardMode.PMI)
    a, b = uavtrack.BatchedUavEnv(cfg), uavtrack.BatchedUavEnv(cfg)
    a.set_pmi(pmi_state_dict); b.set_pmi(pmi_state_dict)
    a.reset(seed=9); b.reset(seed=9)
    act = torch.randint(0, 12, (6, 40, 20), dtype=torch.int32, device="cuda")
    many = a.step_many(act)
    ep = torch.zeros(40, 5, device="cuda")
    for t in range(6):
        obs, rew, _ = b.step(act[t])
        assert torch.equal(rew, many["reward"][t]) and torch.equal(obs, many["obs"][t])
        ep[:, 0] += rew.mean(1); ep[:, 1:4] += b.info["terms"].mean(2).T; ep[:, 4] += b.info["covered"]
    torch.testing.assert_close(many["ep_sums"], ep, rtol=1e-5, atol=1e-5)
    # a scratch budget of a few MB forces several scoring chunks per call: same bits as one chunk
    import os
    os.environ["UAVTRACK_PMI_SCRATCH_MB"] = "1"
    try:
        d = uavtrack.BatchedUavEnv(cfg); d.set_pmi(pmi_state_dict); d.reset(seed=9)
        chunked = d.step_many(act)
    finally:
        del os.environ["UAVTRACK_PMI_SCRATCH_MB"]
    for k in ("obs", "reward", "terms", "covered"):
        assert torch.equal(chunked[k], many[k]), k
    torch.testing.assert_close(chunked["ep_sums"], many["ep_sums"], rtol=1e-6, atol=1e-6)
    # uavtrack_step_accumulate on the MAAC-R path
    e2 = uavtrack.BatchedUavEnv(cfg); e2.set_pmi(pmi_state_dict); e2.reset(seed=9)
    acc = torch.zeros(40, 5, device="cuda")
    for t in range(6):
        e2.step(act[t], ep_sums=acc)
    torch.testing.assert_close(acc, ep, rtol=1e-5, atol=1e-5)
    # and a PMI env without weights refuses to step
    c = uavtrack.BatchedUavEnv(cfg); c.reset(seed=1)
    with pytest.raises(RuntimeError, match="set_pmi_weights"):
        c.step(act[0])


def test_dense_box_many_neighbours(uavtrack):
    """Small box: every range test is busy (neighbour counts near N, many tracked targets,
    UAVs leaving the box)."""
    kw = dict(n_envs=128, n_uav=20, m_targets=10, cooperative=0.3, x_max=500.0, y_max=400.0)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw))
    env.reset(seed=7)
    orc = OracleEnv(OracleConfig(**kw), n_threads=8)
    rng = np.random.RandomState(3)
    tally = Tally()
    for t in range(25):
        act = rng.randint(0, 12, size=(128, 20)).astype(np.int32)
        compare_step(env, orc, act, f"dense t{t}", tally=tally)
    tally.check("dense box", max_rate=0.02)


def test_reset_bitexact_vs_oracle_and_first_obs(uavtrack):
    for N, M in ((20, 10), (5, 3), (50, 25)):
        cfg = uavtrack.EnvConfig(n_envs=37, n_uav=N, m_targets=M, env_offset=1000)
        env = uavtrack.BatchedUavEnv(cfg)
        obs = env.reset(seed=2 ** 40 + 17, episode=3).cpu().numpy()
        orc = OracleEnv(OracleConfig(n_envs=37, n_uav=N, m_targets=M))
        ref_obs = orc.reset_philox(seed=2 ** 40 + 17, episode=3, env_offset=1000)
        st, rs = host(env.get_state()), orc.get_state()
        for k in ("ux", "uy", "uh", "tx", "ty", "th"):
            np.testing.assert_array_equal(st[k].astype(np.float64), rs[k], err_msg=k)
        np.testing.assert_array_equal(st["ua"], rs["ua"])
        assert np.all(st["step_count"] == 0)
        np.testing.assert_allclose(obs, ref_obs, rtol=0, atol=1e-6)
        assert np.all(obs[..., :9] == -1.0)          # empty observation lists (uav.py:174,186)
        # reference layout: x_i = i * x_max / (N + 1), y = y_max / 2 (environment.py:105-107)
        np.testing.assert_allclose(st["ux"][0], np.arange(1, N + 1) * 2000.0 / (N + 1), rtol=1e-7)


@pytest.mark.parametrize("name", ["g1_n5m3_raw", "g2_n20m10_raw", "g3_n20m10_mean", "g5a_n50m25_raw"])
def test_against_reference_goldens(uavtrack, name):
    """HIP vs the REAL reference's recorded outputs: all (episode, step) pairs of a golden
    file become one batch, state injected (rounded to fp32), one step, compared."""
    z, meta = load_golden(name)
    N, M, coop = meta["n_uav"], meta["m_targets"], meta["cooperative"]
    E, T = len(meta["seeds"]), meta["steps"]
    B = E * T
    pick = lambda k: z[k][:, :T].reshape(B, -1)
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=coop)
    env = uavtrack.BatchedUavEnv(cfg)
    state = {k: pick(k) for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th")}
    env.set_state(**state)
    act = z["actions"].reshape(B, N).astype(np.int32)
    # margins from the oracle started at the same fp32-rounded state
    orc = OracleEnv(OracleConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=coop), n_threads=8)
    inject(orc, host(env.get_state()))
    ref = orc.step(act)
    # (wider than MARGIN: the golden's own fp64 state differs from the injected fp32 one by up to 6e-5 m per pose)
    GM = 1e-3
    ok, okr = ref["margin"] > GM, ref["margin_row"] > GM        # per environment (coverage, cooperative reward) / per UAV row
    if os.environ.get("UAVTRACK_TEST_REPORT"):
        print(f"[knife-edge] golden {name}: rows {int((~okr).sum())}/{okr.size} = {1 - okr.mean():.5f}, envs {int((~ok).sum())}/{B}", flush=True)
    assert okr.mean() >= 0.997, f"{name}: {1 - okr.mean():.4f} of the golden UAV-steps within 1 mm of a threshold"
    assert ok.mean() >= 0.97, f"{name}: {1 - ok.mean():.3f} of the golden env-steps within 1 mm of a threshold"
    rok = okr if coop == 0 else ok                               # the reward's mask: its own row (MAAC) or the environment
    obs, rew, _ = env.step(torch.from_numpy(act))
    obs_d, rew_d = obs, rew
    obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
    terms, cov = env.info["terms"].cpu().numpy(), env.info["covered"].cpu().numpy()
    # (1) north_star's 1e-5 against the oracle restarted from the SAME fp32 state the kernel stepped from ...
    np.testing.assert_allclose(obs[okr], ref["obs"][okr], rtol=0, atol=ATOL)
    np.testing.assert_allclose(rew[rok], ref["reward"][rok], rtol=0, atol=ATOL)
    np.testing.assert_allclose(terms[:, okr], ref["terms"][:, okr], rtol=0, atol=ATOL)
    np.testing.assert_array_equal(cov[ok], ref["covered"][ok])
    # (2) ... and the reference's own recorded outputs at 2e-5: the golden stepped from fp64 poses, the injected state
    # is their fp32 rounding (up to 6e-5 m on a pose at 2000 m), which alone moves a normalised output by ~1e-5
    np.testing.assert_allclose(obs[okr], z["obs"].reshape(B, N, 12)[okr], rtol=0, atol=2e-5)
    np.testing.assert_allclose(rew[rok], z["reward"].reshape(B, N)[rok], rtol=0, atol=2e-5)
    np.testing.assert_allclose(terms[:, okr], np.moveaxis(z["terms"].reshape(B, 3, N), 1, 0)[:, okr], rtol=0, atol=2e-5)
    np.testing.assert_array_equal(cov[ok], z["covered"].reshape(B)[ok])
    st = host(env.get_state())
    nxt = lambda k: z[k][:, 1:T + 1].reshape(B, -1)
    np.testing.assert_allclose(st["ux"], nxt("ux"), rtol=RTOL_POSE, atol=2e-4)
    np.testing.assert_allclose(st["uy"], nxt("uy"), rtol=RTOL_POSE, atol=2e-4)
    assert ang_diff(st["uh"], nxt("uh")).max() < 1e-5
    np.testing.assert_array_equal(st["ua"], nxt("ua"))
    # uav.raw_reward (environment.py:219), recorded in every golden file: the optional raw output of the same step (it selects
    # the kernel variant with the per-step extras compiled in, so the step is repeated from the same state and every other
    # output must come out bit for bit as before)
    env.set_state(**state)
    raw_buf = torch.empty(1, B, N, device="cuda")
    env.set_raw_output(raw_buf)
    obs2, rew2, _ = env.step(torch.from_numpy(act))
    env.set_raw_output(None)
    assert torch.equal(obs2, obs_d) and torch.equal(rew2, rew_d)
    raw = raw_buf[0].cpu().numpy()
    np.testing.assert_allclose(raw[okr], ref["raw"][okr], rtol=0, atol=ATOL)
    np.testing.assert_allclose(raw[okr], z["raw"].reshape(B, N)[okr], rtol=0, atol=2e-5)
    if coop == 0:
        np.testing.assert_array_equal(raw, rew)      # MAAC: reward = clip(raw, -1, 1) and |raw| <= 1 (environment.py:225)


def test_edge_cases_exact_thresholds(uavtrack):
    """g7: hand-placed cases whose distances sit EXACTLY on dp / dc / 2dp and on the walls.
    The inputs are exactly representable in fp32, so no margin exclusion: every inclusive /
    strict decision must come out as in the reference."""
    z, meta = load_golden("g7_edges")
    for case in meta["cases"]:
        if case["pmi"]:
            continue
        name, N, M = case["name"], case["n_uav"], case["m_targets"]
        cfg = uavtrack.EnvConfig(n_envs=1, n_uav=N, m_targets=M, cooperative=case["cooperative"])
        env = uavtrack.BatchedUavEnv(cfg)
        g = lambda k: z[f"{name}__{k}"]
        for t in range(case["steps"]):
            env.set_state(**{k: g(k)[t][None] for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th")})
            obs, rew, _ = env.step(torch.from_numpy(g("actions")[t][None].astype(np.int32)))
            tol = 2e-4 if name == "near_origin_weight" else 2e-5   # 1/w with w ~ 0.14 amplifies fp32 rounding
            np.testing.assert_allclose(obs[0].cpu().numpy(), g("obs")[t], rtol=0, atol=tol, err_msg=f"{name} obs t{t}")
            np.testing.assert_allclose(rew[0].cpu().numpy(), g("reward")[t], rtol=0, atol=2e-5, err_msg=f"{name} rew t{t}")
            np.testing.assert_allclose(env.info["terms"][:, 0].cpu().numpy(), g("terms")[t], rtol=0, atol=2e-5,
                                       err_msg=f"{name} terms t{t}")
            assert int(env.info["covered"][0]) == int(g("covered")[t]), f"{name} covered t{t}"
            st = host(env.get_state())
            assert ang_diff(st["th"][0], g("th")[t + 1]).max() < 1e-5, f"{name} th t{t}"
            assert ang_diff(st["uh"][0], g("uh")[t + 1]).max() < 1e-5, f"{name} uh t{t}"
            np.testing.assert_allclose(st["tx"][0], g("tx")[t + 1], rtol=1e-6, atol=1e-4)


def test_step_many_bitwise_equals_single_steps(uavtrack):
    for N, M, coop in ((20, 10, 0.0), (20, 10, 0.3), (50, 25, 0.3), (7, 4, 0.0)):
        T, B = 37, 50
        cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=coop, horizon=30,
                                 x_max=800.0, y_max=700.0)   # small box: targets bounce within T steps
        a = uavtrack.BatchedUavEnv(cfg); b = uavtrack.BatchedUavEnv(cfg)
        a.reset(seed=5); b.reset(seed=5)
        act = torch.randint(0, 12, (T, B, N), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        many = a.step_many(act)
        ep = torch.zeros(B, 5, device="cuda")
        for t in range(T):
            obs, rew, done = b.step(act[t])
            assert torch.equal(obs, many["obs"][t]) and torch.equal(rew, many["reward"][t])
            assert torch.equal(b.info["terms"], many["terms"][t])
            assert torch.equal(b.info["covered"], many["covered"][t])
            assert torch.equal(done, many["done"][t].bool())
            assert bool(done.all()) == (t + 1 >= 30)
            ep[:, 0] += rew.mean(1); ep[:, 1:4] += b.info["terms"].mean(2).T; ep[:, 4] += b.info["covered"]
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
        torch.testing.assert_close(many["ep_sums"], ep, rtol=1e-5, atol=1e-5)
        assert int(sa["step_count"][0]) == T
        # uavtrack_step_accumulate: the kernel adds each step's contribution to caller-owned accumulators
        c = uavtrack.BatchedUavEnv(cfg); c.reset(seed=5)
        acc = torch.zeros(B, 5, device="cuda")
        for t in range(T):
            c.step(act[t], ep_sums=acc)
        torch.testing.assert_close(acc, ep, rtol=1e-5, atol=1e-5)


def test_free_running_rollout_stays_close(uavtrack):
    """200 free-running steps (no re-injection): fp32 drift stays small and the coverage
    trace matches the fp64 oracle except on rare knife-edge steps."""
    B, N, M, T = 64, 20, 10, 200
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M)
    env = uavtrack.BatchedUavEnv(cfg); env.reset(seed=11)
    orc = OracleEnv(OracleConfig(n_envs=B, n_uav=N, m_targets=M), n_threads=8)
    inject(orc, host(env.get_state()))
    act = np.random.RandomState(2).randint(0, 12, size=(T, B, N)).astype(np.int32)
    out = env.step_many(torch.from_numpy(act).cuda())
    cov = out["covered"].cpu().numpy(); rew = out["reward"].cpu().numpy()
    mism, rerr = 0, 0.0
    for t in range(T):
        ref = orc.step(act[t])
        mism += int((cov[t] != ref["covered"]).sum())
        rerr = max(rerr, np.median(np.abs(rew[t] - ref["reward"])))
    st, rs = host(env.get_state()), orc.get_state()
    assert np.abs(st["ux"] - rs["ux"]).max() < 5e-2 and np.abs(st["uy"] - rs["uy"]).max() < 5e-2
    assert mism <= 0.002 * T * B, mism
    assert rerr < 1e-5


def test_full_size_properties_and_shard_equivalence(uavtrack):
    """BASELINE configs[1] size (4096 x 20 x 10): invariants that need no oracle, and the
    multi-GPU contract -- a shard [off, off+cnt) reproduces the unsharded batch bit for bit."""
    B, N, M, T = 4096, 20, 10, 20
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=0.3)
    full = uavtrack.BatchedUavEnv(cfg); full.reset(seed=42)
    act = torch.randint(0, 12, (T, B, N), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(42))
    out = full.step_many(act)
    assert torch.isfinite(out["obs"]).all() and torch.isfinite(out["reward"]).all()
    assert out["reward"].abs().max() <= 1.0
    t = out["terms"]
    assert t[:, 0].min() >= 0 and t[:, 0].max() <= 1 and t[:, 1].min() >= -1 and t[:, 1].max() <= 0
    assert t[:, 2].min() >= -1 and t[:, 2].max() <= 0
    assert out["covered"].min() >= 0 and out["covered"].max() <= M
    assert torch.equal(torch.round(out["obs"][..., 11] * 12).int(), act)   # a / Na carries the action index
    from uavtrack.sharding import shard_range
    for rank in (0, 3, 7):
        off, cnt = shard_range(B, rank, 8)
        sh = uavtrack.BatchedUavEnv(cfg.with_(n_envs=cnt, env_offset=off)); sh.reset(seed=42)
        o2 = sh.step_many(act[:, off:off + cnt].contiguous())
        for k in ("obs", "reward", "terms", "covered"):
            sl = out[k][:, :, off:off + cnt] if k == "terms" else out[k][:, off:off + cnt]
            assert torch.equal(o2[k], sl), (rank, k)
        assert torch.equal(o2["ep_sums"], out["ep_sums"][off:off + cnt])


BASELINE_SHAPES = [
    # BASELINE.json configs[1], [2], [3] at their stated sizes
    ("c1_4096x20x10_raw", dict(n_envs=4096, n_uav=20, m_targets=10, cooperative=0.0), False, 8),
    ("c2_4096x20x10_pmi", dict(n_envs=4096, n_uav=20, m_targets=10, cooperative=0.3), True, 6),
    ("c3_8192x50x25_3d", dict(n_envs=8192, n_uav=50, m_targets=25, cooperative=0.0, dim=3, nc=3, z_max=300.0), False, 5),
]


@pytest.mark.parametrize("name,kw,pmi,steps", BASELINE_SHAPES, ids=[c[0] for c in BASELINE_SHAPES])
def test_baseline_shapes_full_size(uavtrack, pmi_state_dict, name, kw, pmi, steps):
    """The three single-GPU BASELINE configurations at FULL size (environment.py:120-164 outputs): size-independent
    properties over every environment of the batch, and a teacher-forced comparison with the fp64 oracle on a random
    128-environment subset gathered from the full batch at every step (the bounded soak).  The knife-edge exclusion
    (an fp64 range-test margin below 2.5e-4 m in that step) is bounded from above: at most 0.3 % of the compared
    UAV rows (3 % of the environments, for the coverage count and the cooperative reward) may be set aside, and indices
    (coverage counts, actions) are exact on all the others."""
    from oracle import OraclePmi
    B, N, M = kw["n_envs"], kw["n_uav"], kw["m_targets"]
    na = 12 * kw.get("nc", 1)
    mode = uavtrack.RewardMode.PMI if pmi else None
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(reward_mode=mode, horizon=steps, **kw))
    if pmi:
        env.set_pmi(pmi_state_dict)
    env.reset(seed=2026)
    S = 128
    rng = np.random.RandomState(len(name))
    subset = np.sort(rng.choice(B, S, replace=False))
    sub_t = torch.from_numpy(subset).cuda()
    okw = dict(kw, n_envs=S)
    orc = OracleEnv(OracleConfig(**okw), n_threads=8)
    if pmi:
        orc.pmi = OraclePmi.from_state_dict(pmi_state_dict)
    gen = torch.Generator("cuda").manual_seed(7)
    compared = excluded = env_compared = env_excluded = 0
    worst = dict(obs=0.0, reward=0.0, terms=0.0)
    for t in range(steps):
        st = env.get_state()
        inject(orc, {k: v[sub_t].cpu().numpy() for k, v in st.items() if k != "step_count"})
        act = torch.randint(0, na, (B, N), dtype=torch.int32, device="cuda", generator=gen)
        obs, rew, done = env.step(act)
        terms, cov = env.info["terms"], env.info["covered"]
        # ---- properties, every environment
        assert torch.isfinite(obs).all() and torch.isfinite(rew).all(), name
        assert rew.abs().max() <= 1.0
        assert terms[0].min() >= 0 and terms[0].max() <= 1 and terms[1].min() >= -1 and terms[1].max() <= 0
        assert terms[2].min() >= -1 and terms[2].max() <= 0
        assert cov.min() >= 0 and cov.max() <= M
        assert torch.equal(torch.round(obs[..., 11] * na).int(), act)        # a / Na carries the action index
        assert bool(done.all()) == (t == steps - 1) and bool(done.any()) == (t == steps - 1)
        # ---- oracle on the subset
        ref = orc.step(act[sub_t].cpu().numpy())
        ok, okr = ref["margin"] > MARGIN, ref["margin_row"] > MARGIN      # per environment / per UAV row (see the module docstring)
        rok = okr if kw["cooperative"] == 0 else ok
        compared += okr.size
        excluded += int((~okr).sum())
        env_compared += S
        env_excluded += int((~ok).sum())
        o, r = obs[sub_t].cpu().numpy(), rew[sub_t].cpu().numpy()
        tm, cv = terms[:, sub_t].cpu().numpy(), cov[sub_t].cpu().numpy()
        np.testing.assert_allclose(o[okr], ref["obs"][okr], rtol=0, atol=ATOL, err_msg=f"{name} t{t} obs")
        np.testing.assert_allclose(r[rok], ref["reward"][rok], rtol=0, atol=ATOL, err_msg=f"{name} t{t} reward")
        np.testing.assert_allclose(tm[:, okr], ref["terms"][:, okr], rtol=0, atol=ATOL, err_msg=f"{name} t{t} terms")
        np.testing.assert_array_equal(cv[ok], ref["covered"][ok], err_msg=f"{name} t{t} covered")
        worst["obs"] = max(worst["obs"], float(np.abs(o - ref["obs"])[okr].max()))
        worst["reward"] = max(worst["reward"], float(np.abs(r - ref["reward"])[rok].max()))
        worst["terms"] = max(worst["terms"], float(np.abs(tm - ref["terms"])[:, okr].max()))
        # poses after the step
        st2, rs = env.get_state(), orc.get_state()
        for k in ("ux", "uy", "tx", "ty") + (("uz",) if "uz" in st2 else ()):
            np.testing.assert_allclose(st2[k][sub_t].cpu().numpy(), rs[k], rtol=RTOL_POSE, atol=1e-4, err_msg=f"{name} t{t} {k}")
        assert ang_diff(st2["uh"][sub_t].cpu().numpy(), rs["uh"]).max() < 1e-5
    assert excluded <= 0.003 * compared, f"{name}: {excluded} of {compared} UAV-steps on a knife edge (> 0.3 %)"
    assert env_excluded <= 0.03 * env_compared, f"{name}: {env_excluded} of {env_compared} env-steps on a knife edge (> 3 %)"
    assert int(env.get_state()["step_count"].min()) == steps
    env.close()


def test_target_trace_and_reference_csv_export(uavtrack, tmp_path):
    """SURVEY 8f-4 on the device: the [T, B, M, 2] target trace (uavtrack_set_target_trace) equals the target state
    after every single step, fused == stepwise; and the three CSV files written from a BATCHED rollout for environment
    b (export.save_rollout) are byte-identical to what the reference-shaped B = 1 adapter's save_position /
    save_covered_num (environment.py:229-244) writes for the same episode."""
    B, N, M, T = 37, 5, 3, 25
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M)
    a, b = uavtrack.BatchedUavEnv(cfg), uavtrack.BatchedUavEnv(cfg)
    a.reset(seed=5); b.reset(seed=5)
    act = torch.randint(0, 12, (T, B, N), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    res = a.step_many(act, want_targets=True)
    assert res["targets"].shape == (T, B, M, 2)
    for t in range(T):
        b.step(act[t])
        st = b.get_state()
        assert torch.equal(res["targets"][t, ..., 0], st["tx"]) and torch.equal(res["targets"][t, ..., 1], st["ty"]), t
    # the trace is off again afterwards, and a too-short buffer is refused rather than overrun
    a.set_target_trace(torch.empty(3, B, M, 2, device="cuda"))
    with pytest.raises(RuntimeError, match="target-trace buffer"):
        a.step_many(act[:4])
    a.set_target_trace(None)
    # ---- CSV files: batched export of environment `bi` vs the adapter driven step by step from the same state
    import filecmp
    from uavtrack.export import save_rollout
    bi = 11
    c = uavtrack.BatchedUavEnv(cfg); c.reset(seed=5)
    st0 = c.get_state()
    ref_cfg = {"environment": {"n_uav": N, "m_targets": M, "x_max": 2000, "y_max": 2000, "na": 12},
               "uav": {"dt": 1, "v_max": 20, "h_max": 6, "dc": 500, "dp": 200, "alpha": 0.6, "beta": 0.2, "gamma": 0.2},
               "target": {"v_max": 5, "h_max": 6}, "cooperative": 0}
    one = uavtrack.Environment(n_uav=N, m_targets=M, x_max=2000, y_max=2000, na=12)
    one.reset(ref_cfg)
    one._env.set_state(**{k: v[bi:bi + 1] for k, v in st0.items() if k != "step_count"})
    for t in range(T):
        one.step(ref_cfg, None, act[t, bi].cpu().numpy().tolist())
    d1, d2 = tmp_path / "batched", tmp_path / "adapter"
    for d in (d1, d2):
        for sub in ("u_xy", "t_xy", "covered_target_num"):
            (d / sub).mkdir(parents=True)
    paths = save_rollout(str(d1), 3, res, dc=cfg.dc, env_index=bi)
    one.save_position(str(d2), 3)
    one.save_covered_num(str(d2), 3)
    assert len(paths) == 3
    for sub, name in (("t_xy", "t_xy3.csv"), ("covered_target_num", "covered_target_num3.csv")):
        assert filecmp.cmp(d1 / sub / name, d2 / sub / name, shallow=False), name
    # UAV tracks come back from obs[..., 9:11] * dc: the file agrees with the adapter's to fp32 rounding of x / dc * dc
    u1 = np.loadtxt(d1 / "u_xy" / "u_xy3.csv", delimiter=",", skiprows=1)
    u2 = np.loadtxt(d2 / "u_xy" / "u_xy3.csv", delimiter=",", skiprows=1)
    assert u1.shape == u2.shape == (N * T, 2)
    np.testing.assert_allclose(u1, u2, rtol=2e-7, atol=0)


def test_pmi_training_gather_on_device_rollout(uavtrack):
    """SURVEY 8f-3 on the device: sample_pmi_pairs on a real rollout's observation history (the tensor
    train.operate_epoch hands to PMINetwork.train_pmi, train.py:183 order) returns, for its own drawn indices,
    exactly the rows the reference's copy loop selects (PMINet.py:78-84: selected[i] = data[t_i, (u_i0, u_i1)]),
    and its mini-batches are the slices train_pmi iterates (PMINet.py:87-92)."""
    from uavtrack.pmi_data import pmi_batches, pmi_contrastive_loss, sample_pmi_pairs
    B, N, M, T = 16, 10, 10, 30
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=0.3))
    env.reset(seed=4)
    act = torch.randint(0, 12, (T, B, N), dtype=torch.int32, device="cuda")
    obs = env.step_many(act)["obs"]                                    # [T, B, N, 12] on the device
    g = torch.Generator(device="cuda").manual_seed(9)
    b2 = 512
    sel, t_idx, u_idx = sample_pmi_pairs(obs, N, b2, generator=g)
    assert sel.is_cuda and sel.shape == (b2, 2, 12)
    # the reference's loop, restated on the host over the same flattened history and the same indices
    data = obs.reshape(-1, N, 12).cpu().numpy()                        # train_data.view(timesteps, n_uav, 12)
    ti, ui = t_idx.cpu().numpy(), u_idx.cpu().numpy()
    assert ti.min() >= 0 and ti.max() < T * B and ui.min() >= 0 and ui.max() < N
    want = np.zeros((b2, 2, 12), np.float32)
    for i in range(b2):
        want[i] = data[ti[i], ui[i]]
    np.testing.assert_array_equal(sel.cpu().numpy(), want)
    batches = list(pmi_batches(sel, 128))
    assert len(batches) == b2 // 128
    for k, (x12, x13) in enumerate(batches):
        np.testing.assert_array_equal(x12.cpu().numpy(), want[k * 128:(k + 1) * 128, 0])
        np.testing.assert_array_equal(x13.cpu().numpy(), want[k * 128:(k + 1) * 128, 1])
    # CustomLoss (PMINet.py:15-17) in its literal form on the device outputs of a scorer-shaped net
    net = uavtrack.make_pmi_net(64).cuda().eval()
    with torch.no_grad():
        o1, o2 = net(batches[0][0]), net(batches[0][1])
        lit = torch.mean(torch.log(1 + torch.exp(-o1)) + torch.log(1 + torch.exp(o2)))
    torch.testing.assert_close(pmi_contrastive_loss(o1, o2), lit, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode,dim", [("raw", 2), ("mean", 2), ("pmi", 2), ("raw", 3)])
def test_auto_reset_equals_manual_episode_turnover(uavtrack, pmi_state_dict, mode, dim):
    """uavtrack_step_many_autoreset (SURVEY 8d "auto-reset at done"): environments reach their horizon at DIFFERENT
    steps of one launch; each is reset in place to uavtrack_reset(seed, its episode + 1).  The launch must equal, bit
    for bit, single steps with the finished environments spliced to the states a real uavtrack_reset produces."""
    B, N, M, T, H = 40, 20, 10, 23, 7
    kw = dict(n_envs=B, n_uav=N, m_targets=M, cooperative=0.0 if mode == "raw" else 0.3, horizon=H, env_offset=500,
              dim=dim, nc=3 if dim == 3 else 1)
    if mode == "pmi":
        kw["reward_mode"] = uavtrack.RewardMode.PMI
    cfg = uavtrack.EnvConfig(**kw)
    a, b, c = (uavtrack.BatchedUavEnv(cfg) for _ in range(3))
    if mode == "pmi":
        for e in (a, b):
            e.set_pmi(pmi_state_dict)
    a.reset(seed=3, episode=5); b.reset(seed=3, episode=5)
    start = torch.arange(B, dtype=torch.int32, device="cuda") % H                  # environments at different episode positions
    for e in (a, b):
        st = e.get_state()
        e.set_state(**{k: v for k, v in st.items() if k != "step_count"}, step_count=start)
    na = 12 * (3 if dim == 3 else 1)
    act = torch.randint(0, na, (T, B, N), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    fused = a.step_many(act, auto_reset_seed=99, want_targets=True)
    episode = torch.full((B,), 5, dtype=torch.int64)
    saw = 0
    for t in range(T):
        obs, rew, done = b.step(act[t])
        assert torch.equal(obs, fused["obs"][t]) and torch.equal(rew, fused["reward"][t]), (mode, t)
        assert torch.equal(b.info["terms"], fused["terms"][t]) and torch.equal(b.info["covered"], fused["covered"][t])
        assert torch.equal(done, fused["done"][t].bool())
        st = b.get_state()
        assert torch.equal(st["tx"], fused["targets"][t, ..., 0]) and torch.equal(st["ty"], fused["targets"][t, ..., 1])
        d = done.cpu()
        if d.any():                                       # splice the finished environments to their next episode's reset state
            saw += int(d.sum())
            episode[d] += 1
            for ep in episode[d].unique().tolist():
                c.reset(seed=99, episode=int(ep))
                fresh = c.get_state()
                pick = (d & (episode == ep)).cuda()
                for k in st:
                    st[k][pick] = fresh[k][pick]
            b.set_state(**{k: v for k, v in st.items() if k != "step_count"}, step_count=st["step_count"])
    assert saw >= 3 * B - B                                # everybody turned over at least twice
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # the next automatic reset continues the per-environment episode count: one more horizon, same check on the state
    more = torch.randint(0, na, (H, B, N), dtype=torch.int32, device="cuda")
    a.step_many(more, auto_reset_seed=99)
    assert int(a.get_state()["step_count"].max()) < H


def test_compat_environment_reference_call_shapes(uavtrack):
    """The reference-shaped adapter (B = 1) driven exactly like train.operate_epoch."""
    import random
    ref_cfg = {"environment": {"n_uav": 5, "m_targets": 3, "x_max": 2000, "y_max": 2000, "na": 12},
               "uav": {"dt": 1, "v_max": 20, "h_max": 6, "dc": 500, "dp": 200, "alpha": 0.6, "beta": 0.2, "gamma": 0.2},
               "target": {"v_max": 5, "h_max": 6}, "cooperative": 0}
    z, _ = load_golden("g1_n5m3_raw")
    env = uavtrack.Environment(n_uav=5, m_targets=3, x_max=2000, y_max=2000, na=12)
    random.seed(42)
    assert env.reset(config=ref_cfg) is None
    s0 = [u.get_local_state() for u in env.uav_list]
    assert len(s0) == 5 and s0[0].shape == (12,) and np.all(s0[0][:9] == -1)
    # put the adapter on the golden's initial state, then replay the golden's actions
    env._env.set_state(**{k: z[k][0, 0][None] for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th")})
    for t in range(10):
        nxt, reward, covered = env.step(ref_cfg, None, [int(a) for a in z["actions"][0, t]])
        assert isinstance(covered, int) and set(reward) == {"rewards", "target_tracking_reward",
                                                            "boundary_punishment", "duplicate_tracking_punishment"}
        assert len(nxt) == 5 and all(len(v) == 5 for v in reward.values())
        np.testing.assert_allclose(np.array(nxt), z["obs"][0, t], rtol=0, atol=1e-4)   # free-running fp32
        np.testing.assert_allclose(reward["rewards"], z["reward"][0, t], rtol=0, atol=1e-4)
        assert covered == int(z["covered"][0, t])
    assert len(env.covered_target_num) == 10 and len(env.position["all_uav_xs"]) == 10
    assert abs(env.uav_list[0].x - z["ux"][0, 10, 0]) < 1e-2
    # train.run_epoch's inner loop (train.py:346-352): one get_action_by_direction call per UAV, then step
    for _ in range(3):
        action_list = [uav.get_action_by_direction(env.target_list, env.uav_list) for uav in env.uav_list]
        assert all(isinstance(a, int) and 0 <= a < 12 for a in action_list)
        want = env._env.greedy_actions(seed=env._greedy_seed)[0].cpu().numpy()     # all UAVs from ONE policy call
        np.testing.assert_array_equal(action_list, want)
        env.step(ref_cfg, None, action_list)
    assert len(env.covered_target_num) == 13


def test_closed_loop_rollout_graph_equals_eager(uavtrack):
    """SURVEY 8f-1 driver: actor forward -> action -> uavtrack_step chained on one stream; a HIP-graph
    replay of k steps must give exactly what the same steps give eagerly (greedy policy: no RNG)."""
    torch.manual_seed(0)
    actor = uavtrack.ActorMLP().cuda()
    greedy = lambda probs: probs.argmax(dim=-1).to(torch.int32)
    cfg = uavtrack.EnvConfig(n_envs=256, n_uav=20, m_targets=10, cooperative=0.3)
    res = {}
    for mode in ("eager", "graph"):
        env = uavtrack.BatchedUavEnv(cfg)
        ro = uavtrack.BatchedRollout(env, actor, select=greedy, steps_per_graph=4, use_graph=(mode == "graph"))
        ro.reset(seed=5)
        out = ro.run(22)                      # 5 graph replays + 2 eager tail steps
        res[mode] = {k: v.clone() for k, v in out.items()}
        res[mode]["state"] = env.get_state()
    for k in ("ep_sums", "obs", "reward"):
        assert torch.equal(res["eager"][k], res["graph"][k]), k
    for k, v in res["eager"]["state"].items():
        assert torch.equal(v, res["graph"]["state"][k]), k
    assert int(res["graph"]["state"]["step_count"][0]) == 22
    assert res["graph"]["ep_sums"][:, 4].sum() > 0       # something was covered at some point
    # sampled policy runs too (stochastic: only sanity)
    env = uavtrack.BatchedUavEnv(cfg)
    ro = uavtrack.BatchedRollout(env, actor, steps_per_graph=4)
    ro.reset(seed=1)
    out = ro.run(12)
    assert torch.isfinite(out["ep_sums"]).all() and int(env.get_state()["step_count"][0]) == 12


def test_greedy_baseline_policy_vs_oracle(uavtrack):
    """UAV.get_action_by_direction (uav.py:324-369) on device vs the fp64 oracle.  Actions are
    indices: exact wherever the oracle's margins (score gap between the two best targets, distance of the
    angle to an action boundary, |d - dc| of the penalty tests THIS UAV's choice depends on) leave fp32 no room to
    flip; tests/test_hip_greedy.py runs the kernel's own geometry and the hand-made edge scenes."""
    from greedy_scenes import CAP
    from oracle import greedy_actions
    for N, M, B, box in ((20, 10, 512, 2000.0), (5, 3, 300, 2000.0), (50, 25, 64, 2000.0), (20, 10, 256, 600.0)):
        kw = dict(n_envs=B, n_uav=N, m_targets=M, x_max=box, y_max=box)
        env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(env_offset=77, **kw))
        env.reset(seed=13)
        orc = OracleEnv(OracleConfig(**kw))
        rng = np.random.RandomState(1)
        total = 0
        for t in range(4):
            st = host(env.get_state())
            inject(orc, st)
            got = env.greedy_actions(seed=99).cpu().numpy()
            want, mg = greedy_actions(orc, 99, st["step_count"], env_offset=77)
            # (the score 1/d - 0.8 * #others reaches tens in a crowded box, where an fp32 ulp is ~4e-6)
            # Compared: every UAV the oracle's per-UAV verdict calls robust (uav_oracle.h; a pair near dc sets aside only the
            # UAVs whose choice it can change) and every UAV the margins this test used before accepted; at most 10 % of the
            # scoring-branch decisions may be left out (greedy_scenes.CAP).
            ok = mg["robust"] | ((mg["score"] > 2e-5) & (mg["angle"] > 1e-4) & (mg["dist"][:, None] > 1e-2))
            steer = mg["branch"] == 2
            assert (steer & ~ok).sum() <= CAP * steer.sum(), (N, M, t, int((steer & ~ok).sum()), int(steer.sum()))
            assert ok[~steer].all()
            np.testing.assert_array_equal(got[ok], want[ok], err_msg=f"N{N} M{M} t{t}")
            assert got.min() >= 0 and got.max() <= 11
            total += int(ok.sum())
            env.step(torch.from_numpy(rng.randint(0, 12, size=(B, N)).astype(np.int32)))
        assert total > B
    # coincident UAVs do not count each other (position compare, uav.py:351); keep-straight lands on 5
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=1, n_uav=3, m_targets=1))
    orc = OracleEnv(OracleConfig(n_envs=1, n_uav=3, m_targets=1))
    state = dict(ux=[[100.0, 100.0, 900.0]], uy=[[100.0, 100.0, 900.0]], uh=[[0.0, 0.5, 1.0]], ua=[[0, 0, 0]],
                 tx=[[300.0]], ty=[[100.0]], th=[[0.0]])
    env.set_state(**state); orc.set_state(**{k: np.array(v) for k, v in state.items()})
    for seed in range(6):
        got = env.greedy_actions(seed=seed).cpu().numpy()
        want, _ = greedy_actions(orc, seed, np.zeros(1, np.int32))
        np.testing.assert_array_equal(got, want)
    # the whole C-METHOD loop fused into one launch == T x (greedy_actions, step), bit for bit
    for N, M, coop in ((20, 10, 0.0), (20, 10, 0.3), (7, 4, 0.0)):
        cfg = uavtrack.EnvConfig(n_envs=96, n_uav=N, m_targets=M, cooperative=coop, x_max=900.0, y_max=800.0, env_offset=5)
        a, b = uavtrack.BatchedUavEnv(cfg), uavtrack.BatchedUavEnv(cfg)
        a.reset(seed=4); b.reset(seed=4)
        T = 23
        fused = a.run_greedy(T, seed=11)
        for t in range(T):
            act = b.greedy_actions(seed=11)
            assert torch.equal(act, fused["actions"][t]), (N, t)
            obs, rew, _ = b.step(act)
            assert torch.equal(obs, fused["obs"][t]) and torch.equal(rew, fused["reward"][t])
            assert torch.equal(b.info["covered"], fused["covered"][t])
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    # closed loop with the library's own policy: graph replay == eager
    cfg = uavtrack.EnvConfig(n_envs=128, n_uav=20, m_targets=10)
    res = {}
    for mode in (False, True):
        e = uavtrack.BatchedUavEnv(cfg)
        ro = uavtrack.BatchedRollout(e, "greedy", steps_per_graph=5, use_graph=mode, seed=3)
        ro.reset(seed=2)
        res[mode] = ro.run(17)["ep_sums"].clone()
    assert torch.equal(res[False], res[True])
    assert res[True][:, 1].sum() > 0          # the baseline does find targets


def test_greedy_policy_vs_reference_best_angle(uavtrack):
    """uavtrack_greedy_actions against the REFERENCE's own target scoring (tests/golden/greedy_ref.npz: best_angle
    recorded from UAV.get_action_by_direction, uav.py:324-362, in the build container).  Wherever the kernel's
    Philox draws select the scoring branch (the oracle, bit-exact on those draws, says which UAVs), the action must
    be the defined nearest-turn-rate index of the reference's angle; fp32 leaves no room within the angle margin."""
    from oracle import greedy_actions
    from test_oracle_golden import closest_action
    z, meta = load_golden("greedy_ref")
    checked = 0
    for tag, m in meta.items():
        N, M, S = m["n_uav"], m["m_targets"], m["states"]
        kw = dict(n_envs=S, n_uav=N, m_targets=M, x_max=float(m["box"]), y_max=float(m["box"]))
        env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw))
        orc = OracleEnv(OracleConfig(**kw))
        st = {k: z[f"{tag}__{k}"] for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th")}
        env.set_state(**st)
        st32 = host(env.get_state())
        inject(orc, st32)                                       # the oracle's margins on the fp32 state the kernel sees
        idx, near = closest_action(z[f"{tag}__best_angle"])
        for seed in (5, 6, 7, 8):
            got = env.greedy_actions(seed=seed).cpu().numpy()
            _, aid = greedy_actions(orc, seed, np.zeros(S, np.int32))
            sel = (aid["branch"] == 2) & (near[..., 1] - near[..., 0] > 2e-3) & (aid["score"] > 2e-5) & (aid["dist"][:, None] > 1e-2)
            assert sel.mean() > 0.35, (tag, seed, sel.mean())
            np.testing.assert_array_equal(got[sel], idx[sel], err_msg=f"{tag} seed {seed}")
            straight = aid["branch"] == 1
            assert (got[straight] == 5).all()                   # keep-straight: angle 0 -> the lower middle action
            checked += int(sel.sum())
        env.close()
    assert checked > 1000


def golden_actor():
    g, _ = load_golden("actor_h128")
    sd = {k.replace("__", "."): torch.from_numpy(np.asarray(g[k])) for k in g.files if "__" in k}
    return g, sd


def test_device_actor_vs_reference_golden_and_oracle(uavtrack):
    """FnnPolicyNet.forward + take_action (actor_critic.py:85-98, 138-148) on device.  Probabilities
    within 1e-5 of the reference network's own fp32 output (golden) and of the fp64 oracle; the sampled /
    argmax action is an index: exact wherever the oracle's margin (distance of the uniform to a CDF boundary,
    gap between the two best probabilities) leaves fp32 no room to flip."""
    from oracle import actor_actions
    g, sd = golden_actor()
    obs_all = np.asarray(g["obs"], np.float32)
    N = 16
    B = obs_all.shape[0] // N
    kw = dict(n_envs=B, n_uav=N, m_targets=5)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(env_offset=1234567890123, **kw))
    env.reset(seed=3)
    with pytest.raises(RuntimeError, match="uavtrack_set_actor_weights first"):
        env.actor_actions(torch.zeros(B, N, 12, device="cuda"))
    env.set_actor(sd)
    obs = torch.from_numpy(obs_all[:B * N].reshape(B, N, 12)).cuda()
    st = env.get_state()
    st["step_count"] = (torch.arange(B, device="cuda") % 11).int()        # every word of the Philox block, several blocks
    env.set_state(**st)
    sc = env.get_state()["step_count"].cpu().numpy()
    assert sc.max() == 10
    total = 0
    for mode, seed in ((0, 5), (0, 2 ** 40 + 17), (1, 0)):
        act, probs = env.actor_actions(obs, seed=seed, mode=mode, want_probs=True)
        want_a, want_p, mg = actor_actions(OracleConfig(**kw), obs_all[:B * N], sd, seed, sc, mode=mode,
                                           env_offset=1234567890123)
        np.testing.assert_allclose(probs.cpu().numpy(), want_p, rtol=0, atol=ATOL)
        np.testing.assert_allclose(probs.cpu().numpy().reshape(-1, 12), np.asarray(g["probs"])[:B * N], rtol=0, atol=ATOL)
        ok = mg > 1e-5
        assert ok.mean() > 0.9, ok.mean()
        np.testing.assert_array_equal(act.cpu().numpy()[ok], want_a[ok])
        total += int(ok.sum())
    assert total > 2 * B
    # the draw really follows the probabilities: one observation, many (env, uav) keys
    B2 = 2048
    env2 = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=B2, n_uav=N, m_targets=5))
    env2.reset(seed=1)
    env2.set_actor(sd)
    row = torch.from_numpy(obs_all[7]).cuda()
    act, probs = env2.actor_actions(row.expand(B2, N, 12).contiguous(), seed=77, want_probs=True)
    p = probs[0, 0].double().cpu().numpy()
    freq = np.bincount(act.cpu().numpy().ravel(), minlength=12) / (B2 * N)
    assert np.abs(freq - p).max() < 4.0 * np.sqrt(0.25 / (B2 * N)) + 1e-3, (freq, p)
    assert (p > 0.02).sum() >= 3               # the golden policy is not degenerate


@pytest.mark.parametrize("N,M,coop,mode,pmi", [(20, 10, 0.0, 0, False), (20, 10, 0.3, 0, False), (5, 3, 0.0, 1, False),
                                               (7, 4, 0.3, 0, False), (50, 25, 0.0, 0, False), (20, 10, 0.3, 0, True),
                                               (9, 5, 0.3, 0, True)])
def test_fused_actor_rollout_equals_stepwise(uavtrack, pmi_state_dict, monkeypatch, N, M, coop, mode, pmi):
    """uavtrack_run_actor (actor + environment, T steps, one launch -- one launch triple per chunk with MAAC-R)
    == T x (uavtrack_actor_actions, uavtrack_step), bit for bit -- actions, observations, rewards, coverage,
    final state, episode sums."""
    _, sd = golden_actor()
    if pmi:
        monkeypatch.setenv("UAVTRACK_PMI_SCRATCH_MB", "1")      # several chunks per rollout: the actor's input is handed on
    cfg = uavtrack.EnvConfig(n_envs=70, n_uav=N, m_targets=M, cooperative=coop, x_max=1100.0, y_max=900.0, env_offset=9,
                             reward_mode=uavtrack.RewardMode.PMI if pmi else None)
    a, b = uavtrack.BatchedUavEnv(cfg), uavtrack.BatchedUavEnv(cfg)
    a.set_actor(sd); b.set_actor(sd)
    if pmi:
        a.set_pmi(pmi_state_dict); b.set_pmi(pmi_state_dict)
    obs0 = a.reset(seed=6)
    obs = b.reset(seed=6).clone()
    T = 19
    fused = a.run_actor(T, obs0, seed=21, mode=mode)
    ep = torch.zeros(cfg.n_envs, 5, device="cuda")
    for t in range(T):
        act = b.actor_actions(obs, seed=21, mode=mode)
        assert torch.equal(act, fused["actions"][t]), (N, t)
        o, rew, _ = b.step(act, ep_sums=ep)
        obs = o.clone()
        assert torch.equal(obs, fused["obs"][t]) and torch.equal(rew, fused["reward"][t]), (N, t)
        assert torch.equal(b.info["covered"], fused["covered"][t])
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    np.testing.assert_allclose(fused["ep_sums"].cpu().numpy(), ep.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert len(torch.unique(fused["actions"])) > 3   # a policy, not a constant
    # continuing from the last observation == one longer rollout
    c = uavtrack.BatchedUavEnv(cfg)
    c.set_actor(sd)
    if pmi:
        c.set_pmi(pmi_state_dict)
    o0 = c.reset(seed=6)
    first = c.run_actor(8, o0, seed=21, mode=mode)
    second = c.run_actor(T - 8, first["obs"][-1].contiguous(), seed=21, mode=mode)
    assert torch.equal(second["obs"][-1], fused["obs"][-1]) and torch.equal(second["actions"], fused["actions"][8:])


def test_plain_c_client_matches_python_host_layer(uavtrack, tmp_path):
    """tests/abi/abi_roundtrip.c (gcc, C99, hipMalloc'd buffers, no torch) drives libuavtrack.so through
    include/uavtrack.h; its checksums equal the Python host layer's on the same seed and actions, bit for bit."""
    import subprocess
    from test_host_cpu import build_abi_client
    exe = build_abi_client(tmp_path)
    B, N, M, T, seed = 96, 20, 10, 7, 42
    r = subprocess.run([exe, str(B), str(N), str(M), str(T), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split()

    def fnv1a(buf: bytes) -> int:
        h = 1469598103934665603
        for chunk in (buf,):
            for byte in chunk:
                h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
        return h
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M))
    env.reset(seed=seed)
    covered = 0
    g = np.arange(B * N, dtype=np.int64)
    for t in range(T):
        act = ((g * 7 + t * 3) % 12).astype(np.int32).reshape(B, N)
        obs, rew, _ = env.step(torch.from_numpy(act))
        covered += int(env.info["covered"].sum())
    assert got[1] == f"{fnv1a(obs.cpu().numpy().tobytes()):016x}"
    assert got[3] == f"{fnv1a(rew.cpu().numpy().tobytes()):016x}"
    assert int(got[5]) == covered
    # second line: one uavtrack_step_host from there (host actions in, host results out), against the Python layer's step_host
    host_line = r.stdout.splitlines()[1].split()
    assert host_line[0] == "host"
    v = env.step_host(((g * 5 + 1) % 12).astype(np.int32).reshape(B, N))
    want = {"obs": v["obs"], "reward": v["reward"], "raw": v["raw"], "ux": v["ux"]}
    for k, name in enumerate(("obs", "reward", "raw", "ux")):
        assert host_line[2 + 2 * k] == f"{fnv1a(np.ascontiguousarray(want[name]).tobytes()):016x}", name
    assert int(host_line[10]) == int(v["covered"].sum()) and int(host_line[12]) == int(v["ua"][0, 0]) == 1


def test_bench_contract_line(uavtrack):
    """bench.py as the driver runs it (--steps 20 --warmup 5) prints ONE JSON line with the driver's keys, the
    roofline and cpu_baseline objects; `value` agrees with its own ms_per_step; `config.launch` names the launches
    that were really timed; the roofline comes from the fixed 200-step leg, whatever --steps was."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5",
                        "--cpu-seconds", "2", "--no-extras"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "rccl_world_size"):
        assert k in d, k
    assert d["metric"] == "env agent-steps/sec" and d["unit"] == "agent-steps/s" and d["n_gpus"] == 1
    assert d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 4096 * 20 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert d["value"] > 1e9                                   # > 100x the 10 M north-star floor
    cfg = d["config"]
    assert cfg["timed_launch_steps"] == [20] and cfg["warmup_launch_steps"] == [5]
    assert "1 x 20 steps" in cfg["launch"] and "200 steps per call" not in cfg["launch"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert rf["steps_per_launch"] == 200 and rf["launches_timed"] >= 5 and "launch_ms" not in rf     # (per-launch arrays: --verbose only)
    assert rf["agent_steps_per_launch"] == 4096 * 20 * 200
    # achieved = algorithmic bytes / the rollout kernel's own average duration (library-side HIP events around the kernel);
    # the events around the calls agree with it
    want = rf["algorithmic_bytes_per_agent_step"] * rf["agent_steps_per_launch"] / (rf["kernel_avg_ms"] * 1e-3) / 1e9
    assert abs(rf["achieved"] - want) / want < 1e-9 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert abs(rf["kernel_ms_per_launch"]["rollout"] - rf["kernel_avg_ms"]) < 1e-5
    assert 0.97 * rf["avg_launch_ms"] < rf["kernel_avg_ms"] <= rf["avg_launch_ms"] * 1.01
    assert rf["launches_timed"] >= 10 and rf["launches_untimed_before"] >= 3
    assert rf["min_launch_ms"] <= rf["median_launch_ms"] <= rf["max_launch_ms"]
    # sanity floors only (a correctness suite must not fail on a busy box; measured 0.45-0.49 box to box, and
    # tools/perf_floor.py holds the round's real thresholds): a third of the measured figure would be a broken build
    assert 0.25 < rf["frac"] < 1.0 and rf["frac_at_slowest_call"] > 0.15
    # back-to-back launches at loaded clocks: no host latency inside an event pair, no post-idle ramp (tools/drift.py)
    assert rf["max_launch_ms"] < 1.5 * rf["min_launch_ms"]
    # the other single-GPU BASELINE configurations ride on the default line (--no-extras does not drop them)
    oc = {c["config"].split(" ")[0] + (" dense" if "dense" in c["config"] else " H64" if "hidden 64" in c["config"] else ""): c for c in d["other_configs"]}
    assert set(oc) == {"configs[2]", "configs[2] H64", "configs[3]", "configs[2] dense"}
    for key, c in oc.items():
        r2 = c["roofline"]
        assert r2["launches_timed"] >= 10 and r2["launches_untimed_before"] >= 3 and 0.0 < r2["frac"] < 1.0
        if key.startswith("configs[2]"):
            assert r2["bound"] == "mfma" and r2["unit"] == "TFLOP/s" and r2["peak"] == 2500.0 and "pmi_score_t3_kernel" in r2["kernel"]
            assert 0.05 < r2["pairs_per_agent_step"] < 1.0 and r2["scorer_ms_per_launch"] < r2["avg_launch_ms"]
            assert r2["fp32_equivalent_over_fp32_mfma_peak"] > 1.0          # past what the fp32 matrix pipe could do at all
            assert c["agent_steps_per_s"] > (6e9 if "H64" in key else 2.5e9 if "dense" in key else 4e9)     # sanity floors (round 3: 13.6-14 / 5.4-5.6 / 9.2-9.6 G)
            assert r2["rescored_chunks"] == 0
            assert (r2["pairs_per_agent_step"] > 0.3) == ("dense" in key)      # scored pairs: isolated pairs are not emitted
        else:
            assert r2["bound"] == "hbm" and abs(r2["algorithmic_bytes_per_agent_step"] - 124.1) < 1e-9
            assert r2["agent_steps_per_launch"] == 8192 * 50 * 200 and r2["frac"] > 0.15
    # HBM traffic (PMC counters of exactly this launch shape, profiles/traffic.json) against the algorithmic bytes of the
    # same launch: the fused kernels keep the state on chip, so the counter reads BELOW the algorithmic figure but never
    # far below it, and never above (re-reads).  (Round 4's line carried 36 864 B for the MAAC-R scorer: the idle stand-by
    # kernel's counters filed under the scorer's key -- this bound is what would have caught it.)
    def traffic_sane(r, what):
        if r.get("traffic") is None:
            return
        alg = r["algorithmic_bytes_per_launch"]
        assert 0.5 * alg <= r["traffic"] <= 1.05 * alg, (what, r["traffic"], alg)
    traffic_sane(rf, "headline")
    assert rf["traffic"] is not None and rf["algorithmic_bytes_per_launch"] == rf["algorithmic_bytes_per_agent_step"] * rf["agent_steps_per_launch"]
    assert abs(rf["physical_frac"] - rf["traffic"] / (rf["kernel_avg_ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9
    assert rf["physical_frac"] < rf["frac"]                  # both fractions are on the line: counter bytes and algorithmic bytes
    for key, c in oc.items():
        traffic_sane(c["roofline"], key)
        if key in ("configs[2]", "configs[2] H64"):
            assert c["roofline"]["traffic"] > 1e8 and 0.0 < c["roofline"]["physical_hbm_frac"] < 1.0
        if key == "configs[3]":
            assert c["roofline"]["traffic"] is not None and 0.05 < c["roofline"]["physical_frac"] < c["roofline"]["frac"]
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 1e5 and "sample" in cb
    # the compact list of every measured configuration is the LAST key of the line and fits the tail the driver keeps
    assert list(d)[-1] == "configs" and len(json.dumps(d["configs"])) < 2000
    cs = d["configs"]
    assert len(cs) == 5 and all(0.0 < c["frac"] < 1.0 and c["G"] > 1.0 and c["kernel_ms"] > 0 for c in cs)
    assert [c["bound"] for c in cs] == ["hbm", "mfma", "mfma", "hbm", "mfma"]


def test_bench_dump_outputs_reproducible(uavtrack, tmp_path):
    """bench.py --dump-outputs: the last timed step's arrays as float32 .npy files; the same arguments give the same files
    bit for bit, and --steps really moves the step that is dumped."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    B, N, M = 256, 20, 10

    def run(steps, d):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "5",
                            "--envs", str(B), "--no-extras", "--no-cpu-baseline", "--no-other-configs",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0.0
        return line["dumped_outputs"]["arrays"], {k: np.load(tmp_path / d / f"{k}.npy") for k in line["dumped_outputs"]["arrays"]}
    names, a = run(20, "a")
    _, b = run(20, "b")
    _, c = run(21, "c")
    assert names == ["covered", "done", "ep_sums", "obs", "reward", "terms"]
    shapes = dict(obs=(B, N, 12), reward=(B, N), terms=(3, B, N), covered=(B,), done=(B,), ep_sums=(B, 5))
    for k in names:
        assert a[k].dtype == np.float32 and a[k].shape == shapes[k], k
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["obs"]).all() and np.all((a["done"] == 0) | (a["done"] == 1))
    assert not np.array_equal(a["obs"], c["obs"])


def test_example_training_loop_runs(uavtrack):
    """examples/train_maac.py: fused rollouts -> device replay -> PyTorch TD actor-critic update -> weight upload,
    a few iterations end to end; returns stay finite."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("train_maac", os.path.join(ROOT, "examples", "train_maac.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.main(["--envs", "64", "--iters", "3", "--steps", "40", "--batch", "4096", "--updates", "2"])
    assert len(hist) == 3 and all(np.isfinite(h) for h in hist)
    hist = mod.main(["--method", "maac-r", "--envs", "64", "--iters", "3", "--steps", "40", "--batch", "4096", "--updates", "2",
                     "--pmi-b2", "600", "--pmi-batch", "200"])
    assert len(hist) == 3 and all(np.isfinite(h) for h in hist)


def test_random_shapes_api_fuzz_slice(uavtrack):
    """A fixed slice of tests/fuzz_api.py inside the suite (the full fuzzer is run by hand): random N, M, B, box, reward
    mode, PMI width, workgroup size and action count; fused == stepwise bitwise for the given / greedy / actor rollouts,
    MAAC-R vs the fp64 oracle, shard == unsharded."""
    import fuzz_api
    keys = ("UAVTRACK_WGS", "UAVTRACK_PMI_SCRATCH_MB")
    saved = {k: os.environ.get(k) for k in keys}
    try:
        rng = np.random.RandomState(11)
        for c in range(10):
            fuzz_api.case(c, rng)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_create_destroy_does_not_leak_and_errors_are_reported(uavtrack, pmi_state_dict):
    """300 create / use / destroy cycles leave device memory where it was (every mode allocates its scratch);
    misuse comes back as RuntimeError with the library's message, never as a crash or a silent fallback."""
    _, sd = golden_actor()

    def cycle(mode):
        cfg = uavtrack.EnvConfig(n_envs=32, n_uav=20, m_targets=10, cooperative=0.3 if mode else 0.0,
                                 reward_mode=uavtrack.RewardMode.PMI if mode == 2 else None)
        env = uavtrack.BatchedUavEnv(cfg)
        if mode == 2:
            env.set_pmi(pmi_state_dict)
        env.set_actor(sd)
        obs = env.reset(seed=1)
        env.run_actor(3, obs, seed=2)
        env.close()
    for m in (0, 1, 2):
        cycle(m)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for k in range(300):
        cycle(k % 3)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 64 << 20, (free0, free1)

    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=4, n_uav=5, m_targets=3, reward_mode=uavtrack.RewardMode.PMI, cooperative=0.3))
    env.reset(seed=0)
    with pytest.raises(RuntimeError, match="uavtrack_set_pmi_weights first"):
        env.step(torch.zeros(4, 5, dtype=torch.int32))
    with pytest.raises((RuntimeError, ValueError)):
        env.step(torch.zeros(4, 6, dtype=torch.int32))                     # wrong shape
    with pytest.raises(RuntimeError, match="hidden 300 outside"):
        env.set_pmi(random_pmi_state_dict(300, 0))
    with pytest.raises(ValueError, match="do not match"):
        env.set_actor({"fc1.weight": torch.zeros(8, 11), "fc1.bias": torch.zeros(8),
                       "fc2.weight": torch.zeros(12, 8), "fc2.bias": torch.zeros(12)})
    env3 = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=2, n_uav=4, m_targets=2, dim=3, nc=5, na=12, z_max=300.0))
    with pytest.raises(RuntimeError, match="60 actions"):
        env3.set_actor({"fc1.weight": torch.zeros(8, 12), "fc1.bias": torch.zeros(8),
                        "fc2.weight": torch.zeros(60, 8), "fc2.bias": torch.zeros(60)})
    env2 = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=2, n_uav=4, m_targets=2, na=13))
    with pytest.raises(RuntimeError, match="13 actions"):
        env2.set_actor({"fc1.weight": torch.zeros(8, 12), "fc1.bias": torch.zeros(8),
                        "fc2.weight": torch.zeros(13, 8), "fc2.bias": torch.zeros(13)})
    with pytest.raises(RuntimeError, match="planar"):
        env3.greedy_actions()


def test_closed_loop_device_actor_graph_eager_fused_agree(uavtrack):
    """BatchedRollout with the library's actor: per-step launches under HIP-graph replay == eager == one fused
    launch (run_fused) -- same actions, same observations, same episode sums."""
    _, sd = golden_actor()
    actor = uavtrack.ActorMLP(hidden_dim=128, action_dim=12)
    actor.load_state_dict(sd)
    cfg = uavtrack.EnvConfig(n_envs=96, n_uav=20, m_targets=10)
    res = {}
    for name in ("eager", "graph", "fused", "chunks"):
        env = uavtrack.BatchedUavEnv(cfg)
        ro = uavtrack.BatchedRollout(env, actor, steps_per_graph=5, use_graph=(name == "graph"), seed=8, device_actor=True,
                                     fuse_chunks=(name == "chunks"))
        ro.reset(seed=3)
        out = ro.run_fused(17) if name == "fused" else ro.run(17)
        res[name] = (out["obs"][-1].clone() if name == "fused" else out["obs"].clone(), out["ep_sums"].clone(),
                     env.get_state())
    assert torch.equal(res["eager"][0], res["graph"][0]) and torch.equal(res["eager"][1], res["graph"][1])
    assert torch.equal(res["eager"][0], res["fused"][0])
    np.testing.assert_allclose(res["fused"][1].cpu().numpy(), res["eager"][1].cpu().numpy(), rtol=1e-5, atol=1e-5)
    # run() in fused chunks (3 launches of 5 steps + one of 2): the same trajectory, bit for bit
    assert torch.equal(res["eager"][0], res["chunks"][0])
    for k, v in res["eager"][2].items():
        assert torch.equal(v, res["chunks"][2][k]), k
    np.testing.assert_allclose(res["chunks"][1].cpu().numpy(), res["eager"][1].cpu().numpy(), rtol=1e-5, atol=1e-5)
    # ... and with the C-METHOD baseline policy
    gr = {}
    for name in ("eager", "chunks"):
        env = uavtrack.BatchedUavEnv(cfg)
        ro = uavtrack.BatchedRollout(env, "greedy", steps_per_graph=4, use_graph=False, seed=5, fuse_chunks=(name == "chunks"))
        ro.reset(seed=4)
        out = ro.run(11)
        gr[name] = (out["obs"].clone(), env.get_state())
    assert torch.equal(gr["eager"][0], gr["chunks"][0])
    for k, v in gr["eager"][1].items():
        assert torch.equal(v, gr["chunks"][1][k]), k



@pytest.mark.parametrize("N,M,coop,nc,hidden", [(50, 25, 0.0, 3, 128), (9, 6, 0.3, 3, 40), (20, 10, 0.0, 4, 64)])
def test_3d_device_actor_vs_oracle_and_fused(uavtrack, N, M, coop, nc, hidden):
    """The 3-D action space (na * nc = 36 / 48 actions, three action tiles in the second GEMM): probabilities and
    draws against the fp64 oracle, and the fused actor rollout == actor kernel + step, bitwise."""
    from oracle import actor_actions
    B, A = 40, 12 * nc
    torch.manual_seed(N)
    actor = uavtrack.ActorMLP(hidden_dim=hidden, action_dim=A)
    with torch.no_grad():
        actor.fc2.weight.mul_(5.0)
    kw = dict(n_envs=B, n_uav=N, m_targets=M, cooperative=coop, dim=3, nc=nc, z_max=300.0, env_offset=3)
    a, b = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw)), uavtrack.BatchedUavEnv(uavtrack.EnvConfig(**kw))
    a.set_actor(actor); b.set_actor(actor)
    obs0 = a.reset(seed=2)
    obs = b.reset(seed=2).clone()
    for mode in (0, 1):
        act, probs = b.actor_actions(obs, seed=6, mode=mode, want_probs=True)
        want_a, want_p, mg = actor_actions(OracleConfig(n_envs=B, n_uav=N, m_targets=M, dim=3, nc=nc), obs.cpu().numpy(),
                                           actor.state_dict(), 6, np.zeros(B, np.int32), mode=mode, env_offset=3)
        assert probs.shape == (B, N, A)
        np.testing.assert_allclose(probs.cpu().numpy(), want_p, rtol=0, atol=ATOL)
        ok = mg > 1e-5
        assert ok.mean() > 0.5
        np.testing.assert_array_equal(act.cpu().numpy()[ok], want_a[ok])
        assert int(act.max()) >= 12                         # climb actions are really used
    T = 9
    fused = a.run_actor(T, obs0, seed=6)
    for t in range(T):
        act = b.actor_actions(obs, seed=6)
        assert torch.equal(act, fused["actions"][t]), t
        o, rew, _ = b.step(act)
        obs = o.clone()
        assert torch.equal(obs, fused["obs"][t]) and torch.equal(rew, fused["reward"][t]), t
