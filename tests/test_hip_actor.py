"""The device actor (csrc/actor.h via uavtrack_actor_actions and uavtrack_run_actor) against fp64 at its edges, and the
fused closed-loop driver (BatchedRollout(fuse_chunks=True)) against the eager one.

Probabilities: |p - p64| <= 1e-5 max(1, m_row), m_row the row's largest sum of |terms| (tests/actor_mirror.py; the CPU
model of the split, tests/test_actor_cpu.py, is what justifies the form: DESIGN.md 4.5), and the plain 1e-5 where weights
and inputs are nominal.  Draws and argmax: the oracle's (fp64 probabilities, the same Philox word) wherever its margin
leaves fp32 no room to flip."""
import numpy as np
import pytest
import torch

import actor_mirror as mirror
from oracle import OracleConfig

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-5


@pytest.fixture(scope="module")
def uavtrack():
    import uavtrack
    return uavtrack


def policy(H, A, seed, fc2=5.0):
    """ActorMLP's default initialisation (torch.nn.Linear), fc2 scaled so the softmax is far from uniform."""
    import uavtrack
    torch.manual_seed(seed)
    m = uavtrack.ActorMLP(hidden_dim=H, action_dim=A)
    with torch.no_grad():
        m.fc2.weight.mul_(fc2)
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


def nominal_obs(R, xb, seed, factor=1.0):
    """Uniform within +-factor * xb; every eighth row exactly at the bounds (random signs)."""
    r = np.random.RandomState(seed)
    x = r.uniform(-1.0, 1.0, (R, 12)) * xb * factor
    x[::8] = np.sign(r.uniform(-1.0, 1.0, (len(x[::8]), 12))) * xb * factor
    return x.astype(np.float32)


def evaluate(uavtrack, sd, obs, N=16, seed=11, **kw):
    """The stand-alone policy kernel on obs [R, 12] (R a multiple of N): probs, sampled and argmax actions, and the oracle's
    draws and margins for the same rows (step_count = env % 7: every Philox word, several blocks)."""
    from oracle import actor_actions
    R = obs.shape[0]
    B = R // N
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=4, env_offset=77, **kw)
    env = uavtrack.BatchedUavEnv(cfg)
    env.reset(seed=1)
    st = env.get_state()
    st["step_count"] = (torch.arange(B, device=DEV) % 7).int()
    env.set_state(**st)
    env.set_actor({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    o = torch.from_numpy(np.ascontiguousarray(obs.reshape(B, N, 12))).to(DEV)
    act, probs = env.actor_actions(o, seed=seed, want_probs=True)
    am = env.actor_actions(o, seed=seed, mode=1)
    ocfg = OracleConfig(n_envs=B, n_uav=N, m_targets=4, dim=cfg.dim, na=cfg.na, nc=cfg.nc)
    want, _, mg = actor_actions(ocfg, obs.astype(np.float64), sd, seed, np.arange(B) % 7, mode=0, env_offset=77)
    out = dict(probs=probs.reshape(R, -1).double().cpu().numpy(), act=act.reshape(R).cpu().numpy(),
               argmax=am.reshape(R).cpu().numpy(), want=want.reshape(R), margin=np.repeat(mg, N), cfg=cfg)
    env.close()
    return out


def check(res, sd, obs, xb, rel, what, capped=False, draws=True):
    """Probabilities against fp64 (capped: the forward with the kernel's saturation), draws against the oracle, argmax
    against fp64; returns the worst |dp| / bound."""
    lg, p64, m = mirror.forward_fp64(sd, obs, xb, capped=capped)
    p = res["probs"]
    assert np.isfinite(p).all(), what
    np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-5, err_msg=what)
    bound = ATOL * (np.maximum(1.0, m) if rel else 1.0)
    err = np.abs(p - p64).max(axis=1)
    w = int(np.argmax(err / bound))
    assert (err <= bound).all(), f"{what}: |dp| {err[w]:.3g} > {bound[w]:.3g} (m_row {m[w]:.3g}, row {w})"
    A = p64.shape[1]
    assert (res["act"] >= 0).all() and (res["act"] < A).all() and (res["argmax"] < A).all(), what
    # argmax: fp64's wherever the logit gap exceeds twice the split's logit error (2^-20 m_row, tests/test_actor_cpu.py)
    top = np.sort(lg, axis=1)
    ok = top[:, -1] - top[:, -2] > 2.0 ** -19 * m
    assert ok.mean() > 0.5, what
    np.testing.assert_array_equal(res["argmax"][ok], lg.argmax(axis=1)[ok], err_msg=what)
    if draws:
        # the draw: the oracle's wherever its margin exceeds what the measured error can move a CDF entry (16 UAVs per env)
        env_err = np.repeat((A * err).reshape(-1, 16).max(axis=1), 16)
        ok = res["margin"] > np.maximum(2.0 * env_err, ATOL)
        assert ok.mean() > 0.5, what
        np.testing.assert_array_equal(res["act"][ok], res["want"][ok], err_msg=what)
    print(f"[actor] {what}: max |dp| {err.max():.3g}, max |dp|/max(1,m) {(err / np.maximum(1, m)).max():.3g}, "
          f"max m_row {m.max():.3g}, needs relative bound {bool((err > ATOL).any())}")
    return float((err / bound).max())


WIDTHS = [1, 31, 32, 33, 96, 128, 200, 256, 1000, 4096]


@pytest.mark.parametrize("H", WIDTHS)
def test_actor_widths_vs_fp64(uavtrack, H):
    """Every tile count of the general tile loop -- odd ones, a partial last tile, the ActorMLP default 256, the accepted
    4096 -- at nominal inputs: the plain 1e-5."""
    sd = policy(H, 12, H)
    xb = mirror.actor_xb()
    obs = nominal_obs(1024, xb, seed=H)
    check(evaluate(uavtrack, sd, obs), sd, obs, xb, rel=False, what=f"H{H}")


@pytest.mark.parametrize("H,na,dim,nc", [(128, 2, 2, 1), (33, 2, 2, 1), (128, 3, 2, 1), (200, 3, 2, 1), (96, 12, 3, 3),
                                         (128, 12, 3, 3), (200, 12, 3, 4), (4096, 12, 3, 4)])
def test_actor_action_counts_vs_fp64(uavtrack, H, na, dim, nc):
    """na = 2, 3 (most of the 12 softmax slots masked) and the 3-D action space (A = 36, 48 over two action tiles)."""
    sd = policy(H, na * nc, 100 + H + na)
    xb = mirror.actor_xb()
    obs = nominal_obs(1024, xb, seed=H + na)
    kw = dict(na=na, dim=dim, nc=nc) if dim == 3 else dict(na=na)
    if dim == 3:
        kw["z_max"] = 300.0
    check(evaluate(uavtrack, sd, obs, **kw), sd, obs, xb, rel=False, what=f"H{H} na{na} nc{nc}")


def _learned_policy(uavtrack):
    """~200 DeviceActorCritic updates at a high learning rate on rollout-like batches."""
    torch.manual_seed(3)
    L = uavtrack.DeviceActorCritic(12, 128, 12, 3e-2, 3e-2, 0.95, DEV)
    r = np.random.RandomState(7)
    for _ in range(200):
        s = r.uniform(-1, 1, (256, 12)).astype(np.float32)
        s2 = r.uniform(-1, 1, (256, 12)).astype(np.float32)
        s[:, 9:11] *= 16; s2[:, 9:11] *= 16
        L.update({"states": torch.from_numpy(s).to(DEV), "actions": torch.from_numpy(r.randint(0, 12, 256)).to(DEV),
                  "rewards": torch.from_numpy(r.uniform(-2, 2, 256).astype(np.float32)).to(DEV),
                  "next_states": torch.from_numpy(s2).to(DEV)})
    return {k: v.numpy().copy() for k, v in L.actor_state_dict().items()}


SCALES = ["T1_2^60", "T2_2^60", "T1_2^-24", "T2_2^-24", "T1_2^12", "T1_2^-60_raw", "T2_2^-60_raw", "b1_large_W1_tiny",
          "box_20km_dc50", "box_20km_dc5_W1x30", "weights_x2^20", "learned"]


@pytest.mark.parametrize("case", SCALES)
def test_actor_block_scales_vs_fp64(uavtrack, case):
    """The host's block scales T1, T2 at and between their clamps, a bias that dwarfs a tiny W1, a wide box with a small dc
    (small T1: W1's lo plane subnormal in f16), logits beyond 2^30 (the softmax's overflow guard), and weights a learner
    has pushed around.  A policy whose layers are rescaled against each other is the same policy: those cases must give
    the unscaled network's probabilities bit for bit."""
    base = policy(128, 12, 0)
    xb, kw, rel, same_as_base, draws = mirror.actor_xb(), {}, True, False, True
    if case in ("T1_2^60", "T2_2^60", "T1_2^-24", "T2_2^-24", "T1_2^12"):
        t = {"T1_2^60": 60, "T2_2^60": 60, "T1_2^-24": -24, "T2_2^-24": -24, "T1_2^12": 12}[case]
        sd = mirror.at_scale(base, xb, **({"t1": t} if case.startswith("T1") else {"t2": t}))
        T1, T2 = mirror.scales_of(sd, xb)
        assert (T1 if case.startswith("T1") else T2) == 2.0 ** t
        rel, same_as_base = False, True
    elif case == "T1_2^-60_raw":                                  # W1, b1 alone scaled: T1 at its lower clamp, logits huge
        sd = mirror.rescale(base, 2.0 ** 65)
        assert mirror.scales_of(sd, xb)[0] == 2.0 ** -60
        draws = False
    elif case == "T2_2^-60_raw":
        sd = mirror.rescale(base, 1.0, 2.0 ** 75)
        assert mirror.scales_of(sd, xb)[1] == 2.0 ** -60
        draws = False
    elif case == "b1_large_W1_tiny":
        sd = mirror.rescale(base, 2.0 ** -10, 2.0 ** -10, sb1=2.0 ** 10)
    elif case == "box_20km_dc50":
        sd, kw = base, dict(x_max=20000.0, y_max=20000.0, dc=50.0)
    elif case == "box_20km_dc5_W1x30":
        sd, kw = mirror.rescale(base, 30.0, 1.0, sb1=1.0), dict(x_max=20000.0, y_max=20000.0, dc=5.0)
    elif case == "weights_x2^20":
        sd, draws = mirror.rescale(base, 2.0 ** 20, 2.0 ** 20), False
    else:
        sd = _learned_policy(uavtrack)
    if kw:
        xb = mirror.actor_xb(**kw)
    obs = nominal_obs(1024, xb, seed=len(case))
    res = evaluate(uavtrack, sd, obs, **kw)
    check(res, sd, obs, xb, rel=rel, what=case, draws=draws)
    if same_as_base:
        ref = evaluate(uavtrack, base, obs)
        assert np.array_equal(res["probs"], ref["probs"]) and np.array_equal(res["act"], ref["act"]), case


@pytest.mark.parametrize("case", ["x100", "beyond_cap", "dense_box"])
def test_actor_inputs_beyond_nominal(uavtrack, case):
    """Observations ~100x past the nominal bounds (inside the 128x headroom: no saturation), past the 60000 cap (finite,
    normalised, equal to the fp64 forward with the kernel's clamps -- and to the plain one where nothing saturates), and
    from dense-box rollouts where UAV pairs come closer than 1 m (the 1 / min(d, 1) weight, uav.py:165)."""
    sd = policy(128, 12, 0)
    xb = mirror.actor_xb()
    if case == "x100":
        obs = nominal_obs(1024, xb, seed=5, factor=100.0)
        assert not mirror.cap_reached(sd, obs, xb).any()
        check(evaluate(uavtrack, sd, obs), sd, obs, xb, rel=True, what=case)
        return
    if case == "beyond_cap":
        r = np.random.RandomState(9)
        obs = nominal_obs(1024, xb, seed=6)
        hot = r.rand(*obs.shape) < 0.08
        obs[hot] = (np.sign(r.uniform(-1, 1, hot.sum())) * 10.0 ** r.uniform(3, 9, hot.sum())).astype(np.float32)
    else:
        cfg = uavtrack.EnvConfig(n_envs=64, n_uav=65, m_targets=10, x_max=150.0, y_max=150.0)
        env = uavtrack.BatchedUavEnv(cfg)
        env.reset(seed=4)
        r = np.random.RandomState(2)
        rows, closest = [], np.inf
        for t in range(12):
            o, _, _ = env.step(torch.from_numpy(r.randint(0, 12, (64, 65)).astype(np.int32)))
            st = env.get_state()
            ux, uy = st["ux"].cpu().numpy(), st["uy"].cpu().numpy()
            d = np.hypot(ux[:, :, None] - ux[:, None, :], uy[:, :, None] - uy[:, None, :]) + np.eye(65) * 1e9
            closest = min(closest, d.min())
            rows.append(o.reshape(-1, 12).cpu().numpy())
        env.close()
        assert closest < 1.0, closest
        obs = np.concatenate(rows)
        obs = obs[: (len(obs) // 16) * 16]
    capped = mirror.cap_reached(sd, obs, xb)
    res = evaluate(uavtrack, sd, obs)
    check(res, sd, obs, xb, rel=True, what=case, capped=True, draws=False)
    free = ~mirror.cap_reached(sd, obs, xb, slack=1.01)
    _, p64, m = mirror.forward_fp64(sd, obs)
    assert (np.abs(res["probs"] - p64).max(axis=1)[free] <= ATOL * np.maximum(1.0, m[free])).all(), case
    print(f"[actor] {case}: {int(capped.sum())} of {len(obs)} rows saturate, max |obs| {np.abs(obs).max():.3g}")
    if case == "beyond_cap":
        assert capped.mean() > 0.2


def test_actor_degenerate_softmax(uavtrack):
    """All logits equal (argmax 0, uniform probabilities); a maximum duplicated at a later index (the lowest index wins);
    near one-hot logits (the sample is the argmax)."""
    xb = mirror.actor_xb()
    obs = nominal_obs(1024, xb, seed=1)
    for na in (12, 3):
        sd = policy(96, na, 4)
        sd["fc2.weight"][:] = 0.0
        sd["fc2.bias"][:] = 0.3
        res = evaluate(uavtrack, sd, obs, na=na)
        assert (res["argmax"] == 0).all()
        np.testing.assert_allclose(res["probs"], 1.0 / na, rtol=0, atol=1e-6)
    sd = policy(128, 12, 5)
    sd["fc2.weight"][9] = sd["fc2.weight"][4]
    sd["fc2.bias"][[4, 9]] = 40.0
    res = evaluate(uavtrack, sd, obs)
    assert (res["argmax"] == 4).all()
    sd = policy(128, 12, 6, fc2=400.0)
    lg, _, _ = mirror.forward_fp64(sd, obs)
    top = np.sort(lg, axis=1)
    spread = top[:, -1] - top[:, -2] > 100.0
    assert spread.mean() > 0.5
    res = evaluate(uavtrack, sd, obs)
    np.testing.assert_array_equal(res["act"][spread], lg.argmax(axis=1)[spread])
    np.testing.assert_array_equal(res["argmax"][spread], lg.argmax(axis=1)[spread])


def test_actor_masked_slots_never_drawn(uavtrack):
    """A < slots (na = 2, 3 of 12; 36 of 48): over 10^7 draws per case -- the last action favoured, so the inverse CDF
    runs to the end of the row -- no action >= A (and none < 0) appears."""
    B, N = 4096, 64
    xb = mirror.actor_xb()
    obs = torch.from_numpy(nominal_obs(B * N, xb, seed=3).reshape(B, N, 12)).to(DEV)
    for na, dim, nc in ((2, 2, 1), (3, 2, 1), (12, 3, 3)):
        A = na * nc
        sd = policy(64, A, A)
        sd["fc2.bias"][A - 1] += 3.0
        kw = dict(na=na) if dim == 2 else dict(na=na, dim=3, nc=nc, z_max=300.0)
        env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=4, **kw))
        env.reset(seed=0)
        env.set_actor({k: torch.from_numpy(v) for k, v in sd.items()})
        lo = torch.zeros((), dtype=torch.int32, device=DEV)
        hi = torch.zeros((), dtype=torch.int32, device=DEV)
        last = torch.zeros((), dtype=torch.int64, device=DEV)
        draws = 0
        for s in range(40):
            a = env.actor_actions(obs, seed=1000 + s)
            lo = torch.minimum(lo, a.min()); hi = torch.maximum(hi, a.max())
            last += (a == A - 1).sum()
            draws += B * N
        assert draws >= 10 ** 7
        assert int(lo) == 0 and int(hi) == A - 1, (A, int(lo), int(hi))
        assert int(last) > draws // 100, A                 # (the inverse CDF really runs to the end of the row)
        env.close()


def test_actor_draw_frequencies(uavtrack):
    """64 distinct probability rows x 4096 Philox keys each: every action's frequency within 5 sigma (+ one count) of the
    fp64 probability.  Philox is deterministic, so is the test."""
    B, N = 4096, 64
    xb = mirror.actor_xb()
    rows = nominal_obs(N, xb, seed=12)
    sd = policy(128, 12, 8, fc2=3.0)
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=4))
    env.reset(seed=0)
    env.set_actor({k: torch.from_numpy(v) for k, v in sd.items()})
    obs = torch.from_numpy(rows).to(DEV).expand(B, N, 12).contiguous()
    act = env.actor_actions(obs, seed=99).cpu().numpy()
    env.close()
    _, p, _ = mirror.forward_fp64(sd, rows)
    assert (p.max(axis=1) < 0.9).mean() > 0.5                   # rows that really mix
    for i in range(N):
        f = np.bincount(act[:, i], minlength=12) / B
        tol = 5.0 * np.sqrt(p[i] * (1 - p[i]) / B) + 1.0 / B
        assert (np.abs(f - p[i]) <= tol).all(), (i, f, p[i])


@pytest.mark.parametrize("H,lone", [(128, 1), (200, 0)])
def test_fused_actor_draws_every_step(uavtrack, H, lone):
    """uavtrack_run_actor: the action at EVERY step equals the oracle's draw for that step's observation and step_count,
    wherever the margin is > 1e-5 -- launches starting at step_count 0..3 (mid-block) and crossing Philox blocks, on the
    single-wavefront variant (H 128 at 20 x 10) and the general one."""
    from oracle import actor_actions
    B, N, M, T = 48, 20, 10, 9
    sd = policy(H, 12, H)
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, env_offset=5)
    ocfg = OracleConfig(n_envs=B, n_uav=N, m_targets=M)
    env = uavtrack.BatchedUavEnv(cfg)
    env.set_actor({k: torch.from_numpy(v) for k, v in sd.items()})
    checked = 0
    for start in range(4):
        obs0 = env.reset(seed=start)
        st = env.get_state()
        sc0 = start + 4 * (np.arange(B) % 3)
        st["step_count"] = torch.from_numpy(sc0.astype(np.int32))
        env.set_state(**st)
        res = env.run_actor(T, obs0, seed=31)
        assert env.launch_info()["single_wavefront_variant"] == lone
        acts = res["actions"].cpu().numpy()
        for t in range(T):
            o = (obs0 if t == 0 else res["obs"][t - 1]).cpu().numpy().astype(np.float64)
            want, _, mg = actor_actions(ocfg, o, sd, 31, sc0 + t, env_offset=5)
            ok = mg > 1e-5
            assert ok.mean() > 0.8, (start, t)
            np.testing.assert_array_equal(acts[t][ok], want[ok], err_msg=f"start {start} step {t}")
            checked += int(ok.sum())
    assert checked > 0.8 * 4 * T * B
    env.close()


# ---- the fused closed-loop driver against the eager one ---------------------------------------------------------------

def _drive(uavtrack, sds, script, fuse, k=4, wrap=None):
    """Run `script(ro, set_policy)` on a fresh 64 x 20 x 10 environment under BatchedRollout (eager or fused chunks);
    returns (obs, ep_sums, state) at the end."""
    cfg = uavtrack.EnvConfig(n_envs=64, n_uav=20, m_targets=10)
    env = uavtrack.BatchedUavEnv(cfg)
    if wrap is not None:
        wrap(env)
    actor = uavtrack.ActorMLP(hidden_dim=sds[0]["fc1.weight"].shape[0], action_dim=12)
    actor.load_state_dict({k: torch.from_numpy(v) for k, v in sds[0].items()})
    ro = uavtrack.BatchedRollout(env, actor, steps_per_graph=k, use_graph=False, seed=8, device_actor=True,
                                 fuse_chunks=fuse)

    def set_policy(i):
        sd = sds[i]
        if sd["fc1.weight"].shape[0] != ro.policy.fc1.weight.shape[0]:
            ro.policy = uavtrack.ActorMLP(hidden_dim=sd["fc1.weight"].shape[0], action_dim=12)
        ro.policy.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        ro.sync_actor()
    ro.reset(seed=3)
    script(ro, set_policy)
    torch.cuda.synchronize()
    out = (ro.obs.clone(), ro.ep.clone(), env.get_state())
    env.close()
    return out


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), what
    for k, v in a[2].items():
        assert torch.equal(v, b[2][k]), (what, k)
    np.testing.assert_allclose(b[1].cpu().numpy(), a[1].cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg=what)


def test_fused_driver_follows_seed_changes(uavtrack):
    """A run() after `ro.seed` changed draws with the new key -- fused chunks and graph replay alike."""
    sds = [policy(128, 12, 0)]

    def script(ro, _):
        ro.run(13)
        ro.seed = 99
        ro.run(13)
    eager = _drive(uavtrack, sds, script, fuse=False)
    _same(eager, _drive(uavtrack, sds, script, fuse=True), "seed change, fused chunks")
    # (graph replay: the captured launches hold the seed too)
    cfg = uavtrack.EnvConfig(n_envs=64, n_uav=20, m_targets=10)
    env = uavtrack.BatchedUavEnv(cfg)
    actor = uavtrack.ActorMLP(hidden_dim=128, action_dim=12)
    actor.load_state_dict({k: torch.from_numpy(v) for k, v in sds[0].items()})
    ro = uavtrack.BatchedRollout(env, actor, steps_per_graph=4, use_graph=True, seed=8, device_actor=True)
    ro.reset(seed=3)
    script(ro, None)
    torch.cuda.synchronize()
    assert torch.equal(ro.obs, eager[0]), "seed change, graph replay"
    env.close()


def test_fused_driver_follows_the_current_stream(uavtrack):
    """A second run() under a fresh torch.cuda.Stream issues every launch there -- bound calls included (each call's
    stream is recorded when bound and compared with the current one when called) -- and gives the eager result."""
    sds = [policy(128, 12, 0)]
    log = []

    def wrap(env):
        bind = env.bind_run

        def bind_run(*a, **kw):
            bound_to = env._stream().value
            call = bind(*a, **kw)

            def logged():
                log.append((bound_to, torch.cuda.current_stream().cuda_stream))
                return call()
            return logged
        env.bind_run = bind_run

    streams = {}

    def script(ro, _):
        ro.run(13)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        streams["fresh"] = s.cuda_stream
        n0 = len(log)
        with torch.cuda.stream(s):
            ro.run(13)
        streams["calls"] = log[n0:]
        torch.cuda.current_stream().wait_stream(s)
    fused = _drive(uavtrack, sds, script, fuse=True, wrap=wrap)
    calls = streams["calls"]
    assert len(calls) >= 2
    assert all(b == c == streams["fresh"] for b, c in calls), calls
    _same(_drive(uavtrack, sds, script, fuse=False), fused, "fresh stream")


@pytest.mark.parametrize("what", ["ring_fold", "reset_between", "sync_actor"])
def test_fused_driver_equals_eager(uavtrack, what):
    """fuse_chunks=True == the eager driver, bitwise in observations and state: a run() longer than the 256-row
    episode-sum ring (its fold), reset() between runs, sync_actor() after a learner update at the same width and at a new
    one (the library reallocates the weights)."""
    base = policy(128, 12, 0)
    sds = [base]
    if what == "ring_fold":
        def script(ro, _):
            ro.run(2 * 260 + 1)
        k = 2
    elif what == "reset_between":
        def script(ro, _):
            ro.run(9)
            ro.reset(seed=4)
            ro.run(10)
        k = 4
    else:
        upd = {kk: v.copy() for kk, v in base.items()}
        r = np.random.RandomState(1)
        for kk in upd:                                              # one SGD-sized step on every parameter
            upd[kk] = (upd[kk] - 0.05 * r.randn(*upd[kk].shape)).astype(np.float32)
        sds = [base, upd, policy(200, 12, 2)]

        def script(ro, set_policy):
            ro.run(9)
            set_policy(1)
            ro.run(9)
            set_policy(2)
            ro.run(10)
        k = 4
    _same(_drive(uavtrack, sds, script, fuse=False, k=k), _drive(uavtrack, sds, script, fuse=True, k=k), what)
