"""The device learner (uavtrack_learner_*, uavtrack.DeviceActorCritic) on the MI355X: against the reference's recorded
fp32 updates, against the float64 mirror (tests/learner_mirror.py) and a float64 torch.optim.Adam run; determinism,
graph capture, interop with ActorMLP / BatchedUavEnv / the reference's checkpoint format, and refused inputs."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import learner_harness as lh
import learner_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV


def _uav():
    import uavtrack
    return uavtrack


def _store(z):
    return {"states": torch.from_numpy(z["store_states"]).to(DEV),
            "actions": torch.from_numpy(z["store_actions"]).to(DEV),
            "rewards": torch.from_numpy(z["store_rewards"]).to(DEV),
            "next_states": torch.from_numpy(z["store_next_states"]).to(DEV)}


def _opt(L):
    m, v, st = L._optim_state()
    return m, v, st


@pytest.mark.parametrize("case", ["h128", "h48", "n1"])
def test_golden_reference_updates(case):
    z, meta = load_golden("f5_actor_critic_update")
    H, A, cap = meta["cases"][case]["hidden"], meta["A"], meta["capacity"]
    L = lh.learner(H, A, lr=(meta["actor_lr"], meta["critic_lr"]), gamma=meta["gamma"], blob=z[f"{case}_w0"])
    store = _store(z)
    prio = torch.from_numpy(z["prio_before"]).to(DEV) if case == "h128" else None
    for u in range(5):
        idx = torch.from_numpy(z[f"{case}_idx"][u]).to(DEV)
        al, cl, td = L._run(idx.numel(), store, cap, idx, prio if u == 0 else None)
        assert float(al) == pytest.approx(float(z[f"{case}_actor_loss"][u]), rel=1e-5)
        assert float(cl) == pytest.approx(float(z[f"{case}_critic_loss"][u]), rel=1e-5)
        np.testing.assert_allclose(td.cpu().numpy(), z[f"{case}_td"][u], rtol=1e-5, atol=2e-6)
        if u in (0, 4):
            np.testing.assert_allclose(L._get_params(), z[f"{case}_params{u + 1}"], rtol=1e-5, atol=2e-6)
            assert np.array_equal(_opt(L)[2], z[f"{case}_step{u + 1}"])
        if u == 0 and prio is not None:
            np.testing.assert_allclose(prio.cpu().numpy(), z["prio_after"], rtol=1e-5, atol=2e-6)
            untouched = np.setdiff1d(np.arange(cap), z[f"{case}_idx"][0])
            assert np.array_equal(prio.cpu().numpy()[untouched], z["prio_before"][untouched])
    L.check()


@pytest.mark.parametrize("H,A,n,loss,gather", lh.SWEEP)
def test_sweep_against_fp64_mirror(H, A, n, loss, gather):
    """One update against the float64 mirror, at the bounds tests/learner_harness.py states and explains."""
    rng = np.random.RandomState(H * 1000 + n)
    cap = n + 7 if gather else n
    s, a, r, s2 = lh.batch(rng, cap, A)
    idx = rng.randint(0, cap, size=n).astype(np.int64) if gather else np.arange(n)
    blob = lh.init_blob(H, A, H + n)
    L = lh.learner(H, A, loss=loss, blob=blob, max_batch=max(n, 1))
    store = {"states": torch.from_numpy(s).to(DEV), "actions": torch.from_numpy(a).to(DEV),
             "rewards": torch.from_numpy(r).to(DEV), "next_states": torch.from_numpy(s2).to(DEV)}
    it = torch.from_numpy(idx).to(DEV) if gather else None
    al, cl, td = L._run(n, store, cap, it, None)
    L.check()
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, s[idx], a[idx], r[idx], s2[idx], 0.95, loss)[:4]
    lh.assert_losses_and_td(al.cpu().numpy(), cl.cpu().numpy(), td.cpu().numpy(), ral, rcl, rtd)
    lh.assert_step_from_zero(lh.state(L), blob, g, n, H, A)


def test_trajectory_tracks_fp64_torch_adam():
    """50 updates on fresh batches against the reference update run in float64 torch (torch.optim.Adam).  Bound:
    parameters within 2e-3 * lr * steps + 1e-5 relative (rounding differences are amplified only where a gradient
    element sits near 0, and Adam bounds every step by about lr)."""
    u = _uav()
    H, A, n, lr = 64, 12, 4096, (1e-3, 5e-3)
    rng = np.random.RandomState(3)
    blob = lh.init_blob(H, A, 5)
    L = lh.learner(H, A, lr=lr, blob=blob)
    actor, critic = u.ActorMLP(12, H, A).double(), u.ValueMLP(12, H).double()
    params = list(actor.parameters()) + list(critic.parameters())
    o = 0
    with torch.no_grad():
        for p in params:
            p.copy_(torch.from_numpy(blob[o:o + p.numel()].astype(np.float64)).view_as(p)); o += p.numel()
    oa, oc = torch.optim.Adam(actor.parameters(), lr=lr[0]), torch.optim.Adam(critic.parameters(), lr=lr[1])
    for _ in range(50):
        s, a, r, s2 = lh.batch(rng, n, A)
        L.update({"states": torch.from_numpy(s).to(DEV), "actions": torch.from_numpy(a).to(DEV),
                  "rewards": torch.from_numpy(r).to(DEV), "next_states": torch.from_numpy(s2).to(DEV)})
        S, S2, R = (torch.from_numpy(x.astype(np.float64)) for x in (s, s2, r))
        Ai = torch.from_numpy(a.astype(np.int64)).view(-1, 1)
        target = R + 0.95 * critic(S2)
        delta = target - critic(S)
        logp = torch.log(actor(S).gather(1, Ai))
        al = torch.mean(-logp * delta.detach())          # [n,1] * [n]: the reference's broadcast
        cl = torch.nn.functional.mse_loss(critic(S), target.detach())
        oa.zero_grad(); oc.zero_grad(); al.backward(); cl.backward(); oa.step(); oc.step()
    L.check()
    ref = np.concatenate([p.detach().numpy().ravel() for p in params])
    err = np.abs(L._get_params() - ref)
    assert err.max() <= 2e-3 * lr[1] * 50 + 1e-5 * np.abs(ref).max(), err.max()
    assert np.median(err) <= 1e-5 * lr[1] * 50, np.median(err)


def _setup_det(H=128, A=12, n=4096, seed=9):
    rng = np.random.RandomState(seed)
    cap = n + 100
    s, a, r, s2 = lh.batch(rng, cap, A)
    store = {"states": torch.from_numpy(s).to(DEV), "actions": torch.from_numpy(a).to(DEV),
             "rewards": torch.from_numpy(r).to(DEV), "next_states": torch.from_numpy(s2).to(DEV)}
    idx = torch.from_numpy(rng.randint(0, cap, size=(3, n)).astype(np.int64)).to(DEV)
    return store, idx, cap, lh.init_blob(H, A, seed)


def test_determinism_bitwise():
    store, idx, cap, blob = _setup_det()
    outs = []
    for _ in range(2):
        L = lh.learner(128, 12, blob=blob)
        res = [L._run(idx.shape[1], store, cap, idx[k], None) for k in range(3)]
        L.check()
        outs.append((L._get_params(), _opt(L), [tuple(t.cpu().numpy() for t in r) for r in res]))
    assert np.array_equal(outs[0][0], outs[1][0])
    for x, y in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(x, y)
    for ra, rb in zip(outs[0][2], outs[1][2]):
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)


def test_graph_capture_replay_matches_eager():
    store, idx, cap, blob = _setup_det(seed=10)
    prio_e = torch.rand(cap, device=DEV)
    prio_g = prio_e.clone()
    eager = lh.learner(128, 12, blob=blob)
    e_out = [eager._run(idx.shape[1], store, cap, idx[k], prio_e) for k in range(3)]
    graphed = lh.learner(128, 12, blob=blob)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = [graphed._run(idx.shape[1], store, cap, idx[k], prio_g) for k in range(3)]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(_opt(graphed)[2], np.zeros(8))        # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(graphed._get_params(), eager._get_params())
    assert np.array_equal(_opt(graphed)[2], np.full(8, 3))
    for ra, rb in zip(e_out, g_out):
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
    assert torch.equal(prio_e, prio_g)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_opt(graphed)[2], np.full(8, 6))      # the device step counter advances on replay
    graphed.check(); eager.check()


def test_interop_actor_env_and_checkpoints(tmp_path):
    u = _uav()
    store, idx, cap, blob = _setup_det(H=128, A=12, seed=11)
    L = lh.learner(128, 12, blob=blob)
    for k in range(3):
        L._run(idx.shape[1], store, cap, idx[k], None)
    L.check()
    sd = L.actor_state_dict()
    actor = u.ActorMLP(12, 128, 12)
    actor.load_state_dict(sd)
    x = store["states"][:512].cpu()
    flat = L._get_params()
    w1, b1 = flat[:12 * 128].reshape(128, 12), flat[12 * 128:13 * 128]
    w2, b2 = flat[13 * 128:25 * 128].reshape(12, 128), flat[25 * 128:25 * 128 + 12]
    z = np.maximum(x.numpy() @ w1.T + b1, 0) @ w2.T + b2
    assert np.array_equal(actor(x).argmax(1).numpy(), z.argmax(1))
    # BatchedUavEnv.set_actor with the learner's actor == with an ActorMLP holding the same weights
    cfg = u.EnvConfig(n_envs=4, n_uav=20, m_targets=10)
    acts = []
    for w in (sd, actor.state_dict()):
        env = u.BatchedUavEnv(cfg, DEV)
        env.reset(seed=3)
        env.set_actor(w)
        obs = env.reset(seed=3)
        acts.append(env.actor_actions(obs, seed=5).cpu())
        env.close()
    assert torch.equal(acts[0], acts[1])
    # save / load through the reference's checkpoint format; torch.optim.Adam accepts the optimizer state
    L.save(str(tmp_path), 7)
    pa, pc = tmp_path / "actor" / "actor_weights_7.pth", tmp_path / "critic" / "critic_weights_7.pth"
    ck = torch.load(str(pa))
    assert set(ck) == {"model_state_dict", "optimizer_state_dict"}
    torch.optim.Adam(actor.parameters(), lr=1e-3).load_state_dict(ck["optimizer_state_dict"])
    critic = u.ValueMLP(12, 128)
    ckc = torch.load(str(pc))
    critic.load_state_dict(ckc["model_state_dict"])
    torch.optim.Adam(critic.parameters(), lr=5e-3).load_state_dict(ckc["optimizer_state_dict"])
    L2 = lh.learner(128, 12)
    L2.load(str(pa), str(pc))
    assert np.array_equal(L2._get_params(), L._get_params())
    for x1, x2 in zip(_opt(L2), _opt(L)):
        assert np.array_equal(x1, x2)
    sd_all = L.state_dict()
    L3 = lh.learner(128, 12)
    L3.load_state_dict(sd_all)
    assert np.array_equal(L3._get_params(), L._get_params())


def test_refused_inputs_leave_the_learner_unchanged():
    import ctypes as C
    from uavtrack import _lib
    store, idx, cap, blob = _setup_det(H=64, A=12, n=1000, seed=12)
    L = lh.learner(64, 12, blob=blob, max_batch=1000)
    L._run(1000, store, cap, idx[0], None)
    L.check()
    before = (L._get_params(), _opt(L))
    prio = torch.rand(cap, device=DEV)
    prio0 = prio.clone()
    lib = _lib.load()
    out = torch.empty(2, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    # a null required pointer, n above the reserved size, n < 1: refused on the host
    assert lib.uavtrack_learner_update(L._h, 10, None, p(store["actions"]), p(store["rewards"]), p(store["next_states"]),
                                       cap, p(idx[0]), p(out[0:1]), p(out[1:2]), None, None, None) != 0
    assert lib.uavtrack_learner_update(L._h, 10, p(store["states"]), p(store["actions"]), p(store["rewards"]),
                                       p(store["next_states"]), cap, p(idx[0]), None, p(out[1:2]), None, None, None) != 0
    with pytest.raises(RuntimeError, match="reserved"):
        L._run(1001, store, cap, torch.zeros(1001, dtype=torch.int64, device=DEV), None)
    # an action out of range, an index out of range: refused on the device, reported by check()
    bad = {k: v.clone() for k, v in store.items()}
    bad["actions"][int(idx[1][5])] = 12
    al, cl, _ = L._run(1000, bad, cap, idx[1], prio)
    assert torch.isnan(al) and torch.isnan(cl)
    with pytest.raises(RuntimeError, match="refused"):
        L.check()
    bi = idx[1].clone(); bi[3] = cap
    L._run(1000, store, cap, bi, prio)
    bad["actions"][int(idx[1][5])] = -1
    L._run(1000, bad, cap, idx[1], prio)
    with pytest.raises(RuntimeError, match="2 update"):
        L.check()
    L.check()                                                  # the count restarts
    after = (L._get_params(), _opt(L))
    assert np.array_equal(before[0], after[0])
    for x, y in zip(before[1], after[1]):
        assert np.array_equal(x, y)
    assert torch.equal(prio, prio0)
    # hidden out of range: create refuses
    for H in (0, 257):
        with pytest.raises(RuntimeError, match="hidden"):
            lh.learner(H, 12)
    with pytest.raises(RuntimeError, match="n_actions"):
        lh.learner(64, 49)
    # a failing set leaves the previous state in place
    with pytest.raises(RuntimeError):
        L._set_params(np.zeros(5, np.float32))
    assert np.array_equal(L._get_params(), before[0])
    # a refused optimizer-state load: the wrong size, a negative step, a negative or NaN exp_avg_sq; the arrays differ
    # from the current state everywhere, so a partial copy would show
    m0, v0, st0 = before[1]
    P = L.num_params
    for n, bad in ((P - 1, None), (P, ("st", 3, -1)), (P, ("v", 7, -1e-3)), (P, ("v", P - 1, np.nan))):
        arr = {"m": m0 + 1.0, "v": v0 + 1.0, "st": st0 + 1}
        if bad:
            arr[bad[0]][bad[1]] = bad[2]
        with pytest.raises(RuntimeError, match="uavtrack_learner_set_optimizer_state: "):
            _lib.check(lib.uavtrack_learner_set_optimizer_state(L._h, *(C.c_void_p(arr[q].ctypes.data) for q in
                                                                        ("m", "v", "st")), n, None))
        assert np.array_equal(L._get_params(), before[0])
        for a, b in zip(before[1], _opt(L)):
            assert np.array_equal(a, b)
    # a device that does not exist: create refuses
    with pytest.raises(RuntimeError, match=r"uavtrack_learner_create: device_id \d+ out of range"):
        _uav().DeviceActorCritic(12, 64, 12, device=f"cuda:{torch.cuda.device_count()}")


def test_update_from_prioritized_buffer_writes_priorities():
    u = _uav()
    rng = np.random.RandomState(13)
    s, a, r, s2 = lh.batch(rng, 3000, 12)
    buf = u.PrioritizedDeviceReplayBuffer(4000, DEV)
    buf.add({"states": torch.from_numpy(s), "actions": torch.from_numpy(a), "rewards": torch.from_numpy(r),
             "next_states": torch.from_numpy(s2)})
    L = lh.learner(64, 12, blob=lh.init_blob(64, 12, 1))
    gen = torch.Generator(device=DEV); gen.manual_seed(4)
    p0 = buf.priorities.clone()
    al, cl, td = L.update_from(buf, 2048, generator=gen)
    gen.manual_seed(4)
    prob = p0[:buf.count] ** buf.alpha
    idx = torch.multinomial(prob / prob.sum(), 2048, replacement=True, generator=gen).cpu().numpy()
    want = mirror.last_wins(p0.cpu().numpy(), idx, np.abs(td.cpu().numpy()))
    assert np.array_equal(buf.priorities.cpu().numpy(), want.astype(np.float32))
    L.check()
    ub = u.DeviceReplayBuffer(4000, DEV)
    ub.add({"states": torch.from_numpy(s), "actions": torch.from_numpy(a), "rewards": torch.from_numpy(r),
            "next_states": torch.from_numpy(s2)})
    al, cl, td = L.update_from(ub, 1024)
    assert td.shape == (1024,) and torch.isfinite(al)
    L.check()
