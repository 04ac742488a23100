"""The device PMI trainer (uavtrack_pmi_trainer_*, uavtrack.DevicePMINetwork) on the MI355X: against the reference's
recorded fp32 train_pmi calls (tests/golden/f6_pmi_train.npz), against the float64 mirror (tests/pmi_trainer_mirror.py);
determinism, graph capture, interop with make_pmi_net / the reference's checkpoint format / the MAAC-R scorer, refused
inputs and the example.

The pre-BatchNorm biases (and any weight column whose input is constant over a batch) have an analytic gradient of
exactly zero; the reference's fp32 values for them are rounding noise that Adam turns into real moves.  Those elements
are told apart by the float64 mirror (its gradient is zero to ~1e-17 there) and are only bounded: one Adam step moves
an element by at most lr (1 - beta1) / sqrt(1 - beta2) ~= 3.2 lr, so two runs that start equal differ by at most
twice that per step taken."""
import os

import numpy as np
import pytest
import torch

import pmi_trainer_fixture as fixture
import pmi_trainer_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 1e-3
STEP_BOUND = LR * (1 - mirror.BETA1) / np.sqrt(1 - mirror.BETA2)     # largest move of one Adam step


def _uav():
    import uavtrack
    return uavtrack


def _trainer(H, b2, sd=None, max_batch=0):
    tr = _uav().DevicePMINetwork(H, b2, DEV, lr=LR, max_batch=max_batch)
    if sd is not None:
        tr.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return tr


def _call(tr, rows, n_uav, t, u, bs):
    """One train_pmi call on given triples -> (avg_loss, losses [nb], outputs [nb, 2, bs]) on the host."""
    nb = len(t) // bs
    losses = torch.empty(nb, device=DEV)
    outs = torch.empty(nb, 2, bs, device=DEV)
    avg = tr.train_indices(torch.as_tensor(rows, device=DEV, dtype=torch.float32).contiguous(), n_uav,
                           torch.as_tensor(t, device=DEV, dtype=torch.int64).contiguous(),
                           torch.as_tensor(u, device=DEV, dtype=torch.int64).contiguous(), bs, losses=losses,
                           outputs=outs)
    return float(avg), losses.cpu().numpy(), outs.cpu().numpy()


def _flat_params(sd):
    return np.concatenate([np.asarray(sd[k], np.float64).ravel() for k in mirror.param_names()])


def _noise_mask(rec):
    """Trainable elements whose float64 gradient is zero at every step of the call (see the module docstring)."""
    g = np.max([np.abs(_flat_params(gr)) for gr in rec["grads"]], axis=0)
    return g < 1e-12


def _sd_np(tr):
    return {k: v.numpy() for k, v in tr.state_dict().items()}


@pytest.mark.parametrize("case", ["h64", "h128"])
def test_golden_reference_calls(case):
    """Two consecutive calls from the fixture's initial state.  Tolerances: the float64 mirror reproduces these fp32
    recordings to 2e-6 (outputs), 4e-6 (data-determined parameters), 2.5e-6 (running_var); the device's own fp32
    rounding is of the same size, so twice to five times those.  The fixture holds fc1.weight at a sample of its
    elements; every element of every tensor is also compared with the float64 mirror run alongside (2e-5 for the
    data-determined ones).  Noise-driven elements (and running_mean, which follows the pre-BN biases) are bounded by
    2 x STEP_BOUND per step taken so far."""
    z, meta, rows = fixture.load()
    c = meta["cases"][case]
    H, bs, b2, n_uav = c["hidden"], c["batch_size"], c["b2_size"], meta["n_uav"]
    sd0 = fixture.initial_state(z, meta, case)
    tr = _trainer(H, b2, sd0)
    msd, mad = sd0, mirror.new_adam()
    steps = 0
    for call in range(2):
        t, u = fixture.indices(z, meta, case, call)
        avg, losses, outs = _call(tr, rows, n_uav, t, u, bs)
        msd, mad, mavg, rec = mirror.train_pmi(msd, mad, rows, n_uav, t, u, bs)
        steps += b2 // bs
        ref_avg = float(z[f"{case}_c{call}_avg_loss"])
        assert avg == pytest.approx(ref_avg, rel=1e-5), (call, avg, ref_avg)
        np.testing.assert_allclose(losses, np.abs(rec["loss"]), rtol=2e-5)
        np.testing.assert_allclose(outs[:, 0], z[f"{case}_c{call}_o12"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(outs[:, 1], z[f"{case}_c{call}_o13"], rtol=1e-5, atol=1e-5)
        noise = _noise_mask(rec)
        assert noise.sum() == 4 * H                            # the four pre-BN bias vectors
        sd = _sd_np(tr)
        dm = np.abs(_flat_params(sd) - _flat_params(msd))      # every element, against the mirror
        assert dm[~noise].max() < 2e-5, dm[~noise].max()
        nv = fixture.view_flat(noise, H, z, case)
        d = np.abs(fixture.view(sd, z, case) - fixture.recorded(z, case, call))
        assert d[~nv].max() < 2e-5, d[~nv].max()
        assert d[nv].max() <= 2 * steps * STEP_BOUND, d[nv].max()
        for bn in ("bn_comm", "bn_obs", "bn_boundary_state", "bn1"):
            np.testing.assert_allclose(sd[bn + ".running_var"], z[f"{case}_c{call}_sd_{bn}.running_var"], rtol=1e-5,
                                       atol=1e-5)
            drm = np.abs(sd[bn + ".running_mean"] - z[f"{case}_c{call}_sd_{bn}.running_mean"]).max()
            assert drm <= 2 * steps * STEP_BOUND, (bn, drm)
            assert int(sd[bn + ".num_batches_tracked"]) == int(z[f"{case}_c{call}_sd_{bn}.num_batches_tracked"])
        m, v, st = tr.optimizer_state()
        np.testing.assert_array_equal(st, z[f"{case}_c{call}_step"])
        if call == 1:                                           # the moments are recorded after the second call
            mv, vv = fixture.view_flat(m, H, z, case), fixture.view_flat(v, H, z, case)
            np.testing.assert_allclose(mv[~nv], z[f"{case}_c1_exp_avg"][~nv], rtol=1e-4, atol=2e-7)
            np.testing.assert_allclose(vv[~nv], z[f"{case}_c1_exp_avg_sq"][~nv], rtol=1e-4, atol=1e-10)
    tr.check()


def test_golden_smallest_batch():
    """H 48, batch 2, b2 10.  With two rows every BatchNorm output is +-|d| / sqrt(d^2 + eps), and the f3 history has
    features constant over such a pair, so almost every gradient in front of a BatchNorm is fp32 rounding noise in
    the reference (the float64 mirror itself leaves the recording by 1.5e-2 from the second batch on).  The first
    batch is compared tightly; after it, outputs within 5e-2 and every recorded parameter within 2 x STEP_BOUND per
    step; the counters exactly."""
    z, meta, rows = fixture.load()
    case = "h48"
    c = meta["cases"][case]
    H, bs, b2, n_uav = c["hidden"], c["batch_size"], c["b2_size"], meta["n_uav"]
    tr = _trainer(H, b2, fixture.initial_state(z, meta, case))
    steps = 0
    for call in range(2):
        t, u = fixture.indices(z, meta, case, call)
        avg, losses, outs = _call(tr, rows, n_uav, t, u, bs)
        steps += b2 // bs
        o12, o13 = z[f"{case}_c{call}_o12"], z[f"{case}_c{call}_o13"]
        if call == 0:
            np.testing.assert_allclose(outs[0, 0], o12[0], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(outs[0, 1], o13[0], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(outs[:, 0], o12, atol=5e-2)
        np.testing.assert_allclose(outs[:, 1], o13, atol=5e-2)
        assert avg == pytest.approx(float(z[f"{case}_c{call}_avg_loss"]), abs=5e-2)
        sd = _sd_np(tr)
        d = np.abs(fixture.view(sd, z, case) - fixture.recorded(z, case, call))
        assert d.max() <= 2 * steps * STEP_BOUND, d.max()
        for bn in ("bn_comm", "bn_obs", "bn_boundary_state", "bn1"):
            assert int(sd[bn + ".num_batches_tracked"]) == 2 * steps
        np.testing.assert_array_equal(tr.optimizer_state()[2], z[f"{case}_c{call}_step"])
    tr.check()


def _history(rng, T, n_uav):
    x = rng.uniform(-1, 1, size=(T * n_uav, 12)).astype(np.float32)
    x[:, 9:11] = rng.uniform(0, 5, size=(T * n_uav, 2))
    return x


@pytest.mark.parametrize("bs", [2, 64, 128, 500, 1024])
@pytest.mark.parametrize("H", [1, 32, 64, 96, 128, 200, 256])
def test_sweep_against_fp64_mirror(H, bs):
    """Two mini-batch steps (b2 = 2 bs + 1: the remainder row is dropped, as in the reference) on a random in-range
    history.  Losses and outputs of both steps: 1e-4 relative (the second step runs on parameters after one Adam
    step).  Data-determined elements (gradient at least 1e-5 at both steps) within 5e-4: the fp32 torch path on the
    CPU leaves the mirror by up to 4e-4 on these grids, where a second-step gradient is small next to the first and
    its fp32 error moves the second Adam step; the smaller data-determined and the noise-driven elements within
    2 x STEP_BOUND per step.  running_var 1e-4 relative.  Batch 2 gets ten times the output, loss and running_var
    tolerances and 2e-3 on the data-determined elements: with two rows a normalised value is +-d / sqrt(d^2 + eps), so
    where d^2 is near eps the fp32 rounding of d is amplified up to 1 / sqrt(eps) ~ 316 times (measured on the device:
    1.5e-4 on outputs, 5.5e-4 on parameters at H >= 128)."""
    rng = np.random.RandomState(H * 1000 + bs)
    T, n_uav = 40, 10
    rows = _history(rng, T, n_uav)
    b2 = 2 * bs + 1
    t, u = rng.randint(0, T, size=b2), rng.randint(0, n_uav, size=(b2, 2))
    torch.manual_seed(H + bs)
    sd0 = {k: v.numpy().copy() for k, v in _uav().make_pmi_net(H).state_dict().items()}
    tr = _trainer(H, b2, sd0)
    avg, losses, outs = _call(tr, rows, n_uav, t, u, bs)
    msd, _, mavg, rec = mirror.train_pmi(sd0, mirror.new_adam(), rows, n_uav, t, u, bs)
    tol = 1e-3 if bs == 2 else 1e-4
    np.testing.assert_allclose(losses, np.abs(rec["loss"]), rtol=tol)
    assert avg == pytest.approx(mavg, rel=tol)
    np.testing.assert_allclose(outs[:, 0], np.stack(rec["o12"]), rtol=tol, atol=tol)
    np.testing.assert_allclose(outs[:, 1], np.stack(rec["o13"]), rtol=tol, atol=tol)
    gmin = np.min([np.abs(_flat_params(g)) for g in rec["grads"]], axis=0)
    big = gmin >= 1e-5
    d = np.abs(_flat_params(_sd_np(tr)) - _flat_params(msd))
    assert d[big].max() < (2e-3 if bs == 2 else 5e-4), d[big].max()
    assert d.max() <= 2 * 2 * STEP_BOUND, d.max()
    for bn in ("bn_comm", "bn_obs", "bn_boundary_state", "bn1"):
        np.testing.assert_allclose(_sd_np(tr)[bn + ".running_var"], msd[bn + ".running_var"], rtol=tol, atol=1e-5)
    tr.check()


def _setup(H=128, bs=128, b2=1000, seed=3):
    rng = np.random.RandomState(seed)
    T, n_uav = 50, 20
    rows = torch.from_numpy(_history(rng, T, n_uav)).to(DEV)
    t = torch.from_numpy(rng.randint(0, T, size=b2)).to(DEV)
    u = torch.from_numpy(rng.randint(0, n_uav, size=(b2, 2))).to(DEV)
    torch.manual_seed(seed)
    sd = {k: v.numpy().copy() for k, v in _uav().make_pmi_net(H).state_dict().items()}
    return rows, n_uav, t, u, sd


def _full_state(tr):
    st, nbt = tr._get()
    m, v, steps = tr.optimizer_state()
    return st, nbt, m, v, steps


def test_determinism_bitwise():
    rows, n_uav, t, u, sd = _setup()
    a, b = _trainer(128, 1000, sd), _trainer(128, 1000, sd)
    ra = [float(a.train_indices(rows, n_uav, t, u, 128)) for _ in range(2)]
    rb = [float(b.train_indices(rows, n_uav, t, u, 128)) for _ in range(2)]
    assert ra == rb
    for x, y in zip(_full_state(a), _full_state(b)):
        assert np.array_equal(x, y)


def test_graph_capture_replay_matches_eager():
    rows, n_uav, t, u, sd = _setup(seed=4)
    eager = _trainer(128, 1000, sd)
    e_avg = [float(eager.train_indices(rows, n_uav, t, u, 128)) for _ in range(3)]
    graphed = _trainer(128, 1000, sd)
    avg = torch.empty((), device=DEV)
    losses = torch.empty(1000 // 128, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            graphed.train_indices(rows, n_uav, t, u, 128, avg_loss=avg, losses=losses)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(graphed.optimizer_state()[2], np.zeros(18))     # capture ran nothing
    g_avg = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        g_avg.append(float(avg))
        assert np.array_equal(graphed.optimizer_state()[2], np.full(18, 7 * (k + 1)))   # device step counts advance
    assert g_avg == e_avg
    for x, y in zip(_full_state(graphed), _full_state(eager)):
        assert np.array_equal(x, y)
    graphed.check()


def test_train_pmi_draws_reference_triples():
    """train_pmi draws (timestep, uav-pair) as sample_pmi_pairs does: under one seed both see the same rows."""
    rows, n_uav, _, _, sd = _setup(H=64, seed=5)
    a, b = _trainer(64, 640, sd), _trainer(64, 640, sd)
    torch.manual_seed(77)
    la = a.train_pmi({"pmi": {"batch_size": 64}}, rows, n_uav)
    torch.manual_seed(77)
    _, t, uu = _uav().sample_pmi_pairs(rows, n_uav, 640)
    lb = float(b.train_indices(rows, n_uav, t.contiguous(), uu.contiguous(), 64))
    assert la == lb
    for x, y in zip(_full_state(a), _full_state(b)):
        assert np.array_equal(x, y)
    dev_g = torch.Generator(device=DEV)
    dev_g.manual_seed(1)
    out = a.train_pmi({"pmi": {"batch_size": 64}}, rows.view(50, 1, n_uav, 12), n_uav, generator=dev_g, sync=False)
    assert out.device.type == "cuda" and np.isfinite(float(out))


def test_state_dict_roundtrip_with_make_pmi_net():
    rows, n_uav, t, u, sd = _setup(H=64, seed=6)
    tr = _trainer(64, 1000, sd)
    tr.train_indices(rows, n_uav, t, u, 100)
    out = tr.state_dict()
    ref = _uav().make_pmi_net(64).state_dict()
    assert list(out.keys()) == list(ref.keys()) and len(out) == 30
    net = _uav().make_pmi_net(64)
    net.load_state_dict(out)
    tr2 = _trainer(64, 1000)
    tr2.load_state_dict(net.state_dict())
    for k, v in tr2.state_dict().items():
        assert torch.equal(v, out[k]), k
    assert int(out["bn1.num_batches_tracked"]) == 20


def test_save_load_reference_checkpoint_format(tmp_path):
    rows, n_uav, t, u, sd = _setup(H=32, seed=7)
    tr = _trainer(32, 1000, sd)
    tr.train_indices(rows, n_uav, t, u, 250)
    tr.save(str(tmp_path), 3)
    path = os.path.join(str(tmp_path), "pmi", "pmi_weights_3.pth")
    ck = torch.load(path)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict"}
    assert list(ck["model_state_dict"]) == list(_uav().make_pmi_net(32).state_dict())
    net = _uav().make_pmi_net(32)
    net.load_state_dict(ck["model_state_dict"])
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    opt.load_state_dict(ck["optimizer_state_dict"])              # the reference's PMINetwork.load does this
    assert len(opt.state) == 18 and all(float(s["step"]) == 4 for s in opt.state.values())
    # the reverse: a torch make_pmi_net + Adam checkpoint in the reference's format
    torch.manual_seed(8)
    net = _uav().make_pmi_net(32)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    x = torch.rand(16, 12)
    for _ in range(2):
        opt.zero_grad()
        _uav().pmi_contrastive_loss(net(x[:8]), net(x[8:])).backward()
        opt.step()
    torch.save({"model_state_dict": net.state_dict(), "optimizer_state_dict": opt.state_dict()}, path)
    tr2 = _trainer(32, 1000)
    tr2.load(path)
    for k, v in net.state_dict().items():
        assert torch.equal(tr2.state_dict()[k], v), k
    m, v, st = tr2.optimizer_state()
    assert np.array_equal(st, np.full(18, 2))
    np.testing.assert_array_equal(m, np.concatenate([opt.state[p]["exp_avg"].numpy().ravel() for p in net.parameters()]))
    np.testing.assert_array_equal(v, np.concatenate([opt.state[p]["exp_avg_sq"].numpy().ravel() for p in net.parameters()]))


def test_set_pmi_matches_eval_mode_net():
    """env.set_pmi(trainer) uploads the folded eval-mode network; its scores match make_pmi_net in eval mode with the
    trainer's state_dict within the scorer's tolerance against an fp64 forward (tests/test_hip_round4.py: 2e-4)."""
    uav = _uav()
    rows, n_uav, t, u, sd = _setup(H=128, seed=9)
    tr = _trainer(128, 1000, sd)
    tr.train_indices(rows, n_uav, t, u, 128)
    env = uav.BatchedUavEnv(uav.EnvConfig(n_envs=4, n_uav=20, m_targets=10, cooperative=0.3,
                                          reward_mode=uav.RewardMode.PMI), DEV)
    env.set_pmi(tr)
    x = (torch.rand(512, 12, device=DEV) * 2 - 1).contiguous()
    got = env.pmi_inference(x).cpu().numpy()
    net = uav.make_pmi_net(128).double().eval()
    net.load_state_dict(tr.state_dict())
    with torch.no_grad():
        ref = net(x.cpu().double()).numpy().reshape(-1)
    assert np.abs(got - ref).max() < 2e-4 * max(1.0, np.abs(ref).max())
    env.close()


def test_refusals_change_nothing():
    rows, n_uav, t, u, sd = _setup(H=64, seed=11)
    tr = _trainer(64, 1000, sd, max_batch=256)
    before = _full_state(tr)
    for bs, tt, kw in ((1, t, {}), (2000, t, {}), (500, t[:100], {"u": u[:100]}), (512, t, {})):
        with pytest.raises((RuntimeError, ValueError)):
            tr.train_indices(rows, n_uav, tt, kw.get("u", u), bs)
    for H in (0, 257):
        with pytest.raises((RuntimeError, ValueError)):
            _uav().DevicePMINetwork(H, 1000, DEV)
    with pytest.raises(RuntimeError, match=r"uavtrack_pmi_trainer_create: device_id \d+ out of range"):
        _uav().DevicePMINetwork(64, 1000, f"cuda:{torch.cuda.device_count()}")
    for x, y in zip(before, _full_state(tr)):
        assert np.array_equal(x, y)
    # a refused optimizer-state load: the wrong size, a negative step, a negative or NaN exp_avg_sq; the arrays differ
    # from the current state everywhere, so a partial copy would show
    import ctypes as C
    from uavtrack import _lib
    lib = _lib.load()
    _, _, m0, v0, st0 = before
    P = tr.num_params
    for n, bad in ((P - 1, None), (P, ("st", 5, -1)), (P, ("v", 9, -1e-3)), (P, ("v", P - 1, np.nan))):
        arr = {"m": m0 + 1.0, "v": v0 + 1.0, "st": st0 + 1}
        if bad:
            arr[bad[0]][bad[1]] = bad[2]
        with pytest.raises(RuntimeError, match="uavtrack_pmi_trainer_set_optimizer_state: "):
            _lib.check(lib.uavtrack_pmi_trainer_set_optimizer_state(tr._h, *(C.c_void_p(arr[q].ctypes.data) for q in
                                                                             ("m", "v", "st")), n, None))
        for a, b in zip(before, _full_state(tr)):
            assert np.array_equal(a, b)
    tr.reserve(512)
    tr.train_indices(rows, n_uav, t, u, 512)                    # fits after the reserve
    tr.check()


@pytest.mark.parametrize("which", ["t_low", "t_high", "u_high"])
def test_out_of_range_index_is_a_device_side_noop(which):
    rows, n_uav, t, u, sd = _setup(H=64, seed=12)
    tr = _trainer(64, 1000, sd)
    tr.check()
    before = _full_state(tr)
    t, u = t.clone(), u.clone()
    if which == "t_low":
        t[777] = -1
    elif which == "t_high":
        t[3] = 50
    else:
        u[999, 1] = n_uav
    losses = torch.zeros(1000 // 100, device=DEV)
    avg = tr.train_indices(rows, n_uav, t, u, 100, losses=losses)
    assert np.isnan(float(avg)) and torch.isnan(losses).all()
    for x, y in zip(before, _full_state(tr)):
        assert np.array_equal(x, y)
    with pytest.raises(RuntimeError, match="refused"):
        tr.check()
    tr.check()                                                  # the count restarts


def test_example_maac_r_with_device_pmi_trainer():
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    import train_maac
    hist = train_maac.main(["--method", "maac-r", "--pmi-trainer", "device", "--envs", "64", "--steps", "20",
                            "--iters", "2", "--batch", "4096", "--updates", "2"])
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
