"""Device publish of the MAAC-R scorer's weights (uavtrack_publish_pmi_weights, uavtrack_pmi_trainer_publish): BatchNorm
fold, bounds, scales and every packed layout computed on the device equal, word for word over the whole allocation, what
fold_pmi_state_dict + uavtrack_set_pmi_weights write from the same numbers -- at every width class, after training, at the
scale clamps, with weights unfit for f16, subnormal, NaN and infinite ones -- leave nothing of earlier weights behind, give
the host path's scores (through the f16 kernel, through its gate when the weights are unfit, through the fp32 kernel),
publish the trainer's weights of the moment a captured graph replays, and refuse what does not fit with the installed
allocation untouched.  A MAAC-R loop that publishes on the device computes what the host-publish loop computes.

The block scales come from the exponent field of the quotient target / bound on both sides (csrc/pmi_pack.h), not from a
log2, so no case has to stay away from powers of two."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN = (1, 7, 32, 33, 64, 96, 100, 128, 160, 256)
VARIANTS = ("default", "trained", "var0", "gamma", "big", "small", "subnormal", "nonfinite_branch", "nonfinite_fc1")
SPLIT = (64, 96, 128)                      # padded widths with bf16 / f16 planes
LIN = ("fc_comm", "fc_obs", "fc_boundary_state", "fc1", "fc2")
BN = ("bn_comm", "bn_obs", "bn_boundary_state", "bn1")


def _uav():
    import uavtrack
    return uavtrack


def make_env(B=4, N=4, pmi=False, **kw):
    uav = _uav()
    if pmi:
        kw.update(reward_mode=uav.RewardMode.PMI, cooperative=0.3, horizon=20)
    return uav.BatchedUavEnv(uav.EnvConfig(n_envs=B, n_uav=N, m_targets=4, **kw), DEV)


def train_rows(T=12, n_uav=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T * n_uav, 12, generator=g).to(DEV), n_uav


def trained(H, calls=3, seed=0):
    """A DevicePMINetwork after a few train_pmi calls: running statistics, gamma and beta are non-trivial."""
    torch.manual_seed(seed)
    net = _uav().DevicePMINetwork(H, 64, DEV)
    rows, n_uav = train_rows(seed=seed)
    for _ in range(calls):
        net.train_pmi({"pmi": {"batch_size": 16}}, rows, n_uav)
    net.check()
    return net


def weights(H, variant="default", seed=0):
    """make_pmi_net's float state (CPU fp32), then the variant."""
    if variant == "trained":
        sd = trained(H, seed=seed).state_dict()
        return {k: v.clone() for k, v in sd.items() if v.dtype == torch.float32}
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in _uav().make_pmi_net(H).state_dict().items() if v.dtype == torch.float32}
    g = torch.Generator().manual_seed(seed + 1)
    for b in BN:                               # statistics and affine terms away from (0, 1, 1, 0)
        sd[b + ".running_mean"].copy_(0.3 * torch.randn(H, generator=g))
        sd[b + ".running_var"].copy_(0.5 + torch.rand(H, generator=g))
        sd[b + ".weight"].copy_(1.0 + 0.2 * torch.randn(H, generator=g))
        sd[b + ".bias"].copy_(0.1 * torch.randn(H, generator=g))
    if variant == "var0":
        for b in BN:
            sd[b + ".running_var"].zero_()
    elif variant == "gamma":
        for b in BN:
            sd[b + ".weight"][::2] = 0.0
            sd[b + ".weight"][1::3] *= -1.0
    elif variant in ("big", "small", "subnormal"):
        f = {"big": 2.0 ** 10, "small": 2.0 ** -20, "subnormal": 1.0e-40}[variant]
        for l in LIN[:4]:
            sd[l + ".weight"].mul_(f)
            sd[l + ".bias"].mul_(f)
        if variant != "big":
            for b in BN:
                sd[b + ".running_mean"].mul_(f)
                sd[b + ".bias"].mul_(f)
    elif variant == "nonfinite_branch":
        sd["fc_comm.weight"][0, 2] = float("nan")
        sd["fc_obs.weight"][H - 1, 1] = float("inf")
        sd["fc_boundary_state.weight"][H // 2, 0] = float("-inf")
    elif variant == "nonfinite_fc1":
        sd["fc1.weight"][0, 1] = float("nan")
        sd["fc1.weight"][H - 1, 3 * H - 1] = float("-inf")
    return sd


def on_device(sd):
    return {k: v.to(DEV) for k, v in sd.items()}


def assert_same_bits(host, dev, what=""):
    h, d = np.asarray(host).view(np.uint32), np.asarray(dev).view(np.uint32)
    assert h.shape == d.shape, (what, h.shape, d.shape)
    bad = np.flatnonzero(h != d)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[0]}: host {h[bad[0]]:08x}, device {d[bad[0]]:08x}"


def fit_word(blob):
    return int(blob[-8 + 5])                    # csrc/pmi_pack.h: the scalar block's f16 verdict


def padded(H):
    return (H + 31) // 32 * 32


@pytest.fixture(scope="module")
def envs():
    e = {"default": make_env(), "far": make_env(x_max=30000.0, y_max=30000.0)}
    yield e
    for v in e.values():
        v.close()


@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("variant", VARIANTS)
def test_device_pack_equals_host_pack(envs, H, variant):
    env = envs["default"]
    sd = weights(H, variant)
    env.set_pmi(sd)
    host = env.pmi_blob()
    if padded(H) in SPLIT:
        if variant == "big":
            assert fit_word(host) == 0                              # the case covers the unfit verdict ...
        if variant == "default":
            assert fit_word(host) == 1                              # ... and the fit one
        if variant in ("small", "subnormal"):
            assert host[-1:].view(np.float32)[0] == 2.0 ** 15       # T at its upper clamp
        if variant.startswith("nonfinite"):
            assert fit_word(host) == 0
    env.set_pmi(weights(H, "default", seed=99))                     # other weights in the allocation first
    env.publish_pmi(on_device(sd))
    assert_same_bits(host, env.pmi_blob(), f"H={H} {variant}")
    assert env.pmi_publish_info()["device_published"]
    assert env.pmi_info()["f16_range_ok"] == (padded(H) in SPLIT and fit_word(host) == 1)


@pytest.mark.parametrize("H", (33, 64, 128, 256))
def test_large_position_bound(envs, H):
    """x_max / dc = 60: pos^2 = 57600 is beyond the f16 kernel's operand range on its own."""
    env = envs["far"]
    sd = weights(H, "default")
    env.set_pmi(sd)
    host = env.pmi_blob()
    if padded(H) in SPLIT:
        assert fit_word(host) == 0
    env.set_pmi(weights(H, "default", seed=99))
    env.publish_pmi(on_device(sd))
    assert_same_bits(host, env.pmi_blob(), f"far H={H}")


@pytest.mark.parametrize("H", (7, 64, 100, 160))
def test_publish_leaves_no_stale_word(H):
    env, fresh = make_env(), make_env()
    env.set_pmi(weights(H, "default", seed=7))
    for second in ("zeros", "default"):
        env.publish_pmi(on_device(weights(H, "big", seed=1)))       # unfit, every word of the planes non-zero
        nxt = weights(H, "default", seed=2)
        if second == "zeros":
            nxt = {k: torch.zeros_like(v) for k, v in nxt.items()}
        env.publish_pmi(on_device(nxt))
        fresh.set_pmi(nxt)
        assert_same_bits(fresh.pmi_blob(), env.pmi_blob(), f"H={H} then {second}")
    env.close(); fresh.close()


def _counters(env):
    return env.pmi_info()["rescored_chunks"], env.pmi_publish_info()["unfit_chunks"]


@pytest.mark.parametrize("H,variant,kind", ((128, "default", "fit"), (64, "default", "fit"), (64, "big", "unfit"),
                                            (128, "big", "unfit"), (160, "default", "fp32")))
def test_same_scores_as_host_path(H, variant, kind):
    sd = weights(H, variant, seed=3)
    host, dev = make_env(B=8, N=6, pmi=True), make_env(B=8, N=6, pmi=True)
    host.set_pmi(sd)
    dev.set_pmi(weights(H, "default", seed=99))
    dev.publish_pmi(on_device(sd))
    assert dev.pmi_info()["scheme"] == host.pmi_info()["scheme"] == {"fit": "f16x3", "unfit": "bf16x6", "fp32": "fp32"}[kind]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(300, 12, generator=g).to(DEV)
    wild = x.clone()
    wild[5, 9] = 3.0e6                                              # beyond what an f16 operand takes: the run-time range watch
    wild[200, 2] = -7.0e5
    r0, u0 = _counters(dev)
    assert_same_bits(host.pmi_inference(x).cpu().numpy(), dev.pmi_inference(x).cpu().numpy(), f"{kind} inference")
    r1, u1 = _counters(dev)
    assert r1 == r0 and u1 - u0 == (1 if kind == "unfit" else 0)
    assert_same_bits(host.pmi_inference(wild).cpu().numpy(), dev.pmi_inference(wild).cpu().numpy(), f"{kind} wild rows")
    r2, u2 = _counters(dev)
    assert r2 - r1 == (1 if kind == "fit" else 0) and u2 - u1 == (1 if kind == "unfit" else 0)
    if kind == "fit":
        assert host.pmi_info()["rescored_chunks"] == 1              # the host path's own watch saw the same rows
    # a 20-step MAAC-R rollout
    acts = torch.randint(0, 12, (20, 8, 6), generator=g).to(device=DEV, dtype=torch.int32)
    outs = []
    for env in (host, dev):
        env.reset(seed=5, episode=0)
        outs.append(env.step_many(acts))
    for k in ("reward", "obs", "ep_sums"):
        assert_same_bits(outs[0][k].cpu().numpy(), outs[1][k].cpu().numpy(), f"{kind} step_many {k}")
    r3, u3 = _counters(dev)
    assert r3 == r2 and u3 - u2 == (1 if kind == "unfit" else 0)
    assert host.pmi_publish_info() == dict(device_published=False, unfit_chunks=0)
    # the next host upload takes the handle back to the host's verdict
    dev.set_pmi(sd)
    assert not dev.pmi_publish_info()["device_published"]
    assert_same_bits(host.pmi_inference(x).cpu().numpy(), dev.pmi_inference(x).cpu().numpy(), f"{kind} after set_pmi")
    assert _counters(dev)[1] == u3
    host.close(); dev.close()


@pytest.mark.parametrize("H", (64, 100, 128, 192))
def test_trainer_module_and_state_dict_sources(H):
    uav = _uav()
    env = make_env()
    net = trained(H, seed=2)
    env.set_pmi(net)
    host = env.pmi_blob()
    other = weights(H, "default", seed=99)
    env.set_pmi(other)
    net.publish_pmi(env)
    assert_same_bits(host, env.pmi_blob(), f"H={H} trainer")
    env.set_pmi(other)
    env.publish_pmi(net)                                            # the same through the environment's method
    assert_same_bits(host, env.pmi_blob(), f"H={H} trainer via env")
    module = uav.make_pmi_net(H)
    module.load_state_dict(net.state_dict())
    module = module.to(DEV)
    env.set_pmi(other)
    env.publish_pmi(module)
    assert_same_bits(host, env.pmi_blob(), f"H={H} module")
    env.set_pmi(other)
    sd = on_device(weights(H, "trained", seed=2))
    sd["fc1.weight"] = sd["fc1.weight"].t().contiguous().t()        # a non-contiguous view of the same numbers
    assert not sd["fc1.weight"].is_contiguous()
    env.publish_pmi(sd)
    assert_same_bits(host, env.pmi_blob(), f"H={H} state dict")
    env.close()


def test_graph_capture_replay_matches_eager_host_publish():
    """{train_indices; publish_pmi; MAAC-R step_many} captured once, replayed three times (a capture fails on any
    synchronisation or allocation) against an eager loop that trains with the same indices and publishes through the host."""
    uav = _uav()
    H, T, B, N, b2, bs = 128, 20, 8, 6, 256, 64
    g = torch.Generator().manual_seed(21)
    rows = torch.randn(T * N, 12, generator=g).to(DEV)
    t_idx = torch.randint(0, T, (b2,), generator=g).to(DEV)
    u_idx = torch.randint(0, N, (b2, 2), generator=g).to(DEV)
    acts = torch.randint(0, 12, (T, B, N), generator=g).to(device=DEV, dtype=torch.int32)
    torch.manual_seed(8)
    sd0 = uav.make_pmi_net(H).state_dict()

    def fresh():
        env = make_env(B=B, N=N, pmi=True)
        net = uav.DevicePMINetwork(H, b2, DEV)
        net.load_state_dict(sd0)
        env.set_pmi(net)
        env.reset(seed=9, episode=0)
        return env, net
    # eager, host publish
    env_e, net_e = fresh()
    rewards_e = []
    for _ in range(3):
        net_e.train_indices(rows, N, t_idx, u_idx, bs)
        env_e.set_pmi(net_e)
        rewards_e.append(env_e.step_many(acts)["reward"].cpu().numpy().copy())
    blob_e = env_e.pmi_blob()
    # captured, device publish
    env_g, net_g = fresh()
    out = env_g.step_many(acts)                                     # buffers; then back to the start state
    env_g.reset(seed=9, episode=0)
    avg = torch.empty((), device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            net_g.train_indices(rows, N, t_idx, u_idx, bs, avg_loss=avg)
            net_g.publish_pmi(env_g)
            env_g.step_many(acts, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(rewards_e[k], out["reward"].cpu().numpy(), f"replay {k} rewards")
    assert_same_bits(blob_e, env_g.pmi_blob(), "final allocation")
    net_g.check()
    for e in (env_e, env_g):
        e.close()


def test_example_loop_device_publish_equals_host_publish():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_maac
    common = ["--envs", "32", "--n-uav", "6", "--m-targets", "6", "--steps", "20", "--iters", "5", "--updates", "2",
              "--batch", "1024", "--hidden", "64", "--pmi-hidden", "64", "--pmi-b2", "256", "--pmi-batch", "64",
              "--replay", "prioritized", "--pmi-draw", "device",
              "--method", "maac-r", "--pmi-trainer", "device", "--learner", "device"]
    dev = train_maac.main(common + ["--publish", "device", "--log-every", "3"])
    host = train_maac.main(common + ["--publish", "host", "--log-every", "3"])
    assert len(dev) == 5 and np.all(np.isfinite(dev))
    assert dev == host


def test_refusals_leave_the_allocation_untouched():
    uav = _uav()
    H = 64
    sd = on_device(weights(H, "default", seed=4))
    bare = make_env()
    with pytest.raises(RuntimeError, match="no weights installed"):
        bare.publish_pmi(sd)
    with pytest.raises(RuntimeError, match="no weights installed"):
        bare.pmi_blob()
    bare.close()
    env = make_env()
    env.set_pmi(weights(H, "default", seed=5))
    before = env.pmi_blob()

    def refused(exc, source, match=None):
        with pytest.raises(exc, match=match):
            env.publish_pmi(source)
        assert_same_bits(before, env.pmi_blob(), "after a refusal")
    refused(RuntimeError, on_device(weights(128, "default")), "hidden 128")
    refused(RuntimeError, on_device(weights(50, "default")), "hidden 50")       # the same padded width is another width still
    refused(ValueError, weights(H, "default"), "cuda")                           # CPU tensors
    refused(ValueError, {k: v.double() for k, v in sd.items()}, "float32")
    refused(ValueError, {k: v for k, v in sd.items() if k != "bn1.running_var"}, "bn1.running_var")
    bad = dict(sd); bad["fc_obs.weight"] = sd["fc_obs.weight"][:, :3].contiguous()
    refused(ValueError, bad, "fc_obs")
    bad = dict(sd); bad["bn_comm.bias"] = sd["bn_comm.bias"][:-1].contiguous()
    refused(ValueError, bad, "fc_comm")
    if torch.cuda.device_count() > 1:
        refused(ValueError, {k: v.to("cuda:1") for k, v in sd.items()}, "cuda:0")
        other = uav.DevicePMINetwork(H, 64, "cuda:1")
        refused(RuntimeError, other, "device")
    refused(RuntimeError, uav.DevicePMINetwork(128, 64, DEV), "hidden 128")
    # the C ABI: a null pointer among the 26
    import ctypes as C
    from uavtrack import _lib
    ts, _ = env._pmi_publish_tensors(sd, 0)
    arg = _lib.PmiTensors()
    for k, t in enumerate(ts):
        arg.t[k] = t.data_ptr()
    arg.t[17] = None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert env._lib.uavtrack_publish_pmi_weights(env._h, C.byref(arg), H, stream) != 0
    assert b"tensor 17" in env._lib.uavtrack_last_error()
    assert env._lib.uavtrack_publish_pmi_weights(env._h, None, H, stream) != 0
    assert_same_bits(before, env.pmi_blob(), "after null pointers")
    env.close()
