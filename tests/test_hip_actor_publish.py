"""Device publish of the rollout actor (uavtrack_publish_actor_weights, uavtrack_learner_publish_actor): the blob packed on
the device from device tensors equals the host pack of uavtrack_set_actor_weights bit for bit -- at every width, in 2-D
and 3-D, at the scale clamps, with the softmax guard, subnormal, NaN and infinite weights -- leaves nothing of the
previous weights behind, publishes the learner's weights of the moment a captured graph replays, and refuses what does
not fit with the installed blob untouched.  A training loop that publishes on the device computes what the host-publish
loop computes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HIDDEN = (1, 7, 32, 33, 128, 256, 1000, 4096)
VARIANTS = ("default", "rescale_up", "rescale_down", "zeros", "guard_b2", "guard_w2", "subnormal", "nonfinite")


def _uav():
    import uavtrack
    return uavtrack


def make_env(A=12, B=4, N=4):
    uav = _uav()
    kw = {} if A == 12 else dict(dim=3, na=12, nc=A // 12, z_max=300.0)
    return uav.BatchedUavEnv(uav.EnvConfig(n_envs=B, n_uav=N, m_targets=4, **kw), DEV)


def weights(H, A, variant="default", seed=0):
    """ActorMLP's default initialisation (CPU fp32), then the variant."""
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in _uav().ActorMLP(hidden_dim=H, action_dim=A).state_dict().items()}
    w1, b1, w2, b2 = (sd[k] for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))
    if variant in ("rescale_up", "rescale_down"):
        # the same policy with the layers rescaled against each other, j past the +-60 clamp of the block scales
        j = 70 if variant == "rescale_up" else -70
        w1.mul_(2.0 ** j); b1.mul_(2.0 ** j); w2.mul_(2.0 ** -j)
    elif variant == "zeros":
        for t in (w1, b1, w2, b2):
            t.zero_()
    elif variant == "guard_b2":
        b2[A - 1] = 3.0e8                 # the logit bound passes 2^28 through b2 alone
    elif variant == "guard_w2":
        w2.mul_(1.0e9)
    elif variant == "subnormal":
        for t in (w1, b1, w2, b2):
            t.mul_(1.0e-40)               # fp32 subnormals
    elif variant == "nonfinite":
        w1[0, 3] = float("nan"); w1[H - 1, 5] = float("inf")
        w2[1, 0] = float("nan"); w2[A - 2, H - 1] = float("-inf")
    return sd


def on_device(sd):
    return {k: v.to(DEV) for k, v in sd.items()}


def assert_same_bits(host, dev, what=""):
    h, d = host.view(np.uint32), dev.view(np.uint32)
    assert h.shape == d.shape, (what, h.shape, d.shape)
    bad = np.flatnonzero(h != d)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[0]}: host {h[bad[0]]:08x}, device {d[bad[0]]:08x}"


@pytest.fixture(scope="module")
def envs():
    e = {12: make_env(12), 48: make_env(48)}
    yield e
    for v in e.values():
        v.close()


@pytest.mark.parametrize("A", (12, 48))
@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("variant", VARIANTS)
def test_device_pack_equals_host_pack(envs, A, H, variant):
    env = envs[A]
    sd = weights(H, A, variant)
    env.set_actor(sd)
    host = env.actor_blob()
    if variant.startswith("guard"):
        assert host[1] == 1.0                                       # the case covers the guard flag
    env.set_actor(weights(H, A, "default", seed=99))                # other weights in the blob first
    env.publish_actor(on_device(sd))
    assert_same_bits(host, env.actor_blob(), f"A={A} H={H} {variant}")


@pytest.mark.parametrize("A,H", ((12, 33), (36, 33), (48, 100), (12, 4096)))
def test_publish_leaves_no_stale_word(A, H):
    env, fresh = make_env(A), make_env(A)
    for second in ("default", "zeros"):
        env.set_actor(weights(H, A, "guard_w2", seed=1))            # header flag, every fragment nonzero
        nxt = weights(H, A, second, seed=2)
        env.publish_actor(on_device(nxt))
        fresh.set_actor(nxt)
        assert_same_bits(fresh.actor_blob(), env.actor_blob(), f"A={A} H={H} then {second}")


def filled_ring(uav, learner, env, T=20, seed=3):
    """A prioritised ring holding one rollout of env under the learner's actor."""
    per = env.B * env.N * T
    ring = uav.PrioritizedReplayRing(2 * per, DEV, seed=seed, max_batch=4096)
    env.set_actor(learner.actor_state_dict())
    obs_in = env.reset(seed=seed)
    res = env.run_actor(T, obs_in, seed=seed)
    ring.add_rollout(obs_in, res)
    return ring


def test_learner_and_torch_actor_publish_match_host():
    uav = _uav()
    torch.manual_seed(5)
    env = make_env(12, B=16, N=8)
    learner = uav.DeviceActorCritic(12, 128, 12, device=DEV, max_batch=4096)
    ring = filled_ring(uav, learner, env)
    for _ in range(4):
        learner.update_from(ring, 1024)
    learner.publish_actor(env)
    dev = env.actor_blob()
    env.set_actor(learner.actor_state_dict())
    assert_same_bits(env.actor_blob(), dev, "DeviceActorCritic after 4 updates")
    learner.check()
    ring.check()

    actor = uav.ActorMLP(hidden_dim=128, action_dim=12).to(DEV)
    opt = torch.optim.Adam(actor.parameters(), lr=1e-2)
    x = torch.randn(256, 12, device=DEV)
    loss = -torch.log(actor(x)[:, 3]).mean()
    opt.zero_grad(); loss.backward(); opt.step()
    env.set_actor(actor)
    host = env.actor_blob()
    env.set_actor(weights(128, 12, seed=7))
    env.publish_actor(actor)
    assert_same_bits(host, env.actor_blob(), "ActorMLP on the GPU after an Adam step")
    # a non-contiguous tensor is made contiguous on the device
    sd = dict(actor.state_dict())
    sd["fc2.weight"] = sd["fc2.weight"].t().contiguous().t()
    assert not sd["fc2.weight"].is_contiguous()
    env.set_actor(weights(128, 12, seed=7))
    env.publish_actor(sd)
    assert_same_bits(host, env.actor_blob(), "non-contiguous fc2.weight")


def train(publish, iters=3, B=256, N=10, T=50, H=64, updates=3, batch=4096, seed=11):
    """The loop of examples/train_maac.py (device learner, prioritised ring) with host or device publish; nothing is
    synchronised between the steps of the device-publish loop."""
    uav = _uav()
    torch.manual_seed(seed)
    cfg = uav.EnvConfig(n_envs=B, n_uav=N, m_targets=10, horizon=T)
    env = uav.BatchedUavEnv(cfg, DEV)
    learner = uav.DeviceActorCritic(12, H, 12, device=DEV, max_batch=batch)
    actor = uav.ActorMLP(hidden_dim=H, action_dim=12).to(DEV)
    actor.load_state_dict(learner.actor_state_dict())
    rollout = uav.BatchedRollout(env, actor, device_actor=True, seed=seed)
    ring = uav.PrioritizedReplayRing(2 * B * N * T, DEV, seed=seed, max_batch=batch)
    seen = []
    for it in range(iters):
        rollout.seed = seed + it
        rollout.reset(seed=1000 + it)
        obs_in = rollout.obs.clone()
        res = rollout.run_fused(T)
        ring.add_rollout(obs_in, res)
        seen.append({k: res[k].clone() for k in ("obs", "actions", "reward")})
        for _ in range(updates):
            learner.update_from(ring, batch)
        if publish == "host":
            actor.load_state_dict(learner.actor_state_dict())
            rollout.sync_actor()
        else:
            learner.publish_actor(env)
    torch.cuda.synchronize()
    out = dict(seen=[{k: v.cpu().numpy() for k, v in s.items()} for s in seen],
               priorities=ring.priorities.cpu().numpy(), params=learner._get_params(), blob=env.actor_blob())
    ring.check()
    learner.check()
    return out


def test_training_loop_device_publish_equals_host_publish():
    a, b = train("host"), train("device")
    for it, (sa, sb) in enumerate(zip(a["seen"], b["seen"])):
        for k in sa:
            assert_same_bits(np.ascontiguousarray(sa[k]).view(np.uint32), np.ascontiguousarray(sb[k]).view(np.uint32),
                             f"iteration {it} {k}")
    assert_same_bits(a["priorities"], b["priorities"], "ring priorities")
    assert_same_bits(a["params"], b["params"], "learner parameters")
    assert_same_bits(a["blob"], b["blob"], "final actor blob")


def test_learner_publish_captures_and_reads_at_replay():
    uav = _uav()
    torch.manual_seed(13)
    env, ref = make_env(12, B=16, N=8), make_env(12)
    learner = uav.DeviceActorCritic(12, 96, 12, device=DEV, max_batch=4096)
    ring = filled_ring(uav, learner, env)
    before = env.actor_blob()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        learner.publish_actor(env)                     # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        learner.publish_actor(env)
    for _ in range(3):
        learner.update_from(ring, 1024)
    g.replay()
    got = env.actor_blob()
    ref.set_actor(learner.actor_state_dict())
    assert_same_bits(ref.actor_blob(), got, "replayed publish after 3 updates")
    assert not np.array_equal(before.view(np.uint32), got.view(np.uint32))
    learner.check()


def test_refusals_leave_the_blob_unchanged():
    uav = _uav()
    env = make_env(12)
    with pytest.raises(RuntimeError, match="no actor installed"):
        env.publish_actor(on_device(weights(64, 12)))
    with pytest.raises(RuntimeError):
        env.actor_blob()

    env.set_actor(weights(64, 12, seed=1))
    blob = env.actor_blob()

    def unchanged(what):
        torch.cuda.synchronize()
        assert_same_bits(blob, env.actor_blob(), what)

    with pytest.raises(RuntimeError, match="hidden 128"):
        env.publish_actor(on_device(weights(128, 12)))
    unchanged("hidden mismatch")
    learner = uav.DeviceActorCritic(12, 128, 12, device=DEV)
    with pytest.raises(RuntimeError, match="hidden 128"):
        learner.publish_actor(env)
    unchanged("learner hidden mismatch")

    env3 = make_env(48)
    env3.set_actor(weights(128, 48, seed=1))
    blob3 = env3.actor_blob()
    with pytest.raises(RuntimeError, match="12 actions"):
        learner.publish_actor(env3)
    torch.cuda.synchronize()
    assert_same_bits(blob3, env3.actor_blob(), "learner / env action mismatch")

    sd = on_device(weights(64, 12))
    bad = {"dtype": dict(sd, **{"fc1.weight": sd["fc1.weight"].double()}),
           "device": dict(sd, **{"fc2.bias": sd["fc2.bias"].cpu()}),
           "shape w1": dict(sd, **{"fc1.weight": sd["fc1.weight"][:, :11]}),
           "shape w2": dict(sd, **{"fc2.weight": sd["fc2.weight"][:11]}),
           "shape b1": dict(sd, **{"fc1.bias": sd["fc1.bias"][:63]}),
           "missing": {k: v for k, v in sd.items() if k != "fc2.bias"}}
    for what, src in bad.items():
        with pytest.raises(ValueError):
            env.publish_actor(src)
        unchanged(what)
    with pytest.raises(ValueError):
        env.publish_actor(uav.ActorMLP(hidden_dim=64, action_dim=12))      # on the CPU
    unchanged("CPU module")
