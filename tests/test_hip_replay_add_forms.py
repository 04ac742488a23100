"""The contract the five ring adds share (uavtrack_replay_add, _add_rollout, _add_rollout_episodes, _add_rollout_nstep,
_add_rollout_lambda), on both ring classes: every refusal returns non-zero with its whole message and leaves the ring's
image (stores, discounts, priorities) byte for byte as it was, and the good call lands and advances pos / count.

T = 3, B = 2, N = 7: 42 transitions, into a ring of 100 slots at pos 97 (the write wraps) and a ring of 17 (the rollout
exceeds the ring: only its last 17 transitions land)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, B, N = 3, 2, 7
M = B * N
ROWS = T * M
FORMS = ("add", "add_rollout", "add_rollout_episodes", "add_rollout_nstep", "add_rollout_lambda")
RINGS = ((100, 97), (17, 5))                   # (capacity, pos = count)
GAMMA, LAM, N_STEP = 0.95, 0.9, 3

# per form: the pointers that must not be null with their message, and the row arrays that must be 16-byte aligned with theirs
REQUIRED = {
    "add": (("states", "actions", "rewards", "next_states"), "states, actions, rewards and next_states must not be null"),
    "add_rollout": (("obs_in", "obs", "actions", "reward"), "obs_in, obs, actions and reward must not be null"),
    "add_rollout_episodes": (("obs_in", "obs", "actions", "reward", "done", "start_obs"),
                             "obs_in, obs, actions, reward, done and start_obs must not be null"),
    "add_rollout_nstep": (("discounts", "obs_in", "obs", "actions", "reward"),
                          "discounts, obs_in, obs, actions and reward must not be null"),
    "add_rollout_lambda": (("discounts", "obs_in", "obs", "actions", "reward", "values"),
                           "discounts, obs_in, obs, actions, reward and values must not be null"),
}
ALIGNED = {
    "add": (("states", "next_states"), "states and next_states must be 16-byte aligned"),
    "add_rollout": (("obs_in", "obs"), "obs_in and obs must be 16-byte aligned"),
    "add_rollout_episodes": (("obs_in", "obs", "start_obs"), "obs_in, obs and start_obs must be 16-byte aligned"),
    "add_rollout_nstep": (("obs_in", "obs", "start_obs"), "obs_in, obs and start_obs must be 16-byte aligned"),
    "add_rollout_lambda": (("obs_in", "obs", "start_obs"), "obs_in, obs and start_obs must be 16-byte aligned"),
}
ENVS_FORMS = ("add_rollout_episodes", "add_rollout_nstep", "add_rollout_lambda")
STORES = ("states", "actions", "rewards", "next_states")


def _uav():
    import uavtrack
    return uavtrack


@pytest.fixture(scope="module")
def source():
    """One rollout's outputs (and the same transitions flat), shared and never written."""
    g = torch.Generator(device=DEV).manual_seed(5)
    done = torch.zeros(T, B, dtype=torch.uint8, device=DEV)
    done[1, 0] = 1
    s = {"obs_in": torch.randn(B, N, 12, device=DEV, generator=g),
         "obs": torch.randn(T, B, N, 12, device=DEV, generator=g),
         "actions": torch.randint(0, 12, (T, B, N), device=DEV, generator=g, dtype=torch.int32),
         "reward": torch.randn(T, B, N, device=DEV, generator=g),
         "done": done,
         "start_obs": torch.randn(T, B, N, 12, device=DEV, generator=g),
         "values": torch.randn(T, B, N, device=DEV, generator=g)}
    s["states"] = torch.cat([s["obs_in"][None], s["obs"][:-1]]).reshape(ROWS, 12).contiguous()
    s["next_states"] = s["obs"].reshape(ROWS, 12)
    s["rewards"] = s["reward"].reshape(ROWS)
    torch.cuda.synchronize()
    return s


def _make_ring(form, prioritised, capacity, fill):
    uav = _uav()
    ring = uav.PrioritizedReplayRing(capacity, DEV, seed=3) if prioritised else uav.ReplayRing(capacity, DEV, seed=3)
    if form == "add_rollout_nstep":
        ring.with_nstep(N_STEP, GAMMA)
    if form == "add_rollout_lambda":
        ring.with_lambda(LAM, GAMMA)
    g = torch.Generator(device=DEV).manual_seed(capacity)
    for k in ("states", "rewards", "next_states"):
        ring.store[k].copy_(torch.randn(ring.store[k].shape, device=DEV, generator=g))
    ring.store["actions"].copy_(torch.randint(0, 12, (capacity,), device=DEV, generator=g, dtype=torch.int32))
    if prioritised:
        ring.priorities[:fill] = torch.rand(fill, device=DEV, generator=g) + 0.5
    ring.pos = ring.count = fill
    return ring


def _image(ring):
    """The ring's device state as int32 words (a NaN compares equal to itself)."""
    parts = [ring.store[k] for k in STORES] + [t for t in (ring.discounts, ring.priorities) if t is not None]
    torch.cuda.synchronize()
    return [p.view(torch.int32).clone() for p in parts]


def _base(form, ring, s):
    """The good call's arguments by name: addresses as integers, sizes, scalars."""
    a = {k: v.data_ptr() for k, v in s.items()}
    a.update(n=ROWS, steps=T, agents=M, envs=B, n_uav=N, n_step=N_STEP, lam=LAM, gamma=GAMMA,
             discounts=None if ring.discounts is None else ring.discounts.data_ptr())
    return a


def _call(lib, form, handle, ring_struct, a):
    """One direct library call; returns (rc, message)."""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rp = None if ring_struct is None else C.byref(ring_struct)
    rollout = (a["obs_in"], a["obs"], a["actions"], a["reward"])
    if form == "add":
        args = (a["n"], a["states"], a["actions"], a["rewards"], a["next_states"])
    elif form == "add_rollout":
        args = (a["steps"], a["agents"]) + rollout
    elif form == "add_rollout_episodes":
        args = (a["steps"], a["envs"], a["n_uav"]) + rollout + (a["done"], a["start_obs"])
    elif form == "add_rollout_nstep":
        args = (a["discounts"], a["steps"], a["envs"], a["n_uav"]) + rollout + (a["done"], a["start_obs"], a["n_step"],
                                                                                a["gamma"])
    else:
        args = (a["discounts"], a["steps"], a["envs"], a["n_uav"]) + rollout + (a["done"], a["start_obs"], a["values"],
                                                                                a["lam"], a["gamma"])
    rc = getattr(lib, "uavtrack_replay_" + form)(handle, rp, *args, st)
    return rc, lib.uavtrack_last_error().decode()


def _faults(form, capacity):
    """(label, ring fields to change, arguments to change, the message behind the entry point's name).  The handle and
    ring faults are added by the caller.  Every text is the library's, written out."""
    out = [
        ("pos == capacity", {"pos": capacity}, {}, f"pos {capacity} outside [0, capacity = {capacity})"),
        ("capacity > max_capacity", {"capacity": capacity + 1}, {},
         f"capacity {capacity + 1} outside [1, max_capacity = {capacity}]"),
        ("count > capacity", {"count": capacity + 1}, {}, f"count {capacity + 1} outside [0, capacity = {capacity}]"),
    ]
    for k in STORES:
        out.append((f"ring.{k} null", {k: None}, {}, "the ring's states, actions, rewards and next_states must not be null"))
    for k in ("states", "next_states"):
        out.append((f"ring.{k} + 4", {k: 4}, {}, "the ring's states and next_states must be 16-byte aligned"))
    names, msg = REQUIRED[form]
    for k in names:
        out.append((f"{k} null", {}, {k: None}, msg))
    names, msg = ALIGNED[form]
    for k in names:
        out.append((f"{k} + 4", {}, {k: 4}, msg))
    if form == "add":
        out.append(("n = 0", {}, {"n": 0}, "n = 0 < 1"))
    elif form == "add_rollout":
        out += [("steps = 0", {}, {"steps": 0}, "steps and agents must be >= 1"),
                ("agents = 0", {}, {"agents": 0}, "steps and agents must be >= 1"),
                ("steps = 2**62", {}, {"steps": 2**62}, "steps * agents overflows")]
    else:
        out += [(f"{k} = 0", {}, {k: 0}, "steps, envs and n_uav must be >= 1") for k in ("steps", "envs", "n_uav")]
        out += [("steps = 2**62", {}, {"steps": 2**62}, "steps * envs * n_uav overflows"),
                ("envs = 2**62", {}, {"envs": 2**62}, "steps * envs * n_uav overflows")]
    if form in ("add_rollout_nstep", "add_rollout_lambda"):
        for k in ("done", "start_obs"):
            out.append((f"only {k} null", {}, {k: None}, "done and start_obs must both be given or both be null"))
    if form == "add_rollout_nstep":
        for v in (0, 65):
            out.append((f"n_step = {v}", {}, {"n_step": v}, f"n_step = {v} outside [1, 64]"))
    bad = ((float("nan"), "nan"), (-0.1, "-0.1"), (1.5, "1.5"), (float("inf"), "inf"))
    if form == "add_rollout_lambda":
        for v, text in bad:
            out.append((f"lambda = {text}", {}, {"lam": v}, f"lambda = {text} is not a finite value in [0, 1]"))
    if form in ("add_rollout_nstep", "add_rollout_lambda"):
        for v, text in bad:
            out.append((f"gamma = {text}", {}, {"gamma": v}, f"gamma = {text} is not a finite value in [0, 1]"))
    return out


def _good_call(form, ring, s):
    """The entry point through the ring class, which advances pos / count."""
    if form == "add":
        ring.add({"states": s["states"], "actions": s["actions"], "rewards": s["reward"], "next_states": s["next_states"]})
        return
    out = {k: s[k] for k in ("obs", "actions", "reward")}
    if form != "add_rollout":
        out.update(done=s["done"], start_obs=s["start_obs"])
    if form == "add_rollout_lambda":
        ring.add_rollout(s["obs_in"], out, values=s["values"])
    else:
        ring.add_rollout(s["obs_in"], out)


@pytest.mark.parametrize("prioritised", [False, True], ids=["uniform", "prioritised"])
@pytest.mark.parametrize("form", FORMS)
def test_refusals_change_nothing_and_good_call_lands(form, prioritised, source):
    uav = _uav()
    lib = uav._lib.load()
    fn = "uavtrack_replay_" + form
    for capacity, fill in RINGS:
        ring = _make_ring(form, prioritised, capacity, fill)
        before = _image(ring)
        base = _base(form, ring, source)

        def refused(label, handle, ring_struct, args, text):
            rc, msg = _call(lib, form, handle, ring_struct, args)
            assert rc != 0, (label, capacity)
            assert msg == f"{fn}: {text}", (label, capacity)
            for was, now in zip(before, _image(ring)):
                assert torch.equal(was, now), (label, capacity)

        refused("null handle", None, ring._ring(), base, "null handle")
        refused("null ring", ring._h, None, base, "ring is null")
        for label, ring_over, arg_over, text in _faults(form, capacity):
            rs = ring._ring()
            for k, v in ring_over.items():
                setattr(rs, k, getattr(rs, k) + 4 if v == 4 else v)
            args = dict(base)
            for k, v in arg_over.items():
                args[k] = base[k] + 4 if v == 4 else v
            refused(label, ring._h, rs, args, text)

        # the good call, directly with the arguments every fault above changed one of, then through the ring class
        rc, msg = _call(lib, form, ring._h, ring._ring(), base)
        assert rc == 0, msg
        ring._advance(ROWS)
        assert (ring.pos, ring.count) == ((fill + ROWS) % capacity, min(capacity, fill + ROWS))
        _good_call(form, ring, source)
        assert (ring.pos, ring.count) == ((fill + 2 * ROWS) % capacity, min(capacity, fill + 2 * ROWS))
        after = _image(ring)
        # two adds of 42 wrote every slot of the 17-slot ring and slots [97, 100) + [0, 81) of the 100-slot one
        states, actions, nxt = after[0].reshape(capacity, 12), after[1], after[3].reshape(capacity, 12)
        if capacity == 100:
            assert torch.equal(states[81:97], before[0].reshape(capacity, 12)[81:97])
            assert torch.equal(actions[81:97], before[1][81:97])
            slots, rows = torch.arange(39, 81, device=DEV), slice(0, ROWS)
        else:
            # the last 17 transitions of the second add, from pos (5 + 42) % 17 = 13 on
            slots, rows = (torch.arange(17, device=DEV) + 13 + (ROWS - 17)) % 17, slice(ROWS - 17, ROWS)
        assert torch.equal(actions[slots], source["actions"].reshape(ROWS)[rows])
        if form != "add_rollout_nstep":        # (whose next state is the end of the n-step window)
            assert torch.equal(nxt[slots], source["next_states"].view(torch.int32)[rows])
        ring.check()
        ring.close()
