"""The automatic-reset policy rollouts without a GPU: the three new entry points and the start_obs setter are declared
in include/uavtrack.h, exported by the library and bound in uavtrack/_lib.py with matching arguments, and
transitions_from_rollout with done / start_obs equals a plain Python loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from uavtrack import _lib, transitions_from_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uavtrack_run_actor_autoreset", "uavtrack_run_greedy_autoreset", "uavtrack_replay_add_rollout_episodes",
       "uavtrack_set_start_obs_output")
# how a parameter of the header is bound
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_bound_argument_by_argument(name):
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/uavtrack.h"
    params = [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]
    assert name in _lib.SIGNATURES, f"{name} is not bound in uavtrack/_lib.py"
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params), (name, params, args)
    for p, a in zip(params, args):
        if "*" in p:
            want = C.POINTER(_lib.ReplayRing) if "uavtrack_replay_ring" in p else C.c_void_p
        else:
            want = CTYPE[p.split()[0]]
        assert a is want, (name, p, a)
    assert hasattr(_lib.load(), name)


def _loop(obs_in, out):
    obs, done, so = out["obs"], out.get("done"), out.get("start_obs")
    T, B, N, D = obs.shape
    states = np.empty((T, B, N, D), np.float32)
    for t in range(T):
        for b in range(B):
            for i in range(N):
                if t == 0:
                    states[t, b, i] = obs_in[b, i]
                elif done is not None and so is not None and done[t - 1, b]:
                    states[t, b, i] = so[t - 1, b, i]
                else:
                    states[t, b, i] = obs[t - 1, b, i]
    return states.reshape(-1, D)


@pytest.mark.parametrize("T", [1, 2, 7])
def test_transitions_from_rollout_across_episode_ends(T):
    rng = np.random.RandomState(T)
    B, N = 5, 3
    obs_in = torch.from_numpy(rng.randn(B, N, 12).astype(np.float32))
    out = dict(obs=torch.from_numpy(rng.randn(T, B, N, 12).astype(np.float32)),
               actions=torch.from_numpy(rng.randint(0, 12, (T, B, N)).astype(np.int32)),
               reward=torch.from_numpy(rng.randn(T, B, N).astype(np.float32)),
               done=torch.from_numpy((rng.rand(T, B) < 0.4).astype(np.uint8)),
               start_obs=torch.from_numpy(rng.randn(T, B, N, 12).astype(np.float32)))
    out["done"][-1, 0] = 1                                   # a done on the last step has no transition behind it
    tr = transitions_from_rollout(obs_in, out)
    np.testing.assert_array_equal(tr["states"].numpy(), _loop(obs_in.numpy(), {k: v.numpy() for k, v in out.items()}))
    np.testing.assert_array_equal(tr["next_states"].numpy(), out["obs"].numpy().reshape(-1, 12))
    np.testing.assert_array_equal(tr["actions"].numpy(), out["actions"].numpy().reshape(-1))
    np.testing.assert_array_equal(tr["rewards"].numpy(), out["reward"].numpy().reshape(-1))
    # without both keys: today's statement
    for drop in ("done", "start_obs"):
        old = transitions_from_rollout(obs_in, {k: v for k, v in out.items() if k != drop})
        plain = {k: v.numpy() for k, v in out.items() if k in ("obs", "actions", "reward")}
        np.testing.assert_array_equal(old["states"].numpy(), _loop(obs_in.numpy(), plain))
    if T > 1 and out["done"][:-1].any():
        assert not torch.equal(tr["states"], old["states"])
