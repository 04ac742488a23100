"""Multi-step targets without a GPU: the horizon rule of tests/nstep_mirror.py (every window inside its episode and its
rollout, every stop for one of the three reasons), the fp32 Horner return and the repeated-product discount against
float64 within the bounds one rounding per operation gives, n = 1 as uavtrack.transitions_from_rollout, and the three
new symbols declared in include/uavtrack.h, exported by the library and bound in uavtrack/_lib.py with the header's
argument lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nstep_mirror as nm
import uavtrack
from uavtrack import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMAS = (0.0, 0.5, 0.95, 0.99, 1.0)


def _random_case(rng):
    steps, envs = int(rng.integers(1, 12)), int(rng.integers(1, 4))
    n_step = int(rng.choice([1, 2, 3, 5, 8, 11, 64, 69]))
    done = None
    if rng.random() < 0.8:
        done = (rng.random((steps, envs)) < rng.choice([0.0, 0.15, 0.5, 1.0])).astype(np.uint8)
    return steps, envs, n_step, done


def test_windows_stay_inside_their_episode_and_rollout_and_stop_for_a_reason():
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(200):
        steps, envs, n_step, done = _random_case(rng)
        m, why = nm.stop_reasons(steps, envs, n_step, done)
        for t in range(steps):
            for b in range(envs):
                k = int(m[t, b])
                assert 1 <= k <= n_step and t + k <= steps
                if done is not None:                                   # no episode end strictly inside the window
                    assert not done[t:t + k - 1, b].any()
                assert why[t, b], (t, b, k)                            # one of the three reasons holds at m ...
                for j in range(1, k):                                  # ... and none at any smaller m
                    assert j != n_step and t + j != steps and (done is None or done[t + j - 1][b] == 0)
                seen |= why[t, b]
    assert seen == {"n", "tail", "done"}


def test_the_horizon_depends_on_t_and_b_alone_and_n1_is_one():
    done = np.zeros((7, 3), np.uint8)
    done[2, 1] = done[3, 1] = done[6, 0] = 1
    assert (nm.horizon(7, 3, 1, done) == 1).all() and (nm.horizon(7, 3, 1) == 1).all()
    m = nm.horizon(7, 3, 3, done)
    assert m[:, 2].tolist() == [3, 3, 3, 3, 3, 2, 1]
    assert m[:, 1].tolist() == [3, 2, 1, 1, 3, 2, 1]
    assert m[:, 0].tolist() == [3, 3, 3, 3, 3, 2, 1]


def test_return_and_discount_against_float64_within_one_rounding_per_operation():
    """|R - sum g^k r_k| <= 2 m 2^-24 sum g^k |r_k| and |d - g^m| <= m 2^-24 g^m: Horner's m - 1 multiplies and m - 1
    adds (the discount's m - 1 multiplies), each within 2^-24 relative, on terms bounded by sum g^k |r_k| (g^m)."""
    rng = np.random.default_rng(1)
    u = 2.0 ** -24
    worst = [0.0, 0.0]
    for case in range(200):
        m = int(rng.integers(1, 70))
        scale = 10.0 ** rng.integers(-3, 4)
        r = (rng.standard_normal(m) * scale).astype(np.float32)
        gamma = GAMMAS[case % len(GAMMAS)]
        R, d = nm.fold(r, gamma)
        assert R.dtype == np.float32 and d.dtype == np.float32
        g = float(np.float32(gamma))
        want = sum(g ** k * float(r[k]) for k in range(m))
        mag = sum(g ** k * abs(float(r[k])) for k in range(m))
        assert abs(float(R) - want) <= 2 * m * u * mag, (case, m, gamma)
        assert abs(float(d) - g ** m) <= m * u * g ** m, (case, m, gamma)
        if mag > 0:
            worst[0] = max(worst[0], abs(float(R) - want) / (2 * m * u * mag))
        if g > 0:
            worst[1] = max(worst[1], abs(float(d) - g ** m) / (m * u * g ** m))
    print(f"worst fraction of the bounds: return {worst[0]:.2f}, discount {worst[1]:.2f}")
    R, d = nm.fold(np.array([1.5], np.float32), 0.95)
    assert R.tobytes() == np.float32(1.5).tobytes() and d.tobytes() == np.float32(0.95).tobytes()


def _rollout(rng, T=5, B=3, N=2):
    done = (rng.random((T, B)) < 0.3).astype(np.uint8)
    return dict(obs_in=rng.standard_normal((B, N, 12)).astype(np.float32),
                obs=rng.standard_normal((T, B, N, 12)).astype(np.float32),
                actions=rng.integers(0, 12, (T, B, N)).astype(np.int32),
                reward=rng.standard_normal((T, B, N)).astype(np.float32),
                done=done, start_obs=rng.standard_normal((T, B, N, 12)).astype(np.float32))


@pytest.mark.parametrize("episodes", [False, True])
def test_n1_is_transitions_from_rollout(episodes):
    r = _rollout(np.random.default_rng(2))
    out = {k: torch.from_numpy(r[k]) for k in ("obs", "actions", "reward")}
    if episodes:
        assert r["done"][:-1].any()
        out.update(done=torch.from_numpy(r["done"]), start_obs=torch.from_numpy(r["start_obs"]))
    want = uavtrack.transitions_from_rollout(torch.from_numpy(r["obs_in"]), out)
    got, m = nm.transitions(r["obs_in"], r["obs"], r["actions"], r["reward"], 1, 0.95,
                            r["done"] if episodes else None, r["start_obs"] if episodes else None)
    assert (m == 1).all()
    for k in ("states", "actions", "rewards", "next_states"):
        assert got[k].tobytes() == want[k].contiguous().numpy().tobytes(), k
    assert (got["discounts"].view(np.int32) == np.float32(0.95).view(np.int32)).all()


def test_ring_image_window_and_wrap():
    r = _rollout(np.random.default_rng(3), T=7)
    tr, _ = nm.transitions(r["obs_in"], r["obs"], r["actions"], r["reward"], 3, 0.95, r["done"], r["start_obs"])
    n = len(tr["actions"])
    for cap, pos, count in ((n + 9, 0, 0), (n + 9, n + 6, n + 9), (17, 5, 17)):
        img = {"states": np.zeros((cap, 12), np.float32), "actions": np.zeros(cap, np.int32),
               "rewards": np.zeros(cap, np.float32), "next_states": np.zeros((cap, 12), np.float32),
               "discounts": np.full(cap, 7.0, np.float32), "priorities": np.full(cap, 0.5, np.float32)}
        img["priorities"][0] = 2.5
        p2, c2 = nm.ring_add(img, pos, count, tr)
        assert p2 == (pos + n) % cap and c2 == min(cap, count + n)
        k = min(n, cap)
        for j in range(k):                                             # the last k transitions, in order, ending before p2
            slot = (p2 - k + j) % cap
            assert img["rewards"][slot] == tr["rewards"][n - k + j] and img["discounts"][slot] == tr["discounts"][n - k + j]
            assert img["priorities"][slot] == (1.0 if count == 0 else 2.5)
        assert (img["discounts"] == 7.0).sum() == cap - k


ARGS = {
    "uavtrack_replay_add_rollout_nstep": "replay ring discounts steps envs n_uav obs_in obs actions reward done start_obs "
                                         "n_step gamma stream",
    "uavtrack_learner_update_discounted": "learner n states actions rewards next_states capacity indices weights discounts "
                                          "actor_loss critic_loss td_delta priorities stream",
    "uavtrack_learner_grad_discounted": "learner n states actions rewards next_states capacity indices weights discounts "
                                        "td_delta row stream",
}
CTYPE = {"uavtrack_replay *": C.c_void_p, "uavtrack_learner *": C.c_void_p,
         "const uavtrack_replay_ring *": C.POINTER(_lib.ReplayRing), "int32_t": C.c_int32, "int64_t": C.c_int64,
         "double": C.c_double, "const int64_t *": C.c_void_p, "const int32_t *": C.c_void_p, "const uint8_t *": C.c_void_p,
         "const float *": C.c_void_p, "float *": C.c_void_p, "void *": C.c_void_p}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_symbols_are_declared_exported_and_bound_with_the_headers_argument_lists(name):
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/uavtrack.h"
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", a).group(1) for a in decl]
    assert names == ARGS[name].split()
    types = [a[:-len(n)].strip() for a, n in zip(decl, names)]
    assert name in _lib.SIGNATURES, f"{name} is not bound in uavtrack/_lib.py"
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [CTYPE[t] for t in types]
    assert hasattr(_lib.load(), name), f"{name} is not exported by the built library"


def test_limits_and_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    assert int(re.search(r"#define UAVTRACK_REPLAY_MAX_NSTEP (\d+)", hdr).group(1)) == _lib.REPLAY_MAX_NSTEP == 64 \
        == nm.MAX_NSTEP
    assert re.search(r"#define UAVTRACK_ABI_VERSION\s+1\b", hdr) and _lib.ABI_VERSION == 1
    assert C.sizeof(_lib.ReplayRing) == 64 and C.sizeof(_lib.ReplayConfig) == 32
    assert _lib.LEARNER_ROW_TAIL == 8
