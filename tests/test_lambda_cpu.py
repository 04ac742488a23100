"""TD(lambda) targets without a GPU: the recursion of tests/lambda_mirror.py against the textbook lambda-return in float64
within the fold's bound, lambda = 0 as the n-step mirror at n = 1 byte for byte (a reward of -0.0 included), lambda = 1
as the discounted Monte-Carlo sum plus the bootstrap at the cut, the two new symbols declared in include/uavtrack.h,
exported by the library and bound in uavtrack/_lib.py with the header's argument lists, and the Python surface
(signatures, the ValueErrors, the constructors' parameter lists left alone)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import lambda_mirror as lm
import nstep_mirror as nm
import uavtrack
from uavtrack import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (0.0, 0.5, 0.95, 1.0)
GAMMAS = (0.0, 0.95, 1.0)


def _chain_case(rng, T, p_done):
    r = (rng.standard_normal(T) * 3).astype(np.float32)
    V = (rng.standard_normal(T) * 5).astype(np.float32)
    done = None if p_done is None else (rng.random(T) < p_done).astype(np.uint8)
    return r, V, done


@pytest.mark.parametrize("T", [1, 2, 7, 200])
def test_the_recursion_is_the_textbook_lambda_return_within_the_folds_bound(T):
    """R_t + d_t V_t against (1 - l) sum_{n<m} l^(n-1) G^(n) + l^(m-1) G^(m) within
    4 * 2^-24 * L * (max|r| + max|V| + max|G|), L the length of t's segment."""
    rng = np.random.default_rng(T)
    worst = 0.0
    for lam in LAMBDAS:
        for gamma in GAMMAS:
            for p_done in (None, 0.0, 0.1, 0.5, 1.0):
                r, V, done = _chain_case(rng, T, p_done)
                R, d = lm.chain(r, V, done, lam, gamma)
                assert R.dtype == np.float32 and d.dtype == np.float32
                G = R.astype(np.float64) + d.astype(np.float64) * V.astype(np.float64)
                y = lm.textbook(r, V, done, lam, gamma)
                L = lm.segment_lengths(T, done)
                bound = lm.fold_bound(r, V, G, L)
                assert (np.abs(G - y) <= bound).all(), (lam, gamma, p_done, np.abs(G - y).max())
                worst = max(worst, float((np.abs(G - y) / bound).max()))
                g, gl, c = lm.constants(lam, gamma)
                assert ((d == g) | (d == c)).all() and (d >= 0).all() and (d <= 1).all()
                cut = np.array([bool(t == T - 1 or (done is not None and done[t] != 0) or gl == 0) for t in range(T)])
                assert (d[cut] == g).all() and (d[~cut] == c).all() and R[cut].tobytes() == r[cut].tobytes()
    print(f"T = {T}: worst fraction of the fold's bound {worst:.3f}")


def _rollout(rng, T=5, B=3, N=2):
    done = (rng.random((T, B)) < 0.3).astype(np.uint8)
    reward = rng.standard_normal((T, B, N)).astype(np.float32)
    reward[1, 0, 0] = -0.0
    reward[T - 1, 1, 1] = -0.0
    return dict(obs_in=rng.standard_normal((B, N, 12)).astype(np.float32),
                obs=rng.standard_normal((T, B, N, 12)).astype(np.float32),
                actions=rng.integers(0, 12, (T, B, N)).astype(np.int32), reward=reward, done=done,
                start_obs=rng.standard_normal((T, B, N, 12)).astype(np.float32),
                values=rng.standard_normal((T, B, N)).astype(np.float32))


@pytest.mark.parametrize("lam,gamma", [(0.0, 0.95), (0.0, 1.0), (0.7, 0.0), (0.0, 0.0)])
@pytest.mark.parametrize("episodes", [False, True])
def test_lambda_0_or_gamma_0_is_the_one_step_mirror_byte_for_byte(episodes, lam, gamma):
    r = _rollout(np.random.default_rng(2))
    done, so = (r["done"], r["start_obs"]) if episodes else (None, None)
    got = lm.transitions(r["obs_in"], r["obs"], r["actions"], r["reward"], r["values"], lam, gamma, done, so)
    want, m = nm.transitions(r["obs_in"], r["obs"], r["actions"], r["reward"], 1, gamma, done, so)
    assert (m == 1).all() and set(got) == set(want)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert np.signbit(got["rewards"].reshape(r["reward"].shape)[1, 0, 0])          # -0.0 stayed -0.0


def test_lambda_1_without_done_is_the_discounted_sum_plus_the_bootstrap_at_the_cut():
    rng = np.random.default_rng(3)
    for T in (1, 2, 7, 50):
        for gamma in (0.95, 1.0, 0.5):
            r, V, _ = _chain_case(rng, T, None)
            R, d = lm.chain(r, V, None, 1.0, gamma)
            g = float(np.float32(gamma))
            assert (d[:-1] == 0).all() and d[-1] == np.float32(gamma)
            G = R.astype(np.float64) + d.astype(np.float64) * V.astype(np.float64)
            for t in range(T):
                want = sum(g ** k * float(r[t + k]) for k in range(T - t)) + g ** (T - t) * float(V[T - 1])
                assert abs(G[t] - want) <= lm.fold_bound(r, V, G, T - t), (T, gamma, t)


def test_the_critic_forward_and_its_magnitude():
    H, A = 7, 5
    rng = np.random.default_rng(4)
    blob = rng.standard_normal(27 * H + A * H + A + 1).astype(np.float32)
    x = rng.standard_normal((9, 12)).astype(np.float32)
    W1, b1, W2, b2 = lm.critic_of(blob, H, A)
    assert W1.shape == (H, 12) and b2 == blob[-1] and W2[-1] == blob[-2]
    v = lm.critic_forward(blob, H, A, x)
    net = uavtrack.ValueMLP(12, H).double()
    with torch.no_grad():
        net.fc1.weight.copy_(torch.from_numpy(W1.astype(np.float64))); net.fc1.bias.copy_(torch.from_numpy(b1.astype(np.float64)))
        net.fc2.weight.copy_(torch.from_numpy(W2.astype(np.float64)[None])); net.fc2.bias.fill_(float(b2))
        want = net(torch.from_numpy(x.astype(np.float64))).numpy()
    np.testing.assert_allclose(v, want, rtol=1e-13, atol=1e-13)
    assert (lm.critic_magnitude(blob, H, A, x) >= np.abs(v)).all()


ARGS = {
    "uavtrack_learner_values": "learner n rows values stream",
    "uavtrack_replay_add_rollout_lambda": "replay ring discounts steps envs n_uav obs_in obs actions reward done start_obs "
                                          "values lambda gamma stream",
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
    assert re.search(r"#define UAVTRACK_ABI_VERSION\s+1\b", hdr) and _lib.ABI_VERSION == 1
    assert C.sizeof(_lib.ReplayRing) == 64                                # values travel beside the ring struct


def test_python_surface():
    R, P, L = uavtrack.ReplayRing, uavtrack.PrioritizedReplayRing, uavtrack.DeviceActorCritic
    assert list(inspect.signature(L.values).parameters) == ["self", "states", "out"]
    assert inspect.signature(L.values).parameters["out"].default is None
    assert list(inspect.signature(R.with_lambda).parameters) == ["self", "lam", "gamma"]
    assert P.with_lambda is R.with_lambda and P.add_rollout is R.add_rollout
    ps = inspect.signature(R.add_rollout).parameters
    assert list(ps) == ["self", "obs_in", "out", "critic", "values"]
    assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None for k in ("critic", "values"))
    # with_lambda left the constructors' parameter lists alone
    assert list(inspect.signature(R.__init__).parameters)[1:] == ["capacity", "device", "seed", "max_batch", "obs_dim"]
    assert list(inspect.signature(P.__init__).parameters)[1:] == ["capacity", "device", "alpha", "seed", "max_batch",
                                                                  "obs_dim"]
    assert list(inspect.signature(R.with_nstep).parameters) == ["self", "n_step", "gamma"]
    assert R.lam is None and R.n_step == 1 and R.gamma is None and R.discounts is None


class _Bare(uavtrack.ReplayRing):
    """The host-side state of a ring without its device handle: what with_lambda / with_nstep touch."""

    def __init__(self, capacity=8):
        self.capacity, self.device = capacity, torch.device("cpu")


def test_with_lambda_sets_the_ring_up_and_excludes_n_step():
    ring = _Bare()
    assert ring.with_lambda(0.9, 0.95) is ring
    assert ring.lam == 0.9 and ring.gamma == 0.95 and ring.n_step == 1
    assert ring.discounts.dtype == torch.float32 and ring.discounts.shape == (8,)
    assert (ring.discounts.numpy().view(np.int32) == np.float32(0.95).view(np.int32)).all()
    with pytest.raises(ValueError, match="n-step returns or"):
        ring.with_nstep(3, 0.95)
    assert ring.n_step == 1 and ring.lam == 0.9
    for lam, gamma, word in ((-0.1, 0.9, "lam"), (1.5, 0.9, "lam"), (float("nan"), 0.9, "lam"), (0.5, 1.5, "gamma"),
                             (0.5, float("nan"), "gamma")):
        fresh = _Bare()
        with pytest.raises(ValueError, match=word):
            fresh.with_lambda(lam, gamma)
        assert fresh.lam is None and fresh.discounts is None
    nstep = _Bare().with_nstep(3, 0.95)
    with pytest.raises(ValueError, match="n-step returns or"):
        nstep.with_lambda(0.9, 0.95)
    assert nstep.lam is None and nstep.n_step == 3
    assert _Bare().with_nstep(1, 0.95).with_lambda(0.5, 0.95).lam == 0.5   # n_step = 1 is no n-step ring


def test_add_rollout_refuses_what_does_not_fit_the_ring():
    rng = np.random.default_rng(5)
    r = {k: torch.from_numpy(v) for k, v in _rollout(rng).items()}
    out = {k: r[k] for k in ("obs", "actions", "reward")}
    v = r["values"]
    plain = _Bare()
    for kw in (dict(values=v), dict(critic=object())):                     # nothing is silently ignored
        with pytest.raises(ValueError, match="lambda ring"):
            plain.add_rollout(r["obs_in"], out, **kw)
    nstep = _Bare().with_nstep(3, 0.95)
    with pytest.raises(ValueError, match="lambda ring"):
        nstep.add_rollout(r["obs_in"], out, values=v)
    ring = _Bare().with_lambda(0.9, 0.95)
    ring.store = {}
    ring._ring = lambda: None
    for kw in (dict(), dict(values=v, critic=object())):
        with pytest.raises(ValueError, match="exactly one"):
            ring.add_rollout(r["obs_in"], out, **kw)
    for bad in (v.double(), v.reshape(-1)[:-1], v.transpose(0, 1)):
        with pytest.raises(ValueError, match="values must be"):
            ring.add_rollout(r["obs_in"], out, values=bad)
