"""TD(lambda) targets on the MI355X: the critic-forward kernel (uavtrack_learner_values) bitwise against the V(s) an update
forms and against the float64 forward; the lambda ring add (uavtrack_replay_add_rollout_lambda) against the numpy mirror
(tests/lambda_mirror.py), bitwise over all five stores and the priorities; lambda = 0 as with_nstep(1, gamma); values +
add + update end to end; graph capture; host-side errors; the example.  The rollout, the done patterns and the ring
cases are those of tests/test_hip_nstep.py (tests/ring_rollout_harness.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lambda_mirror as lm
import learner_harness as lh
import learner_mirror as mirror
import nstep_mirror as nm
import ring_rollout_harness as rr
from ring_rollout_harness import B, N, NTR, T

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA
LAMBDAS = (0.0, 0.5, 0.95, 1.0)
GAMMAS = (0.0, 0.95, 1.0)
U = 2.0 ** -24


def _uav():
    import uavtrack
    return uavtrack


# ---- 1. values: the update's own V(s), to the bit ------------------------------------------------------------------------

_rows = {}


def _value_rows(n):
    """n rows with entries of every magnitude up to +-1e3 (shared by the hidden widths)."""
    if n not in _rows:
        rng = np.random.RandomState(n)
        x = rng.uniform(-1, 1, (n, 12)) * 10.0 ** rng.randint(-3, 4, (n, 12))
        x.flat[rng.randint(0, x.size)] = 1e3
        x.flat[rng.randint(0, x.size)] = -1e3
        x = x.astype(np.float32)
        _rows[n] = (x, lh.dev(x), lh.dev(rng.randint(0, 5, n).astype(np.int32)))
    return _rows[n]


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
@pytest.mark.parametrize("H", [1, 7, 128, 256])
def test_values_are_the_updates_own_v_bitwise_and_the_fp64_forward_within_the_chains_bound(H, n):
    A = 5
    blob = lh.init_blob(H, A, 100 + H)
    assert lm.critic_of(blob, H, A)[3] != 0                            # b2: V is never an exact zero by accident
    x, xd, act = _value_rows(n)
    L = lh.learner(H, A, "reference", blob, max_batch=n)
    before = lh.state(L)
    v = L.values(xd)
    assert v.shape == (n,) and v.dtype == torch.float32
    # rewards = 0 and a discount store of 0: td_delta = (0 + 0 * V(s')) - V(s) = -V(s) exactly
    store = {"states": xd, "actions": act, "rewards": torch.zeros(n, device=DEV), "next_states": xd}
    _, td = L._grad(n, store, n, None, None, None, None, torch.zeros(n, device=DEV))
    L.check()
    got = v.cpu().numpy()
    assert got.tobytes() == (-td.cpu().numpy()).tobytes()
    lh.same(lh.state(L), before)                                      # values changed nothing
    # out= is written in place; any leading shape
    out = torch.full((n,), 7.0, device=DEV)
    assert L.values(xd.reshape(n, 1, 12), out=out) is out and torch.equal(out, v)
    assert L.values(xd.reshape(1, n, 12)).shape == (1, n)
    # the fp64 forward: H + 14 fused operations per chain, each within 2^-24 of m(x), plus one ulp of the result
    want = lm.critic_forward(blob, H, A, x)
    err = np.abs(got.astype(np.float64) - want)
    bound = (H + 14) * U * lm.critic_magnitude(blob, H, A, x) + np.spacing(np.abs(got)).astype(np.float64)
    print(f"H = {H}, n = {n}: worst fraction of the bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound).max()


def test_values_read_the_parameters_of_the_moment_and_span_more_than_one_grid_pass():
    """n beyond 2048 workgroups x 512 rows (the grid-stride loop's second pass) and beyond max_batch; after
    load_state_dict the same call gives the new critic's values."""
    H, A, n = 16, 5, 2048 * 512 + 700
    blob = lh.init_blob(H, A, 7)
    L = lh.learner(H, A, "reference", blob, max_batch=64)
    rng = np.random.RandomState(3)
    x = rng.uniform(-2, 2, (n, 12)).astype(np.float32)
    xd = lh.dev(x)
    got = L.values(xd).cpu().numpy()
    want = lm.critic_forward(blob, H, A, x)
    bound = (H + 14) * U * lm.critic_magnitude(blob, H, A, x) + np.spacing(np.abs(got)).astype(np.float64)
    assert (np.abs(got - want) <= bound).all()
    tail = L.values(xd[-700:].contiguous()).cpu().numpy()              # the same rows in the first pass: the same bits
    assert tail.tobytes() == got[-700:].tobytes()
    blob2 = lh.init_blob(H, A, 8)
    L._set_params(blob2)
    got2 = L.values(xd[:1000].contiguous()).cpu().numpy()
    want2 = lm.critic_forward(blob2, H, A, x[:1000])
    bound2 = (H + 14) * U * lm.critic_magnitude(blob2, H, A, x[:1000]) + np.spacing(np.abs(got2)).astype(np.float64)
    assert (np.abs(got2 - want2) <= bound2).all()
    assert not np.array_equal(got2, got[:1000])


# ---- 2. the add against the mirror ---------------------------------------------------------------------------------------

_vals = {}


def _values(shape=(T, B, N), seed=11):
    """A random values array given by the test: the fold is pinned independently of the critic."""
    key = (shape, seed)
    if key not in _vals:
        v = (np.random.default_rng(seed).standard_normal(shape) * 4).astype(np.float32)
        _vals[key] = (v, lh.dev(v))
    return _vals[key]


def _new_ring(kind, cap, max_batch=64):
    u = _uav()
    return (u.PrioritizedReplayRing if kind == "prioritised" else u.ReplayRing)(cap, DEV, seed=1, max_batch=max_batch)


def _check_add(ring, pos, count, host, dev_obs_in, out, values, lam, gamma, done):
    """One prefilled lambda add against the mirror's ring image, bitwise (the slots outside the window keep their
    sentinels: the image starts from them)."""
    ring.with_lambda(lam, gamma)
    assert ring.n_step == 1 and ring.lam == lam and ring.gamma == gamma
    rr.prefill(ring, pos, count)
    img = rr.image(ring)
    ring.add_rollout(dev_obs_in, out, values=values[1])
    tr = lm.transitions(host["obs_in"], host["obs"], host["actions"], host["reward"], values[0], lam, gamma, done,
                        None if done is None else host["start_obs"])
    p2, c2 = nm.ring_add(img, pos, count, tr)
    assert (ring.pos, ring.count) == (p2, c2)
    rr.same_image(rr.image(ring), img)
    d = img["discounts"]
    assert ((d >= 0) & (d <= 1) | (d == np.float32(7.0))).all()        # status bit 3 never fires on a written slot
    return tr


@pytest.mark.parametrize("ringcase", sorted(rr.RINGS))
@pytest.mark.parametrize("done_kind", rr.DONES)
@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_add_against_the_mirror_bitwise(kind, done_kind, ringcase):
    r = rr.rollout()
    done = rr.done(done_kind)
    cap, pos, count = rr.RINGS[ringcase]
    ring = _new_ring(kind, cap)
    folded = 0
    for lam in LAMBDAS:
        for gamma in GAMMAS:
            tr = _check_add(ring, pos, count, r, r["dev"]["obs_in"], rr.out(done), _values(), lam, gamma, done)
            folded += int((tr["rewards"] != r["reward"].reshape(-1)).sum())
    assert folded > 0                                                  # some reward carried a tail


@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
@pytest.mark.parametrize("steps", [1, 2])
def test_add_of_one_and_two_steps(steps, kind):
    r = rr.rollout()
    host = {k: (r[k] if k == "obs_in" else r[k][:steps]) for k in ("obs_in", "obs", "actions", "reward", "start_obs")}
    dev = {k: lh.dev(v) for k, v in host.items()}
    v = _values()
    values = (v[0][:steps], lh.dev(v[0][:steps]))
    for done in (None, np.zeros((steps, B), np.uint8), np.ones((steps, B), np.uint8)):
        out = {k: dev[k] for k in ("obs", "actions", "reward")}
        if done is not None:
            out.update(done=lh.dev(done), start_obs=dev["start_obs"])
        ring = _new_ring(kind, 50)
        for lam in LAMBDAS:
            for gamma in GAMMAS:
                _check_add(ring, 45, 30, host, dev["obs_in"], out, values, lam, gamma, done)


_shaped = {}


def _shaped_rollout(Tw, Bw, Nw):
    if (Tw, Bw, Nw) not in _shaped:
        rng = np.random.default_rng(Tw * 1000 + Bw)
        reward = (rng.standard_normal((Tw, Bw, Nw)) * 3).astype(np.float32)
        reward[3, Bw // 2, Nw - 1] = -0.0
        r = dict(obs_in=rng.standard_normal((Bw, Nw, 12)).astype(np.float32),
                 obs=rng.standard_normal((Tw, Bw, Nw, 12)).astype(np.float32),
                 actions=rng.integers(0, 12, (Tw, Bw, Nw)).astype(np.int32), reward=reward,
                 start_obs=rng.standard_normal((Tw, Bw, Nw, 12)).astype(np.float32),
                 done=(rng.random((Tw, Bw)) < 0.2).astype(np.uint8))
        r["dev"] = {k: lh.dev(v) for k, v in r.items()}
        _shaped[Tw, Bw, Nw] = r
    return _shaped[Tw, Bw, Nw]


# T = 9, B x N = 37 x 7: 259 chains -- more than one workgroup of the scan, its last wavefront partly filled; one step
# ahead of one group of eight.  T = 27, 2 x 3: three steps ahead of three groups, so both register groups of the scan
# fold twice and the chain's front is reached from either.  T = 16: groups alone.  Each into a roomy ring and into one
# smaller than the rollout that wraps (the scan's windowed form), with and without done.
@pytest.mark.parametrize("ringcase", ["roomy", "wrap-and-window"])
@pytest.mark.parametrize("with_done", [False, True])
@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
@pytest.mark.parametrize("shape", [(9, 37, 7), (27, 2, 3), (16, 2, 3)])
def test_add_of_many_chains_and_of_long_chains(shape, kind, with_done, ringcase):
    r = _shaped_rollout(*shape)
    n = r["reward"].size
    cap, pos, count = (n + 700, 100, 100) if ringcase == "roomy" else (n // 2 - 3, n // 2 - 10, n // 2 - 3)
    done = r["done"] if with_done else None
    out = {k: r["dev"][k] for k in ("obs", "actions", "reward")}
    if with_done:
        out.update(done=r["dev"]["done"], start_obs=r["dev"]["start_obs"])
    ring = _new_ring(kind, cap)
    values = _values(r["reward"].shape, 22)
    for lam in LAMBDAS:
        for gamma in GAMMAS:
            _check_add(ring, pos, count, r, r["dev"]["obs_in"], out, values, lam, gamma, done)


# ---- 3. lambda = 0 is with_nstep(1, gamma) -------------------------------------------------------------------------------

@pytest.mark.parametrize("ringcase", sorted(rr.RINGS))
@pytest.mark.parametrize("done_kind", ["null", "mid", "every"])
@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_lambda_0_is_with_nstep_1_byte_for_byte(kind, done_kind, ringcase):
    r = rr.rollout()
    reward = r["reward"].copy()
    reward[2, 1, 0] = -0.0                                             # a cut copies the reward: -0.0 stays -0.0
    done = rr.done(done_kind)
    out = dict(rr.out(done), reward=lh.dev(reward))
    cap, pos, count = rr.RINGS[ringcase]
    for lam, gamma in ((0.0, GAMMA), (0.0, 1.0), (0.6, 0.0)):
        new = _new_ring(kind, cap).with_lambda(lam, gamma)
        old = _new_ring(kind, cap).with_nstep(1, gamma)
        rr.prefill(new, pos, count); rr.prefill(old, pos, count)
        new.add_rollout(r["dev"]["obs_in"], out, values=_values()[1])
        old.add_rollout(r["dev"]["obs_in"], out)
        a, b = rr.image(new), rr.image(old)
        rr.same_image(a, b)
        assert (new.pos, new.count) == (old.pos, old.count)
        f = (2 * B + 1) * N                                             # the -0.0 reward's transition, where it was written
        if f >= NTR - min(NTR, cap):
            got = a["rewards"][(pos + f) % cap]
            assert got == 0 and np.signbit(got)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["uniform", "prioritised"])
def test_values_add_and_update_end_to_end(kind):
    H, A, k, lam = 64, 12, 32, 0.9
    r = rr.rollout()
    done = rr.done("mid")
    out = rr.out(done)
    blob = lh.init_blob(H, A, 42)
    L = lh.learner(H, A, "reference", blob, max_batch=k)
    ring = _new_ring(kind, 100, max_batch=k).with_lambda(lam, GAMMA)
    ring.add_rollout(r["dev"]["obs_in"], out, critic=L)
    buf = ring._values
    assert buf is not None and buf.numel() == NTR
    v = L.values(out["obs"])
    assert torch.equal(v.reshape(-1), buf[:NTR])
    tr = lm.transitions(r["obs_in"], r["obs"], r["actions"], r["reward"], v.cpu().numpy(), lam, GAMMA, done, r["start_obs"])
    img = rr.image(ring)
    for key in ("states", "actions", "rewards", "next_states", "discounts"):
        assert img[key][:NTR].tobytes() == tr[key].tobytes(), key
    assert (ring.pos, ring.count) == (NTR, NTR)
    # the update: losses and td_delta against the fp64 mirror on the gathered rows
    al, cl, td = L.update_from(ring, k)
    L.check(); ring.check()
    idx = ring._idx[:k].cpu().numpy()
    ral, rcl, rtd = mirror.losses_and_grads(blob, H, A, *(tr[key][idx] for key in lh.STORES), tr["discounts"][idx], "reference")[:3]
    lh.assert_losses_and_td(al.cpu().numpy(), cl.cpu().numpy(), td.cpu().numpy(), ral, rcl, rtd)
    # a second add of the same shape allocates nothing
    ring.add_rollout(r["dev"]["obs_in"], out, critic=L)
    assert ring._values is buf
    # a ring folded with another gamma is refused by the learner
    other = _new_ring(kind, 100, max_batch=k).with_lambda(lam, 0.9)
    other.add_rollout(r["dev"]["obs_in"], out, critic=L)
    with pytest.raises(ValueError, match=r"0\.9\b.*0\.95\b"):
        L.update_from(other, k)
    # critic= a torch module with the same weights: rewards within the fold's bound of the device path
    L2 = lh.learner(H, A, "reference", blob, max_batch=k)
    net = _uav().ValueMLP(12, H).to(DEV)
    net.load_state_dict(L2.critic_state_dict())
    dev_ring = _new_ring(kind, 100, max_batch=k).with_lambda(lam, GAMMA)
    mod_ring = _new_ring(kind, 100, max_batch=k).with_lambda(lam, GAMMA)
    dev_ring.add_rollout(r["dev"]["obs_in"], out, critic=L2)
    mod_ring.add_rollout(r["dev"]["obs_in"], out, critic=net)
    a, b = rr.image(dev_ring), rr.image(mod_ring)
    for key in ("states", "actions", "next_states", "discounts", "priorities"):
        assert (a[key] is None and b[key] is None) or a[key][:NTR].tobytes() == b[key][:NTR].tobytes(), key
    V = L2.values(out["obs"]).cpu().numpy().astype(np.float64).reshape(T, B, N)
    Ra = a["rewards"][:NTR].astype(np.float64).reshape(T, B, N)
    G = Ra + a["discounts"][:NTR].astype(np.float64).reshape(T, B, N) * V
    seg = np.stack([lm.segment_lengths(T, done[:, e]) for e in range(B)], axis=1)[:, :, None]
    bound = 4 * U * seg * (np.abs(r["reward"]).max() + np.abs(V).max() + np.abs(G).max())
    err = np.abs(Ra - b["rewards"][:NTR].astype(np.float64).reshape(T, B, N))
    print(f"module against device path: worst fraction of the fold's bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert net.fc1.weight.grad is None                                  # called under no_grad


# ---- 5. graph ------------------------------------------------------------------------------------------------------------------

def test_values_add_and_update_captured_and_replayed_equal_eager():
    """values + lambda add + update_from on one stream (a linear capture: every launch follows the one before it, no
    branches), captured once and replayed twice == the same three calls issued eagerly twice, bitwise.  The second
    iteration's values come from the critic the first one updated: parameters are read when the launch executes."""
    H, A, k = 64, 12, 32
    r = rr.rollout()
    out = rr.out(rr.done("mid"))
    blob = lh.init_blob(H, A, 42)

    def fresh():
        return lh.learner(H, A, "reference", blob, max_batch=k), \
            _new_ring("prioritised", 100, max_batch=k).with_lambda(0.9, GAMMA)

    eager, re_ = fresh()
    graphed, rg = fresh()

    def iteration(L, ring):
        ring.pos, ring.count = 0, 0                                     # every iteration enqueues the same add
        ring.add_rollout(r["dev"]["obs_in"], out, critic=L)
        return L.update_from(ring, k, importance=True, beta=0.4)

    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = iteration(graphed, rg)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(graphed)["step"], np.zeros(8))      # capture ran nothing
    rewards = []
    for c in range(2):
        e_out = iteration(eager, re_)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y) and torch.isfinite(x).all(), c
        assert np.array_equal(graphed._get_params(), eager._get_params()), c
        a, b = rr.image(rg), rr.image(re_)
        for key in a:                                                   # the written slots: the rest was never initialised
            assert a[key][:NTR].tobytes() == b[key][:NTR].tobytes(), key
        rewards.append(a["rewards"][:NTR].copy())
    assert not np.array_equal(rewards[0], rewards[1])                   # the replay evaluated the updated critic
    lh.same(lh.state(graphed), lh.state(eager))
    assert np.array_equal(lh.state(graphed)["step"], np.full(8, 2))
    for x in (graphed, eager, re_, rg):
        x.check()


# ---- 6. host-side errors -----------------------------------------------------------------------------------------------------

def test_host_side_errors_of_the_lambda_add_enqueue_nothing():
    from uavtrack import _lib
    lib = _lib.load()
    r = rr.rollout()["dev"]
    done = lh.dev(rr.done("mid"))
    ring = _new_ring("prioritised", 100).with_lambda(0.9, GAMMA)
    rr.prefill(ring, 10, 10)
    torch.cuda.synchronize()
    img = rr.image(ring)
    p = _lib.ptr
    off = lambda t: C.c_void_p(t.data_ptr() + 4)                       # not 16-byte aligned
    vals = _values()[1]

    def call(ring_struct=None, discounts=p(ring.discounts), obs_in=p(r["obs_in"]), obs=p(r["obs"]), act=p(r["actions"]),
             rew=p(r["reward"]), dn=p(done), so=p(r["start_obs"]), values=p(vals), lam=0.9, gamma=GAMMA, steps=T, envs=B,
             n_uav=N):
        rs = ring._ring() if ring_struct is None else ring_struct
        return lib.uavtrack_replay_add_rollout_lambda(ring._h, C.byref(rs), discounts, steps, envs, n_uav, obs_in, obs, act,
                                                      rew, dn, so, values, lam, gamma, ring._stream())

    def ring_with(**kw):
        rs = ring._ring()
        for key, v in kw.items():
            setattr(rs, key, v)
        return rs

    bad_calls = {
        "values": dict(values=None), "discounts": dict(discounts=None), "obs_in, obs": dict(obs=None),
        "reward": dict(rew=None), "actions": dict(act=None),
        "lambda": dict(lam=float("nan")), "lambda = -0.1": dict(lam=-0.1), "lambda = 1.5": dict(lam=1.5),
        "lambda = inf": dict(lam=float("inf")),
        "gamma": dict(gamma=float("nan")), "gamma = 1.5": dict(gamma=1.5),
        "both": dict(dn=None), "both be": dict(so=None),
        "pos": dict(ring_struct=ring_with(pos=100)), "capacity": dict(ring_struct=ring_with(capacity=101)),
        "ring's": dict(ring_struct=ring_with(rewards=None)),
        "aligned": dict(obs=off(r["obs"])), "16-byte": dict(so=off(r["start_obs"])),
        "16-byte aligned": dict(obs_in=off(r["obs_in"])),
        "steps": dict(steps=0),
    }
    for word, kw in bad_calls.items():
        assert call(**kw) != 0, word
        msg = lib.uavtrack_last_error().decode()
        assert msg.startswith("uavtrack_replay_add_rollout_lambda: ") and word.split(" =")[0] in msg, (word, msg)
    torch.cuda.synchronize()
    rr.same_image(rr.image(ring), img)
    assert call() == 0                                                  # and the good call goes through
    torch.cuda.synchronize()
    assert rr.image(ring)["rewards"].tobytes() != img["rewards"].tobytes()


def test_host_side_errors_of_values_enqueue_nothing():
    from uavtrack import _lib
    H, A, n = 64, 5, 63
    L = lh.learner(H, A, "reference", lh.init_blob(H, A, 1), max_batch=n)
    x, xd, _ = _value_rows(n)
    out = torch.full((n,), 7.0, device=DEV)
    before = lh.state(L)
    p = _lib.ptr

    def call(h=L._h, n_=n, rows=p(xd), values=p(out)):
        return L._lib.uavtrack_learner_values(h, n_, rows, values, L._stream())

    for word, kw in {"null handle": dict(h=None), "rows and values": dict(rows=None), "values must": dict(values=None),
                     "n = 0": dict(n_=0), "n = -1": dict(n_=-1),
                     "16-byte aligned": dict(rows=C.c_void_p(xd.data_ptr() + 4), n_=n - 1)}.items():
        assert call(**kw) != 0, word
        msg = L._lib.uavtrack_last_error().decode()
        assert msg.startswith("uavtrack_learner_values: ") and word.split(" =")[0] in msg, (word, msg)
    L.check()
    lh.same(lh.state(L), before)
    assert (out == 7.0).all()
    assert call() == 0
    L.check()
    assert torch.equal(out, L.values(xd))
    # the Python surface's own checks
    for bad in (xd.double(), xd[:, :11], xd.t(), xd.cpu()):
        with pytest.raises(ValueError, match="states must be"):
            L.values(bad)
    with pytest.raises(ValueError, match="out must be"):
        L.values(xd, out=torch.empty(n + 1, device=DEV))


# ---- 7. the example ----------------------------------------------------------------------------------------------------------

def test_example_trains_on_lambda_returns(capsys):
    """examples/train_maac.py --td-lambda 0.9: the device learner over two shards and the torch learner (its critic module
    passed to the add) train; --n-step > 1 and the PyTorch buffer of --replay uniform are refused with a message."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_maac
    common = ["--envs", "64", "--steps", "20", "--iters", "2", "--batch", "4096", "--updates", "2", "--td-lambda", "0.9"]
    for extra in (["--replay", "prioritized", "--learner", "device", "--shards", "2"],
                  ["--replay", "uniform-device", "--learner", "torch"]):
        hist = train_maac.main(common + extra)
        assert len(hist) == 2 and np.isfinite(hist).all(), extra
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == 2 and all(np.isfinite(float(ln.split("critic loss")[1].split()[0])) for ln in lines), extra
    for extra, words in ((["--replay", "uniform"], ("--replay prioritized", "uniform-device")),
                         (["--replay", "prioritized", "--n-step", "3"], ("--n-step", "exclude"))):
        with pytest.raises(SystemExit):
            train_maac.main(common + extra)
        err = capsys.readouterr().err
        assert all(w in err for w in words), err
