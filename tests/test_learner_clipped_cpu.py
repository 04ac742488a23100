"""The clipped surrogate without a GPU: the float64 mirror (tests/learner_mirror.py with clip=) against torch autograd, the
premises of the batches the GPU tests use, the host-side refusals of the Python layer, and the library calls the drawn
paths enqueue with and without clip_eps (tests/learner_call_trace.py's recorder)."""
import json

import numpy as np
import pytest
import torch

import learner_autograd as ag
import learner_call_trace as lt
import learner_clipped_mirror as cm
import learner_harness as lh
import learner_mirror as mirror

INF = float("inf")
GAMMA = cm.GAMMA


# ---- 1. the mirror is torch's gradient -----------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.2, INF])
@pytest.mark.parametrize("H,A,n", [(33, 12, 63), (128, 48, 65)])
def test_the_mirror_is_torch_autograd_in_float64(H, A, n, eps):
    gather = n == 63
    cb = cm.clip_batch(H, A, n, gather)
    rows = tuple(x[cb["idx"]] for x in cb["b"])
    mu = cb["log_mu"][cb["idx"]]
    w = lh.make_weights(np.random.RandomState(n), n)
    c = 0.01
    al, cl, td, g, ent, ratio = mirror.losses_and_grads(cb["blob"], H, A, *rows, GAMMA, "per_sample", weights=w,
                                                        entropy_coef=c, clip=(mu, eps))
    t = ag.update(cb["blob"], H, A, *rows, GAMMA, "per_sample", w, c, clip=(mu, eps))
    tal, tcl, tg = t.actor_loss, t.critic_loss, t.grad
    assert abs(al - tal) <= 1e-12 * abs(tal) and abs(cl - tcl) <= 1e-12 * abs(tcl)
    assert np.abs(g - tg).max() <= 1e-12 * np.abs(tg).max()
    # a row of the split form is the same gradient before its scale, and rows add
    halves = [mirror.shard_sums(cb["blob"], H, A, *(x[lo:hi] for x in rows), GAMMA, "per_sample", w[lo:hi], c, (mu[lo:hi], eps))
              for lo, hi in lh.cuts(n, 2)]
    cal, ccl, cg = mirror.combine(halves, H, A, "per_sample")
    assert abs(cal - tal) <= 1e-12 * abs(tal) and np.abs(cg - tg).max() <= 1e-12 * np.abs(tg).max()
    if eps == 0.2:
        assert not cm.gate(ratio, td, eps).all() and cm.gate(ratio, td, INF).all()


# ---- 2. the premises of the GPU tests' batches ---------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,gather", cm.SHAPES)
def test_every_gpu_case_decides_something_and_sits_off_its_boundaries(H, A, n, gather):
    cb = cm.clip_batch(H, A, n, gather)
    mu = cb["log_mu"]
    assert mu.dtype == np.float32 and mu.shape == (cb["cap"],) and (mu <= 0).all()
    counts, near, ratio = cm.premises(cb["blob"], H, A, cb["b"], cb["idx"], mu)
    print(counts)
    assert not near
    assert ratio.min() >= np.exp(-1.5) * (1 - 1e-6) and ratio.max() <= np.exp(1.5 + 8 * cm.NUDGE)
    for eps in cm.EPS:
        hi, lo, ok = counts[eps]
        assert hi + lo + ok == n
        if n >= 3:                                  # rows gated on each side and rows passing
            assert hi > 0 and lo > 0 and ok > 0
        else:                                       # one row cannot be of three kinds: it is gated, so the gate shows
            assert hi + lo == n


def test_a_case_that_decides_nothing_is_not_accepted():
    assert not cm.decides({0.2: (0, 3, 60)}, 63) and not cm.decides({0.2: (3, 3, 0)}, 6) and not cm.decides({0.2: (0, 0, 1)}, 1)
    assert cm.decides({0.1: (1, 1, 1), 0.2: (1, 2, 3)}, 6) and cm.decides({0.2: (0, 1, 0)}, 1)


def test_the_bounds_are_the_float32_ones_and_the_boundary_passes():
    lo, hi = cm.bounds(0.2)
    assert lo == float(np.float32(1) - np.float32(0.2)) and hi == float(np.float32(1) + np.float32(0.2)) and hi != 1.2
    assert cm.bounds(INF) == (-INF, INF) and cm.bounds(0.0) == (1.0, 1.0)
    assert cm.gate(np.array([hi, lo, 1.0, 1.0]), np.array([1.0, -1.0, 0.0, -0.0]), 0.2).all()
    assert not cm.gate(np.array([np.nextafter(hi, 2), np.nextafter(lo, 0)]), np.array([1.0, -1.0]), 0.2).any()
    assert cm.gate(np.ones(2), np.array([1.0, -1.0]), 0.0).all()


# ---- 3. the host-side refusals -------------------------------------------------------------------------------------------

def _fresh(which="ReplayRing.behaviour"):
    lt.REC.calls, lt.REC.known, lt.REC.fresh, lt.REC.dump = [], {}, [], False
    return lt.Learner(), lt.make_buffer(which)


def _batch(n=5):
    return {"states": torch.zeros(n, 12), "actions": torch.zeros(n, dtype=torch.int32), "rewards": torch.zeros(n),
            "next_states": torch.zeros(n, 12)}


def test_the_python_layer_refuses_before_any_library_call():
    L, ring = _fresh()
    plain = lt.make_buffer("ReplayRing.plain", "ring1")
    out = torch.zeros(8)
    for call in (lambda **kw: L.update_from(ring, 8, **kw), lambda **kw: L.grad_from(ring, 8, **kw),
                 lambda **kw: L.update_from_many([ring], 8, **{k: [v] if k == "ratio_out" else v for k, v in kw.items()})):
        lt.REC.calls = []
        with pytest.raises(ValueError, match="one correction for who acted, not two"):
            call(clip_eps=0.2, rho_bar=1.0)
        with pytest.raises(ValueError, match="ratio_out needs clip_eps"):
            call(ratio_out=out)
        for bad in (-0.1, float("nan"), -INF):
            with pytest.raises(ValueError, match="clip_eps"):
                call(clip_eps=bad)
        assert not [c for c in lt.REC.calls if c.startswith(("uavtrack_learner_update", "uavtrack_learner_grad"))]
    for buf in (plain, lt.make_buffer("DeviceReplayBuffer")):
        with pytest.raises(ValueError, match="with_behaviour"):
            L.update_from(buf, 8, clip_eps=0.2)
    R, ring = _fresh()
    R.loss = "reference"
    for call in (lambda: R.update_from(ring, 8, clip_eps=0.2), lambda: R.grad_from(ring, 8, clip_eps=0.2),
                 lambda: R.update_from_many([ring], 8, clip_eps=0.2), lambda: R.update(_batch(), log_mu=torch.zeros(5), clip_eps=0.2)):
        with pytest.raises(ValueError, match='loss="reference".*cannot share'):
            call()
    assert not [c for c in lt.REC.calls if c.startswith(("uavtrack_learner_update", "uavtrack_learner_grad"))]
    with pytest.raises(ValueError, match="update_from_many: ratio_out holds 2 entries for 1 buffers"):
        L.update_from_many([ring], 8, clip_eps=0.2, ratio_out=[out, out])


def test_update_takes_log_mu_with_exactly_one_of_rho_bar_and_clip_eps():
    L, _ = _fresh()
    mu = torch.full((5,), -1.0)
    with pytest.raises(ValueError, match="exactly one of rho_bar and clip_eps"):
        L.update(_batch(), log_mu=mu)
    with pytest.raises(ValueError, match="exactly one of rho_bar and clip_eps"):
        L.update(_batch(), clip_eps=0.2)
    with pytest.raises(ValueError, match="not two"):
        L.update(_batch(), log_mu=mu, rho_bar=1.0, clip_eps=0.2)
    with pytest.raises(ValueError, match="ratio_out needs clip_eps"):
        L.update(_batch(), log_mu=mu, rho_bar=1.0, ratio_out=torch.zeros(5))
    with pytest.raises(ValueError, match="ratio_out must be a contiguous float32 tensor of 5 elements"):
        L.update(_batch(), log_mu=mu, clip_eps=0.2, ratio_out=torch.zeros(4))
    assert lt.REC.calls == []


# ---- 4. the library calls ------------------------------------------------------------------------------------------------

def test_with_clip_eps_none_the_drawn_paths_enqueue_the_recorded_calls(monkeypatch):
    """Every case of learner_call_trace's matrix with clip_eps=None and ratio_out=None spelled out: the golden trace."""
    with open(lt.GOLDEN) as f:
        golden = json.load(f)
    monkeypatch.setattr(lt, "OPTIONS", {k: dict(v, clip_eps=None, ratio_out=None) for k, v in lt.OPTIONS.items()})
    for key in lt.case_keys():
        assert lt.run_case(key) == golden[key], key


def _update_trace(**kw):
    L, _ = _fresh()
    batch = _batch()
    for k, t in batch.items():
        lt.REC.known[k] = t
    for k, t in kw.items():
        if torch.is_tensor(t):
            lt.REC.known[k] = t
    L.update(batch, **kw)
    return lt.REC.calls


def test_update_without_clip_eps_enqueues_what_it_did():
    head = "uavtrack_learner_update{}(learner, 5, states+0, actions+0, rewards+0, next_states+0, 5, None, "
    tail = "fresh0, fresh1, fresh2, None, None)"
    for kw in ({}, dict(clip_eps=None, ratio_out=None, log_mu=None, rho_bar=None)):
        assert _update_trace(**kw) == [head.format("") + tail]
        assert _update_trace(weights=torch.ones(5), **kw) == [head.format("_weighted") + "weights+0, " + tail]
        assert _update_trace(discounts=torch.ones(5), **kw) == [head.format("_discounted") + "None, discounts+0, " + tail]
    got = _update_trace(log_mu=torch.zeros(5), rho_bar=1.0)
    assert [c.split("(")[0] for c in got] == ["uavtrack_learner_ratio_weights", "uavtrack_learner_update_weighted"]


def test_the_clipped_calls_carry_the_store_the_bound_and_the_ratio_buffer():
    head = "uavtrack_learner_update_clipped(learner, 5, states+0, actions+0, rewards+0, next_states+0, 5, None, "
    assert _update_trace(log_mu=torch.zeros(5), clip_eps=0.2) == [
        head + "None, None, log_mu+0, 0.2, None, fresh0, fresh1, fresh2, None, None)"]
    assert _update_trace(log_mu=torch.zeros(5), clip_eps=INF, ratio_out=torch.zeros(5), weights=torch.ones(5),
                         discounts=torch.ones(5)) == [
        head + "weights+0, discounts+0, log_mu+0, inf, ratio_out+0, fresh0, fresh1, fresh2, None, None)"]
    # a prioritised n-step behaviour ring: the draw, then ONE learner call with the ring's weights, discounts and log_mu
    L, ring = _fresh("PrioritizedReplayRing.nstep+behaviour")
    lt._register("ring0", ring)
    out = lt.REC.known["ratio_out0"] = torch.zeros(8)
    L.update_from(ring, 8, importance=True, clip_eps=0.1, ratio_out=out)
    assert len(lt.REC.calls) == 2 and lt.REC.calls[0].startswith("uavtrack_replay_sample")
    assert lt.REC.calls[1] == ("uavtrack_learner_update_clipped(learner, 8, ring0.store.states+0, ring0.store.actions+0, "
                               "ring0.store.rewards+0, ring0.store.next_states+0, 32, ring0._idx+0, ring0._w+0, "
                               "ring0.discounts+0, ring0.log_mu+0, 0.1, ratio_out0+0, fresh0, fresh1, fresh2, "
                               "ring0.priorities+0, None)")
    L, ring = _fresh("ReplayRing.behaviour")
    lt._register("ring0", ring)
    L.grad_from(ring, 8, clip_eps=0.1)
    assert lt.REC.calls[-1] == ("uavtrack_learner_grad_clipped(learner, 8, ring0.store.states+0, ring0.store.actions+0, "
                                "ring0.store.rewards+0, ring0.store.next_states+0, 32, ring0._idx+0, None, None, "
                                "ring0.log_mu+0, 0.1, None, fresh0, fresh1, None)")


def test_the_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import os
    import re
    from uavtrack import _lib
    hdr = open(os.path.join(lt.ROOT, "include", "uavtrack.h")).read()
    batch = "learner n states actions rewards next_states capacity indices weights discounts log_mu clip_eps ratio_out "
    for name, args in (("uavtrack_learner_update_clipped", batch + "actor_loss critic_loss td_delta priorities stream"),
                       ("uavtrack_learner_grad_clipped", batch + "td_delta row stream")):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        decl = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert [re.search(r"(\w+)$", a).group(1) for a in decl] == args.split()
        res, types = _lib.SIGNATURES[name]
        assert res is C.c_int and len(types) == len(decl)
        assert [t is C.c_double for t in types] == [a.startswith("double ") for a in decl]
        assert [t is C.c_int64 for t in types] == [a.startswith("int64_t ") for a in decl]
        assert hasattr(_lib.load(), name), f"{name} is not exported by the built library"
