"""Fixed GAE advantages without a GPU: the numpy mirror of the GAE add (tests/replay_gae_mirror.py) against an independent
float64 GAE, the host-side refusals of the ring and the learner, the bindings, and the library calls a learner enqueues
with and without a GAE ring (the recorder of tests/learner_call_trace.py).  The stored kernels' rows of the variant table
are pinned with the others, in tests/test_learner_variants_cpu.py."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import lambda_mirror as lm
import learner_call_trace as lct
import replay_gae_mirror as gm
import uavtrack
from conftest import ROOT
from uavtrack import _lib

U = 2.0 ** -24                                                          # the unit roundoff of float32


# ---- the mirror against an independent float64 GAE -------------------------------------------------------------------------

@pytest.mark.parametrize("lam,gamma", [(0.0, 0.95), (0.5, 0.99), (0.9, 0.95), (0.95, 1.0), (1.0, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_the_fp32_fold_agrees_with_the_fp64_sum_of_discounted_td_errors(lam, gamma):
    """The bound, derived, not tuned.  Write S_u = sum_k (g l)^k (|r| + g |V|)_{u+k} over the rest of u's segment; every
    intermediate of step u (gl * G, r + ., d * V, R + .) is at most S_u in magnitude.  A step rounds four times (4 U S_u)
    and uses two rounded constants: gl = fl(g * l), one rounding on the term gl * G (U S_u), and c = fl(g * fl(1 - l)),
    two on the term c * V (2 U S_u).  So e_u <= gl e_{u+1} + 7 U S_u, and since (g l)^k S_{u+k} <= S_u, over the L steps to
    the cut e_t <= 7 L U S_t.  The last subtraction G_t - Vs_t rounds once more: U (S_t + |Vs_t|).  mag_t >= S_t + |Vs_t|,
    so |A32 - A64| <= (7 L + 1) U mag_t to first order; the bound below grants one more U mag_t for the second-order
    terms ((1 + U)^(7 L) - 1 - 7 L U is below U for every L < 2^10)."""
    rng = np.random.default_rng(int(lam * 100) * 7 + int(gamma * 100))
    worst = 0.0
    for T in (1, 2, 9, 64, 200):
        for _ in range(6):
            r = (rng.standard_normal(T) * 3).astype(np.float32)
            V = (rng.standard_normal(T) * 4).astype(np.float32)
            done = (rng.random(T) < 0.1).astype(np.uint8) if rng.random() < 0.7 else None
            # the value of the state a step began in: V(obs_in), then V of the state the step before ended in, or of
            # the fresh state behind a fired done
            fresh = (rng.standard_normal(T) * 4).astype(np.float32)
            Vs = np.concatenate([fresh[:1], V[:-1]])
            if done is not None:
                Vs[1:] = np.where(done[:-1] != 0, fresh[1:], Vs[1:])
            G, adv = gm.chain(r, V, Vs, done, lam, gamma)
            A64, mag = gm.gae64(r, V, Vs, done, lam, gamma)
            L = lm.segment_lengths(T, done)
            bound = (7 * L + 2) * U * mag
            err = np.abs(adv.astype(np.float64) - A64)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (T, float((err / bound).max()))
            # and G itself is the stored value target: advantage + the state's value, to the last rounding
            assert (np.abs(G.astype(np.float64) - (A64 + Vs)) <= bound).all()
    print(f"lambda = {lam}, gamma = {gamma}: worst share of the bound {worst:.3f}")


def test_the_mirrors_stores_are_the_lambda_mirrors_with_the_pair_folded_once_more():
    rng = np.random.default_rng(3)
    T, B, N = 9, 3, 2
    obs_in = rng.standard_normal((B, N, 12)).astype(np.float32)
    obs, so = (rng.standard_normal((T, B, N, 12)).astype(np.float32) for _ in range(2))
    act = rng.integers(0, 12, (T, B, N)).astype(np.int32)
    rew, val, vso = ((rng.standard_normal((T, B, N)) * 3).astype(np.float32) for _ in range(3))
    vin = rng.standard_normal((B, N)).astype(np.float32)
    done = np.zeros((T, B), np.uint8)
    done[0, 0] = done[3, 1] = done[4, 1] = done[T - 1, 2] = 1
    for d, s, v in ((None, None, None), (done, so, vso)):
        g = gm.transitions(obs_in, obs, act, rew, val, vin, v, 0.9, 0.95, d, s)
        l = lm.transitions(obs_in, obs, act, rew, val, 0.9, 0.95, d, s)
        for k in ("states", "actions", "next_states"):
            assert g[k].tobytes() == l[k].tobytes(), k
        want = l["rewards"] + (l["discounts"] * val.reshape(-1)).astype(np.float32)
        assert g["rewards"].tobytes() == want.astype(np.float32).tobytes()
        assert (g["discounts"].view(np.int32) == 0).all()
        Vs = gm.state_values(val, vin, v, d).reshape(-1)
        assert g["advantages"].tobytes() == (g["rewards"] - Vs).astype(np.float32).tobytes()
    # the value of the state a step began in: values_in first, values_start behind a fired done, values[t - 1] otherwise
    Vs = gm.state_values(val, vin, vso, done)
    assert np.array_equal(Vs[0], vin) and np.array_equal(Vs[1, 0], vso[0, 0]) and np.array_equal(Vs[1, 1], val[0, 1])
    assert np.array_equal(Vs[4, 1], vso[3, 1]) and np.array_equal(Vs[5, 1], vso[4, 1]) and np.array_equal(Vs[6, 1], val[5, 1])


# ---- the bindings ----------------------------------------------------------------------------------------------------------

CTYPE = {"uavtrack_replay *": C.c_void_p, "uavtrack_learner *": C.c_void_p, "const uavtrack_replay_ring *": C.POINTER(_lib.ReplayRing),
         "float *": C.c_void_p, "const float *": C.c_void_p, "const int32_t *": C.c_void_p, "const uint8_t *": C.c_void_p,
         "const int64_t *": C.c_void_p, "void *": C.c_void_p, "int64_t": C.c_int64, "double": C.c_double}


@pytest.mark.parametrize("name", ["uavtrack_replay_add_rollout_gae", "uavtrack_learner_update_stored",
                                  "uavtrack_learner_grad_stored"])
def test_symbols_are_declared_exported_and_bound_with_the_headers_argument_lists(name):
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/uavtrack.h"
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", a).group(1) for a in decl]
    types = [a[:-len(n)].strip() for a, n in zip(decl, names)]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [CTYPE[t] for t in types]
    assert hasattr(_lib.load(), name), f"{name} is not exported by the built library"
    assert C.sizeof(_lib.ReplayRing) == 64                                 # advantages travel beside the ring struct
    if name.startswith("uavtrack_learner"):                                # the _clipped list with advantages before log_mu
        clipped = re.search(r"\bint\s+" + name.replace("_stored", "_clipped") + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        cn = [re.search(r"(\w+)$", " ".join(a.split())).group(1) for a in clipped.split(",")]
        assert [x for x in names if x != "advantages"] == cn and names.index("advantages") == names.index("log_mu") - 1


# ---- host refusals ---------------------------------------------------------------------------------------------------------

class _Bare(uavtrack.ReplayRing):
    """The host-side state of a ring without its device handle."""

    def __init__(self, capacity=8):
        self.capacity, self.device, self.max_batch = capacity, torch.device("cpu"), 4


def test_with_gae_sets_the_ring_up_and_excludes_the_other_two_forms():
    ring = _Bare()
    assert ring.with_gae(0.9, 0.95) is ring
    assert ring.gae and ring.lam == 0.9 and ring.gamma == 0.95 and ring.n_step == 1
    assert ring.advantages.dtype == torch.float32 and ring.advantages.shape == (8,) and torch.isnan(ring.advantages).all()
    assert (ring.discounts.numpy().view(np.int32) == np.float32(0.95).view(np.int32)).all()
    with pytest.raises(ValueError, match="GAE ring"):
        ring.with_lambda(0.9, 0.95)
    with pytest.raises(ValueError, match="GAE ring"):
        ring.with_nstep(3, 0.95)
    assert ring.gae and ring.n_step == 1
    with pytest.raises(ValueError, match="lambda ring"):
        _Bare().with_lambda(0.9, 0.95).with_gae(0.9, 0.95)
    with pytest.raises(ValueError, match="n_step = 3"):
        _Bare().with_nstep(3, 0.95).with_gae(0.9, 0.95)
    for lam, gamma, word in ((-0.1, 0.9, "lam"), (float("nan"), 0.9, "lam"), (0.5, 1.5, "gamma")):
        fresh = _Bare()
        with pytest.raises(ValueError, match=word):
            fresh.with_gae(lam, gamma)
        assert not fresh.gae and fresh.advantages is None and fresh.discounts is None
    both = _Bare().with_behaviour().with_gae(0.9, 0.95)                      # composes with the behaviour store
    assert both.log_mu is not None and _Bare().with_gae(0.9, 0.95).with_behaviour().advantages is not None
    assert uavtrack.ReplayRing.advantages is None and not uavtrack.ReplayRing.gae
    ps = inspect.signature(uavtrack.ReplayRing.add_rollout_gae).parameters
    assert list(ps) == ["self", "obs_in", "out", "critic", "values", "values_in", "values_start", "behaviour", "log_mu"]
    assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None for k in list(ps)[3:])


def _small_rollout(rng, T=3, B=2, N=2):
    r = dict(obs_in=rng.standard_normal((B, N, 12)), obs=rng.standard_normal((T, B, N, 12)),
             reward=rng.standard_normal((T, B, N)), values=rng.standard_normal((T, B, N)),
             values_in=rng.standard_normal((B, N)), values_start=rng.standard_normal((T, B, N)))
    r = {k: torch.from_numpy(v.astype(np.float32)) for k, v in r.items()}
    r["actions"] = torch.from_numpy(rng.integers(0, 12, (T, B, N)).astype(np.int32))
    return r


def test_the_new_arguments_are_refused_where_they_do_not_fit():
    r = _small_rollout(np.random.default_rng(5))
    out = {k: r[k] for k in ("obs", "actions", "reward")}
    v3 = dict(values=r["values"], values_in=r["values_in"])
    for ring in (_Bare(), _Bare().with_nstep(3, 0.95), _Bare().with_lambda(0.9, 0.95)):   # not a GAE ring
        with pytest.raises(ValueError, match="GAE ring"):
            ring.add_rollout_gae(r["obs_in"], out, **v3)
        with pytest.raises(ValueError, match="GAE ring"):                    # before anything is enqueued
            ring.add({"states": torch.zeros(2, 12), "actions": torch.zeros(2, dtype=torch.int32), "rewards": torch.zeros(2),
                      "next_states": torch.zeros(2, 12), "advantages": torch.zeros(2)})
    ring = _Bare().with_gae(0.9, 0.95)
    ring.store = {}
    ring._ring = lambda: None
    with pytest.raises(ValueError, match="add_rollout_gae"):                 # add_rollout keeps its list: critic= alone here
        ring.add_rollout(r["obs_in"], out, values=r["values"])
    with pytest.raises(ValueError, match="behaviour ring"):
        ring.add_rollout_gae(r["obs_in"], out, log_mu=r["values"], **v3)
    for kw in (dict(), dict(values=r["values"]), dict(values_in=r["values_in"]), dict(critic=object(), **v3)):
        with pytest.raises(ValueError, match="exactly one"):
            ring.add_rollout_gae(r["obs_in"], out, **kw)
    with pytest.raises(ValueError, match="start_obs"):                       # values_start without done / start_obs
        ring.add_rollout_gae(r["obs_in"], out, values_start=r["values_start"], **v3)
    ends = dict(out, done=torch.zeros(3, 2, dtype=torch.uint8), start_obs=r["obs"].clone())
    with pytest.raises(ValueError, match="exactly one"):                     # and done / start_obs without values_start
        ring.add_rollout_gae(r["obs_in"], ends, **v3)
    for bad in (r["values_in"].double(), r["values_in"].reshape(-1)[:-1], r["values_in"].t()):
        with pytest.raises(ValueError, match="values_in must be"):
            ring.add_rollout_gae(r["obs_in"], out, values=r["values"], values_in=bad)


def test_the_learner_refuses_the_reference_loss_and_another_gamma():
    lct.REC.calls, lct.REC.known, lct.REC.fresh, lct.REC.dump = [], {}, [], False
    ring = lct._bare_ring(uavtrack.ReplayRing, "ring0", 32, 20).with_gae(0.9, 0.95)
    L = lct.Learner()
    L.loss = "reference"
    for call in (lambda: L.update_from(ring, 8), lambda: L.grad_from(ring, 8), lambda: L.update_from(ring.sweep(8, "all"), 8),
                 lambda: L.update({"states": torch.zeros(4, 12), "actions": torch.zeros(4, dtype=torch.int32),
                                   "rewards": torch.zeros(4), "next_states": torch.zeros(4, 12)},
                                  advantages=torch.zeros(4))):
        with pytest.raises(ValueError, match=r"-mean\(delta\) / N"):         # the reason the other per-row features give
            call()
    assert not [c for c in lct.REC.calls if "learner" in c]
    other = lct.Learner(gamma=0.9)
    for call in (lambda: other.update_from(ring, 8), lambda: other.grad_from(ring, 8),
                 lambda: other.update_from_many([ring], 8), lambda: other.update_from(ring.sweep(8, "all"), 8)):
        with pytest.raises(ValueError, match="gamma = 0.95"):
            call()
    assert not [c for c in lct.REC.calls if "learner" in c]


# ---- the calls a learner enqueues ------------------------------------------------------------------------------------------

def _trace(ring, call):
    lct.REC.calls, lct.REC.known, lct.REC.fresh, lct.REC.dump = [], {}, [], False
    lct._register("ring0", ring)
    lct.REC.known["ring0.advantages"] = ring.advantages
    call(lct.Learner())
    return list(lct.REC.calls)


def test_a_gae_ring_takes_the_stored_entry_points_with_its_store_and_nothing_else_changes():
    plain = lambda: lct._bare_ring(uavtrack.ReplayRing, "ring0", 32, 20)      # noqa: E731
    ring = plain().with_gae(0.9, 0.95)
    calls = _trace(ring, lambda L: L.update_from(ring, 8))
    assert [c.split("(")[0] for c in calls] == ["uavtrack_replay_sample_uniform", "uavtrack_learner_update_stored"]
    args = calls[1].split("(", 1)[1].rstrip(")").split(", ")
    # learner, n, four stores, capacity, indices, weights, discounts, advantages, log_mu, clip_eps, ratio_out, outputs, stream
    assert args[6:14] == ["32", "ring0._idx+0", "None", "ring0.discounts+0", "ring0.advantages+0", "None", "0.0", "None"]
    assert len(args) == len(_lib.SIGNATURES["uavtrack_learner_update_stored"][1])
    # a behaviour store is read under clip_eps alone; the sweep presents the ring's advantages
    both = plain().with_gae(0.9, 0.95).with_behaviour()
    calls = _trace(both, lambda L: L.update_from(both, 8))
    assert calls[1].split(", ")[10:12] == ["ring0.advantages+0", "None"]
    calls = _trace(both, lambda L: L.update_from(both.sweep(8, "all"), 8, clip_eps=0.2))
    assert [c.split("(")[0] for c in calls] == ["uavtrack_replay_sample_sweep", "uavtrack_learner_update_stored"]
    assert calls[1].split(", ")[10:13] == ["ring0.advantages+0", "ring0.log_mu+0", "0.2"]
    calls = _trace(both, lambda L: L.grad_from(both, 8, clip_eps=0.2))
    assert calls[1].startswith("uavtrack_learner_grad_stored(") and "ring0.advantages+0, ring0.log_mu+0, 0.2" in calls[1]
    calls = _trace(both, lambda L: L.update_from_many([both], 8))
    assert [c.split("(")[0] for c in calls] == ["uavtrack_replay_sample_uniform", "uavtrack_learner_grad_stored",
                                                "uavtrack_learner_apply"]
    # without advantages: the recorded trace of every buffer, path and option is the one tests/golden holds
    golden = json.load(open(lct.GOLDEN))
    for key in lct.case_keys():
        got = lct.run_case(key)
        assert got == golden[key], key
        assert not any("_stored" in line for line in got), key
