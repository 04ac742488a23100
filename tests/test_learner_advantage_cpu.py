"""The batch-normalised advantage (uavtrack_learner_set_advantage, DeviceActorCritic.set_advantage) without a GPU: the
mirror of tests/learner_advantage_mirror.py against torch autograd in float64; the restated statistics against numpy; the
premises of every case tests/test_hip_learner_advantage.py runs; the refusals of the Python layer before any library call
(on tests/learner_call_trace.py's handle-less learner, whose library is a recorder); the mode "raw" enqueues the recorded
calls; the new symbols are declared, bound and exported; sharding's learner state does not carry the setting."""
import json
import os
import re

import numpy as np
import pytest
import torch

import learner_advantage_mirror as am
import learner_call_trace as lct
import learner_harness as lh
import learner_mirror as mirror
from uavtrack import _lib, sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(32, 12, 2, False), (33, 9, 257, True)]


# ---- 1. the mirror is autograd with the advantage detached -----------------------------------------------------------

@pytest.mark.parametrize("form", ["plain", "entropy+weights", "clipped", "clipped+entropy+weights"])
@pytest.mark.parametrize("H,A,n,gather", SMALL)
def test_the_mirror_is_float64_autograd_with_the_advantage_a_constant(H, A, n, gather, form):
    c = am.host_case(H, A, n, gather)
    b = am.rows(c)
    w = am.weights(n) if "weights" in form else None
    ent = 0.01 if "entropy" in form else 0.0
    clip = (c.log_mu[c.idx], am.EPS_CLIP) if "clipped" in form else None
    u, row = am.losses_and_grads(c.blob, H, A, *b, am.GAMMA, weights=w, entropy_coef=ent, clip=clip)
    al, cl, g = am.autograd(c.blob, H, A, *b, am.GAMMA, row["adv"], w, ent, clip)
    assert abs(u.actor_loss - al) <= 1e-12 * (abs(al) + 1) and abs(u.critic_loss - cl) <= 1e-12 * cl
    assert np.abs(u.grad - g).max() <= 1e-11 * np.abs(g).max()
    # the raw sum w delta is back in loss word 1, and the critic never saw the advantage
    raw = mirror.shard_sums(c.blob, H, A, *b, am.GAMMA, "per_sample", w, ent)
    na = mirror.layout(H, A)[1][4]
    assert row["loss"][1] == raw["loss"][1] and row["loss"][3] == raw["loss"][3] and row["loss"][0] == raw["loss"][0]
    assert np.array_equal(row["g"][na:], raw["g"][na:]) and np.array_equal(row["td"], raw["td"])
    assert np.abs(row["g"][:na] - raw["g"][:na]).max() > 1e-3 * np.abs(raw["g"][:na]).max()


def test_a_given_pair_of_zero_and_one_is_the_raw_mirror_on_float32_deltas():
    H, A, n, gather = SMALL[1]
    c = am.host_case(H, A, n, gather)
    row = am.shard_sums(c.blob, H, A, *am.rows(c), am.GAMMA, given=(0.0, 1.0))
    assert np.array_equal(row["adv"], row["td"].astype(np.float32).astype(np.float64))
    half = am.shard_sums(c.blob, H, A, *am.rows(c), am.GAMMA, given=(0.0, 0.5))
    na = mirror.layout(H, A)[1][4]
    assert np.allclose(half["g"][:na], 0.5 * row["g"][:na], rtol=1e-13, atol=0) and half["loss"][2] == 0.5 * row["loss"][2]


# ---- 2. the statistics -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,gather", am.SHAPES)
def test_the_restated_statistics_are_numpys(H, A, n, gather):
    c = am.host_case(H, A, n, gather)
    td32 = mirror.forward(c.blob, H, A, *am.rows(c), am.GAMMA).delta.astype(np.float32)
    mean, inv, std = am.stats(td32)
    x = td32.astype(np.float64)
    assert abs(mean - np.mean(x)) <= 1e-12 * abs(np.mean(x))
    assert abs(std - np.std(x, ddof=1)) <= 1e-12 * np.std(x, ddof=1)
    assert abs(inv - 1.0 / (np.std(x, ddof=1) + 1e-8)) <= 1e-12 * inv
    assert abs(std - float(torch.from_numpy(x).std())) <= 1e-12 * std
    adv = am.standardise(td32, np.float32(mean), np.float32(inv))
    assert adv.dtype == np.float32 and abs(adv.astype(np.float64).mean()) < 1e-5 and abs(adv.astype(np.float64).std(ddof=1) - 1) < 1e-5


def test_the_order_of_the_sums_is_the_documented_one():
    """Chunks of 256, the halving tree, chunk sums ascending: spelled out once more with Python floats."""
    x = np.random.RandomState(0).standard_normal(700) * np.logspace(-6, 6, 700)
    total = 0.0
    for c0 in range(0, 700, 256):
        part = [float(v) for v in x[c0:c0 + 256]] + [0.0] * (256 - len(x[c0:c0 + 256]))
        h = 128
        while h >= 1:
            for k in range(h):
                part[k] = part[k] + part[k + h]
            h //= 2
        total = total + part[0]
    assert am.ordered_sum(x) == total
    # equal deltas: std 0, inv 1e8, the advantage exactly 0; and a mean of 1000 standard deviations
    mean, inv, std = am.stats(np.full(300, 2.5, np.float32))
    assert (mean, std, inv) == (2.5, 0.0, 1e8) and not am.standardise(np.full(300, 2.5, np.float32), mean, inv).any()
    big = (1000.0 + np.random.RandomState(1).uniform(-1, 1, 4097)).astype(np.float32)
    mean, inv, std = am.stats(big)
    assert abs(std - np.std(big.astype(np.float64), ddof=1)) <= 1e-12 * std and mean / std > 1000


# ---- 3. every GPU case decides something -----------------------------------------------------------------------------

def test_the_gpu_cases_decide_something():
    """The shift makes most raw TD errors positive; the standardised advantage is not: many rows change sign, and in every
    clipped case rows exist whose gate outcome differs between delta_i and A_i, none near a boundary."""
    for H, A, n, gather in am.SHAPES:
        c = am.host_case(H, A, n, gather)
        mean, std, flips, differ, near = am.census(c)
        print(f"H {H} A {A} n {n}: mean {mean:.3f} std {std:.3f}, {flips} sign changes, {differ} rows whose gate differs")
        assert mean > std and near == 0
        assert (c.log_mu <= 0).all()
        if n > 2:
            assert flips >= n // 4 and differ >= n // 10
        if (H, A, n) == (128, 12, 6007):
            assert differ >= 100 and flips >= 100
    # and the normalised update is far from the raw one: a test that compares with the mirror tells them apart
    H, A, n, gather = am.SHAPES[2]
    c = am.host_case(H, A, n, gather)
    raw = mirror.losses_and_grads(c.blob, H, A, *am.rows(c), am.GAMMA, "per_sample")
    u, _ = am.losses_and_grads(c.blob, H, A, *am.rows(c), am.GAMMA)
    assert np.abs(u.grad - raw.grad).max() > 100 * lh.tol_g(n, u.grad)


# ---- 4. the Python layer refuses before any library call -------------------------------------------------------------

def _bare(loss="per_sample"):
    L = lct.Learner()
    L.loss = loss
    lct.REC.calls, lct.REC.known, lct.REC.fresh, lct.REC.dump = [], {}, [], False
    return L


def test_set_advantage_refuses_before_any_library_call():
    L = _bare("reference")
    for mode in ("batch", torch.zeros(2)):
        with pytest.raises(ValueError, match="mean 0"):
            L.set_advantage(mode)
    L.set_advantage("raw")                                            # the default is allowed on either form
    assert lct.REC.calls == ["uavtrack_learner_set_advantage(learner, 0, 1e-08, None)"]
    L = _bare()
    for eps in (float("nan"), -1e-8, -float("inf")):
        with pytest.raises(ValueError, match="eps"):
            L.set_advantage("batch", eps)
    for bad in (torch.zeros(3), torch.zeros(2, 1), torch.zeros(2, dtype=torch.float64), torch.zeros(2, device="meta"),
                torch.zeros(4)[::2]):
        with pytest.raises(ValueError, match=r"float32 tensor \[2\]"):
            L.set_advantage(bad)
    with pytest.raises(ValueError, match="mode"):
        L.set_advantage("running")
    assert lct.REC.calls == [] and L._advantage == "raw" and L.advantage_stats is None
    pair = torch.tensor([0.0, 1.0])
    lct.REC.known["pair"] = pair
    L.set_advantage(pair)
    assert lct.REC.calls == ["uavtrack_learner_set_advantage(learner, 2, 1e-08, pair+0)"] and L._advantage is pair


def test_one_row_in_batch_mode_is_refused_before_any_library_call():
    L = _bare()
    L.set_advantage("batch", 1e-6)
    assert [c.split("(")[0] for c in lct.REC.calls] == ["uavtrack_learner_set_advantage_stats", "uavtrack_learner_set_advantage"]
    assert lct.REC.calls[1].endswith("(learner, 1, 1e-06, None)") and L.advantage_stats.shape == (3,)
    del lct.REC.calls[:]
    store = {"states": torch.zeros(4, 12), "actions": torch.zeros(4, dtype=torch.int32), "rewards": torch.zeros(4),
             "next_states": torch.zeros(4, 12)}
    with pytest.raises(ValueError, match="two rows"):
        L._run(1, store, 4, None, None)
    with pytest.raises(ValueError, match="two rows"):
        L._grad(1, store, 4, None)
    ring = lct.make_buffer("ReplayRing.plain")
    ring.count = 1
    with pytest.raises(ValueError, match="two rows"):
        L.update_from(ring, 8)
    assert not [c for c in lct.REC.calls if c.startswith(("uavtrack_learner_update", "uavtrack_learner_grad"))]
    L._run(2, store, 4, None, None)                                   # two rows pass
    assert lct.REC.calls[-1].startswith("uavtrack_learner_update(")
    L.set_advantage("raw")
    L._run(1, store, 4, None, None)                                   # and raw takes one row again


# ---- 5. raw enqueues the recorded calls ------------------------------------------------------------------------------

def test_with_the_mode_raw_the_drawn_paths_enqueue_the_recorded_calls(monkeypatch):
    """A learner that went to "batch" and back to "raw" draws and enqueues what tests/golden/learner_calls.json holds."""
    golden = json.load(open(lct.GOLDEN))

    class BackToRaw(lct.Learner):
        def __init__(self):
            super().__init__()
            self.set_advantage("batch")
            self.set_advantage("raw")

    monkeypatch.setattr(lct, "Learner", BackToRaw)
    keys = [k for k in lct.case_keys() if k.split("|")[0] in ("ReplayRing.plain", "PrioritizedReplayRing.nstep+behaviour",
                                                               "PrioritizedDeviceReplayBuffer")]
    assert len(keys) == 3 * len(lct.PATHS) * len(lct.OPTIONS)
    for key in keys:
        lines = lct.run_case(key)
        assert [ln.split("(")[0] for ln in lines[:3]] == ["uavtrack_learner_set_advantage_stats"] + ["uavtrack_learner_set_advantage"] * 2
        rest = [re.sub(r"fresh(\d+)", lambda m: f"fresh{int(m.group(1)) - 1}", ln) for ln in lines[3:]]
        assert rest == golden[key], key


# ---- 6. the symbols --------------------------------------------------------------------------------------------------

NEW = ("uavtrack_learner_set_advantage", "uavtrack_learner_get_advantage", "uavtrack_learner_set_advantage_stats")


def test_the_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(uavtrack_learner \*learner", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for word, value in (("RAW", 0), ("BATCH", 1), ("GIVEN", 2)):
        assert re.search(rf"UAVTRACK_ADVANTAGE_{word}\s*=\s*{value}\b", hdr)
        assert getattr(_lib, f"ADVANTAGE_{word}") == value
    # null-handle and null-argument calls fail with the symbol's name, and need no device
    assert lib.uavtrack_learner_set_advantage(None, 1, 1e-8, None) != 0
    assert lib.uavtrack_last_error().decode().startswith("uavtrack_learner_set_advantage: ")


# ---- sharding's learner state does not carry the setting -------------------------------------------------------------

def test_pack_and_unpack_learner_state_do_not_touch_the_setting():
    from test_learner_target_cpu import _Stub

    class Stub(_Stub):
        _advantage = "batch"

        def set_advantage(self, *a, **k):
            raise AssertionError("the advantage setting is not part of the packed state")

        def get_advantage(self):
            raise AssertionError("the advantage setting is not part of the packed state")

    H, A = 5, 3
    src, dst = Stub(H, A, 1, {"tau": 0.5, "period": None}), Stub(H, A, 2, {"tau": None, "period": None})
    dst._advantage = "raw"
    blk = sharding.pack_learner_state(src)
    assert blk.size == 3 * src.num_params + 16 + 6 + 4 + 14 * H + 1              # the block it was
    sharding.unpack_learner_state(dst, blk)
    assert dst._advantage == "raw" and sharding.pack_learner_state(dst).tobytes() == blk.tobytes()
    assert "NOT carried" in sharding.broadcast_learner.__doc__
