"""KL early stopping of the device learner without a GPU: the mirror (tests/learner_kl_mirror.py) against a plain float64
mean, what a stop-on update_from hands the library (the recorder of tests/learner_call_trace.py), and every refusal the
Python layer makes before any library call."""
import numpy as np
import pytest
import torch

import learner_call_trace as trace
import learner_kl_mirror as klm
import uavtrack

BATCH = trace.BATCH


# ---- the mirror ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 6007])
def test_mirror_equals_a_plain_float64_mean(n):
    r = np.exp(np.random.RandomState(n).uniform(-0.5, 0.5, n)).astype(np.float32)
    r64 = r.astype(np.float64)
    plain = np.mean((r64 - 1.0) - np.log(r64))
    assert plain > 0
    assert abs(klm.kl64(r) - plain) <= 1e-12 * plain
    assert klm.kl(r) == np.float32(klm.kl64(r))


def test_mirror_is_exactly_zero_on_policy_and_infinite_at_an_underflowed_ratio():
    for n in (1, 257, 6007):
        assert klm.kl(np.ones(n, np.float32)) == 0.0 and not np.signbit(klm.kl(np.ones(n, np.float32)))
        assert not klm.stops(np.ones(n, np.float32), 0.0)           # kl > 0.0f is false
    r = np.ones(300, np.float32)
    r[299] = 0.0
    assert klm.kl(r) == np.inf and klm.stops(r, 1e30) and not klm.stops(r, np.inf)
    assert (klm.terms(np.array([0.5, 1.0, 2.0], np.float32)) >= 0).all()


# ---- what the library is handed ----------------------------------------------------------------------------------------------

def _buffer(kind):
    ring = trace._bare_ring(uavtrack.ReplayRing, "ring0", 32, 20).with_behaviour()
    return ring if kind == "ring" else ring.sweep(BATCH, (0, 16))


def _calls(kind, limit):
    """(the calls of turning the stop on, the calls of one update_from behind it) against a fresh recorder."""
    rec = trace.REC
    rec.calls, rec.known, rec.fresh, rec.dump = [], {}, [], False
    learner = trace.Learner()
    buffer = _buffer(kind)
    trace._register("ring0", buffer if kind == "ring" else buffer.ring)
    if kind == "sweep":
        rec.known["sweep._idx"], rec.known["sweep._cursor"] = buffer._idx, buffer._cursor
    setting = []
    if limit is not None:
        learner.set_kl_stop(limit)
        assert learner.kl.shape == (1,) and learner.kl.dtype == torch.float32
        assert learner.kl_state.shape == (2,) and learner.kl_state.dtype == torch.int32
        rec.known["kl"], rec.known["kl_state"] = learner.kl, learner.kl_state
        setting, rec.calls, rec.fresh = rec.calls, [], []
    held = learner.update_from(buffer, BATCH, clip_eps=0.2)
    update = list(rec.calls)
    del held
    return setting, update


@pytest.mark.parametrize("kind", ["ring", "sweep"])
def test_a_stop_on_update_from_sets_once_and_then_enqueues_what_it_enqueued(kind):
    none, off = _calls(kind, None)
    setting, on = _calls(kind, 0.015)
    assert none == [] and len(setting) == 1
    assert setting[0].startswith("uavtrack_learner_set_kl_stop(learner, 1, 0.015, fresh0, fresh1)"), setting
    assert len(off) == 2 and off[0].startswith("uavtrack_replay_sample") and off[1].startswith("uavtrack_learner_update_clipped(")
    assert on == off


def test_turning_it_off_and_the_getters():
    rec = trace.REC
    rec.calls, rec.known, rec.fresh = [], {}, []
    learner = trace.Learner()
    assert learner.kl is None and learner.kl_state is None
    learner.set_kl_stop(float("inf"))                               # observes, never stops
    learner.kl_reset()
    learner.set_kl_stop(None)
    assert learner.kl is None and learner.kl_state is None
    assert [c.split("(")[0] for c in rec.calls] == ["uavtrack_learner_set_kl_stop", "uavtrack_learner_kl_reset",
                                                    "uavtrack_learner_set_kl_stop"]
    assert rec.calls[2] == "uavtrack_learner_set_kl_stop(learner, 0, inf, None, None)"
    with pytest.raises(RuntimeError, match="is off"):
        learner.kl_reset()


# ---- refusals, before any library call ---------------------------------------------------------------------------------------

def _stopped_learner(loss="per_sample"):
    rec = trace.REC
    learner = trace.Learner()
    learner.loss = loss
    rec.calls, rec.known, rec.fresh = [], {}, []
    return learner, rec


@pytest.mark.parametrize("limit", [float("nan"), -1e-3, -float("inf")])
def test_a_bad_limit_raises(limit):
    learner, rec = _stopped_learner()
    with pytest.raises(ValueError, match="must be >= 0"):
        learner.set_kl_stop(limit)
    assert rec.calls == [] and learner.kl is None and learner._kl_limit is None


def test_the_reference_loss_raises():
    learner, rec = _stopped_learner("reference")
    with pytest.raises(ValueError, match='loss="reference"'):
        learner.set_kl_stop(0.02)
    assert rec.calls == []


def test_every_path_without_the_ratios_raises_while_on():
    learner, rec = _stopped_learner()
    learner.set_kl_stop(0.02)
    del rec.calls[:]
    ring, sweep = _buffer("ring"), _buffer("sweep")
    rows = {"states": torch.zeros(4, 12), "actions": torch.zeros(4, dtype=torch.int32), "rewards": torch.zeros(4),
            "next_states": torch.zeros(4, 12)}
    why = "without clip_eps while KL early stopping is on"
    with pytest.raises(ValueError, match=why):
        learner.update(rows)
    with pytest.raises(ValueError, match=why):
        learner.update(rows, weights=torch.ones(4))
    with pytest.raises(ValueError, match=why):
        learner.update(rows, discounts=torch.ones(4))
    with pytest.raises(ValueError, match=why):
        learner.update(rows, advantages=torch.ones(4))              # stored, without log_mu
    with pytest.raises(ValueError, match=why):
        learner.update(rows, log_mu=torch.zeros(4), rho_bar=1.0)
    for buffer in (ring, sweep):
        with pytest.raises(ValueError, match=why):
            learner.update_from(buffer, BATCH)
    with pytest.raises(ValueError, match=why):
        learner._run(4, rows, 4, None, None)                        # behind the public calls: _launch itself
    split = "nowhere to carry a KL sum"
    with pytest.raises(ValueError, match=split):
        learner.grad_from(ring, BATCH, clip_eps=0.2)
    with pytest.raises(ValueError, match=split):
        learner._grad(4, rows, 4, None)
    with pytest.raises(ValueError, match=split):
        learner.apply(torch.zeros(1, learner.row_floats))
    with pytest.raises(ValueError, match=split):
        learner.update_from_many([ring], BATCH, clip_eps=0.2)
    with pytest.raises(ValueError, match=split):
        learner.update_from(ring, BATCH, group="group", clip_eps=0.2)
    assert rec.calls == []                                          # not even a draw: the counters stand
    learner.update(rows, log_mu=torch.zeros(4), clip_eps=0.2)       # and the form that does bring them goes through
    assert [c.split("(")[0] for c in rec.calls] == ["uavtrack_learner_update_clipped"]
    learner.set_kl_stop(None)
    del rec.calls[:]
    learner.update(rows)                                            # off again: as before
    assert [c.split("(")[0] for c in rec.calls] == ["uavtrack_learner_update"]
