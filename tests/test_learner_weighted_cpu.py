"""The importance-weighted learner update without a GPU: the float64 mirror (tests/learner_mirror.py) with weights
against torch float64 autograd on the losses as the header defines them (tests/learner_autograd.py), its w = 1 case
against the call without weights to the bit, and the new entry points' declarations."""
import os
import re

import numpy as np
import pytest

import learner_autograd as ag
import learner_harness as lh
import learner_mirror as mirror
from learner_autograd import rel as _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, A, N, GAMMA = 7, 9, 5, 0.95


def _case(seed=0):
    rng = np.random.RandomState(seed)
    b = lh.batch(rng, N, A)
    blob = lh.init_blob(H, A, 4).astype(np.float64)
    w = rng.uniform(0.0, 1.0, size=N)
    w[2] = 0.0                                                        # one weight exactly 0
    return blob, b, w


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_weighted_mirror_matches_torch_fp64_autograd(loss):
    blob, b, w = _case()
    assert (w == 0).sum() == 1 and w.min() >= 0 and w.max() <= 1
    al, cl, td, g = mirror.losses_and_grads(blob, H, A, *b, GAMMA, loss, weights=w)[:4]
    t = ag.update(blob, H, A, *b, GAMMA, loss, w)
    tal, tcl, ttd, tg = t.actor_loss, t.critic_loss, t.td, t.grad
    assert abs(al - tal) <= 1e-12 * abs(tal) and abs(cl - tcl) <= 1e-12 * abs(tcl)
    assert _rel(td, ttd) <= 1e-12
    assert _rel(g, tg) <= 1e-12
    # the weights matter: the unweighted mirror is far outside that bound on the same batch
    assert _rel(mirror.losses_and_grads(blob, H, A, *b, GAMMA, loss)[3], tg) > 1e-3


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_reference_form_is_the_pairwise_weighted_double_sum(loss):
    """(1 / n^2) sum_i sum_j w_i w_j (-log p_i) delta_j is the reference form's loss; the per-sample form is the diagonal
    rule and differs from it."""
    blob, b, w = _case(1)
    f = mirror.forward(blob, H, A, *b, GAMMA)
    pair = (np.outer(w * -f.logp[np.arange(N), f.a], w * f.delta)).sum() / N ** 2
    al = mirror.losses_and_grads(blob, H, A, *b, GAMMA, loss, weights=w).actor_loss
    if loss == "reference":
        assert abs(al - pair) <= 1e-12 * abs(pair)
    else:
        assert abs(al - pair) > 1e-3 * abs(pair)


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_unit_weights_equal_the_unweighted_mirror_exactly(loss):
    blob, b, _ = _case(2)
    want = mirror.losses_and_grads(blob, H, A, *b, GAMMA, loss)
    for w in (None, np.ones(N)):
        got = mirror.losses_and_grads(blob, H, A, *b, GAMMA, loss, weights=w)
        assert got[0] == want[0] and got[1] == want[1]
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    rows_w, rows_u = mirror.shard_sums(blob, H, A, *b, GAMMA, loss, np.ones(N)), mirror.shard_sums(blob, H, A, *b, GAMMA, loss)
    assert np.array_equal(rows_w["g"], rows_u["g"]) and np.array_equal(rows_w["loss"], rows_u["loss"])


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_weighted_rows_combine_to_the_whole_weighted_batch(loss):
    """Two weighted rows over the halves of a batch, combined by learner_mirror.combine (N = the row counts, not the
    weight sums), give the whole batch's weighted losses and gradient."""
    n = 40
    rng = np.random.RandomState(5)
    b = lh.batch(rng, n, A)
    blob = lh.init_blob(H, A, 6)
    w = lh.make_weights(rng, n)
    rows = [mirror.shard_sums(blob, H, A, *(x[lo:hi] for x in b), GAMMA, loss, w[lo:hi]) for lo, hi in ((0, 17), (17, n))]
    al, cl, g = mirror.combine(rows, H, A, loss)
    wal, wcl, _, wg = mirror.losses_and_grads(blob, H, A, *b, GAMMA, loss, weights=w)[:4]
    assert abs(al - wal) <= 1e-12 * abs(wal) and abs(cl - wcl) <= 1e-12 * abs(wcl)
    assert _rel(g, wg) <= 1e-12


def test_header_and_binding_declare_the_weighted_entry_points():
    from uavtrack import _lib
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    for name, first in (("uavtrack_learner_update_weighted", "uavtrack_learner"),
                        ("uavtrack_learner_grad_weighted", "uavtrack_learner"),
                        ("uavtrack_replay_sample_annealed", "uavtrack_replay")):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + first + r"\s*\*", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    # the weighted calls are the plain ones with one more pointer after `indices`; the annealed draw takes beta0, beta1
    # and anneal_calls where the plain draw takes beta
    S = _lib.SIGNATURES
    for plain, weighted in (("uavtrack_learner_update", "uavtrack_learner_update_weighted"),
                            ("uavtrack_learner_grad", "uavtrack_learner_grad_weighted")):
        pa, wa = S[plain][1], S[weighted][1]
        assert len(wa) == len(pa) + 1 and wa[:8] == pa[:8] and wa[9:] == pa[8:]
    pa, wa = S["uavtrack_replay_sample"][1], S["uavtrack_replay_sample_annealed"][1]
    assert len(wa) == len(pa) + 2 and wa[:5] == pa[:5] and wa[7:] == pa[5:]
    m = re.search(r"int\s+uavtrack_learner_update_weighted\s*\(([^;]*)\)\s*;", hdr)
    args = [x.strip() for x in m.group(1).split(",")]
    assert args[args.index("const int64_t *indices") + 1] == "const float *weights"


def test_python_interface_takes_the_importance_arguments():
    import inspect
    import uavtrack
    L, R = uavtrack.DeviceActorCritic, uavtrack.PrioritizedReplayRing
    assert "weights" in inspect.signature(L.update).parameters
    for fn in (L.update_from, L.grad_from, L.update_from_many):
        ps = inspect.signature(fn).parameters
        assert ps["importance"].default is False and ps["beta_final"].default is None and ps["anneal_calls"].default == 0
        assert ps["beta"].default == 0.4
    ps = inspect.signature(R.draw).parameters
    assert ps["beta_final"].default is None and ps["anneal_calls"].default == 0
