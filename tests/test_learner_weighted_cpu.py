"""The importance-weighted learner update without a GPU: the float64 weighted mirror (tests/learner_weighted_mirror.py)
against torch float64 autograd on the losses as the header defines them, its w = 1 case against the unweighted mirror
(tests/learner_mirror.py) to the bit, and the new entry points' declarations."""
import os
import re

import numpy as np
import pytest
import torch

import learner_dp_mirror as dp
import learner_mirror as mirror
import learner_weighted_mirror as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, A, N, GAMMA = 7, 9, 5, 0.95


def _rel(x, y):
    return np.abs(np.asarray(x) - np.asarray(y)).max() / (np.abs(np.asarray(y)).max() + 1e-300)


def _case(seed=0):
    rng = np.random.RandomState(seed)
    b = dp.batch(rng, N, A)
    blob = dp.init_blob(H, A, 4).astype(np.float64)
    w = rng.uniform(0.0, 1.0, size=N)
    w[2] = 0.0                                                        # one weight exactly 0
    return blob, b, w


def _torch_losses(blob, b, w, loss):
    """The weighted losses in torch float64, written as the header states them, and their autograd gradient."""
    import uavtrack
    actor, critic = uavtrack.ActorMLP(12, H, A).double(), uavtrack.ValueMLP(12, H).double()
    params = list(actor.parameters()) + list(critic.parameters())
    o = 0
    with torch.no_grad():
        for p in params:
            p.copy_(torch.from_numpy(blob[o:o + p.numel()]).view_as(p)); o += p.numel()
    s, a, r, s2 = b
    S, S2, R = (torch.from_numpy(np.asarray(x, np.float64)) for x in (s, s2, r))
    Ai = torch.from_numpy(a.astype(np.int64)).view(-1, 1)
    W = torch.from_numpy(np.asarray(w, np.float64))
    target = (R + GAMMA * critic(S2)).detach()
    delta = (target - critic(S)).detach()
    nlp = -torch.log(actor(S).gather(1, Ai).squeeze(1))
    if loss == "reference":
        al = (W * nlp).mean() * (W * delta).mean()                    # the product of the two weighted means
    else:
        al = (W * (nlp * delta)).mean()
    cl = (W * (critic(S) - target) ** 2).mean()
    ga = torch.autograd.grad(al, list(actor.parameters()))
    gc = torch.autograd.grad(cl, list(critic.parameters()))
    g = np.concatenate([x.numpy().ravel() for x in list(ga) + list(gc)])
    return float(al.detach()), float(cl.detach()), delta.numpy(), g


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_weighted_mirror_matches_torch_fp64_autograd(loss):
    blob, b, w = _case()
    assert (w == 0).sum() == 1 and w.min() >= 0 and w.max() <= 1
    al, cl, td, g = wm.losses_and_grads(blob, H, A, *b, GAMMA, loss, w)
    tal, tcl, ttd, tg = _torch_losses(blob, b, w, loss)
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
    f = wm._forward(blob, H, A, *b, GAMMA)
    pair = (np.outer(w * f["nlp"], w * f["delta"])).sum() / N ** 2
    al = wm.losses_and_grads(blob, H, A, *b, GAMMA, loss, w)[0]
    if loss == "reference":
        assert abs(al - pair) <= 1e-12 * abs(pair)
    else:
        assert abs(al - pair) > 1e-3 * abs(pair)


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_unit_weights_equal_the_unweighted_mirror_exactly(loss):
    blob, b, _ = _case(2)
    want = mirror.losses_and_grads(blob, H, A, *b, GAMMA, loss)
    for w in (None, np.ones(N)):
        got = wm.losses_and_grads(blob, H, A, *b, GAMMA, loss, w)
        assert got[0] == want[0] and got[1] == want[1]
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    rows_w, rows_u = wm.shard_sums(blob, H, A, *b, GAMMA, loss, np.ones(N)), dp.shard_sums(blob, H, A, *b, GAMMA, loss)
    assert np.array_equal(rows_w["g"], rows_u["g"]) and np.array_equal(rows_w["loss"], rows_u["loss"])


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_weighted_rows_combine_to_the_whole_weighted_batch(loss):
    """Two weighted rows over the halves of a batch, combined by learner_dp_mirror.combine (N = the row counts, not the
    weight sums), give the whole batch's weighted losses and gradient."""
    n = 40
    rng = np.random.RandomState(5)
    b = dp.batch(rng, n, A)
    blob = dp.init_blob(H, A, 6)
    w = wm.make_weights(rng, n)
    rows = [wm.shard_sums(blob, H, A, *(x[lo:hi] for x in b), GAMMA, loss, w[lo:hi]) for lo, hi in ((0, 17), (17, n))]
    al, cl, g = dp.combine(rows, H, A, loss)
    wal, wcl, _, wg = wm.losses_and_grads(blob, H, A, *b, GAMMA, loss, w)
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
