"""The device learner's gradients on the MI355X, element by element against float64 (tests/learner_gradient_cases.py):
per case a fresh learner's gradient row (the P unscaled sums and the four loss sums of learner_grad_body, whichever of
its four instantiations the case selects) and its closed update from zero moments (the scaled, clipped gradient,
recovered from exp_avg to one fp32 rounding), both in the metric |g - g_fp64| / S, S the float64 sum of the absolute
terms of the element's defining sum, at the tolerance of the case's class.  The grid sits where the kernel changes
path: the rows per tile R = min(256, 4096 / max(H, 16)), partial tiles, more tiles than one, tiles striding over the
256 workgroups, every action count, the peaked policy, the clip.  Three cases take a second update on fresh rows.

Device worst per class, in units of the tolerance (TOL_FACTOR x the worse of two fp32 CPU references): DESIGN.md 4.8."""
import numpy as np
import pytest

import learner_gradient_cases as lg
import learner_harness as lh
import pmi_gradient_cases as pc

pytestmark = pytest.mark.gpu

NEVER = 10 ** 9            # a period no test reaches: a target block that stays what it was given


def _learner(c, lr=lh.LR):
    L = lh.learner(c.H, c.A, c.loss, c.blob, max_batch=c.n, c=c.c, mgn=c.mgn, diag=c.diag, gamma=lg.GAMMA, lr=lr)
    if c.theta is not None:
        L.set_target(period=NEVER)
        L._set_target_params(c.theta)
    return L


def _inputs(c, h=0):
    """(n, store, capacity, indices, weights, discounts) of the case's batch h on the device: through the index vector
    where the case has one, else the batch's own rows as the store."""
    if c.gather:
        rows, cap, it = slice(None), c.cap, lh.dev(c.idx[h])
    else:
        rows, cap, it = slice(h * c.n, (h + 1) * c.n), c.n, None
    store = {k: lh.dev(x[rows]) for k, x in zip(lh.STORES, c.store)}
    return (c.n, store, cap, it, None if c.weights is None else lh.dev(c.weights[h]),
            None if c.disc is None else lh.dev(c.disc[rows]))


def _update(L, inp):
    n, store, cap, it, w, d = inp
    return lh.update(L, n, store, cap, it, None, w, d)


@pytest.mark.parametrize("sp", lg.GRID, ids=[lg.spec_id(sp) for sp in lg.GRID])
def test_gradients_against_fp64(sp):
    c = lg.build_case(sp)
    ref = lg.fp64(c)
    P = ref.sums.size
    inp = _inputs(c)
    L = _learner(c)
    n, store, cap, it, w, d = inp
    row, td_row = lh.row(L, n, store, cap, it, w, d)
    out = _update(L, inp)
    rtol, gtol = lg.tolerances(sp)
    er = lg.errors(row[:P + 4], np.concatenate([ref.sums, ref.loss4]), ref.S_row, c.H, c.A)
    eg = lg.errors(pc.recovered_gradient(out["exp_avg"], out["exp_avg_sq"]), ref.grad, ref.S_grad, c.H, c.A)
    lg.report(f"{lg.spec_id(sp)} [{lg.case_class(sp)}] row:", er, rtol)         # every figure, before anything is asserted
    lg.report(f"{lg.spec_id(sp)} [{lg.case_class(sp)}] grad:", eg, gtol)
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ref.actor_loss, ref.critic_loss, ref.td,
                            c=c.c, A=c.A)
    np.testing.assert_array_equal(td_row, out["td"])
    tail = row.view(np.int32)[P + 4:]
    assert (int(tail[0]), int(tail[1]), int(tail[2]), int(tail[3])) == (n, 0, 0, P)
    assert not lg.over(er, rtol), lg.over(er, rtol)
    assert not lg.over(eg, gtol), lg.over(eg, gtol)
    if c.mgn and "grad_norm" in out:                            # the norms before clipping, where diagnostics are installed
        np.testing.assert_allclose(out["grad_norm"] * ref.coef, np.minimum(out["grad_norm"], c.mgn), rtol=1e-4)
    np.testing.assert_array_equal(out["step"], np.ones(8, np.int64))
    L.check()


@pytest.mark.parametrize("sp", lg.TWO_STEP, ids=[lg.spec_id(sp) for sp in lg.TWO_STEP])
def test_second_step_gradients(sp):
    """A stale accumulator, partial row or gsum: learner A takes batch 1, learner B batch 1 and then batch 2 (fresh
    rows).  B's first update is A's bit for bit; its second gradient, recovered from the two exp_avg, is the float64
    result at A's device parameters on batch 2, within the class's tolerance plus the recovery's own rounding."""
    c = lg.build_two_step_case(sp)
    a, b = _learner(c, lg.LR_TWO_STEP), _learner(c, lg.LR_TWO_STEP)
    one, two = _inputs(c, 0), _inputs(c, 1)
    out_a = _update(a, one)
    lh.same(_update(b, one), out_a, "the first update")
    out_b = _update(b, two)
    np.testing.assert_array_equal(out_a["step"], np.ones(8, np.int64))
    np.testing.assert_array_equal(out_b["step"], np.full(8, 2, np.int64))
    theta = a._get_target_params() if c.theta is not None else None
    if theta is not None:
        assert theta.tobytes() == c.theta.tobytes()
    # the case's condition at the parameters the device holds
    lo, err = lg.margin(c, blob=out_a["params"], theta=theta, rows=tuple(x[c.idx[1]] for x in c.store))
    assert lo >= lg.MARGIN_FACTOR * err, (lo, err)
    ref = lg.fp64(c, 1, blob=out_a["params"], theta=theta)
    g, bound = pc.second_step_gradient(out_b["exp_avg"], out_a["exp_avg"])
    e = lg.errors(g, ref.grad, ref.S_grad, c.H, c.A, slack=bound)
    gtol = lg.tolerances(sp)[1]
    lg.report(f"second step {lg.spec_id(sp)}:", e, gtol)
    lh.assert_losses_and_td(out_b["actor_loss"], out_b["critic_loss"], out_b["td"], ref.actor_loss, ref.critic_loss,
                            ref.td, c=c.c, A=c.A)
    assert not lg.over(e, gtol), lg.over(e, gtol)
    for L in (a, b):
        L.check()
