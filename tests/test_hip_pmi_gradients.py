"""The device PMI trainer's gradients on the MI355X, element by element against the float64 mirror: a fresh trainer
(zero moments), one mini-batch, every trainable element's gradient recovered from exp_avg to one fp32 rounding and
compared in the metric of tests/pmi_gradient_cases.py (|g - g_fp64| over the sum of the absolute terms of the element's
defining sum) at the tolerance of the case's class.  The grid sits where the kernels change their code path: the
512-row limit of the column kernels, partial 16 x 16 tiles and 128-element slices of the GEMM, a slice across the side
boundary, the head's 256-row passes and its 32-feature unrolled loop.  Three cases take a second step in the same call.

Device worst over the grid, in units of the tolerance (TOL_FACTOR x the fp32 torch CPU reference's worst): see
DESIGN.md 4.9."""
import numpy as np
import pytest

import pmi_gradient_cases as pc
import pmi_trainer_mirror as mirror
from test_hip_pmi_trainer import LR, _call, _sd_np, _trainer

pytestmark = pytest.mark.gpu
assert LR == pc.LR


def _ids(cases):
    return [f"H{H}-B{B}" for H, B in cases]


def _report(tag, e, tol):
    print(tag, " ".join(f"{k}={e[k]:.2e}/{e[k] / tol[k]:.2f}" for k in mirror.param_names()))


@pytest.mark.parametrize("H,B", pc.GRID, ids=_ids(pc.GRID))
def test_gradients_against_fp64_mirror(H, B):
    c = pc.build_case(H, B)
    tr = _trainer(H, B, c.sd)
    avg, losses, outs = _call(tr, c.rows, pc.N_UAV, c.t, c.u, B)
    tr.check()
    m, v, steps = tr.optimizer_state()
    np.testing.assert_array_equal(steps, np.ones(18, np.int64))
    msd, _, mavg, rec = mirror.train_pmi(c.sd, mirror.new_adam(), c.rows, pc.N_UAV, c.t, c.u, B, lr=pc.LR)
    got = pc.split_params(pc.recovered_gradient(m, v), H)
    e = pc.gradient_errors(got, rec["grads"][0], pc.gradient_scales(c.sd, c.x12, c.x13))
    gtol = pc.tolerance(B)
    _report(f"H={H} B={B}", e, gtol)                             # every figure, before anything is asserted
    # outputs, loss and running statistics: the tolerances of test_sweep_against_fp64_mirror
    tol = 1e-3 if B == 2 else 1e-4
    np.testing.assert_allclose(losses, np.abs(rec["loss"]), rtol=tol)
    assert avg == pytest.approx(mavg, rel=tol)
    np.testing.assert_allclose(outs[:, 0], np.stack(rec["o12"]), rtol=tol, atol=tol)
    np.testing.assert_allclose(outs[:, 1], np.stack(rec["o13"]), rtol=tol, atol=tol)
    # every tensor's gradient
    over = {k: (e[k], gtol[k]) for k in e if not e[k] <= gtol[k]}
    assert not over, over
    sd = _sd_np(tr)
    for bn in pc.BN:
        np.testing.assert_allclose(sd[bn + ".running_var"], msd[bn + ".running_var"], rtol=tol, atol=1e-5)
        np.testing.assert_allclose(sd[bn + ".running_mean"], msd[bn + ".running_mean"], rtol=tol, atol=1e-5)
        assert int(sd[bn + ".num_batches_tracked"]) == int(c.sd[bn + ".num_batches_tracked"]) + 2


@pytest.mark.parametrize("H,B", pc.TWO_STEP, ids=_ids(pc.TWO_STEP))
def test_second_step_gradients(H, B):
    """The step's row offset and the rewriting of the gradient buffer: trainer A takes the first B triples, trainer B
    the same and B more in one call.  B's first step is A's bit for bit; its second step's gradient, recovered from
    the two exp_avg, is the mirror's at A's device parameters on the second B triples, within the class's tolerance
    plus the recovery's own rounding (second_step_gradient)."""
    c = pc.build_two_step_case(H, B)
    a, b = _trainer(H, B, c.sd), _trainer(H, 2 * B, c.sd)
    _, _, outs_a = _call(a, c.rows, pc.N_UAV, c.t[:B], c.u[:B], B)
    _, losses_b, outs_b = _call(b, c.rows, pc.N_UAV, c.t, c.u, B)
    a.check()
    b.check()
    np.testing.assert_array_equal(outs_b[0], outs_a[0])
    m_a, _, steps_a = a.optimizer_state()
    m_b, _, steps_b = b.optimizer_state()
    np.testing.assert_array_equal(steps_a, np.ones(18, np.int64))
    np.testing.assert_array_equal(steps_b, np.full(18, 2, np.int64))
    sd_a = _sd_np(a)
    x12, x13 = c.b2
    # the case's condition at the parameters the device holds
    assert pc.min_abs_y(sd_a, c.b2) >= pc.MARGIN_FACTOR * pc.fp32_forward_error(sd_a, x12, x13)
    loss, o12, o13, g64, _ = mirror.loss_and_grads(sd_a, x12, x13)
    np.testing.assert_allclose(losses_b[1], abs(loss), rtol=1e-4)
    np.testing.assert_allclose(outs_b[1, 0], o12, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(outs_b[1, 1], o13, rtol=1e-4, atol=1e-4)
    g, bound = pc.second_step_gradient(m_b, m_a)
    e = pc.gradient_errors(pc.split_params(g, H), g64, pc.gradient_scales(sd_a, x12, x13), slack=pc.split_params(bound, H))
    gtol = pc.tolerance(B)
    _report(f"second step H={H} B={B}", e, gtol)
    over = {k: (e[k], gtol[k]) for k in e if not e[k] <= gtol[k]}
    assert not over, over
