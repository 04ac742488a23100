"""The bounds of tests/learner_harness.py without a GPU: a synthetic device result made from the float64 mirror passes
them, and a perturbation of 0.9 x a bound passes where 1.1 x the same bound raises, so every bound the learner's GPU
tests apply sits within 10 % of the figure written here.  The factors bracket; they measure nothing."""
import numpy as np
import pytest

import learner_harness as lh
import learner_mirror as mirror

H, A, N = 33, 12, 63
NA = mirror.layout(H, A)[1][4]                                         # the actor's span of the gradient


def _adam(blob, g):
    return mirror.adam(blob.astype(np.float64), np.zeros(g.size), np.zeros(g.size), np.ones(8, np.int64), g, lh.LR, H, A)[0]


@pytest.fixture(scope="module", params=["reference", "per_sample"])
def synthetic(request):
    """The mirror's update and a device result that is the mirror's: td_delta and the losses cast to fp32, exp_avg
    0.1 g, the parameters mirror.adam's."""
    blob = lh.init_blob(H, A, H + N)
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, *lh.batch(np.random.RandomState(1), N, A), lh.GAMMA, request.param)[:4]
    res = dict(al=float(np.float32(ral)), cl=float(np.float32(rcl)), td=rtd.astype(np.float32).astype(np.float64))
    return blob, (ral, rcl, rtd), g, res, {"exp_avg": 0.1 * g, "params": _adam(blob, g)}


def _losses(ref, res, **changed):
    r = dict(res, **changed)
    lh.assert_losses_and_td(r["al"], r["cl"], r["td"], *ref)


def _brackets(check, bound):
    """check(perturbation) passes at 0 and at 0.9 x the bound and raises at 1.1 x it."""
    check(0.0)
    check(0.9 * bound)
    with pytest.raises(AssertionError):
        check(1.1 * bound)


def test_the_gradient_bound_is_the_figure_written_here():
    """2e-6 of the largest element per doubling of n and once more: log2(2 n) = 1 + log2 n."""
    assert lh.tol_g(63, np.array([3.0, -4.0])) == pytest.approx(2e-6 * np.log2(126) * 4.0, rel=1e-12)
    assert lh.tol_g(1, np.array([0.5])) == pytest.approx(1e-6, rel=1e-12)


def test_td_and_both_losses_sit_at_2e_5_of_their_scale(synthetic):
    blob, ref, g, res, st = synthetic
    ral, rcl, rtd = ref
    k = np.abs(rtd).argmax()

    def td_off(e):
        td = res["td"].copy()
        td[k] += e
        _losses(ref, res, td=td)
    _brackets(td_off, 2e-5 * (np.abs(rtd).max() + 1e-6))
    _brackets(lambda e: _losses(ref, res, cl=res["cl"] + e), 2e-5 * (np.mean(rtd ** 2) + 1e-12) + 1e-12)
    _brackets(lambda e: _losses(ref, res, al=res["al"] - e), 2e-5 * (abs(ral) + 30 * np.mean(np.abs(rtd))))


def test_the_entropy_term_widens_the_actor_loss_scale_by_c_log_a(synthetic):
    blob, ref, g, res, st = synthetic
    ral, rcl, rtd = ref
    c = 1.0
    _brackets(lambda e: lh.assert_losses_and_td(res["al"] + e, res["cl"], res["td"], *ref, c, A),
              2e-5 * (abs(ral) + 30 * np.mean(np.abs(rtd)) + c * np.log(A)))


def test_the_gradient_and_the_parameters_sit_at_their_bounds(synthetic):
    blob, ref, g, res, st = synthetic
    k = np.abs(g).argmax()

    def grad_off(e):
        m = st["exp_avg"].copy()
        m[k] += 0.1 * e
        lh.assert_step_from_zero(dict(st, exp_avg=m), blob, g, N, H, A)
    _brackets(grad_off, lh.tol_g(N, g))

    def param_off(e):                                                  # g[k] is the largest element: far from zero
        p = st["params"].copy()
        p[k] -= e
        lh.assert_step_from_zero(dict(st, params=p), blob, g, N, H, A)
    _brackets(param_off, 1e-3 * lh.LR[0 if k < NA else 1] + 1e-6 * abs(st["params"][k]))


def test_a_clip_coefficient_scales_its_networks_gradient(synthetic):
    blob, ref, g, res, st = synthetic
    coef = (0.5, 1.0)
    gc = g.copy()
    gc[:NA] *= 0.5
    lh.assert_step_from_zero({"exp_avg": 0.1 * gc, "params": _adam(blob, gc)}, blob, g, N, H, A, coef)
    with pytest.raises(AssertionError):
        lh.assert_step_from_zero(st, blob, g, N, H, A, coef)
