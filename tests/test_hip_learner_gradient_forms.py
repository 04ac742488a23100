"""The clip, advantage and stored gradient kernels on the MI355X, element by element against float64
(tests/learner_gradient_forms.py): the ten instantiations of learner_grad_body that test_hip_learner_gradients.py does not
reach.  Per case a fresh learner's gradient row (P unscaled sums, four loss sums) and its closed update from zero moments
(the scaled gradient, recovered from exp_avg), in the metric |g - g_fp64| / S at the tolerance of the case's class, the
ratios, td_delta bit-equal between the two calls.  Under set_advantage("batch") the float64 side takes the device's own
advantage_stats[:2], which are held to the numpy restatement here as test_hip_learner_advantage.py holds them.  One case
takes a second update on fresh rows.  The gate is pinned one ulp from its bound on the device's own ratios.

Device worst per class, in units of the tolerance: DESIGN.md 4.8."""
import types

import numpy as np
import pytest
import torch

import learner_advantage_mirror as am
import learner_gradient_cases as lg
import learner_gradient_forms as lf
import learner_harness as lh
import learner_mirror as mirror
import pmi_gradient_cases as pc

pytestmark = pytest.mark.gpu

NEVER = 10 ** 9            # a period no test reaches: a target block that stays what it was given
F32 = np.float32


def _learner(c, lr=lh.LR):
    L = lh.learner(c.H, c.A, "per_sample", c.blob, max_batch=c.n, c=c.c, diag=c.diag, gamma=lg.GAMMA, lr=lr)
    if c.theta is not None:
        L.set_target(period=NEVER)
        L._set_target_params(c.theta)
    if c.form.adv == "batch":
        L.set_advantage("batch")
    elif c.form.adv == "given":
        L.set_advantage(lh.dev(np.array(c.given, F32)))
    return L


def _inputs(c, h=0, eps=None):
    """(n, store, capacity, indices) and _Batch's fields from weights on (weights, discounts, log_mu, clip_eps, a new
    ratio_out, advantages) of the case's batch h on the device; eps: a clip_eps in the case's place."""
    if c.gather:
        rows, cap, it = slice(None), c.cap, lh.dev(c.idx[h])
    else:
        rows, cap, it = slice(h * c.n, (h + 1) * c.n), c.n, None
    store = {k: lh.dev(x[rows]) for k, x in zip(lh.STORES, c.store)}
    opt = lambda x: None if x is None else lh.dev(x[rows])                              # noqa: E731
    clip = c.form.clip is not None
    rest = (None if c.weights is None else lh.dev(c.weights[h]), opt(c.disc), opt(c.log_mu),
            (float(c.form.clip) if eps is None else float(eps)) if clip else None,
            torch.empty(c.n, device=lh.DEV) if clip else None, opt(c.advantages))
    return (c.n, store, cap, it), rest


def _row(L, inp):
    (n, store, cap, it), rest = inp
    row, td = L._grad(n, store, cap, it, None, None, *rest)
    return row.cpu().numpy(), td.cpu().numpy(), None if rest[4] is None else rest[4].cpu().numpy()


def _update(L, inp):
    (n, store, cap, it), rest = inp
    al, cl, td = L._run(n, store, cap, it, None, *rest)
    return lh._result(L, n, al, cl, td, None), None if rest[4] is None else rest[4].cpu().numpy()


def _stats(L, c, td, h=0):
    """(advantage_stats of the last batch-mode call, the restatement's from the call's own td_delta or from the stored
    advantages): to be bit for bit the same."""
    stats = L.advantage_stats.cpu().numpy()
    want = am.stats32(c.advantages[c.idx[h]] if c.form.stored else td)
    print(f"stats {stats} want {want}: ulps {[am.ulps(x, y) for x, y in zip(stats, want)]}")
    return stats, want


def _assert_ratios(got, ref, fs):
    if ref.ratio is not None:
        err, tol = np.abs(got - ref.ratio), lf.ratio_tolerance(fs, ref.ratio)
        print(f"ratios [{lf.form_class(fs)}]: worst share of the bound: {(err / tol).max():.3f}")
        assert (err <= tol).all()


@pytest.mark.parametrize("fs", lf.FORM_GRID, ids=[lf.form_id(fs) for fs in lf.FORM_GRID])
def test_form_gradients_against_fp64(fs):
    c = lf.build_case(fs)
    L = _learner(c)
    row, td_row, ratio_row = _row(L, _inputs(c))
    batch = fs.adv == "batch"
    seen = [_stats(L, c, td_row)] if batch else []
    out, ratio_run = _update(L, _inputs(c))
    if batch:
        seen.append(_stats(L, c, out["td"]))
    ref = lf.fp64(c, stats=seen[0][0][:2].copy() if batch else None)
    P, tag = ref.sums.size, f"{lf.form_id(fs)} [{lf.form_class(fs)}, {lf.kernel_of(fs)[13:-7]}]"
    rtol, gtol = lf.tolerances(fs)
    er = lg.errors(row[:P + 4], np.concatenate([ref.sums, ref.loss4]), ref.S_row, c.H, c.A)
    eg = lg.errors(pc.recovered_gradient(out["exp_avg"], out["exp_avg_sq"]), ref.grad, ref.S_grad, c.H, c.A)
    lg.report(f"{tag} row:", er, rtol)                           # every figure, before anything is asserted
    lg.report(f"{tag} grad:", eg, gtol)
    for stats, want in seen:                                    # the statistics kernels, at the restatement's bits
        assert np.array_equal(stats, want), (stats, want)
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ref.actor_loss, ref.critic_loss, ref.td,
                            c=c.c, A=c.A)
    np.testing.assert_array_equal(td_row, out["td"])
    if fs.clip is not None:
        np.testing.assert_array_equal(ratio_row, ratio_run)
        _assert_ratios(ratio_row, ref, fs)
    tail = row.view(np.int32)[P + 4:]
    assert (int(tail[0]), int(tail[1]), int(tail[2]), int(tail[3])) == (c.n, 0, 0, P)
    assert not lg.over(er, rtol), lg.over(er, rtol)
    assert not lg.over(eg, gtol), lg.over(eg, gtol)
    if fs.inv0 or fs.A == 1:                                    # S = 0: the actor's sums and moments are exactly 0
        na = mirror.layout(c.H, c.A)[1][4]
        assert not row[:na].any() and not out["exp_avg"][:na].any() and not out["exp_avg_sq"][:na].any()
    np.testing.assert_array_equal(out["step"], np.ones(8, np.int64))
    L.check()


@pytest.mark.parametrize("fs", lf.FORM_TWO_STEP, ids=[lf.form_id(fs) for fs in lf.FORM_TWO_STEP])
def test_form_second_step_gradients(fs):
    """A stale lm / xa tile or accumulator: learner A takes batch 1, learner B batch 1 and then batch 2 (fresh rows, fresh
    slots of log_mu and advantages).  B's first update is A's bit for bit; its second gradient, recovered from the two
    exp_avg, is the float64 result at A's device parameters on batch 2."""
    c = lf.build_two_step_case(fs)
    a, b = _learner(c, lg.LR_TWO_STEP), _learner(c, lg.LR_TWO_STEP)
    out_a, _ = _update(a, _inputs(c, 0))
    lh.same(_update(b, _inputs(c, 0))[0], out_a, "the first update")
    out_b, ratio_b = _update(b, _inputs(c, 1))
    np.testing.assert_array_equal(out_b["step"], np.full(8, 2, np.int64))
    theta = a._get_target_params()
    assert theta.tobytes() == c.theta.tobytes()
    lo, err = lg.margin(c, blob=out_a["params"], theta=theta, rows=tuple(x[c.idx[1]] for x in c.store))
    assert lo >= lg.MARGIN_FACTOR * err, (lo, err)
    ref = lf.fp64(c, 1, blob=out_a["params"], theta=theta)
    g, bound = pc.second_step_gradient(out_b["exp_avg"], out_a["exp_avg"])
    e = lg.errors(g, ref.grad, ref.S_grad, c.H, c.A, slack=bound)
    gtol = lf.tolerances(fs)[1]
    lg.report(f"second step {lf.form_id(fs)}:", e, gtol)
    lh.assert_losses_and_td(out_b["actor_loss"], out_b["critic_loss"], out_b["td"], ref.actor_loss, ref.critic_loss,
                            ref.td, c=c.c, A=c.A)
    _assert_ratios(ratio_b, ref, fs)
    assert not lg.over(e, gtol), lg.over(e, gtol)
    for L in (a, b):
        L.check()


# ---- the gate one ulp from its bound

def _gate_case(H, stored):
    """A clip = inf case of R + 1 rows whose weights are powers of two: 2^-12 on every row, and 1 on the rows that share
    the ratio a run picks.  The difference of two rounded sums carries the roundings of both sums, each relative to its own S; it is
    judged against the S of the picked rows' contribution alone, so the other rows must be a small share of every sum
    (124 rows at 2^-12 are 3 % of one at 1).  A row the two runs treated differently by mistake would still show: 2^-12
    of its contribution is some 200 tolerances."""
    n = lg.rows_per_tile(H) + 1
    c = lf.build_case(lf.Form(H, 12, n, "weighted", H == 33, "default", np.inf, "raw", stored, False))
    return types.SimpleNamespace(**{**vars(c), "weights": [np.full(n, 2.0 ** -12, F32)]})


@pytest.mark.parametrize("H,stored", [(256, False), (33, True)])
def test_the_gate_is_inclusive_at_its_bound(H, stored):
    """clip_eps from the device's own ratio: eps_i = r_i - 1 for a row of positive advantage and ratio in (1, 2), so that
    the host folds hi == r_i; eps_j = 1 - r_j for a row of negative advantage and ratio in (0.5, 1), lo == r_j (both
    exact in float32).  Against the run whose bound lies one float32 step of the RATIO further in (eps = next(r_i) - 1:
    one step of eps itself does not move the folded bound), the rows treated differently are those whose ratio equals
    the bound on that side; the unscaled rows differ by those rows' w r A (onehot - p) through the backward pass; the
    critic's words and td are the same bits; loss word 2 moves by a rounding, the surrogate being continuous there."""
    c = _gate_case(H, stored)
    n, i0 = c.n, c.idx[0]
    P = mirror.layout(c.H, c.A)[1][8]
    na = mirror.layout(c.H, c.A)[1][4]
    _, td_inf, ratio = _row(_learner(c), _inputs(c))
    ref = lf.fp64(c)
    _assert_ratios(ratio, ref, c.form)
    adv = ref.adv
    up = np.flatnonzero((adv > 0) & (ratio > 1) & (ratio < 2))
    down = np.flatnonzero((adv < 0) & (ratio > 0.5) & (ratio < 1))
    assert up.size and down.size
    rtol = lf.tolerances(c.form)[0]
    for side, k in (("hi", up[0]), ("lo", down[0])):
        r = ratio[k]
        at = F32(r) - F32(1) if side == "hi" else F32(1) - F32(r)
        step = np.nextafter(r, F32(0)) if side == "hi" else np.nextafter(r, F32(1))
        inside = F32(step) - F32(1) if side == "hi" else F32(1) - F32(step)
        assert mirror.bounds(at)[side == "hi"] == float(r) and mirror.bounds(inside)[side == "hi"] == float(step)
        assert 0 < inside < at
        on_bound = (adv >= 0) & (ratio == r) if side == "hi" else (adv < 0) & (ratio == r)
        w = c.weights[0].copy()
        w[on_bound] = 1.0                                       # (every row of that ratio: a unit that is on in one of
                                                                # them alone has that row's weight in its S)
        ck = types.SimpleNamespace(**{**vars(c), "weights": [w]})
        runs = [_row(_learner(ck), _inputs(ck, eps=e)) for e in (at, inside)]
        (row_at, td_at, ratio_at), (row_in, td_in, ratio_in) = runs
        np.testing.assert_array_equal(ratio_at, ratio); np.testing.assert_array_equal(ratio_in, ratio)
        r64 = ratio.astype(np.float64)
        differ = mirror.gate(r64, adv, float(at)) != mirror.gate(r64, adv, float(inside))
        np.testing.assert_array_equal(differ, on_bound)
        assert differ[k] and mirror.gate(r64, adv, float(at))[k] and not mirror.gate(r64, adv, float(inside))[k]
        # the rows' own contribution, through the backward pass, and its own S
        gz = np.zeros_like(ref.f.p)
        gz[differ] = (w[differ] * r64[differ] * adv[differ])[:, None] * (ref.f.onehot - ref.f.p)[differ]
        zero = np.zeros(n)
        want = mirror.backward(ref.f, gz, zero)
        S = lg.gradient_scales(c, ref.f, gz, zero, np.zeros((4, n)))[0][:P]
        e = lg.errors(row_at[:P].astype(np.float64) - row_in[:P].astype(np.float64), want, S, c.H, c.A)
        lg.report(f"H{H} {side} == {r!r} (row {k}, {int(differ.sum())} on the bound): the rows' difference:", e, rtol)
        assert not lg.over({q: e[q] for q in lg.ACTOR}, rtol)
        assert row_at[na:P].tobytes() == row_in[na:P].tobytes()
        for q in (0, 1, 3):
            assert row_at[P + q].tobytes() == row_in[P + q].tobytes()
        assert td_at.tobytes() == td_in.tobytes() == td_inf.tobytes()
        full = lf.fp64(ck)
        moved = abs(float(row_at[P + 2]) - float(row_in[P + 2]))
        print(f"loss word 2 moves by {moved:.3e}, {moved / (rtol['sum.actor'] * full.S_row[P + 2]):.3f} of its tolerance")
        assert moved <= rtol["sum.actor"] * full.S_row[P + 2]
