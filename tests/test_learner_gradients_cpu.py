"""The gradient comparison of tests/learner_gradient_cases.py without a GPU: every case meets its margin condition, both
fp32 CPU references (torch autograd, the strictly sequential float32 sum) pass the comparator with a factor of two to
spare, the wrapper's float64 sums are the mirror's one-call forms' wherever they overlap, the recovery of a gradient from
Adam's first moments round-trips, and wrong backward passes (mutants: changed copies of the float64 backward, held here
and never in the library) fail where they must and only there.  The second half does the same for the form cases of
tests/learner_gradient_forms.py (the clip, advantage and stored kernels): the two grids reach all fourteen kernels, every
case's conditions hold, both references stay within half a tolerance, fourteen wrong per-row blocks are caught."""
import numpy as np
import pytest

import learner_advantage_mirror as am
import learner_gradient_cases as lg
import learner_gradient_forms as lf
import learner_mirror as mirror
import pmi_gradient_cases as pc

IDS = [lg.spec_id(sp) for sp in lg.GRID]
assert len(set(IDS)) == len(IDS)

_REF = {}


def _reference(sp):
    """(case, float64 result, its row words) of a grid case, computed once."""
    if sp not in _REF:
        c = lg.build_case(sp)
        ref = lg.fp64(c)
        _REF[sp] = (c, ref, np.concatenate([ref.sums, ref.loss4]))
    return _REF[sp]


# ---- the cases' own conditions and the two fp32 references

@pytest.mark.parametrize("sp", lg.GRID, ids=IDS)
def test_case_conditions_and_fp32_references(sp):
    c, ref, row64 = _reference(sp)
    lo, err = lg.margin(c)
    assert lo >= lg.MARGIN_FACTOR * err, (lo, err)
    if sp.cls == "peaked":
        assert 30.0 < lg.logit_spread(c.blob, c.H, c.A, c.rows[0]) < 60.0
    if sp.loss == "reference" and sp.n > 2:                     # mean(delta) away from 0 in the shifted half only
        share = abs(ref.td.sum()) / np.abs(ref.td).sum()
        assert share > 0.5 if sp.shift else share < 0.5, share
    rtol, gtol = lg.tolerances(sp)
    for fn in (lg.torch_fp32, lg.sequential_fp32):
        r, g = fn(c)
        er = lg.errors(r, row64, ref.S_row, c.H, c.A)
        eg = lg.errors(g, ref.grad, ref.S_grad, c.H, c.A)
        half = lambda tol: {k: v / 2 for k, v in tol.items()}
        assert not lg.over(er, half(rtol)), (fn.__name__, lg.over(er, half(rtol)))
        assert not lg.over(eg, half(gtol)), (fn.__name__, lg.over(eg, half(gtol)))


def test_the_grid_covers_what_it_names():
    R = lg.rows_per_tile
    assert {sp.H for sp in lg.GRID} == set(lg.HS) and {sp.A for sp in lg.GRID} >= set(lg.AS)
    for H in (200, 256):
        assert {sp.n for sp in lg.GRID if sp.H == H} >= {1, 2, R(H) - 1, R(H), R(H) + 1, 2 * R(H) + 1, 256 * R(H),
                                                          256 * R(H) + 1, 257 * R(H) + 1}
    for H in lg.HS:
        assert {sp.n for sp in lg.GRID if sp.H == H} >= {R(H) + 1, 2 * R(H) + 1}
    for body in lg.BODIES:
        mine = [sp for sp in lg.GRID if sp.body == body]
        assert len({(sp.H, sp.n) for sp in mine}) >= 3 and {sp.gather for sp in mine} == {False, True}
        assert {sp.loss for sp in mine} == ({"per_sample"} if body == "regc" else {"reference", "per_sample"})
    refs = [sp for sp in lg.GRID if sp.loss == "reference"]
    assert abs(sum(sp.shift for sp in refs) - len(refs) / 2) <= 1
    assert sum(sp.cls == "peaked" for sp in lg.GRID) == 4 and sum(sp.mgn is not None for sp in lg.GRID) == 2
    assert any(sp.n == 65537 and sp.H == 16 for sp in lg.GRID)
    assert [R(H) for H in lg.HS] == [256, 256, 256, 240, 128, 124, 64, 32, 20, 16, 16]


@pytest.mark.parametrize("sp", lg.TWO_STEP, ids=[lg.spec_id(sp) for sp in lg.TWO_STEP])
def test_two_step_cases_have_margin(sp):
    """Both steps' margins, the second at the mirror's parameters after step one (the GPU test asserts it again at the
    device's)."""
    c = lg.build_two_step_case(sp)
    lo, err = lg.margin(c, rows=tuple(x[c.idx[0]] for x in c.store))
    assert lo >= lg.MARGIN_FACTOR * err
    g = lg.fp64(c, 0).grad
    blob1 = mirror.adam(c.blob, np.zeros(g.size), np.zeros(g.size), np.ones(8, np.int64), g, lg.LR_TWO_STEP, c.H, c.A)[0]
    lo, err = lg.margin(c, blob=blob1.astype(np.float32), rows=tuple(x[c.idx[1]] for x in c.store))
    assert lo >= 4 * lg.MARGIN_FACTOR * err, (lo, err)


# ---- zero scales, and the scale bounds its sum

@pytest.mark.parametrize("sp", lg.GRID, ids=IDS)
def test_scales_bound_their_sums_and_zero_scales_are_exact_zeros(sp):
    c, ref, row64 = _reference(sp)
    assert (np.abs(row64) <= ref.S_row * (1 + 1e-12)).all() and (np.abs(ref.grad) <= ref.S_grad * (1 + 1e-12)).all()
    assert (row64[ref.S_row == 0] == 0).all() and (ref.grad[ref.S_grad == 0] == 0).all()
    o = mirror.layout(c.H, c.A)[1]
    if sp.n == 1:                                               # one term: the scale is the term (behind the actor's
        np.testing.assert_allclose(ref.S_row[o[2]:o[8]], np.abs(ref.sums[o[2]:]), rtol=1e-12, atol=0)   # layer 1, whose
        assert (ref.S_row[:o[2]] >= np.abs(ref.sums[:o[2]])).all()                # terms are sums over the logits)
    if sp.A == 1:                                               # onehot - p is exactly 0
        assert (ref.S_row[:o[4]] == 0).all() and (ref.S_grad[:o[4]] == 0).all()
    if sp.dead:                                                 # the actor's unit 0 and the critic's unit H - 1
        assert (ref.S_row[o[0]:o[0] + 12] == 0).all() and ref.S_row[o[1]] == 0 and ref.S_row[o[2]] == 0
        assert (ref.S_row[o[5] - 12:o[5]] == 0).all() and ref.S_row[o[6] - 1] == 0 and ref.S_row[o[7] - 1] == 0
    if (ref.S_row == 0).any():                                  # the comparator: anything but 0 there is infinite
        e = lg.errors(row64 + (ref.S_row == 0) * 1e-300, row64, ref.S_row, c.H, c.A)
        assert any(np.isinf(v) for v in e.values())
    assert not any(np.isinf(v) for v in lg.errors(row64, row64, ref.S_row, c.H, c.A).values())


# ---- the wrapper against the mirror's one-call forms

@pytest.mark.parametrize("sp", lg.GRID, ids=IDS)
def test_wrapper_is_the_existing_mirrors_where_they_overlap(sp):
    c, ref, row64 = _reference(sp)
    (s, a, r, s2), w, d = lg.batch_of(c)
    H, A, n = c.H, c.A, c.n
    close = lambda x, y: np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-12 * (1 + np.abs(y).max()))
    g = float(np.float32(lg.GAMMA))
    unclipped = ref.grad / np.concatenate([np.full(mirror.layout(H, A)[1][4], ref.coef[0]),
                                           np.full(ref.grad.size - mirror.layout(H, A)[1][4], ref.coef[1])])

    def same(row, lag):
        close(ref.sums, row["g"]); close(ref.loss4, row["loss"]); close(ref.td, row["td"])
        close(ref.actor_loss, lag[0]); close(ref.critic_loss, lag[1]); close(ref.td, lag[2]); close(unclipped, lag[3])
    args = (c.blob, H, A, s, a, r, s2)
    if sp.body == "plain":
        same(mirror.shard_sums(*args, g, c.loss), mirror.losses_and_grads(*args, g, c.loss))
        comb = mirror.combine([mirror.shard_sums(*args, g, c.loss)], H, A, c.loss)
        close(unclipped, comb[2])
    elif sp.body == "weighted":
        same(mirror.shard_sums(*args, g, c.loss, w), mirror.losses_and_grads(*args, g, c.loss, weights=w))
    elif sp.body in ("reg0", "regc"):
        same(mirror.shard_sums(*args, g, c.loss, None, c.c), mirror.losses_and_grads(*args, g, c.loss, entropy_coef=c.c))
        close(ref.entropy, mirror.policy(c.blob, H, A, s)[2])
    elif sp.body == "target":
        lag = mirror.losses_and_grads(*args, g, c.loss, theta=c.theta)
        close(ref.actor_loss, lag[0]); close(ref.critic_loss, lag[1]); close(ref.td, lag[2]); close(unclipped, lag[3])
    else:                                                       # discounts: the mirror on y folded by hand
        th = c.theta if c.theta is not None else mirror.critic_block(c.blob, H, A)
        y = np.asarray(r, np.float64) + np.asarray(d, np.float64) * mirror.values64(th, H, s2)
        same(mirror.shard_sums(c.blob, H, A, s, a, y, s2, 0.0, c.loss, w, c.c),
             mirror.losses_and_grads(c.blob, H, A, s, a, y, s2, 0.0, c.loss, weights=w, entropy_coef=c.c))
    if c.mgn:
        coef, _, clipped = mirror.clip_grad_norm(unclipped, H, A, c.mgn)
        close(ref.grad, clipped)
        assert (coef < 1).all() and abs(coef[0] - coef[1]) > 0.1 * coef.max()


# ---- the recovery

def test_recovery_round_trips_on_a_learner_gradient():
    """adam_element's first step in numpy float32 (csrc/adam.h) on a case's scaled gradient, and a second one."""
    c, ref, _ = _reference(lg.GRID[-2])
    g1 = ref.grad.astype(np.float32)
    m = np.float32(0.1) * g1
    v = np.float32(0.001) * g1 * g1
    got = pc.recovered_gradient(m, v)
    assert np.all(np.abs(got - g1.astype(np.float64)) <= 2.0 ** -23 * np.abs(g1.astype(np.float64)))
    with pytest.raises(AssertionError):
        pc.recovered_gradient(m, v * np.float32(1.001))
    g2 = (ref.grad[::-1] * 0.7).astype(np.float32)
    m_b = m + np.float32(0.1) * (g2 - m)
    got, bound = pc.second_step_gradient(m_b, m)
    assert np.all(np.abs(got - g2.astype(np.float64)) <= bound)


# ---- mutants

G32 = float(np.float32(lg.GAMMA))


def _backward(f, gz, gv, keep=slice(None), mask_c=None, no_unit=False, no_logit=False):
    """learner_mirror.backward with the rows of the sums, the critic's mask and the actor's dL/dh open to change."""
    s, ha, hc, pa, pc_, w2a, w2c = f.s, f.ha, f.hc, f.pa, f.pc, f.w2a, f.w2c
    A, H = w2a.shape
    g_w2a = gz[keep].T @ ha[keep]; g_b2a = gz[keep].sum(0)
    dha = (gz[:, :A - 1] @ w2a[:A - 1] if no_logit else gz @ w2a) * (pa > 0)
    if no_unit:
        dha[:, H - 1] = 0.0
    g_w1a = dha[keep].T @ s[keep]; g_b1a = dha[keep].sum(0)
    g_w2c = (gv[keep, None] * hc[keep]).sum(0)[None, :]; g_b2c = np.array([gv[keep].sum()])
    dhc = gv[:, None] * w2c * ((pc_ > 0) if mask_c is None else mask_c)
    g_w1c = dhc[keep].T @ s[keep]; g_b1c = dhc[keep].sum(0)
    return np.concatenate([g.ravel() for g in (g_w1a, g_b1a, g_w2a, g_b2a, g_w1c, g_b1c, g_w2c, g_b2c)])


def _mutant(c, kind):
    """(row words, scaled gradient) of the float64 update with one thing wrong."""
    H, A, n, R = c.H, c.A, c.n, lg.rows_per_tile(c.H)
    (s, a, r, s2), w, d = lg.batch_of(c)
    th = c.theta
    blob, cc = c.blob, c.c
    if kind == "gamma_for_discount":
        d = np.full(n, G32)
    if kind == "online_in_next":
        th = None
    if kind == "target_in_v":
        blob = mirror.with_critic(c.blob, H, A, c.theta)
    if kind == "entropy_sign":
        cc = -cc
    f = mirror.forward(blob, H, A, s, a, r, s2, d, th)
    gz, gv, lt, _ = mirror.terms(f, c.loss, w, cc)
    kw = {}
    keep = np.ones(n, bool)
    if kind in ("last_row", "row_R"):
        keep[n - 1 if kind == "last_row" else R] = False
    if kind == "revisited_tile":
        keep[256 * R:257 * R] = False
    if kind in ("last_row", "row_R", "revisited_tile"):
        kw["keep"] = keep
    if kind == "critic_mask_next":
        t64 = np.asarray(mirror.critic_block(c.blob, H, A) if th is None else th, np.float64)
        kw["mask_c"] = (np.asarray(s2, np.float64) @ t64[:12 * H].reshape(H, 12).T + t64[12 * H:13 * H]) > 0
    if kind == "no_unit":
        kw["no_unit"] = True
    if kind == "no_logit":
        kw["no_logit"] = True
    if kind == "unweighted_value":
        gv = f.v - f.target
    sums, loss4 = _backward(f, gz, gv, **kw), lt.sum(axis=1)
    md = lt[1][:R].sum() / R if kind == "first_tile_mean" else None
    return np.concatenate([sums, loss4]), lg._scaled(c, sums, loss4, n, md=md, swap=kind == "other_clip")[0]


ALL = lg.TENSORS
EVERY = lg.ROW_WORDS
_ORDINARY = [sp for sp in lg.GRID if sp.cls != "peaked"]


def _last_weight(sp, row):
    w = lg.build_case(sp).weights
    return w is None or w[0][row] > 0


def _cases(pred):
    return [sp for sp in _ORDINARY if pred(sp, lg.rows_per_tile(sp.H))]


# kind -> (the cases named for it, the words it can reach).  A row left out of the 65537-row case is 1.5e-5 of a typical
# element's S, near that batch's own sequential float32 wander, but the comparison is per element, and for the elements
# the row weighs most in it leaves the tolerance by 21: that case is named too.  Under a clip a wrong element moves its
# network's norm, and through the coefficient every element of that network, and a wrong scale is normalised away: the
# two clipped cases are named for the mutants that reach every tensor only.
MUTANTS = {
    "last_row": (_cases(lambda sp, R: sp.n > 2 and sp.n % R != 0 and sp.n != R + 1 and _last_weight(sp, -1)), ALL),
    "row_R": (_cases(lambda sp, R: sp.n == R + 1 and _last_weight(sp, R)), ALL),
    "revisited_tile": (_cases(lambda sp, R: sp.n in (256 * R + 1, 257 * R + 1)), ALL),
    "critic_mask_next": (_cases(lambda sp, R: sp.n >= 15 and not sp.mgn), lg.CRITIC[:2]),
    "no_unit": (_cases(lambda sp, R: sp.n >= 15 and sp.A >= 2 and not sp.mgn), lg.ACTOR[:2]),
    "no_logit": (_cases(lambda sp, R: sp.n >= 15 and sp.A >= 2 and not sp.mgn), lg.ACTOR[:2]),
    "unweighted_value": (_cases(lambda sp, R: sp.body in ("weighted", "discounted", "all")), lg.CRITIC),
    "gamma_for_discount": (_cases(lambda sp, R: sp.body in ("discounted", "all")), EVERY),
    "target_in_v": (_cases(lambda sp, R: sp.body in ("target", "all")), EVERY),
    "online_in_next": (_cases(lambda sp, R: sp.body in ("target", "all")), EVERY),
    "entropy_sign": ([sp for sp in lg.GRID if lg.build_case(sp).c > 0], lg.ACTOR + ("sum.actor",)),
    "first_tile_mean": (_cases(lambda sp, R: sp.loss == "reference" and sp.n > R and sp.A >= 2 and not sp.mgn), lg.ACTOR),
    "other_clip": (_cases(lambda sp, R: sp.mgn is not None), ALL),
}


def test_no_mutant_is_the_mirror():
    for sp in (lg.GRID[0], lg.GRID[40], lg.GRID[-2]):
        c, ref, row64 = _reference(sp)
        row, g = _mutant(c, None)
        np.testing.assert_array_equal(row, row64)
        np.testing.assert_array_equal(g, ref.grad)


def test_every_mutant_has_cases():
    assert all(len(cases) >= 2 for cases, _ in MUTANTS.values()), {k: len(v[0]) for k, v in MUTANTS.items()}


@pytest.mark.parametrize("kind,sp", [(k, sp) for k, (cases, _) in MUTANTS.items() for sp in cases],
                         ids=[f"{k}-{lg.spec_id(sp)}" for k, (cases, _) in MUTANTS.items() for sp in cases])
def test_mutant_fails(kind, sp):
    """The mutant leaves a tolerance, by MUTANT_ROOM, on at least one word it can reach (in the row or in the scaled
    gradient), and stays inside on every word it cannot."""
    c, ref, row64 = _reference(sp)
    row, g = _mutant(c, kind)
    rtol, gtol = lg.tolerances(sp)
    er = lg.errors(row, row64, ref.S_row, c.H, c.A)
    eg = lg.errors(g, ref.grad, ref.S_grad, c.H, c.A)
    reach = MUTANTS[kind][1]
    room = {("row", k): er[k] / rtol[k] for k in er if k in reach}
    room.update({("grad", k): eg[k] / gtol[k] for k in eg if k in reach})
    assert max(room.values()) > lg.MUTANT_ROOM, room
    for e, tol in ((er, rtol), (eg, gtol)):
        for k in e:
            if k not in reach:
                assert e[k] <= tol[k], (k, e[k], tol[k])


# ---- the forms: the clip, advantage and stored kernels (tests/learner_gradient_forms.py) ------------------------------

FORM_IDS = [lf.form_id(fs) for fs in lf.FORM_GRID]
assert len(set(FORM_IDS)) == len(FORM_IDS)
_FORM_REF = {}


def _form_reference(fs):
    """(case, float64 result with the CPU side's statistics, its row words) of a form case, computed once."""
    if fs not in _FORM_REF:
        c = lf.build_case(fs)
        ref = lf.fp64(c)
        _FORM_REF[fs] = (c, ref, np.concatenate([ref.sums, ref.loss4]))
    return _FORM_REF[fs]


def test_the_two_grids_reach_the_fourteen_kernels():
    """learner_grad_variant restated (kernel_name) is the table test_learner_variants_cpu.py pins; the form grid reaches
    the ten kernels the old grid does not, each from at least three cases, with and without an index vector; the old
    grid reaches the other four."""
    import test_learner_variants_cpu as tv
    for f in range(32):
        reg, target, log_mu, adv, stored = (bool(f >> b & 1) for b in range(5))
        want = tv.EXPECTED_STORED[target, log_mu] if stored else tv.EXPECTED[reg, target, log_mu, adv]
        assert lf.kernel_name(reg, target, log_mu, adv, stored) == want
    assert set(lf.NEW_KERNELS) | set(lf.OLD_KERNELS) == set(tv.INSTANTIATIONS) | set(tv.STORED_INSTANTIATIONS)
    assert {lf.kernel_of(sp) for sp in lg.GRID} == set(lf.OLD_KERNELS)
    mine = {k: [fs for fs in lf.FORM_GRID if lf.kernel_of(fs) == k] for k in lf.NEW_KERNELS}
    assert set(mine) == {lf.kernel_of(fs) for fs in lf.FORM_GRID} and len(mine) == 10
    for k, cases in mine.items():
        assert len(cases) >= 3 and {fs.gather for fs in cases} == {False, True}, k
        assert {(fs.H, fs.A, fs.n) for fs in cases} >= set(lf.POINTS), k
    assert {lf.kernel_of(fs) for fs in lf.FORM_TWO_STEP} == {"learner_grad_stored_clip_target_kernel"}


def test_the_form_grid_covers_what_it_names():
    R = lg.rows_per_tile
    for kernel in ("learner_grad_stored_clip_target_kernel", "learner_grad_clip_kernel"):
        mine = [fs for fs in lf.FORM_GRID if lf.kernel_of(fs) == kernel]
        assert {(fs.H, fs.n) for fs in mine} >= {(H, R(H) + 1) for H in lg.HS}
        for H in (200, 256):
            assert {fs.n for fs in mine if fs.H == H} >= {2, R(H) - 1, R(H), R(H) + 1, 2 * R(H) + 1, 256 * R(H) + 1}
    assert any(fs.n == 2 and fs.adv == "batch" and not fs.stored for fs in lf.FORM_GRID)
    assert {fs.A for fs in lf.FORM_GRID if (fs.H, fs.n) == (64, 65) and fs.stored and fs.clip} >= {1, 2, 48}
    assert any(fs.cls == "peaked" and fs.clip for fs in lf.FORM_GRID)
    assert sum(fs.inv0 for fs in lf.FORM_GRID) == 1 and all(fs.adv == "given" and fs.body == "weighted"
                                                           for fs in lf.FORM_GRID if fs.inv0)
    assert {fs.clip for fs in lf.FORM_GRID} == {None, lf.EPS, np.inf}
    assert {(fs.adv, fs.stored) for fs in lf.FORM_GRID} == {(m, s) for m in ("raw", "given", "batch") for s in (False, True)}
    big = {256 * R(H) + 1 for H in (200, 256)}
    assert max(fs.n for fs in lf.FORM_GRID if fs.n not in big) == 4113


@pytest.mark.parametrize("fs", lf.FORM_GRID, ids=FORM_IDS)
def test_form_case_conditions_and_fp32_references(fs):
    c, ref, row64 = _form_reference(fs)
    n, i = c.n, c.idx[0]
    lo, err = lg.margin(c)
    assert lo >= lg.MARGIN_FACTOR * err, (lo, err)
    assert np.abs(ref.td).min() >= lg.MIN_DELTA
    if fs.cls == "peaked":
        assert 30.0 < lg.logit_spread(c.blob, c.H, c.A, c.rows[0]) < 60.0
    # the stores: NaN outside the batch, the designed zeros
    for store in (c.log_mu, c.advantages):
        if store is not None:
            outside = np.setdiff1d(np.arange(c.cap), i)
            assert np.isnan(store[outside]).all() and np.isfinite(store[i]).all() and outside.size == c.cap - n
    zeros = ref.adv == 0
    if fs.inv0:
        assert zeros.all() and c.given[1] == 0 and c.c == 0
    elif fs.stored and fs.adv == "raw":
        x = c.advantages[i]
        assert zeros.sum() == -(-n // 16) + 1 and np.signbit(x[zeros]).sum() == 1 and np.signbit(x[1])
        assert 0.25 <= np.abs(x[~zeros]).min() and np.abs(x).max() <= 4
    else:
        assert not zeros.any()
    if fs.stored:
        assert 0.25 <= np.abs(c.advantages[i][~zeros]).min() and np.abs(c.advantages[i]).max() <= 4
    assert np.abs(ref.adv[~zeros]).min(initial=np.inf) >= lf.MIN_ADV
    # the two fp32 references: their advantage, ratio and gate against float64, then the comparator at half a tolerance
    rtol, gtol = lf.tolerances(fs)
    half = lambda tol: {k: v / 2 for k, v in tol.items()}
    ratio_err = 0.0
    for fn in (lg.torch_fp32, lg.sequential_fp32):
        seen = {}
        r, g = fn(c, lf.cpu_stats(c, ref), seen)
        assert lf.MIN_ADV >= 16 * np.abs(seen["adv"] - ref.adv).max(), fn.__name__
        if fs.clip is not None:
            np.testing.assert_array_equal(seen["pass"], ref.passes, fn.__name__)
            ratio_err = max(ratio_err, float(np.abs(seen["ratio"] - ref.ratio).max()))
            assert (np.abs(seen["ratio"] - ref.ratio) <= lf.ratio_tolerance(fs, ref.ratio) / 2).all(), fn.__name__
        er = lg.errors(r, row64, ref.S_row, c.H, c.A)
        eg = lg.errors(g, ref.grad, ref.S_grad, c.H, c.A)
        assert not lg.over(er, half(rtol)), (fn.__name__, lg.over(er, half(rtol)))
        assert not lg.over(eg, half(gtol)), (fn.__name__, lg.over(eg, half(gtol)))
    if fs.clip is not None:
        if np.isfinite(fs.clip):
            nearest = min(np.abs(ref.ratio - b).min() for b in mirror.bounds(fs.clip))
            assert nearest >= 16 * ratio_err, (nearest, ratio_err)
        else:
            assert ref.passes.all()
        cells = lf.cells(ref.ratio, ref.adv)
        if n >= 16 and fs.A >= 2 and not fs.inv0:               # (A = 1: log p = 0 and log_mu <= 0, no ratio below 1)
            assert min(cells) >= n // 8, cells
    if fs.adv == "batch" and not fs.stored and n >= 16:         # a gate that read delta's sign would show
        assert ((ref.adv >= 0) != (ref.td >= 0)).sum() >= n // 8
        assert (ref.td > 0).all()
    if fs.adv == "batch":
        src = c.advantages[i] if fs.stored else ref.td.astype(np.float32)
        np.testing.assert_array_equal(np.array(ref.stats), am.stats32(src)[:2])
        assert (np.sign(ref.adv) == lf.dealt_signs(n)).all()


@pytest.mark.parametrize("fs", lf.FORM_GRID, ids=FORM_IDS)
def test_form_results_against_the_stripped_case_and_the_existing_mirrors(fs):
    """The critic's four tensors, td, loss words 0, 1 and 3 and the critic loss are those of the same batch with the
    form stripped, to the bit; the scales bound their sums; without a store the sums are learner_advantage_mirror's
    shard_sums(given=) (clip=) for a normalised advantage and learner_mirror's shard_sums(clip=) for the raw one."""
    c, ref, row64 = _form_reference(fs)
    plain = lg.fp64(lf.stripped(c))
    o = mirror.layout(c.H, c.A)[1]
    np.testing.assert_array_equal(ref.sums[o[4]:], plain.sums[o[4]:])
    np.testing.assert_array_equal(ref.td, plain.td)
    np.testing.assert_array_equal(ref.loss4[[0, 1, 3]], plain.loss4[[0, 1, 3]])
    np.testing.assert_array_equal(ref.grad[o[4]:], plain.grad[o[4]:])
    assert ref.critic_loss == plain.critic_loss
    np.testing.assert_array_equal(ref.S_row[o[4]:o[8]], plain.S_row[o[4]:o[8]])
    assert (np.abs(row64) <= ref.S_row * (1 + 1e-12)).all() and (np.abs(ref.grad) <= ref.S_grad * (1 + 1e-12)).all()
    assert (row64[ref.S_row == 0] == 0).all() and (ref.grad[ref.S_grad == 0] == 0).all()
    if fs.A == 1 or fs.inv0:                                    # onehot - p is exactly 0; every advantage is +-0
        assert (ref.S_row[:o[4]] == 0).all() and (ref.S_grad[:o[4]] == 0).all()
        assert (ref.S_row[o[8] + 2] == 0) == fs.inv0            # (A = 1 has its surrogate: a loss and no gradient)
    if not fs.stored:
        (s, a, r, s2), w, d = lg.batch_of(c)
        clip = None if fs.clip is None else (c.log_mu[c.idx[0]], fs.clip)
        if fs.adv == "raw":
            row = mirror.shard_sums(c.blob, c.H, c.A, s, a, r, s2, d, "per_sample", w, c.c, clip, c.theta)
        else:
            row = am.shard_sums(c.blob, c.H, c.A, s, a, r, s2, d, w, c.c, clip, c.theta, ref.stats)
            np.testing.assert_array_equal(row["adv"], ref.adv)
        np.testing.assert_array_equal(row["g"], ref.sums)
        np.testing.assert_array_equal(row["loss"], ref.loss4)


@pytest.mark.parametrize("fs", lf.FORM_TWO_STEP, ids=[lf.form_id(fs) for fs in lf.FORM_TWO_STEP])
def test_form_two_step_cases_have_margin(fs):
    c = lf.build_two_step_case(fs)
    lo, err = lg.margin(c, rows=tuple(x[c.idx[0]] for x in c.store))
    assert lo >= lg.MARGIN_FACTOR * err
    g = lf.fp64(c, 0).grad
    blob1 = mirror.adam(c.blob, np.zeros(g.size), np.zeros(g.size), np.ones(8, np.int64), g, lg.LR_TWO_STEP, c.H, c.A)[0]
    lo, err = lg.margin(c, blob=blob1.astype(np.float32), rows=tuple(x[c.idx[1]] for x in c.store))
    assert lo >= 4 * lg.MARGIN_FACTOR * err, (lo, err)
    two = lf.fp64(c, 1, blob=blob1.astype(np.float32))
    assert min(lf.cells(two.ratio, two.adv)) >= c.n // 8
    nearest = min(np.abs(two.ratio - b).min() for b in mirror.bounds(fs.clip))
    assert nearest > 1e-2                                       # one Adam step at LR_TWO_STEP moves a ratio by < 1e-3


# ---- mutants of the forms

def _form_mutant(c, ref, kind):
    """(row words, scaled gradient) of a form case's float64 update with one thing wrong in the per-row block."""
    fs, n, R = c.form, c.n, lg.rows_per_tile(c.H)
    (s, a, r, s2), w, d = lg.batch_of(c)
    f = mirror.forward(c.blob, c.H, c.A, s, a, r, s2, d, c.theta)
    delta, i = f.delta, c.idx[0]
    iw = np.ones(n) if w is None else np.asarray(w, np.float64)
    lm = None if c.log_mu is None else c.log_mu[i].astype(np.float64)
    x = c.advantages[i].copy() if fs.stored else delta.astype(np.float32)
    if kind == "log_mu_by_row":
        lm = c.log_mu[:n].astype(np.float64)
    if kind == "advantages_by_row":
        x = c.advantages[:n].copy()
    if kind == "xa_is_lm":
        x = c.log_mu[i].copy()
    if kind == "stale_lm":
        lm[R - 1::R] = lm[R - 2::R][:len(lm[R - 1::R])]
    if kind == "stale_xa":
        x[R - 1::R] = x[R - 2::R][:len(x[R - 1::R])]
    if fs.adv == "raw":
        adv = x.astype(np.float64) if fs.stored or kind == "xa_is_lm" else delta
    elif kind == "scale_then_shift":
        adv = np.subtract(np.multiply(x, ref.stats[1], dtype=np.float32), ref.stats[0], dtype=np.float32).astype(np.float64)
    else:
        adv = am.standardise(x, *ref.stats).astype(np.float64)
    lp = f.logp[np.arange(n), f.a]
    with np.errstate(invalid="ignore"):
        if fs.clip is None:
            ok, dr = np.ones(n, bool), adv
            surr = lp * adv
        else:
            lo, hi = mirror.bounds(fs.clip)
            ratio = np.exp(lp - lm)
            side = (delta if kind == "gate_from_delta" else adv) >= 0
            ok, edge = np.where(side, ratio <= hi, ratio >= lo), np.where(side, hi, lo)
            dr = np.where(ok, adv if kind == "dr_without_ratio" else ratio * adv, 0.0)
            surr = np.where(ok, dr, edge * adv)
        k = np.where(ok, dr, edge * adv) if kind == "clipped_bound" else dr
        keep = ok if kind == "no_entropy_on_clipped" else np.ones(n, bool)
        eg = np.where(f.p > 0, f.p * (f.logp + f.entropy[:, None]), 0.0) * keep[:, None]
        gz = iw[:, None] * (k[:, None] * (f.onehot - f.p) - c.c * eg)
        gv = (-adv if kind == "advantage_in_gv" else f.v - f.target) * iw
        wl = np.where(ok, iw, 1.0) if kind == "unweighted_clipped_loss" else iw
        actor = wl * (-(dr if kind == "loss_from_dr" else surr) - c.c * f.entropy)
        lt = np.stack([-lp * iw, (adv if kind == "advantage_in_word1" else delta) * iw, actor, (f.v - f.target) ** 2 * iw])
    sums, loss4 = mirror.backward(f, gz, gv), lt.sum(axis=1)
    return np.concatenate([sums, loss4]), lg._scaled(c, sums, loss4, n)[0]


_FORMS = [fs for fs in lf.FORM_GRID if fs.cls != "peaked" and not fs.inv0 and fs.A >= 2]


def _forms(pred):
    return [fs for fs in _FORMS if pred(fs, lg.rows_per_tile(fs.H))]


def _finite(fs):
    return fs.clip is not None and np.isfinite(fs.clip)


def _weighs(fs, rows, passing=False):
    """Some of `rows` of the batch has a positive weight and a non-zero advantage (passing: and passes the gate, so that
    its ratio is in the gradient: another log_mu need not move a clipped row across its bound)."""
    c, ref, _ = _form_reference(fs)
    w = np.ones(c.n) if c.weights is None else c.weights[0]
    return bool(((w[rows] > 0) & (ref.adv[rows] != 0) & (ref.passes[rows] | (not passing))).any())


ACTOR_WORDS = lg.ACTOR + ("sum.actor",)
# kind -> (the cases named for it, the words it can reach); 15 rows and more: every gate cell is occupied
FORM_MUTANTS = {
    "gate_from_delta": (_forms(lambda fs, R: _finite(fs) and (fs.stored or fs.adv != "raw") and fs.n >= 15), ACTOR_WORDS),
    "dr_without_ratio": (_forms(lambda fs, R: fs.clip is not None), ACTOR_WORDS),
    "clipped_bound": (_forms(lambda fs, R: _finite(fs) and fs.n >= 15), lg.ACTOR),
    "log_mu_by_row": (_forms(lambda fs, R: fs.gather and fs.clip is not None), ACTOR_WORDS),
    "advantages_by_row": (_forms(lambda fs, R: fs.gather and fs.stored), ACTOR_WORDS),
    "xa_is_lm": (_forms(lambda fs, R: fs.stored and fs.clip is not None), ACTOR_WORDS),
    "stale_lm": (_forms(lambda fs, R: fs.clip is not None and fs.n >= R and
                        _weighs(fs, slice(R - 1, None, R), True)), ACTOR_WORDS),
    "stale_xa": (_forms(lambda fs, R: fs.stored and fs.n >= R and _weighs(fs, slice(R - 1, None, R))), ACTOR_WORDS),
    "scale_then_shift": (_forms(lambda fs, R: fs.adv != "raw"), ACTOR_WORDS),
    "advantage_in_gv": (_forms(lambda fs, R: fs.stored), lg.CRITIC),
    "advantage_in_word1": (_forms(lambda fs, R: fs.stored), ("sum.delta",)),
    "no_entropy_on_clipped": (_forms(lambda fs, R: _finite(fs) and fs.n >= 15 and fs.body in ("regc", "all")), lg.ACTOR),
    "unweighted_clipped_loss": (_forms(lambda fs, R: _finite(fs) and fs.n >= 15 and
                                       fs.body in ("weighted", "discounted", "all")), ("sum.actor",)),
    "loss_from_dr": (_forms(lambda fs, R: _finite(fs) and fs.n >= 15), ("sum.actor",)),
}


def test_no_form_mutant_is_the_mirror():
    for fs in (lf.FORM_GRID[0], lf.FORM_GRID[5], lf.FORM_GRID[13], lf.FORM_GRID[29], lf.FORM_GRID[-1]):
        c, ref, row64 = _form_reference(fs)
        row, g = _form_mutant(c, ref, None)
        np.testing.assert_array_equal(row, row64)
        np.testing.assert_array_equal(g, ref.grad)


@pytest.mark.parametrize("kind", list(FORM_MUTANTS))
def test_form_mutant_fails(kind):
    """On every case named for it the mutant leaves a tolerance, by MUTANT_ROOM, on a word it can reach (a NaN from a
    slot outside the batch counts as leaving it), and stays inside on every word it cannot.  Prints the least excess."""
    cases, reach = FORM_MUTANTS[kind]
    assert len(cases) >= 3, len(cases)
    least = (np.inf, None)
    for fs in cases:
        c, ref, row64 = _form_reference(fs)
        row, g = _form_mutant(c, ref, kind)
        rtol, gtol = lf.tolerances(fs)
        er = lg.errors(np.nan_to_num(row, nan=np.inf), row64, ref.S_row, c.H, c.A)
        eg = lg.errors(np.nan_to_num(g, nan=np.inf), ref.grad, ref.S_grad, c.H, c.A)
        room = {("row", k): er[k] / rtol[k] for k in er if k in reach}
        room.update({("grad", k): eg[k] / gtol[k] for k in eg if k in reach})
        assert max(room.values()) > lg.MUTANT_ROOM, (lf.form_id(fs), room)
        least = min(least, (max(room.values()), lf.form_id(fs)), key=lambda x: x[0])
        for e, tol in ((er, rtol), (eg, gtol)):
            for k in e:
                if k not in reach:
                    assert e[k] <= tol[k], (lf.form_id(fs), k, e[k], tol[k])
    print(f"{kind}: {len(cases)} cases, least excess {least[0]:.3g} tolerances ({least[1]})")


def test_a_stored_advantage_in_td_would_show():
    """td_delta is judged at 2e-5 of max |delta| (learner_harness.assert_losses_and_td); in every stored case the
    advantage is further than a hundred such bounds from delta in some row."""
    for fs in lf.FORM_GRID:
        if fs.stored:
            c, ref, _ = _form_reference(fs)
            assert np.abs(ref.adv - ref.td).max() > 100 * 2e-5 * np.abs(ref.td).max()
