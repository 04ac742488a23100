"""The gradient comparison of tests/learner_gradient_cases.py without a GPU: every case meets its margin condition, both
fp32 CPU references (torch autograd, the strictly sequential float32 sum) pass the comparator with a factor of two to
spare, the wrapper's float64 sums are the mirror's one-call forms' wherever they overlap, the recovery of a gradient from
Adam's first moments round-trips, and wrong backward passes (mutants: changed copies of the float64 backward, held here
and never in the library) fail where they must and only there."""
import numpy as np
import pytest

import learner_gradient_cases as lg
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
