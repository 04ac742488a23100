"""The gradient comparison of tests/pmi_gradient_cases.py without a GPU: every case meets its margin condition, the fp32
torch CPU autograd of the same step passes the comparator at the tolerance of the case's class, wrong backward passes
(mutants: changed copies of the mirror's backward, held here and never in the library) fail it where they must and only
there, and the recovery of a gradient from Adam's first moments round-trips."""
import numpy as np
import pytest

import pmi_gradient_cases as pc
import pmi_trainer_mirror as mirror

ALL = tuple(mirror.param_names())
BRANCH_DATA = tuple(n + s for lin, bn, _, _ in mirror.BRANCHES for n, s in ((lin, ".weight"), (bn, ".weight"), (bn, ".bias")))
DATA = tuple(k for k in ALL if k not in pc.PRE_BN_BIAS)
# what a wrong factor in front of a BatchNorm backward's dz reaches: everything upstream of a BatchNorm
BEHIND_BN = BRANCH_DATA + ("fc1.weight",)
LARGE = [c for c in pc.GRID if c[1] >= 63]


def _ids(cases):
    return [f"H{H}-B{B}" for H, B in cases]


_REF = {}


def _reference(H, B):
    """(case, float64 gradients, scales) of a grid case, computed once."""
    if (H, B) not in _REF:
        c = pc.build_case(H, B)
        _REF[(H, B)] = (c, mirror.loss_and_grads(c.sd, c.x12, c.x13)[3], pc.gradient_scales(c.sd, c.x12, c.x13))
    return _REF[(H, B)]


@pytest.mark.parametrize("H,B", pc.GRID, ids=_ids(pc.GRID))
def test_reference_passes(H, B):
    """The case's margin condition, and the fp32 torch CPU gradients inside the class's tolerance on every tensor."""
    c, g64, S = _reference(H, B)
    err = pc.fp32_forward_error(c.sd, c.x12, c.x13)
    assert c.min_abs_y >= pc.MARGIN_FACTOR * err, (c.min_abs_y, err)
    e = pc.gradient_errors(pc.torch_fp32_gradients(c.sd, c.x12, c.x13), g64, S)
    tol = pc.tolerance(B)
    over = {k: (v, tol[k]) for k, v in e.items() if not v <= tol[k]}
    assert not over, over


@pytest.mark.parametrize("H,B", pc.TWO_STEP, ids=_ids(pc.TWO_STEP))
def test_two_step_cases_have_margin(H, B):
    """Both steps' margins, the second at the mirror's parameters after step one (the GPU test asserts it again at the
    device's)."""
    c = pc.build_two_step_case(H, B)
    for sd, b in ((c.sd, c.b1), (c.sd1, c.b2)):
        assert pc.min_abs_y(sd, b) >= pc.MARGIN_FACTOR * pc.fp32_forward_error(sd, *b)


# ---- mutants

def _mutant_bn_backward(dy, xh, inv, gamma, kind, rows):
    n = dy.shape[0]
    if kind == "unbiased_var":                                   # inv from var n / (n - 1): var = 1 / inv^2 - eps
        inv = 1.0 / np.sqrt((1.0 / inv ** 2 - mirror.EPS) * n / (n - 1) + mirror.EPS)
    proj = 0.0 if kind == "no_xh_term" else xh * (dy * xh).sum(0) / n
    dz = gamma * inv * (dy - dy.sum(0) / n - proj)
    return dz, (dy * xh)[rows].sum(0), dy[rows].sum(0)


def _mutant_backward(sd, cache, d_out, grads, kind, side, inv_of):
    """mirror.backward with one thing wrong.  inv_of: the cache whose inv this side normalises with."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    H = g("fc2.weight").shape[1]
    a0, a1 = cache["a0"], cache["a1"]
    rows = slice(0, len(d_out) - 1) if (kind == "drop_last_row" and side == 1) else slice(None)
    grads["fc2.weight"] += (d_out[rows] @ a1[rows])[None, :]
    grads["fc2.bias"] += d_out[rows].sum(keepdims=True)
    xh1, y1, _ = cache["bn1"]
    dy1 = np.outer(d_out, g("fc2.weight")[0]) * (y1 > 0)
    dz1, dg1, db1 = _mutant_bn_backward(dy1, xh1, inv_of["bn1"][2], g("bn1.weight"), kind, rows)
    grads["bn1.weight"] += dg1
    grads["bn1.bias"] += db1
    grads["fc1.weight"] += dz1[rows].T @ a0[rows]
    grads["fc1.bias"] += dz1[rows].sum(0)
    W1 = g("fc1.weight")
    da0 = dz1[:, :H - 1] @ W1[:H - 1] if kind == "da0_short" else dz1 @ W1
    for j, (lin, bn, a, b) in enumerate(mirror.BRANCHES):
        xh, y, _ = cache[bn]
        dy = da0[:, j * H:(j + 1) * H] * (y > 0)
        dz, dgam, dbet = _mutant_bn_backward(dy, xh, inv_of[bn][2], g(bn + ".weight"), kind, rows)
        grads[bn + ".weight"] += dgam
        grads[bn + ".bias"] += dbet
        grads[lin + ".weight"] += dz[rows].T @ cache["x"][rows, a:b]
        grads[lin + ".bias"] += dz[rows].sum(0)


def _mutant_grads(sd, x12, x13, kind):
    o12, c12, _ = mirror.forward(sd, x12)
    o13, c13, _ = mirror.forward(sd, x13)
    n = x12.shape[0]
    if kind == "fc2_first_32":                                   # the features c >= 32 left out of fc2's forward sum
        w2, b2 = np.asarray(sd["fc2.weight"], np.float64)[0], float(np.asarray(sd["fc2.bias"])[0])
        o12, o13 = c12["a1"][:, :32] @ w2[:32] + b2, c13["a1"][:, :32] @ w2[:32] + b2
    div = 2 * n if kind == "half_d_out" else n
    grads = {k: np.zeros_like(np.asarray(sd[k], dtype=np.float64)) for k in mirror.param_names()}
    _mutant_backward(sd, c12, -mirror.sigmoid(-o12) / div, grads, kind, 0, c12)
    _mutant_backward(sd, c13, mirror.sigmoid(o13) / div, grads, kind, 1, c12 if kind == "other_sides_inv" else c13)
    return grads


def _cases(pred):
    return [c for c in pc.GRID if pred(*c)]


# kind -> (the cases named for it, the tensors it can reach); the three the issue names no cases for run on every
# case of the B >= 63 class
MUTANTS = {
    "unbiased_var": (_cases(lambda H, B: B in (512, 513)), BEHIND_BN),
    "no_xh_term": (LARGE, BEHIND_BN),
    "drop_last_row": (_cases(lambda H, B: B in (65, 129, 513)), ALL),
    "other_sides_inv": (LARGE, BEHIND_BN),
    "half_d_out": (LARGE, DATA),
    "fc2_first_32": (_cases(lambda H, B: H == 33), DATA),
    "da0_short": (_cases(lambda H, B: H in (17, 43)), BRANCH_DATA),
}


def test_no_mutant_is_the_mirror():
    c, g64, S = _reference(17, 65)
    g = _mutant_grads(c.sd, c.x12, c.x13, None)
    for k in ALL:
        np.testing.assert_array_equal(g[k], g64[k])


@pytest.mark.parametrize("kind,H,B", [(k, H, B) for k, (cases, _) in MUTANTS.items() for H, B in cases],
                         ids=[f"{k}-H{H}-B{B}" for k, (cases, _) in MUTANTS.items() for H, B in cases])
def test_mutant_fails(kind, H, B):
    """The mutant leaves the tolerance, by MUTANT_ROOM, on at least one tensor it can reach, and stays inside it on
    every tensor it cannot."""
    c, g64, S = _reference(H, B)
    e = pc.gradient_errors(_mutant_grads(c.sd, c.x12, c.x13, kind), g64, S)
    tol = pc.tolerance(B)
    reach = MUTANTS[kind][1]
    room = {k: e[k] / tol[k] for k in reach}
    assert max(room.values()) > pc.MUTANT_ROOM, room
    for k in ALL:
        if k not in reach:
            assert e[k] <= tol[k], (k, e[k], tol[k])


# ---- the recovery

def _adam_first_step_f32(g):
    """adam_element's moments after one step from zero state, in numpy float32 (csrc/adam.h)."""
    g = g.astype(np.float32)
    m = np.float32(0.0) + np.float32(0.1) * (g - np.float32(0.0))
    v = np.float32(0.0) * np.float32(0.999) + np.float32(0.001) * g * g
    assert m.dtype == np.float32 and v.dtype == np.float32
    return m, v


def test_recovery_round_trips():
    rng = np.random.RandomState(0)
    g = (10.0 ** rng.uniform(-12, 3, size=20000) * rng.choice([-1.0, 1.0], size=20000)).astype(np.float32)
    m, v = _adam_first_step_f32(g)
    got = pc.recovered_gradient(m, v)
    assert np.all(np.abs(got - g.astype(np.float64)) <= 2.0 ** -23 * np.abs(g.astype(np.float64)))
    with pytest.raises(AssertionError):                          # a second moment that is not this gradient's
        pc.recovered_gradient(m, v * np.float32(1.001))


def test_second_step_recovery_bound():
    """m after two float32 Adam steps gives back the second gradient within second_step_gradient's own bound."""
    rng = np.random.RandomState(1)
    g1 = (10.0 ** rng.uniform(-8, 1, size=20000) * rng.choice([-1.0, 1.0], size=20000)).astype(np.float32)
    g2 = (10.0 ** rng.uniform(-8, 1, size=20000) * rng.choice([-1.0, 1.0], size=20000)).astype(np.float32)
    m_a = _adam_first_step_f32(g1)[0]
    m_b = m_a + np.float32(0.1) * (g2 - m_a)
    got, bound = pc.second_step_gradient(m_b, m_a)
    assert np.all(np.abs(got - g2.astype(np.float64)) <= bound)
