"""Cases, error scales and the comparator for the device PMI trainer's gradients, element by element against the
float64 mirror (tests/pmi_trainer_mirror.py).  Plain numpy and torch on the CPU; used by test_pmi_gradients_cpu.py (no
GPU) and test_hip_pmi_gradients.py.

Reading a gradient off the device.  A fresh trainer has zero moments and step counts, so after ONE mini-batch
adam_element (csrc/adam.h) has left exp_avg = fl(0.1f g) and exp_avg_sq = fl(fl(0.001f g) g): `recovered_gradient`
returns g = exp_avg / float32(0.1) in float64, one fp32 rounding from the gradient the kernels wrote.

The metric.  For every gradient element `gradient_scales` returns S, the float64 sum of the absolute values of the
terms of that element's defining sum over both sides (sum |dz_n| |x_n| for a Linear weight, sum |dz_n| for a Linear
bias, sum |dy_n xh_n| and sum |dy_n| for a BatchNorm weight and bias, sum |d_out_n| |a1_n| and sum |d_out_n| for fc2).
`gradient_errors` is max over the tensor of |g - g_fp64| / S.  An fp32 sum of n terms is off by about eps32 S however
the terms cancel, so the pre-BatchNorm biases (analytic gradient zero, computed value rounding noise) are compared like
every other tensor.

No ReLU knife edges.  A pre-ReLU value within the fp32 forward error of zero can fall on the other side on the device,
which changes one term of B in that feature's sums and everything upstream.  BatchNorm's bias does not enter the batch
statistics, so `build_case` moves every BatchNorm bias into the middle of the widest gap, near the present threshold,
of that column's 2B values (both sides share the bias): first the three branches, then, after a new forward, bn1.  The
cases' own condition, asserted for every case (`fp32_forward_error`): the smallest |y| over the four BatchNorm layers
and both sides is at least MARGIN_FACTOR = 16 times the largest |y_fp32 - y_fp64| of the fp32 torch CPU forward.

Parameters: make_pmi_net(H) under torch.manual_seed(H + B); BatchNorm weights then drawn from +-[0.5, 1.5] (a quarter
negative) and the running statistics away from (0, 1), so that a kernel which ignored any of them would show.  Rows are
those of test_hip_pmi_trainer._history (40 timesteps of 10 UAVs), triples from RandomState(H * 1000 + B).

Tolerances.  Two classes, B >= 63 and B <= 5 (with few rows a normalised value is d / sqrt(d^2 + eps) and roundings grow
by up to 1 / sqrt(eps)).  The reference for a tolerance is the fp32 torch CPU autograd of the same step
(`torch_fp32_gradients`), never the device: WORST holds, per class and tensor, its largest error over the grid in the
metric above, and the tolerance is TOL_FACTOR = 4 times that -- the device adds in another order (an xor butterfly over
lanes, 128-element GEMM slices), and reordering an fp32 sum of this length moves it by a small multiple of the same
eps32 S.  Measured (x86-64, torch CPU), worst over the class's cases:

    tensor                      B >= 63   tolerance    B <= 5   tolerance
    fc_comm.weight             5.04e-07   2.02e-06   3.05e-03   1.22e-02
    fc_comm.bias               5.57e-08   2.23e-07   6.21e-04   2.48e-03
    bn_comm.weight             4.36e-07   1.74e-06   3.01e-04   1.20e-03
    bn_comm.bias               4.35e-07   1.74e-06   3.01e-04   1.20e-03
    fc_obs.weight              4.67e-07   1.87e-06   3.35e-03   1.34e-02
    fc_obs.bias                9.39e-08   3.76e-07   6.64e-04   2.66e-03
    bn_obs.weight              5.17e-07   2.07e-06   3.21e-04   1.28e-03
    bn_obs.bias                4.42e-07   1.77e-06   3.21e-04   1.28e-03
    fc_boundary_state.weight   4.15e-07   1.66e-06   4.99e-02   2.00e-01
    fc_boundary_state.bias     8.04e-08   3.22e-07   2.08e-02   8.32e-02
    bn_boundary_state.weight   3.99e-07   1.60e-06   3.92e-03   1.57e-02
    bn_boundary_state.bias     3.85e-07   1.54e-06   3.92e-03   1.57e-02
    fc1.weight                 1.11e-06   4.44e-06   1.57e-03   6.28e-03
    fc1.bias                   5.27e-07   2.11e-06   3.85e-04   1.54e-03
    bn1.weight                 2.87e-07   1.15e-06   2.66e-06   1.06e-05
    bn1.bias                   9.91e-08   3.96e-07   1.94e-07   7.76e-07
    fc2.weight                 4.28e-07   1.71e-06   3.56e-06   1.42e-05
    fc2.bias                   7.74e-08   3.10e-07   8.41e-08   3.36e-07

The weakest mutant of test_pmi_gradients_cpu.py must exceed MUTANT_ROOM = 2 times a tolerance somewhere: a device with that error
plus rounding of its own, which is at most the tolerance, is then still outside.

A second step.  `build_two_step_case` draws 2B triples; trainer A takes the first B, trainer B all of them in one call.
The second step's gradient is (m_B - (1 - 0.1f) m_A) / 0.1f in float64 (`second_step_gradient`), compared with the
mirror at A's device parameters on the second B triples; the margin construction is applied to the union of the first
batch's values and the second batch's values at the mirror's parameters after one step, shifted by the bias' own Adam
move, and checked again at the device's parameters by the GPU test."""
import functools
import types

import numpy as np

import pmi_trainer_mirror as mirror

T_STEPS, N_UAV = 40, 10
LR = 1e-3
MARGIN_FACTOR = 16.0
TOL_FACTOR = 4.0
MUTANT_ROOM = 2.0
BN = ("bn_comm", "bn_obs", "bn_boundary_state", "bn1")
PRE_BN_BIAS = ("fc_comm.bias", "fc_obs.bias", "fc_boundary_state.bias", "fc1.bias")

_BS = (2, 3, 5, 63, 64, 65, 127, 128, 129, 512, 513)
_HS = (1, 15, 16, 17, 32, 33, 43, 128, 200, 256)
GRID = sorted(set([(H, B) for H in (17, 43) for B in _BS] + [(H, B) for H in _HS for B in (5, 65)]
                  + [(1, 2), (256, 513), (128, 128)]))
TWO_STEP = [(17, 65), (43, 129), (200, 5)]

F32 = np.float32
U32 = 2.0 ** -24                         # unit roundoff of fp32
B1F, B2F = float(F32(0.1)), float(F32(0.001))     # adam_element's 1 - beta as it holds them


def case_class(B):
    return "large" if B >= 63 else "small"


# ---- the recovery

def recovered_gradient(exp_avg, exp_avg_sq):
    """The gradient of the one Adam step that led from zero state to (exp_avg, exp_avg_sq), in float64.
    exp_avg = g (1 + d1) 0.1f, so g' = exp_avg / 0.1f = g (1 + d1); exp_avg_sq = 0.001f g^2 (1 + d2)(1 + d3), each
    |d| <= 2^-24: against 0.001f g'^2 = 0.001f g^2 (1 + d1)^2 that is a relative 4 x 2^-24 to first order (5 allowed
    for the second-order terms), plus 2^-126 absolute where the product leaves the normal range."""
    m, v = np.asarray(exp_avg, np.float64), np.asarray(exp_avg_sq, np.float64)
    g = m / B1F
    want = B2F * g * g
    bad = np.abs(v - want) > 5 * U32 * want + 2.0 ** -126
    assert not bad.any(), ("exp_avg_sq is not 0.001f g^2 of the recovered g", int(bad.sum()),
                           float(np.max(np.abs(v - want) / (want + 2.0 ** -126))))
    return g


def second_step_gradient(m_b, m_a):
    """(gradient of the second step, its recovery error bound) from exp_avg after two steps (m_b) and after the first
    alone (m_a).  m_b = fl(m_a + fl(0.1f fl(g - m_a))), fused or not: the inner roundings are each at most
    2^-24 |g - m_a| 0.1f and the outer 2^-24 |m_b|; divided by 0.1f that is 2^-24 (10 |m_b| + 2 |g - m_a|)
    <= 2^-24 (11 |m_a| + 3 |g|), about ten fp32 roundings of |m_a|."""
    m_b, m_a = np.asarray(m_b, np.float64), np.asarray(m_a, np.float64)
    g = (m_b - (1.0 - B1F) * m_a) / B1F
    return g, U32 * (11.0 * np.abs(m_a) + 3.0 * np.abs(g))


def split_params(flat, H):
    """A flat [P] array in parameters() order -> {name: array of the parameter's shape}."""
    shapes = param_shapes(H)
    out, o = {}, 0
    for k in mirror.param_names():
        n = int(np.prod(shapes[k]))
        out[k] = np.asarray(flat[o:o + n]).reshape(shapes[k])
        o += n
    assert o == len(flat)
    return out


def param_shapes(H):
    s = {}
    for (lin, bn, a, b) in mirror.BRANCHES:
        s[lin + ".weight"], s[lin + ".bias"], s[bn + ".weight"], s[bn + ".bias"] = (H, b - a), (H,), (H,), (H,)
    s["fc1.weight"], s["fc1.bias"], s["bn1.weight"], s["bn1.bias"] = (H, 3 * H), (H,), (H,), (H,)
    s["fc2.weight"], s["fc2.bias"] = (1, H), (1,)
    return s


# ---- the error scale and the comparator

def _add_scales(sd, cache, d_out, S):
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    H = g("fc2.weight").shape[1]
    a0, a1 = cache["a0"], cache["a1"]
    S["fc2.weight"] += (np.abs(d_out) @ np.abs(a1))[None, :]
    S["fc2.bias"] += np.abs(d_out).sum(keepdims=True)
    xh1, y1, inv1 = cache["bn1"]
    dy1 = np.outer(d_out, g("fc2.weight")[0]) * (y1 > 0)
    dz1 = mirror._bn_backward(dy1, xh1, inv1, g("bn1.weight"))[0]
    S["bn1.weight"] += np.abs(dy1 * xh1).sum(0)
    S["bn1.bias"] += np.abs(dy1).sum(0)
    S["fc1.weight"] += np.abs(dz1).T @ np.abs(a0)
    S["fc1.bias"] += np.abs(dz1).sum(0)
    da0 = dz1 @ g("fc1.weight")
    for j, (lin, bn, a, b) in enumerate(mirror.BRANCHES):
        xh, y, inv = cache[bn]
        dy = da0[:, j * H:(j + 1) * H] * (y > 0)
        dz = mirror._bn_backward(dy, xh, inv, g(bn + ".weight"))[0]
        S[bn + ".weight"] += np.abs(dy * xh).sum(0)
        S[bn + ".bias"] += np.abs(dy).sum(0)
        S[lin + ".weight"] += np.abs(dz).T @ np.abs(cache["x"][:, a:b])
        S[lin + ".bias"] += np.abs(dz).sum(0)


def gradient_scales(sd, x12, x13):
    """{param name: S}, S shaped like the parameter: the float64 sum of |term| of each gradient element's defining sum
    over both sides of the step mirror.loss_and_grads(sd, x12, x13) takes."""
    o12, c12, _ = mirror.forward(sd, x12)
    o13, c13, _ = mirror.forward(sd, x13)
    n = x12.shape[0]
    S = {k: np.zeros_like(np.asarray(sd[k], dtype=np.float64)) for k in mirror.param_names()}
    _add_scales(sd, c12, -mirror.sigmoid(-o12) / n, S)
    _add_scales(sd, c13, mirror.sigmoid(o13) / n, S)
    return S


def gradient_errors(got, ref, S, slack=None):
    """{param name: max over the tensor of max(|got - ref| - slack, 0) / S}.  An element whose S is zero has no
    nonzero term: there any difference is infinite."""
    out = {}
    for k in mirror.param_names():
        d = np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64))
        if slack is not None:
            d = np.maximum(d - slack[k], 0.0)
        s = np.asarray(S[k], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))
        out[k] = float(e.max())
    return out


# ---- the cases

def _initial_state(H, B, rng):
    import torch
    import uavtrack
    torch.manual_seed(H + B)
    sd = {k: v.numpy().copy() for k, v in uavtrack.make_pmi_net(H).state_dict().items()}
    for bn in BN:
        sign = np.where(rng.uniform(size=H) < 0.25, -1.0, 1.0)
        sd[bn + ".weight"] = (sign * rng.uniform(0.5, 1.5, size=H)).astype(F32)
        sd[bn + ".running_mean"] = rng.normal(0.0, 0.5, size=H).astype(F32)
        sd[bn + ".running_var"] = rng.uniform(0.5, 2.0, size=H).astype(F32)
        sd[bn + ".num_batches_tracked"] = np.int64(3)
    return sd


def _pre_relu(sd, batches):
    """{bn: [y [2B, H] of each batch]} from the mirror's forward of both sides."""
    out = {bn: [] for bn in BN}
    for x12, x13 in batches:
        c12, c13 = mirror.forward(sd, x12)[1], mirror.forward(sd, x13)[1]
        for bn in BN:
            out[bn].append(np.concatenate([c12[bn][1], c13[bn][1]], axis=0))
    return out


def _widest_gap_threshold(v, tau):
    """The middle of the widest gap between neighbours of the sorted values v, among the gaps whose both ends lie
    within max(2, len(v) // 8) places of where tau sorts in."""
    v = np.sort(v)
    pos = int(np.searchsorted(v, tau))
    w = max(2, len(v) // 8)
    lo, hi = max(0, pos - w), min(len(v), pos + w)
    if hi - lo < 2:
        lo, hi = max(0, min(lo, len(v) - 2)), min(len(v), max(hi, 2))
    gaps = np.diff(v[lo:hi])
    i = int(np.argmax(gaps))
    return 0.5 * (v[lo + i] + v[lo + i + 1])


def _place(sd, layers, evals):
    """Moves the BatchNorm bias of every feature of `layers` so that zero falls into the widest gap of the column's
    pre-ReLU values.  evals: [(state, batch, {bn: bias move})]: the values of `batch` under `state`, whose bias is
    sd's plus the move (a later step's parameters)."""
    ys = [(_pre_relu(st, [batch]), st, mv) for st, batch, mv in evals]
    for bn in layers:
        beta = np.asarray(sd[bn + ".bias"], np.float64)
        # y = v + beta_state = v + beta + move > 0  <=>  v + move > -beta
        cols = np.concatenate([y[bn][0] - np.asarray(st[bn + ".bias"], np.float64) + mv[bn] for y, st, mv in ys], axis=0)
        new = np.array([-_widest_gap_threshold(cols[:, c], -beta[c]) for c in range(cols.shape[1])])
        sd[bn + ".bias"] = new.astype(F32)


def min_abs_y(sd, batch):
    y = _pre_relu(sd, [batch])
    return min(float(np.abs(y[bn][0]).min()) for bn in BN)


def _rows_and_triples(H, B, n):
    from test_hip_pmi_trainer import _history
    rng = np.random.RandomState(H * 1000 + B)
    rows = _history(rng, T_STEPS, N_UAV)
    t, u = rng.randint(0, T_STEPS, size=n), rng.randint(0, N_UAV, size=(n, 2))
    return rng, rows, t, u


@functools.lru_cache(maxsize=None)
def build_case(H, B):
    """One mini-batch of B triples at hidden width H: rows, t, u, the state (fp32 arrays, reference keys), the gathered
    float64 batch (x12, x13) and min_abs_y, the smallest |pre-ReLU value| of the case."""
    rng, rows, t, u = _rows_and_triples(H, B, B)
    sd = _initial_state(H, B, rng)
    batch = mirror.gather(rows, N_UAV, t, u)
    _place(sd, BN[:3], [(sd, batch, {bn: 0.0 for bn in BN})])
    _place(sd, BN[3:], [(sd, batch, {bn: 0.0 for bn in BN})])
    return types.SimpleNamespace(H=H, B=B, rows=rows, t=t, u=u, sd=sd, x12=batch[0], x13=batch[1],
                                 min_abs_y=min_abs_y(sd, batch))


def mirror_step(sd, rows, t, u, B):
    """The mirror's state after one call on the triples, as the fp32 arrays a device would hold."""
    msd = mirror.train_pmi(sd, mirror.new_adam(), rows, N_UAV, t, u, B, lr=LR)[0]
    return {k: (np.asarray(v, np.float64).astype(F32) if not k.endswith("num_batches_tracked") else np.int64(v))
            for k, v in msd.items()}


@functools.lru_cache(maxsize=None)
def build_two_step_case(H, B):
    """2B triples: the first B are step one, the second B step two.  sd is the initial state; sd1 the mirror's after
    step one; min_abs_y the smaller of step one's margin at sd and step two's at sd1."""
    rng, rows, t, u = _rows_and_triples(H, B, 2 * B)
    sd = _initial_state(H, B, rng)
    b1 = mirror.gather(rows, N_UAV, t[:B], u[:B])
    b2 = mirror.gather(rows, N_UAV, t[B:], u[B:])
    zero = {bn: 0.0 for bn in BN}
    for _ in range(10):
        for layers in (BN[:3], BN[3:]):
            sd1 = mirror_step(sd, rows, t[:B], u[:B], B)
            move = {bn: np.asarray(sd1[bn + ".bias"], np.float64) - np.asarray(sd[bn + ".bias"], np.float64)
                    for bn in BN}
            _place(sd, layers, [(sd, b1, zero), (sd1, b2, move)])
        sd1 = mirror_step(sd, rows, t[:B], u[:B], B)
        m = min(min_abs_y(sd, b1), min_abs_y(sd1, b2))
        if m >= 4 * MARGIN_FACTOR * max(fp32_forward_error(sd, *b1), fp32_forward_error(sd1, *b2)):
            break
    else:
        raise AssertionError(("no margin for the two-step case", H, B, m))
    return types.SimpleNamespace(H=H, B=B, rows=rows, t=t, u=u, sd=sd, sd1=sd1, b1=b1, b2=b2, min_abs_y=m)


# ---- the fp32 torch reference

def _torch_net(sd, H):
    import torch
    import uavtrack
    net = uavtrack.make_pmi_net(H).train()
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return net


def fp32_forward_error(sd, x12, x13):
    """The largest |y_fp32 - y_fp64| over the four BatchNorm outputs and both sides: the fp32 torch CPU train-mode
    forward (forward hooks on make_pmi_net(H).train()) against the mirror."""
    import torch
    H = np.asarray(sd["fc2.weight"]).shape[1]
    net = _torch_net(sd, H)
    got = {bn: [] for bn in BN}
    hooks = [getattr(net, bn).register_forward_hook(lambda mod, inp, out, bn=bn: got[bn].append(out.detach().numpy()))
             for bn in BN]
    with torch.no_grad():
        for x in (x12, x13):
            net(torch.from_numpy(np.asarray(x, F32)))
    for h in hooks:
        h.remove()
    ref = _pre_relu(sd, [(x12, x13)])
    return max(float(np.abs(np.concatenate(got[bn], axis=0).astype(np.float64) - ref[bn][0]).max()) for bn in BN)


def torch_fp32_gradients(sd, x12, x13):
    """{param name: gradient} of pmi_contrastive_loss of two train-mode forwards, fp32 torch autograd on the CPU."""
    import torch
    import uavtrack
    H = np.asarray(sd["fc2.weight"]).shape[1]
    net = _torch_net(sd, H)
    o1 = net(torch.from_numpy(np.asarray(x12, F32)))
    o2 = net(torch.from_numpy(np.asarray(x13, F32)))
    uavtrack.pmi_contrastive_loss(o1, o2).backward()
    return {k: p.grad.numpy().astype(np.float64) for k, p in net.named_parameters()}


# ---- tolerances: WORST[class][tensor] is the fp32 torch CPU reference's largest error over the class's grid cases
WORST = {
    "large": {
        "fc_comm.weight": 5.04e-07,
        "fc_comm.bias": 5.57e-08,
        "bn_comm.weight": 4.36e-07,
        "bn_comm.bias": 4.35e-07,
        "fc_obs.weight": 4.67e-07,
        "fc_obs.bias": 9.39e-08,
        "bn_obs.weight": 5.17e-07,
        "bn_obs.bias": 4.42e-07,
        "fc_boundary_state.weight": 4.15e-07,
        "fc_boundary_state.bias": 8.04e-08,
        "bn_boundary_state.weight": 3.99e-07,
        "bn_boundary_state.bias": 3.85e-07,
        "fc1.weight": 1.11e-06,
        "fc1.bias": 5.27e-07,
        "bn1.weight": 2.87e-07,
        "bn1.bias": 9.91e-08,
        "fc2.weight": 4.28e-07,
        "fc2.bias": 7.74e-08,
    },
    "small": {
        "fc_comm.weight": 3.05e-03,
        "fc_comm.bias": 6.21e-04,
        "bn_comm.weight": 3.01e-04,
        "bn_comm.bias": 3.01e-04,
        "fc_obs.weight": 3.35e-03,
        "fc_obs.bias": 6.64e-04,
        "bn_obs.weight": 3.21e-04,
        "bn_obs.bias": 3.21e-04,
        "fc_boundary_state.weight": 4.99e-02,
        "fc_boundary_state.bias": 2.08e-02,
        "bn_boundary_state.weight": 3.92e-03,
        "bn_boundary_state.bias": 3.92e-03,
        "fc1.weight": 1.57e-03,
        "fc1.bias": 3.85e-04,
        "bn1.weight": 2.66e-06,
        "bn1.bias": 1.94e-07,
        "fc2.weight": 3.56e-06,
        "fc2.bias": 8.41e-08,
    },
}


def tolerance(B):
    """{param name: tolerance} of a case's class: TOL_FACTOR times the fp32 torch reference's worst."""
    return {k: TOL_FACTOR * w for k, w in WORST[case_class(B)].items()}
