"""Cases, error scales and tolerances for the device learner's gradients, element by element against float64.  Plain
numpy and torch on the CPU; used by test_learner_gradients_cpu.py (no GPU) and test_hip_learner_gradients.py.  The
whole-blob bound learner_harness.tol_g stays what it is; this sits beside it.  The seven bodies below reach the first four
gradient kernels; the clip, advantage and stored kernels have their cases, float64 side and tables in
tests/learner_gradient_forms.py, on this module's metric, comparator and fp32 references (`--forms` prints its tables).

Two observables, one float64 result (`fp64`).  The gradient row of DeviceActorCritic._grad holds the P UNSCALED sums
the gradient kernel accumulates and the four loss sums; a fresh learner's closed update leaves exp_avg = fl(0.1f g), g
the SCALED (and, with a finite max_grad_norm, clipped) gradient, read back by pmi_gradient_cases.recovered_gradient.
`fp64` is tests/learner_mirror.py's forward (theta= the target block, None while no target is enabled; discount= the
rows' discounts), terms (weights and the entropy term) and backward.

The metric.  `gradient_scales` returns S per element: for an unscaled sum the float64 sum over the batch's rows of the
absolute terms (sum_r |dh_rj| |s_rk| for a layer-1 weight with |dh_rj| = mask_rj sum_o |W2_oj| |gz_ro|, sum_r |gz_ro| ha_rj
for the actor's fc2.weight, sum_r |gv_r| for the critic's fc2.bias, sum_r |term| for a loss word); for the scaled
gradient that times the network's |scale|, where under the reference loss the actor's factor mean_j(w_j delta_j), itself
a cancelling sum, enters as mean_j |w_j delta_j|.  `errors` is per tensor max |g - g_fp64| / S; where S = 0 (A = 1, a
unit dead on every row) the expected value is exactly 0 and any other value is an infinite error.

No ReLU knife edges.  Layer-1 biases enter nothing else, so `build_case` moves each into the middle of the widest gap,
near its present value, of that unit's pre-activations: the actor's over the n values on s, the critic's over the 2n
values on s and s' (with a target critic: n values on s, and the target block's own bias over its n values on s').
The gap is chosen among the max(2, m / 8) distinct values on either side of the present threshold, and among as many
at an end of the range: S sees the terms of a sum, not how a term was formed, and a unit that is on in a single row just
above zero hands its layer-2 weight ha_rj with the forward pass's absolute error, a large share of that element's S
whoever computes it.  (With a window that shrank to two values at the top of the range, the case H 255, A 48, n 17 had
the actor's unit 219 on in row 8 alone at 3.4220e-4; the device's chain of 12 fused operations gives 3.421473e-4, which a
float32 emulation of that chain reproduces to the bit, 5.5e-8 away: 1.6e-4 of S for that unit's 48 fc2 weights.)
The case's condition, asserted for every case (`margin`): the smallest |pre-activation| is at least MARGIN_FACTOR = 16
times the largest |pre_fp32 - pre_fp64| of a numpy float32 forward.

Parameters: learner_harness.init_blob ("default"); "peaked" scales the actor's fc2 so that the widest logit spread of
the batch is 40 (a trained, confident policy: probabilities down to e^-40, the spread below 60 so that logf(p) never
sees a denormal); a target block is an independent draw.  Inputs: learner_harness.batch, rewards shifted by +1.5 in
every other reference-loss case (mean(delta) away from 0) and, where a row's delta would lie within MIN_DELTA = 0.25 of
zero, moved by that much away from it (delta is a difference of two values; a unit that is on in a few rows only would
make the relative error of one small delta most of an element, for whoever computes in fp32: torch's autograd on two
CPUs differed by a factor of 3.4 there), weights from learner_harness.make_weights (exact zeros, a maximum of
exactly 1), per-slot discounts from {g, g^2, g^3, 0, 1}, g = float32(0.95).  `dead` cases push one unit of each network
below every row.

The grid sits where the kernel changes path: R = min(256, 4096 / max(H, 16)) rows per tile, 256 threads, at most 256
workgroups.  H 200 and 256 against every n of {1, 2, R - 1, R, R + 1, 2R + 1, 256 R, 256 R + 1, 257 R + 1}; every H
of HS at R + 1 and 2R + 1; the seven bodies at (33, 125), (128, 65), (256, 4113); every A at (64, 65); four peaked
cases; two clipped ones; and H = 16 at n = 65537, the one shape where a 256-row tile is revisited.

Tolerances.  The reference for a tolerance is never the device: it is the same update in fp32 on the CPU in two orders,
torch's fp32 autograd (`torch_fp32`) and a strictly sequential row-ascending float32 sum (`sequential_fp32`; the kernel
adds rows one after another and then 256 partials in order, which torch's blocked sums understate).  WORST_ROW and
WORST_GRAD hold, per class and per tensor, the larger of the two references' worst error over the grid; the tolerance
is TOL_FACTOR = 4 times that (another order of the same sum moves it by a small multiple of the same u S).  The classes
(`case_class`) are by n: "two" n <= 2, "few" n <= 64 (a unit is on in a handful of rows), "mid" n <= 1025, "large"
n <= 8192, "huge" beyond (the 65537-row case alone, whose sequential sum wanders furthest); and "peaked" for the four
peaked cases, whatever their n: 1 - p of a taken action with p within 1e-2 of 1 is a cancellation that no sum's S sees
(1.4e-2 of S in the actor's fc2.weight).  test_learner_gradients_cpu.py holds both references to half a tolerance on
whichever machine runs it.  Measured (x86-64, `python tests/learner_gradient_cases.py` from the repository's root):

    row word                   two         few         mid       large        huge      peaked
    actor.fc1.weight    3.27e-07 t  4.81e-07 t  2.82e-07 s  4.90e-07 s  7.36e-07 s  1.49e-06 s
    actor.fc1.bias      3.13e-07 t  4.59e-07 t  2.58e-07 s  4.66e-07 t  1.05e-06 s  8.55e-07 s
    actor.fc2.weight    2.36e-06 t  2.26e-06 t  1.73e-06 t  6.73e-06 t  3.64e-06 s  1.41e-02 s
    actor.fc2.bias      2.39e-07 t  2.80e-07 t  2.99e-07 s  9.79e-07 s  1.36e-06 s  1.76e-06 s
    critic.fc1.weight   2.89e-07 t  4.11e-07 t  5.05e-07 s  3.22e-06 s  6.80e-06 s  4.89e-07 s
    critic.fc1.bias     2.42e-07 t  3.60e-07 s  4.68e-07 s  2.55e-06 s  4.23e-06 s  4.46e-07 s
    critic.fc2.weight   3.81e-06 t  1.04e-06 t  1.57e-06 t  8.25e-06 t  5.62e-06 s  3.85e-06 s
    critic.fc2.bias     1.90e-07 t  6.28e-08 s  3.87e-07 s  1.24e-06 s  1.84e-06 s  1.29e-07 s
    sum.nlp             4.10e-08 t  1.39e-07 t  4.34e-07 s  1.67e-06 s  5.90e-06 s  4.31e-07 s
    sum.delta           1.90e-07 t  6.28e-08 s  3.87e-07 s  1.24e-06 s  1.84e-06 s  1.29e-07 s
    sum.actor           1.56e-07 t  1.38e-07 s  2.68e-07 s  4.31e-07 s  2.04e-06 s  1.78e-07 s
    sum.critic          3.95e-07 t  1.08e-07 s  5.05e-07 s  1.64e-06 s  1.05e-06 s  1.03e-06 s
    scaled gradient            two         few         mid       large        huge      peaked
    actor.fc1.weight    3.27e-07 t  4.88e-07 t  3.03e-07 s  1.05e-06 s  9.56e-07 s  1.48e-06 s
    actor.fc1.bias      3.13e-07 t  4.70e-07 t  3.00e-07 s  1.02e-06 s  9.34e-07 s  8.45e-07 s
    actor.fc2.weight    1.82e-06 t  2.13e-06 s  1.72e-06 s  6.28e-06 t  4.07e-06 s  1.41e-02 s
    actor.fc2.bias      4.30e-07 t  3.01e-07 t  4.30e-07 s  7.58e-07 s  9.98e-07 s  1.76e-06 s
    critic.fc1.weight   2.89e-07 t  4.40e-07 s  5.03e-07 s  3.20e-06 s  6.82e-06 s  5.02e-07 s
    critic.fc1.bias     2.42e-07 t  4.21e-07 s  4.15e-07 s  2.53e-06 s  4.25e-06 s  4.29e-07 s
    critic.fc2.weight   3.81e-06 t  9.76e-07 t  1.55e-06 t  8.23e-06 t  5.58e-06 s  3.86e-06 s
    critic.fc2.bias     1.90e-07 t  8.16e-08 s  3.77e-07 s  1.26e-06 s  1.86e-06 s  1.28e-07 s
    (t: set by torch's autograd, s: by the sequential sum; a tolerance is 4 times the entry)

Second steps (`TWO_STEP`): 2n rows, learner A takes the first n, learner B the first n and then the second n; B's second
gradient is pmi_gradient_cases.second_step_gradient of the two exp_avg, compared with `fp64` at A's device parameters on
the second n rows.  The biases are placed over both halves, the learning rates are LR_TWO_STEP so that one Adam step
moves a pre-activation by at most 1e-3, and the margin is asserted again at the parameters after the step."""
import collections
import functools
import types
import zlib

import numpy as np

import learner_advantage_mirror as am
import learner_harness as lh
import learner_mirror as mirror
import pmi_gradient_cases as pc

F32 = np.float32
GAMMA = 0.95
LR_TWO_STEP = (1e-5, 5e-5)
C_ENT = 0.1
MIN_DELTA = 0.25
MARGIN_FACTOR, TOL_FACTOR, MUTANT_ROOM = pc.MARGIN_FACTOR, pc.TOL_FACTOR, pc.MUTANT_ROOM
TENSORS = ("actor.fc1.weight", "actor.fc1.bias", "actor.fc2.weight", "actor.fc2.bias",
           "critic.fc1.weight", "critic.fc1.bias", "critic.fc2.weight", "critic.fc2.bias")
ACTOR, CRITIC = TENSORS[:4], TENSORS[4:]
LOSS_WORDS = ("sum.nlp", "sum.delta", "sum.actor", "sum.critic")
ROW_WORDS = TENSORS + LOSS_WORDS
BODIES = ("plain", "weighted", "discounted", "reg0", "regc", "target", "all")
HS = (1, 15, 16, 17, 32, 33, 64, 128, 200, 255, 256)
AS = (1, 2, 9, 12, 47, 48)

Spec = collections.namedtuple("Spec", "H A n loss body gather cls shift mgn dead")


def rows_per_tile(H):
    """learner_rows_per_tile of csrc/learner_kernel.hip."""
    return min(256, 4096 // max(H, 16))


def n_values(H):
    R = rows_per_tile(H)
    tail = [256 * R, 256 * R + 1, 257 * R + 1] if H in (200, 256) else []
    return sorted({1, 2, R - 1, R, R + 1, 2 * R + 1, *tail})


CLASSES = ("two", "few", "mid", "large", "huge", "peaked")


def case_class(sp):
    """By n, the peaked parameters apart: 1 - p of a taken action with p near 1 is a cancellation no sum's scale sees."""
    n = sp.n
    return "peaked" if sp.cls == "peaked" else \
        "two" if n <= 2 else "few" if n <= 64 else "mid" if n <= 1025 else "large" if n <= 8192 else "huge"


def spec_id(sp):
    return (f"H{sp.H}-A{sp.A}-n{sp.n}-{sp.loss}-{sp.body}" + ("-indexed" if sp.gather else "") +
            ("-peaked" if sp.cls == "peaked" else "") + ("-shift" if sp.shift else "") + ("-clip" if sp.mgn else "") +
            ("-dead" if sp.dead else ""))


def _grid():
    out, seen, refs = [], set(), [0]

    def add(H, A, n, loss, body="plain", gather=False, cls="default", mgn=None, dead=False):
        if body == "regc":
            loss = "per_sample"
        key = (H, A, n, loss, body, gather, cls, mgn, dead)
        if key in seen:
            return
        seen.add(key)
        shift = False
        if loss == "reference":
            refs[0] += 1
            shift = refs[0] % 2 == 0
        out.append(Spec(H, A, n, loss, body, gather, cls, shift, mgn, dead))

    forms = (("reference", False), ("per_sample", True), ("reference", True), ("per_sample", False))
    k = 0
    plain = set()
    for H in (200, 256):                                    # two widths against every n
        for n in n_values(H):
            add(H, (12, 48, 9)[k % 3], n, forms[k % 4][0], "plain", forms[k % 4][1])
            plain.add((H, n))
            k += 1
    for H in HS:                                            # every width at R + 1 and 2R + 1
        for n in (rows_per_tile(H) + 1, 2 * rows_per_tile(H) + 1):
            if (H, n) not in plain:
                add(H, (12, 48, 9)[k % 3], n, forms[k % 4][0], "plain", forms[k % 4][1])
                k += 1
    turns = (("reference", True), ("per_sample", False), ("per_sample", True), ("reference", False))
    for b, body in enumerate(BODIES):                       # every body at three points, both losses, both batch forms
        for p, (H, A, n) in enumerate(((33, 9, 125), (128, 12, 65), (256, 48, 4113))):
            add(H, A, n, turns[(b + p) % 4][0], body, turns[(b + p) % 4][1])
        add(33, 9, 125, "per_sample" if b % 2 == 0 else "reference", body, b % 2 == 1)
    for A in AS:                                            # every action count
        add(64, A, 65, "per_sample" if A in (2, 47) else "reference", "plain", A in (9, 47), dead=A in (1, 12))
    add(33, 9, 125, "reference", "plain", False, "peaked")
    add(128, 12, 65, "per_sample", "plain", True, "peaked")
    add(256, 48, 4113, "per_sample", "regc", False, "peaked")
    add(16, 12, 257, "reference", "all", True, "peaked")
    add(128, 12, 33, "per_sample", "plain", False, mgn=(1e-3, 1e-3))
    add(33, 9, 249, "reference", "all", True, mgn=(1e-3, 5e-4))
    add(16, 12, 65537, "reference", "plain", False)         # the one shape whose 256-row tiles are revisited
    return out


GRID = _grid()
TWO_STEP = [Spec(33, 12, 125, "reference", "plain", False, "default", True, None, False),
            Spec(256, 48, 33, "per_sample", "all", True, "default", False, None, False),
            Spec(16, 12, 257, "reference", "weighted", True, "default", False, None, False)]


# ---- the cases

def _threshold(v, tau):
    """Where zero goes among a unit's values v (pre-activation minus bias, so the unit is on where v > threshold)."""
    v = np.unique(v)                                            # sorted; an index vector may name a row twice
    if len(v) < 2:
        return tau if abs(v[0] - tau) >= 0.05 else v[0] - 0.05
    w = max(2, len(v) // 8)
    lo = max(0, min(int(np.searchsorted(v, tau)) - w, len(v) - 2 * w - 1))
    gaps = np.diff(v[lo:lo + 2 * w + 1])
    i = lo + int(np.argmax(gaps))
    if len(v) <= 4 and gaps.max() < 0.1:                        # a handful of values close together: all of them on
        return v[0] - 0.05
    return 0.5 * (v[i] + v[i + 1])


def _placed(W, b, x):
    """The bias b of a layer-1 block moved so that no pre-activation of rows x lies near zero."""
    v = np.asarray(x, np.float64) @ np.asarray(W, np.float64).T
    return np.array([-_threshold(v[:, j], -float(b[j])) for j in range(len(b))]).astype(F32)


def _blocks(blob, theta, H, A, s, s2):
    """[(layer-1 weight, bias, the rows it is evaluated on)] of the three forwards of one update."""
    w1a, b1a, _, _, w1c, b1c, _, _ = mirror.unpack(blob, H, A)
    if theta is None:
        return [(w1a, b1a, s), (w1c, b1c, np.concatenate([s, s2]))]
    th = np.asarray(theta, np.float64)
    return [(w1a, b1a, s), (w1c, b1c, s), (th[:12 * H].reshape(H, 12), th[12 * H:13 * H], s2)]


def margin(c, blob=None, theta=None, rows=None):
    """(the smallest |pre-activation| in float64, the largest |pre_fp32 - pre_fp64| of a numpy float32 forward) over
    the layer-1 blocks of the case's update, at `blob` / `theta` (default: the case's) on `rows` (default: its batch)."""
    blob = c.blob if blob is None else blob
    theta = c.theta if theta is None else theta
    s, _, _, s2 = c.rows if rows is None else rows
    lo, err = np.inf, 0.0
    for W, b, x in _blocks(blob, theta, c.H, c.A, s, s2):
        p64 = np.asarray(x, np.float64) @ W.T + b
        p32 = np.asarray(x, F32) @ W.astype(F32).T + b.astype(F32)
        assert p32.dtype == F32
        lo, err = min(lo, float(np.abs(p64).min())), max(err, float(np.abs(p32 - p64).max()))
    return lo, err


def logit_spread(blob, H, A, s):
    """The widest max - min of a row's logits, in float64."""
    z = mirror.logits(blob, H, A, s)
    return float((z.max(axis=1) - z.min(axis=1)).max())


def _build(sp, halves, distinct=False):
    """The case of sp over `halves` batches of sp.n rows each (two for a second-step case); distinct: an index vector
    names no slot twice (the form cases, whose per-slot stores are dealt by batch row)."""
    H, A, n = sp.H, sp.A, sp.n
    seed = zlib.crc32(repr((tuple(sp), halves)).encode()) % (2 ** 31 - 1)
    rng = np.random.RandomState(seed)
    cap = halves * n + (7 if sp.gather else 0)
    blob = lh.init_blob(H, A, seed)
    has_target = sp.body in ("target", "all")
    theta = mirror.critic_block(lh.init_blob(H, A, seed + 5000), H, A) if has_target else None
    s, a, r, s2 = lh.batch(rng, cap, A)
    if sp.shift:
        r = (r + F32(1.5)).astype(F32)
    if sp.gather and distinct:
        perm = rng.permutation(cap).astype(np.int64)
        idx = [perm[h * n:(h + 1) * n] for h in range(halves)]
    elif sp.gather:
        idx = [rng.randint(0, cap, size=n).astype(np.int64) for _ in range(halves)]
    else:
        idx = [np.arange(h * n, (h + 1) * n) for h in range(halves)]
    weights = [lh.make_weights(rng, n) for _ in range(halves)] if sp.body in ("weighted", "discounted", "all") else None
    g = F32(GAMMA)
    disc = rng.choice(np.array([g, g * g, g * g * g, 0.0, 1.0], F32), size=cap).astype(F32) \
        if sp.body in ("discounted", "all") else None
    # layer-1 biases away from the batch's ReLU decisions
    o = mirror.layout(H, A)[1]
    every = np.concatenate(idx)
    (w1a, b1a, xa), (w1c, b1c, xc), *rest = _blocks(blob, theta, H, A, s[every], s2[every])
    blob[o[1]:o[2]] = _placed(w1a, b1a, xa)
    blob[o[5]:o[6]] = _placed(w1c, b1c, xc)
    if rest:
        theta[12 * H:13 * H] = _placed(*rest[0])
    if sp.dead:
        blob[o[1]] = blob[o[6] - 1] = -50.0
    if sp.cls == "peaked":
        f = 40.0 / logit_spread(blob, H, A, s[every])
        blob[o[2]:o[4]] = (blob[o[2]:o[4]].astype(np.float64) * f).astype(F32)
    # no row's delta within MIN_DELTA of zero: delta is a difference of two values, and a unit that is on in a few rows
    # only would make the relative error of one small delta most of an element
    dslot = np.full(cap, F32(GAMMA), F32) if disc is None else disc
    delta = mirror.forward(blob, H, A, s, a, r, s2, dslot, theta).delta
    near = np.abs(delta) < MIN_DELTA
    r = np.where(near, r + np.where(delta >= 0, MIN_DELTA, -MIN_DELTA), r).astype(F32)
    c = types.SimpleNamespace(
        spec=sp, H=H, A=A, n=n, loss=sp.loss, blob=blob, theta=theta, cap=cap, store=(s, a, r, s2), idx=idx,
        weights=weights, disc=disc, mgn=sp.mgn, gather=sp.gather,
        c=C_ENT if sp.body == "regc" or (sp.body == "all" and sp.loss == "per_sample") else 0.0,
        diag=sp.body in ("reg0", "regc", "all"))
    c.rows = tuple(x[idx[0]] for x in c.store)
    return c


@functools.lru_cache(maxsize=None)
def build_case(sp):
    """One batch of sp.n rows: blob, theta (None without a target), the store's four arrays and its capacity, idx[0] the
    batch's slots, weights[0] (or None) per batch row, disc (or None) per slot, c the entropy coefficient, diag whether
    the entropy buffer is installed, rows the gathered batch."""
    return _build(sp, 1)


@functools.lru_cache(maxsize=None)
def build_two_step_case(sp):
    """2 n rows: idx[0], weights[0] are step one's, idx[1], weights[1] step two's; the biases placed over all of them."""
    return _build(sp, 2)


def batch_of(c, h=0):
    """(gathered (s, a, r, s2), weights or None, the rows' discounts) of the case's batch h."""
    i = c.idx[h]
    d = np.full(c.n, F32(GAMMA), F32) if c.disc is None else c.disc[i]
    return tuple(x[i] for x in c.store), None if c.weights is None else c.weights[h], d


# ---- the float64 side

def _scaled(c, sums, loss4, n, md=None, swap=False):
    """(scaled and clipped gradient, coefficients, actor scale, critic scale, actor loss, critic loss) from the sums."""
    md = loss4[1] / n if md is None else md
    na = mirror.layout(c.H, c.A)[1][4]
    sa, sc = (-md / n if c.loss == "reference" else -1.0 / n), 2.0 / n
    g = sums * np.concatenate([np.full(na, sa), np.full(sums.size - na, sc)])
    coef = mirror.clip_grad_norm(g, c.H, c.A, c.mgn)[0] if c.mgn else np.ones(2)
    if swap:
        coef = coef[::-1]
    g = g * np.concatenate([np.full(na, coef[0]), np.full(sums.size - na, coef[1])])
    al = (loss4[0] / n) * (loss4[1] / n) if c.loss == "reference" else loss4[2] / n
    return g, coef, sa, sc, al, loss4[3] / n


def pieces(c, h=0, blob=None, theta=None):
    """The per-row pieces of batch h in float64 at `blob` / `theta` (default: the case's): the forward record, the logit
    weights gz [n][A], the value weights gv [n], the four loss terms lt [4][n]."""
    (s, a, r, s2), w, d = batch_of(c, h)
    f = mirror.forward(c.blob if blob is None else blob, c.H, c.A, s, a, r, s2, d, c.theta if theta is None else theta)
    return (f, *mirror.terms(f, c.loss, w, c.c)[:3])


def fp64(c, h=0, blob=None, theta=None):
    """The float64 result of batch h: sums [P] (unscaled), loss4, grad [P] (scaled, clipped), td, the two losses, the
    clip coefficients, and S_row [P + 4], S_grad [P] from gradient_scales."""
    f, gz, gv, lt = pieces(c, h, blob, theta)
    sums, loss4 = mirror.backward(f, gz, gv), lt.sum(axis=1)
    g, coef, sa, sc, al, cl = _scaled(c, sums, loss4, f.n)
    S_row, S_grad = gradient_scales(c, f, gz, gv, lt, coef)
    return types.SimpleNamespace(sums=sums, loss4=loss4, grad=g, td=f.delta, actor_loss=al, critic_loss=cl, coef=coef,
                                 entropy=f.entropy, S_row=S_row, S_grad=S_grad)


def _network_factors(c, lt, n, coef, size):
    """|scale| per word of the scaled gradient, the reference loss's mean(w delta) entering as mean |w delta|."""
    na = mirror.layout(c.H, c.A)[1][4]
    fa = (np.abs(lt[1]).sum() / n if c.loss == "reference" else 1.0) / n * coef[0]
    return np.concatenate([np.full(na, fa), np.full(size - na, 2.0 / n * coef[1])])


def gradient_scales(c, f, gz, gv, lt, coef=(1.0, 1.0), agz=None):
    """(S of the row's P + 4 words, S of the scaled gradient's P words): the float64 sums of the absolute terms.  agz:
    the absolute parts of the logit weights where they are not |gz| (the form cases, below)."""
    n = f.n
    sa_, agz, agv = np.abs(f.s), np.abs(gz) if agz is None else agz, np.abs(gv)
    adh = (agz @ np.abs(f.w2a)) * (f.pa > 0)
    adc = agv[:, None] * np.abs(f.w2c) * (f.pc > 0)
    S = np.concatenate([x.ravel() for x in (adh.T @ sa_, adh.sum(0), agz.T @ f.ha, agz.sum(0), adc.T @ sa_, adc.sum(0),
                                            (agv[:, None] * f.hc).sum(0), np.array([agv.sum()]))])
    return np.concatenate([S, np.abs(lt).sum(axis=1)]), S * _network_factors(c, lt, n, coef, S.size)


def errors(got, ref, S, H, A, slack=None):
    """{name: max over the tensor of max(|got - ref| - slack, 0) / S} over TENSORS, and over LOSS_WORDS where the
    arrays hold P + 4 words.  An element whose S is zero has no nonzero term: there any difference is infinite."""
    got, ref, S = (np.asarray(x, np.float64) for x in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    d = np.abs(got - ref)
    if slack is not None:
        d = np.maximum(d - slack, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(S > 0, d / S, np.where(d > 0, np.inf, 0.0))
    o = mirror.layout(H, A)[1]
    out = {k: float(e[o[t]:o[t + 1]].max()) for t, k in enumerate(TENSORS)}
    if got.size == o[8] + 4:
        out.update({k: float(e[o[8] + q]) for q, k in enumerate(LOSS_WORDS)})
    return out


# ---- the two fp32 references

def torch_fp32(c, stats=None, out=None):
    """(row words [P + 4], scaled gradient [P]) of batch 0 by torch's fp32 autograd on the CPU: the unscaled sums are
    the gradient of sum_i w_i (coef_i log p_i(a_i) + c H_i) + sum_i w_i (V_i - y_i)^2 / 2 with delta and y detached,
    the scales are formed in fp32 from the loss sums as the finalize kernel forms them.  A form case (c.form, below)
    has its surrogate in coef_i log p_i(a_i)'s place: A_i log p_i(a_i), or r_i A_i where the row passes and bound A_i
    where it does not, A_i a constant; stats = (mean, inv_std) of a "batch" form; out, a dict, receives "pass", "ratio"
    and "adv" of the rows."""
    import torch
    (s, a, r, s2), w, d = batch_of(c)
    H, A, n = c.H, c.A, c.n
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, F32))
    prm = [t(x).requires_grad_() for x in mirror.unpack(c.blob, H, A)]
    w1a, b1a, w2a, b2a, w1c, b1c, w2c, b2c = prm
    th = c.theta if c.theta is not None else mirror.critic_block(c.blob, H, A)
    w1t, b1t, w2t, b2t = t(th[:12 * H].reshape(H, 12)), t(th[12 * H:13 * H]), t(th[13 * H:14 * H]), t(th[14 * H:])
    s, s2, r, d = t(s), t(s2), t(r), t(d)
    iw = torch.ones(n) if w is None else t(w)
    logp = torch.log_softmax(torch.relu(s @ w1a.T + b1a) @ w2a.T + b2a, dim=1)
    v = (torch.relu(s @ w1c.T + b1c) @ w2c.T)[:, 0] + b2c[0]
    with torch.no_grad():
        y = r + d * (torch.relu(s2 @ w1t.T + b1t) @ w2t + b2t[0])
    delta = (y - v).detach()
    lpa = logp[torch.arange(n), torch.from_numpy(np.asarray(a, np.int64))]
    ent = -(torch.exp(logp) * logp).sum(dim=1)
    if getattr(c, "form", None) is None:
        coef = delta if c.loss == "per_sample" else torch.ones(n)
        gain, surr = coef * lpa, lpa * delta
    else:
        adv = t(_advantage32(c, delta.numpy(), stats))
        if c.form.clip is None:
            ok, ratio, gain = None, None, adv * lpa
        else:
            lo, hi = (float(x) for x in mirror.bounds(c.form.clip))
            ratio = torch.exp(lpa - t(c.log_mu[c.idx[0]]))
            with torch.no_grad():
                ok = torch.where(adv >= 0, ratio <= hi, ratio >= lo)
                edge = torch.where(adv >= 0, torch.tensor(hi), torch.tensor(lo))
                flat = torch.where(ok, torch.zeros(n), edge * adv)      # (inf * 0 on a passing row is not selected)
            gain = torch.where(ok, ratio * adv, flat)
        surr = gain.detach()
        if out is not None:
            out.update({"pass": None if ok is None else ok.numpy(), "adv": adv.numpy(),
                        "ratio": None if ratio is None else ratio.detach().numpy()})
    ((iw * (gain + float(c.c) * ent)).sum() + (iw * (v - y) ** 2).sum() / 2).backward()
    sums = torch.cat([p.grad.reshape(-1) for p in prm])
    with torch.no_grad():
        loss4 = torch.stack([(-lpa * iw).sum(), (delta * iw).sum(), (iw * (-surr - float(c.c) * ent)).sum(),
                             (iw * (v - y) ** 2).sum()])
    return _finish32(c, sums.numpy(), loss4.numpy())


def _finish32(c, sums, loss4):
    """fp32 sums -> (row words, scaled gradient), the scales and the clip in float32 / float64 as the kernels hold them."""
    assert sums.dtype == F32 and loss4.dtype == F32
    n, na = c.n, mirror.layout(c.H, c.A)[1][4]
    inv_n = F32(1.0) / F32(n)
    sa = -inv_n if c.loss == "per_sample" else -(loss4[1] * inv_n) * inv_n
    g = sums * np.concatenate([np.full(na, sa, F32), np.full(sums.size - na, F32(2.0) * inv_n, F32)])
    assert g.dtype == F32
    if c.mgn:
        coef = mirror.clip_grad_norm(g.astype(np.float64), c.H, c.A, c.mgn)[0].astype(F32)
        g = g * np.concatenate([np.full(na, coef[0], F32), np.full(sums.size - na, coef[1], F32)])
    return np.concatenate([sums, loss4]).astype(np.float64), g.astype(np.float64)


def _advantage32(c, delta32, stats):
    """The float32 advantage of a form case's batch 0 from a reference's own float32 delta: the stored value where there
    is one, through fl(fl(x - mean) * inv_std) unless raw."""
    x = c.advantages[c.idx[0]] if c.form.stored else np.asarray(delta32, F32)
    if c.form.adv == "raw":
        return x
    mean, inv = c.given if c.form.adv == "given" else stats
    return am.standardise(x, mean, inv)


def sequential_fp32(c, stats=None, out=None):
    """(row words, scaled gradient) of batch 0 in numpy float32, every sum over rows taken one row after another in
    ascending order.  stats and out as torch_fp32's."""
    (s, a, r, s2), w, d = batch_of(c)
    H, A, n = c.H, c.A, c.n
    w1a, b1a, w2a, b2a, w1c, b1c, w2c, b2c = (x.astype(F32) for x in mirror.unpack(c.blob, H, A))
    th = (c.theta if c.theta is not None else mirror.critic_block(c.blob, H, A)).astype(F32)
    iw = np.ones(n, F32) if w is None else w.astype(F32)
    pa = s @ w1a.T + b1a; ha = np.maximum(pa, 0)
    z = ha @ w2a.T + b2a
    dz = z - z.max(axis=1, keepdims=True)
    e = np.exp(dz)
    logp = dz - np.log(e.sum(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    pc_ = s @ w1c.T + b1c; hc = np.maximum(pc_, 0)
    v = hc @ w2c[0] + b2c[0]
    y = r + d * (np.maximum(s2 @ th[:12 * H].reshape(H, 12).T + th[12 * H:13 * H], 0) @ th[13 * H:14 * H] + th[14 * H])
    delta = y - v
    ent = -np.where(p > 0, p * logp, F32(0)).sum(axis=1)
    onehot = np.zeros_like(p); onehot[np.arange(n), a] = 1
    nlp = -logp[np.arange(n), a]
    if getattr(c, "form", None) is None:
        coef = delta if c.loss == "per_sample" else np.ones(n, F32)
        actor = nlp * delta
    else:
        adv = _advantage32(c, delta, stats)
        if c.form.clip is None:
            ok, ratio, coef, actor = None, None, adv, nlp * adv
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                lo, hi = F32(1.0) - F32(c.form.clip), F32(1.0) + F32(c.form.clip)
                ratio = np.exp(-nlp - c.log_mu[c.idx[0]])
                ok = np.where(adv >= 0, ratio <= hi, ratio >= lo)
                coef = np.where(ok, adv * ratio, F32(0))
                actor = -np.where(ok, coef, np.where(adv >= 0, hi, lo) * adv)
        if out is not None:
            out.update({"pass": ok, "adv": adv, "ratio": ratio})
    gz = iw[:, None] * (coef[:, None] * (onehot - p) - F32(c.c) * np.where(p > 0, p * (logp + ent[:, None]), F32(0)))
    gv = (v - y) * iw
    lt = np.stack([nlp * iw, delta * iw, iw * (actor - F32(c.c) * ent), (v - y) ** 2 * iw], axis=1)
    dh = (gz @ w2a) * (pa > 0)
    dc = gv[:, None] * w2c * (pc_ > 0)
    for x in (gz, gv, lt, dh, dc, ha, hc):
        assert x.dtype == F32
    acc = [np.zeros(k, F32) for k in ((H, 12), H, (A, H), A, (H, 12), H, H, 1, 4)]
    for i in range(n):
        acc[0] += np.outer(dh[i], s[i]); acc[1] += dh[i]
        acc[2] += np.outer(gz[i], ha[i]); acc[3] += gz[i]
        acc[4] += np.outer(dc[i], s[i]); acc[5] += dc[i]
        acc[6] += gv[i] * hc[i]; acc[7] += gv[i]
        acc[8] += lt[i]
    return _finish32(c, np.concatenate([x.ravel() for x in acc[:8]]), acc[8])


# ---- tolerances: per class and word, the larger of the two fp32 CPU references' worst error over the class's grid cases
WORST_ROW = {
    "two": {
        "actor.fc1.weight": 3.27e-07,
        "actor.fc1.bias": 3.13e-07,
        "actor.fc2.weight": 2.36e-06,
        "actor.fc2.bias": 2.39e-07,
        "critic.fc1.weight": 2.89e-07,
        "critic.fc1.bias": 2.42e-07,
        "critic.fc2.weight": 3.81e-06,
        "critic.fc2.bias": 1.90e-07,
        "sum.nlp": 4.10e-08,
        "sum.delta": 1.90e-07,
        "sum.actor": 1.56e-07,
        "sum.critic": 3.95e-07,
    },
    "few": {
        "actor.fc1.weight": 4.81e-07,
        "actor.fc1.bias": 4.59e-07,
        "actor.fc2.weight": 2.26e-06,
        "actor.fc2.bias": 2.80e-07,
        "critic.fc1.weight": 4.11e-07,
        "critic.fc1.bias": 3.60e-07,
        "critic.fc2.weight": 1.04e-06,
        "critic.fc2.bias": 6.28e-08,
        "sum.nlp": 1.39e-07,
        "sum.delta": 6.28e-08,
        "sum.actor": 1.38e-07,
        "sum.critic": 1.08e-07,
    },
    "mid": {
        "actor.fc1.weight": 2.82e-07,
        "actor.fc1.bias": 2.58e-07,
        "actor.fc2.weight": 1.73e-06,
        "actor.fc2.bias": 2.99e-07,
        "critic.fc1.weight": 5.05e-07,
        "critic.fc1.bias": 4.68e-07,
        "critic.fc2.weight": 1.57e-06,
        "critic.fc2.bias": 3.87e-07,
        "sum.nlp": 4.34e-07,
        "sum.delta": 3.87e-07,
        "sum.actor": 2.68e-07,
        "sum.critic": 5.05e-07,
    },
    "large": {
        "actor.fc1.weight": 4.90e-07,
        "actor.fc1.bias": 4.66e-07,
        "actor.fc2.weight": 6.73e-06,
        "actor.fc2.bias": 9.79e-07,
        "critic.fc1.weight": 3.22e-06,
        "critic.fc1.bias": 2.55e-06,
        "critic.fc2.weight": 8.25e-06,
        "critic.fc2.bias": 1.24e-06,
        "sum.nlp": 1.67e-06,
        "sum.delta": 1.24e-06,
        "sum.actor": 4.31e-07,
        "sum.critic": 1.64e-06,
    },
    "huge": {
        "actor.fc1.weight": 7.36e-07,
        "actor.fc1.bias": 1.05e-06,
        "actor.fc2.weight": 3.64e-06,
        "actor.fc2.bias": 1.36e-06,
        "critic.fc1.weight": 6.80e-06,
        "critic.fc1.bias": 4.23e-06,
        "critic.fc2.weight": 5.62e-06,
        "critic.fc2.bias": 1.84e-06,
        "sum.nlp": 5.90e-06,
        "sum.delta": 1.84e-06,
        "sum.actor": 2.04e-06,
        "sum.critic": 1.05e-06,
    },
    "peaked": {
        "actor.fc1.weight": 1.49e-06,
        "actor.fc1.bias": 8.55e-07,
        "actor.fc2.weight": 1.41e-02,
        "actor.fc2.bias": 1.76e-06,
        "critic.fc1.weight": 4.89e-07,
        "critic.fc1.bias": 4.46e-07,
        "critic.fc2.weight": 3.85e-06,
        "critic.fc2.bias": 1.29e-07,
        "sum.nlp": 4.31e-07,
        "sum.delta": 1.29e-07,
        "sum.actor": 1.78e-07,
        "sum.critic": 1.03e-06,
    },
}
WORST_GRAD = {
    "two": {
        "actor.fc1.weight": 3.27e-07,
        "actor.fc1.bias": 3.13e-07,
        "actor.fc2.weight": 1.82e-06,
        "actor.fc2.bias": 4.30e-07,
        "critic.fc1.weight": 2.89e-07,
        "critic.fc1.bias": 2.42e-07,
        "critic.fc2.weight": 3.81e-06,
        "critic.fc2.bias": 1.90e-07,
    },
    "few": {
        "actor.fc1.weight": 4.88e-07,
        "actor.fc1.bias": 4.70e-07,
        "actor.fc2.weight": 2.13e-06,
        "actor.fc2.bias": 3.01e-07,
        "critic.fc1.weight": 4.40e-07,
        "critic.fc1.bias": 4.21e-07,
        "critic.fc2.weight": 9.76e-07,
        "critic.fc2.bias": 8.16e-08,
    },
    "mid": {
        "actor.fc1.weight": 3.03e-07,
        "actor.fc1.bias": 3.00e-07,
        "actor.fc2.weight": 1.72e-06,
        "actor.fc2.bias": 4.30e-07,
        "critic.fc1.weight": 5.03e-07,
        "critic.fc1.bias": 4.15e-07,
        "critic.fc2.weight": 1.55e-06,
        "critic.fc2.bias": 3.77e-07,
    },
    "large": {
        "actor.fc1.weight": 1.05e-06,
        "actor.fc1.bias": 1.02e-06,
        "actor.fc2.weight": 6.28e-06,
        "actor.fc2.bias": 7.58e-07,
        "critic.fc1.weight": 3.20e-06,
        "critic.fc1.bias": 2.53e-06,
        "critic.fc2.weight": 8.23e-06,
        "critic.fc2.bias": 1.26e-06,
    },
    "huge": {
        "actor.fc1.weight": 9.56e-07,
        "actor.fc1.bias": 9.34e-07,
        "actor.fc2.weight": 4.07e-06,
        "actor.fc2.bias": 9.98e-07,
        "critic.fc1.weight": 6.82e-06,
        "critic.fc1.bias": 4.25e-06,
        "critic.fc2.weight": 5.58e-06,
        "critic.fc2.bias": 1.86e-06,
    },
    "peaked": {
        "actor.fc1.weight": 1.48e-06,
        "actor.fc1.bias": 8.45e-07,
        "actor.fc2.weight": 1.41e-02,
        "actor.fc2.bias": 1.76e-06,
        "critic.fc1.weight": 5.02e-07,
        "critic.fc1.bias": 4.29e-07,
        "critic.fc2.weight": 3.86e-06,
        "critic.fc2.bias": 1.28e-07,
    },
}


def tolerances(sp):
    """({row word: tolerance}, {tensor: tolerance}) of a case's class: TOL_FACTOR times the references' worst."""
    k = case_class(sp)
    return ({w: TOL_FACTOR * x for w, x in WORST_ROW[k].items()}, {w: TOL_FACTOR * x for w, x in WORST_GRAD[k].items()})


def over(e, tol):
    """The entries of e beyond their tolerance: {name: (error, tolerance)}."""
    return {k: (e[k], tol[k]) for k in e if not e[k] <= tol[k]}


def report(tag, e, tol):
    print(tag, " ".join(f"{k}={e[k]:.2e}/{e[k] / tol[k] if tol[k] > 0 else float(e[k] > 0):.2f}" for k in e))


def measure():
    """Both references over the grid: (worst row errors, worst gradient errors) per class, and who set each."""
    row = {k: {w: (0.0, "") for w in ROW_WORDS} for k in CLASSES}
    grad = {k: {w: (0.0, "") for w in TENSORS} for k in row}
    for sp in GRID:
        c = build_case(sp)
        ref = fp64(c)
        for name, fn in (("torch", torch_fp32), ("sequential", sequential_fp32)):
            r, g = fn(c)
            for table, e in ((row, errors(r, np.concatenate([ref.sums, ref.loss4]), ref.S_row, c.H, c.A)),
                             (grad, errors(g, ref.grad, ref.S_grad, c.H, c.A))):
                t = table[case_class(sp)]
                for w, x in e.items():
                    if x > t[w][0]:
                        t[w] = (x, name, spec_id(sp))
    return row, grad


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl-uavs-targets-tracking_amd"))
    forms = "--forms" in sys.argv                               # the form cases' tables (learner_gradient_forms.py)
    if forms:
        import learner_gradient_forms
        row, grad, ratio = learner_gradient_forms.measure()
        print("RATIO_WORST =", {k: float(f"{x:.2e}") for k, x in ratio.items()})
    else:
        row, grad = measure()
    for title, table in (("FORM_WORST_ROW", row), ("FORM_WORST_GRAD", grad)) if forms else \
            (("WORST_ROW", row), ("WORST_GRAD", grad)):
        print(f"{title} = {{")
        for k, t in table.items():
            print(f'    "{k}": {{')
            for w, (x, *who) in t.items():
                print(f'        "{w}": {x:.2e},')
            print("    },")
        print("}")
    for title, table in (("row", row), ("scaled gradient", grad)):
        print(f"    {title:<18}" + "".join(f"{k:>16}" for k in table))
        for w in table["two"]:
            print(f"    {w:<18}" + "".join(f"{table[k][w][0]:>11.2e} {table[k][w][1][:3]:<4}" if w in table[k] else
                                           f"{'':>16}" for k in table))
    if "--who" in sys.argv:
        for table in (row, grad):
            for k, t in table.items():
                for w, x in t.items():
                    print(k, w, *x)
