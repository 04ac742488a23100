"""Cases, two references, the error metric and the tolerances for the device trainers' Adam step (adam_element,
csrc/adam.h) from a LOADED state: non-zero moments and one step count per tensor.  Plain numpy on the CPU; used by
test_adam_cpu.py (no GPU) and test_hip_adam.py.

Two references.  `restate32` is adam_element operation for operation in numpy float32: the library is built without
contraction, so every fp32 subtract, multiply, add, sqrtf and divide has one IEEE result, and the two fp64 scalars of a
tensor, lr / bc1 and sqrt(bc2) with bc = 1 - beta^step, are rounded to fp32 once.  `fp64_learner` / `fp64_pmi` are
torch's formula in float64 through the mirrors' own Adam (learner_mirror.adam, pmi_trainer_mirror.adam_step), given the
learning rate the handle holds, float(np.float32(lr)).

An exactly known gradient.  DeviceActorCritic.apply takes gradient rows from the caller: P unscaled sums, 4 loss sums,
then the int32 words n_lo, n_hi, status, P.  learner_finalize_kernel scales the ordered sum of the rows by -1 / N (actor,
"per_sample"), -mean_delta / N (actor, "reference") and 2 / N (critic).  `learner_rows` writes rows whose scales are powers
of two (FORMS: one row of n = 1; three rows (G, G, 2 G) of n = (1, 1, 2), whose ordered sum 4 G is exact; one "reference"
row of n = 2 with sum.delta = 4), and `finalize32` is the finalize arithmetic in float32, so the gradient adam_element
receives is known to the bit, the sign of a zero included.

Element classes, dealt round-robin over the flat blob (so every tensor longer than six holds every class and both sides
of every tensor boundary carry different ones); the deal is rotated from case to case:
    typical   g, m of order 1e-2, v of order 1e-4
    tiny      g, m of order 1e-8, v of order 1e-16: sqrt(v) is near eps, where the place of eps shows
    momentum  g = 0 (+0 and -0 in the rows), m, v != 0
    still     g = m = v = 0: w' is w's bits
    cancel    m = -g / 9 to within two ulp: the new exp_avg is a rounding remainder
    big       |g|, |m| up to 1e15, v up to 1e30
    cold      v = 0, g = 0, m != 0: the denominator is eps alone
Parameters w cycle through 0, order 1, order 1e6, order 1e-2 and order 1 again: a period of five, coprime to the classes'.

Loaded steps.  STEPS interleaves small, middle and saturated counts (from sqrt(bc2) == 1.0f on, about 16 600 steps, the
step no longer matters); every tensor gets its own value, neighbours a small or middle one on at least one side, and
every (H, A) another window of the list (`loaded_steps`).  The kernel executes step s0 + 1.  A step at which lr / bc1 or
sqrt(bc2) lies within 2^-44 relative of a float32 rounding boundary is replaced by its neighbour (`safe_step`): a
last-place difference of the device's fp64 pow, sqrt or division from numpy's cannot then move the float32 value.  One
step of the list does not qualify: at step 1 with lr = 5e-3, (double)0.005f / (1 - 0.9) lies 2^-52 relative from a tie, so
a critic tensor dealt s0 = 0 starts at 1 instead (an actor tensor starts fresh in two shapes; a fresh critic tensor runs
in test_hip_adam.py's checkpoint test, learner against learner).

The metric.  Per element, S is the sum of the absolute terms of the word's defining sum,
    S_m = 0.9 |m| + 0.1 |g|        S_v = 0.999 v + 0.001 g^2        S_w = (lr / bc1) S_m / denom64
    e_m = |m' - m'64| / S_m        e_v = |v' - v'64| / S_v          e_w = max(|w' - w'64| - ulp32(w'64) / 2, 0) / S_w
with denom64 = sqrt(v'64) / sqrt(bc2) + 1e-8.  Where S = 0 any difference is infinite.  S_w is built from the absolute
terms, not from |w - w'|, which is a rounding remainder where m and g cancel.

Tolerances are never measured on the device.  WORST[family][class][word] is the largest error of restate32 against the
fp64 reference over the CPU grid (`measure`; `python tests/adam_cases.py` reprints it) and a tolerance is TOL_FACTOR = 4
times the entry.  Family "given" is the learner grid with each class's own gradient; family "net" keeps the classes'
(m, v) and draws |g| log-uniformly from [1e-12, 1], which is what the PMI trainer's test meets: there the gradient is the
network's and cannot be injected.  In units of u = 2^-24 (x86-64, numpy), worst over the grid:

    given     typical     tiny momentum    still   cancel      big     cold
    m            1.55     1.31     1.00     0.00     1.11     2.77     1.00
    v            2.09     2.11     1.21     0.00     2.15     3.40     0.00
    w            3.71     3.51     3.21     0.00     1.10     3.46     2.49

    net       typical     tiny momentum    still   cancel      big     cold
    m            2.16     2.81     1.92     1.20     2.54     1.00     2.77
    v            2.53     3.39     2.47     2.66     2.60     1.21     2.73
    w            4.00     5.00     3.86     3.80     3.65     3.02     4.94
"""
import types

import numpy as np

import learner_mirror
import pmi_gradient_cases as pc
import pmi_trainer_mirror

F32 = np.float32
U32 = 2.0 ** -24
TOL_FACTOR = 4.0
MUTANT_ROOM = pc.MUTANT_ROOM
LRS = (1e-3, 5e-3)                       # the learner's (actor, critic); the PMI trainer's is pc.LR
SHAPES = ((1, 1), (33, 9), (128, 12), (256, 48))
FORMS = ("one_row", "three_rows", "reference")
CLASSES = ("typical", "tiny", "momentum", "still", "cancel", "big", "cold")
WORDS = ("m", "v", "w")
# small, middle and saturated loaded steps, interleaved: no two saturated ones are neighbours, cyclically
STEPS = (0, 65536, 1, 10 ** 7, 2, 2 ** 31 - 1, 9, 2 ** 31, 99, 2 ** 40, 999, 6930)
SMALL, MIDDLE = (0, 1, 2, 9), (99, 999, 6930)
BOUNDARY_MARGIN = 2.0 ** -44
MIN_NORMAL = 2.0 ** -126
PMI_CASES = ((1, 2), (43, 65))           # of pc.GRID: the fewest rows; an H that is no multiple of 64


# ---- the float32 reading of adam_element -----------------------------------------------------------------------------

def lr32(lr):
    """The learning rate as the handle holds it (a C float), as a Python double."""
    return float(F32(lr))


def scalars64(step, lr):
    """(lr / bc1, sqrt(bc2)) in float64 at Adam step `step` (already advanced), lr as the handle's float."""
    s = np.asarray(step, np.int64).astype(np.float64)
    lr = np.asarray(lr, F32).astype(np.float64)
    with np.errstate(under="ignore", divide="ignore"):
        bc1, bc2 = 1.0 - np.power(0.9, s), 1.0 - np.power(0.999, s)
        return lr / bc1, np.sqrt(bc2)


def trace32(w, m, v, g, step, lr):
    """Every fp32 value adam_element forms, by name, in its order; step and lr per element or scalar."""
    w, m, v, g = (np.asarray(x, F32) for x in (w, m, v, g))
    a64, b64 = scalars64(step, lr)
    t = {"step_size": np.asarray(a64).astype(F32), "bc2_sqrt": np.asarray(b64).astype(F32)}
    c1, c2, d2, eps = F32(0.1), F32(0.001), F32(0.999), F32(1e-8)
    with np.errstate(all="ignore"):
        t["g_m"] = g - m
        t["lerp"] = c1 * t["g_m"]
        t["m"] = m + t["lerp"]
        t["v_decay"] = v * d2
        t["c2_g"] = c2 * g
        t["c2_g_g"] = t["c2_g"] * g
        t["v"] = t["v_decay"] + t["c2_g_g"]
        t["root"] = np.sqrt(t["v"])
        t["root_bc"] = t["root"] / t["bc2_sqrt"]
        t["denom"] = t["root_bc"] + eps
        t["ratio"] = t["m"] / t["denom"]
        t["move"] = t["step_size"] * t["ratio"]
        t["w"] = w - t["move"]
    assert all(x.dtype == F32 for x in t.values())
    return t


def restate32(w, m, v, g, step, lr):
    """(w', m', v') of adam_element in numpy float32."""
    t = trace32(w, m, v, g, step, lr)
    return t["w"], t["m"], t["v"]


CHAIN = dict(H=33, A=9, rot=5, form="three_rows", count=3)      # test_hip_adam.py's chain of applies


def chain32(c, g, count):
    """[(w, m, v)] after 1 .. count steps of the same gradient g from the case's loaded state."""
    out, (w, m, v) = [], (c.w, c.m, c.v)
    for k in range(count):
        w, m, v = restate32(w, m, v, g, c.step + k, c.lr)
        out.append((w, m, v))
    return out


def boundary_distance(x64):
    """The relative distance of float64 x from the nearest point at which its float32 rounding changes (the midpoint
    of two neighbouring float32 values)."""
    x64 = np.asarray(x64, np.float64)
    r = x64.astype(F32)
    up, down = np.nextafter(r, F32(np.inf)).astype(np.float64), np.nextafter(r, F32(-np.inf)).astype(np.float64)
    r = r.astype(np.float64)
    return np.minimum(np.abs(0.5 * (r + up) - x64), np.abs(0.5 * (r + down) - x64)) / np.abs(x64)


def step_is_safe(step, lrs):
    return all(float(boundary_distance(x)) >= BOUNDARY_MARGIN for lr in lrs for x in scalars64(step, lr))


def safe_step(s0, lrs, used=()):
    """s0, or the nearest s0 + k not in `used` whose executed step s0 + k + 1 keeps both scalars clear of a rounding
    boundary."""
    s0 = int(s0)
    while s0 in used or not step_is_safe(s0 + 1, lrs):
        s0 += 1
    return s0


# where each case's window of STEPS begins: with these four every learner tensor meets a small, a middle and a saturated
# step somewhere in the grid, and an actor tensor starts fresh (s0 = 0) in two of them
LEARNER_WINDOWS = (4, 5, 9, 10)
PMI_WINDOWS = (0, 6)


def loaded_steps(first, lrs):
    """One distinct loaded step per tensor (lrs: each tensor's learning rate): the window of STEPS that begins at
    `first` (a second pass adds 4), each value made safe at its own tensor's learning rate."""
    n, out = len(STEPS), []
    for t, lr in enumerate(lrs):
        out.append(safe_step(STEPS[(first + t) % n] + 4 * (t // n), (lr,), out))
    assert len(set(out)) == len(lrs), out
    return np.array(out, np.int64)


# ---- the element classes ---------------------------------------------------------------------------------------------

def deal(offs, rot, rng):
    """(class index [P], w, m, v, g) as float32: the classes dealt round-robin from rotation `rot` over the tensors that
    begin at offs[:-1]; a tensor whose two ends would carry one class has its last two elements trade theirs."""
    P = int(offs[-1])
    cls = (np.arange(P) + rot) % len(CLASSES)
    for a, b in zip(offs[:-1], offs[1:]):
        if b - a > 2 and cls[a] == cls[b - 1]:
            cls[b - 2], cls[b - 1] = cls[b - 1], cls[b - 2]
    sign = lambda: rng.choice([-1.0, 1.0], size=P)
    mant = lambda: rng.uniform(0.3, 3.0, size=P)
    is_ = lambda name: cls == CLASSES.index(name)
    g, m, v = np.zeros(P), np.zeros(P), np.zeros(P)
    for name, sg, sv in (("typical", 1e-2, 1e-4), ("tiny", 1e-8, 1e-16)):
        k = is_(name)
        g[k], m[k], v[k] = (sign() * mant() * sg)[k], (sign() * mant() * sg)[k], (mant() * sv)[k]
    k = is_("momentum")
    m[k], v[k] = (sign() * mant() * 1e-2)[k], (mant() * 1e-4)[k]
    k = is_("big")
    g[k], m[k] = (sign() * 10.0 ** rng.uniform(9, 15, size=P))[k], (sign() * 10.0 ** rng.uniform(9, 15, size=P))[k]
    v[k] = (10.0 ** rng.uniform(18, 30, size=P))[k]
    k = is_("cold")
    m[k] = (sign() * 10.0 ** rng.uniform(-5, -2, size=P))[k]
    g, m, v = g.astype(F32), m.astype(F32), v.astype(F32)
    k = is_("cancel")
    gc = (sign() * mant() * 1e-2).astype(F32)
    mc = (-gc / F32(9.0)).astype(F32)
    nudge = rng.randint(-2, 3, size=P)
    mc = (mc.view(np.int32) + nudge.astype(np.int32)).view(F32)           # a few ulp either way
    g[k], m[k], v[k] = gc[k], mc[k], (mant() * 1e-4).astype(F32)[k]
    wc = np.arange(P) % 5
    w = np.select([wc == 0, wc == 1, wc == 2, wc == 3], [np.zeros(P), sign() * mant(), sign() * mant() * 1e6,
                                                         sign() * mant() * 1e-2], -mant()).astype(F32)
    return cls, w, m, v, g


def net_gradient(P, rng):
    """What a network's gradient looks like to the step: |g| log-uniform over [1e-12, 1], either sign."""
    return (rng.choice([-1.0, 1.0], size=P) * 10.0 ** rng.uniform(-12, 0, size=P)).astype(F32)


def _per_element(sizes, values):
    return np.concatenate([np.full(n, x) for n, x in zip(sizes, values)])


def learner_case(H, A, rot=0, family="given"):
    """The learner's case at (H, A): cls, w, m, v, g (float32 [P]), s0 [8], and per element step (s0 + 1) and lr.  A
    shape outside SHAPES takes the first window of steps."""
    k = SHAPES.index((H, A)) if (H, A) in SHAPES else 0
    sizes, offs = learner_mirror.layout(H, A)
    P = int(offs[-1])
    rng = np.random.RandomState(1000 * H + 10 * A + rot)
    cls, w, m, v, g = deal(offs, rot, rng)
    if family == "net":
        g = net_gradient(P, rng)
    s0 = loaded_steps(LEARNER_WINDOWS[k], [LRS[0]] * 4 + [LRS[1]] * 4)
    return types.SimpleNamespace(H=H, A=A, P=P, na=int(offs[4]), sizes=sizes, offs=offs, cls=cls, w=w, m=m, v=v, g=g,
                                 s0=s0, step=_per_element(sizes, s0 + 1),
                                 lr=_per_element(sizes, [LRS[0]] * 4 + [LRS[1]] * 4), lrs=LRS)


def pmi_sizes(H):
    shapes = pc.param_shapes(H)
    return [int(np.prod(shapes[k])) for k in pmi_trainer_mirror.param_names()]


def pmi_case(H, B, rot=0):
    """The PMI trainer's loaded state at pc.build_case(H, B): class-dealt (m, v) and 18 distinct s0; g is a stand-in
    (net_gradient) for the CPU grid, the device's own recovered gradient replaces it in the GPU test."""
    k = PMI_CASES.index((H, B)) if (H, B) in PMI_CASES else 0
    sizes = pmi_sizes(H)
    P = sum(sizes)
    rng = np.random.RandomState(77000 + 100 * H + B + rot)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    cls, w, m, v, _ = deal(offs, rot, rng)
    s0 = loaded_steps(PMI_WINDOWS[k], [pc.LR] * 18)
    return types.SimpleNamespace(H=H, B=B, P=P, sizes=sizes, offs=offs, cls=cls, w=w,
                                 m=m, v=v, g=net_gradient(P, rng), s0=s0, step=_per_element(sizes, s0 + 1),
                                 lr=np.full(P, pc.LR), lrs=(pc.LR,))


# ---- the fp64 reference ----------------------------------------------------------------------------------------------

def fp64_learner(c, w=None, m=None, v=None, g=None, s0=None):
    """(w', m', v') in float64 through learner_mirror.adam from the case's (or the given) state."""
    pick = lambda x, d: np.asarray(d if x is None else x, np.float64)
    step = np.asarray(c.s0 if s0 is None else s0, np.int64) + 1
    with np.errstate(under="ignore"):
        return learner_mirror.adam(pick(w, c.w), pick(m, c.m), pick(v, c.v), step, pick(g, c.g),
                                   tuple(lr32(x) for x in c.lrs), c.H, c.A)


def fp64_pmi(c, w=None, m=None, v=None, g=None, s0=None):
    """(w', m', v') flat in float64 through pmi_trainer_mirror.adam_step from the case's (or the given) state."""
    pick = lambda x, d: np.asarray(d if x is None else x, np.float64)
    names = pmi_trainer_mirror.param_names()
    s0 = c.s0 if s0 is None else s0
    sd = dict(pc.split_params(pick(w, c.w), c.H))
    adam = {"exp_avg": dict(pc.split_params(pick(m, c.m), c.H)), "exp_avg_sq": dict(pc.split_params(pick(v, c.v), c.H)),
            "step": {k: int(s) for k, s in zip(names, s0)}}
    pmi_trainer_mirror.adam_step(sd, adam, pc.split_params(pick(g, c.g), c.H), lr32(c.lrs[0]))
    cat = lambda d: np.concatenate([np.asarray(d[k], np.float64).ravel() for k in names])
    assert [adam["step"][k] for k in names] == [int(s) + 1 for s in s0]
    return cat(sd), cat(adam["exp_avg"]), cat(adam["exp_avg_sq"])


# ---- the metric ------------------------------------------------------------------------------------------------------

def scales(m, v, g, v_new64, step, lr):
    """{word: S [P]} in float64; v_new64 is the fp64 reference's v'."""
    m, v, g = (np.abs(np.asarray(x, np.float64)) for x in (m, v, g))
    a, b = scalars64(step, lr)
    S_m = 0.9 * m + 0.1 * g
    return {"m": S_m, "v": 0.999 * v + 0.001 * g * g, "w": a * S_m / (np.sqrt(v_new64) / b + 1e-8)}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


def element_errors(got, ref, S, slack=None):
    """{word: e [P]}: got and ref are (w', m', v') triples; slack {word: [P]} is subtracted from the difference."""
    out = {}
    for word, i in (("m", 1), ("v", 2), ("w", 0)):
        with np.errstate(invalid="ignore"):
            d = np.abs(np.asarray(got[i], np.float64) - np.asarray(ref[i], np.float64))
        d = np.where(np.isnan(d), np.inf, d)                               # a NaN is infinitely wrong
        if word == "w":
            d = np.maximum(d - 0.5 * ulp32(ref[0]), 0.0)
        if slack is not None:
            d = np.maximum(d - slack[word], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[word] = np.where(S[word] > 0, d / S[word], np.where(d > 0, np.inf, 0.0))
    return out


def class_errors(e, cls):
    """{class: {word: max over the class's elements}} (0 where a class has no element)."""
    return {name: {word: float(e[word][cls == k].max()) if (cls == k).any() else 0.0 for word in WORDS}
            for k, name in enumerate(CLASSES)}


def case_errors(c, got, ref, slack=None):
    return class_errors(element_errors(got, ref, scales(c.m, c.v, c.g, ref[2], c.step, c.lr), slack), c.cls)


def recovery_slack(c, g, ref):
    """What one rounding of a recovered gradient may move the fp64 reference by.  The gradient read off a trainer that
    started from zero is g' = exp_avg / 0.1f = g (1 + d), |d| <= u = 2^-24 (pc.recovered_gradient).  With g' for g,
    m' = 0.9 m + 0.1 g moves by 0.1 |g| u and v' = 0.999 v + 0.001 g^2 by 0.001 g^2 (2 d + d^2) <= 0.002 g^2 u to first
    order, plus 2^-126 absolute where 0.001f g^2 leaves the normal range on the device; w' = w - a m' / (sqrt(v') / b + eps)
    moves by their image, a (dm / denom + |m'| (sqrt(v') - sqrt(v' - dv)) / (b denom^2))."""
    g = np.abs(np.asarray(g, np.float64))
    a, b = scalars64(c.step, c.lr)
    dm, dv = U32 * 0.1 * g, U32 * 0.002 * g * g + MIN_NORMAL
    v_new, m_new = np.asarray(ref[2], np.float64), np.abs(np.asarray(ref[1], np.float64))
    denom = np.sqrt(v_new) / b + 1e-8
    droot = np.sqrt(v_new) - np.sqrt(np.maximum(v_new - dv, 0.0))
    return {"m": dm, "v": dv, "w": a * (dm / denom + m_new * droot / (b * denom * denom))}


# ---- gradient rows ---------------------------------------------------------------------------------------------------

ROW_TAIL = 8


def make_rows(sums, loss, n, status, tag):
    """[count, P + 8] float32 gradient rows from sums [count, P], loss sums [count, 4], and per row n (int64, split
    into two int32 words), the status bits and the layout tag (P for a row of this learner)."""
    sums = np.asarray(sums, F32)
    count, P = sums.shape
    rows = np.empty((count, P + ROW_TAIL), F32)
    rows[:, :P] = sums
    rows[:, P:P + 4] = np.asarray(loss, F32).reshape(count, 4)
    tail = rows.view(np.int32)[:, P + 4:]
    n = np.asarray(n, np.int64).reshape(count).astype(np.uint64)
    tail[:, 0] = (n & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    tail[:, 1] = (n >> np.uint64(32)).astype(np.uint32).view(np.int32)
    tail[:, 2] = np.asarray(status, np.int32).reshape(count)
    tail[:, 3] = np.asarray(tag, np.int32).reshape(count)
    return rows


def read_tail(row):
    """(n, status, P) of one gradient row, read as the finalize kernel reads it."""
    t = np.ascontiguousarray(np.asarray(row, F32).reshape(-1)[-4:]).view(np.uint32)
    return int(t[0]) | (int(t[1]) << 32), int(t[2].view(np.int32)), int(t[3].view(np.int32))


# loss sums (sum.nlp, sum.delta, sum.actor, sum.critic) of the rows: arbitrary exact values; "reference" needs sum.delta = 4
_LOSS = {"one_row": [[0.75, -1.5, 0.625, 2.25]],
         "three_rows": [[0.75, -1.5, 0.625, 2.25], [0.5, 0.25, -0.375, 1.0], [1.25, 2.0, 0.125, 0.5]],
         "reference": [[0.75, 4.0, 0.625, 2.25]]}
_N = {"one_row": [1], "three_rows": [1, 1, 2], "reference": [2]}
_PARTS = {"one_row": [1.0], "three_rows": [1.0, 1.0, 2.0], "reference": [1.0]}


def form_loss(form):
    return "reference" if form == "reference" else "per_sample"


def learner_rows(c, form, status=0, tag=None, n=None):
    """The rows of `form` that hand adam_element the case's g: the actor's sums are -g (scale -1, -1/4 of 4 G, or
    -mean_delta / N = -1), the critic's g / 2 (scales 2 and 1/2 of 4 G) or g ("reference": 2 / N = 1).  A zero takes
    either sign, alternating along the row."""
    g64 = c.g.astype(np.float64)
    G = np.where(np.arange(c.P) < c.na, -g64, g64 * (1.0 if form == "reference" else 0.5))
    zero = c.g == 0
    G[zero] = np.where(np.arange(c.P) % 2 == 0, 0.0, -0.0)[zero]
    parts = _PARTS[form]
    sums = np.stack([(G * x).astype(F32) for x in parts])
    assert np.array_equal(sums.astype(np.float64), np.stack([G * x for x in parts]))      # exact in fp32
    count = len(parts)
    return make_rows(sums, _LOSS[form], _N[form] if n is None else n, np.full(count, status),
                     np.full(count, c.P if tag is None else tag))


def finalize32(rows, P, na, per_sample):
    """learner_finalize_kernel and the Adam kernel's gradient in float32: (actor_loss, critic_loss, g [P])."""
    rows = np.asarray(rows, F32).reshape(-1, P + ROW_TAIL)
    N = sum(read_tail(r)[0] for r in rows)
    total = np.zeros(P + 4, F32)
    for r in rows:
        total = total + r[:P + 4]                                        # 0.0f + x first, rows ascending
    s = total[P:]
    inv_n = F32(1.0) / F32(N)
    mean_nlp, mean_delta = s[0] * inv_n, s[1] * inv_n
    al = s[2] * inv_n if per_sample else mean_nlp * mean_delta
    cl = s[3] * inv_n
    scal = (-inv_n if per_sample else -mean_delta * inv_n, F32(2.0) * inv_n)
    g = np.concatenate([total[:na] * scal[0], total[na:P] * scal[1]])
    assert g.dtype == F32
    return F32(al), F32(cl), g


# ---- tolerances ------------------------------------------------------------------------------------------------------

# WORST[family][class][word]: restate32 against the fp64 reference, worst over the CPU grid (measure())
WORST = {
    "given": {
        "typical": {"m": 9.24e-08, "v": 1.24e-07, "w": 2.21e-07},
        "tiny": {"m": 7.79e-08, "v": 1.26e-07, "w": 2.09e-07},
        "momentum": {"m": 5.96e-08, "v": 7.21e-08, "w": 1.92e-07},
        "still": {"m": 0.00e+00, "v": 0.00e+00, "w": 0.00e+00},
        "cancel": {"m": 6.60e-08, "v": 1.28e-07, "w": 6.58e-08},
        "big": {"m": 1.65e-07, "v": 2.02e-07, "w": 2.06e-07},
        "cold": {"m": 5.96e-08, "v": 0.00e+00, "w": 1.48e-07},
    },
    "net": {
        "typical": {"m": 1.29e-07, "v": 1.51e-07, "w": 2.38e-07},
        "tiny": {"m": 1.67e-07, "v": 2.02e-07, "w": 2.98e-07},
        "momentum": {"m": 1.14e-07, "v": 1.47e-07, "w": 2.30e-07},
        "still": {"m": 7.15e-08, "v": 1.58e-07, "w": 2.27e-07},
        "cancel": {"m": 1.52e-07, "v": 1.55e-07, "w": 2.18e-07},
        "big": {"m": 5.96e-08, "v": 7.22e-08, "w": 1.80e-07},
        "cold": {"m": 1.65e-07, "v": 1.63e-07, "w": 2.95e-07},
    },
}


def tolerance(family):
    """{class: {word: tolerance}}: TOL_FACTOR times the CPU grid's worst."""
    return {k: {w: TOL_FACTOR * x for w, x in t.items()} for k, t in WORST[family].items()}


def over(e, tol):
    """The (class, word) entries of e beyond their tolerance: {(class, word): (error, tolerance)}."""
    return {(k, w): (e[k][w], tol[k][w]) for k in e for w in e[k] if not e[k][w] <= tol[k][w]}


def report(tag, e, tol):
    """Every figure in units of u, with its share of the tolerance."""
    share = lambda x, t: x / t if t > 0 else float(x > 0)
    print(tag, " ".join(f"{k}.{w}={e[k][w] / U32:.2f}u/{share(e[k][w], tol[k][w]):.2f}" for k in e for w in WORDS))


def grid():
    """[(family, case, fp64 function)] of the CPU grid: every learner shape under every rotation of the deal in both
    families, and the PMI cases' layouts under every rotation."""
    out = []
    for rot in range(len(CLASSES)):
        for H, A in SHAPES:
            out += [(family, learner_case(H, A, rot, family), fp64_learner) for family in ("given", "net")]
        out += [("net", pmi_case(H, B, rot), fp64_pmi) for H, B in PMI_CASES]
    return out


def merge_worst(table, e):
    for k in e:
        for w in e[k]:
            table[k][w] = max(table[k][w], e[k][w])


def measure():
    """{family: {class: {word: worst}}} of restate32 against the fp64 reference over grid()."""
    worst = {f: {k: {w: 0.0 for w in WORDS} for k in CLASSES} for f in ("given", "net")}
    for family, c, fp64 in grid():
        merge_worst(worst[family], case_errors(c, restate32(c.w, c.m, c.v, c.g, c.step, c.lr), fp64(c)))
    return worst


if __name__ == "__main__":
    worst = measure()
    print("WORST = {")
    for f, t in worst.items():
        print(f'    "{f}": {{')
        for k, row in t.items():
            print(f'        "{k}": {{' + ", ".join(f'"{w}": {x:.2e}' for w, x in row.items()) + "},")
        print("    },")
    print("}")
    for f, t in worst.items():
        print(f"    {f:<8}" + "".join(f"{k:>9}" for k in CLASSES))
        for w in WORDS:
            print(f"    {w:<8}" + "".join(f"{t[k][w] / U32:>9.2f}" for k in CLASSES))
        print()
