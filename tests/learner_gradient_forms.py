"""The element-wise gradient comparison of tests/learner_gradient_cases.py for the ten gradient kernels its seven bodies do
not reach: learner_grad_clip{,_target}, _adv{,_target}, _adv_clip{,_target}, _stored{,_target}, _stored_clip{,_target}
(csrc/learner_variants.h).  Same metric, same rule for tolerances (never from the device), same mutant discipline; the
cases, the float64 side and the tolerance tables of the forms live here, the two fp32 references are
learner_gradient_cases.torch_fp32 / sequential_fp32, which take a form case as they take any other.  Used by
test_learner_gradients_cpu.py (no GPU) and test_hip_learner_gradient_forms.py.

A case is a per-sample `Spec` case (its body brings importance weights, per-slot discounts, a target critic, c in
{0, 0.1}) plus a form: clip in {None, 0.2, inf}; adv in {"raw", "given", "batch"}; stored or not; inv0, the one `given`
case whose inv_std is 0.  `kernel_of` restates learner_grad_variant.

Inputs are dealt, not drawn, by batch row k (an index vector names no slot twice, so a slot has one row):
  log_mu[slot] = float32(min(log p64 + OFFS[k % 8], 0)): ratios of 0.95, 1.16, 0.67, 1.49, 1.05, 0.86, 1.49, 0.67;
  the advantage's sign from `dealt_signs`, which puts a non-negative advantage on every row k % 8 == 3 (ratio above) and,
  in even blocks of eight, on k % 8 == 6, a negative one on every row k % 8 == 2 (ratio below) and, in odd blocks, on
  k % 8 == 7, and both signs on the rest: each of the four gate cells at eps = 0.2 (adv >= 0 passes / is clipped, adv < 0
  passes / is clipped) holds at least n / 8 rows from n = 16 on (asserted: a random deal gave (13, 0, 4, 0) at n = 17);
  its size from MAGS (|t| in [0.4, 0.9] or [1.6, 2.5]: the gap around zero is the widest).
Without a store the advantage is delta, so the rewards are solved for: delta_k = CENTRE + t_k in float64 at the case's
parameters, CENTRE 0 for raw, 1.25 for given and 3 for batch (a critic that is wrong by about 3, as
learner_advantage_mirror's cases: under batch every row of negative advantage has a positive delta, so a gate that reads
delta's sign shows).  |delta| >= 0.35 > MIN_DELTA in every case.  With a store the rewards stay the Spec case's (delta
and the advantage are unrelated) and advantages[slot] = float32(shift + t_k), shift 0 for raw and 1.25 otherwise; in
stored raw cases the rows k % 16 == 0 hold +0.0 and row 1 holds -0.0 (they contribute exactly nothing; -0 goes to the
`hi` side).  Under batch the positive sizes are scaled so that the t_k sum to zero, and the sign of the standardised
advantage is the dealt one.  Slots outside the batch hold NaN in log_mu and advantages.  given = (the middle of the
gap at the median of the advantages' sources -- the widest near it; a window of several values either side finds the
gaps between the sizes of a small batch instead --, 0.37).

Conditions, asserted for every case by the CPU test: learner_gradient_cases.margin; |delta| >= MIN_DELTA; no advantage
within MIN_ADV = 0.05 of zero but the designed zeros, and MIN_ADV at least 16 times the largest |A_fp32 - A_fp64| of a
numpy float32 forward (measured: at most 3.8e-7); no float64 ratio within 16 times the largest |ratio32 - ratio64| of a
clip bound (measured: the worst relative ratio error 8.8e-7 outside the peaked class, the nearest ratio 1.5e-2 from a bound);
both fp32 references take the float64 gate decision on every row; the four cells; the sign census under batch.

The float64 side (`fp64`): learner_mirror.forward, the advantage as learner_advantage_mirror forms it (the float32
source, fl(fl(x - mean) * inv_std)), learner_mirror.terms(clip=) with the advantage in delta's place, loss word 1 put back
to the raw sum w delta, learner_mirror.backward.  A batch form takes its statistics as an argument: the CPU test passes
stats32 of the mirror's float32 deltas (or of the store), the GPU test the device's own advantage_stats[:2], so that the
gradient kernel is judged apart from the statistics kernels.

The scale of a logit weight.  gz_o = w (k (onehot - p)_o - c p_o (log p_o + H)); on a clipped row k = 0 and the
entropy part stands alone, where log p_o + H cancels: a unit that is on in one such row gave the sequential fp32
reference 4.5e-4 of S in the actor's fc2.weight (H 128, A 12, n 65, c = 0.1), every other tensor at most 7e-7.  S sees the
terms of a sum, not how a term was formed, so in these cases every row's scale counts the entropy part by its absolute
parts: |gz|_o = w (|k| |onehot - p|_o + c p_o (|log p_o| + H)).  What the references then measure is in the tables below.

Tolerances: FORM_WORST_ROW / FORM_WORST_GRAD, per class (learner_gradient_cases.case_class: two, few, mid, large,
peaked) and word the larger of the two fp32 CPU references' worst error over FORM_GRID; a tolerance is TOL_FACTOR = 4
times the entry.  Measured on x86-64 by `python tests/learner_gradient_cases.py --forms`."""
import collections
import functools
import types

import numpy as np

import learner_advantage_mirror as am
import learner_gradient_cases as lg
import learner_mirror as mirror

F32 = np.float32
OFFS = (0.05, -0.15, 0.4, -0.4, -0.05, 0.15, -0.4, 0.4)
MAGS = (0.4, 1.7, 0.55, 2.3, 0.8, 1.9, 0.45, 2.45, 0.7, 1.6, 0.9)
EPS = 0.2
INV_GIVEN = 0.37
CENTRE = {"raw": 0.0, "given": 1.25, "batch": 3.0}
MIN_ADV = 0.05
CLASSES = ("two", "few", "mid", "large", "peaked")
POINTS = ((33, 9, 125), (128, 12, 65), (256, 48, 4113))

Form = collections.namedtuple("Form", "H A n body gather cls clip adv stored inv0")

# kernel -> (clip, a normalised advantage, stored, target), and the rule of learner_variants.h restated
NEW_KERNELS = {
    "learner_grad_clip_kernel": (1, 0, 0, 0), "learner_grad_clip_target_kernel": (1, 0, 0, 1),
    "learner_grad_adv_kernel": (0, 1, 0, 0), "learner_grad_adv_target_kernel": (0, 1, 0, 1),
    "learner_grad_adv_clip_kernel": (1, 1, 0, 0), "learner_grad_adv_clip_target_kernel": (1, 1, 0, 1),
    "learner_grad_stored_kernel": (0, 0, 1, 0), "learner_grad_stored_target_kernel": (0, 0, 1, 1),
    "learner_grad_stored_clip_kernel": (1, 0, 1, 0), "learner_grad_stored_clip_target_kernel": (1, 0, 1, 1),
}
OLD_KERNELS = ("learner_grad_kernel", "learner_grad_reg_kernel", "learner_grad_target_kernel",
               "learner_grad_reg_target_kernel")


def kernel_name(reg, target, log_mu, adv, stored):
    """learner_grad_variant: stored advantages choose by (target, log_mu) whatever reg and adv are; else a normalised
    advantage by (log_mu, target) whatever reg is; else log_mu by target; else one of the first four by (reg, target)."""
    t = "_target" if target else ""
    if stored:
        return f"learner_grad_stored{'_clip' if log_mu else ''}{t}_kernel"
    if adv:
        return f"learner_grad_adv{'_clip' if log_mu else ''}{t}_kernel"
    if log_mu:
        return f"learner_grad_clip{t}_kernel"
    return f"learner_grad{'_reg' if reg else ''}{t}_kernel"


def _flags(body):
    """(reg, target) of a body: the entropy term or the installed entropy buffer; a target critic."""
    return body in ("reg0", "regc", "all"), body in ("target", "all")


def kernel_of(fs):
    """The kernel a Form takes, or a Spec of the old grid (no log_mu, a raw advantage, no store)."""
    form = isinstance(fs, Form)
    return kernel_name(*_flags(fs.body), form and fs.clip is not None, form and fs.adv != "raw", form and fs.stored)


def base_spec(fs):
    return lg.Spec(fs.H, fs.A, fs.n, "per_sample", fs.body, fs.gather, fs.cls, False, None, False)


def form_class(fs):
    return lg.case_class(base_spec(fs))


CRITIC_WORDS = lg.CRITIC + ("sum.delta", "sum.critic")


def word_class(fs, word):
    """The class a word of a case is judged in: the case's own, but the critic's words of a peaked case by its n alone.
    Peaked scales the actor's fc2 and nothing else: the critic's tensors, sum w delta and sum w (V - y)^2 are the
    same function of the same inputs as in a default case of that size, and a class of four cases of 65 to 4113 rows
    would judge the largest by what the smallest measured."""
    if word in CRITIC_WORDS:
        return lg.case_class(base_spec(fs)._replace(cls="default"))
    return form_class(fs)


def form_id(fs):
    return (f"H{fs.H}-A{fs.A}-n{fs.n}-{fs.body}" + ("-indexed" if fs.gather else "") +
            ("-peaked" if fs.cls == "peaked" else "") + ("" if fs.clip is None else f"-clip{fs.clip}") + f"-{fs.adv}" +
            ("-stored" if fs.stored else "") + ("-inv0" if fs.inv0 else ""))


def _form_grid():
    out, seen = [], set()

    def add(H, A, n, body, gather, clip, adv, stored, cls="default", inv0=False):
        fs = Form(H, A, n, body, gather, cls, clip, adv, stored, inv0)
        if fs not in seen:
            seen.add(fs)
            out.append(fs)

    plain_bodies, target_bodies = ("weighted", "regc", "discounted", "plain", "reg0"), ("target", "all")
    for q, (clip, adv, stored, target) in enumerate(NEW_KERNELS.values()):          # every kernel at the three points
        for p, (H, A, n) in enumerate(POINTS):
            body = target_bodies[(q + p) % 2] if target else plain_bodies[(q + p) % 5]
            mode = ("raw", "given", "batch")[(q + p) % 3] if stored else ("given", "batch")[(q + p) % 2] if adv else "raw"
            add(H, A, n, body, (q + p) % 2 == 1, (EPS, EPS, np.inf)[(q + p) % 3] if clip else None, mode, bool(stored))
    # the largest LDS footprint (lds_extra 2) and the clip kernel (lds_extra 1): every width at R + 1, two widths
    # against every n where the body changes path; k deals the action count, body, batch form, clip and mode
    k = 3 * len(NEW_KERNELS)
    for kernel in ("learner_grad_stored_clip_target_kernel", "learner_grad_clip_kernel"):
        stored = kernel.startswith("learner_grad_stored")
        bodies = target_bodies if stored else plain_bodies
        shapes = [(H, lg.rows_per_tile(H) + 1) for H in lg.HS]
        for H in (200, 256):
            R = lg.rows_per_tile(H)
            shapes += [(H, n) for n in (2, R - 1, R, R + 1, 2 * R + 1, 256 * R + 1)]
        for H, n in shapes:
            mode = "raw" if not stored else "batch" if n == 2 else ("raw", "given", "batch")[k % 3]
            add(H, (12, 48, 9)[k % 3], n, bodies[k % len(bodies)], k % 2 == 1, (EPS, np.inf, EPS, EPS)[k % 4], mode, stored)
            k += 1
    add(32, 12, 2, "plain", False, None, "batch", False)        # the smallest legal batch under the batch's own statistics
    add(33, 9, 2, "regc", True, EPS, "batch", False)
    for A in (1, 2, 48):                                        # action counts under stored + clip; A = 1: S = 0
        add(64, A, 65, "plain" if A != 2 else "regc", A == 48, EPS, ("raw", "given", "batch")[A % 3], True)
    add(128, 12, 65, "plain", True, EPS, "raw", False, cls="peaked")      # a confident policy: the ratios spread widely
    add(33, 9, 125, "weighted", False, EPS, "raw", False, cls="peaked")
    add(16, 12, 257, "all", True, EPS, "batch", True, cls="peaked")
    add(256, 48, 4113, "regc", False, EPS, "given", False, cls="peaked")
    add(64, 12, 65, "weighted", True, EPS, "given", False, inv0=True)
    return out


FORM_GRID = _form_grid()
FORM_TWO_STEP = [Form(256, 48, 33, "all", True, "default", EPS, "given", True, False)]


# ---- the cases

def dealt_signs(n):
    """+1 / -1 per batch row: see the module docstring."""
    k = np.arange(n)
    p, even = k % 8, (k // 8) % 2 == 0
    sg = np.where(np.isin(p, (0, 5)) == even, 1, -1)
    sg = np.where(p == 3, 1, np.where(p == 2, -1, sg))
    sg = np.where(p == 6, np.where(even, 1, -1), sg)
    return np.where(p == 7, np.where(even, 1, -1), sg)


def dealt_sources(n, balanced):
    """t_k = sign_k * size_k in float64; balanced: the positive sizes scaled so that the t_k sum to zero."""
    k = np.arange(n)
    t = dealt_signs(n) * np.array(MAGS)[k % len(MAGS)]
    if balanced:
        t = np.where(t > 0, t * (-t[t < 0].sum() / t[t > 0].sum()), t)
    return t


def median_gap(v):
    """The middle of the gap that holds the median of v; the wider of the two beside it where the median is a value."""
    v = np.unique(np.round(v, 3))           # (solved rewards leave equal sizes a float32 rounding apart)
    m = len(v) // 2
    if len(v) % 2 == 0 or v[m] - v[m - 1] >= v[m + 1] - v[m]:
        return 0.5 * (v[m - 1] + v[m])
    return 0.5 * (v[m] + v[m + 1])


def _build(fs, halves):
    c = lg._build(base_spec(fs), halves, distinct=True)
    H, A, n = fs.H, fs.A, fs.n
    s, a, r, s2 = c.store
    dslot = np.full(c.cap, F32(lg.GAMMA), F32) if c.disc is None else c.disc
    f = mirror.forward(c.blob, H, A, s, a, np.zeros(c.cap), s2, dslot, c.theta)      # f.delta: d V(s') - V(s)
    logp = f.logp[np.arange(c.cap), f.a]
    c.form, c.log_mu, c.advantages, c.given = fs, None, None, None
    if fs.clip is not None:
        c.log_mu = np.full(c.cap, np.nan, F32)
    if fs.stored:
        c.advantages = np.full(c.cap, np.nan, F32)
    r = r.copy()
    for h in range(halves):
        i = c.idx[h]
        t = dealt_sources(n, fs.adv == "batch")
        if fs.clip is not None:
            c.log_mu[i] = np.minimum(logp[i] + np.array(OFFS)[np.arange(n) % 8], 0.0).astype(F32)
        if fs.stored:
            x = ((0.0 if fs.adv == "raw" else CENTRE["given"]) + t).astype(F32)
            if fs.adv == "raw":
                x[::16] = F32(0.0)
                x[1] = -F32(0.0)
            c.advantages[i] = x
        else:
            r[i] = (CENTRE[fs.adv] + t - f.delta[i]).astype(F32)
    c.store = (s, a, r, s2)
    c.rows = tuple(x[c.idx[0]] for x in c.store)
    if fs.adv == "given":
        src = c.advantages[np.concatenate(c.idx)].astype(np.float64) if fs.stored else \
            mirror.forward(c.blob, H, A, s, a, r, s2, dslot, c.theta).delta[np.concatenate(c.idx)]
        c.given = (F32(median_gap(src)), F32(0.0 if fs.inv0 else INV_GIVEN))
    return c


@functools.lru_cache(maxsize=None)
def build_case(fs):
    """learner_gradient_cases.build_case's record plus form (the Form), log_mu and advantages ([cap] float32, NaN outside
    the batch, or None) and given ((mean, inv_std) as float32, or None)."""
    return _build(fs, 1)


@functools.lru_cache(maxsize=None)
def build_two_step_case(fs):
    return _build(fs, 2)


def stripped(c):
    """The same batch without its form: what learner_gradient_cases.fp64 takes."""
    return types.SimpleNamespace(**{**vars(c), "form": None})


# ---- the float64 side

def advantage(c, delta, h=0, stats=None):
    """(A [n] in float64, (mean32, inv32) or None) of batch h, as learner_advantage_mirror forms it from the float32
    source; stats: (mean, inv_std) of a batch form, None for the source's own stats32."""
    fs = c.form
    x = c.advantages[c.idx[h]] if fs.stored else np.asarray(delta, np.float64).astype(F32)
    if fs.adv == "raw":
        return (x.astype(np.float64) if fs.stored else np.asarray(delta, np.float64)), None
    st = c.given if fs.adv == "given" else (am.stats32(x)[:2] if stats is None else stats)
    st = (F32(st[0]), F32(st[1]))
    return am.standardise(x, *st).astype(np.float64), st


def form_terms(c, f, w, adv, log_mu):
    """learner_mirror.terms with the advantage in delta's place and loss word 1 put back; and the logit weights'
    absolute parts."""
    g = types.SimpleNamespace(**{**vars(f), "delta": adv})
    gz, gv, lt, ratio = mirror.terms(g, "per_sample", w, c.c, None if c.form.clip is None else (log_mu, c.form.clip))
    iw = np.ones(f.n) if w is None else np.asarray(w, np.float64)
    lt[1] = f.delta * iw
    ok = np.ones(f.n, bool) if ratio is None else mirror.gate(ratio, adv, c.form.clip)
    k = np.where(ok, (1.0 if ratio is None else ratio) * adv, 0.0)
    agz = iw[:, None] * (np.abs(k)[:, None] * np.abs(f.onehot - f.p) +
                         c.c * np.where(f.p > 0, f.p * (np.abs(f.logp) + f.entropy[:, None]), 0.0))
    return gz, gv, lt, ratio, ok, agz


def fp64(c, h=0, blob=None, theta=None, stats=None):
    """The float64 result of batch h of a form case: sums [P] (unscaled), loss4, grad [P] (scaled), td, the two losses,
    entropy, ratio [n] or None, passes [n], adv [n], stats, S_row [P + 4], S_grad [P]."""
    (s, a, r, s2), w, d = lg.batch_of(c, h)
    f = mirror.forward(c.blob if blob is None else blob, c.H, c.A, s, a, r, s2, d, c.theta if theta is None else theta)
    adv, st = advantage(c, f.delta, h, stats)
    gz, gv, lt, ratio, ok, agz = form_terms(c, f, w, adv, None if c.log_mu is None else c.log_mu[c.idx[h]])
    sums, loss4 = mirror.backward(f, gz, gv), lt.sum(axis=1)
    g, coef, _, _, al, cl = lg._scaled(c, sums, loss4, f.n)
    S_row, S_grad = lg.gradient_scales(c, f, gz, gv, lt, coef, agz=agz)
    return types.SimpleNamespace(sums=sums, loss4=loss4, grad=g, td=f.delta, actor_loss=al, critic_loss=cl, coef=coef,
                                 entropy=f.entropy, ratio=ratio, passes=ok, adv=adv, stats=st, S_row=S_row, S_grad=S_grad,
                                 f=f, gz=gz, gv=gv, lt=lt)


def cells(ratio, adv, eps=EPS):
    """Rows per gate cell at eps: (adv >= 0 passes, adv >= 0 clipped, adv < 0 passes, adv < 0 clipped)."""
    ok, pos = mirror.gate(ratio, adv, eps), adv >= 0
    return int((pos & ok).sum()), int((pos & ~ok).sum()), int((~pos & ok).sum()), int((~pos & ~ok).sum())


# ---- tolerances: per class and word, the larger of the two fp32 CPU references' worst error over the class's form cases
FORM_WORST_ROW = {
    "two": {
        "actor.fc1.weight": 5.19e-07,
        "actor.fc1.bias": 5.02e-07,
        "actor.fc2.weight": 1.94e-06,
        "actor.fc2.bias": 4.52e-07,
        "critic.fc1.weight": 1.95e-07,
        "critic.fc1.bias": 1.53e-07,
        "critic.fc2.weight": 1.72e-06,
        "critic.fc2.bias": 5.38e-08,
        "sum.nlp": 6.36e-08,
        "sum.delta": 5.38e-08,
        "sum.actor": 2.93e-07,
        "sum.critic": 7.43e-08,
    },
    "few": {
        "actor.fc1.weight": 4.76e-07,
        "actor.fc1.bias": 4.57e-07,
        "actor.fc2.weight": 2.48e-06,
        "actor.fc2.bias": 4.83e-07,
        "critic.fc1.weight": 3.49e-07,
        "critic.fc1.bias": 3.05e-07,
        "critic.fc2.weight": 1.42e-06,
        "critic.fc2.bias": 6.46e-08,
        "sum.nlp": 1.11e-07,
        "sum.delta": 6.46e-08,
        "sum.actor": 1.62e-07,
        "sum.critic": 1.29e-07,
    },
    "mid": {
        "actor.fc1.weight": 3.22e-07,
        "actor.fc1.bias": 2.77e-07,
        "actor.fc2.weight": 1.40e-06,
        "actor.fc2.bias": 4.24e-07,
        "critic.fc1.weight": 4.14e-07,
        "critic.fc1.bias": 3.46e-07,
        "critic.fc2.weight": 1.63e-06,
        "critic.fc2.bias": 2.55e-07,
        "sum.nlp": 4.91e-07,
        "sum.delta": 2.55e-07,
        "sum.actor": 1.04e-07,
        "sum.critic": 5.60e-07,
    },
    "large": {
        "actor.fc1.weight": 4.34e-07,
        "actor.fc1.bias": 3.59e-07,
        "actor.fc2.weight": 8.59e-06,
        "actor.fc2.bias": 3.55e-07,
        "critic.fc1.weight": 3.23e-06,
        "critic.fc1.bias": 1.51e-05,
        "critic.fc2.weight": 5.76e-06,
        "critic.fc2.bias": 3.89e-07,
        "sum.nlp": 1.35e-06,
        "sum.delta": 3.89e-07,
        "sum.actor": 1.23e-06,
        "sum.critic": 1.05e-05,
    },
    "peaked": {
        "actor.fc1.weight": 3.61e-06,
        "actor.fc1.bias": 3.56e-06,
        "actor.fc2.weight": 5.77e-06,
        "actor.fc2.bias": 2.32e-06,
        "sum.nlp": 4.31e-07,
        "sum.actor": 2.94e-07,
    },
}
FORM_WORST_GRAD = {
    "two": {
        "actor.fc1.weight": 5.19e-07,
        "actor.fc1.bias": 5.02e-07,
        "actor.fc2.weight": 1.94e-06,
        "actor.fc2.bias": 4.52e-07,
        "critic.fc1.weight": 1.95e-07,
        "critic.fc1.bias": 1.53e-07,
        "critic.fc2.weight": 1.72e-06,
        "critic.fc2.bias": 5.38e-08,
    },
    "few": {
        "actor.fc1.weight": 4.76e-07,
        "actor.fc1.bias": 4.57e-07,
        "actor.fc2.weight": 2.51e-06,
        "actor.fc2.bias": 4.94e-07,
        "critic.fc1.weight": 3.88e-07,
        "critic.fc1.bias": 3.48e-07,
        "critic.fc2.weight": 1.42e-06,
        "critic.fc2.bias": 7.13e-08,
    },
    "mid": {
        "actor.fc1.weight": 3.34e-07,
        "actor.fc1.bias": 2.63e-07,
        "actor.fc2.weight": 1.45e-06,
        "actor.fc2.bias": 4.02e-07,
        "critic.fc1.weight": 3.97e-07,
        "critic.fc1.bias": 3.42e-07,
        "critic.fc2.weight": 1.65e-06,
        "critic.fc2.bias": 2.90e-07,
    },
    "large": {
        "actor.fc1.weight": 4.49e-07,
        "actor.fc1.bias": 3.58e-07,
        "actor.fc2.weight": 8.59e-06,
        "actor.fc2.bias": 3.61e-07,
        "critic.fc1.weight": 3.19e-06,
        "critic.fc1.bias": 1.51e-05,
        "critic.fc2.weight": 5.78e-06,
        "critic.fc2.bias": 4.32e-07,
    },
    "peaked": {
        "actor.fc1.weight": 3.61e-06,
        "actor.fc1.bias": 3.54e-06,
        "actor.fc2.weight": 5.80e-06,
        "actor.fc2.bias": 2.29e-06,
    },
}


# the worst relative error of a reference's float32 ratio per class (measure's third result)
RATIO_WORST = {"two": 2.51e-07, "few": 4.48e-07, "mid": 5.58e-07, "large": 8.81e-07, "peaked": 9.9e-06}


def ratio_tolerance(fs, ratio):
    """The bound on |r - r_fp64| per row: the learner tests' 4e-6 r + 1e-7 (test_hip_learner_clipped.py), which the
    references meet five times over outside the peaked class.  Under the peaked parameters a logit of size 32 to 40 has
    a float32 ulp of 3.8e-6, log p inherits a few of those as an absolute error and the ratio as a relative one: the
    references themselves are 9.9e-6 off, so that class takes TOL_FACTOR times its own entry like every other word."""
    rel = lg.TOL_FACTOR * RATIO_WORST["peaked"] if form_class(fs) == "peaked" else 4e-6
    return rel * np.asarray(ratio, np.float64) + 1e-7


def tolerances(fs):
    """({row word: tolerance}, {tensor: tolerance}) of a form case: TOL_FACTOR times the references' worst in the class
    the word is judged in (word_class)."""
    return ({w: lg.TOL_FACTOR * FORM_WORST_ROW[word_class(fs, w)][w] for w in lg.ROW_WORDS},
            {w: lg.TOL_FACTOR * FORM_WORST_GRAD[word_class(fs, w)][w] for w in lg.TENSORS})


def cpu_stats(c, ref):
    """The statistics the CPU side passes to the fp32 references of a batch form: the float64 result's."""
    return ref.stats if c.form.adv == "batch" else None


def measure():
    """Both references over FORM_GRID: (worst row errors, worst gradient errors, worst relative error of a float32
    ratio) per class, and who set each entry.  The peaked class holds the words it judges (word_class)."""
    mine = lambda k, words: [w for w in words if k != "peaked" or w not in CRITIC_WORDS]    # noqa: E731
    row = {k: {w: (0.0, "") for w in mine(k, lg.ROW_WORDS)} for k in CLASSES}
    grad = {k: {w: (0.0, "") for w in mine(k, lg.TENSORS)} for k in CLASSES}
    ratio = {k: 0.0 for k in CLASSES}
    for fs in FORM_GRID:
        c = build_case(fs)
        ref = fp64(c)
        for name, fn in (("torch", lg.torch_fp32), ("sequential", lg.sequential_fp32)):
            seen = {}
            r, g = fn(c, cpu_stats(c, ref), seen)
            if fs.clip is not None:
                k = form_class(fs)
                ratio[k] = max(ratio[k], float((np.abs(seen["ratio"] - ref.ratio) / ref.ratio).max()))
            for table, e in ((row, lg.errors(r, np.concatenate([ref.sums, ref.loss4]), ref.S_row, c.H, c.A)),
                             (grad, lg.errors(g, ref.grad, ref.S_grad, c.H, c.A))):
                for w, x in e.items():
                    t = table[word_class(fs, w)]
                    if x > t[w][0]:
                        t[w] = (x, name, form_id(fs))
    return row, grad, ratio
