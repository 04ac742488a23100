"""The Adam step's cases and references without a GPU (tests/adam_cases.py): restate32 against the fp64 reference over
the grid, the fp64 reference against torch.optim.Adam in float64, the conditions the cases promise, the gradient-row
helper, and mutants of restate32 that the tolerances must tell from it."""
import contextlib

import numpy as np
import pytest
import torch

import adam_cases as ac

F32 = np.float32


def test_restate32_stays_within_half_a_tolerance_and_the_table_is_current():
    worst = ac.measure()
    for family in worst:
        tol = ac.tolerance(family)
        for k in ac.CLASSES:
            for w in ac.WORDS:
                assert worst[family][k][w] <= 0.5 * tol[k][w], (family, k, w, worst[family][k][w])
                # the committed table, to 1 % (another libm or numpy may move a last printed digit)
                assert abs(worst[family][k][w] - ac.WORST[family][k][w]) <= 0.01 * ac.WORST[family][k][w], (family, k, w)


# ---- fp64 against torch.optim.Adam in float64 ------------------------------------------------------------------------

@contextlib.contextmanager
def _float64_default():
    """torch.tensor(float(step)) of adam.to_state_dict is then a float64 scalar: steps past 2^24 stay exact."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


class _count_adam_paths:
    """Counts the calls of torch's single-tensor and multi-tensor (foreach) Adam while it is entered."""

    def __enter__(self):
        import torch.optim.adam as ta
        self.single = self.multi = 0
        self._ta, self._saved = ta, (ta._single_tensor_adam, ta._multi_tensor_adam)

        def single(*a, **k):
            self.single += 1
            return self._saved[0](*a, **k)

        def multi(*a, **k):
            self.multi += 1
            return self._saved[1](*a, **k)

        ta._single_tensor_adam, ta._multi_tensor_adam = single, multi
        return self

    def __exit__(self, *exc):
        self._ta._single_tensor_adam, self._ta._multi_tensor_adam = self._saved


def _torch_adam64(sizes, w, m, v, g, s0, lr, foreach):
    """One torch.optim.Adam step in float64 over tensors of `sizes` from the loaded state, through the library's own
    adam.to_state_dict: (w', m', v') flat."""
    from uavtrack import adam
    offs = np.concatenate([[0], np.cumsum(sizes)])
    with _float64_default():
        params = [torch.nn.Parameter(torch.from_numpy(w[a:b].copy())) for a, b in zip(offs[:-1], offs[1:])]
        sd = adam.to_state_dict(params, lr, m, v, s0)
        for group in sd["param_groups"]:                  # load_state_dict takes the saved groups' settings, foreach too
            group["foreach"] = foreach
        opt = torch.optim.Adam(params, lr=lr, foreach=foreach)
        opt.load_state_dict(sd)
        assert all(group["foreach"] is foreach for group in opt.param_groups)
        taken = _count_adam_paths()
        for p, (a, b) in zip(params, zip(offs[:-1], offs[1:])):
            p.grad = torch.from_numpy(g[a:b].copy())
        with taken:
            opt.step()
        assert (taken.multi > 0, taken.single > 0) == (foreach, not foreach), (taken.single, taken.multi)
        st = [opt.state[p] for p in params]
        assert [int(s["step"]) for s in st] == [int(x) + 1 for x in s0]
        assert all(s["exp_avg"].dtype == torch.float64 for s in st)
        cat = lambda xs: np.concatenate([x.detach().numpy().ravel() for x in xs])
        return cat(params), cat([s["exp_avg"] for s in st]), cat([s["exp_avg_sq"] for s in st])


def _loadable(c):
    """The case's state in float64 with zero moments on the tensors at step 0, which torch writes as 'no state'."""
    w, m, v, g = (np.asarray(x, np.float64) for x in (c.w, c.m, c.v, c.g))
    fresh = np.concatenate([np.full(n, s == 0) for n, s in zip(c.sizes, c.s0)])
    return w, np.where(fresh, 0.0, m), np.where(fresh, 0.0, v), g


def _assert_close(got, ref, c, m, v, g, what):
    S = ac.scales(m, v, g, ref[2], c.step, c.lr)
    for name, i, scale in (("w", 0, np.abs(ref[0]) + S["w"]), ("m", 1, S["m"]), ("v", 2, S["v"])):
        d = np.abs(got[i] - ref[i])
        assert (d <= 1e-14 * scale).all(), (what, name, float(np.max(d / np.maximum(scale, 1e-300))))


@pytest.mark.parametrize("foreach", [False, True])
def test_fp64_is_torch_adam_in_float64(foreach):
    for H, A in ac.SHAPES:
        c = ac.learner_case(H, A, rot=H % 7)
        w, m, v, g = _loadable(c)
        ref = ac.fp64_learner(c, w, m, v, g)
        got = [[], [], []]
        for lr, ts in ((c.lrs[0], slice(0, 4)), (c.lrs[1], slice(4, 8))):      # the actor's optimizer, then the critic's
            fl = slice(c.offs[ts.start], c.offs[ts.stop])
            out = _torch_adam64(c.sizes[ts], w[fl], m[fl], v[fl], g[fl], c.s0[ts], ac.lr32(lr), foreach)
            for acc, x in zip(got, out):
                acc.append(x)
        _assert_close([np.concatenate(x) for x in got], ref, c, m, v, g, (H, A))
    for H, B in ac.PMI_CASES:
        c = ac.pmi_case(H, B, rot=3)
        w, m, v, g = _loadable(c)
        got = _torch_adam64(c.sizes, w, m, v, g, c.s0, ac.lr32(c.lrs[0]), foreach)
        _assert_close(got, ac.fp64_pmi(c, w, m, v, g), c, m, v, g, (H, B))


# ---- what the cases promise ------------------------------------------------------------------------------------------

def test_input_conditions():
    zero_actor = 0
    by_tensor = [set() for _ in range(8)]
    for family, c, _ in ac.grid():
        assert len(set(c.s0.tolist())) == len(c.s0)
        # both fp64 scalars of every tensor clear of a float32 rounding boundary
        for t, s in enumerate(c.s0):
            lr = c.lr[c.offs[t]]
            for x in ac.scalars64(int(s) + 1, lr):
                assert np.isfinite(x) and float(ac.boundary_distance(x)) >= ac.BOUNDARY_MARGIN, (family, t, int(s), lr)
        # every class in every tensor long enough, another class on either side of every boundary
        for t in range(len(c.sizes)):
            if c.sizes[t] >= len(ac.CLASSES):
                assert set(c.cls[c.offs[t]:c.offs[t + 1]]) == set(range(len(ac.CLASSES)))
            if c.sizes[t] > 1:
                assert c.cls[c.offs[t]] != c.cls[c.offs[t + 1] - 1]
            if t:
                assert c.cls[c.offs[t]] != c.cls[c.offs[t] - 1]
        # every intermediate zero or normal, nothing NaN or infinite
        for name, x in ac.trace32(c.w, c.m, c.v, c.g, c.step, c.lr).items():
            assert np.isfinite(x).all(), (family, name)
            assert ((x == 0) | (np.abs(x.astype(np.float64)) >= ac.MIN_NORMAL)).all(), (family, name)
        assert (np.abs(c.g[c.g != 0]) >= 1e-17).all()
        assert {0.0, 1.0, 1e6} <= {10.0 ** np.round(np.log10(abs(x))) if x else 0.0 for x in c.w[:10].tolist()}
        if len(c.s0) == 8:
            zero_actor += int((c.s0[:4] == 0).any())
            for t, s in enumerate(c.s0.tolist()):
                by_tensor[t].add("small" if s in ac.SMALL else "middle" if s in ac.MIDDLE else "saturated")
    assert zero_actor and all(x == {"small", "middle", "saturated"} for x in by_tensor), by_tensor
    for name in ("momentum", "still", "cold"):
        c = ac.learner_case(33, 9)
        assert (c.g[c.cls == ac.CLASSES.index(name)] == 0).all()
    # saturated means what the docstring says: sqrt(bc2) is 1.0f
    for s in ac.STEPS:
        if s not in ac.SMALL + ac.MIDDLE:
            assert ac.trace32(0, 0, 0, 0, s + 1, 1e-3)["bc2_sqrt"] == F32(1.0)


def test_chain_conditions():
    """The three steps of the chain: every executed step clear of a rounding boundary, every intermediate normal."""
    q = ac.CHAIN
    c = ac.learner_case(q["H"], q["A"], q["rot"])
    w, m, v = c.w, c.m, c.v
    for k in range(q["count"]):
        for t, s in enumerate(c.s0):
            assert ac.step_is_safe(int(s) + 1 + k, (c.lr[c.offs[t]],)), (t, int(s), k)
        tr = ac.trace32(w, m, v, c.g, c.step + k, c.lr)
        for name, x in tr.items():
            assert (np.isfinite(x) & ((x == 0) | (np.abs(x.astype(np.float64)) >= ac.MIN_NORMAL))).all(), (k, name)
        w, m, v = tr["w"], tr["m"], tr["v"]
    assert all(np.array_equal(a, b) for a, b in zip(ac.chain32(c, c.g, q["count"])[-1], (w, m, v)))


def test_rows_round_trip_and_exact_scales():
    c = ac.learner_case(33, 9, rot=2)
    for form in ac.FORMS:
        rows = ac.learner_rows(c, form)
        assert rows.dtype == F32 and rows.shape == (len(ac._N[form]), c.P + 8)
        for r, n in zip(rows, ac._N[form]):
            assert ac.read_tail(r) == (n, 0, c.P)
        al, cl, g = ac.finalize32(rows, c.P, c.na, ac.form_loss(form) == "per_sample")
        assert np.array_equal(g, c.g)                                       # the value; a zero's sign is the kernel's
        zero = c.g == 0
        assert set(np.signbit(rows[:, :c.P][:, zero]).ravel().tolist()) == {True, False}
        ls = np.asarray(ac._LOSS[form], np.float64).sum(0)
        N = sum(ac._N[form])
        want = (ls[0] / N * ls[1] / N if form == "reference" else ls[2] / N, ls[3] / N)
        assert (float(al), float(cl)) == want                               # exact: the sums are dyadic
    big = ac.make_rows(np.zeros((2, 3)), np.zeros((2, 4)), [2 ** 40 + 5, 2 ** 31], [64, 0], [3, -7])
    assert ac.read_tail(big[0]) == (2 ** 40 + 5, 64, 3) and ac.read_tail(big[1]) == (2 ** 31, 0, -7)
    assert ac.learner_rows(c, "one_row", status=2, tag=c.P + 1, n=[0])[0, c.P:].view(np.int32)[4:].tolist() == \
        [0, 0, 2, c.P + 1]


# ---- mutants ---------------------------------------------------------------------------------------------------------

def _mutant32(kind, c):
    """restate32 with one thing changed: (w', m', v') in float32."""
    w, m, v, g = (np.asarray(x, F32) for x in (c.w, c.m, c.v, c.g))
    step, lr = c.step.copy(), c.lr.copy()
    if kind == "step_not_advanced":
        step = step - 1
    if kind == "previous_tensor_step":
        for t in range(1, len(c.sizes)):
            step[c.offs[t]] = c.s0[t - 1] + 1
    if kind == "lr_swapped":
        lr = np.where(lr == c.lrs[0], c.lrs[1], c.lrs[0])
    a64, b64 = ac.scalars64(step, lr)
    if kind == "no_bc1":
        a64 = np.asarray(lr, F32).astype(np.float64)
    if kind == "no_bc2":
        b64 = np.ones_like(b64)
    step_size, bc2_sqrt = np.asarray(a64).astype(F32), np.asarray(b64).astype(F32)
    c1 = F32(0.9) if kind == "lerp_0.9" else F32(0.1)
    d2 = F32(0.99) if kind == "decay_0.99" else F32(0.999)
    eps = F32(1e-6) if kind == "eps_1e-6" else F32(1e-8)
    with np.errstate(all="ignore"):
        mi = m + c1 * (g - m)
        if kind == "decay_after_add":
            vi = (v + F32(0.001) * g * g) * d2
        else:
            vi = v * d2 + F32(0.001) * g * g
        if kind == "eps_inside":
            denom = (np.sqrt(vi) + eps) / bc2_sqrt
        else:
            denom = np.sqrt(vi) / bc2_sqrt + eps
        return w - step_size * (mi / denom), mi, vi


# mutant -> the (class, word) at which it must leave the tolerance by MUTANT_ROOM
MUTANTS = {
    "decay_0.99": ("momentum", "v"),
    "eps_inside": ("tiny", "w"),
    "eps_1e-6": ("tiny", "w"),
    "no_bc2": ("typical", "w"),
    "no_bc1": ("typical", "w"),
    "step_not_advanced": ("typical", "w"),
    "previous_tensor_step": ("typical", "w"),
    "lr_swapped": ("typical", "w"),
    "lerp_0.9": ("typical", "m"),
    "decay_after_add": ("typical", "v"),
}


def _given_grid():
    return [(c, fp64(c)) for family, c, fp64 in ac.grid() if family == "given"]


def _worst_of(kind, grid):
    worst = {k: {w: 0.0 for w in ac.WORDS} for k in ac.CLASSES}
    with np.errstate(all="ignore"):
        for c, ref in grid:
            ac.merge_worst(worst, ac.case_errors(c, _mutant32(kind, c), ref))
    return worst


def test_the_unchanged_copy_is_restate32():
    for c, _ in _given_grid()[:4]:
        for a, b in zip(_mutant32("none", c), ac.restate32(c.w, c.m, c.v, c.g, c.step, c.lr)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", list(MUTANTS))
def test_mutant_leaves_the_tolerance(kind):
    tol = ac.tolerance("given")
    worst = _worst_of(kind, _given_grid())
    k, w = MUTANTS[kind]
    ac.report(kind, worst, tol)
    assert worst[k][w] > ac.MUTANT_ROOM * tol[k][w], (kind, k, w, worst[k][w], tol[k][w])


@pytest.mark.parametrize("kind", ["previous_tensor_step", "step_not_advanced", "state_shifted"])
def test_indexing_mutant_leaves_the_pmi_tolerance(kind):
    """What test_hip_adam.py's PMI test is there for: a step taken from the neighbouring tensor, a step not advanced, or
    moments read one element off leave the "net" tolerance by MUTANT_ROOM although the recovery's slack is granted."""
    tol = ac.tolerance("net")
    for H, B in ac.PMI_CASES:
        c = ac.pmi_case(H, B, rot=2)
        ref = ac.fp64_pmi(c)
        if kind == "state_shifted":
            got = ac.restate32(c.w, np.roll(c.m, 1), np.roll(c.v, 1), c.g, c.step, c.lr)
        else:
            with np.errstate(all="ignore"):
                got = _mutant32(kind, c)
        e = ac.case_errors(c, got, ref, ac.recovery_slack(c, c.g, ref))
        ac.report(f"{kind} ({H}, {B}):", e, tol)
        assert max(e[k][w] / tol[k][w] for k in e for w in e[k] if tol[k][w] > 0) > ac.MUTANT_ROOM, (kind, H, B)
        exact = ac.case_errors(c, ac.restate32(c.w, c.m, c.v, c.g, c.step, c.lr), ref, ac.recovery_slack(c, c.g, ref))
        assert not ac.over(exact, tol)


def test_eps_inside_shows_on_tiny_at_small_steps_only():
    """(sqrt(v) + eps) / sqrt(bc2) against sqrt(v) / sqrt(bc2) + eps: the same bits once sqrt(bc2) is 1.0f, far apart
    where sqrt(v) is near eps and the step is small -- the reason the class `tiny` exists."""
    tol = ac.tolerance("given")
    tiny = ac.CLASSES.index("tiny")
    seen_small = seen_saturated = 0
    for c, ref in _given_grid():
        got, exact = _mutant32("eps_inside", c), ac.restate32(c.w, c.m, c.v, c.g, c.step, c.lr)
        saturated = ac.trace32(c.w, c.m, c.v, c.g, c.step, c.lr)["bc2_sqrt"] == F32(1.0)
        for a, b in zip(got, exact):
            assert np.array_equal(a[saturated], b[saturated])
        e = ac.element_errors(got, ref, ac.scales(c.m, c.v, c.g, ref[2], c.step, c.lr))["w"]
        # (a parameter of order 1e6 absorbs the whole move into its own last place)
        small = (c.cls == tiny) & np.isin(c.step - 1, ac.SMALL) & (np.abs(c.w) < 10)
        if small.any():
            assert (e[small] > ac.MUTANT_ROOM * tol["tiny"]["w"]).all(), float(e[small].min())
        seen_small += int(small.sum())
        seen_saturated += int((saturated & (c.cls == tiny)).sum())
    assert seen_small and seen_saturated
