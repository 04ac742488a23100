"""The device trainers' Adam step (adam_element, csrc/adam.h) from a LOADED state on the MI355X: non-zero moments, one
step count per tensor, past 2^31 included.  The learner's gradient is given exactly through apply (hand-made gradient
rows, tests/adam_cases.py), so its step is compared bit for bit with restate32, the float32 reading of adam_element, and
within the CPU-measured tolerances with torch's formula in float64.  The PMI trainer's gradient cannot be injected; there
a trainer that starts from zero yields it, and a second one that starts from a loaded state is compared with the float64
reference: that pins the indexing (tensor -> step, parameter offset -> state offset), the learner pins the arithmetic."""
import numpy as np
import pytest
import torch

import adam_cases as ac
import learner_harness as lh
import pmi_gradient_cases as pc
import pmi_trainer_mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV
F32 = np.float32


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ulps(a, b):
    """The distance of two float32 arrays in units in the last place (of the ordered integer line)."""
    key = lambda x: np.where(_bits(x) >> 31, -(_bits(x) & 0x7FFFFFFF).astype(np.int64), (_bits(x) & 0x7FFFFFFF).astype(np.int64))
    return np.abs(key(a) - key(b))


def _loaded(c, loss, w=None, m=None, v=None, s0=None):
    """A learner holding the case's parameters, moments and step counts (or the given ones)."""
    pick = lambda x, d: d if x is None else x
    L = lh.learner(c.H, c.A, loss=loss, blob=pick(w, c.w), lr=c.lrs)
    L._set_optim_state(pick(m, c.m), pick(v, c.v), pick(s0, c.s0))
    return L


def _triple(st):
    return st["params"], st["exp_avg"], st["exp_avg_sq"]


def _assert_landed(tag, c, st, losses, rows, form):
    """One apply of `rows` from the case's loaded state landed: moments, steps, losses and parameters bit for bit
    restate32 / finalize32, all three words within the fp64 tolerance.  Every figure is printed first."""
    al32, cl32, g = ac.finalize32(rows, c.P, c.na, ac.form_loss(form) == "per_sample")
    assert np.array_equal(g, c.g)
    want = ac.restate32(c.w, c.m, c.v, g, c.step, c.lr)
    got = _triple(st)
    tol = ac.tolerance("given")
    e = ac.case_errors(c, got, ac.fp64_learner(c))
    ac.report(tag, e, tol)
    off = {name: int((_bits(a) != _bits(b)).sum()) for name, a, b in zip(("w", "m", "v"), got, want)}
    print(tag, "elements off restate32's bits:", off, "worst distance of a parameter:", int(_ulps(got[0], want[0]).max()),
          "ulp; losses", [float(x) for x in losses], "against", [float(al32), float(cl32)])
    assert _same_bits(got[1], want[1]) and _same_bits(got[2], want[2]), off
    assert st["step"].dtype == np.int64 and np.array_equal(st["step"], c.s0 + 1)
    assert _same_bits(losses[0], al32) and _same_bits(losses[1], cl32)
    assert not ac.over(e, tol), ac.over(e, tol)
    still = c.cls == ac.CLASSES.index("still")
    assert _same_bits(got[0][still], c.w[still])
    assert _same_bits(got[0], want[0]), off


def _apply(L, rows):
    al, cl = L.apply(lh.dev(rows))
    return al.cpu().numpy(), cl.cpu().numpy()


# ---- 1: one apply, bitwise and against fp64 --------------------------------------------------------------------------

@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("H,A", ac.SHAPES)
def test_apply_from_loaded_state_is_restate32_to_the_bit(H, A, form):
    c = ac.learner_case(H, A, rot=(2 * ac.FORMS.index(form) + ac.SHAPES.index((H, A))) % len(ac.CLASSES))
    rows = ac.learner_rows(c, form)
    L = _loaded(c, ac.form_loss(form))
    losses = _apply(L, rows)
    L.check()
    _assert_landed(f"({H}, {A}) {form}:", c, lh.state(L), losses, rows, form)


# ---- 2: a chain of applies, eager and as one captured apply replayed -------------------------------------------------

def test_chain_of_applies_eager_and_replayed():
    q = ac.CHAIN
    c = ac.learner_case(q["H"], q["A"], q["rot"])
    rows = ac.learner_rows(c, q["form"])
    g = ac.finalize32(rows, c.P, c.na, True)[2]
    want = ac.chain32(c, g, q["count"])
    drows = lh.dev(rows)
    eager = _loaded(c, "per_sample")
    for k in range(q["count"]):
        eager.apply(drows)
        st = lh.state(eager)
        off = [int((_bits(a) != _bits(b)).sum()) for a, b in zip(_triple(st), want[k])]
        print(f"step {k + 1}: elements off restate32's bits (w, m, v): {off}")
        assert off == [0, 0, 0] and np.array_equal(st["step"], c.s0 + 1 + k)
    eager.check()
    graphed = _loaded(c, "per_sample")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            graphed.apply(drows)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(graphed._optim_state()[2], c.s0)                  # the capture ran nothing
    for k in range(q["count"]):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(graphed._optim_state()[2], c.s0 + 1 + k)      # each replay takes the next step
    lh.same(lh.state(graphed), lh.state(eager), "replayed against eager")
    graphed.check()


# ---- 3: the closed update and grad -> apply from one loaded state ----------------------------------------------------

@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_closed_and_split_update_from_loaded_state(loss):
    H, A, n = 33, 12, 65
    blob, b, store, cap, idx, it = lh.case(H, A, n, True)
    c = ac.learner_case(H, A, rot=4)
    a, bb = _loaded(c, loss, w=blob), _loaded(c, loss, w=blob)
    before = lh.state(a)
    lh.same(before, lh.state(bb), "loaded")
    assert _same_bits(before["exp_avg"], c.m) and _same_bits(before["exp_avg_sq"], c.v) and np.array_equal(before["step"], c.s0)
    al_a, cl_a, _ = a._run(n, store, cap, it, None)
    row, _ = bb._grad(n, store, cap, it)
    assert ac.read_tail(row.cpu().numpy()) == (n, 0, c.P)                  # a real row's tail, by make_rows' reader
    al_b, cl_b = bb.apply(row)
    a.check(); bb.check()
    sa, sb = lh.state(a), lh.state(bb)
    lh.same(sa, sb, "closed against split")
    assert _same_bits(al_a.cpu().numpy(), al_b.cpu().numpy()) and _same_bits(cl_a.cpu().numpy(), cl_b.cpu().numpy())
    assert np.array_equal(sa["step"], c.s0 + 1)
    moved = ~((c.m == 0) & (c.v == 0))
    assert (_bits(sa["exp_avg"]) != _bits(c.m))[moved].mean() > 0.9         # the step did run on the loaded moments


# ---- 4: a refused apply leaves a loaded state alone ------------------------------------------------------------------

def test_refused_apply_from_loaded_state_changes_nothing():
    H, A, form = 33, 9, "three_rows"
    c = ac.learner_case(H, A, rot=6)
    L = _loaded(c, "per_sample")
    loaded = lh.state(L)
    for what, kw in (("a status bit", dict(status=2)), ("a foreign P", dict(tag=c.P + 1)), ("n = 0", dict(n=[1, 0, 2]))):
        losses = _apply(L, ac.learner_rows(c, form, **kw))
        assert np.isnan(losses[0]) and np.isnan(losses[1]), what
        st = lh.state(L)
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert _same_bits(st[k], loaded[k]), (what, k)
        assert _same_bits(st["params"], c.w) and _same_bits(st["exp_avg"], c.m) and _same_bits(st["exp_avg_sq"], c.v)
        assert np.array_equal(st["step"], c.s0), what
        with pytest.raises(RuntimeError, match="refused"):
            L.check()
        L.check()                                                            # once
    rows = ac.learner_rows(c, form)
    losses = _apply(L, rows)
    L.check()
    _assert_landed("behind three refusals:", c, lh.state(L), losses, rows, form)


# ---- 5: a checkpoint carries the state the next step starts from -----------------------------------------------------

def test_checkpoint_continuation():
    H, A, form = 33, 9, "one_row"
    c = ac.learner_case(H, A, rot=1)
    s0 = np.array([0, 3, 99, 2 ** 24, 0, 999, 6930, 65536], np.int64)      # a float32 step tensor holds these exactly
    fresh = np.concatenate([np.full(n, s == 0) for n, s in zip(c.sizes, s0)])
    m, v = np.where(fresh, F32(0), c.m), np.where(fresh, F32(0), c.v)      # torch writes step 0 as "no state"
    a = _loaded(c, "per_sample", m=m, v=v, s0=s0)
    sd = a.state_dict()
    assert [len(sd[k]["state"]) for k in ("actor_optimizer", "critic_optimizer")] == [3, 3]
    b = lh.learner(H, A, loss="per_sample")
    b.load_state_dict(sd)
    sb = lh.state(b)
    lh.same(lh.state(a), sb, "loaded from the checkpoint")
    assert _same_bits(sb["params"], c.w) and _same_bits(sb["exp_avg"], m) and _same_bits(sb["exp_avg_sq"], v)
    assert np.array_equal(sb["step"], s0)
    rows = lh.dev(ac.learner_rows(c, form))
    la, lb = a.apply(rows), b.apply(rows)
    a.check(); b.check()
    lh.same(lh.state(a), lh.state(b), "one apply on each")
    assert np.array_equal(lh.state(b)["step"], s0 + 1)
    assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(la, lb))


# ---- 6: the PMI trainer: tensor -> step, parameter offset -> state offset --------------------------------------------

def _pmi_flat(sd):
    return np.concatenate([np.asarray(sd[k], F32).ravel() for k in pmi_trainer_mirror.param_names()])


@pytest.mark.parametrize("H,B", ac.PMI_CASES)
def test_pmi_trainer_step_from_loaded_state(H, B):
    """Z starts from zero moments and yields the gradient (pc.recovered_gradient: it does not depend on the Adam state);
    R starts from class-dealt moments and 18 distinct step counts and is compared with the fp64 reference on that
    gradient, in the metric of adam_cases with the recovery's slack (ac.recovery_slack)."""
    from test_hip_pmi_trainer import _call, _trainer
    from uavtrack import adam
    case = pc.build_case(H, B)
    c = ac.pmi_case(H, B, rot=2)
    z, r = _trainer(H, B, case.sd), _trainer(H, B, case.sd)
    adam.write(r._lib.uavtrack_pmi_trainer_set_optimizer_state, r._h, c.m, c.v, c.s0, r._stream())
    m0, v0, st0 = r.optimizer_state()
    assert _same_bits(m0, c.m) and _same_bits(v0, c.v) and np.array_equal(st0, c.s0)
    out_z, out_r = _call(z, case.rows, pc.N_UAV, case.t, case.u, B), _call(r, case.rows, pc.N_UAV, case.t, case.u, B)
    z.check(); r.check()
    assert out_z[0] == out_r[0] and _same_bits(out_z[1], out_r[1]) and _same_bits(out_z[2], out_r[2])
    mz, vz, sz = z.optimizer_state()
    assert np.array_equal(sz, np.ones(18, np.int64))
    g = pc.recovered_gradient(mz, vz)
    c.w, c.g = _pmi_flat(case.sd), g
    mr, vr, sr = r.optimizer_state()
    assert sr.dtype == np.int64 and np.array_equal(sr, c.s0 + 1)
    sd_z, sd_r = z.state_dict(), r.state_dict()
    ref = ac.fp64_pmi(c)
    e = ac.case_errors(c, (_pmi_flat({k: v.numpy() for k, v in sd_r.items()}), mr, vr), ref, ac.recovery_slack(c, g, ref))
    tol = ac.tolerance("net")
    ac.report(f"PMI ({H}, {B}):", e, tol)
    print("gradient magnitudes:", float(np.abs(g).min()), float(np.median(np.abs(g))), float(np.abs(g).max()))
    assert not ac.over(e, tol), ac.over(e, tol)
    for k in sd_z:                                                          # BatchNorm's statistics: not the optimizer's
        if "running" in k or "num_batches" in k:
            assert torch.equal(sd_z[k], sd_r[k]), k
    assert int(sd_r["bn1.num_batches_tracked"]) == int(case.sd["bn1.num_batches_tracked"]) + 2
