"""The regularised device learner (uavtrack_learner_set_regularisation / _set_diagnostics, DeviceActorCritic's
entropy_coef / max_grad_norm / enable_diagnostics) on the MI355X: with the settings off every call keeps its bits; the
entropy bonus and the gradient-norm clip against the float64 mirror (tests/learner_mirror.py) at
test_sweep_against_fp64_mirror's bounds; the edges of the softmax; weights; the split form and the shared tail;
determinism and graph capture; refusals.

Shapes are corners of learner_harness.SWEEP: H in {1, 33, 128, 256}, A in {2, 12, 48}, n in {1, 63, 65, 4096}, and
n = 4113 at H = 256 (16 rows per tile: 258 tiles for 256 workgroups, so workgroups loop)."""
import os
import sys

import numpy as np
import pytest
import torch

import learner_harness as lh
import learner_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA
INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, A, n, gathered)
SHAPES = [(1, 2, 1, False), (33, 12, 63, True), (128, 48, 65, False), (128, 12, 4096, True), (256, 48, 4113, True),
          (256, 2, 63, False)]
SMALL = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[4]]


def _uav():
    import uavtrack
    return uavtrack


def _weights(n, seed=0):
    return lh.make_weights(np.random.RandomState(n + 11 + seed), n)


_mirror_cache = {}


def _mirror(H, A, n, gather, loss, c, weighted, blob=None):
    """The fp64 update of a case, computed once: (actor_loss, critic_loss, td, gradient, entropy, None)."""
    key = (H, A, n, gather, loss, c, weighted, None if blob is None else blob.tobytes())
    if key not in _mirror_cache:
        blob0, b, _, _, idx, _ = lh.case(H, A, n, gather)
        w = _weights(n) if weighted else None
        _mirror_cache[key] = mirror.losses_and_grads(blob0 if blob is None else blob, H, A, *lh.gathered(b, idx), GAMMA, loss,
                                                     weights=w, entropy_coef=np.float32(c))
    return _mirror_cache[key]


def _entropy_tol(A):
    return 1e-5 * max(1.0, np.log(A))


def _bits(out):
    """An update's result without the diagnostics: what a learner that has them installed shares with one that has not."""
    return {k: v for k, v in out.items() if k not in ("entropy", "grad_norm")}


# ---- 1. off is off -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("diag", [False, True], ids=["bare", "diag"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n,gather", SMALL)
def test_off_is_off(H, A, n, gather, loss, weighted, diag):
    """set_regularisation(0, inf, inf), diagnostics installed or not: three consecutive updates, closed and as
    grad -> apply -> write_priorities, are an untouched learner's bit for bit (parameters, both moments, steps, losses,
    td_delta, priorities)."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    w = lh.dev(_weights(n)) if weighted else None
    prio0 = torch.rand(cap, device=DEV) + 0.1
    for run in (lh.update, lh.split_update):
        outs = []
        for touched in (False, True):
            L = lh.learner(H, A, loss, blob, n, diag=diag and touched)
            if touched:
                L.set_regularisation(0.0, (INF, INF))
                assert L.get_regularisation() == (0.0, INF, INF)
            prio = prio0.clone()
            outs.append([run(L, n, store, cap, it, prio, w) for _ in range(3)])
            L.check()
            if diag and touched:
                ent = mirror.policy(outs[-1][1]["params"], H, A, lh.gathered(b, idx)[0])[2]     # the policy of the third update
                assert np.abs(L.entropy(n).cpu().numpy() - ent).max() <= _entropy_tol(A)
                assert torch.isnan(L.grad_norm).all()                                      # no clip, no norm
        assert np.isfinite(outs[0][2]["actor_loss"]) and np.array_equal(outs[0][2]["step"], np.full(8, 3))
        assert not np.array_equal(outs[0][2]["prio"], prio0.cpu().numpy())
        for x, y in zip(*outs):
            lh.same(_bits(x), _bits(y))


# ---- 2. the entropy gradient ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [0.01, 1.0])
@pytest.mark.parametrize("H,A,n,gather", SHAPES)
def test_entropy_update_against_fp64_mirror(H, A, n, gather, c):
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    weighted = (H + n) % 2 == 0
    w = lh.dev(_weights(n)) if weighted else None
    L = lh.learner(H, A, "per_sample", blob, n, c=c, diag=True)
    out = lh.update(L, n, store, cap, it, None, w)
    L.check()
    ral, rcl, rtd, g, ent, _ = _mirror(H, A, n, gather, "per_sample", c, weighted)
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ral, rcl, rtd, c, A)
    lh.assert_step_from_zero(out, blob, g, n, H, A)
    assert np.abs(L.entropy(n).cpu().numpy() - ent).max() <= _entropy_tol(A)
    if c == 1.0 and A > 2 and n >= 63:       # the term is in the result: the plain gradient is far outside the bound
        g0 = _mirror(H, A, n, gather, "per_sample", 0.0, weighted)[3]
        assert np.abs(out["exp_avg"] / 0.1 - g0).max() > 100 * lh.tol_g(n, g)


# ---- 3. the edges of the softmax -----------------------------------------------------------------------------------------

def _with_fc2(blob, H, A, scale, ramp):
    """The blob with the actor's fc2 scaled and a ramp of `ramp` over its bias."""
    o = mirror.layout(H, A)[1]
    out = blob.copy()
    out[o[2]:o[3]] *= np.float32(scale)
    out[o[3]:o[4]] = np.float32(scale) * out[o[3]:o[4]] + np.linspace(0.0, ramp, A).astype(np.float32)
    return out


@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[2]])
def test_logits_spanning_more_than_250_stay_finite(H, A, n, gather):
    """fc2 with a ramp of 300 over its bias: every row's fp32 probabilities underflow to 0 somewhere, also at some rows'
    own action.  The row is finite and is the mirror's.  (The ramp sits in the bias, not in a scale on fc2.weight: a
    scale would also multiply the fp32 forward's rounding of the logits, which is not the softmax's doing.)"""
    blob0, b, store, cap, idx, it = lh.case(H, A, n, gather)
    blob = _with_fc2(blob0, H, A, 1.0, 300.0)
    logp = mirror.policy(blob, H, A, lh.gathered(b, idx)[0])[0]
    assert (logp.max(axis=1) - logp.min(axis=1) > 250).all()
    assert (np.exp(logp.astype(np.float32)).min(axis=1) == 0).all()
    assert (np.exp(logp[np.arange(n), lh.gathered(b, idx)[1]].astype(np.float32)) == 0).any()
    c = 1.0
    L = lh.learner(H, A, "per_sample", blob, n, c=c, diag=True)
    row, td = L._grad(n, store, cap, it)
    L.check()
    row = row.cpu().numpy()
    P = L.num_params
    want = mirror.shard_sums(blob, H, A, *lh.gathered(b, idx), GAMMA, "per_sample", None, np.float32(c))
    assert np.isfinite(row[:P + 4]).all() and np.isfinite(want["g"]).all()
    assert np.abs(row[:P] - want["g"]).max() <= lh.tol_g(n, want["g"])
    for q in range(4):                                  # sums of n terms, each within 2e-5 of the loss scales above
        scale = [np.abs(want["loss"][0]), np.abs(want["td"]).sum(),
                 np.abs(want["loss"][2]) + np.abs(want["td"]).sum() * 30 + n * c * np.log(A), want["loss"][3]][q]
        assert abs(row[P + q] - want["loss"][q]) <= 2e-5 * scale + 1e-12, q
    assert np.abs(L.entropy(n).cpu().numpy() - want["entropy"]).max() <= _entropy_tol(A)
    assert np.abs(td.cpu().numpy() - want["td"]).max() <= 2e-5 * (np.abs(want["td"]).max() + 1e-6)


@pytest.mark.parametrize("H,A,n,gather", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_uniform_policy_has_entropy_log_a_and_no_entropy_gradient(H, A, n, gather):
    blob0, b, store, cap, idx, it = lh.case(H, A, n, gather)
    blob = _with_fc2(blob0, H, A, 0.0, 0.0)
    outs = []
    for c in (0.0, 1.0):
        L = lh.learner(H, A, "per_sample", blob, n, c=c, diag=True)
        outs.append(lh.update(L, n, store, cap, it, None))
        L.check()
        assert np.abs(L.entropy(n).cpu().numpy() - np.log(A)).max() <= _entropy_tol(A)
    g = _mirror(H, A, n, gather, "per_sample", 1.0, False, blob)[3]
    lh.assert_step_from_zero(outs[1], blob, g, n, H, A)
    assert np.abs(outs[1]["exp_avg"] / 0.1 - outs[0]["exp_avg"] / 0.1).max() <= lh.tol_g(n, g)


# ---- 4. weights ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,gather", SMALL)
def test_weights_with_settings_on(H, A, n, gather):
    """Entropy and clipping on: a vector of ones is no weights, bitwise; weights of 0.5 halve words [0, P + 4) of a row
    exactly; a NaN weight still refuses."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    nr = mirror.norms(_mirror(H, A, n, gather, "per_sample", 0.5, False)[3], H, A)
    mgn = (float(nr[0] / 4), float(nr[1] / 4))
    outs = []
    for w in (None, torch.ones(n, device=DEV)):
        L = lh.learner(H, A, "per_sample", blob, n, c=0.5, mgn=mgn, diag=True)
        outs.append(dict(lh.update(L, n, store, cap, it, None, w), ent=L.entropy(n).cpu().numpy(),
                         norm=L.grad_norm.cpu().numpy()))
        L.check()
    lh.same(*outs)
    assert np.isfinite(outs[0]["norm"]).all() and np.array_equal(outs[0]["step"], np.ones(8))
    P = L.num_params
    before = lh.state(L)
    row_u, td_u = L._grad(n, store, cap, it)
    row_h, td_h = L._grad(n, store, cap, it, None, None, torch.full((n,), 0.5, device=DEV))
    L.check()
    row_u, row_h = row_u.cpu().numpy(), row_h.cpu().numpy()
    assert np.abs(row_u[:P]).max() > 0 and np.isfinite(row_u[:P + 4]).all()
    assert np.array_equal(row_h[:P + 4], np.float32(0.5) * row_u[:P + 4])
    assert np.array_equal(row_h[P + 4:].view(np.int32), row_u[P + 4:].view(np.int32))
    assert torch.equal(td_h, td_u)
    w = torch.ones(n, device=DEV)
    w[n // 2] = float("nan")
    al, cl, _ = L._run(n, store, cap, it, None, w)
    assert torch.isnan(al) and torch.isnan(cl) and torch.isnan(L.grad_norm).all()
    lh.same(lh.state(L), before)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()


# ---- 5. the clip ---------------------------------------------------------------------------------------------------------

def _max_norms(nr, which):
    """max norms a factor 4 away from the fp64 norms: clipped networks at norm / 4, the others at 4 norm (or inf)."""
    return {"both": (nr[0] / 4, nr[1] / 4), "actor": (nr[0] / 4, INF), "critic": (4 * nr[0], nr[1] / 4),
            "neither": (4 * nr[0], 4 * nr[1])}[which]


@pytest.mark.parametrize("which", ["both", "actor", "critic", "neither"])
@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n,gather", SMALL)
def test_clip_against_fp64_mirror(H, A, n, gather, loss, which):
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    c = 0.01 if loss == "per_sample" else 0.0
    weighted = loss == "reference"
    w = lh.dev(_weights(n)) if weighted else None
    ral, rcl, rtd, g, ent, _ = _mirror(H, A, n, gather, loss, c, weighted)
    nr = mirror.norms(g, H, A)
    mgn = _max_norms(nr, which)
    assert all(max(m / x, x / m) >= 1.05 for m, x in zip(mgn, nr))          # the decision is far from its knife edge
    coef, _, _ = mirror.clip_grad_norm(g, H, A, mgn)
    assert [x < 1 for x in coef] == [which in ("both", "actor"), which in ("both", "critic")]
    L = lh.learner(H, A, loss, blob, n, c=c, mgn=tuple(float(x) for x in mgn), diag=True)
    out = lh.update(L, n, store, cap, it, None, w)
    L.check()
    lh.assert_losses_and_td(out["actor_loss"], out["critic_loss"], out["td"], ral, rcl, rtd, c, A)
    lh.assert_step_from_zero(out, blob, g, n, H, A, coef)
    got = L.grad_norm.cpu().numpy()
    print("norms", got, nr)
    assert (np.abs(got - nr) <= np.sqrt(g.size) * lh.tol_g(n, g)).all(), (got, nr)
    if which == "neither":                      # bit for bit the unclipped update, and the norms are still written
        U = lh.learner(H, A, loss, blob, n, c=c)
        lh.same(_bits(out), lh.update(U, n, store, cap, it, None, w))
        U.check()


# ---- 6. the split form and the shared tail -------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[3], SHAPES[4]])
def test_one_row_applied_alone_is_the_closed_update(H, A, n, gather, loss):
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    c = 0.5 if loss == "per_sample" else 0.0
    nr = mirror.norms(_mirror(H, A, n, gather, loss, c, False)[3], H, A)
    mgn = (float(nr[0] / 4), float(nr[1] / 4))
    prio0 = torch.rand(cap, device=DEV) + 0.1
    outs = []
    for run in (lh.update, lh.split_update):
        L = lh.learner(H, A, loss, blob, n, c=c, mgn=mgn, diag=True)
        prio = prio0.clone()
        outs.append(dict(run(L, n, store, cap, it, prio), ent=L.entropy(n).cpu().numpy(), norm=L.grad_norm.cpu().numpy()))
        L.check()
    assert np.isfinite(outs[0]["norm"]).all() and not np.array_equal(outs[0]["prio"], prio0.cpu().numpy())
    lh.same(*outs)


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n,gather", [SHAPES[3], SHAPES[4]])
def test_three_rows_match_the_mirror_and_two_learners_stay_equal(H, A, n, gather, loss):
    """K = 3 rows of different n, applied together with entropy and clipping on, against the closed update of the
    concatenated batch in the mirror; the same rows applied on two learners that started equal leave them bitwise
    equal."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    c = 0.5 if loss == "per_sample" else 0.0
    ral, rcl, rtd, g, ent, _ = _mirror(H, A, n, gather, loss, c, False)
    nr = mirror.norms(g, H, A)
    mgn = (nr[0] / 4, nr[1] / 4)
    coef = mirror.clip_grad_norm(g, H, A, mgn)[0]
    one, two = (lh.learner(H, A, loss, blob, n, c=c, mgn=tuple(float(x) for x in mgn), diag=True) for _ in range(2))
    rows = one.new_rows(3)
    tds = []
    for k, (lo, hi) in enumerate(lh.cuts(n, 3, seed=n)):
        _, td = one._grad(hi - lo, store, cap, it[lo:hi].contiguous(), rows[k])
        tds.append(td)
    res = [L.apply(rows) for L in (one, two)]
    one.check(); two.check()
    lh.same(lh.state(one), lh.state(two))
    assert torch.equal(one.grad_norm, two.grad_norm)
    for x, y in zip(*res):
        assert torch.equal(x, y)
    lh.assert_losses_and_td(res[0][0].cpu().numpy(), res[0][1].cpu().numpy(), torch.cat(tds).cpu().numpy(), ral, rcl, rtd, c, A)
    lh.assert_step_from_zero(lh.state(one), blob, g, n, H, A, coef)
    assert (np.abs(one.grad_norm.cpu().numpy() - nr) <= np.sqrt(g.size) * lh.tol_g(n, g)).all()


# ---- 7. determinism and capture ------------------------------------------------------------------------------------------

def test_identical_calls_give_identical_bits():
    H, A, n, gather = SHAPES[3]
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    nr = mirror.norms(_mirror(H, A, n, gather, "per_sample", 0.3, False)[3], H, A)
    outs = []
    for _ in range(2):
        L = lh.learner(H, A, "per_sample", blob, n, c=0.3, mgn=(float(nr[0] / 4), float(nr[1] / 4)), diag=True)
        res = [lh.update(L, n, store, cap, it, None) for _ in range(3)]
        L.check()
        outs.append(res + [{"ent": L.entropy(n).cpu().numpy(), "norm": L.grad_norm.cpu().numpy()}])
    for x, y in zip(*outs):
        lh.same(x, y)


def test_graph_replay_matches_eager():
    """One update with entropy and clipping captured in a graph and replayed three times == three eager updates."""
    H, A, n, gather = SHAPES[3]
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    nr = mirror.norms(_mirror(H, A, n, gather, "per_sample", 0.3, False)[3], H, A)
    kw = dict(c=0.3, mgn=(float(nr[0] / 4), float(nr[1] / 4)), diag=True)
    prio_e = torch.rand(cap, device=DEV) + 0.1
    prio_g = prio_e.clone()
    eager = lh.learner(H, A, "per_sample", blob, n, **kw)
    graphed = lh.learner(H, A, "per_sample", blob, n, **kw)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = graphed._run(n, store, cap, it, prio_g)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(graphed)["step"], np.zeros(8))           # capture ran nothing
    for k in range(3):
        e_out = eager._run(n, store, cap, it, prio_e)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y), k
        lh.same(lh.state(graphed), lh.state(eager))
        assert torch.equal(prio_e, prio_g) and torch.equal(eager.grad_norm, graphed.grad_norm)
        assert torch.equal(eager.entropy(n), graphed.entropy(n))
    assert np.array_equal(lh.state(graphed)["step"], np.full(8, 3)) and torch.isfinite(graphed.grad_norm).all()
    assert float(graphed.grad_norm[0]) > kw["mgn"][0] and float(graphed.grad_norm[1]) > kw["mgn"][1]   # both clipped
    graphed.check(); eager.check()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------

def test_the_setter_refuses_bad_values_and_changes_nothing():
    H, A, n, gather = SHAPES[1]
    blob = lh.case(H, A, n, gather)[0]
    L = lh.learner(H, A, "per_sample", blob, n, c=0.25, mgn=(1.5, None))
    assert L.get_regularisation() == (0.25, 1.5, INF)
    for c, mgn in ((float("nan"), None), (-0.1, None), (INF, None), (0.1, 0.0), (0.1, (1.0, 0.0)), (0.1, float("nan")),
                   (0.1, (-1.0, 1.0))):
        with pytest.raises(RuntimeError, match="uavtrack_learner_set_regularisation: "):
            L.set_regularisation(c, mgn)
        assert L.get_regularisation() == (0.25, 1.5, INF)
    R = lh.learner(H, A, "reference", blob, n, mgn=2.0)
    assert R.get_regularisation() == (0.0, 2.0, 2.0)
    with pytest.raises(RuntimeError, match="UAVTRACK_LOSS_REFERENCE.*cannot share"):
        R.set_regularisation(0.1, 2.0)
    assert R.get_regularisation() == (0.0, 2.0, 2.0)
    with pytest.raises(RuntimeError, match="UAVTRACK_LOSS_REFERENCE"):
        _uav().DeviceActorCritic(12, H, A, device=DEV, loss="reference", entropy_coef=0.1)
    R.set_regularisation(0.0, None)
    assert R.get_regularisation() == (0.0, INF, INF)


def test_a_bad_action_with_clipping_on_changes_nothing():
    H, A, n, gather = SHAPES[2]
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    L = lh.learner(H, A, "per_sample", blob, n, c=0.1, mgn=(0.01, 0.01), diag=True)
    al, cl, _ = L._run(n, store, cap, it, None)
    L.check()
    assert torch.isfinite(L.grad_norm).all()
    before = lh.state(L)
    prio = torch.rand(cap, device=DEV) + 0.1
    prio0 = prio.clone()
    bad = {k: v.clone() for k, v in store.items()}
    bad["actions"][int(idx[40])] = A
    al, cl, _ = L._run(n, bad, cap, it, prio)
    assert torch.isnan(al) and torch.isnan(cl) and torch.isnan(L.grad_norm).all()
    assert float(L.entropy(n)[40]) == 0.0 and float(L.entropy(n)[39]) > 0.0
    lh.same(lh.state(L), before)
    assert torch.equal(prio, prio0)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    al, cl, _ = L._run(n, store, cap, it, prio)
    L.check()
    assert torch.isfinite(al) and torch.isfinite(L.grad_norm).all() and not torch.equal(prio, prio0)


def test_an_update_larger_than_the_entropy_buffer_is_refused_on_the_host():
    H, A, n, gather = SHAPES[1]
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    L = lh.learner(H, A, "per_sample", blob, n)
    L.enable_diagnostics(n - 1)
    before = lh.state(L)
    with pytest.raises(RuntimeError, match="entropy buffer holds 62"):
        L._run(n, store, cap, it, None)
    with pytest.raises(RuntimeError, match="entropy buffer holds 62"):
        L._grad(n, store, cap, it)
    lh.same(lh.state(L), before)
    L._run(n - 1, store, cap, it[:n - 1].contiguous(), None)
    L.disable_diagnostics()
    L._run(n, store, cap, it, None)
    L.check()
    assert np.array_equal(lh.state(L)["step"], np.full(8, 2))


# ---- 9. the example ------------------------------------------------------------------------------------------------------

def test_example_trains_with_both_terms_in_either_learner(capsys):
    """examples/train_maac.py --entropy-coef --max-grad-norm: both learners train, the printed lines carry the mean
    entropy and the two norms, without the flags the lines are what they were, and an entropy bonus on the device
    learner's reference loss exits with the library's message."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_maac
    common = ["--envs", "64", "--iters", "2", "--batch", "4096", "--updates", "2", "--replay", "prioritized"]
    reg = ["--entropy-coef", "0.01", "--max-grad-norm", "0.5"]
    for learner in (["--learner", "device", "--actor-loss", "per_sample", "--publish", "device"], ["--learner", "torch"]):
        hist = train_maac.main(common + learner + reg)
        assert len(hist) == 2 and np.isfinite(hist).all()
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == 2
        for ln in lines:
            ent = float(ln.split("entropy")[1].split()[0])
            norms = [float(x) for x in ln.split("grad norm")[1].split()[:2]]
            assert 0.0 < ent <= np.log(12) + 1e-4 and all(np.isfinite(norms)) and min(norms) > 0, ln
    train_maac.main(common + ["--learner", "device", "--actor-loss", "per_sample", "--publish", "device"])
    assert not any("entropy" in ln for ln in capsys.readouterr().out.splitlines())
    with pytest.raises(SystemExit, match="UAVTRACK_LOSS_REFERENCE"):
        train_maac.main(common + ["--learner", "device", "--actor-loss", "reference", "--entropy-coef", "0.01"])
