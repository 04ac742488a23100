"""The batch-normalised advantage of the device learner (uavtrack_learner_set_advantage, DeviceActorCritic.set_advantage)
on the MI355X: what is promised bitwise (a given pair of (0, 1) is the raw update, (0, 0.5) halves the actor's words, batch
is given fed its own statistics, split is closed, calls repeat, a captured graph replays, back to raw is raw); the
statistics against their exact restatement; the update against the float64 mirror at the harness's bounds; the edges.

Shapes (H, A, n) and cases are tests/learner_advantage_mirror.py's, whose premises tests/test_learner_advantage_cpu.py
pins; every case is a single update from zero moments."""
import types

import numpy as np
import pytest
import torch

import learner_advantage_mirror as am
import learner_harness as lh
import learner_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA
SHAPES = am.SHAPES
EPS = am.EPS_CLIP
NAN = float("nan")

_device = {}


def _case(H, A, n, gather):
    """am.host_case and its device copies: (case, store, device indices or None, device log_mu)."""
    c = am.host_case(H, A, n, gather)
    key = (H, A, n, gather)
    if key not in _device:
        _device[key] = ({k: lh.dev(x) for k, x in zip(lh.STORES, c.b)}, lh.dev(c.idx) if gather else None, lh.dev(c.log_mu))
    return (c,) + _device[key]


def _pair(mean, inv):
    return torch.tensor([mean, inv], dtype=torch.float32, device=DEV)


def _stats(L):
    return None if L.advantage_stats is None else L.advantage_stats.cpu().numpy()


def run(L, c, store, it, prio=None, w=None, d=None, mu=None, eps=None):
    """One closed update, the learner's state after it, the ratios and the statistics."""
    al, cl, td = L._run(c.n, store, c.cap, it, prio, w, d, mu, eps)
    return dict(lh._result(L, c.n, al, cl, td, prio), stats=_stats(L))


def run_split(L, c, store, it, prio=None, w=None, d=None, mu=None, eps=None):
    """The same update as grad -> apply -> write_priorities."""
    r, td = L._grad(c.n, store, c.cap, it, None, None, w, d, mu, eps)
    al, cl = L.apply(r)
    if prio is not None:
        L.write_priorities(types.SimpleNamespace(priorities=prio, capacity=c.cap), it, td)
    return dict(lh._result(L, c.n, al, cl, td, prio), stats=_stats(L))


def _theta(H, A):
    return mirror.critic_block(lh.init_blob(H, A, 4242), H, A)


# the variants of the update: name -> (learner options, target critic?, weights?, discount store?, clip_eps or None)
VARIANTS = {
    "plain": (dict(), False, False, False, None),
    "entropy+gradclip": (dict(c=0.01, mgn=(0.5, 0.5)), False, False, False, None),
    "weights": (dict(), False, True, False, None),
    "discounts": (dict(), False, False, True, None),
    "target": (dict(), True, False, False, None),
    "clip0.2": (dict(c=0.01), False, True, False, 0.2),
    "clip0": (dict(), False, False, False, 0.0),
}


def _make(c, variant, diag=True):
    """A learner of a variant over a case, and the arguments its updates take."""
    opts, target, weighted, discounted, eps = VARIANTS[variant]
    L = lh.learner(c.H, c.A, "per_sample", c.blob, c.n, diag=diag, **opts)
    if target:
        L.set_target(tau=0.5)
        L._set_target_params(_theta(c.H, c.A))
    kw = dict(w=lh.dev(am.weights(c.n)) if weighted else None,
              d=lh.dev(np.random.RandomState(c.n).uniform(0.0, 1.0, c.cap).astype(np.float32)) if discounted else None,
              eps=eps)
    return L, kw


def _prio(c):
    return torch.rand(c.cap, device=DEV, generator=torch.Generator(DEV).manual_seed(c.n)) + 0.1


# ---- bitwise ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[3]])
def test_a_given_pair_of_zero_and_one_leaves_the_bits_of_the_raw_update(H, A, n, gather, variant):
    """Parameters, both moments, step counts, both losses, td_delta, priorities, entropy(n) (and the ratios' effect) of
    two consecutive updates; the raw learner once with diagnostics (all of it) and once without (all but the entropies)."""
    c, store, it, mu = _case(H, A, n, gather)
    clip = VARIANTS[variant][4] is not None
    outs = {}
    for who in ("raw", "raw-bare", "given"):
        L, kw = _make(c, variant, diag=who != "raw-bare")
        if who == "given":
            L.set_advantage(_pair(0.0, 1.0))
            assert torch.is_tensor(L.get_advantage()[0])
        prio = _prio(c)
        outs[who] = [run(L, c, store, it, prio, mu=mu if clip else None, **kw) for _ in range(2)]
        L.check()
    for k in range(2):
        got, want, bare = outs["given"][k], outs["raw"][k], outs["raw-bare"][k]
        lh.same(got, want, (variant, k))
        lh.same({q: v for q, v in got.items() if q not in ("entropy", "grad_norm")}, bare, (variant, "bare", k))
    assert np.array_equal(got["step"], np.full(8, 2)) and np.isfinite(got["actor_loss"])
    assert not np.array_equal(got["prio"], _prio(c).cpu().numpy())


@pytest.mark.parametrize("clip", [False, True], ids=["per_sample", "clipped"])
@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[3]])
def test_a_given_inverse_of_one_half_halves_the_actor_and_nothing_else(H, A, n, gather, clip):
    c, store, it, mu = _case(H, A, n, gather)
    w = lh.dev(am.weights(n))
    rows = {}
    for inv in (None, 0.5):
        L = lh.learner(H, A, "per_sample", c.blob, n)
        if inv is not None:
            L.set_advantage(_pair(0.0, inv))
        r, td = L._grad(n, store, c.cap, it, None, None, w, None, mu if clip else None, EPS if clip else None)
        L.check()
        rows[inv] = (r.cpu().numpy(), td.cpu().numpy())
    (raw, td0), (half, td1) = rows[None], rows[0.5]
    P = mirror.layout(H, A)[1][8]
    na = mirror.layout(H, A)[1][4]
    assert np.array_equal(half[:na], np.float32(0.5) * raw[:na]) and np.abs(raw[:na]).max() > 0
    assert half[P + 2] == np.float32(0.5) * raw[P + 2] and raw[P + 2] != 0
    assert np.array_equal(half[na:P], raw[na:P]) and np.array_equal(half[[P, P + 1, P + 3]], raw[[P, P + 1, P + 3]])
    assert np.array_equal(half[P + 4:].view(np.int32), raw[P + 4:].view(np.int32)) and np.array_equal(td0, td1)


@pytest.mark.parametrize("variant", ["plain", "target", "discounts", "clip0.2"])
@pytest.mark.parametrize("H,A,n,gather", SHAPES)
def test_batch_is_given_fed_the_statistics_batch_wrote(H, A, n, gather, variant):
    c, store, it, mu = _case(H, A, n, gather)
    clip = VARIANTS[variant][4] is not None
    B, kw = _make(c, variant)
    B.set_advantage("batch")
    assert B.get_advantage() == ("batch", 1e-8)
    got = run(B, c, store, it, _prio(c), mu=mu if clip else None, **kw)
    B.check()
    assert np.isfinite(got["stats"]).all() and got["stats"][2] > 0
    G, kw = _make(c, variant)
    G.set_advantage(lh.dev(got["stats"][:2].copy()))
    want = run(G, c, store, it, _prio(c), mu=mu if clip else None, **kw)
    G.check()
    lh.same({q: v for q, v in got.items() if q != "stats"}, {q: v for q, v in want.items() if q != "stats"}, variant)
    assert np.array_equal(got["step"], np.ones(8))


@pytest.mark.parametrize("variant", ["entropy+gradclip", "clip0.2"])
@pytest.mark.parametrize("H,A,n,gather", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_split_is_closed_and_identical_calls_give_identical_bits(H, A, n, gather, variant):
    c, store, it, mu = _case(H, A, n, gather)
    clip = VARIANTS[variant][4] is not None
    outs = []
    for runner in (run, run, run_split):
        L, kw = _make(c, variant)
        L.set_advantage("batch")
        prio = _prio(c)
        outs.append([runner(L, c, store, it, prio, mu=mu if clip else None, **kw) for _ in range(3)])
        L.check()
    assert np.array_equal(outs[0][2]["step"], np.full(8, 3)) and np.isfinite(outs[0][2]["actor_loss"])
    for x, y, z in zip(*outs):
        lh.same(x, y)
        lh.same(x, z)


@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[3]])
def test_back_to_raw_after_batch_is_raw(H, A, n, gather):
    c, store, it, mu = _case(H, A, n, gather)
    for loss_kw in (dict(), dict(c=0.01)):
        first = lh.learner(H, A, "per_sample", c.blob, n, **loss_kw)
        want = [lh.update(first, n, store, c.cap, it, None) for _ in range(2)]
        first.check()
        L = lh.learner(H, A, "per_sample", c.blob, n, **loss_kw)
        L.set_advantage("batch")
        L.set_advantage("raw")
        assert L.get_advantage() == ("raw", 1e-8)
        got = [lh.update(L, n, store, c.cap, it, None) for _ in range(2)]
        L.check()
        for x, y in zip(got, want):
            lh.same(x, y)
        # and a learner that did update in batch mode, from the state it is in, is raw again
        M = lh.learner(H, A, "per_sample", c.blob, n, **loss_kw)
        M.set_advantage("batch")
        lh.update(M, n, store, c.cap, it, None)
        N = lh.learner(H, A, "per_sample", c.blob, n, **loss_kw)
        N._set_params(M._get_params()); N._set_optim_state(*M._optim_state())
        M.set_advantage("raw")
        lh.same(lh.update(M, n, store, c.cap, it, None), lh.update(N, n, store, c.cap, it, None))
        M.check(); N.check()


CAP, T, B, N = 257, 3, 4, 5


def _rollout(k):
    rng = np.random.default_rng(1000 + k)
    return (lh.dev(rng.uniform(-1, 1, (B, N, 12)).astype(np.float32)),
            {"obs": lh.dev(rng.uniform(-1, 1, (T, B, N, 12)).astype(np.float32)),
             "actions": lh.dev(rng.integers(0, 12, (T, B, N)).astype(np.int32)),
             "reward": lh.dev((3.0 + rng.uniform(-2, 2, (T, B, N))).astype(np.float32))})


def _filled_ring(L, seed=3):
    import uavtrack
    ring = uavtrack.ReplayRing(CAP, DEV, seed=seed, max_batch=64).with_behaviour()
    for k in range(5):
        ring.add_rollout_behaviour(*_rollout(k), behaviour=L)
    assert ring.count == CAP
    return ring


def test_a_captured_batch_mode_update_replays_with_fresh_statistics():
    """A captured update_from(ring, 63, clip_eps=0.2) in batch mode, replayed twice on a ring that changed in between,
    against two eager calls on a twin ring and learner: the same results, and new statistics each time."""
    blob = lh.init_blob(64, 12, 77)
    L1, L2 = (lh.learner(64, 12, "per_sample", blob, max_batch=64, c=0.01) for _ in range(2))
    r1, r2 = _filled_ring(L1), _filled_ring(L2)
    for L in (L1, L2):
        L._set_params(0.5 * (L._get_params() + lh.init_blob(64, 12, 78)))          # the actor moves on; log_mu stays
        L.set_advantage("batch")

    def iteration(L, ring):
        return L.update_from(ring, 63, clip_eps=0.2)

    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = iteration(L2, r2)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(L2)["step"], np.zeros(8))                      # capture ran nothing
    seen = []
    for k in range(2):
        e_out = iteration(L1, r1)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y) and torch.isfinite(x).all(), k
        lh.same(lh.state(L1), lh.state(L2), k)
        assert torch.equal(L1.advantage_stats, L2.advantage_stats) and torch.isfinite(L2.advantage_stats).all()
        td = g_out[2].cpu().numpy()
        assert _stats(L2)[0] == am.stats32(td)[0]
        seen.append(_stats(L2).copy())
        for ring, L in ((r1, L1), (r2, L2)):
            ring.add_rollout_behaviour(*_rollout(10 + k), behaviour=L)
    L1.check(); L2.check()
    assert lh.state(L1)["step"][0] == 2 and not np.array_equal(seen[0], seen[1])


# ---- exact statistics ------------------------------------------------------------------------------------------------

def _assert_stats(stats, td, eps=1e-8):
    """All three floats bit for bit the restatement's from the update's own td_delta (which also holds the TD pass to the
    gradient kernel's delta).  The contract allows inv_std and std one float32 ulp (an fp64 sqrt or division one ulp off
    can move the float32 rounding by that much); on the MI355X the device's fp64 sqrt and division came out correctly
    rounded in every case, so the test asks for equality."""
    want = am.stats32(td, eps)
    print(f"stats {stats} want {want}: ulps {[am.ulps(x, y) for x, y in zip(stats, want)]}")
    assert np.array_equal(stats, want)


@pytest.mark.parametrize("variant", ["plain", "target", "discounts", "clip0.2"])
@pytest.mark.parametrize("H,A,n,gather", SHAPES)
def test_the_statistics_are_the_restatement_of_the_updates_own_td(H, A, n, gather, variant):
    c, store, it, mu = _case(H, A, n, gather)
    clip = VARIANTS[variant][4] is not None
    L, kw = _make(c, variant)
    L.set_advantage("batch", 1e-6)
    out = run(L, c, store, it, None, mu=mu if clip else None, **kw)
    L.check()
    _assert_stats(out["stats"], out["td"], 1e-6)
    r, td = L._grad(n, store, c.cap, it, None, None, kw["w"], kw["d"], mu if clip else None, kw["eps"])
    _assert_stats(_stats(L), td.cpu().numpy(), 1e-6)


# ---- against fp64 ----------------------------------------------------------------------------------------------------

FORMS = {"plain": "plain", "entropy": "entropy+gradclip", "clipped": "clip0.2", "target": "target", "weights": "weights"}


def _assert_against(out, u, row, blob, n, H, A, c, ratio=None):
    """td and the critic loss at assert_losses_and_td's bounds; the actor loss at the harness's formula with the
    advantage in delta's place (times the ratio under the clipped surrogate); the gradient and the first Adam step at
    tol_g / assert_step_from_zero."""
    lh.assert_losses_and_td(u.actor_loss, out["critic_loss"], out["td"], u.actor_loss, u.critic_loss, u.td, c, A)
    scale = np.abs(row["adv"]) if ratio is None else ratio * np.abs(row["adv"])
    al_tol = 2e-5 * (abs(u.actor_loss) + np.mean(scale) * 30 + c * np.log(A))
    print(f"share of the bound: normalised actor loss {abs(float(out['actor_loss']) - u.actor_loss) / al_tol:.3f}")
    assert abs(float(out["actor_loss"]) - u.actor_loss) <= al_tol, (float(out["actor_loss"]), u.actor_loss)
    lh.assert_step_from_zero(out, blob, u.grad, n, H, A)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("H,A,n,gather", SHAPES)
def test_batch_mode_against_the_fp64_mirror(H, A, n, gather, form):
    c, store, it, mu = _case(H, A, n, gather)
    opts, target, weighted, _, eps = VARIANTS[FORMS[form]]
    ent = 0.01 if form in ("entropy", "clipped") else 0.0
    L = lh.learner(H, A, "per_sample", c.blob, n, c=ent)
    theta = _theta(H, A) if target else None
    if target:
        L.set_target(tau=0.5)
        L._set_target_params(theta)
    L.set_advantage("batch")
    w = am.weights(n) if weighted else None
    out = run(L, c, store, it, None, w=None if w is None else lh.dev(w), mu=mu if eps is not None else None, eps=eps)
    L.check()
    u, row = am.losses_and_grads(c.blob, H, A, *am.rows(c), GAMMA, weights=w, entropy_coef=np.float32(ent),
                                 clip=None if eps is None else (c.log_mu[c.idx], eps), theta=theta)
    _assert_against(out, u, row, c.blob, n, H, A, ent, u.ratio)
    raw = mirror.losses_and_grads(c.blob, H, A, *am.rows(c), GAMMA, "per_sample", weights=w, entropy_coef=np.float32(ent),
                                  clip=None if eps is None else (c.log_mu[c.idx], eps), theta=theta)
    if n > 2:                                 # the normalisation is in the result: the raw gradient is far outside the bound
        assert np.abs(out["exp_avg"] / 0.1 - raw.grad).max() > 100 * lh.tol_g(n, u.grad)


class _Shard:
    """A buffer that hands out a fixed slice of a store: what update_from_many needs of one."""
    priorities = discounts = None

    def __init__(self, store, cap, idx):
        self.store, self.capacity, self.idx, self.count = store, cap, idx, idx.numel()

    def _draw_batch(self, k, spec):
        return self.idx[:k], None


@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[2]])
def test_three_uneven_shards_are_standardised_each_by_its_own_statistics(H, A, n, gather):
    c, store, it, mu = _case(H, A, n, gather)
    it = it if it is not None else torch.arange(n, device=DEV)
    pieces = lh.cuts(n, 3, seed=n)
    L = lh.learner(H, A, "per_sample", c.blob, n, c=0.01)
    L.set_advantage("batch")
    al, cl, tds = L.update_from_many([_Shard(store, c.cap, it[lo:hi].contiguous()) for lo, hi in pieces], n)
    L.check()
    b = am.rows(c)
    rows = [am.shard_sums(c.blob, H, A, *(x[lo:hi] for x in b), GAMMA, entropy_coef=np.float32(0.01)) for lo, hi in pieces]
    ral, rcl, g = mirror.combine(rows, H, A, "per_sample")
    st = lh.state(L)
    assert np.array_equal(st["step"], np.ones(8))
    lh.assert_step_from_zero(st, c.blob, g, n, H, A)
    assert abs(float(cl) - rcl) <= 2e-5 * rcl + 1e-12
    adv = np.concatenate([r["adv"] for r in rows])
    assert abs(float(al) - ral) <= 2e-5 * (abs(ral) + np.mean(np.abs(adv)) * 30 + 0.01 * np.log(A))
    # standardising the whole batch at once is another update, far outside the bound
    whole = am.losses_and_grads(c.blob, H, A, *b, GAMMA, entropy_coef=np.float32(0.01))[0].grad
    if n == 257:                                                      # (thousands of i.i.d. rows per shard: nearly the same)
        assert np.abs(g - whole).max() > 10 * lh.tol_g(n, g)
    _assert_stats(_stats(L), tds[2].cpu().numpy())                   # the statistics are the last draw's


# ---- edges -----------------------------------------------------------------------------------------------------------

def test_equal_deltas_leave_the_actor_alone():
    """A zero critic and constant rewards: std = 0, inv_std = 1e8, every advantage exactly 0.  No NaN anywhere; the
    actor's parameters and moments are unchanged by the step, the critic steps as in raw."""
    H, A, n, gather = SHAPES[1]
    c, store, it, mu = _case(H, A, n, gather)
    na = mirror.layout(H, A)[1][4]
    blob = c.blob.copy()
    blob[na:] = 0.0
    flat = dict(store, rewards=torch.full((c.cap,), 2.5, device=DEV))
    outs = []
    for mode in ("raw", "batch"):
        L = lh.learner(H, A, "per_sample", blob, n)
        L.set_advantage(mode)
        outs.append(run(L, c, flat, it))
        L.check()
    raw, got = outs
    assert np.array_equal(got["stats"], np.array([2.5, 1e8, 0.0], np.float32))
    for k in ("params", "exp_avg", "exp_avg_sq", "td", "actor_loss", "critic_loss"):
        assert np.isfinite(got[k]).all(), k
    assert np.array_equal(got["params"][:na], blob[:na]) and not got["exp_avg"][:na].any() and not got["exp_avg_sq"][:na].any()
    assert np.array_equal(got["step"], np.ones(8)) and got["actor_loss"] == 0
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(got[k][na:], raw[k][na:]) and not np.array_equal(got["params"][na:], blob[na:])
    assert np.array_equal(got["td"], raw["td"]) and got["critic_loss"] == raw["critic_loss"]


def test_a_mean_of_a_thousand_standard_deviations():
    H, A, n, gather = SHAPES[3]
    c, store, it, mu = _case(H, A, n, gather)
    r = (1000.0 + np.random.RandomState(5).uniform(-1, 1, c.cap)).astype(np.float32)
    L = lh.learner(H, A, "per_sample", c.blob, n)
    L.set_advantage("batch")
    out = run(L, c, dict(store, rewards=lh.dev(r)), it)
    L.check()
    assert out["stats"][0] > 1000 * out["stats"][2] > 0
    _assert_stats(out["stats"], out["td"])


def _row_status(L, row):
    return int(row.cpu().numpy()[L.num_params + 6:L.num_params + 7].view(np.int32)[0])


def test_a_bad_action_in_batch_mode_is_a_no_op_with_nan_statistics():
    H, A, n, gather = SHAPES[1]
    c, store, it, mu = _case(H, A, n, gather)
    L = lh.learner(H, A, "per_sample", c.blob, n)
    L.set_advantage("batch")
    bad = dict(store, actions=store["actions"].clone())
    bad["actions"][int(c.idx[40])] = A
    before = lh.state(L)
    prio = _prio(c)
    for runner in (run, run_split):
        out = runner(L, c, bad, it, prio)
        assert np.isnan(out["actor_loss"]) and np.isnan(out["critic_loss"]) and np.isnan(out["stats"]).all()
        lh.same(lh.state(L), before)
        assert torch.equal(prio, _prio(c))
        with pytest.raises(RuntimeError, match="1 update"):
            L.check()
    good = run(L, c, store, it, prio)                                 # and the next good update writes them again
    L.check()
    assert np.isfinite(good["stats"]).all()


@pytest.mark.parametrize("pair", [(0.0, NAN), (0.0, float("inf")), (0.0, -1.0), (NAN, 1.0)])
def test_a_bad_given_pair_is_refused_on_the_device(pair):
    H, A, n, gather = SHAPES[1]
    c, store, it, mu = _case(H, A, n, gather)
    L = lh.learner(H, A, "per_sample", c.blob, n)
    given = _pair(*pair)
    L.set_advantage(given)
    row, td = L._grad(n, store, c.cap, it)
    assert _row_status(L, row) == 64
    before = lh.state(L)
    prio = _prio(c)
    for runner in (run, run_split):
        out = runner(L, c, store, it, prio)
        assert np.isnan(out["actor_loss"]) and np.isnan(out["critic_loss"])
        lh.same(lh.state(L), before)
        assert torch.equal(prio, _prio(c))
        with pytest.raises(RuntimeError, match="1 update"):
            L.check()
    given.copy_(_pair(0.0, 1.0))                                      # read when the launch runs: the same tensor, mended
    out = run(L, c, store, it, prio)
    L.check()
    assert np.array_equal(out["step"], np.ones(8)) and np.isfinite(out["actor_loss"])


def test_the_host_refuses_what_the_header_says_and_enqueues_nothing():
    H, A, n, gather = SHAPES[1]
    c, store, it, mu = _case(H, A, n, gather)
    from uavtrack import _lib
    p = _lib.ptr

    def last_error():
        return _lib.load().uavtrack_last_error().decode("utf-8", "replace")
    L = lh.learner(H, A, "per_sample", c.blob, n)
    R = lh.learner(H, A, "reference", c.blob, n)
    pair = _pair(0.0, 1.0)
    set_adv = L._lib.uavtrack_learner_set_advantage
    for mode in (_lib.ADVANTAGE_BATCH, _lib.ADVANTAGE_GIVEN):
        assert set_adv(R._h, mode, 1e-8, p(pair)) != 0 and "UAVTRACK_LOSS_REFERENCE" in last_error() and "mean 0" in last_error()
    assert set_adv(R._h, _lib.ADVANTAGE_RAW, 1e-8, None) == 0
    for eps in (NAN, -1e-8):
        assert set_adv(L._h, _lib.ADVANTAGE_BATCH, eps, None) != 0 and "eps" in last_error()
    assert set_adv(L._h, _lib.ADVANTAGE_GIVEN, 1e-8, None) != 0 and "given" in last_error()
    assert set_adv(L._h, 3, 1e-8, None) != 0 and "mode" in last_error()
    assert L.get_advantage() == ("raw", 1e-8)                        # a refused call changed nothing
    assert set_adv(L._h, _lib.ADVANTAGE_BATCH, 1e-8, None) == 0
    losses, td, row = torch.empty(2, device=DEV), torch.empty(n, device=DEV), torch.empty(L.row_floats, device=DEV)
    one = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert L._lib.uavtrack_learner_update(L._h, 1, *L._batch_args(store, c.cap, one), p(losses[0:1]), p(losses[1:2]), p(td),
                                          None, L._stream()) != 0 and "n >= 2" in last_error()
    assert L._lib.uavtrack_learner_grad(L._h, 1, *L._batch_args(store, c.cap, one), p(td), p(row), L._stream()) != 0
    assert "n >= 2" in last_error()
    L.check(); R.check()
    assert np.array_equal(lh.state(L)["step"], np.zeros(8)) and np.array_equal(lh.state(L)["params"], c.blob)
    with pytest.raises(ValueError, match="mean 0"):
        R.set_advantage("batch")


# ---- the example -----------------------------------------------------------------------------------------------------

def test_example_trains_on_normalised_advantages_and_prints_their_statistics(capsys):
    """examples/train_maac.py --normalise-advantage: the device learner with the clipped surrogate, two shards, and the
    torch learner train; every printed line carries the mean and std of td; --actor-loss reference is refused."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_maac
    common = ["--envs", "64", "--steps", "20", "--iters", "2", "--batch", "4096", "--updates", "2", "--normalise-advantage"]
    device = ["--learner", "device", "--actor-loss", "per_sample"]
    for extra in (["--replay", "prioritized", "--ppo-clip", "0.2", "--publish", "device"] + device,
                  ["--replay", "uniform-device", "--shards", "2", "--entropy-coef", "0.01"] + device,
                  ["--replay", "prioritized", "--ppo-clip", "0.2", "--learner", "torch"]):
        hist = train_maac.main(common + extra)                               # learner.check() inside: nothing was refused
        assert len(hist) == 2 and np.isfinite(hist).all(), extra
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == 2, extra
        for ln in lines:
            mean, std = float(ln.split("td mean")[1].split()[0]), float(ln.split("td mean")[1].split("std")[1].split()[0])
            assert np.isfinite(mean) and 0.0 < std < 100.0, ln
            assert np.isfinite(float(ln.split("critic loss")[1].split()[0])), ln
    with pytest.raises(SystemExit):
        train_maac.main(common + ["--replay", "prioritized", "--learner", "device"])
    assert "per_sample" in capsys.readouterr().err
