"""The clipped-surrogate actor loss of the device learner (uavtrack_learner_update_clipped / _grad_clipped,
DeviceActorCritic.update(log_mu=, clip_eps=), DrawSpec.clip_eps) on the MI355X: against the float64 mirror
(tests/learner_mirror.py with clip=) at the harness's bounds; on-policy it is the per-sample update bit for bit; the split
form; refusals on the device; determinism and graph capture; off is off.

Shapes are corners of learner_harness.SWEEP (learner_clipped_mirror.SHAPES).  Every case's log_mu store comes from
learner_clipped_mirror.clip_batch, whose premises tests/test_learner_clipped_cpu.py pins: rows gated on both sides and
rows passing (the one-row case: its row gated), none within a relative 1e-4 of the boundary that decides it."""
import types

import numpy as np
import pytest
import torch

import learner_clipped_mirror as cm
import learner_harness as lh
import learner_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV
GAMMA = lh.GAMMA
INF = float("inf")
SHAPES = cm.SHAPES
KEYS = ("params", "exp_avg", "exp_avg_sq", "step", "td", "critic_loss", "prio")


def _uav():
    import uavtrack
    return uavtrack


def _case(H, A, n, gather):
    """learner_harness.case plus the clipped case's per-slot log_mu, on the host and on the device."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    cb = cm.clip_batch(H, A, n, gather)
    return blob, b, store, cap, idx, it, cb["log_mu"], lh.dev(cb["log_mu"])


def _weights(n):
    return lh.make_weights(np.random.RandomState(n + 11), n)


def clipped(L, n, store, cap, it, prio, mu, eps, w=None):
    """One closed clipped update, the learner's state after it and the ratios."""
    ratio = torch.full((n,), -1.0, device=DEV)
    al, cl, td = L._run(n, store, cap, it, prio, w, None, mu, eps, ratio)
    return dict(lh._result(L, n, al, cl, td, prio), ratio=ratio.cpu().numpy())


def split_clipped(L, n, store, cap, it, prio, mu, eps, w=None):
    """The same update as grad_clipped -> apply -> write_priorities."""
    ratio = torch.full((n,), -1.0, device=DEV)
    r, td = L._grad(n, store, cap, it, None, None, w, None, mu, eps, ratio)
    al, cl = L.apply(r)
    if prio is not None:
        L.write_priorities(types.SimpleNamespace(priorities=prio, capacity=cap), it, td)
    return dict(lh._result(L, n, al, cl, td, prio), ratio=ratio.cpu().numpy())


_mirrors = {}


def _mirror(H, A, n, gather, eps, c, weighted):
    """The fp64 clipped update of a case, computed once: (actor_loss, critic_loss, td, gradient, entropy, ratios)."""
    key = (H, A, n, gather, eps, c, weighted)
    if key not in _mirrors:
        cb = cm.clip_batch(H, A, n, gather)
        idx = cb["idx"]
        _mirrors[key] = mirror.losses_and_grads(cb["blob"], H, A, *lh.gathered(cb["b"], idx), GAMMA, "per_sample",
                                                weights=_weights(n) if weighted else None, entropy_coef=np.float32(c),
                                                clip=(cb["log_mu"][idx], eps))
    return _mirrors[key]


def _assert_against(out, ref, blob, n, H, A, c):
    """td and the critic loss at assert_losses_and_td's bounds; the actor loss at the harness's formula with
    mean(r |delta|) in place of mean |delta| (each term's rounding is relative to its own size); the gradient and the
    first Adam step at tol_g / assert_step_from_zero; the ratios at 4e-6 r + 1e-7."""
    ral, rcl, rtd, g, ent, ratio = ref
    lh.assert_losses_and_td(ral, out["critic_loss"], out["td"], ral, rcl, rtd, c, A)      # (the actor loss: below)
    al_tol = 2e-5 * (abs(ral) + np.mean(ratio * np.abs(rtd)) * 30 + c * np.log(A))
    r_tol = 4e-6 * ratio + 1e-7
    print(f"share of the bound: clipped actor loss {abs(float(out['actor_loss']) - ral) / al_tol:.3f}, ratios "
          f"{np.max(np.abs(out['ratio'] - ratio) / r_tol):.3f}")
    assert abs(float(out["actor_loss"]) - ral) <= al_tol, (float(out["actor_loss"]), ral)
    assert (np.abs(out["ratio"] - ratio) <= r_tol).all()
    lh.assert_step_from_zero(out, blob, g, n, H, A)


# ---- 1. against the fp64 mirror ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("c", [0.0, 0.01])
@pytest.mark.parametrize("eps", [0.2, INF])
@pytest.mark.parametrize("H,A,n,gather", SHAPES)
def test_clipped_update_against_fp64_mirror(H, A, n, gather, eps, c, weighted):
    blob, b, store, cap, idx, it, mu_h, mu = _case(H, A, n, gather)
    w = lh.dev(_weights(n)) if weighted else None
    L = lh.learner(H, A, "per_sample", blob, n, c=c)
    out = clipped(L, n, store, cap, it, None, mu, eps, w)
    L.check()
    ref = _mirror(H, A, n, gather, eps, c, weighted)
    _assert_against(out, ref, blob, n, H, A, c)
    if eps == 0.2:                            # the gate is in the result: the unclipped gradient is far outside the bound
        g_inf = _mirror(H, A, n, gather, INF, c, weighted)[3]
        assert np.abs(out["exp_avg"] / 0.1 - g_inf).max() > 100 * lh.tol_g(n, ref[3])
        assert np.abs(ref[3] - g_inf).max() > 100 * lh.tol_g(n, ref[3])


@pytest.mark.parametrize("eps", [0.2, INF])
def test_clipped_update_with_a_target_critic_against_fp64_mirror(eps):
    """A target critic that differs from the critic: y = r + gamma V_target(s') in the mirror (theta=), log_mu built
    against those deltas."""
    H, A, n, gather = SHAPES[1]
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    theta = mirror.critic_block(lh.init_blob(H, A, 4242), H, A)
    cb = cm.clip_batch(H, A, n, gather, theta)
    c = 0.01
    L = lh.learner(H, A, "per_sample", blob, n, c=c)
    L.set_target(tau=0.5)
    L._set_target_params(theta)
    out = clipped(L, n, store, cap, it, None, lh.dev(cb["log_mu"]), eps)
    L.check()
    ref = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), GAMMA, "per_sample", entropy_coef=np.float32(c),
                                  clip=(cb["log_mu"][idx], eps), theta=theta)
    _assert_against(out, ref, blob, n, H, A, c)
    if eps == 0.2:
        g_inf = mirror.losses_and_grads(blob, H, A, *lh.gathered(b, idx), GAMMA, "per_sample", entropy_coef=np.float32(c),
                                        clip=(cb["log_mu"][idx], INF), theta=theta).grad
        assert np.abs(out["exp_avg"] / 0.1 - g_inf).max() > 100 * lh.tol_g(n, ref[3])
    want = mirror.polyak(theta, mirror.critic_block(out["params"], H, A), 0.5)       # and the sync rule ran behind the step
    assert np.array_equal(L._get_target_params(), want)


# ---- 2. on-policy is the per-sample update, bit for bit ------------------------------------------------------------------

@pytest.mark.parametrize("diag", [False, True], ids=["bare", "diag"])
@pytest.mark.parametrize("c", [0.01, 0.0])
@pytest.mark.parametrize("eps", [0.2, 0.0])
@pytest.mark.parametrize("H,A,n,gather", SHAPES)
def test_on_policy_the_clipped_update_is_the_per_sample_update_bit_for_bit(H, A, n, gather, eps, c, diag):
    """log_mu filled by log_probs on the same slots: every ratio is exactly 1.0f, on the boundary at eps = 0 (which pins
    the inclusive rule), and two consecutive updates leave the parameters, moments, steps, td_delta, critic loss and
    priorities of the per-sample update (whose actor loss is another expression of the same rows).  With c = 0 the
    reference learner is one with diagnostics installed (the logits path) and one without (the probabilities path)."""
    blob, b, store, cap, idx, it = lh.case(H, A, n, gather)
    w = lh.dev(_weights(n)) if (H + n) % 2 == 0 else None
    P = lh.learner(H, A, "per_sample", blob, n, c=c, diag=diag)
    Q = lh.learner(H, A, "per_sample", blob, n, c=c)
    prio0 = torch.rand(cap, device=DEV) + 0.1
    prio_p, prio_q = prio0.clone(), prio0.clone()
    for k in range(2):
        mu = Q.log_probs(store["states"], store["actions"])
        want = lh.update(P, n, store, cap, it, prio_p, w)
        got = clipped(Q, n, store, cap, it, prio_q, mu, eps, w)
        assert np.array_equal(got["ratio"], np.ones(n, np.float32)), k
        lh.same({q: got[q] for q in KEYS}, {q: want[q] for q in KEYS}, k)
        assert np.isfinite(got["actor_loss"])
    P.check(); Q.check()
    assert np.array_equal(got["step"], np.full(8, 2)) and not np.array_equal(got["prio"], prio0.cpu().numpy())


# ---- 3. split equals closed ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[3], SHAPES[4]])
def test_grad_apply_write_priorities_is_the_closed_clipped_update(H, A, n, gather):
    blob, b, store, cap, idx, it, mu_h, mu = _case(H, A, n, gather)
    w = lh.dev(_weights(n))
    prio0 = torch.rand(cap, device=DEV) + 0.1
    outs = []
    for run in (clipped, split_clipped):
        L = lh.learner(H, A, "per_sample", blob, n, c=0.01)
        prio = prio0.clone()
        outs.append([run(L, n, store, cap, it, prio, mu, 0.2, w) for _ in range(3)])
        L.check()
    assert np.array_equal(outs[0][2]["step"], np.full(8, 3)) and np.isfinite(outs[0][2]["actor_loss"])
    assert not np.array_equal(outs[0][2]["prio"], prio0.cpu().numpy())
    for x, y in zip(*outs):
        lh.same(x, y)


@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[4]])
def test_two_clipped_rows_and_a_mixed_pair_meet_the_mirrors_combine(H, A, n, gather):
    """Two clipped rows of uneven n applied together, and a clipped row with a plain per-sample row: both applies are
    accepted and are the mirror's combine of the same rows within tol_g."""
    blob, b, store, cap, idx, it, mu_h, mu = _case(H, A, n, gather)
    c, eps = 0.01, 0.2
    (lo0, hi0), (lo1, hi1) = lh.cuts(n, 2, seed=n)
    rows_of = lambda lo, hi: lh.gathered(b, idx[lo:hi])                                           # noqa: E731
    clip_row = lambda lo, hi: mirror.shard_sums(blob, H, A, *rows_of(lo, hi), GAMMA, "per_sample", None, np.float32(c),  # noqa: E731
                                                (mu_h[idx[lo:hi]], eps))
    plain_row = mirror.shard_sums(blob, H, A, *rows_of(lo1, hi1), GAMMA, "per_sample", None, np.float32(c))
    for second_clipped in (True, False):
        L = lh.learner(H, A, "per_sample", blob, n, c=c)
        rows = L.new_rows(2)
        L._grad(hi0 - lo0, store, cap, it[lo0:hi0].contiguous(), rows[0], None, None, None, mu, eps)
        if second_clipped:
            L._grad(hi1 - lo1, store, cap, it[lo1:hi1].contiguous(), rows[1], None, None, None, mu, eps)
        else:
            L._grad(hi1 - lo1, store, cap, it[lo1:hi1].contiguous(), rows[1])
        al, cl = L.apply(rows)
        L.check()
        ral, rcl, g = mirror.combine([clip_row(lo0, hi0), clip_row(lo1, hi1) if second_clipped else plain_row], H, A, "per_sample")
        st = lh.state(L)
        assert np.array_equal(st["step"], np.ones(8))
        lh.assert_step_from_zero(st, blob, g, n, H, A)
        assert abs(float(cl) - rcl) <= 2e-5 * rcl + 1e-12
        if second_clipped:
            g_inf = _mirror(H, A, n, gather, INF, c, False)[3]
            assert np.abs(g - _mirror(H, A, n, gather, eps, c, False)[3]).max() <= 1e-9 * np.abs(g).max()
            assert np.abs(st["exp_avg"] / 0.1 - g_inf).max() > 100 * lh.tol_g(n, g)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------

def _row_status(L, row):
    return int(row.cpu().numpy()[L.num_params + 6:L.num_params + 7].view(np.int32)[0])


@pytest.mark.parametrize("what,value", [("unknown", float("nan")), ("positive", 0.5), ("overflow", -200.0)])
def test_a_bad_behaviour_log_prob_refuses_on_the_device(what, value):
    """One drawn slot whose log_mu is NaN, +0.5, or -200 (a ratio of e^197 and more: not finite): status bit 4 in the
    row, state and priorities untouched, NaN losses, check() counts one; with a bad action as well, both bits; the same
    bad slot where it is not drawn refuses nothing."""
    H, A, n, gather = SHAPES[1]
    blob, b, store, cap, idx, it, mu_h, mu = _case(H, A, n, gather)
    logp = mirror.policy(blob, H, A, b[0])[0][np.arange(cap), b[1].astype(np.int64)]
    k = 40
    slot = int(idx[k])
    undrawn = int(np.setdiff1d(np.arange(cap), idx)[0])
    if what == "overflow":
        assert logp[slot] + 200.0 > 100.0 and logp[undrawn] + 200.0 > 100.0      # expf overflows well below that
    L = lh.learner(H, A, "per_sample", blob, n, c=0.01, diag=True)
    bad = mu.clone()
    bad[slot] = value
    ratio = torch.full((n,), -1.0, device=DEV)
    row, td = L._grad(n, store, cap, it, None, None, None, None, bad, 0.2, ratio)
    assert _row_status(L, row) == 16
    r = ratio.cpu().numpy()
    hit = idx == slot
    assert np.isnan(r[hit]).all() and np.isfinite(r[~hit]).all() and (r[~hit] > 0).all()
    assert (L.entropy(n).cpu().numpy()[hit] == 0).all()
    before = lh.state(L)
    prio = torch.rand(cap, device=DEV) + 0.1
    prio0 = prio.clone()
    for run in (clipped, split_clipped):
        out = run(L, n, store, cap, it, prio, bad, 0.2)
        assert np.isnan(out["actor_loss"]) and np.isnan(out["critic_loss"])
        lh.same(lh.state(L), before)
        assert torch.equal(prio, prio0)
        with pytest.raises(RuntimeError, match="1 update"):
            L.check()
    # a bad action together with the bad log_mu: both bits
    acts = {q: v.clone() for q, v in store.items()}
    acts["actions"][int(idx[3])] = A
    row, _ = L._grad(n, acts, cap, it, None, None, None, None, bad, 0.2)
    assert _row_status(L, row) == 17
    # the bad slot where nothing draws it: nothing is refused, and the update is the one with the good store
    assert undrawn not in idx
    spare = mu.clone()
    spare[undrawn] = value
    row, _ = L._grad(n, store, cap, it, None, None, None, None, spare, 0.2)
    assert _row_status(L, row) == 0
    got = clipped(L, n, store, cap, it, prio, spare, 0.2)
    L.check()
    M = lh.learner(H, A, "per_sample", blob, n, c=0.01, diag=True)
    lh.same(got, clipped(M, n, store, cap, it, prio0.clone(), mu, 0.2))
    M.check()


def test_the_host_refuses_what_the_header_says_and_enqueues_nothing():
    H, A, n, gather = SHAPES[1]
    blob, b, store, cap, idx, it, mu_h, mu = _case(H, A, n, gather)
    from uavtrack import _lib
    p = _lib.ptr

    def last_error():
        return _lib.load().uavtrack_last_error().decode("utf-8", "replace")
    L = lh.learner(H, A, "per_sample", blob, n)
    R = lh.learner(H, A, "reference", blob, n)
    before = lh.state(L)
    losses, td, row = torch.empty(2, device=DEV), torch.empty(n, device=DEV), torch.empty(L.row_floats, device=DEV)

    def update(h, log_mu, eps):
        return h._lib.uavtrack_learner_update_clipped(h._h, n, *h._batch_args(store, cap, it), None, None, p(log_mu), eps,
                                                      None, p(losses[0:1]), p(losses[1:2]), p(td), None, h._stream())

    def grad(h, log_mu, eps):
        return h._lib.uavtrack_learner_grad_clipped(h._h, n, *h._batch_args(store, cap, it), None, None, p(log_mu), eps,
                                                    None, p(td), p(row), h._stream())

    for call in (update, grad):
        assert call(L, None, 0.2) != 0 and "log_mu" in last_error()
        for eps in (float("nan"), -0.1, -INF):
            assert call(L, mu, eps) != 0 and "clip_eps" in last_error()
        assert call(R, mu, 0.2) != 0 and "UAVTRACK_LOSS_REFERENCE" in last_error() and "cannot share" in last_error()
        assert call(L, mu, INF) == 0 and call(L, mu, 0.0) == 0
    L.check(); R.check()
    assert np.array_equal(lh.state(L)["step"], np.full(8, 2))                # the two accepted updates, nothing else
    assert np.array_equal(lh.state(R)["step"], np.zeros(8)) and not np.array_equal(lh.state(L)["params"], before["params"])
    with pytest.raises(ValueError, match="cannot share"):
        R.update({q: store[q][:n] for q in lh.STORES}, log_mu=mu[:n], clip_eps=0.2)


# ---- 5. determinism and capture ------------------------------------------------------------------------------------------

def test_identical_calls_give_identical_bits():
    H, A, n, gather = SHAPES[3]
    blob, b, store, cap, idx, it, mu_h, mu = _case(H, A, n, gather)
    outs = []
    for _ in range(2):
        L = lh.learner(H, A, "per_sample", blob, n, c=0.01)
        outs.append([clipped(L, n, store, cap, it, None, mu, 0.2) for _ in range(3)])
        L.check()
    for x, y in zip(*outs):
        lh.same(x, y)


CAP, T, B, N = 257, 3, 4, 5


def _filled_ring(kind, L, seed=3):
    """A behaviour ring of 257 slots behind five rollouts of 60 transitions, log_mu by the learner as it stands."""
    u = _uav()
    ring = (u.PrioritizedReplayRing if kind == "prioritised" else u.ReplayRing)(CAP, DEV, seed=seed, max_batch=64)
    ring.with_behaviour()
    for k in range(5):
        rng = np.random.default_rng(1000 + k)
        obs_in = lh.dev(rng.uniform(-1, 1, (B, N, 12)).astype(np.float32))
        out = {"obs": lh.dev(rng.uniform(-1, 1, (T, B, N, 12)).astype(np.float32)),
               "actions": lh.dev(rng.integers(0, 12, (T, B, N)).astype(np.int32)),
               "reward": lh.dev(rng.uniform(-2, 2, (T, B, N)).astype(np.float32))}
        ring.add_rollout_behaviour(obs_in, out, behaviour=L)
    assert ring.count == CAP
    return ring


def _twins():
    blob = lh.init_blob(64, 12, 77)
    return [lh.learner(64, 12, "per_sample", blob, max_batch=64, c=0.01) for _ in range(2)]


def _move_on(L):
    """The actor moves on; the ring's log_mu stays."""
    L._set_params(0.5 * (L._get_params() + lh.init_blob(64, 12, 78)))


def test_update_from_captures_into_one_graph():
    """A captured update_from(ring, k, clip_eps=0.2, ratio_out=buf) replayed three times == three eager calls on a twin
    ring and learner."""
    L1, L2 = _twins()
    r1, r2 = _filled_ring("prioritised", L1), _filled_ring("prioritised", L2)
    _move_on(L1); _move_on(L2)
    q1, q2 = torch.empty(63, device=DEV), torch.empty(63, device=DEV)

    def iteration(L, ring, buf):
        return L.update_from(ring, 63, importance=True, clip_eps=0.2, ratio_out=buf)

    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = iteration(L2, r2, q2)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(L2)["step"], np.zeros(8))                # capture ran nothing
    for k in range(3):
        e_out = iteration(L1, r1, q1)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out, g_out):
            assert torch.equal(x, y) and torch.isfinite(x).all(), k
        assert torch.equal(q1, q2) and not (q1 == 1.0).all() and (q1 > 0).all()
        lh.same(lh.state(L1), lh.state(L2), k)
        assert torch.equal(r1.priorities, r2.priorities)
    L1.check(); L2.check()
    assert lh.state(L1)["step"][0] == 3


def test_the_drawn_paths_are_the_explicit_clipped_calls():
    """update_from on a uniform ring, grad_from and update_from_many with clip_eps: the bits of the ring's draw followed
    by the explicit clipped update or rows, the ratios of every buffer in its own ratio_out."""
    from uavtrack.replay import DrawSpec
    L1, L2 = _twins()
    rings1 = [_filled_ring("uniform", L1, 3), _filled_ring("prioritised", L1, 4)]
    rings2 = [_filled_ring("uniform", L2, 3), _filled_ring("prioritised", L2, 4)]
    _move_on(L1); _move_on(L2)
    q = torch.empty(40, device=DEV)
    al, cl, td = L1.update_from(rings1[0], 40, clip_eps=0.1, ratio_out=q)
    i, w = rings2[0]._draw_batch(40, DrawSpec())
    assert w is None
    want = clipped(L2, 40, rings2[0].store, CAP, i, None, rings2[0].log_mu, 0.1)
    lh.same(dict(lh.state(L1), td=td.cpu().numpy(), al=al.cpu().numpy()), dict(lh.state(L2), td=want["td"], al=want["actor_loss"]))
    assert np.array_equal(q.cpu().numpy(), want["ratio"]) and (np.abs(want["ratio"] - 1) > 0.1).any()
    qs = [torch.empty(40, device=DEV) for _ in rings1]
    al, cl, tds = L1.update_from_many(rings1, 40, importance=True, clip_eps=0.1, ratio_out=qs)
    rows = L2.new_rows(2)
    drawn = []
    for k, ring in enumerate(rings2):
        i, w = ring._draw_batch(40, DrawSpec(importance=True))
        ratio = torch.empty(40, device=DEV)
        _, t = L2._grad(40, ring.store, CAP, i, rows[k], None, w, None, ring.log_mu, 0.1, ratio)
        drawn.append((i.clone(), t, ratio))
    al2, cl2 = L2.apply(rows)
    for ring, (i, t, _) in zip(rings2, drawn):
        L2.write_priorities(ring, i, t)
    L1.check(); L2.check()
    lh.same(lh.state(L1), lh.state(L2))
    assert torch.equal(al, al2) and torch.equal(cl, cl2) and torch.isfinite(al)
    for a, x, (_, t, ratio) in zip(tds, qs, drawn):
        assert torch.equal(a, t) and torch.equal(x, ratio)
    assert torch.equal(rings1[1].priorities, rings2[1].priorities)


# ---- 6. off is off -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n,gather", [SHAPES[1], SHAPES[4]])
def test_off_is_off(H, A, n, gather, loss):
    """After clipped updates on another handle, three plain updates on a fresh handle, closed and split, are bit for bit
    those of a handle made before any clipped call ran (the comparison test_hip_learner_regularised.py::test_off_is_off
    makes for the regularisation)."""
    blob, b, store, cap, idx, it, mu_h, mu = _case(H, A, n, gather)
    prio0 = torch.rand(cap, device=DEV) + 0.1
    for run in (lh.update, lh.split_update):
        first = lh.learner(H, A, loss, blob, n)
        prio = prio0.clone()
        want = [run(first, n, store, cap, it, prio) for _ in range(3)]
        first.check()
        other = lh.learner(H, A, "per_sample", blob, n, c=0.01)
        clipped(other, n, store, cap, it, None, mu, 0.2)
        other.check()
        fresh = lh.learner(H, A, loss, blob, n)
        prio = prio0.clone()
        got = [run(fresh, n, store, cap, it, prio) for _ in range(3)]
        fresh.check()
        assert np.array_equal(got[2]["step"], np.full(8, 3)) and np.isfinite(got[2]["actor_loss"])
        for x, y in zip(got, want):
            lh.same(x, y)


# ---- the example ---------------------------------------------------------------------------------------------------------

def test_example_trains_with_the_clipped_surrogate_and_prints_the_ratios(capsys):
    """examples/train_maac.py --ppo-clip 0.2: the device learner (prioritised ring with importance weights, device publish,
    one printed line per two iterations), two shards over uniform rings, and the torch learner train; every printed line
    carries the mean ratio, the share of rows beyond the clip range and mean(-log r); what the flag excludes is refused
    with a message."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_maac
    common = ["--envs", "64", "--steps", "20", "--iters", "2", "--batch", "4096", "--updates", "2", "--ppo-clip", "0.2"]
    device = ["--learner", "device", "--actor-loss", "per_sample"]
    for extra, printed in ((["--replay", "prioritized", "--publish", "device", "--log-every", "2", "--importance"] + device, 1),
                           (["--replay", "uniform-device", "--shards", "2", "--entropy-coef", "0.01"] + device, 2),
                           (["--replay", "prioritized", "--learner", "torch"], 2)):
        hist = train_maac.main(common + extra)                               # learner.check() inside: nothing was refused
        assert len(hist) == 2 and np.isfinite(hist).all(), extra
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
        assert len(lines) == printed, extra
        for ln in lines:
            mean, share = float(ln.split("ratio mean")[1].split()[0]), float(ln.split("clipped")[1].split()[0])
            kl = float(ln.split(" kl ")[1].split()[0])
            assert 0.5 < mean < 2.0 and 0.0 <= share <= 1.0 and abs(kl) < 0.5, ln
            assert np.isfinite(float(ln.split("critic loss")[1].split()[0])), ln
    for bad, word in ((["--replay", "uniform"], "--ppo-clip"), (["--replay", "prioritized", "--rho-bar", "1.0"], "exclude"),
                      (["--replay", "prioritized", "--learner", "device"], "per_sample")):
        with pytest.raises(SystemExit):
            train_maac.main(common + bad)
        assert word in capsys.readouterr().err
