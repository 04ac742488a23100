"""tests/learner_regularised_mirror.py held against torch autograd in float64 (no GPU): the loss
mean(w (-log p delta - c H)), its gradient, torch.nn.utils.clip_grad_norm_'s coefficient and the clipped gradient, each
to 1e-12 relative, for A in {2, 12, 48}, with and without weights; a policy whose logits span more than 250 (fp32
probabilities underflow there) stays finite; and with c = 0 and no clip the mirror is the weighted mirror's."""
import numpy as np
import pytest
import torch

import learner_mirror as mirror
import learner_regularised_mirror as rm
import learner_weighted_mirror as wm

GAMMA = 0.95
REL = 1e-12


def _blob(H, A, seed):
    rng = np.random.RandomState(seed)
    sizes = mirror.layout(H, A)[0]
    return np.concatenate([rng.uniform(-1, 1, k) / np.sqrt(12 if t in (0, 1, 4, 5) else H)
                           for t, k in enumerate(sizes)]).astype(np.float32)


def _batch(rng, n, A):
    s = rng.uniform(-1, 1, size=(n, 12)).astype(np.float32)
    s2 = rng.uniform(-1, 1, size=(n, 12)).astype(np.float32)
    a = rng.randint(0, A, size=n).astype(np.int32)
    r = rng.uniform(-2, 2, size=n).astype(np.float32)
    return s, a, r, s2


def _wide(blob, H, A, span=300.0):
    """The same networks with the actor's fc2.bias a ramp of `span`: every row's logits span more than 250."""
    out = blob.copy()
    o = mirror.layout(H, A)[1]
    out[o[3]:o[4]] = np.linspace(0.0, span, A).astype(np.float32)
    return out


def _torch_update(blob, H, A, s, a, r, s2, weights, c, max_norms):
    """(actor_loss, critic_loss, gradient, coefficients, clipped gradient) by autograd and clip_grad_norm_ in float64."""
    t = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in mirror.unpack(blob, H, A)]
    w1a, b1a, w2a, b2a, w1c, b1c, w2c, b2c = t
    S, S2, R = (torch.from_numpy(np.asarray(x, np.float64)) for x in (s, s2, r))
    W = torch.ones(len(a), dtype=torch.float64) if weights is None else torch.from_numpy(np.asarray(weights, np.float64))
    critic = lambda x: (torch.relu(x @ w1c.T + b1c) @ w2c.T)[:, 0] + b2c[0]
    logp = torch.log_softmax(torch.relu(S @ w1a.T + b1a) @ w2a.T + b2a, dim=1)
    ent = -(logp.exp() * logp).sum(dim=1)
    target = (R + GAMMA * critic(S2)).detach()
    v = critic(S)
    delta = (target - v).detach()
    lpa = logp.gather(1, torch.from_numpy(np.asarray(a, np.int64)).view(-1, 1))[:, 0]
    al = torch.mean(W * (-lpa * delta - c * ent))
    cl = torch.mean(W * (v - target) ** 2)
    al.backward(); cl.backward()
    g = np.concatenate([x.grad.numpy().ravel() for x in t])
    coefs = []
    for params, mx in ((t[:4], max_norms[0]), (t[4:], max_norms[1])):
        if np.isinf(mx):
            coefs.append(1.0)
            continue
        total = torch.nn.utils.clip_grad_norm_(params, mx)
        coefs.append(min(1.0, mx / (float(total) + 1e-6)))
    gc = np.concatenate([x.grad.numpy().ravel() for x in t])
    return float(al.detach()), float(cl.detach()), g, np.array(coefs), gc, ent.detach().numpy()


def _close(x, y, what):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert np.isfinite(x).all() and np.isfinite(y).all(), what
    err, scale = np.abs(x - y).max(), max(np.abs(y).max(), 1e-300)
    assert err <= REL * scale, (what, err, scale)


@pytest.mark.parametrize("wide", [False, True], ids=["init", "span300"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("c", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("A", [2, 12, 48])
def test_mirror_against_autograd_and_clip_grad_norm(A, c, weighted, wide):
    H, n = 33, 65
    rng = np.random.RandomState(A * 10 + int(weighted))
    blob = _blob(H, A, A)
    if wide:
        blob = _wide(blob, H, A)
    s, a, r, s2 = _batch(rng, n, A)
    w = wm.make_weights(rng, n) if weighted else None
    al, cl, td, g, ent = rm.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, "per_sample", w, c)
    nr = rm.norms(g, H, A)
    for max_norms in ((nr[0] / 4, nr[1] / 4), (4 * nr[0], nr[1] / 4), (nr[0] / 4, np.inf), (4 * nr[0], 4 * nr[1])):
        tal, tcl, tg, tcoef, tgc, tent = _torch_update(blob, H, A, s, a, r, s2, w, c, max_norms)
        coef, nr2, gc = rm.clip(g, H, A, max_norms)
        _close(al, tal, "actor loss"); _close(cl, tcl, "critic loss")
        _close(g, tg, "gradient"); _close(ent, tent, "entropy")
        _close(coef, tcoef, "coefficient"); _close(gc, tgc, "clipped gradient")
        assert [x == 1.0 for x in coef] == [m > x for m, x in zip(max_norms, nr)]
    if wide:
        logp, p, _ = rm.policy(blob, H, A, s)
        assert (logp.max(axis=1) - logp.min(axis=1) > 250).all()
        assert (np.exp(logp.astype(np.float32)).min(axis=1) == 0).all()      # fp32 probabilities do underflow here
        assert (ent >= 0).all() and (ent <= np.log(A) + 1e-12).all()


def test_exact_zero_probabilities_add_nothing():
    """Logits 2000 apart: the small probabilities are exactly 0 even in float64, and the mirror stays finite."""
    H, A, n = 8, 12, 9
    blob = _wide(_blob(H, A, 1), H, A, span=22000.0)
    s, a, r, s2 = _batch(np.random.RandomState(2), n, A)
    al, cl, td, g, ent = rm.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, "per_sample", None, 1.0)
    assert (rm.policy(blob, H, A, s)[1].min(axis=1) == 0).all()
    assert np.isfinite(al) and np.isfinite(g).all() and np.isfinite(ent).all() and (np.abs(ent) < 1e-300).all()


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_without_settings_the_mirror_is_the_weighted_mirror(loss):
    H, A, n = 33, 12, 65
    rng = np.random.RandomState(5)
    blob = _blob(H, A, 5)
    s, a, r, s2 = _batch(rng, n, A)
    w = wm.make_weights(rng, n)
    al, cl, td, g, _ = rm.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, loss, w, 0.0)
    wal, wcl, wtd, wg = wm.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, loss, w)
    _close(al, wal, "actor loss"); _close(cl, wcl, "critic loss"); _close(g, wg, "gradient")
    assert np.array_equal(td, wtd)
    coef, _, gc = rm.clip(g, H, A, (np.inf, np.inf))
    assert np.array_equal(coef, [1.0, 1.0]) and np.array_equal(gc, g)
    with pytest.raises(ValueError, match="per-sample"):
        rm.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, "reference", w, 0.5)


def test_rows_add_up_to_the_whole_batch():
    """The row algebra: regularised shard sums, added and scaled once, are the regularised update of the whole batch."""
    import learner_dp_mirror as dp
    H, A, n, c = 33, 12, 130, 0.3
    rng = np.random.RandomState(6)
    blob = _blob(H, A, 6)
    b = _batch(rng, n, A)
    w = wm.make_weights(rng, n)
    rows = [rm.shard_sums(blob, H, A, *(x[lo:hi] for x in b), GAMMA, "per_sample", w[lo:hi], c)
            for lo, hi in ((0, 17), (17, 80), (80, n))]
    al, cl, g = dp.combine(rows, H, A, "per_sample")
    wal, wcl, _, wg, _ = rm.losses_and_grads(blob, H, A, *b, GAMMA, "per_sample", w, c)
    _close(al, wal, "actor loss"); _close(cl, wcl, "critic loss"); _close(g, wg, "gradient")
