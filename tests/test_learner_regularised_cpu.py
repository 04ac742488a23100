"""tests/learner_mirror.py with the entropy bonus and the gradient-norm clip held against torch autograd in float64
(tests/learner_autograd.py; no GPU): the loss mean(w (-log p delta - c H)), its gradient, torch.nn.utils.clip_grad_norm_'s
coefficient and the clipped gradient, each to 1e-12 relative, for A in {2, 12, 48}, with and without weights; a policy
whose logits span more than 250 (fp32 probabilities underflow there) stays finite; and with c = 0 and no clip the mirror
is the mirror without them."""
import numpy as np
import pytest

import learner_autograd as ag
import learner_harness as lh
import learner_mirror as mirror
from learner_autograd import batch as _batch, blob as _blob, close as _close, wide as _wide

GAMMA = 0.95


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
    w = lh.make_weights(rng, n) if weighted else None
    al, cl, td, g, ent, _ = mirror.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, "per_sample", weights=w, entropy_coef=c)
    nr = mirror.norms(g, H, A)
    for max_norms in ((nr[0] / 4, nr[1] / 4), (4 * nr[0], nr[1] / 4), (nr[0] / 4, np.inf), (4 * nr[0], 4 * nr[1])):
        t = ag.update(blob, H, A, s, a, r, s2, GAMMA, "per_sample", w, c, max_norms)
        coef, nr2, gc = mirror.clip_grad_norm(g, H, A, max_norms)
        _close(al, t.actor_loss, "actor loss"); _close(cl, t.critic_loss, "critic loss")
        _close(g, t.grad, "gradient"); _close(ent, t.entropy, "entropy")
        _close(coef, t.coef, "coefficient"); _close(gc, t.clipped, "clipped gradient")
        assert [x == 1.0 for x in coef] == [m > x for m, x in zip(max_norms, nr)]
    if wide:
        logp, p, _ = mirror.policy(blob, H, A, s)
        assert (logp.max(axis=1) - logp.min(axis=1) > 250).all()
        assert (np.exp(logp.astype(np.float32)).min(axis=1) == 0).all()      # fp32 probabilities do underflow here
        assert (ent >= 0).all() and (ent <= np.log(A) + 1e-12).all()


def test_exact_zero_probabilities_add_nothing():
    """Logits 2000 apart: the small probabilities are exactly 0 even in float64, and the mirror stays finite."""
    H, A, n = 8, 12, 9
    blob = _wide(_blob(H, A, 1), H, A, span=22000.0)
    s, a, r, s2 = _batch(np.random.RandomState(2), n, A)
    al, cl, td, g, ent, _ = mirror.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, "per_sample", entropy_coef=1.0)
    assert (mirror.policy(blob, H, A, s)[1].min(axis=1) == 0).all()
    assert np.isfinite(al) and np.isfinite(g).all() and np.isfinite(ent).all() and (np.abs(ent) < 1e-300).all()


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
def test_without_settings_the_mirror_is_the_weighted_mirror(loss):
    H, A, n = 33, 12, 65
    rng = np.random.RandomState(5)
    blob = _blob(H, A, 5)
    s, a, r, s2 = _batch(rng, n, A)
    w = lh.make_weights(rng, n)
    al, cl, td, g = mirror.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, loss, weights=w, entropy_coef=0.0)[:4]
    wal, wcl, wtd, wg = mirror.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, loss, weights=w)[:4]
    _close(al, wal, "actor loss"); _close(cl, wcl, "critic loss"); _close(g, wg, "gradient")
    assert np.array_equal(td, wtd)
    coef, _, gc = mirror.clip_grad_norm(g, H, A, (np.inf, np.inf))
    assert np.array_equal(coef, [1.0, 1.0]) and np.array_equal(gc, g)
    with pytest.raises(ValueError, match="per-sample"):
        mirror.losses_and_grads(blob, H, A, s, a, r, s2, GAMMA, "reference", weights=w, entropy_coef=0.5)


def test_rows_add_up_to_the_whole_batch():
    """The row algebra: regularised shard sums, added and scaled once, are the regularised update of the whole batch."""
    H, A, n, c = 33, 12, 130, 0.3
    rng = np.random.RandomState(6)
    blob = _blob(H, A, 6)
    b = _batch(rng, n, A)
    w = lh.make_weights(rng, n)
    rows = [mirror.shard_sums(blob, H, A, *(x[lo:hi] for x in b), GAMMA, "per_sample", w[lo:hi], c)
            for lo, hi in ((0, 17), (17, 80), (80, n))]
    al, cl, g = mirror.combine(rows, H, A, "per_sample")
    wal, wcl, _, wg = mirror.losses_and_grads(blob, H, A, *b, GAMMA, "per_sample", weights=w, entropy_coef=c)[:4]
    _close(al, wal, "actor loss"); _close(cl, wcl, "critic loss"); _close(g, wg, "gradient")
