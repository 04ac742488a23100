"""float64 numpy mirror of the regularised learner update (uavtrack_learner_set_regularisation), built on
tests/learner_mirror.py and tests/learner_weighted_mirror.py, which stay the yardsticks of the unregularised update:
    actor_loss, "per_sample"  = mean_i( w_i ( -log p_i(a_i) delta_i - c H_i ) ),   H_i = -sum_o p_io log p_io
    dL/dz_io                  = -(1/n) w_i ( delta_i (onehot - p_i)_o - c p_io (log p_io + H_i) )
and torch.nn.utils.clip_grad_norm_ per network: coef = min(1, max_norm / (norm + 1e-6)) on the flat gradient's actor
and critic parts.  Every log p comes from the logits, (z - max) - log sum exp(z - max), so nothing here needs a
probability to be representable: a probability of exactly 0 contributes 0 to H and to its gradient."""
import numpy as np

import learner_mirror as mirror
import learner_weighted_mirror as wm


def policy(blob, H, A, s):
    """(log p [n][A], p, entropy [n]) of the actor on states s, from the logits."""
    w1a, b1a, w2a, b2a = mirror.unpack(blob, H, A)[:4]
    s = np.asarray(s, np.float64)
    z = np.maximum(s @ w1a.T + b1a, 0) @ w2a.T + b2a
    d = z - z.max(axis=1, keepdims=True)
    logp = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    plogp = np.where(p > 0, p * logp, 0.0)
    return logp, p, -plogp.sum(axis=1)


def _terms(blob, H, A, s, a, r, s2, gamma, loss, weights, c):
    """The unscaled per-row pieces: forward dict, weights, logit weights [n][A], value weights [n], the four loss terms."""
    if c != 0 and loss != "per_sample":
        raise ValueError("the entropy bonus exists for the per-sample loss only")
    with np.errstate(divide="ignore"):          # its nlp = -log(p) is not used here; p may be exactly 0
        f = wm._forward(blob, H, A, s, a, r, s2, gamma)
    n, delta, v, target = f["n"], f["delta"], f["v"], f["target"]
    iw = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    assert iw.shape == (n,)
    logp, p, ent = policy(blob, H, A, s)
    nlp = -logp[np.arange(n), np.asarray(a, np.int64)]
    pg = (delta if loss == "per_sample" else np.ones(n))[:, None] * (f["onehot"] - p)
    eg = np.where(p > 0, p * (logp + ent[:, None]), 0.0)
    gz = iw[:, None] * (pg - c * eg)
    gv = (v - target) * iw
    lt = np.stack([nlp * iw, delta * iw, iw * (nlp * delta - c * ent), (v - target) ** 2 * iw])
    return f, iw, gz, gv, lt, ent


def losses_and_grads(blob, H, A, s, a, r, s2, gamma, loss="per_sample", weights=None, entropy_coef=0.0):
    """(actor_loss, critic_loss, td_delta, flat gradient, entropy [n]) of one update in float64, before any clip."""
    f, iw, gz, gv, lt, ent = _terms(blob, H, A, s, a, r, s2, gamma, loss, weights, float(entropy_coef))
    n = f["n"]
    if loss == "reference":
        actor_loss = lt[0].mean() * lt[1].mean()
        gz = gz * lt[1].mean()
    else:
        actor_loss = lt[2].mean()
    return actor_loss, lt[3].mean(), f["delta"], wm._backward(f, -gz / n, 2 * gv / n), ent


def shard_sums(blob, H, A, s, a, r, s2, gamma, loss="per_sample", weights=None, entropy_coef=0.0):
    """One regularised gradient row in float64, in learner_dp_mirror.shard_sums' form ({"g", "loss", "n", "td"}):
    learner_dp_mirror.combine adds such rows and scales them once."""
    f, iw, gz, gv, lt, ent = _terms(blob, H, A, s, a, r, s2, gamma, loss, weights, float(entropy_coef))
    return {"g": wm._backward(f, gz, gv), "loss": lt.sum(axis=1), "n": f["n"], "td": f["delta"], "entropy": ent}


def norms(grad, H, A):
    """The actor's and the critic's gradient norm."""
    na = mirror.layout(H, A)[1][4]
    return np.array([np.sqrt((grad[:na] ** 2).sum()), np.sqrt((grad[na:] ** 2).sum())])


def clip(grad, H, A, max_norms):
    """clip_grad_norm_ per network: (coef [2], norms [2], clipped flat gradient); max_norms = (actor, critic), inf = off."""
    na = mirror.layout(H, A)[1][4]
    nr = norms(grad, H, A)
    coef = np.array([1.0 if np.isinf(m) else min(1.0, m / (x + 1e-6)) for m, x in zip(max_norms, nr)])
    out = np.array(grad, np.float64, copy=True)
    out[:na] *= coef[0]
    out[na:] *= coef[1]
    return coef, nr, out
