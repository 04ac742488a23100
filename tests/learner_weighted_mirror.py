"""float64 numpy mirror of the importance-weighted update (uavtrack_learner_update_weighted / _grad_weighted), beside
tests/learner_mirror.py, which stays the unweighted yardstick.  One weight w_i >= 0 per batch row, in batch order:
    critic_loss               = mean_i(w_i (V(s_i) - y_i)^2)
    actor_loss, "per_sample"  = mean_i(-w_i log p_i delta_i)
    actor_loss, "reference"   = mean_i(-w_i log p_i) * mean_j(w_j delta_j)
Means divide by n; td_delta stays the unweighted delta.  Every expression keeps learner_mirror's order of operations
with w as one more exact factor, so w = 1 reproduces learner_mirror.losses_and_grads to the last bit."""
import numpy as np

import learner_mirror as mirror


def _forward(blob, H, A, s, a, r, s2, gamma):
    w1a, b1a, w2a, b2a, w1c, b1c, w2c, b2c = mirror.unpack(blob, H, A)
    s, s2, r = np.asarray(s, np.float64), np.asarray(s2, np.float64), np.asarray(r, np.float64)
    a = np.asarray(a, np.int64)
    n = len(a)
    pa = s @ w1a.T + b1a; ha = np.maximum(pa, 0)
    z = ha @ w2a.T + b2a
    z = z - z.max(axis=1, keepdims=True)
    p = np.exp(z); p /= p.sum(axis=1, keepdims=True)
    pc = s @ w1c.T + b1c; hc = np.maximum(pc, 0)
    v = (hc @ w2c.T)[:, 0] + b2c[0]
    hn = np.maximum(s2 @ w1c.T + b1c, 0)
    vn = (hn @ w2c.T)[:, 0] + b2c[0]
    target = r + gamma * vn
    delta = target - v
    nlp = -np.log(p[np.arange(n), a])
    onehot = np.zeros_like(p); onehot[np.arange(n), a] = 1
    return dict(s=s, n=n, pa=pa, ha=ha, p=p, pc=pc, hc=hc, v=v, target=target, delta=delta, nlp=nlp, onehot=onehot,
                w2a=w2a, w2c=w2c)


def _backward(f, gz, gv):
    """The flat gradient from dL/dz [n][A] and dL/dV [n]."""
    s, ha, hc, pa, pc, w2a, w2c = f["s"], f["ha"], f["hc"], f["pa"], f["pc"], f["w2a"], f["w2c"]
    g_w2a = gz.T @ ha; g_b2a = gz.sum(0)
    dha = (gz @ w2a) * (pa > 0)
    g_w1a = dha.T @ s; g_b1a = dha.sum(0)
    g_w2c = (gv[:, None] * hc).sum(0)[None, :]; g_b2c = np.array([gv.sum()])
    dhc = gv[:, None] * w2c * (pc > 0)
    g_w1c = dhc.T @ s; g_b1c = dhc.sum(0)
    return np.concatenate([g.ravel() for g in (g_w1a, g_b1a, g_w2a, g_b2a, g_w1c, g_b1c, g_w2c, g_b2c)])


def losses_and_grads(blob, H, A, s, a, r, s2, gamma, loss="reference", weights=None):
    """(actor_loss, critic_loss, td_delta, flat gradient) of one weighted update in float64; weights None = ones."""
    f = _forward(blob, H, A, s, a, r, s2, gamma)
    n, delta, nlp, v, target = f["n"], f["delta"], f["nlp"], f["v"], f["target"]
    iw = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    assert iw.shape == (n,)
    if loss == "reference":
        actor_loss = (nlp * iw).mean() * (delta * iw).mean()
        w = np.full(n, (delta * iw).mean()) * iw
    else:
        actor_loss = ((nlp * delta) * iw).mean()
        w = delta * iw
    critic_loss = (((v - target) ** 2) * iw).mean()
    gz = -(w[:, None] * (f["onehot"] - f["p"])) / n                        # dL/dz
    gv = 2 * ((v - target) * iw) / n
    return actor_loss, critic_loss, delta, _backward(f, gz, gv)


def shard_sums(blob, H, A, s, a, r, s2, gamma, loss="reference", weights=None):
    """One weighted gradient row in float64, in learner_dp_mirror.shard_sums' form ({"g", "loss", "n", "td"}): every term
    of the unscaled sums carries its row's w_i, n stays the row count; learner_dp_mirror.combine takes such rows."""
    f = _forward(blob, H, A, s, a, r, s2, gamma)
    n, delta, nlp, v, target = f["n"], f["delta"], f["nlp"], f["v"], f["target"]
    iw = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    w = iw if loss == "reference" else delta * iw
    gz = w[:, None] * (f["onehot"] - f["p"])
    gv = (v - target) * iw
    return {"g": _backward(f, gz, gv),
            "loss": np.array([(nlp * iw).sum(), (delta * iw).sum(), (nlp * delta * iw).sum(), ((v - target) ** 2 * iw).sum()]),
            "n": n, "td": delta}


def make_weights(rng, n):
    """Weights in [0, 1] with some exact zeros and the maximum exactly 1 (what a prioritised draw's weights / max look
    like, plus the zeros): n = 1 is [1], n = 2 is a zero and a one."""
    w = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    if n >= 2:
        zeros = rng.choice(n, size=max(1, n // 10), replace=False)
        w[zeros] = 0.0
        free = np.setdiff1d(np.arange(n), zeros)
        w[free[rng.randint(free.size)]] = 1.0
    else:
        w[:] = 1.0
    return w

