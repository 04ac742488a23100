"""float64 numpy mirror of ActorCritic.update (actor_critic.py:150-179) + torch.optim.Adam, the yardstick of the
device learner's tests.  Parameters travel as one flat blob in torch order (actor fc1.weight [H][12], fc1.bias,
fc2.weight [A][H], fc2.bias, then the critic's four tensors)."""
import numpy as np


def layout(H, A):
    sizes = [12 * H, H, A * H, A, 12 * H, H, H, 1]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return sizes, offs


def unpack(blob, H, A):
    sizes, o = layout(H, A)
    t = [np.asarray(blob[o[i]:o[i + 1]], np.float64) for i in range(8)]
    return t[0].reshape(H, 12), t[1], t[2].reshape(A, H), t[3], t[4].reshape(H, 12), t[5], t[6].reshape(1, H), t[7]


def losses_and_grads(blob, H, A, s, a, r, s2, gamma, loss="reference"):
    """(actor_loss, critic_loss, td_delta, flat gradient) of one update in float64."""
    w1a, b1a, w2a, b2a, w1c, b1c, w2c, b2c = unpack(blob, H, A)
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
    if loss == "reference":
        actor_loss = nlp.mean() * delta.mean()
        w = np.full(n, delta.mean())
    else:
        actor_loss = (nlp * delta).mean()
        w = delta
    critic_loss = ((v - target) ** 2).mean()
    onehot = np.zeros_like(p); onehot[np.arange(n), a] = 1
    gz = -(w[:, None] * (onehot - p)) / n                        # dL/dz
    g_w2a = gz.T @ ha; g_b2a = gz.sum(0)
    dha = (gz @ w2a) * (pa > 0)
    g_w1a = dha.T @ s; g_b1a = dha.sum(0)
    gv = 2 * (v - target) / n
    g_w2c = (gv[:, None] * hc).sum(0)[None, :]; g_b2c = np.array([gv.sum()])
    dhc = gv[:, None] * w2c * (pc > 0)
    g_w1c = dhc.T @ s; g_b1c = dhc.sum(0)
    grad = np.concatenate([g.ravel() for g in (g_w1a, g_b1a, g_w2a, g_b2a, g_w1c, g_b1c, g_w2c, g_b2c)])
    return actor_loss, critic_loss, delta, grad


def adam(blob, m, v, step, grad, lrs, H, A):
    """torch.optim.Adam defaults; step [8] per tensor (already advanced); lrs = (actor_lr, critic_lr)."""
    sizes, o = layout(H, A)
    blob, m, v = blob.astype(np.float64).copy(), m.astype(np.float64).copy(), v.astype(np.float64).copy()
    for t in range(8):
        sl = slice(o[t], o[t + 1])
        lr = lrs[0] if t < 4 else lrs[1]
        m[sl] = 0.9 * m[sl] + 0.1 * grad[sl]
        v[sl] = 0.999 * v[sl] + 0.001 * grad[sl] ** 2
        bc1, bc2 = 1 - 0.9 ** step[t], 1 - 0.999 ** step[t]
        blob[sl] -= lr / bc1 * m[sl] / (np.sqrt(v[sl]) / np.sqrt(bc2) + 1e-8)
    return blob, m, v


def update(state, H, A, s, a, r, s2, gamma, lrs, loss="reference"):
    """state = dict(params, exp_avg, exp_avg_sq, step [8]) -> (new state, actor_loss, critic_loss, td_delta)."""
    al, cl, td, g = losses_and_grads(state["params"], H, A, s, a, r, s2, gamma, loss)
    step = np.asarray(state["step"], np.int64) + 1
    p, m, v = adam(state["params"], state["exp_avg"], state["exp_avg_sq"], step, g, lrs, H, A)
    return {"params": p, "exp_avg": m, "exp_avg_sq": v, "step": step}, al, cl, td


def last_wins(prio, idx, values):
    """PrioritizedReplayBuffer.update_priorities (train.py:136-138): a sequential loop, the last write wins."""
    out = np.array(prio, copy=True)
    for i, x in zip(idx, values):
        out[i] = x
    return out
