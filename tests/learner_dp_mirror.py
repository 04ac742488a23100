"""float64 mirror of the split update (uavtrack_learner_grad / _apply): a shard's UNSCALED gradient and loss sums, the
ordered combine with its one global scale, and Adam through tests/learner_mirror.py.  Also the rule the split must NOT
be mistaken for -- the average of the shards' own reference-loss gradients -- and the batches and initial parameters the learner tests draw."""
import numpy as np

import learner_mirror as mirror


def shard_sums(blob, H, A, s, a, r, s2, gamma, loss="reference"):
    """One shard's row in float64: {"g": unscaled gradient sums [P], "loss": the four loss sums, "n", "td"}.  The
    actor's sums are those of w (onehot - p) with w = 1 (reference) or delta (per_sample), the critic's of V - target."""
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
    vn = (np.maximum(s2 @ w1c.T + b1c, 0) @ w2c.T)[:, 0] + b2c[0]
    target = r + gamma * vn
    delta = target - v
    nlp = -np.log(p[np.arange(n), a])
    onehot = np.zeros_like(p); onehot[np.arange(n), a] = 1
    w = np.ones(n) if loss == "reference" else delta
    gz = w[:, None] * (onehot - p)
    dha = (gz @ w2a) * (pa > 0)
    gv = v - target
    dhc = gv[:, None] * w2c * (pc > 0)
    g = np.concatenate([x.ravel() for x in (dha.T @ s, dha.sum(0), gz.T @ ha, gz.sum(0), dhc.T @ s, dhc.sum(0),
                                            (gv[:, None] * hc).sum(0), np.array([gv.sum()]))])
    return {"g": g, "loss": np.array([nlp.sum(), delta.sum(), (nlp * delta).sum(), (gv ** 2).sum()]), "n": n, "td": delta}


def combine(rows, H, A, loss="reference"):
    """(actor_loss, critic_loss, gradient [P]) of the ONE update the rows make: sums added in row order, N = sum n, the
    actor scaled by the GLOBAL -mean(delta) / N (reference) or -1 / N (per_sample), the critic by 2 / N."""
    g = np.zeros_like(rows[0]["g"])
    ls = np.zeros(4)
    N = 0
    for row in rows:
        g = g + row["g"]; ls = ls + row["loss"]; N += row["n"]
    mean_delta = ls[1] / N
    actor_loss = (ls[0] / N) * mean_delta if loss == "reference" else ls[2] / N
    na = sum(mirror.layout(H, A)[0][:4])
    scale = np.concatenate([np.full(na, -mean_delta / N if loss == "reference" else -1.0 / N), np.full(g.size - na, 2.0 / N)])
    return actor_loss, ls[3] / N, g * scale


def update_from_rows(state, rows, H, A, lrs, loss="reference"):
    """learner_mirror.update with the gradient taken from rows."""
    al, cl, g = combine(rows, H, A, loss)
    step = np.asarray(state["step"], np.int64) + 1
    p, m, v = mirror.adam(state["params"], state["exp_avg"], state["exp_avg_sq"], step, g, lrs, H, A)
    return {"params": p, "exp_avg": m, "exp_avg_sq": v, "step": step}, al, cl


def averaged_shard_gradients(blob, H, A, shards, gamma, loss="reference"):
    """The rule the split is NOT: every shard's own loss gradient (its own mean(delta) for the reference loss),
    averaged over the shards."""
    return np.mean([mirror.losses_and_grads(blob, H, A, s, a, r, s2, gamma, loss)[3] for s, a, r, s2 in shards], axis=0)


def cuts(n, K, seed=0):
    """K uneven contiguous pieces of range(n): K - 1 distinct interior boundaries, every piece non-empty."""
    if K == 1:
        return [(0, n)]
    b = np.sort(np.random.RandomState(seed + K).choice(np.arange(1, n), size=K - 1, replace=False))
    edges = [0] + [int(x) for x in b] + [n]
    return list(zip(edges[:-1], edges[1:]))


def split(batch, pieces):
    return [tuple(x[lo:hi] for x in batch) for lo, hi in pieces]


def init_blob(H, A, seed):
    """torch.nn.Linear's default initialisation of both networks as one fp32 blob."""
    import torch
    import uavtrack
    torch.manual_seed(seed)
    return np.concatenate([p.detach().numpy().ravel() for p in list(uavtrack.ActorMLP(12, H, A).parameters()) +
                           list(uavtrack.ValueMLP(12, H).parameters())]).astype(np.float32)


def batch(rng, n, A):
    """A batch of n transitions for the learner tests: (states, actions, rewards, next_states)."""
    s = rng.uniform(-1, 1, size=(n, 12)).astype(np.float32)
    s2 = rng.uniform(-1, 1, size=(n, 12)).astype(np.float32)
    s[:, 9:11] = rng.uniform(0, 5, size=(n, 2)); s2[:, 9:11] = rng.uniform(0, 5, size=(n, 2))
    a = rng.randint(0, A, size=n).astype(np.int32)
    r = rng.uniform(-2, 2, size=n).astype(np.float32)
    return s, a, r, s2


TEETH = dict(H=128, A=12, n=6007, gamma=0.95, lrs=(1e-3, 5e-3), seed=21)


def teeth_batch():
    """(blob, (s, a, r, s2)): a batch whose rewards ramp by 6 from the first row to the last, so that every contiguous
    shard has its own mean(delta) and a rule that scales a shard by its own mean shows.  n is not a multiple of the
    gradient kernel's tile."""
    c = TEETH
    s, a, r, s2 = batch(np.random.RandomState(c["seed"]), c["n"], c["A"])
    r = (r + np.linspace(-3.0, 3.0, c["n"])).astype(np.float32)
    return init_blob(c["H"], c["A"], c["seed"]), (s, a, r, s2)
