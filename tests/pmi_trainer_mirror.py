"""A float64 numpy mirror of the reference's PMINetwork.train_pmi (PMINet.py:74-100) as the device trainer computes
it: the rows gathered through the (timestep, uav-pair) index triples, two train-mode forwards (each BatchNorm1d
normalises with its own batch's biased statistics and then updates its running statistics), CustomLoss, a
hand-written train-mode BatchNorm backward and torch.optim.Adam.  State is a dict keyed like the reference's
state_dict (30 keys); the Adam state is {"exp_avg": {name: array}, "exp_avg_sq": {...}, "step": {name: int}} over
the 18 trainable parameters in PMINetwork.parameters() order."""
import numpy as np

EPS, MOMENTUM = 1e-5, 0.1
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
BRANCHES = (("fc_comm", "bn_comm", 0, 5), ("fc_obs", "bn_obs", 5, 9), ("fc_boundary_state", "bn_boundary_state", 9, 12))


def param_names():
    """PMINetwork.parameters() order (PMINet.py:28-38)."""
    out = []
    for lin, bn, _, _ in BRANCHES + (("fc1", "bn1", 0, 0),):
        out += [lin + ".weight", lin + ".bias", bn + ".weight", bn + ".bias"]
    return out + ["fc2.weight", "fc2.bias"]


def state_names():
    """PMINetwork.state_dict() order: 30 keys."""
    out = []
    for lin, bn, _, _ in BRANCHES + (("fc1", "bn1", 0, 0),):
        out += [lin + ".weight", lin + ".bias", bn + ".weight", bn + ".bias", bn + ".running_mean", bn + ".running_var",
                bn + ".num_batches_tracked"]
    return out + ["fc2.weight", "fc2.bias"]


def _bn_forward(z, gamma, beta):
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    inv = 1.0 / np.sqrt(var + EPS)
    xh = (z - mu) * inv
    return xh, gamma * xh + beta, mu, var, inv


def _bn_backward(dy, xh, inv, gamma):
    """dL/dz of y = gamma * (z - mean) / sqrt(var + eps) + beta with batch statistics; also dgamma, dbeta."""
    n = dy.shape[0]
    dz = gamma * inv * (dy - dy.sum(0) / n - xh * (dy * xh).sum(0) / n)
    return dz, (dy * xh).sum(0), dy.sum(0)


def forward(sd, x):
    """One train-mode forward of a batch x [n, 12] -> (output [n], cache, batch statistics {bn: (mean, biased var)})."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    parts, cache, stats = [], {"x": x}, {}
    for lin, bn, a, b in BRANCHES:
        z = x[:, a:b] @ g(lin + ".weight").T + g(lin + ".bias")
        xh, y, mu, var, inv = _bn_forward(z, g(bn + ".weight"), g(bn + ".bias"))
        cache[bn] = (xh, y, inv)
        stats[bn] = (mu, var)
        parts.append(np.maximum(y, 0.0))
    a0 = np.concatenate(parts, axis=1)
    z1 = a0 @ g("fc1.weight").T + g("fc1.bias")
    xh1, y1, mu1, var1, inv1 = _bn_forward(z1, g("bn1.weight"), g("bn1.bias"))
    a1 = np.maximum(y1, 0.0)
    cache.update(a0=a0, a1=a1, bn1=(xh1, y1, inv1))
    stats["bn1"] = (mu1, var1)
    return a1 @ g("fc2.weight")[0] + g("fc2.bias")[0], cache, stats


def backward(sd, cache, d_out, grads):
    """Adds this forward's gradients (d_out = dL/doutput [n]) into grads {param name: array}."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    H = g("fc2.weight").shape[1]
    a0, a1 = cache["a0"], cache["a1"]
    grads["fc2.weight"] += (d_out @ a1)[None, :]
    grads["fc2.bias"] += d_out.sum(keepdims=True)
    xh1, y1, inv1 = cache["bn1"]
    dy1 = np.outer(d_out, g("fc2.weight")[0]) * (y1 > 0)
    dz1, dg1, db1 = _bn_backward(dy1, xh1, inv1, g("bn1.weight"))
    grads["bn1.weight"] += dg1
    grads["bn1.bias"] += db1
    grads["fc1.weight"] += dz1.T @ a0
    grads["fc1.bias"] += dz1.sum(0)
    da0 = dz1 @ g("fc1.weight")
    for j, (lin, bn, a, b) in enumerate(BRANCHES):
        xh, y, inv = cache[bn]
        dy = da0[:, j * H:(j + 1) * H] * (y > 0)
        dz, dgam, dbet = _bn_backward(dy, xh, inv, g(bn + ".weight"))
        grads[bn + ".weight"] += dgam
        grads[bn + ".bias"] += dbet
        grads[lin + ".weight"] += dz.T @ cache["x"][:, a:b]
        grads[lin + ".bias"] += dz.sum(0)


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def loss_and_grads(sd, x12, x13):
    """CustomLoss(forward(x12), forward(x13)) and its gradient of every parameter (zero_grad semantics)."""
    o12, c12, s12 = forward(sd, x12)
    o13, c13, s13 = forward(sd, x13)
    n = x12.shape[0]
    loss = float(np.mean(softplus(-o12) + softplus(o13)))
    grads = {k: np.zeros_like(np.asarray(sd[k], dtype=np.float64)) for k in param_names()}
    backward(sd, c12, -sigmoid(-o12) / n, grads)
    backward(sd, c13, sigmoid(o13) / n, grads)
    return loss, o12, o13, grads, (s12, s13)


def _update_running(sd, stats, n):
    for bn, (mu, var) in stats.items():
        sd[bn + ".running_mean"] = (1 - MOMENTUM) * np.asarray(sd[bn + ".running_mean"], np.float64) + MOMENTUM * mu
        sd[bn + ".running_var"] = ((1 - MOMENTUM) * np.asarray(sd[bn + ".running_var"], np.float64)
                                   + MOMENTUM * var * n / (n - 1))
        sd[bn + ".num_batches_tracked"] = int(sd[bn + ".num_batches_tracked"]) + 1


def new_adam():
    return {"exp_avg": {}, "exp_avg_sq": {}, "step": {}}


def adam_step(sd, adam, grads, lr):
    """torch.optim.Adam's single-tensor step (defaults betas (0.9, 0.999), eps 1e-8)."""
    for k in param_names():
        gr = grads[k]
        m = adam["exp_avg"].get(k, np.zeros_like(gr))
        v = adam["exp_avg_sq"].get(k, np.zeros_like(gr))
        t = adam["step"].get(k, 0) + 1
        m = m + (1 - BETA1) * (gr - m)
        v = v * BETA2 + (1 - BETA2) * gr * gr
        denom = np.sqrt(v) / np.sqrt(1 - BETA2 ** t) + ADAM_EPS
        sd[k] = np.asarray(sd[k], np.float64) - (lr / (1 - BETA1 ** t)) * m / denom
        adam["exp_avg"][k], adam["exp_avg_sq"][k], adam["step"][k] = m, v, t


def gather(rows, n_uav, t_idx, u_idx):
    """(input_1_2, input_1_3) of every selected row: rows[t * n_uav + u[0]], rows[t * n_uav + u[1]] (PMINet.py:83-91)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 12)
    return rows[t_idx * n_uav + u_idx[:, 0]], rows[t_idx * n_uav + u_idx[:, 1]]


def train_pmi(sd, adam, rows, n_uav, t_idx, u_idx, batch_size, lr=1e-3):
    """One train_pmi call on copies of (sd, adam).  -> (sd, adam, avg_loss, record) where record holds per batch:
    loss, o12, o13, grads."""
    sd = {k: (np.array(v, np.float64) if not k.endswith("num_batches_tracked") else int(v)) for k, v in sd.items()}
    adam = {k: dict(v) for k, v in adam.items()}
    x12, x13 = gather(rows, n_uav, np.asarray(t_idx), np.asarray(u_idx))
    nb = len(t_idx) // batch_size
    rec = {"loss": [], "o12": [], "o13": [], "grads": []}
    total = 0.0
    for b in range(nb):
        sl = slice(b * batch_size, (b + 1) * batch_size)
        loss, o12, o13, grads, (s12, s13) = loss_and_grads(sd, x12[sl], x13[sl])
        _update_running(sd, s12, batch_size)
        _update_running(sd, s13, batch_size)
        adam_step(sd, adam, grads, lr)
        total += abs(loss)
        for k, v in (("loss", loss), ("o12", o12), ("o13", o13), ("grads", grads)):
            rec[k].append(v)
    return sd, adam, total / nb, rec
