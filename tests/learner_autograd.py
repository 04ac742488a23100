"""torch float64 autograd on the learner's losses as include/uavtrack.h states them: the oracle tests/learner_mirror.py is
held to without a GPU, with the mirror's options; and the small helpers of the tests that compare the two."""
import types

import numpy as np
import torch

import learner_mirror as mirror


def update(blob, H, A, s, a, r, s2, gamma, loss="per_sample", weights=None, entropy_coef=0.0, max_norms=None, clip=None):
    """One update by autograd and torch.nn.utils.clip_grad_norm_: the record actor_loss, critic_loss, td, grad (before
    the norm clip), entropy [n], coef [2], clipped (the gradient after it).  clip = (log_mu, eps) is the clipped
    surrogate -min(r A, clamp(r, lo, hi) A) at the float32 bounds the library folds; max_norms = (actor, critic)."""
    t = [torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in mirror.unpack(blob, H, A)]
    w1a, b1a, w2a, b2a, w1c, b1c, w2c, b2c = t
    S, S2, R = (torch.from_numpy(np.asarray(x, np.float64)) for x in (s, s2, r))
    n = len(a)
    W = torch.ones(n, dtype=torch.float64) if weights is None else torch.from_numpy(np.asarray(weights, np.float64))
    critic = lambda x: (torch.relu(x @ w1c.T + b1c) @ w2c.T)[:, 0] + b2c[0]                            # noqa: E731
    logp = torch.log_softmax(torch.relu(S @ w1a.T + b1a) @ w2a.T + b2a, dim=1)
    ent = -(logp.exp() * logp).sum(dim=1)
    target = (R + gamma * critic(S2)).detach()
    v = critic(S)
    delta = (target - v).detach()
    lpa = logp.gather(1, torch.from_numpy(np.asarray(a, np.int64)).view(-1, 1))[:, 0]
    if loss == "reference":
        assert entropy_coef == 0 and clip is None
        al = (W * -lpa).mean() * (W * delta).mean()                        # the product of the two weighted means
    elif clip is None:
        al = torch.mean(W * (-lpa * delta - entropy_coef * ent))
    else:
        ratio = torch.exp(lpa - torch.from_numpy(np.asarray(clip[0], np.float64)))
        lo, hi = mirror.bounds(clip[1])
        al = torch.mean(W * (-torch.min(ratio * delta, ratio.clamp(lo, hi) * delta) - entropy_coef * ent))
    cl = torch.mean(W * (v - target) ** 2)
    al.backward(); cl.backward()
    g = np.concatenate([x.grad.numpy().ravel() for x in t])
    coefs = []
    for params, mx in zip((t[:4], t[4:]), (np.inf, np.inf) if max_norms is None else max_norms):
        if np.isinf(mx):
            coefs.append(1.0)
            continue
        total = torch.nn.utils.clip_grad_norm_(params, mx)
        coefs.append(min(1.0, mx / (float(total) + 1e-6)))
    return types.SimpleNamespace(actor_loss=float(al.detach()), critic_loss=float(cl.detach()), td=delta.numpy(), grad=g,
                                 entropy=ent.detach().numpy(), coef=np.array(coefs),
                                 clipped=np.concatenate([x.grad.numpy().ravel() for x in t]))


def rel(x, y):
    return np.abs(np.asarray(x) - np.asarray(y)).max() / (np.abs(np.asarray(y)).max() + 1e-300)


def close(x, y, what, bound=1e-12):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert np.isfinite(x).all() and np.isfinite(y).all(), what
    err, scale = np.abs(x - y).max(), max(np.abs(y).max(), 1e-300)
    assert err <= bound * scale, (what, err, scale)


def blob(H, A, seed):
    """Both networks drawn uniformly at a Linear layer's scale, without the package."""
    rng = np.random.RandomState(seed)
    sizes = mirror.layout(H, A)[0]
    return np.concatenate([rng.uniform(-1, 1, k) / np.sqrt(12 if t in (0, 1, 4, 5) else H)
                           for t, k in enumerate(sizes)]).astype(np.float32)


def batch(rng, n, A):
    s = rng.uniform(-1, 1, size=(n, 12)).astype(np.float32)
    s2 = rng.uniform(-1, 1, size=(n, 12)).astype(np.float32)
    a = rng.randint(0, A, size=n).astype(np.int32)
    r = rng.uniform(-2, 2, size=n).astype(np.float32)
    return s, a, r, s2


def wide(blob, H, A, span=300.0):
    """The same networks with the actor's fc2.bias a ramp of `span`: every row's logits span more than 250."""
    out = blob.copy()
    o = mirror.layout(H, A)[1]
    out[o[3]:o[4]] = np.linspace(0.0, span, A).astype(np.float32)
    return out
