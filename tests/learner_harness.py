"""What the device learner's GPU tests share (tests/test_hip_learner*.py, test_hip_nstep.py, test_hip_lambda.py): the
learner and its cases (the host half of every case is drawn here, without a GPU), one update or gradient row through
Python or straight through an entry point, and the bounds against the float64 mirror.  Imports without a GPU: uavtrack
is imported inside functions, and nothing touches DEV until a function that needs it is called.

The bounds (a single update from zero moments against tests/learner_mirror.py): td_delta and the losses within 2e-5 of
their magnitude scale; the gradient (exp_avg / 0.1 after one step) within tol_g, 2e-6 (1 + log2 n) of its largest element;
the parameters within 1e-3 * lr, except where the fp64 gradient is within the gradient's rounding of 0 (then Adam's
first step, lr * g / (|g| + eps), may take either sign: within 2 lr).  tests/test_learner_harness_cpu.py pins them.
tol_g is a whole-blob bound (one max |g| over the actor and the critic together); the element-wise one, every element
against the sum of its own absolute terms, lives in tests/learner_gradient_cases.py and test_hip_learner_gradients.py."""
import types

import numpy as np
import torch

import learner_mirror as mirror

DEV = "cuda:0"
LR = (1e-3, 5e-3)
GAMMA = 0.95
STORES = ("states", "actions", "rewards", "next_states")

# test_hip_learner.py::test_sweep_against_fp64_mirror's grid of (H, A, n, loss, gather)
SWEEP = [(H, A, n, loss, gather)
         for k, (H, n) in enumerate([(1, 1), (33, 2), (64, 63), (128, 65), (200, 4096), (256, 65537),
                                     (33, 65537), (128, 4096), (256, 63), (1, 65), (200, 2), (64, 1)])
         for A in ([9, 12, 48][k % 3],)
         for loss, gather in ((("reference", True),) if k % 2 == 0 else (("per_sample", False),)) +
         ((("per_sample", True),) if k % 4 == 1 else ()) + ((("reference", False),) if k % 4 == 0 else ())]


# ---- construction ----------------------------------------------------------------------------------------------------

def learner(H, A, loss="reference", blob=None, max_batch=0, c=0.0, mgn=None, diag=False, gamma=GAMMA, lr=LR):
    """A DeviceActorCritic holding `blob`; c, mgn: entropy_coef and max_grad_norm (at 0.0 and None the constructor makes
    no regularisation call); diag: diagnostics installed."""
    import uavtrack
    L = uavtrack.DeviceActorCritic(12, H, A, lr[0], lr[1], gamma, DEV, loss=loss, max_batch=max_batch, entropy_coef=c,
                                   max_grad_norm=mgn)
    if blob is not None:
        L._set_params(np.ascontiguousarray(blob, np.float32))
    if diag:
        L.enable_diagnostics()
    return L


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def init_blob(H, A, seed):
    """torch.nn.Linear's default initialisation of both networks as one fp32 blob."""
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


def cuts(n, K, seed=0):
    """K uneven contiguous pieces of range(n): K - 1 distinct interior boundaries, every piece non-empty."""
    if K == 1:
        return [(0, n)]
    b = np.sort(np.random.RandomState(seed + K).choice(np.arange(1, n), size=K - 1, replace=False))
    edges = [0] + [int(x) for x in b] + [n]
    return list(zip(edges[:-1], edges[1:]))


def split(batch, pieces):
    return [tuple(x[lo:hi] for x in batch) for lo, hi in pieces]


TEETH = dict(H=128, A=12, n=6007, gamma=0.95, lrs=(1e-3, 5e-3), seed=21)


def teeth_batch():
    """(blob, (s, a, r, s2)): a batch whose rewards ramp by 6 from the first row to the last, so that every contiguous
    shard has its own mean(delta) and a rule that scales a shard by its own mean shows.  n is not a multiple of the
    gradient kernel's tile."""
    c = TEETH
    s, a, r, s2 = batch(np.random.RandomState(c["seed"]), c["n"], c["A"])
    r = (r + np.linspace(-3.0, 3.0, c["n"])).astype(np.float32)
    return init_blob(c["H"], c["A"], c["seed"]), (s, a, r, s2)


_cases = {}


def host_case(H, A, n, gather):
    """(blob, host batch over the store, capacity, host indices), built once."""
    key = (H, A, n, gather)
    if key not in _cases:
        rng = np.random.RandomState(H * 1000 + n + (7 if gather else 0))
        cap = n + 7 if gather else n
        b = batch(rng, cap, A)
        idx = rng.randint(0, cap, size=n).astype(np.int64) if gather else np.arange(n)
        _cases[key] = (init_blob(H, A, H + n), b, cap, idx)
    return _cases[key]


_device = {}


def case(H, A, n, gather):
    """host_case and its device copies: (blob, host batch, device store, capacity, host indices, device indices or
    None), built once."""
    key = (H, A, n, gather)
    blob, b, cap, idx = host_case(*key)
    if key not in _device:
        _device[key] = ({k: dev(x) for k, x in zip(STORES, b)}, dev(idx) if gather else None)
    store, it = _device[key]
    return blob, b, store, cap, idx, it


def gathered(b, idx):
    return tuple(x[idx] for x in b)


# ---- observation -----------------------------------------------------------------------------------------------------

def state(L):
    m, v, st = L._optim_state()
    return {"params": L._get_params(), "exp_avg": m, "exp_avg_sq": v, "step": st}


def same(a, b, what=""):
    """Two dicts of arrays (or None) hold the same keys and the same bits, NaN equal to NaN."""
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


# ---- calls -----------------------------------------------------------------------------------------------------------

def _direct(L, kind, entry, n, store, cap, it, w, d, outs):
    """uavtrack_learner_{kind}_{entry} itself through ctypes, whatever of w and d is NULL."""
    from uavtrack import _lib
    assert entry in ("weighted", "discounted") and (entry == "discounted" or d is None)
    name = f"uavtrack_learner_{kind}_{entry}"
    extra = (_lib.ptr(w), _lib.ptr(d)) if entry == "discounted" else (_lib.ptr(w),)
    _lib.check(getattr(L._lib, name)(L._h, n, *L._batch_args(store, cap, it), *extra, *(_lib.ptr(t) for t in outs),
                                     L._stream()), name)


def _result(L, n, al, cl, td, prio):
    out = dict(state(L), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy(), td=td.cpu().numpy(),
               prio=None if prio is None else prio.cpu().numpy())
    if L._entropy is not None:
        out["entropy"] = L.entropy(n).cpu().numpy()
        out["grad_norm"] = L.grad_norm.cpu().numpy()
    return out


def update(L, n, store, cap, it, prio, w=None, d=None, entry=None):
    """One closed update and the learner's state after it.  entry None: through L._run, so Python picks the entry point;
    "weighted" / "discounted": that entry point called directly."""
    if entry is None:
        al, cl, td = L._run(n, store, cap, it, prio, w, d)
    else:
        losses, td = torch.empty(2, device=DEV), torch.empty(n, device=DEV)
        al, cl = losses[0], losses[1]
        _direct(L, "update", entry, n, store, cap, it, w, d, (losses[0:1], losses[1:2], td, prio))
    return _result(L, n, al, cl, td, prio)


def row(L, n, store, cap, it, w=None, d=None, entry=None):
    """One gradient row and its td_delta as numpy arrays; entry as for update."""
    if entry is None:
        r, td = L._grad(n, store, cap, it, None, None, w, d)
    else:
        r, td = torch.empty(L.row_floats, device=DEV), torch.empty(n, device=DEV)
        _direct(L, "grad", entry, n, store, cap, it, w, d, (td, r))
    return r.cpu().numpy(), td.cpu().numpy()


def split_update(L, n, store, cap, it, prio, w=None):
    """The same update as grad -> apply -> write_priorities."""
    r, td = L._grad(n, store, cap, it, None, None, w)
    al, cl = L.apply(r)
    if prio is not None:
        L.write_priorities(types.SimpleNamespace(priorities=prio, capacity=cap), it, td)
    return _result(L, n, al, cl, td, prio)


# ---- bounds ----------------------------------------------------------------------------------------------------------

def tol_g(n, g):
    """The gradient bound of a batch of n rows whose fp64 gradient is g."""
    return 2e-6 * (1 + np.log2(n)) * np.abs(g).max()


def _share(err, bound):
    return float(np.max(err / np.maximum(bound, 1e-300)))


def assert_losses_and_td(al, cl, td, ral, rcl, rtd, c=0.0, A=1):
    """td_delta and the losses at 2e-5 of their scale; the actor-loss scale gains c log A, the size of the entropy
    term."""
    td_tol = 2e-5 * (np.abs(rtd).max() + 1e-6)
    cl_tol = 2e-5 * (np.mean(rtd ** 2) + 1e-12) + 1e-12
    al_tol = 2e-5 * (abs(ral) + np.mean(np.abs(rtd)) * 30 + c * np.log(A))
    print(f"share of the bound: td {_share(np.abs(td - rtd), td_tol):.3f}, critic loss "
          f"{_share(abs(float(cl) - rcl), cl_tol):.3f}, actor loss {_share(abs(float(al) - ral), al_tol):.3f}")
    np.testing.assert_allclose(td, rtd, rtol=0, atol=td_tol)
    assert abs(float(cl) - rcl) <= cl_tol, (float(cl), rcl)
    assert abs(float(al) - ral) <= al_tol, (float(al), ral)


def assert_step_from_zero(st, blob, g, n, H, A, coef=(1.0, 1.0), lr=LR):
    """The first Adam step from zero moments, g the fp64 gradient before clipping and coef the two networks' clip
    coefficients: exp_avg / 0.1 within tol_g (times the coefficient) of coef g, the parameters within 1e-3 lr except
    where the gradient is within its rounding of 0 (then within 2 lr)."""
    na = mirror.layout(H, A)[1][4]
    cf = np.concatenate([np.full(na, coef[0]), np.full(g.size - na, coef[1])])
    tol = tol_g(n, g) * cf
    err = np.abs(st["exp_avg"] / 0.1 - g * cf)
    p64 = mirror.adam(blob.astype(np.float64), np.zeros(g.size), np.zeros(g.size), np.ones(8, np.int64), g * cf, lr, H, A)[0]
    lr_of = np.concatenate([np.full(k, lr[0] if t < 4 else lr[1]) for t, k in enumerate(mirror.layout(H, A)[0])])
    near0 = np.abs(g * cf) <= 4 * tol + 1e-8
    perr = np.abs(st["params"] - p64)
    far_tol, near_tol = 1e-3 * lr_of + 1e-6 * np.abs(p64), 2 * lr_of + 1e-6
    print(f"share of the bound: gradient {_share(err, tol):.3f}, parameters "
          f"{_share(perr[~near0], far_tol[~near0]) if (~near0).any() else 0:.3f} away from g = 0, "
          f"{_share(perr[near0], near_tol[near0]) if near0.any() else 0:.3f} near it")
    assert (err <= tol + 1e-30).all(), _share(err, tol)
    assert (perr[~near0] <= far_tol[~near0]).all(), perr[~near0].max()
    assert (perr[near0] <= near_tol[near0]).all()
