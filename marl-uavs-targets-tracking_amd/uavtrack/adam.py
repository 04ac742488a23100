"""The device trainers' flat torch.optim.Adam state and torch's own format for it.  The library keeps, per handle, one
float array of exp_avg, one of exp_avg_sq (the trainable tensors concatenated in parameters() order) and one step
count per tensor; checkpoints hold torch.optim.Adam state_dicts.  Both directions go through torch itself, so the
dicts are the ones torch writes and reads."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import host_ptr


def flat(tensors) -> np.ndarray:
    """The tensors' values concatenated in order: one contiguous float32 array."""
    return np.ascontiguousarray(np.concatenate([t.detach().cpu().float().numpy().ravel() for t in tensors]),
                                dtype=np.float32)


def split(a: np.ndarray, like) -> List[torch.Tensor]:
    """flat's inverse: consecutive spans of `a` as CPU tensors shaped like the tensors of `like`, each a copy."""
    out, o = [], 0
    for p in like:
        out.append(torch.from_numpy(a[o:o + p.numel()].copy()).view_as(p))
        o += p.numel()
    return out


def to_state_dict(params: Sequence[torch.Tensor], lr: float, exp_avg: np.ndarray, exp_avg_sq: np.ndarray,
                  step: np.ndarray) -> dict:
    """torch.optim.Adam(params, lr).state_dict() holding the flat moments and per-tensor steps.  A tensor whose step is
    0 has no state, as before torch's first step."""
    params = list(params)
    opt = torch.optim.Adam(params, lr=lr)
    for p, m, v, s in zip(params, split(exp_avg, params), split(exp_avg_sq, params), step):
        if s > 0:
            opt.state[p] = {"step": torch.tensor(float(s)), "exp_avg": m, "exp_avg_sq": v}
    return opt.state_dict()


def from_state_dict(params: Sequence[torch.Tensor], lr: float, sd: dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(exp_avg, exp_avg_sq, step) of a torch.optim.Adam state_dict over `params`, which torch validates by loading it.
    A tensor without state loads as zeros."""
    params = list(params)
    opt = torch.optim.Adam(params, lr=lr)
    opt.load_state_dict(sd)
    ms, vs, steps = [], [], np.zeros(len(params), np.int64)
    for i, p in enumerate(params):
        st = opt.state.get(p, {})
        if st:
            steps[i] = int(float(st["step"]))
            ms.append(st["exp_avg"].detach().float().cpu().reshape(p.shape))
            vs.append(st["exp_avg_sq"].detach().float().cpu().reshape(p.shape))
        else:
            ms.append(torch.zeros_like(p))
            vs.append(torch.zeros_like(p))
    return flat(ms), flat(vs), steps


def read(get, h, n_floats: int, tensors: int, stream) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(exp_avg [n_floats], exp_avg_sq [n_floats], step [tensors]) as numpy arrays, through `get`, a
    uavtrack_*_get_optimizer_state symbol of handle `h`."""
    m, v, steps = np.empty(n_floats, np.float32), np.empty(n_floats, np.float32), np.empty(tensors, np.int64)
    _lib.check(get(h, host_ptr(m), host_ptr(v), host_ptr(steps), n_floats, stream), get.__name__)
    return m, v, steps


def write(set_, h, exp_avg: np.ndarray, exp_avg_sq: np.ndarray, step: np.ndarray, stream) -> None:
    """read's inverse through `set_`, a uavtrack_*_set_optimizer_state symbol: contiguous float32 moments and int64
    steps."""
    _lib.check(set_(h, host_ptr(exp_avg), host_ptr(exp_avg_sq), host_ptr(step), exp_avg.size, stream), set_.__name__)
