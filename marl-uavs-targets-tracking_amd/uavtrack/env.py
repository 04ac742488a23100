"""BatchedUavEnv: the batched reset()/step(actions) -> (obs, reward, done) surface over
libuavtrack.so.  Tensors are torch-ROCm device tensors owned by Python; the kernels
write them in place on torch's current stream (no host sync, no copies)."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .config import EnvConfig, RewardMode
from .pmi import fold_pmi_state_dict
from ._handle import Handle
from ._lib import ptr as _ptr
from .pmi_trainer import DevicePMINetwork

_STATE_KEYS = ("ux", "uy", "uz", "uh", "ua", "tx", "ty", "tz", "th")

# every output of a rollout call: result key -> (shape of a T-step launch on B x N UAVs and M targets, dtype)
_OUTPUTS = {
    "actions": (lambda T, B, N, M: (T, B, N), torch.int32),
    "obs": (lambda T, B, N, M: (T, B, N, _lib.OBS_DIM), torch.float32),
    "reward": (lambda T, B, N, M: (T, B, N), torch.float32),
    "terms": (lambda T, B, N, M: (T, 3, B, N), torch.float32),
    "covered": (lambda T, B, N, M: (T, B), torch.int32),
    "done": (lambda T, B, N, M: (T, B), torch.uint8),
    "ep_sums": (lambda T, B, N, M: (B, 5), torch.float32),
    "targets": (lambda T, B, N, M: (T, B, M, 2), torch.float32),
    "raw": (lambda T, B, N, M: (T, B, N), torch.float32),
    "start_obs": (lambda T, B, N, M: (T, B, N, _lib.OBS_DIM), torch.float32),
}
# the outputs a handle has installed rather than passed per call: result key -> (attribute that keeps the installed
# tensor alive, the ABI setter, what error messages call the buffer)
_INSTALLED = {
    "targets": ("_trace", "uavtrack_set_target_trace", "target trace"),
    "raw": ("_raw", "uavtrack_set_raw_reward_output", "raw-reward buffer"),
    "start_obs": ("_start_obs", "uavtrack_set_start_obs_output", "start-observation buffer"),
}


class BatchedUavEnv(Handle):
    """B independent copies of the reference `Environment` (src/environment.py:12) on one GPU.

    reset(seed)            -> obs [B, N, 12]                           (environment.py:87-118)
    step(actions [B, N])   -> (obs [B, N, 12], reward [B, N], done [B]) (environment.py:120-164)
                              self.info = {"terms": [3, B, N], "covered": [B]}
    step_many(actions [T, B, N]) -> dict with a leading T axis, one launch
    """

    def __init__(self, cfg: EnvConfig, device: str = "cuda:0"):
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("uavtrack runs on an MI355X only (device must be cuda:N); there is no CPU path")
        idx = self.device.index if self.device.index is not None else 0
        self._device_index = idx
        self._create(cfg.c_struct(idx))
        self.info: Dict[str, torch.Tensor] = {}
        self._episode = 0
        self._trace: Optional[torch.Tensor] = None    # the installed target-trace buffer (kept alive: the library holds its raw pointer)
        self._raw: Optional[torch.Tensor] = None      # ... and the raw-reward buffer (set_raw_output)
        self._start_obs: Optional[torch.Tensor] = None   # ... and the fresh-state observations of automatic resets (set_start_obs_output)
        self._host_step = _lib.HostStep()             # step_host: the library's host result block and numpy views of it
        self._host_views: Optional[Dict[str, np.ndarray]] = None

    # -- plumbing ---------------------------------------------------------------------
    @property
    def B(self) -> int: return self.cfg.n_envs
    @property
    def N(self) -> int: return self.cfg.n_uav
    @property
    def M(self) -> int: return self.cfg.m_targets

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _fits(self, t, shape, dtype) -> bool:
        """True if `t` can be handed to a kernel that writes a contiguous `shape` / `dtype` array on this device."""
        return (t is not None and tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.device == self.device
                and t.is_contiguous())

    def _shape(self, key, T):
        shape, dtype = _OUTPUTS[key]
        return shape(T, self.B, self.N, self.M), dtype

    def _reuse(self, o, key, T, want=True):
        """Output buffer `key` of a previous result `o` if it has exactly the shape this launch writes, else a
        fresh one (a kernel writing T2 rows into a T1-row buffer would corrupt device memory)."""
        if not want:
            return None
        t = o.get(key) if o else None
        return t if self._fits(t, *self._shape(key, T)) else self._empty(*self._shape(key, T))

    def _check_out(self, out, keys, T):
        """The caller's buffers of a bound call: each one present fits what the launch writes, and reward is there."""
        for k in keys:
            if out.get(k) is not None and not self._fits(out[k], *self._shape(k, T)):
                shape, dtype = self._shape(k, T)
                raise ValueError(f"out[{k!r}] must be a contiguous {dtype} {shape} tensor on {self.device}")
        if out.get("reward") is None:
            raise ValueError("out['reward'] is required")

    def _rollout_call(self, entry, T, t, seed=0, mode=0, auto_reset_seed=None):
        """(ctypes function, its argument tuple, its name in error messages) of uavtrack_<entry>[_autoreset] on the stream
        current now.  entry: "step_many", "run_greedy" or "run_actor"; t: the tensors by result key ("actions" is the
        input of step_many and an output of the other two; "obs_in" for the actor), None or missing for a null pointer."""
        name = f"uavtrack_{entry}" + ("_autoreset" if auto_reset_seed is not None else "")
        u64 = lambda v: C.c_uint64(v & (2 ** 64 - 1))
        args = (self._h, C.c_int32(T)) + ((u64(seed),) if entry != "step_many" else ())
        if auto_reset_seed is not None:
            args += (u64(auto_reset_seed),)
        if entry == "run_actor":
            args += (C.c_int32(mode), _ptr(t["obs_in"]))
        args += tuple(_ptr(t.get(k)) for k in ("actions", "obs", "reward", "terms", "covered", "done", "ep_sums"))
        return getattr(self._lib, name), args + (self._stream(),), name

    def _out_arg(self, t, shape, dtype, name):
        if t is None:
            return self._empty(shape, dtype)
        if not self._fits(t, shape, dtype):
            raise ValueError(f"{name} must be a contiguous {dtype} {tuple(shape)} tensor on {self.device}")
        return t

    def _actions(self, actions, shape) -> torch.Tensor:
        a = torch.as_tensor(actions)
        if a.device != self.device or a.dtype != torch.int32:
            a = a.to(device=self.device, dtype=torch.int32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"actions shape {tuple(a.shape)} != {tuple(shape)}")
        return a.contiguous()


    def kernel_info(self) -> Dict[str, int]:
        out = (C.c_int64 * 5)()
        _lib.check(self._lib.uavtrack_kernel_info(self._h, out), "uavtrack_kernel_info")
        return dict(workgroup=out[0], envs_per_workgroup=out[1], workgroups=out[2], lds_bytes=out[3],
                    specialised=out[4])

    # -- reference surface ------------------------------------------------------------
    def reset(self, seed: int = 0, episode: Optional[int] = None) -> torch.Tensor:
        if episode is None:
            episode = self._episode
        self._episode = episode + 1
        obs = self._empty((self.B, self.N, _lib.OBS_DIM), torch.float32)
        _lib.check(self._lib.uavtrack_reset(self._h, C.c_uint64(seed & (2 ** 64 - 1)), C.c_uint32(episode),
                                            _ptr(obs), self._stream()), "uavtrack_reset")
        return obs

    def step(self, actions, want_terms: bool = True, ep_sums: Optional[torch.Tensor] = None,
             out_obs: Optional[torch.Tensor] = None, out_reward: Optional[torch.Tensor] = None):
        """`ep_sums` [B, 5] (float32, this device): running episode accumulators the kernel adds
        this step's contribution to (train.py:181-192).  `out_obs` / `out_reward`: caller-owned
        buffers the kernel writes instead of fresh tensors (static graph I/O)."""
        a = self._actions(actions, (self.B, self.N))
        obs = self._out_arg(out_obs, (self.B, self.N, _lib.OBS_DIM), torch.float32, "out_obs")
        reward = self._out_arg(out_reward, (self.B, self.N), torch.float32, "out_reward")
        terms = self._empty((3, self.B, self.N), torch.float32) if want_terms else None
        covered = self._empty((self.B,), torch.int32)
        done = self._empty((self.B,), torch.uint8)
        if ep_sums is not None:
            if ep_sums.shape != (self.B, 5) or ep_sums.dtype != torch.float32 or not ep_sums.is_contiguous():
                raise ValueError("ep_sums must be a contiguous float32 [B, 5] tensor")
            _lib.check(self._lib.uavtrack_step_accumulate(self._h, _ptr(a), _ptr(obs), _ptr(reward), _ptr(terms),
                                                          _ptr(covered), _ptr(done), _ptr(ep_sums), self._stream()),
                       "uavtrack_step_accumulate")
        else:
            _lib.check(self._lib.uavtrack_step(self._h, _ptr(a), _ptr(obs), _ptr(reward), _ptr(terms),
                                               _ptr(covered), _ptr(done), self._stream()), "uavtrack_step")
        self.info = {"terms": terms, "covered": covered}
        if self._raw is not None:
            self.info["raw"] = self._raw[0]       # uav.raw_reward of this step (set_raw_output)
        return obs, reward, done.bool()

    def _set_output(self, kind: str, buf: Optional[torch.Tensor]) -> None:
        attr, setter, what = _INSTALLED[kind]
        steps = 0
        if buf is not None:
            steps = buf.shape[0] if buf.dim() else 0
            shape, dtype = self._shape(kind, steps)
            if not self._fits(buf, shape, dtype):
                raise ValueError(f"{what} must be a contiguous float32 [T, {', '.join(map(str, shape[1:]))}] tensor on {self.device}")
        _lib.check(getattr(self._lib, setter)(self._h, _ptr(buf), C.c_int32(steps)), setter)
        setattr(self, attr, buf)      # every later launch writes through the raw pointer: the tensor must outlive them

    def set_target_trace(self, buf: Optional[torch.Tensor]) -> None:
        """Target positions after each step, [T, B, M, 2] (environment.py:150-153), written by every later stepping
        call until replaced; None switches the output off."""
        self._set_output("targets", buf)

    def set_raw_output(self, buf: Optional[torch.Tensor]) -> None:
        """uav.raw_reward of every UAV after each step, [T, B, N] (environment.py:219: the weighted sum of the three
        normalised terms before any cooperative sharing), written by every later stepping call until replaced; None
        switches the output off."""
        self._set_output("raw", buf)

    def set_start_obs_output(self, buf: Optional[torch.Tensor]) -> None:
        """Observation of the fresh state behind every in-launch reset, [T, B, N, 12]: row (t, b) is written where
        done[t, b] fired in an automatic-reset launch (what the policy sees at step t + 1) and left untouched elsewhere;
        launches without the automatic reset never write it.  None switches the output off."""
        self._set_output("start_obs", buf)

    def _attached(self, kind: str, T: int, want: bool, o, launch) -> Dict[str, torch.Tensor]:
        """Run `launch()` with a T-step buffer of `kind` installed when asked (reused from `o` if it fits); a buffer the
        caller installed earlier comes back afterwards.  Returns the buffers attached to the launch by result key:
        launch's own (a nested _attached) and this one."""
        if not want:
            return launch() or {}
        buf = self._reuse(o, kind, T)
        installed = getattr(self, _INSTALLED[kind][0])
        self._set_output(kind, buf)
        try:
            return {**(launch() or {}), kind: buf}
        finally:
            self._set_output(kind, installed)

    def _count_episodes(self, T: int, auto_reset_seed) -> None:
        if auto_reset_seed is not None and self.cfg.horizon > 0:
            self._episode += T // self.cfg.horizon + 1      # stay ahead of the episode numbers the device has used

    def step_host(self, actions: np.ndarray, stream=None) -> Dict[str, np.ndarray]:
        """Environment.step for a host caller (uavtrack_step_host): `actions` is a C-contiguous int32 numpy array [B, N];
        returns numpy VIEWS of the library's page-locked result block -- obs [B, N, 12], reward [B, N], terms [3, B, N],
        raw [B, N], covered [B], done [B] and the state behind the step (ux uy uh ua tx ty th [uz tz] step_count) -- valid
        until the next step_host on this environment.  Synchronises the stream.  `stream`: a ctypes stream handle the caller
        looked up once (a per-step `torch.cuda.current_stream()` lookup is a visible share of a 30 us step); default: torch's
        current stream."""
        if actions.dtype != np.int32 or not actions.flags.c_contiguous or actions.size != self.B * self.N:
            raise ValueError(f"actions must be a C-contiguous int32 array of {self.B} x {self.N} entries")
        hs = self._host_step
        if self._lib.uavtrack_step_host(self._h, C.c_void_p(actions.ctypes.data), C.byref(hs),
                                        self._stream() if stream is None else stream) != 0:
            _lib.check(1, "uavtrack_step_host")
        if self._host_views is None:      # (the library's block is allocated once per handle: the pointers never change)
            B, N, M = self.B, self.N, self.M

            def view(ptr, shape, ctype, dtype):
                if not ptr:
                    return None
                n = int(np.prod(shape))
                return np.frombuffer((ctype * n).from_address(ptr), dtype=dtype).reshape(shape)
            f, i32, u8 = (C.c_float, np.float32), (C.c_int32, np.int32), (C.c_uint8, np.uint8)
            spec = dict(obs=((B, N, _lib.OBS_DIM), f), reward=((B, N), f), terms=((3, B, N), f), raw=((B, N), f),
                        covered=((B,), i32), done=((B,), u8), ux=((B, N), f), uy=((B, N), f), uz=((B, N), f), uh=((B, N), f),
                        ua=((B, N), i32), tx=((B, M), f), ty=((B, M), f), tz=((B, M), f), th=((B, M), f), step_count=((B,), i32))
            self._host_views = {k: view(getattr(hs, k), shape, ct, dt) for k, (shape, (ct, dt)) in spec.items()}
        return self._host_views

    def step_many(self, actions, want_obs: bool = True, want_terms: bool = True, want_ep_sums: bool = True,
                  out: Optional[Dict[str, torch.Tensor]] = None, want_targets: bool = False,
                  auto_reset_seed: Optional[int] = None, want_raw: bool = False) -> Dict[str, torch.Tensor]:
        """T steps in one launch; `actions` is [T, B, N].  Pass the previous result as
        `out` to reuse its buffers.  want_targets adds "targets" [T, B, M, 2], the target tracks of t_xy<ep>.csv;
        want_raw adds "raw" [T, B, N], uav.raw_reward (environment.py:219).
        auto_reset_seed: environments whose done flag fires are reset inside the launch (reset(seed, next episode)),
        so the launch may span episodes (uavtrack_step_many_autoreset)."""
        a = torch.as_tensor(actions)
        T = int(a.shape[0])
        a = self._actions(a, (T, self.B, self.N))
        return self._eager("step_many", T, out, dict(obs=want_obs, reward=True, terms=want_terms, covered=True, done=True,
                                                     ep_sums=want_ep_sums), dict(targets=want_targets, raw=want_raw),
                           dict(actions=a), auto_reset_seed=auto_reset_seed)

    def _eager(self, entry, T, out, want, attach, given, seed=0, mode=0, auto_reset_seed=None) -> Dict[str, torch.Tensor]:
        """step_many / run_greedy / run_actor: the wanted buffers (reused from `out` where they fit) and the `given`
        inputs, one launch with the `attach`ed installed outputs around it, the result dictionary."""
        o = out or {}
        res = {k: self._reuse(o, k, T, w) for k, w in want.items()}
        fn, args, name = self._rollout_call(entry, T, {**res, **given}, seed, mode, auto_reset_seed)
        launch = lambda: _lib.check(fn(*args), name)
        for kind, w in attach.items():
            launch = functools.partial(self._attached, kind, T, w, o, launch)
        res.update(launch() or {})
        self._count_episodes(T, auto_reset_seed)
        return res

    def bind_step_many(self, actions: torch.Tensor, out: Dict[str, torch.Tensor]):
        """A zero-argument callable that issues `uavtrack_step_many(actions -> out)` on the stream current NOW, with
        every ctypes argument built once: what a driver replays when the per-call Python of step_many (tensor checks,
        slicing, dict building: tens of microseconds) would be a visible share of a short launch."""
        T = int(actions.shape[0])
        a = self._actions(actions, (T, self.B, self.N))
        self._check_out(out, ("obs", "reward", "terms", "covered", "done", "ep_sums"), T)
        fn, args, name = self._rollout_call("step_many", T, dict(out, actions=a))
        keep = (a, out)

        def call():
            if fn(*args) != 0:
                _lib.check(1, name)
            return keep[1]
        return call

    def bind_reset(self, seed: int, obs: torch.Tensor):
        """Callable(episode) issuing `uavtrack_reset` into the caller's obs buffer with pre-built arguments."""
        if not self._fits(obs, (self.B, self.N, _lib.OBS_DIM), torch.float32):
            raise ValueError("obs must be a contiguous float32 [B, N, 12] tensor on this device")
        h, fn, s64, optr, st = self._h, self._lib.uavtrack_reset, C.c_uint64(seed & (2 ** 64 - 1)), _ptr(obs), self._stream()

        def call(episode: int):
            if fn(h, s64, C.c_uint32(episode), optr, st) != 0:
                _lib.check(1, "uavtrack_reset")
            return obs
        return call

    # -- state injection / checkpoint -------------------------------------------------
    def get_state(self) -> Dict[str, torch.Tensor]:
        three = self.cfg.dim == 3
        s = dict(ux=self._empty((self.B, self.N), torch.float32), uy=self._empty((self.B, self.N), torch.float32),
                 uz=self._empty((self.B, self.N), torch.float32) if three else None,
                 uh=self._empty((self.B, self.N), torch.float32), ua=self._empty((self.B, self.N), torch.int32),
                 tx=self._empty((self.B, self.M), torch.float32), ty=self._empty((self.B, self.M), torch.float32),
                 tz=self._empty((self.B, self.M), torch.float32) if three else None,
                 th=self._empty((self.B, self.M), torch.float32),
                 step_count=self._empty((self.B,), torch.int32),
                 episode=self._empty((self.B,), torch.int32))
        _lib.check(self._lib.uavtrack_get_state(self._h, *[_ptr(s[k]) for k in _STATE_KEYS],
                                                _ptr(s["step_count"]), self._stream()), "uavtrack_get_state")
        _lib.check(self._lib.uavtrack_get_episodes(self._h, _ptr(s["episode"]), self._stream()), "uavtrack_get_episodes")
        return {k: v for k, v in s.items() if v is not None}

    def set_state(self, ux, uy, uh, ua, tx, ty, th, uz=None, tz=None, step_count=None, episode=None) -> None:
        """Inject a state (parity tests) or restore a get_state() checkpoint: `env.set_state(**ckpt)`.  `episode` [B]
        (the number of each environment's last reset) keys the next automatic reset; when it is given the host-side
        episode counter moves past its largest entry, so a later reset() does not replay a used episode number."""
        def f(v, shape, dtype):
            if v is None:
                return None
            t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)
            t = t.to(device=self.device, dtype=dtype).reshape(shape).contiguous()
            return t
        BN, BM = (self.B, self.N), (self.B, self.M)
        arrs = dict(ux=f(ux, BN, torch.float32), uy=f(uy, BN, torch.float32), uz=f(uz, BN, torch.float32),
                    uh=f(uh, BN, torch.float32), ua=f(ua, BN, torch.int32),
                    tx=f(tx, BM, torch.float32), ty=f(ty, BM, torch.float32), tz=f(tz, BM, torch.float32),
                    th=f(th, BM, torch.float32))
        sc = f(step_count, (self.B,), torch.int32)
        ep = f(episode, (self.B,), torch.int32)
        _lib.check(self._lib.uavtrack_set_state(self._h, *[_ptr(arrs[k]) for k in _STATE_KEYS], _ptr(sc),
                                                self._stream()), "uavtrack_set_state")
        if ep is not None:
            _lib.check(self._lib.uavtrack_set_episodes(self._h, _ptr(ep), self._stream()), "uavtrack_set_episodes")
            self._episode = max(self._episode, int(ep.max().item()) + 1)
        # the D2D copies are stream-ordered; keep the sources alive until they have run
        torch.cuda.current_stream(self.device).synchronize()

    def set_pmi(self, state_dict) -> None:
        """state_dict of a reference PMINetwork, a uavtrack.DevicePMINetwork (its current weights, through the same host
        blob), or None to disable."""
        if state_dict is None:
            _lib.check(self._lib.uavtrack_set_pmi_weights(self._h, None, 0, 0, self._stream()), "set_pmi")
            return
        blob, hidden = state_dict.folded() if isinstance(state_dict, DevicePMINetwork) else fold_pmi_state_dict(state_dict)
        _lib.check(self._lib.uavtrack_set_pmi_weights(self._h, C.c_void_p(blob.ctypes.data), blob.size, hidden,
                                                      self._stream()), "uavtrack_set_pmi_weights")

    @staticmethod
    def _pmi_publish_tensors(source, device_index: int):
        """The 26 tensors of publish_pmi's source, validated (ValueError) and contiguous -> (tensors, hidden)."""
        sd = source.state_dict() if isinstance(source, torch.nn.Module) else source
        keys = _lib.PMI_STATE_KEYS
        missing = [k for k in keys if k not in sd]
        if missing:
            raise ValueError(f"publish_pmi: the source lacks the tensors {missing}")
        ts = [sd[k] for k in keys]
        for k, t in zip(keys, ts):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" \
                    or t.device.index != device_index:
                raise ValueError(f"publish_pmi: {k} must be a float32 tensor on cuda:{device_index}")
        H = ts[0].shape[0] if ts[0].dim() == 2 else -1
        for b, fan in enumerate((5, 4, 3, 3 * H)):
            if tuple(ts[6 * b].shape) != (H, fan) or any(tuple(t.shape) != (H,) for t in ts[6 * b + 1:6 * b + 6]):
                raise ValueError(f"publish_pmi: the tensors of {keys[6 * b]} and its BatchNorm1d do not have the shapes of "
                                 f"Linear({fan}, H) + BatchNorm1d(H), H = {H}")
        if tuple(ts[24].shape) != (1, H) or ts[25].numel() != 1:
            raise ValueError(f"publish_pmi: fc2 must be Linear({H}, 1), got weight {tuple(ts[24].shape)}")
        return [t.detach().contiguous() for t in ts], int(H)

    def publish_pmi(self, source) -> None:
        """set_pmi without the host: BatchNorm fold, bounds, scales and every packed layout are computed on the device
        from device tensors, stream-ordered (no copy to the host, no synchronisation; capturable), bit for bit what
        set_pmi installs from the same numbers.  source: a DevicePMINetwork (its own state), a module with make_pmi_net's
        parameter names, or a state dict of fp32 tensors on this device.  Weights of the same hidden width must be
        installed (set_pmi sizes the allocation).  A non-contiguous tensor is made contiguous on the device; a missing
        key, a wrong device, dtype or shape raises ValueError before anything is enqueued."""
        if isinstance(source, DevicePMINetwork):
            source.publish_pmi(self)
            return
        ts, H = self._pmi_publish_tensors(source, self._device_index)
        arg = _lib.PmiTensors()
        for k, t in enumerate(ts):
            arg.t[k] = t.data_ptr()
        _lib.check(self._lib.uavtrack_publish_pmi_weights(self._h, C.byref(arg), C.c_int32(H), self._stream()),
                   "uavtrack_publish_pmi_weights")
        # the launches read the tensors when they run: keep the contiguous copies alive until the next publish
        self._pmi_publish_keep = ts

    def pmi_blob(self) -> np.ndarray:
        """The installed PMI weights allocation (csrc/pmi_pack.h: the fp32 blob in scorer order, the bf16 / f16 planes,
        the scalar block) as uint32 words, read back to the host (synchronises): an inspection aid, e.g. to compare
        set_pmi and publish_pmi bit for bit."""
        n = C.c_int64(0)
        _lib.check(self._lib.uavtrack_pmi_blob_floats(self._h, C.byref(n)), "uavtrack_pmi_blob_floats")
        out = np.empty(n.value, np.uint32)
        _lib.check(self._lib.uavtrack_get_pmi_blob(self._h, _lib.host_ptr(out), out.size, self._stream()),
                   "uavtrack_get_pmi_blob")
        return out

    def set_pmi_scheme(self, scheme: str = "auto") -> None:
        """Pin the MAAC-R pair scorer: "auto" (default: the fastest the weights allow), "f16x3", "bf16x6" or "fp32"
        (uavtrack_set_pmi_scheme).  Raises if the loaded weights cannot run on it."""
        if scheme not in _lib.PMI_SCHEMES:
            raise ValueError(f"scheme must be one of {_lib.PMI_SCHEMES}")
        _lib.check(self._lib.uavtrack_set_pmi_scheme(self._h, C.c_int32(_lib.PMI_SCHEMES.index(scheme))), "uavtrack_set_pmi_scheme")

    def pmi_info(self) -> Dict[str, object]:
        """{"scheme": the scorer the next MAAC-R step launches (None without weights), "hidden_padded", "f16_range_ok": the
        host-side range guard passed, "rescored_chunks": chunks the wide-range kernel scored again because an operand left
        f16's range at run time}.  After a publish_pmi, "scheme" and "f16_range_ok" follow the verdict the device reached
        (pmi_publish_info has the counters of that path).  Synchronises the stream."""
        out = (C.c_int64 * 4)()
        _lib.check(self._lib.uavtrack_pmi_info(self._h, out, self._stream()), "uavtrack_pmi_info")
        return dict(scheme=_lib.PMI_SCHEMES[out[0]] if out[0] else None, hidden_padded=int(out[1]), f16_range_ok=bool(out[2]),
                    rescored_chunks=int(out[3]))

    def pmi_publish_info(self) -> Dict[str, object]:
        """{"device_published": the installed weights come from publish_pmi (False after set_pmi), "unfit_chunks": chunks
        the wide-range kernel scored because device-published weights did not fit f16's range -- counted apart from
        pmi_info's "rescored_chunks", which stays the run-time range watch's}.  Synchronises the stream."""
        pub = (C.c_int64 * 2)()
        _lib.check(self._lib.uavtrack_pmi_publish_info(self._h, pub, self._stream()), "uavtrack_pmi_publish_info")
        return dict(device_published=bool(pub[0]), unfit_chunks=int(pub[1]))

    def launch_info(self) -> Dict[str, int]:
        """Geometry of the most recent rollout launch (uavtrack_launch_info)."""
        out = (C.c_int64 * 4)()
        _lib.check(self._lib.uavtrack_launch_info(self._h, out), "uavtrack_launch_info")
        return dict(workgroup=int(out[0]), envs_per_workgroup=int(out[1]), workgroups=int(out[2]), single_wavefront_variant=int(out[3]))

    def variant_info(self) -> tuple:
        """Template arguments of the rollout kernel the most recent launch ran (uavtrack_variant_info): (N_, M_, MODE as
        instantiated, Z3, POLICY, ALLOUT, EXTRAS, LONE); N_ = M_ = 0 is the generic kernel.  All -1 before the first
        launch (all zeros is a real kernel)."""
        out = (C.c_int64 * 8)()
        _lib.check(self._lib.uavtrack_variant_info(self._h, out), "uavtrack_variant_info")
        return tuple(int(x) for x in out)

    def pmi_inference(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """PMINetwork.inference (PMINet.py:64-72) on a batch of pair inputs x [n, 12] (= la_i * la_j, uav.py:281) with the
        uploaded weights, on the MAAC-R scorer kernels -> scores [n]."""
        if x.dim() != 2 or not self._fits(x, (x.shape[0], _lib.OBS_DIM), torch.float32):
            raise ValueError(f"x must be a contiguous float32 [n, {_lib.OBS_DIM}] tensor on {self.device}")
        n = int(x.shape[0])
        s = self._out_arg(out, (n,), torch.float32, "out")
        _lib.check(self._lib.uavtrack_pmi_inference(self._h, _ptr(x), C.c_int64(n), _ptr(s), self._stream()),
                   "uavtrack_pmi_inference")
        return s

    def greedy_actions(self, seed: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The reference's C-METHOD baseline policy (uav.py:324-369) for every UAV -> int32 [B, N]."""
        a = self._out_arg(out, (self.B, self.N), torch.int32, "out")
        _lib.check(self._lib.uavtrack_greedy_actions(self._h, C.c_uint64(seed & (2 ** 64 - 1)), _ptr(a),
                                                     self._stream()), "uavtrack_greedy_actions")
        return a

    def run_greedy(self, T: int, seed: int = 0, want_obs: bool = True, want_terms: bool = True,
                   want_actions: bool = True, want_targets: bool = False,
                   out: Optional[Dict[str, torch.Tensor]] = None, auto_reset_seed: Optional[int] = None,
                   want_start_obs: bool = False) -> Dict[str, torch.Tensor]:
        """T closed-loop steps of the C-METHOD baseline (train.py:326-370) in one launch.  Pass a previous result as
        `out` to reuse its buffers.  auto_reset_seed / want_start_obs: as run_actor."""
        return self._eager("run_greedy", T, out, dict(actions=want_actions, obs=want_obs, reward=True, terms=want_terms,
                                                      covered=True, done=True, ep_sums=True),
                           dict(targets=want_targets, start_obs=want_start_obs), {}, seed, 0, auto_reset_seed)

    # ---- the learner's shared actor on the device (actor_critic.py:85-98, 138-148) ----
    def set_actor(self, actor) -> None:
        """Upload FnnPolicyNet parameters: a module / state_dict with fc1.weight [H,12], fc1.bias, fc2.weight
        [na,H], fc2.bias (actor_critic.py:85-98), or None to remove them."""
        if actor is None:
            _lib.check(self._lib.uavtrack_set_actor_weights(self._h, None, None, None, None, C.c_int32(0),
                                                            self._stream()), "uavtrack_set_actor_weights")
            self._actor_hidden = 0
            return
        sd = actor.state_dict() if hasattr(actor, "state_dict") else actor
        host = [sd[k].detach().to("cpu", torch.float32).contiguous()
                for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")]
        w1, b1, w2, b2 = host
        if w1.shape[1] != _lib.OBS_DIM or w2.shape != (self.cfg.na_total, w1.shape[0]):
            raise ValueError(f"actor shapes fc1 {tuple(w1.shape)}, fc2 {tuple(w2.shape)} do not match "
                             f"Linear({_lib.OBS_DIM}, H) / Linear(H, {self.cfg.na_total})")
        _lib.check(self._lib.uavtrack_set_actor_weights(self._h, *[C.c_void_p(t.data_ptr()) for t in host],
                                                        C.c_int32(w1.shape[0]), self._stream()),
                   "uavtrack_set_actor_weights")
        self._actor_hidden = w1.shape[0]

    def publish_actor(self, source) -> None:
        """set_actor without the host: the blob is packed on the device from device tensors, stream-ordered (no copy to
        the host, no synchronisation; capturable).  source: a DeviceActorCritic (its own parameters), an ActorMLP or a
        state dict of fp32 tensors on this device (fc1.weight [H, 12], fc1.bias, fc2.weight [na*nc, H], fc2.bias).  The
        installed actor must have the same H (set_actor sizes it).  A non-contiguous tensor is made contiguous on the
        device; a wrong device, dtype or shape raises ValueError before anything is enqueued."""
        from .learner import DeviceActorCritic
        if isinstance(source, DeviceActorCritic):
            source.publish_actor(self)
            return
        sd = source.state_dict() if isinstance(source, torch.nn.Module) else source
        keys = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
        if not all(k in sd for k in keys):
            raise ValueError(f"publish_actor: the source needs the tensors {keys}")
        ts = [sd[k] for k in keys]
        for k, t in zip(keys, ts):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" \
                    or t.device.index != self._device_index:
                raise ValueError(f"publish_actor: {k} must be a float32 tensor on cuda:{self._device_index}")
        w1, b1, w2, b2 = ts
        H, A = (w1.shape[0] if w1.dim() == 2 else -1), self.cfg.na_total
        if w1.shape != (H, _lib.OBS_DIM) or b1.shape != (H,) or w2.shape != (A, H) or b2.shape != (A,):
            raise ValueError(f"publish_actor: shapes fc1 {tuple(w1.shape)} / {tuple(b1.shape)}, fc2 {tuple(w2.shape)} / "
                             f"{tuple(b2.shape)} do not match Linear({_lib.OBS_DIM}, H) / Linear(H, {A})")
        ts = [t.detach().contiguous() for t in ts]
        _lib.check(self._lib.uavtrack_publish_actor_weights(self._h, *[_ptr(t) for t in ts], C.c_int32(H),
                                                            self._stream()), "uavtrack_publish_actor_weights")

    def actor_blob(self) -> np.ndarray:
        """The installed actor blob (csrc/actor.h layout) as float32, read back to the host (synchronises): an
        inspection aid, e.g. to compare set_actor and publish_actor bit for bit."""
        H = getattr(self, "_actor_hidden", 0)
        at = 2 if self.cfg.dim == 3 else 1
        out = np.empty(128 + (H + 31) // 32 * (2 + 4 * at) * 256, np.float32)
        _lib.check(self._lib.uavtrack_get_actor_blob(self._h, _lib.host_ptr(out), out.size, self._stream()),
                   "uavtrack_get_actor_blob")
        return out

    def actor_actions(self, obs: torch.Tensor, seed: int = 0, mode: int = _lib.ACTOR_SAMPLE,
                      want_probs: bool = False, out: Optional[torch.Tensor] = None):
        """take_action for every UAV (actor_critic.py:138-148) -> int32 [B, N] (and probs [B, N, na] if asked)."""
        if obs.shape != (self.B, self.N, _lib.OBS_DIM) or obs.dtype != torch.float32 or not obs.is_contiguous() \
                or obs.device != self.device:
            raise ValueError(f"obs must be a contiguous float32 [{self.B}, {self.N}, {_lib.OBS_DIM}] tensor on {self.device}")
        a = self._out_arg(out, (self.B, self.N), torch.int32, "out")
        probs = self._empty((self.B, self.N, self.cfg.na_total), torch.float32) if want_probs else None
        _lib.check(self._lib.uavtrack_actor_actions(self._h, _ptr(obs), C.c_uint64(seed & (2 ** 64 - 1)),
                                                    C.c_int32(mode), _ptr(a), _ptr(probs), self._stream()),
                   "uavtrack_actor_actions")
        return (a, probs) if want_probs else a

    def run_actor(self, T: int, obs_in: torch.Tensor, seed: int = 0, mode: int = _lib.ACTOR_SAMPLE,
                  want_terms: bool = True, out: Optional[Dict[str, torch.Tensor]] = None,
                  want_targets: bool = False, auto_reset_seed: Optional[int] = None,
                  want_start_obs: bool = False) -> Dict[str, torch.Tensor]:
        """T closed-loop steps of actor + environment (the rollout of train.operate_epoch, train.py:160-192) in
        one launch.  obs_in [B, N, 12] is what the policy sees first (reset()'s return or the last obs).
        auto_reset_seed: environments whose done flag fires are reset inside the launch (reset(auto_reset_seed, next
        episode)), so the launch may span episodes; episode e of an environment draws with seed + e
        (uavtrack_run_actor_autoreset).  want_start_obs adds "start_obs" [T, B, N, 12]: where done[t, b] fired, the fresh
        state's observation -- the policy's input at step t + 1; other rows are never written (and without
        auto_reset_seed none is)."""
        if obs_in.shape != (self.B, self.N, _lib.OBS_DIM) or obs_in.dtype != torch.float32 \
                or not obs_in.is_contiguous() or obs_in.device != self.device:
            raise ValueError(f"obs_in must be a contiguous float32 [{self.B}, {self.N}, {_lib.OBS_DIM}] tensor on {self.device}")
        return self._eager("run_actor", T, out, dict(actions=True, obs=True, reward=True, terms=want_terms, covered=True,
                                                     done=True, ep_sums=True),
                           dict(targets=want_targets, start_obs=want_start_obs), dict(obs_in=obs_in), seed, mode, auto_reset_seed)

    def bind_run(self, T: int, out: Dict[str, torch.Tensor], policy: str = "actor", obs_in: Optional[torch.Tensor] = None,
                 seed: int = 0, mode: int = _lib.ACTOR_SAMPLE, auto_reset_seed: Optional[int] = None,
                 want_start_obs: bool = False):
        """A zero-argument callable that issues `uavtrack_run_actor` / `uavtrack_run_greedy` (T steps, policy inside the
        kernel) into `out` on the stream current NOW, with every ctypes argument built once -- what a driver that issues
        short fused chunks replays (the per-call Python of run_actor is a visible share of a 10-step launch).
        auto_reset_seed: the automatic-reset forms of the two calls (the host episode counter advances per call, as in
        run_actor).  want_start_obs: out["start_obs"] [T, B, N, 12] (allocated when missing) is installed as the
        start-observation buffer now and stays installed."""
        self._check_out(out, ("actions", "obs", "reward", "terms", "covered", "done", "ep_sums"), T)
        if policy not in ("actor", "greedy"):
            raise ValueError("policy must be 'actor' or 'greedy'")
        if policy == "actor" and not self._fits(obs_in, (self.B, self.N, _lib.OBS_DIM), torch.float32):
            raise ValueError("obs_in must be a contiguous float32 [B, N, 12] tensor on this device")
        if want_start_obs:
            out["start_obs"] = self._reuse(out, "start_obs", T)
            self.set_start_obs_output(out["start_obs"])
        fn, args, name = self._rollout_call(f"run_{policy}", T, dict(out, obs_in=obs_in), seed, mode, auto_reset_seed)
        keep = (out, obs_in)

        def call():
            if fn(*args) != 0:
                _lib.check(1, name)
            self._count_episodes(T, auto_reset_seed)
            return keep[0]
        return call

    @staticmethod
    def clip_saturation(terms: torch.Tensor, reward: torch.Tensor) -> Dict[str, int]:
        """Diagnostic counterpart of the reference's "overstep in clip." print (data_util.py:44-47): how many values of a
        rollout's outputs sit ON a clip bound -- terms [..., 3, B, N] (tracking at 1, duplicate at -1) and reward [..., B, N]
        (at +-1).  A raw value beyond the bound ends there (the kernels clamp like `np.clip`), so a non-zero count where
        `EnvConfig.clip_can_overstep()` says it can happen is the reference's message; exactly on the bound is counted too."""
        tt, dup = terms.select(-3, 0), terms.select(-3, 2)
        return {"tracking": int((tt >= 1.0).sum()), "duplicate": int((dup <= -1.0).sum()),
                "reward": int((reward.abs() >= 1.0).sum())}

    def set_profiling(self, on: bool) -> None:
        """HIP event pairs around every kernel launch of the stepping calls (uavtrack_set_profiling); read with profile()."""
        _lib.check(self._lib.uavtrack_set_profiling(self._h, C.c_int32(1 if on else 0)), "uavtrack_set_profiling")

    def profile(self) -> Dict[str, Dict[str, float]]:
        """{kernel class: {"ms": total, "launches": n}} since the last call (synchronises the stream)."""
        ms = (C.c_double * len(_lib.PROF_CLASSES))()
        cnt = (C.c_int64 * len(_lib.PROF_CLASSES))()
        _lib.check(self._lib.uavtrack_get_profile(self._h, ms, cnt, self._stream()), "uavtrack_get_profile")
        return {k: {"ms": float(ms[i]), "launches": int(cnt[i])} for i, k in enumerate(_lib.PROF_CLASSES)}

    def pmi_pairs_scored(self) -> int:
        """Neighbour pairs the PMI network has scored so far (synchronises the stream)."""
        out = C.c_uint64(0)
        _lib.check(self._lib.uavtrack_pmi_pairs_scored(self._h, C.byref(out), self._stream()), "pmi_pairs_scored")
        return int(out.value)

    @property
    def reward_mode(self) -> RewardMode:
        return self.cfg.resolved_mode()
