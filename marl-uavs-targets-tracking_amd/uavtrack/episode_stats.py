"""The reference's `ReturnValueOfTrain` (src/train.py:12-38) on the device: the six per-episode results of
train.py:181-196 -- the return and the three reward terms, each divided by steps * n_uav, and the mean and the maximum
of the covered-target count -- folded from the outputs a rollout launch has already written (uavtrack_episode_stats_*),
one record per finished episode, across automatic resets and chunked rollouts.  Nothing returns to the host until
`read()`.  The record layout, the order of every sum and of the log, and the overflow rule are in include/uavtrack.h.

`evaluate` is the reference's `train.evaluate` (train.py:298-324) and, with policy="greedy", `train.run`
(train.py:326-396, the C-METHOD baseline), batched: every environment of the handle plays `episodes` episodes.
"""
from __future__ import annotations

import csv
import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._handle import Handle, current_device
from ._lib import ptr as _ptr

# the keys of ReturnValueOfTrain.item() (train.py:21-30) -> the record's fields
RESULT_KEYS = (("return_list", "ret"), ("target_tracking_return_list", "tracking"),
               ("boundary_punishment_return_list", "boundary"), ("duplicate_tracking_punishment_return_list", "duplicate"),
               ("average_covered_targets_list", "average_covered"), ("max_covered_targets_list", "max_covered"))
# data_util.save_csv (data_util.py:6-40): file name = key + ".csv", and its header row
CSV_HEADERS = {"return_list": "Reward", "target_tracking_return_list": "target_tracking",
               "boundary_punishment_return_list": "boundary_punishment",
               "duplicate_tracking_punishment_return_list": "duplicate_tracking_punishment",
               "average_covered_targets_list": "average_covered_targets", "max_covered_targets_list": "max_covered_targets"}
RECORD_DTYPE = np.dtype([("ret", "<f8"), ("tracking", "<f8"), ("boundary", "<f8"), ("duplicate", "<f8"),
                         ("average_covered", "<f8"), ("max_covered", "<f8"), ("env", "<i8"), ("steps", "<i4"),
                         ("ordinal", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(_lib.EpisodeRecord) == 64


def results_from_records(rec: np.ndarray, dropped: int = 0) -> Dict[str, np.ndarray]:
    """Records (RECORD_DTYPE, log order) -> the dict read() returns."""
    out = {key: rec[field].copy() for key, field in RESULT_KEYS}
    out.update(env=rec["env"].copy(), steps=rec["steps"].copy(), ordinal=rec["ordinal"].copy(), dropped=int(dropped))
    return out


def save_csv(results: Dict[str, np.ndarray], save_dir: str, extra: bool = False) -> None:
    """data_util.save_csv (data_util.py:6-40): the four files return_list.csv, target_tracking_return_list.csv,
    boundary_punishment_return_list.csv and duplicate_tracking_punishment_return_list.csv, the reference's header row,
    then one csv.writer row per value (Python floats, so the digits are the reference's).  extra adds
    average_covered_targets_list.csv and max_covered_targets_list.csv under the headers average_covered_targets and
    max_covered_targets."""
    for key, _ in RESULT_KEYS[:6 if extra else 4]:
        with open(os.path.join(save_dir, key + ".csv"), mode="w", newline="") as f:
            w = csv.writer(f)
            w.writerow([CSV_HEADERS[key]])
            for v in results[key]:
                w.writerow([float(v)])


class EpisodeStats(Handle):
    """EpisodeStats(env, log_capacity, max_steps) or EpisodeStats((n_envs, n_uav), log_capacity, max_steps, device=...).

    add(out)   folds the result dict of step_many / run_actor / run_greedy / run_fused (reward, terms, covered and, if
               present, done) into the open episodes; a step whose done flag is set closes its episode
    close()    ends every open episode that holds a step (fixed-length rollouts reset by hand)
    read()     synchronises and returns the log as numpy arrays under ReturnValueOfTrain's keys, plus env, steps,
               ordinal and dropped
    clear()    empties the log; the open episodes stay
    destroy()  frees the handle (close() is taken by the episodes, so the handle's own release has this name)
    """
    _prefix = "uavtrack_episode_stats_"

    def __init__(self, env, log_capacity: int, max_steps: int, env_offset: Optional[int] = None, device=None):
        if isinstance(env, (tuple, list)):
            n_envs, n_uav = (int(v) for v in env)
            self.device = current_device("cuda" if device is None else device)
            env_offset = 0 if env_offset is None else env_offset
        else:
            n_envs, n_uav = env.B, env.N
            self.device = current_device(env.device if device is None else device)
            env_offset = env.cfg.env_offset if env_offset is None else env_offset
        self.B, self.N = n_envs, n_uav
        self.log_capacity, self.max_steps, self.env_offset = int(log_capacity), int(max_steps), int(env_offset)
        self._create(_lib.EpisodeStatsConfig(device_id=self.device.index, n_envs=n_envs, n_uav=n_uav,
                                             env_offset=self.env_offset, max_steps=self.max_steps,
                                             log_capacity=self.log_capacity))
        self._rec = np.empty(self.log_capacity, RECORD_DTYPE)

    # the handle's release: Handle.close is the name the episodes need
    def destroy(self) -> None:
        Handle.close(self)

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def _input(self, out, key, shape, dtype):
        t = out.get(key)
        if t is None:
            raise ValueError(f"EpisodeStats.add: the rollout result has no {key!r} (ask the launch for it: want_terms=True)")
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"EpisodeStats.add: {key} must be a contiguous {dtype} {shape} tensor on {self.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
        return t

    def add(self, out: Dict[str, torch.Tensor]) -> None:
        """One launch's outputs: reward [T, B, N], terms [T, 3, B, N], covered [T, B] int32 and done [T, B] uint8 (absent
        or None: nothing closes).  Raises, enqueuing nothing, if reward, terms or covered is missing or misshapen.
        Stream-ordered on the current stream: no synchronisation, no allocation, capturable."""
        rew = out.get("reward")
        if rew is None or rew.dim() != 3:
            raise ValueError("EpisodeStats.add: the rollout result has no 'reward' [T, B, N]")
        T = int(rew.shape[0])
        rew = self._input(out, "reward", (T, self.B, self.N), torch.float32)
        terms = self._input(out, "terms", (T, 3, self.B, self.N), torch.float32)
        cov = self._input(out, "covered", (T, self.B), torch.int32)
        done = self._input(out, "done", (T, self.B), torch.uint8) if out.get("done") is not None else None
        _lib.check(self._lib.uavtrack_episode_stats_add(self._h, C.c_int64(T), _ptr(rew), _ptr(terms), _ptr(cov), _ptr(done),
                                                        self._stream()), "uavtrack_episode_stats_add")

    def close(self) -> None:
        """Ends every open episode that holds at least one step; their records follow in ascending environment."""
        _lib.check(self._lib.uavtrack_episode_stats_close(self._h, self._stream()), "uavtrack_episode_stats_close")

    def clear(self) -> None:
        _lib.check(self._lib.uavtrack_episode_stats_clear(self._h, self._stream()), "uavtrack_episode_stats_clear")

    def read_records(self):
        """(records as a RECORD_DTYPE array in log order, dropped).  Synchronises the stream."""
        n, dropped = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.uavtrack_episode_stats_read(self._h, _lib.host_ptr(self._rec), C.c_int64(self.log_capacity),
                                                         C.byref(n), C.byref(dropped), self._stream()),
                   "uavtrack_episode_stats_read")
        return self._rec[:n.value].copy(), int(dropped.value)

    def read(self) -> Dict[str, np.ndarray]:
        """The log under the reference's keys (return_list, target_tracking_return_list, boundary_punishment_return_list,
        duplicate_tracking_punishment_return_list, average_covered_targets_list, max_covered_targets_list: float64
        arrays, one entry per finished episode in log order) plus env (int64), steps, ordinal (int32) and dropped (int:
        records that found the log full since the last clear).  Synchronises the stream."""
        return results_from_records(*self.read_records())

    def save_csv(self, save_dir: str, extra: bool = False) -> None:
        """read(), then the files of data_util.save_csv (see save_csv above)."""
        save_csv(self.read(), save_dir, extra)


def evaluate(env, policy, num_steps: int, episodes: int = 1, seed: int = 0, mode: str = "sample",
             auto_reset: bool = False) -> Dict[str, np.ndarray]:
    """train.evaluate (train.py:298-324) for every environment of `env`, `episodes` times: reset, one fused launch of
    `num_steps` closed-loop steps, the six results per episode -> EpisodeStats.read() with episodes * B records (episode
    e of all environments, in ascending environment, before episode e + 1).

    policy  an FnnPolicyNet-shaped module (e.g. ActorMLP), a state dict of one, or a DeviceActorCritic: it runs as the
            fused device actor (uavtrack_run_actor), mode "sample" (Categorical sampling, what the reference evaluates
            with) or "argmax"; policy seed `seed + e`.
            "greedy": train.run (train.py:326-396), the C-METHOD baseline inside the step kernel (uavtrack_run_greedy).
            The reference's run_epoch leaves its four sums undivided; here they are divided by num_steps * n_uav like
            every other record.
    auto_reset=True: all `episodes` run in ONE launch of episodes * num_steps steps that resets each environment inside
    the kernel (uavtrack_run_actor_autoreset / _run_greedy_autoreset; the handle's horizon must equal num_steps): one
    reset(seed, episode 0) by hand, then episode e is the in-launch reset(seed, e) and draws with policy seed
    `seed + e`.  The records come from the launch's own done flags ("path" is "auto_reset"), in EpisodeStats' order for
    one add, ascending (t, b) of the closing step: episode e of all environments before episode e + 1, as below.  "ep_sums" is then [1, B, 5], the sums over
    the whole launch.  (The reset seed is `seed` for every episode here, `seed + e` below: the two forms play different
    episodes.)
    Otherwise episode e is reset by hand with reset seed `seed + e`.  How its
    record is closed depends on the handle: where the environment was created with horizon == num_steps, the launch's
    own done flags close it (the "done" path); otherwise done never fires inside the episode and
    EpisodeStats.close() ends it (the "close" path).  The returned dict says which ran under "path"; the records are
    the same either way.  "ep_sums" [episodes, B, 5] (a device tensor) holds the launches' own fp32 episode sums
    (uavtrack_run_actor's ep_sums), for cross-checks."""
    from .learner import DeviceActorCritic
    if mode not in ("sample", "argmax"):
        raise ValueError("mode must be 'sample' or 'argmax'")
    if num_steps < 1 or episodes < 1:
        raise ValueError("num_steps and episodes must be >= 1")
    greedy = isinstance(policy, str)
    if greedy and policy != "greedy":
        raise ValueError("the only named policy is 'greedy'")
    if not greedy:
        env.set_actor(policy.actor_state_dict() if isinstance(policy, DeviceActorCritic) else policy)
    by_done = env.cfg.horizon == num_steps
    if auto_reset and not by_done:
        raise ValueError(f"evaluate(auto_reset=True) needs an environment whose horizon ({env.cfg.horizon}) equals num_steps "
                         f"({num_steps}): the in-launch reset fires on the handle's own done flag")
    stats = EpisodeStats(env, log_capacity=episodes * env.B, max_steps=num_steps * (episodes if auto_reset else 1))
    out, ep = None, []
    try:
        if auto_reset:
            obs = env.reset(seed=seed, episode=0)
            kw = dict(seed=seed, auto_reset_seed=seed)
            if greedy:
                out = env.run_greedy(episodes * num_steps, want_actions=False, **kw)
            else:
                out = env.run_actor(episodes * num_steps, obs, want_terms=True,
                                    mode=_lib.ACTOR_ARGMAX if mode == "argmax" else _lib.ACTOR_SAMPLE, **kw)
            ep.append(out["ep_sums"].clone())
            stats.add(out)
        for e in range(0 if auto_reset else episodes):
            obs = env.reset(seed=seed + e, episode=e)
            if greedy:
                out = env.run_greedy(num_steps, seed=seed + e, want_actions=False, out=out)
            else:
                out = env.run_actor(num_steps, obs, seed=seed + e, want_terms=True, out=out,
                                    mode=_lib.ACTOR_ARGMAX if mode == "argmax" else _lib.ACTOR_SAMPLE)
            ep.append(out["ep_sums"].clone())
            stats.add(out if by_done else dict(out, done=None))
            if not by_done:
                stats.close()
        res = stats.read()
    finally:
        stats.destroy()
    res["path"] = "auto_reset" if auto_reset else "done" if by_done else "close"
    res["ep_sums"] = torch.stack(ep)
    return res
