"""Multi-GPU layout: environments are independent (each reference Environment owns its
own lists, src/environment.py:36-43), so the batch is split by rank with no per-step
traffic.  The only exchange is the end-of-rollout gather of the per-environment episode
accumulators (train.py:181-192), one all-gather over RCCL/xGMI (gloo on CPU tensors)."""
from __future__ import annotations

from typing import Optional, Tuple


def shard_range(n_envs_total: int, rank: int, world_size: int) -> Tuple[int, int]:
    """(first global env id, env count) of `rank`; the remainder goes to the low ranks."""
    if not (0 <= rank < world_size):
        raise ValueError(f"rank {rank} outside world of {world_size}")
    q, r = divmod(n_envs_total, world_size)
    count = q + (1 if rank < r else 0)
    offset = rank * q + min(rank, r)
    return offset, count


class SummaryGather:
    """Handle of one in-flight end-of-rollout gather (gather_rollout_summary_async).  `wait()` returns the
    [B_total, 5] tensor ordered by global env id; on RCCL it makes the *current stream* wait, not the host."""

    def __init__(self, work, out, dev, n_envs_total, world, b_max, passthrough=None):
        self._work, self._out, self._dev = work, out, dev
        self._n, self._world, self._b_max = n_envs_total, world, b_max
        self._result = passthrough

    def wait(self):
        if self._result is not None:
            return self._result
        if self._work is not None:
            self._work.wait()
        out = self._out.to(self._dev)
        if self._n != self._world * self._b_max:
            parts = []
            for r in range(self._world):
                _, cnt = shard_range(self._n, r, self._world)
                parts.append(out[r * self._b_max:r * self._b_max + cnt])
            out = torch_cat(parts)
        self._result = out
        return out


def torch_cat(parts):
    import torch
    return torch.cat(parts, dim=0)


def gather_rollout_summary_async(ep_sums, n_envs_total: Optional[int] = None, group=None) -> SummaryGather:
    """Start the all-gather of the [B_local, 5] episode accumulators and return at once: the collective runs on
    RCCL's own stream from a private copy of `ep_sums`, so the next rollout (which overwrites `ep_sums`) can be
    launched immediately and overlaps the exchange and any skew between ranks."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return SummaryGather(None, None, None, 0, 1, 0, passthrough=ep_sums)
    world = dist.get_world_size(group)
    b_local = ep_sums.shape[0]
    if n_envs_total is None:
        n_envs_total = b_local * world
    b_max = -(-n_envs_total // world)
    send = torch.zeros((b_max,) + tuple(ep_sums.shape[1:]), dtype=ep_sums.dtype, device=ep_sums.device)
    send[:b_local] = ep_sums           # private copy (also the padding of an uneven shard)
    dev = ep_sums.device
    if dev.type == "cuda" and dist.get_backend(group) == "gloo":
        send = send.cpu()          # rehearsal / debugging on gloo: stage through the host
    out = torch.empty((world * b_max,) + tuple(ep_sums.shape[1:]), dtype=ep_sums.dtype, device=send.device)
    work = dist.all_gather_into_tensor(out, send.contiguous(), group=group, async_op=True)
    return SummaryGather(work, out, dev, n_envs_total, world, b_max)


def gather_rollout_summary(ep_sums, n_envs_total: Optional[int] = None, group=None):
    """All-gather the [B_local, 5] episode accumulators into [B_total, 5], ordered by
    global env id.  Uneven shards (n_envs_total % world != 0) are padded for the
    collective and trimmed afterwards."""
    return gather_rollout_summary_async(ep_sums, n_envs_total, group).wait()


# ---------------------------------------------------------------------------------------------------------------------
# The learner's side of a sharded rollout.  The reference has ONE learner that consumes (state, action, reward,
# next_state) transitions (train.py:176-194, 250-252); with the rollouts on R ranks it needs a sample of every rank's
# transitions, not the trajectories themselves (1 GB per rank and rollout at 4096 x 20 x 200).  Each rank draws K of its
# own transitions, packs them into one [K, 28] int32 block (bit views: nothing is converted) and ONE all-gather per rollout
# hands every rank -- the learner among them -- the R K sampled rows, ready for DeviceReplayBuffer.add().

TRANSITION_WORDS = 12 + 1 + 1 + 12 + 2      # state, action, reward, next_state, global transition id (int64)


def sample_local_transitions(obs_in, out, k: int, env_offset: int = 0, n_envs_total: Optional[int] = None, generator=None):
    """K transitions of this rank's rollout, uniformly without replacement: out = {obs [T,B,N,12], actions [T,B,N],
    reward [T,B,N]} (a step_many / run_actor result plus the actions that drove it), obs_in [B,N,12] what the policy saw
    first.  Returns {"states" [K,12], "actions" [K] int32, "rewards" [K], "next_states" [K,12], "index" [K] int64}; index =
    (t * B_total + env_offset + b) * N + i, the transition's place in the UNSHARDED rollout's [T, B_total, N] grid (for
    priorities, de-duplication, and the tests).  The [T+1] state array of transitions_from_rollout is never built."""
    import torch
    obs, act, rew = out["obs"], out["actions"], out["reward"]
    T, B, N = rew.shape
    n = T * B * N
    if not (0 < k <= n):
        raise ValueError(f"k = {k} outside (0, {n}] transitions of this rollout")
    if n_envs_total is None:
        n_envs_total = B
    dev = rew.device
    if 16 * k <= n:
        # k << n (4096 of 16.4 M at the reference shape): a permutation of all n would cost more than the rollout.  The
        # distinct values among m uniform draws are a uniform random subset of their size; a uniform k-subset of that set
        # is a uniform k-subset of the rollout, and the permutation that picks it also randomises the order.
        cand = torch.unique(torch.randint(0, n, (k + k // 4 + 64,), device=dev, generator=generator))
        pick = (cand[torch.randperm(cand.numel(), device=dev, generator=generator)[:k]] if cand.numel() >= k
                else torch.randperm(n, device=dev, generator=generator)[:k])
    else:
        pick = torch.randperm(n, device=dev, generator=generator)[:k]
    t, rem = pick // (B * N), pick % (B * N)
    b, i = rem // N, rem % N
    prev = obs[(t - 1).clamp(min=0), b, i]
    states = torch.where((t == 0).unsqueeze(1), obs_in[b, i], prev)
    return {"states": states, "actions": act[t, b, i].to(torch.int32), "rewards": rew[t, b, i],
            "next_states": obs[t, b, i], "index": (t * n_envs_total + env_offset + b) * N + i}


def _pack_transitions(s):
    import torch
    k = s["actions"].shape[0]
    return torch.cat([s["states"].contiguous().view(torch.int32), s["actions"].view(k, 1),
                      s["rewards"].contiguous().view(torch.int32).view(k, 1), s["next_states"].contiguous().view(torch.int32),
                      s["index"].contiguous().view(torch.int32).view(k, 2)], dim=1).contiguous()


def _unpack_transitions(blk):
    import torch
    return {"states": blk[:, 0:12].contiguous().view(torch.float32), "actions": blk[:, 12].contiguous(),
            "rewards": blk[:, 13].contiguous().view(torch.float32), "next_states": blk[:, 14:26].contiguous().view(torch.float32),
            "index": blk[:, 26:28].contiguous().view(torch.int64).view(-1)}


class TransitionGather:
    """Handle of one in-flight transition gather; wait() -> the dict of sample_local_transitions with R K rows, rank-major."""

    def __init__(self, work, out, dev, world=1, passthrough=None):
        self._work, self._out, self._dev, self._world, self._result = work, out, dev, world, passthrough

    @property
    def nbytes_per_rank(self) -> int:
        """bytes each rank contributes to the collective (0 without a process group)"""
        return 0 if self._out is None else self._out.numel() * 4 // self._world

    def wait(self):
        if self._result is None:
            if self._work is not None:
                self._work.wait()
            self._result = _unpack_transitions(self._out.to(self._dev))
        return self._result


def gather_transitions_async(sample, group=None) -> TransitionGather:
    """Start the all-gather of every rank's K sampled transitions (equal K on all ranks) and return at once; like
    gather_rollout_summary_async it runs from a private packed copy on RCCL's own stream."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return TransitionGather(None, None, None, passthrough=dict(sample))
    world = dist.get_world_size(group)
    send = _pack_transitions(sample)
    dev = send.device
    if dev.type == "cuda" and dist.get_backend(group) == "gloo":
        send = send.cpu()          # rehearsal on gloo: stage through the host
    out = torch.empty((world * send.shape[0], TRANSITION_WORDS), dtype=torch.int32, device=send.device)
    work = dist.all_gather_into_tensor(out, send, group=group, async_op=True)
    return TransitionGather(work, out, dev, world)


def gather_transitions(sample, group=None):
    """Blocking form: {"states" [R K, 12], "actions", "rewards", "next_states", "index"} on every rank."""
    return gather_transitions_async(sample, group).wait()


# ---------------------------------------------------------------------------------------------------------------------
# Data-parallel learners.  Each rank holds a shard, its own replay ring and a DeviceActorCritic; one update is the
# gradient row of every rank's batch (DeviceActorCritic.grad_from), ONE all-gather of the rows in rank order, and the
# same ordered apply on every rank (DeviceActorCritic.update_from(..., group=...)).  The rows travel as int32 bit views
# (their tail words are integers), so no backend touches a bit.


def gather_learner_rows(row, group=None):
    """All-gather of one gradient row per rank into [world, row_floats], rank-major, on the row's device.  Without a
    process group, or with one rank, the row itself as [1, row_floats]."""
    import torch
    import torch.distributed as dist
    row = row.reshape(1, -1)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return row
    world = dist.get_world_size(group)
    dev = row.device
    send = row.contiguous().view(torch.int32)
    if dev.type == "cuda" and dist.get_backend(group) == "gloo":
        send = send.cpu()          # rehearsal on gloo: stage through the host
    out = torch.empty((world, send.shape[1]), dtype=torch.int32, device=send.device)
    dist.all_gather_into_tensor(out, send, group=group)
    return out.to(dev).view(torch.float32)


def pack_learner_state(learner):
    """Everything that makes two learners update alike, as one int32 numpy block of a length that depends on the shapes
    alone: the parameters and both Adam moments as bit views [3 P], the step counts [8 int64], the regularisation
    settings (entropy_coef and the two max norms) and the target settings (tau or NaN, period or 0) as float64 bit views,
    then the target critic's 14 H + 1 words (zeros while no target is enabled)."""
    import numpy as np
    m, v, steps = learner._optim_state()
    tgt = learner.get_target()
    on = tgt["tau"] is not None or tgt["period"] is not None
    settings = np.array([float("nan") if tgt["tau"] is None else tgt["tau"], tgt["period"] or 0], np.float64)
    theta = learner._get_target_params() if on else np.zeros(14 * learner.hidden_dim + 1, np.float32)
    return np.concatenate([learner._get_params().view(np.int32), m.view(np.int32), v.view(np.int32),
                           np.ascontiguousarray(steps, np.int64).view(np.int32),
                           np.array(learner.get_regularisation(), np.float64).view(np.int32), settings.view(np.int32),
                           np.ascontiguousarray(theta, np.float32).view(np.int32)])


def unpack_learner_state(learner, blk) -> None:
    """pack_learner_state's inverse into a learner of the same shapes: afterwards it updates bit for bit like the one
    that was packed.  A block without a target turns this learner's target off."""
    import numpy as np

    def f32(a):
        return np.ascontiguousarray(a).view(np.float32)
    P, T = learner.num_params, 14 * learner.hidden_dim + 1
    blk = np.ascontiguousarray(blk, np.int32)
    if blk.size != 3 * P + 16 + 6 + 4 + T:
        raise ValueError(f"unpack_learner_state: a block of {blk.size} words, this learner's has {3 * P + 26 + T}")
    learner._set_params(f32(blk[:P]))
    steps, rest = blk[3 * P:3 * P + 16], blk[3 * P + 16:]
    learner._set_optim_state(f32(blk[P:2 * P]), f32(blk[2 * P:3 * P]), np.ascontiguousarray(steps).view(np.int64))
    c, a_max, c_max, tau, period = np.ascontiguousarray(rest[:10]).view(np.float64)
    learner.set_regularisation(float(c), (float(a_max), float(c_max)))
    learner.set_target(tau=None if np.isnan(tau) else float(tau), period=int(period) or None)
    if not np.isnan(tau) or period:
        learner._set_target_params(f32(rest[10:]))


def broadcast_learner(learner, group=None, src: int = 0) -> None:
    """Rank `src`'s parameters, Adam moments, step counts, regularisation settings (entropy_coef and the two max norms)
    and target critic (its settings and, where enabled, its parameters) to every rank of `group` (src is a global
    rank), so that the ranks' learners start equal: pack_learner_state on every rank, one broadcast,
    unpack_learner_state.  Gradient rows carry no settings, so ranks that share updates must hold equal ones: change
    them on every rank alike afterwards, or broadcast again.  The advantage setting (learner.set_advantage) is NOT carried:
    call it on every rank alike.  Synchronises; meant for start-up and checkpoint loads, not the training loop."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    blk = torch.from_numpy(pack_learner_state(learner))
    if dist.get_backend(group) != "gloo":
        blk = blk.to(learner.device)
    dist.broadcast(blk, src=src, group=group)
    unpack_learner_state(learner, blk.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# MAAC-R over ranks.  PMINetwork.train_pmi trains on b2 selected (timestep, uav-pair) row pairs; only the selection
# touches the observation history.  So the ranks exchange the 2 b2 selected rows (288 KB at b2 = 3000), never a
# history, and every rank runs the whole, unsplit training step on them (DevicePMINetwork.train_pmi(group=...)): the
# BatchNorm statistics stay those of the full mini-batch and no synchronised BatchNorm is needed.


def gather_pmi_selected(selected, group=None):
    """All-gather of each rank's [b2, 2, 12] selected block (uavtrack_pmi_trainer_select into a zeroed buffer) into
    [world * b2, 2, 12], rank-major, on the block's device.  The rows travel as int32 bit views, so no backend
    touches a bit (NaN payloads, -0.0).  Without a process group, or with one rank, the block itself."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return selected
    world = dist.get_world_size(group)
    dev = selected.device
    send = selected.contiguous().view(torch.int32)
    if dev.type == "cuda" and dist.get_backend(group) == "gloo":
        send = send.cpu()          # rehearsal on gloo: stage through the host
    out = torch.empty((world * send.shape[0],) + tuple(send.shape[1:]), dtype=torch.int32, device=send.device)
    dist.all_gather_into_tensor(out, send, group=group)
    return out.to(dev).view(torch.float32)


def _pmi_owner_triples(t_idx, u_idx, group_counts, n_uav: int):
    """The triples that read draw i's rows out of the rank-major gathered block: rank r owns the timeline's timesteps
    [base_r, base_r + group_counts[r]), draw i belongs to owner(i), the rank whose span holds t_idx[i], and its two
    rows are "timestep" owner(i) * b2 + i of the block taken as world * b2 timesteps of 2 rows: t' = owner(i) * b2 + i,
    u' = (0, 1).  If any draw lies outside the timeline or [0, n_uav) (every rank's select then wrote nothing), every
    t' is -1, so that the training call on the block is refused on the device as the same draws would be on one
    process.  Device arithmetic only: no synchronisation.  Returns (t' [b2], u' [b2, 2]) int64 on t_idx's device."""
    import torch
    b2 = t_idx.numel()
    ends = torch.cumsum(torch.as_tensor(list(group_counts), dtype=torch.int64), 0).to(t_idx.device)
    owner = torch.bucketize(t_idx, ends, right=True).clamp_(max=len(group_counts) - 1)
    t2 = owner * b2 + torch.arange(b2, dtype=torch.int64, device=t_idx.device)
    bad = ((t_idx < 0) | (t_idx >= ends[-1])).any() | ((u_idx < 0) | (u_idx >= int(n_uav))).any()
    t2 = torch.where(bad, torch.full_like(t2, -1), t2)
    u2 = torch.tensor([0, 1], dtype=torch.int64, device=t_idx.device).repeat(b2, 1)
    return t2.contiguous(), u2.contiguous()


def broadcast_pmi_trainer(trainer, group=None, src: int = 0) -> None:
    """Rank `src`'s PMI network state (the state blob and num_batches_tracked), Adam moments and step counts to every
    rank of `group` (src is a global rank), so that the ranks' trainers start equal.  Synchronises; meant for start-up
    and checkpoint loads, not the training loop."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from . import _lib, adam
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    st, nbt = trainer._get()
    m, v, steps = trainer.optimizer_state()
    # one int32 block: the three float blobs as bit views, then the two int64 count arrays
    blk = torch.from_numpy(np.concatenate([st.view(np.int32), m.view(np.int32), v.view(np.int32),
                                           np.ascontiguousarray(nbt, np.int64).view(np.int32),
                                           np.ascontiguousarray(steps, np.int64).view(np.int32)]))
    if dist.get_backend(group) != "gloo":
        blk = blk.to(trainer.device)
    dist.broadcast(blk, src=src, group=group)
    blk = blk.cpu().numpy()
    S, P, nb = trainer.num_state, trainer.num_params, 2 * _lib.PMI_BN_LAYERS
    st = np.ascontiguousarray(blk[:S]).view(np.float32)
    nbt = np.ascontiguousarray(blk[S + 2 * P:S + 2 * P + nb]).view(np.int64)
    _lib.check(trainer._lib.uavtrack_pmi_trainer_set_params(trainer._h, _lib.host_ptr(st), _lib.host_ptr(nbt), st.size,
                                                            trainer._stream()), "uavtrack_pmi_trainer_set_params")
    adam.write(trainer._lib.uavtrack_pmi_trainer_set_optimizer_state, trainer._h,
               np.ascontiguousarray(blk[S:S + P]).view(np.float32), np.ascontiguousarray(blk[S + P:S + 2 * P]).view(np.float32),
               np.ascontiguousarray(blk[S + 2 * P + nb:]).view(np.int64), trainer._stream())
