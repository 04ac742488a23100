"""Device-resident replay buffers: the reference's `ReplayBuffer` / `PrioritizedReplayBuffer`
(src/train.py:41-139) hold Python tuples in a deque and are filled one UAV transition at a time
(train.py:176-180, 194).  Here a buffer is four preallocated device tensors used as a ring, filled with the
[T, B, N] outputs of a rollout in one indexed copy, and sampled with one gather -- nothing leaves the GPU.

Semantics kept from the reference: capacity-bounded FIFO overwrite (deque(maxlen) / `pos` ring); uniform
sampling WITHOUT replacement of min(batch, size) transitions (random.sample, train.py:57); prioritised sampling
WITH replacement from p_i^alpha / sum (np.random.choice, train.py:106), new transitions enter at the current
maximum priority (train.py:87-96), importance weights (size * P(i))^-beta / max (train.py:109-112).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch

KEYS = ("states", "actions", "rewards", "next_states")


class _DrawFields(NamedTuple):
    """DrawSpec's seven tuple fields, in the order they have always had."""
    importance: bool = False
    beta: float = 0.4
    beta_final: Optional[float] = None
    anneal_calls: int = 0
    rho_bar: Optional[float] = None
    rho_out: Optional[torch.Tensor] = None
    generator: Optional[torch.Generator] = None


class DrawSpec(_DrawFields):
    """How DeviceActorCritic.update_from, grad_from, update_from_many and the group path draw a batch from a buffer and
    weigh its rows: each builds one of these from its arguments and hands it to the buffer's _draw_batch(k, spec), which
    returns (indices, weights or None).  The defaults enqueue exactly the reference's update: sample(), the unweighted
    update, |td_delta| into a prioritised buffer's priorities.

    importance    train on the prioritised draw's importance weights (count * P(i))^-beta / max over this draw, one per
                  batch row (the weighted losses of uavtrack/learner.py); False drops them as the reference's update
                  does, and beta then has no effect.  A PrioritizedReplayRing writes them beside its indices in the same
                  library call, a PrioritizedDeviceReplayBuffer forms them in torch as its sample() does; a uniform
                  buffer has none.  A refused ring draw hands out NaN weights, which refuse the update on the device as
                  well.  Several buffers or ranks in one update: each draw is normalised by its own maximum.
    beta_final, anneal_calls
                  PrioritizedReplayRing only: beta runs linearly from beta to beta_final over the ring's first
                  anneal_calls draws, counted on the device, so a replayed graph anneals (every ring over its own counter).
    rho_bar       > 0, a ring made with_behaviour() (any other buffer raises): between the draw and the update,
                  uavtrack_learner_ratio_weights forms rho_i = min(rho_bar, pi(a_i|s_i) / mu(a_i|s_i)) from the ring's
                  log_mu store and the actor as it stands, and the update trains on w_i rho_i (w_i the importance weight,
                  or 1; no second normalisation), capturable like the rest.  inf does not truncate.  A drawn slot whose
                  log_mu is NaN (unknown) or positive refuses the update on the device.  td_delta and the priorities stay
                  the unweighted delta and |delta|; on an n-step or lambda ring the ratio corrects the first action only.
                  Participants of one update (ranks, shards) must pass equal rho_bar.
    rho_out       float32 [k], optional, needs rho_bar: receives the ratios.
    clip_eps      >= 0 (inf never clips), a ring made with_behaviour(), a loss="per_sample" learner, not together with
                  rho_bar (one correction for who acted, not two): the update trains PPO's clipped surrogate
                  min(r A, clip(r, 1 - eps, 1 + eps) A) with r = pi / mu from the ring's log_mu store and A = td_delta,
                  formed inside the gradient kernel (uavtrack_learner_update_clipped / _grad_clipped; no further library
                  call); the critic, td_delta and the priorities stay what they are.  importance composes: w_i is the
                  draw's weight.  A drawn slot whose log_mu is NaN (unknown) or positive, or whose ratio is not finite,
                  refuses the update on the device.  Participants of one update (ranks, shards) must pass equal clip_eps.
    ratio_out     float32 [k], optional, needs clip_eps: receives the ratios r_i (NaN for a row that refused).
    clip_eps and ratio_out are keyword-only attributes beside the seven tuple fields (which keep their order and their
    number for whoever unpacks a spec); _replace takes them like fields.
    generator     the torch.Generator of a torch buffer's draw; a ring draws from its own seed and device call counter."""
    clip_eps: Optional[float] = None
    ratio_out: Optional[torch.Tensor] = None

    def __new__(cls, *args, clip_eps: Optional[float] = None, ratio_out: Optional[torch.Tensor] = None, **kw):
        self = super().__new__(cls, *args, **kw)
        self.clip_eps, self.ratio_out = clip_eps, ratio_out
        return self

    def _replace(self, **kw):
        clip = {k: kw.pop(k, getattr(self, k)) for k in ("clip_eps", "ratio_out")}
        return type(self)(*super()._replace(**kw), **clip)

    def __repr__(self):
        return f"{super().__repr__()[:-1]}, clip_eps={self.clip_eps!r}, ratio_out={self.ratio_out!r})"


def transitions_from_rollout(obs_in: torch.Tensor, out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The (state, action, reward, next_state) tuples of train.py:176-180 from one rollout's outputs:
    obs_in [B,N,12] is what the policy saw first; out = {obs [T,B,N,12], actions [T,B,N], reward [T,B,N]}.
    A rollout that crossed episode ends (run_actor(auto_reset_seed=..., want_start_obs=True)) also carries done [T,B]
    and start_obs [T,B,N,12]: where done[t-1, b] fired, the state of step t is start_obs[t-1, b] -- the observation of
    the fresh state the environment was reset to -- not the finished episode's last observation obs[t-1, b]."""
    obs = out["obs"]
    states = torch.cat([obs_in.unsqueeze(0), obs[:-1]], dim=0)
    if out.get("done") is not None and out.get("start_obs") is not None and obs.shape[0] > 1:
        fired = out["done"][:-1].bool()[:, :, None, None]
        states[1:] = torch.where(fired, out["start_obs"][:-1], states[1:])
    D = obs.shape[-1]
    return {"states": states.reshape(-1, D), "actions": out["actions"].reshape(-1),
            "rewards": out["reward"].reshape(-1), "next_states": obs.reshape(-1, D)}


class DeviceReplayBuffer:
    """ReplayBuffer (train.py:41-70) as a device ring."""
    priorities = discounts = log_mu = gamma = None     # what a prioritised, an n-step or a behaviour buffer would hold

    def __init__(self, capacity: int, device, obs_dim: int = 12):
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.store = {"states": torch.empty(self.capacity, obs_dim, device=self.device),
                      "actions": torch.empty(self.capacity, dtype=torch.int32, device=self.device),
                      "rewards": torch.empty(self.capacity, device=self.device),
                      "next_states": torch.empty(self.capacity, obs_dim, device=self.device)}
        self.pos = 0          # next slot to write
        self.count = 0        # valid transitions

    def size(self) -> int:
        return self.count

    def _slots(self, n: int) -> Tuple[torch.Tensor, int]:
        """Ring slots for n new transitions (only the last `capacity` of them survive, like deque(maxlen))."""
        skip = max(0, n - self.capacity)
        start = (self.pos + skip) % self.capacity
        idx = (torch.arange(n - skip, device=self.device) + start) % self.capacity
        return idx, skip

    def add(self, transition_dict: Dict[str, torch.Tensor]) -> torch.Tensor:
        """transition_dict: states [n,12], actions [n], rewards [n], next_states [n,12] (any leading shape is
        flattened).  Returns the ring slots written."""
        D = self.store["states"].shape[1]
        n = transition_dict["actions"].numel()
        idx, skip = self._slots(n)
        for k in KEYS:
            src = transition_dict[k].to(self.device)
            src = src.reshape(n, D) if k.endswith("states") else src.reshape(n)
            self.store[k].index_copy_(0, idx, src[skip:].to(self.store[k].dtype))
        self.pos = (self.pos + n) % self.capacity
        self.count = min(self.capacity, self.count + n)
        return idx

    def _draw_batch(self, k: int, spec: DrawSpec = DrawSpec()):
        """(k distinct indices, None): the draw of sample() and of the learner's update_from."""
        return torch.randperm(self.count, device=self.device, generator=spec.generator)[:k], None

    def sample(self, batch_size: int, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        idx, _ = self._draw_batch(min(int(batch_size), self.count), DrawSpec(generator=generator))
        return {key: self.store[key][idx] for key in KEYS}


class PrioritizedDeviceReplayBuffer(DeviceReplayBuffer):
    """PrioritizedReplayBuffer (train.py:73-139) as a device ring."""

    def __init__(self, capacity: int, device, alpha: float = 0.6, obs_dim: int = 12):
        super().__init__(capacity, device, obs_dim)
        self.alpha = float(alpha)
        self.priorities = torch.zeros(self.capacity, device=self.device)

    def add(self, transition_dict: Dict[str, torch.Tensor]) -> torch.Tensor:
        # every transition of the call enters at the maximum priority seen so far (1.0 for an empty buffer);
        # within one reference add() the maximum cannot grow, so one value serves the whole batch
        top = self.priorities.max() if self.count > 0 else torch.ones((), device=self.device)
        idx = super().add(transition_dict)
        self.priorities.index_fill_(0, idx, 0.0)
        self.priorities.index_add_(0, idx, top.expand(idx.numel()))
        return idx

    def _draw_batch(self, k: int, spec: DrawSpec = DrawSpec()):
        """(k indices drawn with replacement from p_i^alpha / sum, their importance weights or None)."""
        prob = self.priorities[:self.count] ** self.alpha
        prob = prob / prob.sum()
        idx = torch.multinomial(prob, k, replacement=True, generator=spec.generator)
        if not spec.importance:
            return idx, None
        if spec.beta_final is not None:
            raise ValueError("beta_final anneals over a PrioritizedReplayRing's device call counter; a "
                             "PrioritizedDeviceReplayBuffer has none: pass this call's beta")
        weights = (self.count * prob[idx]) ** (-spec.beta)
        return idx, weights / weights.max()

    def sample(self, batch_size: int, beta: float = 0.4, generator: Optional[torch.Generator] = None):
        if self.count == 0:
            return {k: self.store[k][:0] for k in KEYS}, None, None
        idx, weights = self._draw_batch(min(int(batch_size), self.count),
                                        DrawSpec(importance=True, beta=beta, generator=generator))
        return {key: self.store[key][idx] for key in KEYS}, idx, weights

    def update_priorities(self, batch_indices: torch.Tensor, batch_priorities: torch.Tensor) -> None:
        self.priorities.index_copy_(0, batch_indices.to(self.device), batch_priorities.to(self.device, torch.float32))
