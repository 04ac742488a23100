"""The reference's two replay buffers (src/train.py:41-139) with their add and their draw in HIP (uavtrack_replay_*):
`ReplayRing` is `ReplayBuffer` (uniform, without replacement), `PrioritizedReplayRing` is `PrioritizedReplayBuffer`.
The ring's stores and priorities are device tensors laid out as in DeviceReplayBuffer, owned here and passed to the
library as pointers; the library handle keeps only scratch and the device-side draw counter.

Against DeviceReplayBuffer (uavtrack/replay.py, which stays the plain-PyTorch reference), ReplayRing:
  - add_rollout writes a rollout's outputs straight into the ring, as below;
  - the draw is O(batch) instead of a shuffle of the whole ring (torch.randperm(count)[:k]): draw j of call c is a keyed
    bijection of j walked below count, keyed by (seed, device call counter), so it allocates nothing and every replay
    of a captured graph draws afresh.  The stream is documented in include/uavtrack.h.

Against PrioritizedDeviceReplayBuffer (uavtrack/replay.py, which stays the plain-PyTorch reference):
  - add_rollout writes a rollout's outputs straight into the ring (no [T*B*N, 12] concatenation, only the last
    `capacity` transitions written), new transitions entering at the device-side maximum priority;
  - the draw has no 2^24-slot limit (torch.multinomial's), keeps its CDF in fp64 as np.random.choice does, and is
    keyed by (seed, device call counter), so every replay of a captured graph draws afresh.  The stream is documented
    in include/uavtrack.h;
  - beta can follow a linear schedule over that same call counter (draw(..., beta_final=, anneal_calls=):
    uavtrack_replay_sample_annealed), formed on the device, so a replayed graph anneals too.

Multi-step targets.  Either ring turned into an n-step ring, ring.with_nstep(n_step, gamma), owns a fifth per-slot store, `discounts`: add_rollout
then folds each transition's next n_step rewards into its reward, takes the next state from the end of that window and
leaves gamma^m in the slot's discount (uavtrack_replay_add_rollout_nstep; the horizon m never crosses an episode end and
is cut at the rollout's last step).  DeviceActorCritic.update_from and its relatives pick the store up, so the target of
a row is r + discount * V(s').  Without with_nstep a ring is exactly what it was.

TD(lambda) targets.  ring.with_lambda(lam, gamma) makes either ring a lambda ring instead: add_rollout(obs_in, out,
critic=learner) (or values=V) walks each agent's chain backwards and stores every transition as the one-step transition
with reward R_t = r_t + gamma lam G_{t+1} and discount gamma (1 - lam) (uavtrack_replay_add_rollout_lambda), so the same
target r + discount * V(s') is the lambda-return: its tail evaluated by the critic at add time, its first bootstrap term
by the critic at update time.  Windows never cross an episode end and are cut at the rollout's last step, where the
transition is the plain one-step one; lam = 0 is with_nstep(1, gamma) to the byte.  Slots keep the tail they were added
with.

Behaviour log-probabilities.  ring.with_behaviour() gives either ring (n-step and lambda rings included) a sixth per-slot
store, `log_mu`: log mu(action[slot] | state[slot]) of the policy that acted, NaN where it is not known.
add_rollout_behaviour(obs_in, out, behaviour=learner) is add_rollout followed, on the same stream, by the learner's actor
over the ring window the add has just written (uavtrack_learner_log_probs_window: it reads the ring's own states and
actions, so one path serves every add form and no add kernel changes).  That is right when the learner's actor at add
time is the one that acted: add before the iteration's updates.  The rollout's actor runs on the f16 matrix cores "at
fp32 accuracy", so mu is the acting distribution to that accuracy, not to the bit.  DeviceActorCritic.update_from(ring,
k, rho_bar=R) turns the store into truncated importance ratios min(R, pi / mu), one weight per batch row; they correct
the first action of a transition only (on an n-step or lambda ring the rest of the window stays uncorrected).
update_from(ring, k, clip_eps=E) reads the same store inside the gradient kernel for PPO's clipped surrogate instead
(uavtrack_learner_update_clipped); a drawn slot that is still NaN refuses that update on the device.  Without
with_behaviour a ring is exactly what it was.

Fixed GAE advantages.  ring.with_gae(lam, gamma) makes either ring a GAE ring instead of an n-step or lambda ring:
add_rollout(obs_in, out, critic=learner) (or add_rollout_gae(values=, values_in=, values_start=)) runs the lambda add's fold and stores,
per slot, the lambda-return G_t itself as the reward, a discount of +0 (so the learner's target r + discount * V(s') is
the fixed value target G_t) and the advantage G_t - V(s_t) in a seventh per-slot store, `advantages`
(uavtrack_replay_add_rollout_gae): GAE(lambda), bootstrapped at the rollout's last step and at a fired done.  NaN means
unknown.  DeviceActorCritic.update_from and its relatives pick the store up from the ring or from a sweep over it
(uavtrack_learner_update_stored): advantage and value target are then constants of the iteration, whatever the
minibatches before have done to the critic.  Composes with with_behaviour().  Without with_gae a ring is exactly what it
was.

On-policy epochs.  ring.sweep(batch_size, window="last") returns a RingSweep over a window of either ring -- by default
the slots the most recent add wrote -- whose consecutive draws are the disjoint minibatches of an epoch, every slot of the
window once per epoch, epoch after epoch in another order (uavtrack_replay_sample_sweep, numbered by a device cursor the
sweep owns; the ring's own call counter is not touched).  The learner's update_from and its relatives take a sweep where
they take a ring.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._handle import Handle, current_device
from ._lib import ptr as _ptr
from .replay import KEYS, DrawSpec

# The per-slot side stores a ring may own: (the ring's attribute, which is also its key in a transitions dict, what add
# fills in where the dict lacks the key; None: float32(the ring's gamma)).
SIDE_STORES = (("discounts", None), ("log_mu", float("nan")), ("advantages", float("nan")))


def _unit_range(name: str, value) -> float:
    value = float(value)
    if not 0.0 <= value <= 1.0:
        raise ValueError(f"{name} must be in [0, 1], got {value}")
    return value


class ReplayRing(Handle):
    """ReplayBuffer(capacity) (train.py:41-70) as a device ring with HIP add and sampling: uniform draws without
    replacement.  Also what PrioritizedReplayRing shares with it: the stores, the adds and the handle."""
    _prefix = "uavtrack_replay_"
    priorities: Optional[torch.Tensor] = None
    discounts: Optional[torch.Tensor] = None
    n_step: int = 1
    gamma: Optional[float] = None
    lam: Optional[float] = None                 # with_lambda: the ring stores lambda-returns
    _values: Optional[torch.Tensor] = None      # add_rollout(critic=...)'s buffer, kept and only grown
    advantages: Optional[torch.Tensor] = None   # with_gae: per-slot fixed advantages, NaN where not known
    gae: bool = False                           # with_gae: lam and gamma are GAE's, the ring stores G_t, +0 and G_t - V(s_t)
    _values_in: Optional[torch.Tensor] = None   # a GAE ring's add_rollout(critic=...): V(obs_in) and V(start_obs), likewise
    _values_start: Optional[torch.Tensor] = None
    log_mu: Optional[torch.Tensor] = None       # with_behaviour: per-slot behaviour log-probabilities
    _w: Optional[torch.Tensor] = None           # a prioritised ring's importance weights of update_from's draws
    _rho_w: Optional[torch.Tensor] = None       # with_behaviour: update_from's ratio weights (a prioritised ring: its _w)
    _last: Optional[Tuple[int, int]] = None     # (first slot, length) of what the most recent add wrote

    def __init__(self, capacity: int, device, seed: int = 0, max_batch: int = 65536, obs_dim: int = _lib.OBS_DIM):
        if obs_dim != _lib.OBS_DIM:
            raise ValueError(f"obs_dim must be {_lib.OBS_DIM}, got {obs_dim}")
        self.capacity = int(capacity)
        self.device = current_device(device)
        self.seed, self.max_batch = int(seed), int(max_batch)
        self.store = {"states": torch.empty(self.capacity, obs_dim, device=self.device),
                      "actions": torch.empty(self.capacity, dtype=torch.int32, device=self.device),
                      "rewards": torch.empty(self.capacity, device=self.device),
                      "next_states": torch.empty(self.capacity, obs_dim, device=self.device)}
        self.pos = 0          # next slot to write
        self.count = 0        # valid transitions
        self._create(_lib.ReplayConfig(device_id=self.device.index, max_capacity=self.capacity, max_batch=self.max_batch,
                                       seed=self.seed & (2**64 - 1)))
        self._idx = torch.empty(self.max_batch, dtype=torch.int64, device=self.device)   # update_from's draws

    def with_nstep(self, n_step: int = 1, gamma: Optional[float] = None) -> "ReplayRing":
        """Makes this ring an n-step ring and returns it: ReplayRing(capacity, device).with_nstep(3, gamma=0.95).  The ring
        then owns `discounts` [capacity] (every slot float32(gamma) to begin with, which is what the one-step transitions
        it may already hold bootstrap with), add_rollout stores n_step-step returns and add fills the discounts.  gamma
        None (then n_step must be 1) leaves the ring exactly what it was: discounts is None."""
        n_step = int(n_step)
        if not 1 <= n_step <= _lib.REPLAY_MAX_NSTEP:
            raise ValueError(f"n_step must be in [1, {_lib.REPLAY_MAX_NSTEP}], got {n_step}")
        if self.gae and n_step > 1:
            raise ValueError(f"with_nstep({n_step}) on a GAE ring: a ring stores n-step returns, lambda-returns or GAE "
                             f"advantages, one of the three")
        if self.lam is not None and n_step > 1:
            raise ValueError(f"with_nstep({n_step}) on a lambda ring: a ring stores n-step returns or lambda-returns")
        if gamma is None:
            if n_step != 1:
                raise ValueError(f"n_step = {n_step} needs gamma (the discount the n-step return is folded with)")
            return self
        self.n_step, self.gamma = n_step, _unit_range("gamma", gamma)
        self.discounts = torch.full((self.capacity,), self.gamma, dtype=torch.float32, device=self.device)
        return self

    def with_lambda(self, lam: float, gamma: float) -> "ReplayRing":
        """Makes this ring a lambda ring and returns it: ReplayRing(capacity, device).with_lambda(0.9, gamma=0.95).  The
        ring then owns `discounts` [capacity] (every slot float32(gamma) to begin with, as with_nstep) and add_rollout
        stores lambda-returns as (reward, discount) pairs, from `values=` or a `critic=`.  n_step stays 1; a ring is an
        n-step ring (n_step > 1) or a lambda ring, not both."""
        lam, gamma = _unit_range("lam", lam), _unit_range("gamma", gamma)
        if self.gae:
            raise ValueError("with_lambda on a GAE ring: a ring stores n-step returns, lambda-returns or GAE advantages, "
                             "one of the three")
        if self.n_step > 1:
            raise ValueError(f"with_lambda on a ring with n_step = {self.n_step}: a ring stores n-step returns or "
                             f"lambda-returns")
        self.lam, self.gamma = lam, gamma
        self.discounts = torch.full((self.capacity,), gamma, dtype=torch.float32, device=self.device)
        return self

    def with_gae(self, lam: float, gamma: float) -> "ReplayRing":
        """Makes this ring a GAE ring and returns it: ReplayRing(capacity, device).with_gae(0.95, gamma=0.99).  The ring
        then owns `advantages` [capacity] float32, every slot NaN ("unknown") to begin with, and `discounts` [capacity]
        (kept if the ring has them already, else every slot float32(gamma), which is what one-step transitions it may
        already hold bootstrap with); add_rollout stores the lambda-return as the reward, +0 as the discount and
        G_t - V(s_t) as the advantage, from `critic=` or from add_rollout_gae's `values=, values_in=, values_start=`.  A ring is an n-step
        ring (n_step > 1), a lambda ring or a GAE ring: with_gae raises after either, and they raise after it.
        Composes with with_behaviour in either order."""
        lam, gamma = _unit_range("lam", lam), _unit_range("gamma", gamma)
        if self.n_step > 1:
            raise ValueError(f"with_gae on a ring with n_step = {self.n_step}: a ring stores n-step returns, lambda-returns "
                             f"or GAE advantages, one of the three")
        if self.lam is not None and not self.gae:
            raise ValueError("with_gae on a lambda ring: a ring stores n-step returns, lambda-returns or GAE advantages, "
                             "one of the three")
        if self.discounts is not None and not self.gae and self.gamma != gamma:
            raise ValueError(f"with_gae(gamma = {gamma}) on a ring whose discounts were made with gamma = {self.gamma}")
        self.gae, self.lam, self.gamma = True, lam, gamma
        if self.discounts is None:
            self.discounts = torch.full((self.capacity,), gamma, dtype=torch.float32, device=self.device)
        if self.advantages is None:
            self.advantages = torch.full((self.capacity,), float("nan"), dtype=torch.float32, device=self.device)
        return self

    def with_behaviour(self) -> "ReplayRing":
        """Gives this ring the behaviour store and returns it: ReplayRing(capacity, device).with_lambda(0.9, 0.95)
        .with_behaviour().  The ring then owns `log_mu` [capacity] float32, every slot NaN ("unknown") to begin with, and
        a [max_batch] float32 buffer for the ratio weights of update_from(..., rho_bar=) (a prioritised ring multiplies
        into its importance-weight buffer instead); add_rollout_behaviour and add fill the store, sample() returns it.
        Composes with with_nstep and with_lambda in either order."""
        if self.log_mu is None:
            self.log_mu = torch.full((self.capacity,), float("nan"), dtype=torch.float32, device=self.device)
            if self._w is None:                            # a prioritised ring's own importance-weight buffer serves
                self._rho_w = torch.empty(self.max_batch, dtype=torch.float32, device=self.device)
        return self

    def _copy_last(self, dst: torch.Tensor, src: torch.Tensor, n: int) -> None:
        """The last min(n, capacity) of src's n elements into dst's slots from pos on, as an add of n rows places them."""
        k = min(n, self.capacity)
        start = (self.pos + n - k) % self.capacity
        head = min(k, self.capacity - start)
        dst[start:start + head] = src[n - k:n - k + head]
        dst[:k - head] = src[n - k + head:]

    def _rollout_values(self, obs: torch.Tensor, critic, values: Optional[torch.Tensor], what: str = "values",
                        of: str = "obs") -> torch.Tensor:
        """The lambda add's values [T*B*N]: the caller's, or the critic's over obs into the ring's own buffer.  A GAE
        ring's values_in (over obs_in) and values_start (over start_obs) likewise, each into a buffer of its own."""
        n = obs.numel() // _lib.OBS_DIM
        if (critic is None) == (values is None):
            raise ValueError(f"add_rollout: a {'GAE' if self.gae else 'lambda'} ring needs exactly one of critic= and "
                             f"{what}=")
        if values is not None:
            return _lib.tensor_arg(values, torch.float32, n, self.device,
                                   f"add_rollout: {what} must be a contiguous float32 tensor of {n} elements (one per "
                                   f"row of {of}) on {self.device}")
        held = getattr(self, "_" + what)
        if held is None or held.numel() < n:
            held = torch.empty(n, dtype=torch.float32, device=self.device)
            setattr(self, "_" + what, held)
        buf = held[:n]
        if isinstance(critic, torch.nn.Module):
            with torch.no_grad():
                buf.copy_(critic(obs.reshape(-1, _lib.OBS_DIM)).reshape(n))
        else:
            critic.values(obs, out=buf)
        return buf

    def _ring(self) -> _lib.ReplayRing:
        s = self.store
        return _lib.ReplayRing(states=s["states"].data_ptr(), actions=s["actions"].data_ptr(),
                               rewards=s["rewards"].data_ptr(), next_states=s["next_states"].data_ptr(),
                               priorities=None if self.priorities is None else self.priorities.data_ptr(),
                               capacity=self.capacity, pos=self.pos, count=self.count)

    def _advance(self, n: int) -> None:
        k = min(n, self.capacity)
        self._last = ((self.pos + n - k) % self.capacity, k)      # what every add path has just written: sweep("last")
        self.pos = (self.pos + n) % self.capacity
        self.count = min(self.capacity, self.count + n)

    def size(self) -> int:
        return self.count

    def check(self) -> None:
        """Synchronises; raises if a draw since the last check was refused on the device (a NaN, infinite or negative
        priority in [0, count), or all of them zero).  A refused draw returned slot 0 and NaN weights.  A uniform draw
        reads no ring data and is never refused."""
        self._check()

    # ---- add (train.py:47-54, 87-96)
    def add(self, transition_dict: Dict[str, torch.Tensor]) -> None:
        """transition_dict: states [n,12], actions [n], rewards [n], next_states [n,12] (any leading shape is
        flattened).  One library call writes the last min(n, capacity) of them (a prioritised ring: at the current
        maximum priority).  A ring with discounts then fills the same slots' discounts from an optional "discounts"
        entry [n], or with float32(gamma) where it is absent (a torch slice copy: the flat add is not the hot path).  A
        behaviour ring fills their log_mu likewise from an optional "log_mu" entry [n], or with NaN ("unknown"), and a GAE
        ring their advantages from an optional "advantages" entry [n], or with NaN; on any other ring that entry raises."""
        n = transition_dict["actions"].numel()
        if n < 1:
            return
        if self.advantages is None and transition_dict.get("advantages") is not None:
            raise ValueError('add: "advantages" is for a GAE ring (ring.with_gae(lam, gamma))')
        dev, D = self.device, _lib.OBS_DIM
        s = transition_dict["states"].to(dev, torch.float32).reshape(n, D).contiguous()
        a = transition_dict["actions"].to(dev, torch.int32).reshape(n).contiguous()
        r = transition_dict["rewards"].to(dev, torch.float32).reshape(n).contiguous()
        s2 = transition_dict["next_states"].to(dev, torch.float32).reshape(n, D).contiguous()
        ring = self._ring()
        _lib.check(self._lib.uavtrack_replay_add(self._h, C.byref(ring), n, _ptr(s), _ptr(a), _ptr(r), _ptr(s2),
                                                 self._stream()), "uavtrack_replay_add")
        for name, fill in SIDE_STORES:
            held, v = getattr(self, name), transition_dict.get(name)
            if held is not None:
                v = torch.full((n,), self.gamma if fill is None else fill, dtype=torch.float32, device=dev) if v is None \
                    else v.to(dev, torch.float32).reshape(n)
                self._copy_last(held, v, n)
        self._advance(n)

    def add_rollout(self, obs_in: torch.Tensor, out: Dict[str, torch.Tensor], *, critic=None,
                    values: Optional[torch.Tensor] = None) -> None:
        """add(transitions_from_rollout(obs_in, out)) in one library call: obs_in [B,N,12] is what the policy saw
        first, out = {obs [T,B,N,12], actions [T,B,N] int32, reward [T,B,N]} (BatchedRollout.run_fused's outputs).  When
        `out` carries start_obs (a rollout across episode ends, with its done [T,B] uint8), the state behind a fired done
        is the fresh state's observation (uavtrack_replay_add_rollout_episodes).  A ring with discounts (with_nstep)
        stores n_step-step returns and their discounts instead (uavtrack_replay_add_rollout_nstep), with or without
        done / start_obs as above; obs must then be [T,B,N,12].  A lambda ring (with_lambda) stores lambda-returns
        (uavtrack_replay_add_rollout_lambda) and needs exactly one of `values` (float32, contiguous, T*B*N elements:
        V(obs[t][b][i])) and `critic` (an object with .values(states, out=), a DeviceActorCritic, or a torch module such
        as ValueMLP, called under no_grad on obs.reshape(-1, 12)); the critic's values go into a buffer the ring keeps
        and only grows.  Any other ring given either raises.  A GAE ring (with_gae) stores G_t, +0 and the advantage
        (uavtrack_replay_add_rollout_gae) and takes `critic`, run over obs_in, over obs and, when the rollout carries it,
        over start_obs, into three such buffers; its explicit form, three value arrays, is add_rollout_gae's.  A
        behaviour ring (with_behaviour) is added to through add_rollout_behaviour, which says who acted; this call
        refuses it."""
        self._add_rollout(obs_in, out, critic, values, None, None)

    def add_rollout_gae(self, obs_in: torch.Tensor, out: Dict[str, torch.Tensor], *, critic=None,
                        values: Optional[torch.Tensor] = None, values_in: Optional[torch.Tensor] = None,
                        values_start: Optional[torch.Tensor] = None, behaviour=None,
                        log_mu: Optional[torch.Tensor] = None) -> None:
        """add_rollout on a GAE ring (with_gae; any other ring raises) with the explicit form spelled out: either
        `critic` (as add_rollout: run over obs_in, obs and start_obs), or all of values= (float32, contiguous, T*B*N
        elements: V(obs[t][b][i])), values_in= (B*N: V(obs_in[b][i])) and, exactly when `out` carries start_obs,
        values_start= (T*B*N: V(start_obs[t][b][i]), read only where done fired).  add_rollout and
        add_rollout_behaviour keep the parameter lists they had, so the three arrays travel through this call alone.
        behaviour=, log_mu=: as add_rollout_behaviour, required on a behaviour ring and refused on any other."""
        if not self.gae:
            raise ValueError("add_rollout_gae: values_in= and values_start= are for a GAE ring (ring.with_gae(lam, gamma))")
        if self.log_mu is None and (behaviour is not None or log_mu is not None):
            raise ValueError("add_rollout_gae: behaviour= and log_mu= are for a behaviour ring (ring.with_behaviour())")
        self._add_rollout(obs_in, out, critic, values, behaviour, log_mu, values_in, values_start, explicit=True)

    def add_rollout_behaviour(self, obs_in: torch.Tensor, out: Dict[str, torch.Tensor], *, behaviour=None,
                              log_mu: Optional[torch.Tensor] = None, critic=None,
                              values: Optional[torch.Tensor] = None) -> None:
        """add_rollout on a behaviour ring (with_behaviour; any other ring raises): the same add, then the behaviour
        log-probabilities of the slots it wrote, from exactly one of
          behaviour=  a DeviceActorCritic (an object with .log_probs_window): after the add's own library call, on the
                      same stream, its actor over the window the add has just written -- the last min(T*B*N, capacity)
                      rows (uavtrack_learner_log_probs_window; the hot path: no torch kernel, capturable).  Right when
                      that actor is the one that acted: add before the iteration's updates.  Or a torch module that
                      returns action probabilities, such as ActorMLP: called under no_grad on the window's states, the
                      logarithm of the taken action's probability gathered in torch (not the hot path);
          log_mu=     float32, contiguous, T*B*N elements in add order, on the ring's device: slice-copied as add copies
                      discounts.
        critic=, values=: as add_rollout."""
        if self.log_mu is None:
            raise ValueError("add_rollout_behaviour: behaviour= and log_mu= are for a behaviour ring (ring.with_behaviour())")
        self._add_rollout(obs_in, out, critic, values, behaviour, log_mu)

    def _add_rollout(self, obs_in, out, critic, values, behaviour, log_mu, values_in=None, values_start=None,
                     explicit=False) -> None:
        if self.log_mu is not None and (behaviour is None) == (log_mu is None):
            raise ValueError("add_rollout: a behaviour ring needs exactly one of behaviour= and log_mu= "
                             "(add_rollout_behaviour)")
        if self.lam is None and (critic is not None or values is not None):
            raise ValueError("add_rollout: critic= and values= are for a lambda ring (ring.with_lambda(lam, gamma))")
        if self.gae and values is not None and not explicit:
            raise ValueError("add_rollout: a GAE ring takes critic= here; the explicit form values=, values_in=, "
                             "values_start= is add_rollout_gae's")
        obs, act, rew = out["obs"], out["actions"], out["reward"]
        so = out.get("start_obs")
        T = obs.shape[0]
        M = obs_in.numel() // _lib.OBS_DIM
        if obs.numel() != T * M * _lib.OBS_DIM or act.numel() != T * M or rew.numel() != T * M:
            raise ValueError(f"add_rollout: obs {tuple(obs.shape)}, actions {tuple(act.shape)}, reward "
                             f"{tuple(rew.shape)} do not match obs_in {tuple(obs_in.shape)}")
        if obs.dtype != torch.float32 or obs_in.dtype != torch.float32 or act.dtype != torch.int32 \
                or rew.dtype != torch.float32:
            raise TypeError("add_rollout: obs_in, obs and reward must be float32, actions int32")
        self._on_ring(obs_in, obs, act, rew)
        episode_ends = (None, None)                  # done, start_obs as the library takes them
        if so is not None:
            done = out.get("done")
            if obs.dim() != 4 or done is None or tuple(done.shape) != tuple(obs.shape[:2]) or done.dtype != torch.uint8 \
                    or tuple(so.shape) != tuple(obs.shape) or so.dtype != torch.float32:
                raise ValueError("add_rollout: with start_obs, obs must be [T,B,N,12], done uint8 [T,B] and start_obs "
                                 "float32 of obs's shape")
            self._on_ring(done, so)
            episode_ends = (done.data_ptr(), so.data_ptr())
        # the form and what its entry point takes behind (handle, ring): lambda, then n-step, then episodes, then plain
        source = (obs_in.data_ptr(), obs.data_ptr(), act.data_ptr(), rew.data_ptr())     # (void * arguments take integers)
        if self.lam is not None or self.discounts is not None:
            if obs.dim() != 4:
                raise ValueError(f"add_rollout: {'an n-step' if self.lam is None else 'a GAE' if self.gae else 'a lambda'} "
                                 f"ring needs obs as [T,B,N,12]")
            args = (self.discounts.data_ptr(), T, obs.shape[1], obs.shape[2], *source, *episode_ends)
            if self.gae:
                name = "uavtrack_replay_add_rollout_gae"
                if so is None and values_start is not None:
                    raise ValueError("add_rollout: values_start= comes with a rollout that carries start_obs")
                v = self._rollout_values(obs, critic, values)
                v_in = self._rollout_values(obs_in, critic, values_in, "values_in", "obs_in")
                v_so = None if so is None else self._rollout_values(so, critic, values_start, "values_start", "start_obs")
                args = (args[0], self.advantages.data_ptr(), *args[1:], _ptr(v), _ptr(v_in), _ptr(v_so), self.lam, self.gamma)
            elif self.lam is not None:
                name = "uavtrack_replay_add_rollout_lambda"
                args += (_ptr(self._rollout_values(obs, critic, values)), self.lam, self.gamma)
            else:
                name, args = "uavtrack_replay_add_rollout_nstep", args + (self.n_step, self.gamma)
        elif so is not None:
            name, args = "uavtrack_replay_add_rollout_episodes", (T, obs.shape[1], obs.shape[2], *source, *episode_ends)
        else:
            name, args = "uavtrack_replay_add_rollout", (T, M, *source)
        n = T * M
        if log_mu is not None:
            _lib.tensor_arg(log_mu, torch.float32, n, self.device,
                            f"add_rollout: log_mu must be a contiguous float32 tensor of {n} elements (one per row of "
                            f"obs, in add order) on {self.device}")
        ring = self._ring()
        _lib.check(getattr(self._lib, name)(self._h, C.byref(ring), *args, self._stream()), name)
        if log_mu is not None:
            self._copy_last(self.log_mu, log_mu.reshape(n), n)
        elif behaviour is not None:
            k = min(n, self.capacity)
            self._window_log_mu(behaviour, (self.pos + n - k) % self.capacity, k)
        self._advance(n)

    def _window_log_mu(self, behaviour, first: int, k: int) -> None:
        """log_mu of the k slots from `first` on (wrapping) from the ring's own states and actions."""
        if not isinstance(behaviour, torch.nn.Module):
            behaviour.log_probs_window(self.store["states"], self.store["actions"], first, k, self.log_mu)
            return
        slots = (first + torch.arange(k, device=self.device)) % self.capacity
        with torch.no_grad():
            p = behaviour(self.store["states"][slots])
            a = self.store["actions"][slots].to(torch.int64).unsqueeze(1)
            self.log_mu[slots] = torch.log(p.gather(1, a).squeeze(1)).clamp_(max=0.0).to(torch.float32)

    def _on_ring(self, *tensors) -> None:
        for t in tensors:
            if t.device != self.device or not t.is_contiguous():
                raise ValueError("add_rollout: every input must be contiguous on the ring's device")

    # ---- sample (train.py:56-58)
    def _draw_uniform(self, k: int, idx: torch.Tensor) -> None:
        ring = self._ring()
        _lib.check(self._lib.uavtrack_replay_sample_uniform(self._h, C.byref(ring), k, _ptr(idx), self._stream()),
                   "uavtrack_replay_sample_uniform")

    def _draw_batch(self, k: int, spec: DrawSpec = DrawSpec()):
        """(k distinct indices in the preallocated index tensor, None): what DeviceActorCritic.update_from uses."""
        idx = self._idx[:k]
        self._draw_uniform(k, idx)
        return idx, None

    def _ratio_out(self, k: int) -> torch.Tensor:
        """Where update_from(..., rho_bar=) leaves the k weights it trains with: a prioritised ring's importance weights
        are multiplied in place, a uniform behaviour ring has the buffer with_behaviour made."""
        return (self._rho_w if self._w is None else self._w)[:k]

    def draw(self, batch_size: int) -> Optional[torch.Tensor]:
        """indices int64 [k], k = min(batch_size, count): distinct slots of [0, count) in random order, as
        random.sample's; None for an empty ring.  No synchronisation."""
        if self.count == 0:
            return None
        idx = torch.empty(min(int(batch_size), self.count), dtype=torch.int64, device=self.device)
        self._draw_uniform(idx.numel(), idx)
        return idx

    def sample(self, batch_size: int) -> Dict[str, torch.Tensor]:
        """ReplayBuffer.sample (as DeviceReplayBuffer.sample returns it): the transitions dict of min(batch_size, count)
        distinct transitions."""
        if self.count == 0:
            return self._gather(slice(0, 0))
        return self._gather(self.draw(batch_size))

    def sweep(self, batch_size: int, window="last") -> "RingSweep":
        """A RingSweep over a window of this ring (either ring): epochs of disjoint minibatches of batch_size slots, every
        slot of the window once per epoch.  window: "last", the slots the most recent add, add_rollout or
        add_rollout_behaviour wrote (the last min(n, capacity) of its n transitions); "all", the valid slots; or a
        (first, length) pair, the slots first, first + 1, ... taken mod capacity.  The sweep stays on the window it was
        made on; a later add does not move it (sweep.rebind does)."""
        return RingSweep(self, batch_size, window)

    def _gather(self, idx) -> Dict[str, torch.Tensor]:
        """The transitions dict at idx: KEYS, "discounts" on a ring that has them, "log_mu" on a behaviour ring and
        "advantages" on a GAE ring."""
        out = {key: self.store[key][idx] for key in KEYS}
        out.update({name: getattr(self, name)[idx] for name, _ in SIDE_STORES if getattr(self, name) is not None})
        return out


class PrioritizedReplayRing(ReplayRing):
    """PrioritizedReplayBuffer(capacity, alpha) (train.py:73-139) as a device ring with HIP add and sampling."""

    def __init__(self, capacity: int, device, alpha: float = 0.6, seed: int = 0, max_batch: int = 65536,
                 obs_dim: int = _lib.OBS_DIM):
        if not alpha > 0:
            raise ValueError(f"alpha must be > 0, got {alpha}")
        super().__init__(capacity, device, seed, max_batch, obs_dim)
        self.alpha = float(alpha)
        self.priorities = torch.zeros(self.capacity, device=self.device)
        self._w = torch.empty(self.max_batch, dtype=torch.float32, device=self.device)   # update_from's importance weights

    # ---- sample (train.py:98-112)
    def _draw(self, k: int, beta: float, idx: torch.Tensor, weights: Optional[torch.Tensor],
              beta_final: Optional[float] = None, anneal_calls: int = 0) -> None:
        ring = self._ring()
        if beta_final is None:
            _lib.check(self._lib.uavtrack_replay_sample(self._h, C.byref(ring), k, self.alpha, float(beta), _ptr(idx),
                                                        _ptr(weights), self._stream()), "uavtrack_replay_sample")
            return
        if int(anneal_calls) < 1:
            raise ValueError(f"beta_final needs anneal_calls >= 1 (the draws the schedule runs over), got {anneal_calls}")
        _lib.check(self._lib.uavtrack_replay_sample_annealed(
            self._h, C.byref(ring), k, self.alpha, float(beta), float(beta_final), int(anneal_calls), _ptr(idx),
            _ptr(weights), self._stream()), "uavtrack_replay_sample_annealed")

    def _draw_batch(self, k: int, spec: DrawSpec = DrawSpec()):
        """(k indices, their importance weights) in the preallocated pair: what DeviceActorCritic.update_from uses.
        Without spec.importance no weights are formed: (indices, None)."""
        idx = self._idx[:k]
        if not spec.importance:
            self._draw(k, 0.0, idx, None)
            return idx, None
        w = self._w[:k]
        self._draw(k, spec.beta, idx, w, spec.beta_final, spec.anneal_calls)
        return idx, w

    def draw(self, batch_size: int, beta: float = 0.4, beta_final: Optional[float] = None,
             anneal_calls: int = 0) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """(indices int64 [k], importance weights fp32 [k]) with k = min(batch_size, count), drawn with replacement
        from P(i) = p_i^alpha / sum_j p_j^alpha; (None, None) for an empty ring.  No synchronisation.  With beta_final,
        draw number c of this ring (its device call counter, which every draw advances) uses
        beta + (beta_final - beta) * min(1, c / anneal_calls), formed on the device."""
        if self.count == 0:
            return None, None
        k = min(int(batch_size), self.count)
        idx = torch.empty(k, dtype=torch.int64, device=self.device)
        w = torch.empty(k, dtype=torch.float32, device=self.device)
        self._draw(k, beta, idx, w, beta_final, anneal_calls)
        return idx, w

    def sample(self, batch_size: int, beta: float = 0.4, beta_final: Optional[float] = None, anneal_calls: int = 0):
        """PrioritizedReplayBuffer.sample: (transitions dict, indices int64, weights), or (empty dict, None, None)
        for an empty ring.  beta_final, anneal_calls: as draw."""
        if self.count == 0:
            return self._gather(slice(0, 0)), None, None
        idx, w = self.draw(batch_size, beta, beta_final, anneal_calls)
        return self._gather(idx), idx, w

    def update_priorities(self, batch_indices: torch.Tensor, batch_priorities: torch.Tensor) -> None:
        """PrioritizedReplayBuffer.update_priorities (train.py:136-138): a repeated index keeps its last value, as the
        reference's sequential loop."""
        idx = batch_indices.to(self.device, torch.int64).reshape(-1)
        val = batch_priorities.to(self.device, torch.float32).reshape(-1)
        srt, perm = torch.sort(idx, stable=True)
        last = torch.ones_like(srt, dtype=torch.bool)
        last[:-1] = srt[1:] != srt[:-1]
        self.priorities.index_copy_(0, srt[last], val[perm[last]])


class RingSweep:
    """On-policy epochs over a window of a ring (ring.sweep(batch_size, window)): call q of the sweep is minibatch
    q % M of epoch q // M, M = W // batch_size, and an epoch's M minibatches are disjoint -- together the whole window
    when batch_size divides W, else all but W % batch_size slots of it, other slots every epoch (a shuffled loader's
    drop_last).  Every epoch is another order.  One library call (uavtrack_replay_sample_sweep; the stream is documented
    in include/uavtrack.h), numbered by a two-word device cursor the sweep owns, so a captured draw replayed E * M times
    performs E epochs.  The ring's own call counter is not touched: its draws are what they are without any sweep.

    Where DeviceActorCritic.update_from, grad_from, update_from_many (a list of sweeps, one per shard) and the group path
    take a buffer they take a sweep: it presents the ring's stores, priorities, discounts, behaviour store and advantages, its count
    is the window's length, and its _draw_batch is the next minibatch.  rho_bar, clip_eps, ratio_out and the n-step and
    lambda discounts compose as on the ring, and a prioritised ring's priorities still receive |td_delta|.  A sweep is
    uniform and has no weights: importance=True and beta_final raise, and so does a batch size other than the sweep's."""

    def __init__(self, ring: ReplayRing, batch_size: int, window="last"):
        self.ring = ring
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= ring.max_batch:
            raise ValueError(f"sweep: batch_size = {batch_size} outside [1, max_batch = {ring.max_batch}]")
        self._window = self._resolve(window)
        self._cursor = torch.zeros(2, dtype=torch.int64, device=ring.device)     # [next call, this call]
        self._idx = torch.empty(self.batch_size, dtype=torch.int64, device=ring.device)   # update_from's draws

    def _resolve(self, window) -> Tuple[int, int]:
        """(first, length) of `window` on the ring as it stands, checked as the library checks it."""
        ring = self.ring
        if isinstance(window, str):
            if window == "last":
                if ring._last is None:
                    raise ValueError('sweep: window="last" before any add: nothing has been written yet')
                first, length = ring._last
            elif window == "all":
                first, length = 0, ring.count
            else:
                raise ValueError(f'sweep: window must be "last", "all" or a (first, length) pair, got {window!r}')
        else:
            try:
                first, length = (int(v) for v in window)
            except (TypeError, ValueError):
                raise ValueError(f'sweep: window must be "last", "all" or a (first, length) pair, got {window!r}') from None
        if length < 1:
            raise ValueError(f"sweep: the window holds {length} slots (an empty ring?)")
        if not 0 <= first < ring.capacity:
            raise ValueError(f"sweep: first = {first} outside [0, capacity = {ring.capacity})")
        if self.batch_size > length:
            raise ValueError(f"sweep: batch_size = {self.batch_size} exceeds the window's {length} slots")
        if length > ring.count or (ring.count < ring.capacity and first + length > ring.count):
            raise ValueError(f"sweep: the window ({first}, {length}) leaves the ring's {ring.count} valid slots "
                             f"(capacity {ring.capacity}; only a full ring's window may wrap)")
        return first, length

    # ---- the window and the cursor
    @property
    def window(self) -> Tuple[int, int]:
        """(first, length): the slots first, first + 1, ... (mod capacity), length of them."""
        return self._window

    @property
    def minibatches(self) -> int:
        """M: minibatches (calls) per epoch, length // batch_size."""
        return self._window[1] // self.batch_size

    def rebind(self, window="last") -> "RingSweep":
        """Pins the sweep to `window` of the ring as it stands now (as ring.sweep takes it) and rewinds the cursor to call
        0.  Stream-ordered and allocation-free: one sweep object serves a training run, rebound after each add.  A
        captured graph keeps the window it was captured with."""
        self._window = self._resolve(window)
        self._cursor.zero_()
        return self

    def seek(self, q: int) -> None:
        """The next call becomes call q (minibatch q % M of epoch q // M): a stream-ordered fill of the cursor."""
        q = int(q)
        if not 0 <= q < 2 ** 63:
            raise ValueError(f"seek: q = {q} outside [0, 2^63)")
        self._cursor[:1].fill_(q)

    def position(self) -> int:
        """The number of the next call.  Synchronises."""
        return int(self._cursor[0].item())

    # ---- drawing
    def _draw_into(self, idx: torch.Tensor) -> None:
        ring = self.ring
        view = ring._ring()
        first, length = self._window
        _lib.check(ring._lib.uavtrack_replay_sample_sweep(ring._h, C.byref(view), first, length, idx.numel(),
                                                          _ptr(self._cursor), _ptr(idx), ring._stream()),
                   "uavtrack_replay_sample_sweep")

    def draw(self) -> torch.Tensor:
        """The next minibatch: indices int64 [batch_size], distinct slots of the window.  No synchronisation."""
        idx = torch.empty(self.batch_size, dtype=torch.int64, device=self.ring.device)
        self._draw_into(idx)
        return idx

    def sample(self) -> Dict[str, torch.Tensor]:
        """The next minibatch's transitions dict, with the keys ring.sample()'s dict has ("discounts" and "log_mu" on a
        ring that has them)."""
        return self.ring._gather(self.draw())

    # ---- what the learner's draw functions read from a buffer
    count = property(lambda self: self._window[1])
    store = property(lambda self: self.ring.store)
    capacity = property(lambda self: self.ring.capacity)
    priorities = property(lambda self: self.ring.priorities)
    gamma = property(lambda self: self.ring.gamma)      # (discounts, log_mu and advantages: behind the class)

    def _ratio_out(self, k: int) -> torch.Tensor:
        return self.ring._ratio_out(k)

    def _draw_batch(self, k: int, spec: DrawSpec = DrawSpec()):
        """(the next minibatch in the preallocated index tensor, None).  Raises, enqueuing nothing, for what a sweep
        does not have."""
        if spec.importance or spec.beta_final is not None:
            raise ValueError("a sweep is a uniform pass over its window and has no importance weights: importance=True and "
                             "beta_final are for a PrioritizedReplayRing's own draw")
        if k != self.batch_size:
            raise ValueError(f"batch_size = {k}: this sweep was made for minibatches of {self.batch_size}")
        self._draw_into(self._idx)
        return self._idx, None


for _name, _ in SIDE_STORES:                            # a sweep presents its ring's side stores under their names
    setattr(RingSweep, _name, property(lambda self, _name=_name: getattr(self.ring, _name)))
