"""The reference's learner `ActorCritic` (src/models/actor_critic.py:115-205) on the device: one `update` is ONE
library call (uavtrack_learner_update) -- both forwards, both backwards and both torch.optim.Adam steps, with the
batch gathered in the kernel from a device replay ring and, for a prioritised ring, the |td_delta| priorities of
train.py:262 written back -- stream-ordered, with no synchronisation and no allocation inside the library.

The actor loss of the reference broadcasts: log_probs is [n, 1], td_delta is [n], so `-log_probs * td_delta` is
[n, n] and actor_loss = mean_i(-log p_i) * mean_j(delta_j).  That is the default here (loss="reference");
loss="per_sample" is mean_i(-log p_i * delta_i), the form examples/train_maac.py's PyTorch learner trains with.

The same update also comes in pieces (uavtrack_learner_grad / _apply / _write_priorities): grad_from leaves a batch's
unscaled sums in a device gradient row, apply adds rows in row order, scales once and steps Adam.  update_from_many
(several rings, one GPU) and update_from(..., group=...) (one ring per rank) are built on them; every participant that
applies the same rows in the same order ends with the same bits, and one row is bit for bit `update`.

What update_from, grad_from, update_from_many and the group path draw and weigh a batch by (importance, beta, beta_final,
anneal_calls, rho_bar, rho_out, generator) is one replay.DrawSpec, documented there; the losses they reach are these.

Importance weights (update(weights=...), DrawSpec.importance) put a prioritised draw's importance-sampling weights
w_i >= 0, one per batch row in batch order, into the losses:
    critic_loss                = mean_i(w_i (V(s_i) - y_i)^2)
    actor_loss, "per_sample"   = mean_i(-w_i log p_i delta_i)
    actor_loss, "reference"    = mean_i(-w_i log p_i) * mean_j(w_j delta_j)    (the pair (i, j) of the broadcast weighs w_i w_j)
Means divide by n, not by sum w; td_delta and the priorities written back stay the unweighted delta and |delta|.  Without
them (the default) every call is bit for bit what it was: the reference's update does not use the weights its sample()
returns.

Regularisation (entropy_coef, max_grad_norm; both off by default, and then every call is bit for bit what it was):
    actor_loss, "per_sample"   = mean_i(w_i (-log p_i delta_i - c H_i)),  H_i = -sum_o p_io log p_io,  c = entropy_coef
and, per network, torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm) on the gradient Adam is about to see:
coef = min(1, max_norm / (norm + 1e-6)), the norm taken in float64 in a fixed order, so a split or data-parallel update
clips by the same bits everywhere and an update that does not clip is bit for bit the unclipped one.  The entropy bonus
exists for loss="per_sample" only (the reference form scales the actor's sums once by -mean(delta) / N, which an entropy
term cannot share); clipping works with both forms and with apply, where the norm is that of the summed rows.  Gradient
rows carry no settings: learners that share an update (ranks, shards) must be given equal ones
(sharding.broadcast_learner copies them).  enable_diagnostics() installs two device buffers, the per-row entropies and
the two gradient norms before clipping; reading them is a torch reduction of the caller's.

Multi-step targets (update(discounts=...), and update_from / grad_from / update_from_many / the group path on an
n-step ring, ring.with_nstep(n_step, gamma)): the target of row i is y_i = r_i + d_i V(s'_i) with d_i the row's slot in the ring's `discounts`
store (gamma^m of its n-step window), gathered in the kernel beside the reward (uavtrack_learner_update_discounted /
_grad_discounted).  Everything behind the target is unchanged.  Without discounts every call is bit for bit what it
was, and a store of float32(gamma) gives the same bits; d_i = 0 means "do not bootstrap".  A discount that is NaN,
negative or above 1 refuses the update on the device like a bad action.

Off-policy correction (update(log_mu=, rho_bar=), DrawSpec.rho_bar on a ring made with_behaviour()): the truncated
importance ratio rho_i = min(R, pi(a_i|s_i) / mu(a_i|s_i)) is one more weight per batch row, formed by
uavtrack_learner_ratio_weights from the ring's per-slot log mu and the actor as it stands, and multiplied into the draw's
importance weights (or 1).  With loss="per_sample" the losses above are then the truncated-importance-sampling policy
gradient and the rho-weighted TD(0) critic, rho a constant of the differentiation: the one-step case of V-trace; n-step and
lambda windows carry no traces.  A row whose log mu holds the bits the actor forms now has rho = 1 exactly, so an on-policy
batch at R >= 1 trains with the unweighted update's bits.  log_probs(states, actions) is the actor alone
(uavtrack_learner_log_probs).

The clipped surrogate (update(log_mu=, clip_eps=), DrawSpec.clip_eps on a ring made with_behaviour(); loss="per_sample"
only): PPO's answer to the same staleness, instead of rho_bar.  With r_i = pi(a_i|s_i) / mu(a_i|s_i), A_i = td_delta_i (a
constant of the differentiation), lo = 1 - eps, hi = 1 + eps in float32:
    actor_loss = mean_i(w_i (-min(r_i A_i, clip(r_i, lo, hi) A_i) - c H_i))
so a row's policy gradient is r_i A_i grad log p_i while r_i <= hi (A_i >= 0) or r_i >= lo (A_i < 0), boundaries included,
and 0 beyond; the critic, td_delta, the priorities, the entropy term and everything else are unchanged.  The ratio is
formed inside the gradient kernel from the logits it already holds (uavtrack_learner_update_clipped / _grad_clipped): no
second forward.  ratio_out receives r_i; the clip fraction and an approximate KL are one torch reduction over it.  A row
whose log mu holds the bits log_probs forms now has r = 1 exactly and trains with the per-sample update's bits.  A drawn
log mu that is NaN or positive, or a ratio that is not finite, refuses the update on the device.  The reference form
scales the actor's sums once by -mean(delta) / N, which a per-row gate cannot share: loss="reference" raises.

The critic alone (values(states), uavtrack_learner_values): V(s) of any number of rows with the parameters as they stand
when the launch runs, bit for bit the V(s) an update forms.  A lambda ring (ring.with_lambda(lam, gamma)) takes it as
add_rollout(..., critic=learner) to fold a rollout's rewards with its values into lambda-returns.

The target critic (set_target(tau=) or set_target(period=), uavtrack_learner_set_target; off by default, and then every
call is bit for bit what it was): a second copy theta- of the critic's 14 H + 1 words from which V(s') alone is formed,
y_i = r_i + d_i V_theta-(s'_i), inside the same gradient kernel.  After every successful update or apply theta- moves by
t <- (1 - tau) t + tau w in float32 (two multiplies and an add, each rounded on its own), or is copied from the critic
whenever the critic's device step count is a multiple of period; a refused update leaves it alone.  grad_from bootstraps
from it and apply runs the sync rule; gradient rows carry no settings, so learners that share an update must hold equal
settings and theta- (sharding.pack_learner_state / unpack_learner_state carry both).  learner.target.values(states) is
V of theta-; state_dict / save carry theta- and the settings while a target is enabled.

Batch-normalised advantages (set_advantage("batch"), or a (mean, inv_std) device tensor; loss="per_sample" only; off by
default, and then every call is bit for bit what it was and enqueues what it enqueued): the advantage of the actor's
terms above becomes A_i = (delta_i - mean) / (std + eps) with the batch's own mean and unbiased standard deviation, found
by a pass of its own ahead of the gradient kernel (float64 sums in a fixed order, include/uavtrack.h); it also chooses
the side of the clip gate.  The critic, td_delta, the priorities and the entropy term are unchanged; importance weights
and truncated ratios multiply afterwards.  Each gradient row of a split update is standardised by its own draw's
statistics, as K independent learners would (the choice importance weights made: each draw is normalised by its own
maximum); learner.advantage_stats holds (mean, inv_std, std) of the last batch.

Stored advantages (update(advantages=), and update_from / grad_from / update_from_many / the group path on a GAE ring,
ring.with_gae(lam, gamma), or a sweep over one; loss="per_sample" only): the actor's advantage of row i is
x_i = advantages[slot_i], gathered in the kernel beside the reward (uavtrack_learner_update_stored / _grad_stored), in
delta_i's place in the logit weight, the actor-loss term and the clip gate; set_advantage applies on top ("batch"
standardises the gathered x_i).  The critic, td_delta and the priorities keep delta_i, and on a GAE ring (reward G_t,
discount 0) delta_i = G_t - V_now(s_i): a fixed value target.  An advantage that is NaN (unknown) or infinite refuses the
update on the device.  Without advantages every call enqueues exactly what it enqueued.

KL early stopping (set_kl_stop(limit), uavtrack_learner_set_kl_stop; loss="per_sample" only; off by default, and then
every call enqueues exactly what it enqueued): every clipped update forms kl = mean_i((r_i - 1) - log r_i) of its own
minibatch from the ratios above, before its step, and steps only while kl <= limit; the first one beyond it sets a latch
on the device and is stopped, with every update behind it, until kl_reset().  The host never reads the estimate, so E
epochs of M minibatches stay E M replays of one captured update.  learner.kl and learner.kl_state are device tensors.
Nothing is claimed about learning curves.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict, namedtuple
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import adam
from ._handle import Handle, current_device
from ._lib import host_ptr, ptr as _ptr
from .adam import flat, from_state_dict, split, to_state_dict
from .replay import DrawSpec
from .rollout import ActorMLP


# One batch as _run_batch, _grad_batch and _launch take it: n rows of a store of `capacity` slots (its dict of states,
# actions, rewards, next_states) through idx (None: rows 0..n-1), the priorities to write back, the weights per batch row, and
# per slot of the store the discounts and the behaviour log-probabilities (read with clip_eps, and by _ratio_weights);
# ratio_out per batch row; per slot of the store again the actor's stored advantages (a GAE ring's).
_Batch = namedtuple("_Batch", "n store capacity idx priorities weights discounts log_mu clip_eps ratio_out advantages",
                    defaults=(None,) * 7)


def num_params(hidden_dim: int, action_dim: int) -> int:
    """Floats of the learner's parameter blob: actor fc1 (12 H + H), fc2 (A H + A), critic fc1 (12 H + H), fc2 (H + 1)."""
    H, A = int(hidden_dim), int(action_dim)
    return 27 * H + A * H + A + 1


def row_floats(hidden_dim: int, action_dim: int) -> int:
    """Words of one gradient row of the split update (include/uavtrack.h): the P gradient sums, four loss sums, n as
    two words, the row's status bits and the layout tag P."""
    return num_params(hidden_dim, action_dim) + _lib.LEARNER_ROW_TAIL


class ValueMLP(torch.nn.Module):
    """Same shape as the reference's critic `FnnValueNet` (actor_critic.py:101-112): Linear(12, H) - ReLU -
    Linear(H, 1), squeezed to [b].  Weights load from its state_dict."""

    def __init__(self, state_dim: int = 12, hidden_dim: int = 128):
        super().__init__()
        self.fc1 = torch.nn.Linear(state_dim, hidden_dim)
        self.fc2 = torch.nn.Linear(hidden_dim, 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc2(torch.relu(self.fc1(x))).squeeze(1)


class DeviceActorCritic(Handle):
    """ActorCritic(state_dim, hidden_dim, action_dim, actor_lr, critic_lr, gamma, device) with the update on the GPU.
    Initial weights are torch.nn.Linear's defaults drawn from torch's global generator, like the reference's."""
    _prefix = "uavtrack_learner_"
    _Batch = _Batch                                                   # for a caller of _corrected / _ratio_weights

    def __init__(self, state_dim: int = 12, hidden_dim: int = 128, action_dim: int = 12, actor_lr: float = 1e-4,
                 critic_lr: float = 5e-4, gamma: float = 0.95, device="cuda:0", loss: str = "reference",
                 max_batch: int = 0, entropy_coef: float = 0.0, max_grad_norm=None):
        if state_dim != _lib.OBS_DIM:
            raise ValueError(f"state_dim must be {_lib.OBS_DIM} (the environment's observation), got {state_dim}")
        if loss not in _lib.LOSS_FORMS:
            raise ValueError(f"loss must be one of {_lib.LOSS_FORMS}, got {loss!r}")
        self.device = current_device(device)
        self.hidden_dim, self.action_dim, self.gamma, self.loss = int(hidden_dim), int(action_dim), float(gamma), loss
        self.actor_lr, self.critic_lr = float(actor_lr), float(critic_lr)
        self._max_batch = int(max_batch)
        # host-side modules: the reference's layouts, default initialisation, and the format of state dicts
        self._actor = ActorMLP(state_dim, self.hidden_dim, self.action_dim)
        self._critic = ValueMLP(state_dim, self.hidden_dim)
        self._create(_lib.LearnerConfig(device_id=self.device.index, hidden=self.hidden_dim, n_actions=self.action_dim,
                                        loss=_lib.LOSS_FORMS.index(loss), pad_=0, max_batch=int(max_batch),
                                        gamma=self.gamma, actor_lr=self.actor_lr, critic_lr=self.critic_lr))
        n = C.c_int64()
        _lib.check(self._lib.uavtrack_learner_num_params(self._h, C.byref(n)), "uavtrack_learner_num_params")
        self.num_params = n.value
        self.row_floats = row_floats(self.hidden_dim, self.action_dim)     # = uavtrack_learner_row_floats
        self._set_params(flat(self._params()))
        self._entropy = self.grad_norm = None
        if entropy_coef != 0.0 or max_grad_norm is not None:
            self.set_regularisation(entropy_coef, max_grad_norm)

    # ---- regularisation and its diagnostics
    def set_regularisation(self, entropy_coef: float = 0.0, max_grad_norm=None) -> None:
        """The entropy bonus c >= 0 (loss="per_sample" only) and the gradient-norm clip: max_grad_norm is one float for
        both networks, an (actor, critic) pair, or None / inf for off (also inside the pair).  Host-side settings that
        hold for every update, grad_from and apply enqueued afterwards; a captured graph keeps the ones it was captured
        with.  A refused call (a NaN or negative value, a norm of 0, an entropy bonus on loss="reference") raises and
        changes nothing."""
        pair = max_grad_norm if isinstance(max_grad_norm, (tuple, list)) else (max_grad_norm, max_grad_norm)
        if len(pair) != 2:
            raise ValueError(f"max_grad_norm must be a float or an (actor, critic) pair, got {max_grad_norm!r}")
        a, c = (float("inf") if x is None else float(x) for x in pair)
        _lib.check(self._lib.uavtrack_learner_set_regularisation(self._h, float(entropy_coef), a, c),
                   "uavtrack_learner_set_regularisation")

    def get_regularisation(self):
        """(entropy_coef, actor_max_norm, critic_max_norm) as last set; inf = no clipping."""
        out = (C.c_double * 3)()
        _lib.check(self._lib.uavtrack_learner_get_regularisation(self._h, out), "uavtrack_learner_get_regularisation")
        return tuple(out)

    def enable_diagnostics(self, max_batch: Optional[int] = None) -> None:
        """Allocates and installs the two diagnostic buffers: per-row entropies for batches of up to max_batch rows
        (default: the learner's max_batch, or 65536) and the two gradient norms.  Afterwards entropy(n) is H_i of the
        last update's or grad_from's first n rows (whatever entropy_coef is) and grad_norm the [2] tensor of the actor's
        and critic's norms before clipping, written by every update or apply that clips (NaN before the first one and
        for a refused one).  Installing them changes no other result; no call synchronises."""
        rows = int(max_batch) if max_batch else (self._max_batch or 65536)
        self._entropy = torch.zeros(rows, device=self.device)
        self.grad_norm = torch.full((2,), float("nan"), device=self.device)
        _lib.check(self._lib.uavtrack_learner_set_diagnostics(self._h, _ptr(self._entropy), rows, _ptr(self.grad_norm)),
                   "uavtrack_learner_set_diagnostics")

    def disable_diagnostics(self) -> None:
        _lib.check(self._lib.uavtrack_learner_set_diagnostics(self._h, None, 0, None), "uavtrack_learner_set_diagnostics")
        self._entropy = self.grad_norm = None

    def entropy(self, n: int) -> torch.Tensor:
        """H_i of the first n rows of the last batch (enable_diagnostics first)."""
        if self._entropy is None:
            raise RuntimeError("entropy: call enable_diagnostics() first")
        return self._entropy[:int(n)]

    # ---- the target critic
    def set_target(self, tau: Optional[float] = None, period: Optional[int] = None) -> None:
        """Bootstrap from a target critic theta-: tau in (0, 1] keeps it by Polyak averaging
        (t <- (1 - tau) t + tau w in float32 after every successful update or apply), period >= 1 copies the critic
        whenever its device step count is a multiple of period; exactly one of the two, or neither to turn it off.
        Enabling hard-copies the current critic (stream-ordered; it allocates once, so not inside a graph capture);
        changing tau, period or the rule while enabled keeps theta-.  Host-side settings like set_regularisation: they
        hold for every update, grad_from and apply enqueued afterwards, and a captured graph keeps the ones it was
        captured with.  Both arguments given, or a bad value, raise ValueError before any library call."""
        if tau is not None and period is not None:
            raise ValueError("set_target: tau (Polyak) or period (periodic copy), not both")
        mode, t, k = _lib.TARGET_OFF, 0.0, 0
        if tau is not None:
            mode, t = _lib.TARGET_POLYAK, float(tau)
            if not 0.0 < t <= 1.0:                                    # NaN fails both comparisons
                raise ValueError(f"set_target: tau = {tau!r} must lie in (0, 1]")
        elif period is not None:
            if isinstance(period, bool) or int(period) != period or int(period) < 1:
                raise ValueError(f"set_target: period = {period!r} must be an integer >= 1")
            mode, k = _lib.TARGET_PERIODIC, int(period)
        _lib.check(self._lib.uavtrack_learner_set_target(self._h, mode, t, k, self._stream()), "uavtrack_learner_set_target")

    def get_target(self) -> dict:
        """{"tau": float or None, "period": int or None} as last set (set_target(**get_target()) sets the same); both
        None while no target is enabled."""
        out = (C.c_double * 3)()
        _lib.check(self._lib.uavtrack_learner_get_target(self._h, out), "uavtrack_learner_get_target")
        mode = int(out[0])
        return {"tau": float(out[1]) if mode == _lib.TARGET_POLYAK else None,
                "period": int(out[2]) if mode == _lib.TARGET_PERIODIC else None}

    def _target_on(self) -> bool:
        return any(v is not None for v in self.get_target().values())

    def sync_target(self) -> None:
        """theta- <- the critic as it stands when the copy runs: stream-ordered, capturable; an error while off."""
        _lib.check(self._lib.uavtrack_learner_sync_target(self._h, self._stream()), "uavtrack_learner_sync_target")

    def _set_target_params(self, flat: np.ndarray) -> None:
        """theta- from a float32 blob of 14 H + 1 words in the critic's torch order; an error while off."""
        flat = np.ascontiguousarray(flat, np.float32)
        _lib.check(self._lib.uavtrack_learner_set_target_params(self._h, host_ptr(flat), flat.size, self._stream()),
                   "uavtrack_learner_set_target_params")

    def _get_target_params(self) -> np.ndarray:
        flat = np.empty(14 * self.hidden_dim + 1, np.float32)
        _lib.check(self._lib.uavtrack_learner_get_target_params(self._h, host_ptr(flat), flat.size, self._stream()),
                   "uavtrack_learner_get_target_params")
        return flat

    def target_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """theta- as FnnValueNet's state_dict (CPU fp32); an error while off."""
        names, params = zip(*self._critic.named_parameters())
        return OrderedDict(zip(names, split(self._get_target_params(), params)))

    @property
    def target(self) -> "_TargetCritic":
        """The target critic as something with .values(states, out=None): what a lambda ring's
        add_rollout(..., critic=learner.target) folds its returns with."""
        return _TargetCritic(self)

    def _restore_target(self, settings: Optional[dict], target_sd: Optional[dict]) -> None:
        """Behind a checkpoint load: the checkpoint's settings where it has them, then theta- from the checkpoint's
        copy, or -- while a target is enabled and the checkpoint has none -- a hard sync to the loaded critic."""
        if settings is not None:
            self.set_target(**settings)
        if not self._target_on():
            return
        if target_sd is None:
            return self.sync_target()
        probe = ValueMLP(_lib.OBS_DIM, self.hidden_dim)
        probe.load_state_dict(target_sd)                              # torch checks keys and shapes
        self._set_target_params(flat(list(probe.parameters())))

    # ---- the normalised advantage
    _advantage = "raw"                                                # "raw", "batch" or the installed [2] tensor
    advantage_stats = None                                            # the [3] tensor, from the first "batch" on

    def set_advantage(self, mode="raw", eps: float = 1e-8) -> None:
        """What multiplies grad log p, gates the clip and enters the actor loss (loss="per_sample" only): "raw", the TD
        error delta_i (the default); "batch", A_i = (delta_i - mean) / (std + eps) over the rows of each batch, formed in
        the library ahead of the gradient kernel (uavtrack_learner_set_advantage; std is torch's unbiased one, so a batch
        needs two rows); or a float32 [2] device tensor (mean, inv_std) that is read when an update runs, for running
        statistics or ones reduced over shards or ranks.  The critic, td_delta and the priorities keep delta_i.  After
        the first "batch", advantage_stats is the float32 [3] device tensor (mean, inv_std, std) of the last batch-mode
        update or grad_from (NaN for a refused one).  A host-side setting like set_regularisation: it holds for every
        update, update_from, grad_from, update_from_many and group update enqueued afterwards, a captured graph keeps
        what it was captured with, each gradient row of a split update is standardised by its own draw's statistics,
        and learners that share an update must hold equal settings (checkpoints and sharding.broadcast_learner do not
        carry it).  The first "batch" allocates, so not inside a graph capture.  The reference loss, a bad eps or a
        tensor of the wrong shape, dtype or device raise ValueError before any library call."""
        if torch.is_tensor(mode):
            if mode.shape != (2,) or mode.dtype != torch.float32 or mode.device != self.device or not mode.is_contiguous():
                raise ValueError(f"set_advantage: a given (mean, inv_std) must be a contiguous float32 tensor [2] on "
                                 f"{self.device}, got {tuple(mode.shape)} {mode.dtype} on {mode.device}")
        elif mode not in ("raw", "batch"):
            raise ValueError(f'set_advantage: mode must be "raw", "batch" or a float32 [2] device tensor, got {mode!r}')
        e = float(eps)
        if not e >= 0.0:                                              # NaN fails the comparison
            raise ValueError(f"set_advantage: eps = {eps!r} must be >= 0")
        if self.loss != "per_sample" and not (isinstance(mode, str) and mode == "raw"):
            raise ValueError('set_advantage: a normalised advantage on a loss="reference" learner: that form scales the '
                             "actor's gradient sums once by -mean(delta) / N, and a standardised advantage has mean 0; "
                             'use loss="per_sample"')
        given = mode if torch.is_tensor(mode) else None
        if given is None and mode == "batch" and self.advantage_stats is None:
            stats = torch.full((3,), float("nan"), device=self.device)
            _lib.check(self._lib.uavtrack_learner_set_advantage_stats(self._h, _ptr(stats)),
                       "uavtrack_learner_set_advantage_stats")
            self.advantage_stats = stats
        code = _lib.ADVANTAGE_GIVEN if given is not None else (_lib.ADVANTAGE_BATCH if mode == "batch" else _lib.ADVANTAGE_RAW)
        _lib.check(self._lib.uavtrack_learner_set_advantage(self._h, code, e, _ptr(given)), "uavtrack_learner_set_advantage")
        self._advantage = mode

    def get_advantage(self):
        """(mode, eps) as last set: mode "raw", "batch" or the installed tensor."""
        mode, eps, given = C.c_int32(), C.c_double(), C.c_void_p()
        _lib.check(self._lib.uavtrack_learner_get_advantage(self._h, C.byref(mode), C.byref(eps), C.byref(given)),
                   "uavtrack_learner_get_advantage")
        return ("raw", "batch", self._advantage)[mode.value], eps.value

    # ---- KL early stopping
    _kl_limit = None                                                  # None while off, else the limit as set
    kl = None                                                         # float32 [1]: the last evaluated minibatch's KL
    kl_state = None                                                   # int32 [2]: (stopped, skipped)

    def set_kl_stop(self, limit: Optional[float]) -> None:
        """PPO's `if approx_kl > limit: break` without the host (uavtrack_learner_set_kl_stop; loss="per_sample" only;
        None turns it off).  While on, every update(..., clip_eps=) and update_from(ring | sweep, K, clip_eps=) forms the
        KL estimate mean_i((r_i - 1) - log r_i) of its own minibatch from the ratios of the policy as it stands
        (float64 sums in the fixed order of include/uavtrack.h, unweighted) into `kl`, and steps only where it does not
        exceed `limit` (compared in float32; inf observes and never stops).  The first update beyond it sets a latch on
        the device and is stopped, and so is every later one, whatever its own KL, until kl_reset(): nothing moves
        (parameters, moments, step counts, the target critic, priorities), the losses are NaN, and check() does not count
        it.  `kl` (float32 [1]) and `kl_state` (int32 [2]: stopped, skipped since the last reset) are device tensors;
        reading them is the caller's own synchronisation, and no call here synchronises.  A ring's draw counter and a
        sweep's cursor are advanced by the draw, so they move under stopped updates too (sweep.rebind() or seek rewind
        as before).  A refused update never sets the latch and leaves kl NaN; an underflowed ratio of 0 gives inf.
        A host-side setting like set_advantage: it holds for every update enqueued afterwards, a captured graph keeps
        the one it was captured with (the latch is device state, so replays obey it), and checkpoints and
        sharding.broadcast_learner do not carry it.  Turning it on allocates, so not inside a graph capture.  While on,
        an update without clip_eps, grad_from, apply, update_from_many and the group path raise: the estimate needs the
        clipped surrogate's ratios, and a gradient row has nowhere to carry a KL sum."""
        if limit is None:
            _lib.check(self._lib.uavtrack_learner_set_kl_stop(self._h, 0, float("inf"), None, None),
                       "uavtrack_learner_set_kl_stop")
            self._kl_limit = self.kl = self.kl_state = None
            return
        lim = float(limit)
        if not lim >= 0.0:                                            # NaN fails the comparison
            raise ValueError(f"set_kl_stop: limit = {limit!r} must be >= 0 (inf observes and never stops)")
        if self.loss != "per_sample":
            raise ValueError('set_kl_stop on a loss="reference" learner: the estimate is formed from the clipped '
                             'surrogate\'s ratios, which that form does not have; use loss="per_sample"')
        kl = torch.full((1,), float("nan"), device=self.device)
        state = torch.zeros(2, dtype=torch.int32, device=self.device)
        _lib.check(self._lib.uavtrack_learner_set_kl_stop(self._h, 1, lim, _ptr(kl), _ptr(state)),
                   "uavtrack_learner_set_kl_stop")
        self._kl_limit, self.kl, self.kl_state = lim, kl, state

    def get_kl_stop(self) -> Optional[float]:
        """The limit as last set, or None while off."""
        on, limit, kl, state = C.c_int32(), C.c_double(), C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.uavtrack_learner_get_kl_stop(self._h, C.byref(on), C.byref(limit), C.byref(kl), C.byref(state)),
                   "uavtrack_learner_get_kl_stop")
        return limit.value if on.value else None

    def kl_reset(self) -> None:
        """kl_state <- (0, 0): stream-ordered, capturable (uavtrack_learner_kl_reset); an error while off."""
        if self._kl_limit is None:
            raise RuntimeError("kl_reset: KL early stopping is off (set_kl_stop)")
        _lib.check(self._lib.uavtrack_learner_kl_reset(self._h, self._stream()), "uavtrack_learner_kl_reset")

    def _kl_refuses_split(self, what: str) -> None:
        """Raises while KL early stopping is on: `what` is a piece of the split update."""
        if self._kl_limit is not None:
            raise ValueError(f"{what} while KL early stopping is on (set_kl_stop): a gradient row has nowhere to carry a KL "
                             f"sum, so the split update is refused; use update or update_from with clip_eps, or "
                             f"set_kl_stop(None)")

    def _kl_refuses_unclipped(self, what: str, clip_eps) -> None:
        """Raises while KL early stopping is on and `what`, a closed update, comes without clip_eps."""
        if self._kl_limit is not None and clip_eps is None:
            raise ValueError(f"{what} without clip_eps while KL early stopping is on (set_kl_stop): the estimate is formed "
                             f"from the clipped surrogate's ratios; pass clip_eps (inf never clips), or set_kl_stop(None)")

    def _params(self):
        return list(self._actor.parameters()) + list(self._critic.parameters())

    def _set_params(self, flat: np.ndarray) -> None:
        _lib.check(self._lib.uavtrack_learner_set_params(self._h, host_ptr(flat), flat.size,
                                                         self._stream()), "uavtrack_learner_set_params")

    def _get_params(self) -> np.ndarray:
        flat = np.empty(self.num_params, np.float32)
        _lib.check(self._lib.uavtrack_learner_get_params(self._h, host_ptr(flat), flat.size,
                                                         self._stream()), "uavtrack_learner_get_params")
        return flat

    def reserve(self, max_batch: int) -> None:
        """Scratch for batches of up to max_batch rows (an update beyond the reserved size is an error)."""
        _lib.check(self._lib.uavtrack_learner_reserve(self._h, int(max_batch)), "uavtrack_learner_reserve")

    def check(self) -> None:
        """Synchronises; raises if an update since the last check was refused on the device (an action outside
        [0, action_dim), an index outside the ring, an importance weight that is NaN, infinite or negative -- what a
        refused ring draw hands out --, a discount that is NaN or outside [0, 1], or, under the clipped surrogate, a
        behaviour log-probability that is NaN or positive or a ratio that is not finite, or, under a normalised
        advantage, a mean that is not finite or an inv_std that is NaN, infinite or negative, or a stored advantage that
        is NaN or infinite), which then changed nothing."""
        self._check()

    # ---- the critic alone, the actor alone, and the argument checks they share
    def _rows_arg(self, what: str, states: torch.Tensor) -> int:
        """The row count of states [..., 12]: float32, contiguous, on the learner's device."""
        D = _lib.OBS_DIM
        if states.dim() < 1 or states.shape[-1] != D or states.dtype != torch.float32 or not states.is_contiguous() \
                or states.device != self.device:
            raise ValueError(f"{what}: states must be a contiguous float32 tensor [..., {D}] on {self.device}, got "
                             f"{tuple(states.shape)} {states.dtype} on {states.device}")
        return states.numel() // D

    def _actions_arg(self, what: str, actions: torch.Tensor, n: int) -> None:
        _lib.tensor_arg(actions, torch.int32, n, self.device,
                        f"{what}: actions must be a contiguous int32 tensor of {n} elements on {self.device}")

    def _out_arg(self, what: str, out: Optional[torch.Tensor], states: torch.Tensor, n: int) -> torch.Tensor:
        """`out`, or a new float32 tensor of states' leading shape."""
        if out is None:
            out = torch.empty(tuple(states.shape[:-1]), dtype=torch.float32, device=self.device)
        return _lib.tensor_arg(out, torch.float32, n, self.device,
                               f"{what}: out must be a contiguous float32 tensor of {n} elements on {self.device}")

    def values(self, states: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """V(s) of states [..., 12] (float32, contiguous, on the learner's device) with the critic's parameters as they
        stand when the launch runs (uavtrack_learner_values): a float32 tensor of the leading shape, bit for bit the V(s)
        an update with the same parameters forms.  `out` (float32, contiguous, that many elements, same device) is
        written in place and returned.  No synchronisation, no limit from max_batch, no change to the learner."""
        return self._values("uavtrack_learner_values", states, out)

    def _values(self, entry: str, states: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        """values() through uavtrack_learner_values or, for the target critic, uavtrack_learner_values_target."""
        n = self._rows_arg("values", states)
        out = self._out_arg("values", out, states, n)
        if n:
            _lib.check(getattr(self._lib, entry)(self._h, n, _ptr(states), _ptr(out), self._stream()), entry)
        return out

    def log_probs(self, states: torch.Tensor, actions: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """log pi(a | s) of states [..., 12] (float32) and actions [...] (int32), both contiguous on the learner's
        device, with the actor's parameters as they stand when the launch runs (uavtrack_learner_log_probs): a float32
        tensor of the leading shape, NaN where an action lies outside [0, action_dim).  The bits of a row do not depend
        on how many rows travel with it.  `out` (float32, contiguous, that many elements, same device) is written in
        place and returned.  No synchronisation, no limit from max_batch, no change to the learner."""
        n = self._rows_arg("log_probs", states)
        self._actions_arg("log_probs", actions, n)
        out = self._out_arg("log_probs", out, states, n)
        if n:
            _lib.check(self._lib.uavtrack_learner_log_probs(self._h, n, _ptr(states), _ptr(actions), n, None, _ptr(out),
                                                            self._stream()), "uavtrack_learner_log_probs")
        return out

    def log_probs_window(self, states: torch.Tensor, actions: torch.Tensor, first: int, n: int,
                         log_mu: torch.Tensor) -> None:
        """log pi(actions[slot] | states[slot]) into log_mu[slot] for the n slots (first + k) % capacity of a ring's
        stores (uavtrack_learner_log_probs_window): what a behaviour ring runs behind an add."""
        capacity = self._rows_arg("log_probs_window", states)
        self._actions_arg("log_probs_window", actions, capacity)
        _lib.tensor_arg(log_mu, torch.float32, capacity, self.device,
                        f"log_probs_window: log_mu must be a contiguous float32 tensor of {capacity} elements on {self.device}")
        _lib.check(self._lib.uavtrack_learner_log_probs_window(self._h, _ptr(states), _ptr(actions), capacity, int(first),
                                                               int(n), _ptr(log_mu), self._stream()),
                   "uavtrack_learner_log_probs_window")

    def _ratio_weights(self, b: _Batch, rho_bar: float, w_out: torch.Tensor,
                       rho_out: Optional[torch.Tensor]) -> torch.Tensor:
        """uavtrack_learner_ratio_weights: w_out[i] = (b.weights[i] or 1) * min(rho_bar, pi / mu of batch row i)."""
        n, store, capacity, idx, _, w_in, _, log_mu = b[:8]
        _lib.tensor_arg(log_mu, torch.float32, capacity, self.device,
                        f"log_mu must be a contiguous float32 tensor of {capacity} elements (one per slot of the store) on "
                        f"{self.device}")
        _lib.tensor_arg(rho_out, torch.float32, n, self.device,
                        f"rho_out must be a contiguous float32 tensor of {n} elements (one per batch row) on {self.device}")
        _lib.check(self._lib.uavtrack_learner_ratio_weights(
            self._h, n, _ptr(store["states"]), _ptr(store["actions"]), _ptr(log_mu), capacity, _ptr(idx), float(rho_bar),
            _ptr(w_in), _ptr(w_out), _ptr(rho_out), self._stream()), "uavtrack_learner_ratio_weights")
        return w_out

    _NEEDS_BEHAVIOUR = "needs the buffer's behaviour log-probabilities: a ReplayRing or PrioritizedReplayRing made " \
                       "ring.with_behaviour()"

    def _corrected(self, b: _Batch, rho_bar: Optional[float], rho_out: Optional[torch.Tensor], w_out, who: str = "") -> _Batch:
        """The batch as it trains under its correction for who acted.  b arrives with the behaviour log-probabilities at
        hand (a ring's per-slot store, update()'s argument, or None) and the weights as drawn; it leaves with w (or 1)
        times the truncated ratios into w_out(n) for weights under rho_bar (log_mu stays; _launch reads it under clip_eps
        alone).  `who` is "update: " for update(), whose log_mu is an argument of its own and comes with exactly one of
        the two."""
        log_mu, clip_eps, ratio_out = b[7:10]
        if rho_bar is None and rho_out is not None:
            raise ValueError("rho_out needs rho_bar")
        if rho_bar is not None and clip_eps is not None:
            raise ValueError(f"{who}clip_eps together with rho_bar: one correction for who acted, not two")
        if who and (log_mu is None) != (rho_bar is None and clip_eps is None):
            raise ValueError("update: log_mu and rho_bar come together (log_mu comes with exactly one of rho_bar and "
                             "clip_eps)")
        if rho_bar is not None and log_mu is None:
            raise ValueError(f"rho_bar {self._NEEDS_BEHAVIOUR}")
        if clip_eps is not None:
            self._clip_eps_arg(clip_eps)
            if log_mu is None:
                raise ValueError(f"clip_eps {self._NEEDS_BEHAVIOUR}")
            return b
        if ratio_out is not None:
            raise ValueError(f"{who}ratio_out needs clip_eps")
        if rho_bar is None:
            return b
        return _Batch._make((*b[:5], self._ratio_weights(b, rho_bar, w_out(b.n), rho_out), *b[6:]))   # (_replace: 1 us)

    # ---- the update
    @staticmethod
    def _batch_args(store: Dict[str, torch.Tensor], capacity: int, idx: Optional[torch.Tensor]):
        """A batch as uavtrack_learner_update and _grad take it: the store's four arrays, its capacity, the indices."""
        return (*(_ptr(store[k]) for k in ("states", "actions", "rewards", "next_states")), capacity, _ptr(idx))

    def _drawn_batch(self, buffer, batch_size: int, spec: DrawSpec, caller: str) -> _Batch:
        """min(batch_size, buffer.count) rows drawn as the buffer's own sample() draws them (_draw_batch), the weights
        they train with, and the buffer's per-slot discounts, which must have been folded with this learner's gamma."""
        k = min(int(batch_size), buffer.count)
        if k < 1:
            raise ValueError(f"{caller}: the buffer is empty")
        idx, w = buffer._draw_batch(k, spec)
        b = self._corrected(_Batch(k, buffer.store, buffer.capacity, idx, buffer.priorities, w, buffer.discounts,
                                   getattr(buffer, "log_mu", None),   # an object that is no buffer gets the same answer
                                   spec.clip_eps, spec.ratio_out, getattr(buffer, "advantages", None)),
                            spec.rho_bar, spec.rho_out, getattr(buffer, "_ratio_out", None))
        if b.discounts is not None and np.float32(buffer.gamma) != np.float32(self.gamma):
            raise ValueError(f"the buffer's returns were folded with gamma = {buffer.gamma}, the learner bootstraps with "
                             f"gamma = {self.gamma}: both must be the same float32")
        return b

    def _clip_eps_arg(self, clip_eps) -> float:
        """clip_eps as the library takes it: >= 0, inf allowed, on a per-sample learner."""
        if self.loss != "per_sample":
            raise ValueError('clip_eps on a loss="reference" learner: that form scales the actor\'s gradient sums once by '
                             '-mean(delta) / N, a factor a per-row gate cannot share; use loss="per_sample"')
        eps = float(clip_eps)
        if not eps >= 0.0:                                            # NaN fails the comparison
            raise ValueError(f"clip_eps = {clip_eps!r} must be >= 0 (inf never clips)")
        return eps

    def _launch(self, kind: str, b: _Batch, *outputs) -> None:
        """uavtrack_learner_<kind> ("update" or "grad") in the form the batch takes: plain, _weighted (weights, one per
        batch row), _discounted (weights or NULL, then discounts, one per slot of the store) or, with clip_eps,
        _clipped (weights or NULL, discounts or NULL, log_mu per slot, eps, ratios or NULL) or, with advantages,
        _stored (_clipped's with advantages per slot behind the discounts, log_mu NULL without clip_eps); then the
        outputs."""
        n, store, capacity, idx, _, weights, discounts, log_mu, clip_eps, ratio_out, advantages = b
        if kind == "grad":
            self._kl_refuses_split("uavtrack_learner_grad")
        self._kl_refuses_unclipped("uavtrack_learner_update", clip_eps)
        if isinstance(self._advantage, str) and self._advantage == "batch" and n < 2:
            raise ValueError(f'n = {n} row under set_advantage("batch"): the standard deviation of a batch needs two rows')
        w = _lib.tensor_arg(weights, torch.float32, n, self.device,
                            f"weights must be a contiguous float32 tensor of {n} elements (one per batch row, in batch "
                            f"order) on {self.device}")
        d = _lib.tensor_arg(discounts, torch.float32, capacity, self.device,
                            f"discounts must be a contiguous float32 tensor of {capacity} elements (one per slot of the "
                            f"store) on {self.device}")
        clip = (None, 0.0, None)                                      # what _stored takes where there is no clip_eps
        if clip_eps is not None:
            _lib.tensor_arg(log_mu, torch.float32, capacity, self.device,
                            f"log_mu must be a contiguous float32 tensor of {capacity} elements (one per slot of the "
                            f"store) on {self.device}")
            _lib.tensor_arg(ratio_out, torch.float32, n, self.device,
                            f"ratio_out must be a contiguous float32 tensor of {n} elements (one per batch row) on "
                            f"{self.device}")
            clip = (_ptr(log_mu), self._clip_eps_arg(clip_eps), _ptr(ratio_out))
        if advantages is not None:
            if self.loss != "per_sample":
                raise ValueError('advantages on a loss="reference" learner: that form scales the actor\'s gradient sums once '
                                 'by -mean(delta) / N, a factor a per-row advantage cannot share; use loss="per_sample"')
            _lib.tensor_arg(advantages, torch.float32, capacity, self.device,
                            f"advantages must be a contiguous float32 tensor of {capacity} elements (one per slot of the "
                            f"store) on {self.device}")
        suffix, extra = ("_stored", (_ptr(w), _ptr(d), _ptr(advantages), *clip)) if advantages is not None else \
            ("_clipped", (_ptr(w), _ptr(d), *clip)) if clip_eps is not None else \
            ("_discounted", (_ptr(w), _ptr(d))) if d is not None else \
            ("_weighted", (_ptr(w),)) if w is not None else ("", ())
        name = f"uavtrack_learner_{kind}{suffix}"
        _lib.check(getattr(self._lib, name)(self._h, n, *self._batch_args(store, capacity, idx), *extra,
                                            *map(_ptr, outputs), self._stream()), name)

    def _run_batch(self, b: _Batch):
        losses = torch.empty(2, device=self.device)
        td = torch.empty(b.n, device=self.device)
        self._launch("update", b, losses[0:1], losses[1:2], td, b.priorities)
        return losses[0], losses[1], td

    def _run(self, *batch):
        """_run_batch of a batch spelled out in _Batch's order, for a caller that holds no record (tests, tools)."""
        return self._run_batch(_Batch(*batch))

    def update(self, transition_dict: Dict[str, torch.Tensor], weights: Optional[torch.Tensor] = None,
               discounts: Optional[torch.Tensor] = None, log_mu: Optional[torch.Tensor] = None,
               rho_bar: Optional[float] = None, clip_eps: Optional[float] = None,
               ratio_out: Optional[torch.Tensor] = None, advantages: Optional[torch.Tensor] = None):
        """ActorCritic.update (actor_critic.py:150-179) on a batch {states [n,12], actions [n], rewards [n],
        next_states [n,12]}: returns (actor_loss, critic_loss, td_delta) as device tensors, without synchronising.
        weights [n] (optional): importance weights w_i >= 0, one per row (the module docstring has the weighted losses);
        None is the reference's unweighted update, and a vector of ones gives its bits.
        discounts [n] (optional): d_i in [0, 1] of row i, in batch order (row i is slot i here): the target becomes
        r_i + d_i V(s'_i); None is gamma for every row, and a vector of float32(gamma) gives its bits.
        log_mu [n], the behaviour log-probability of each row's action, comes with exactly one of rho_bar and clip_eps.
        rho_bar > 0: the row's weight becomes w_i min(rho_bar, pi / mu) (uavtrack_learner_ratio_weights, then the
        weighted update).  clip_eps >= 0 (loss="per_sample"): the clipped surrogate of the module docstring
        (uavtrack_learner_update_clipped), ratio_out [n] (optional) receiving the ratios.  Either way a NaN or positive
        log_mu refuses the update on the device.
        advantages [n] (optional, loss="per_sample"): the actor's advantage of each row, per slot of the store like
        discounts (row i is slot i here), in td_delta's place wherever the actor uses one, the advantage mode applied on
        top (uavtrack_learner_update_stored); the critic, td_delta and the priorities keep td_delta.  One that is NaN or
        infinite refuses the update on the device."""
        self._kl_refuses_unclipped("update", clip_eps)
        dev = self.device
        s = torch.as_tensor(transition_dict["states"], device=dev, dtype=torch.float32).reshape(-1, _lib.OBS_DIM).contiguous()
        n = s.shape[0]
        store = {"states": s,
                 "actions": torch.as_tensor(transition_dict["actions"], device=dev).reshape(n).to(torch.int32).contiguous(),
                 "rewards": torch.as_tensor(transition_dict["rewards"], device=dev, dtype=torch.float32).reshape(n).contiguous(),
                 "next_states": torch.as_tensor(transition_dict["next_states"], device=dev,
                                                dtype=torch.float32).reshape(n, _lib.OBS_DIM).contiguous()}
        if weights is not None:
            weights = torch.as_tensor(weights, device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if discounts is not None:
            discounts = torch.as_tensor(discounts, device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if log_mu is not None:
            log_mu = torch.as_tensor(log_mu, device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if advantages is not None:
            advantages = torch.as_tensor(advantages, device=dev, dtype=torch.float32).reshape(-1).contiguous()
        return self._run_batch(self._corrected(_Batch(n, store, n, None, None, weights, discounts, log_mu, clip_eps, ratio_out,
                                                      advantages),
                                               rho_bar, None, lambda n: torch.empty(n, device=dev), "update: "))

    def update_from(self, buffer, batch_size: int, beta: float = 0.4,
                    generator: Optional[torch.Generator] = None, group=None, importance: bool = False,
                    beta_final: Optional[float] = None, anneal_calls: int = 0, rho_bar: Optional[float] = None,
                    rho_out: Optional[torch.Tensor] = None, clip_eps: Optional[float] = None,
                    ratio_out: Optional[torch.Tensor] = None):
        """buffer.sample(batch_size) + update + (prioritised buffer) update_priorities(indices, |td_delta|)
        (train.py:253-262), the gather and the priority write inside the library call.  The indices are drawn as
        the buffer's own sample() draws them.  For a ReplayRing or a PrioritizedReplayRing the draw is one library call
        of its own, so the whole update is two library calls (three with rho_bar) with no torch kernel between them,
        and can be captured into a graph.  beta, generator, importance, beta_final, anneal_calls, rho_bar, rho_out,
        clip_eps, ratio_out: the fields of replay.DrawSpec, documented there; the defaults are the reference's update.

        An n-step ring (ring.with_nstep(n_step, gamma)) brings its per-slot discounts: the target is then
        r + discounts[slot] * V(s'), gathered in the same library call.  Its gamma must be this learner's (as float32).

        A GAE ring (ring.with_gae(lam, gamma)), or a sweep over one, brings its per-slot advantages as well: the actor
        then trains on advantages[slot] (uavtrack_learner_update_stored) and the critic on the ring's fixed value
        targets, whatever earlier minibatches have done to the critic.  loss="per_sample" only.

        With a torch.distributed `group`, every rank of it takes ONE common update from all ranks' batches: the
        gradient row of this rank's batch (grad_from), an all-gather of the rows in rank order
        (sharding.gather_learner_rows), the apply of all of them, and the priority write into this rank's buffer.
        Ranks that start equal (sharding.broadcast_learner) stay bitwise equal; batch sizes may differ between ranks.
        The returned losses are the global ones, td_delta this rank's."""
        if group is not None:
            self._kl_refuses_split("update_from(group=)")
        self._kl_refuses_unclipped("update_from", clip_eps)
        spec = DrawSpec(importance=importance, beta=beta, beta_final=beta_final, anneal_calls=anneal_calls,
                        rho_bar=rho_bar, rho_out=rho_out, generator=generator, clip_eps=clip_eps, ratio_out=ratio_out)
        if group is None:
            return self._run_batch(self._drawn_batch(buffer, batch_size, spec, "update_from"))
        from .sharding import gather_learner_rows
        al, cl, (td,) = self._update_split([buffer], batch_size, [spec], lambda rows: gather_learner_rows(rows, group))
        return al, cl, td

    # ---- the split update: gradient rows and an ordered apply
    def new_rows(self, count: int) -> torch.Tensor:
        """A [count, row_floats] device tensor for `count` gradient rows (pass rows[k] to grad_from as `row`)."""
        return torch.empty(int(count), self.row_floats, device=self.device)

    def _grad_batch(self, b: _Batch, row: Optional[torch.Tensor] = None, td: Optional[torch.Tensor] = None):
        if row is None:
            row = torch.empty(self.row_floats, device=self.device)
        _lib.tensor_arg(row, torch.float32, self.row_floats, self.device,
                        f"row must be a contiguous float32 tensor of {self.row_floats} words on {self.device}")
        if td is None:
            td = torch.empty(b.n, device=self.device)
        self._launch("grad", b, td, row)
        return row, td

    def _grad(self, n, store, capacity, idx, row=None, td=None, *rest):
        """_grad_batch of a batch spelled out: rest is _Batch's fields from weights on."""
        return self._grad_batch(_Batch(n, store, capacity, idx, None, *rest), row, td)

    def grad_from(self, buffer, batch_size: int, row: Optional[torch.Tensor] = None,
                  generator: Optional[torch.Generator] = None, importance: bool = False, beta: float = 0.4,
                  beta_final: Optional[float] = None, anneal_calls: int = 0, rho_bar: Optional[float] = None,
                  rho_out: Optional[torch.Tensor] = None, clip_eps: Optional[float] = None,
                  ratio_out: Optional[torch.Tensor] = None):
        """The gradient half of update_from: draws min(batch_size, buffer.count) rows as update_from does (for a
        ReplayRing or PrioritizedReplayRing the ring's own library call) and leaves their unscaled gradient and loss sums
        in `row` (a new tensor if None).  Returns (row, td_delta, indices); changes nothing in the learner.  The indices
        of either ring live in the ring's own draw tensor until its next draw: call write_priorities (or clone
        them) before drawing from the same ring again.  The other arguments are the fields of replay.DrawSpec; the
        row's sums carry the weights it describes."""
        self._kl_refuses_split("grad_from")
        return self._grad_drawn(buffer, batch_size, DrawSpec(
            importance=importance, beta=beta, beta_final=beta_final, anneal_calls=anneal_calls, rho_bar=rho_bar,
            rho_out=rho_out, generator=generator, clip_eps=clip_eps, ratio_out=ratio_out), row)

    def _grad_drawn(self, buffer, batch_size: int, spec: DrawSpec, row: Optional[torch.Tensor]):
        b = self._drawn_batch(buffer, batch_size, spec, "grad_from")
        row, td = self._grad_batch(b, row)
        return row, td, b.idx

    def apply(self, rows):
        """One update from gradient rows ([count, row_floats], or a sequence of rows): the sums added in row order, one
        global scale, both Adam steps.  Returns (actor_loss, critic_loss) as device tensors, without synchronising.  A
        row that carries a refusal (or another learner's layout) refuses the whole update, on every participant."""
        self._kl_refuses_split("apply")
        if not torch.is_tensor(rows):
            rows = torch.stack([r.reshape(-1) for r in rows])
        rows = rows.reshape(-1, rows.shape[-1])
        if rows.shape[1] != self.row_floats or rows.dtype != torch.float32 or rows.device != self.device:
            raise ValueError(f"rows must be float32 [count, {self.row_floats}] on {self.device}, got "
                             f"{tuple(rows.shape)} {rows.dtype} on {rows.device}")
        rows = rows.contiguous()
        losses = torch.empty(2, device=self.device)
        _lib.check(self._lib.uavtrack_learner_apply(self._h, _ptr(rows), rows.shape[0], _ptr(losses[0:1]),
                                                    _ptr(losses[1:2]), self._stream()), "uavtrack_learner_apply")
        return losses[0], losses[1]

    def write_priorities(self, buffer, idx: Optional[torch.Tensor], td: torch.Tensor) -> None:
        """|td| into a prioritised buffer's priorities at idx (the last occurrence of a repeated slot winning), unless
        the most recent apply on this learner was refused.  A buffer without priorities is left alone."""
        if buffer.priorities is not None:
            _lib.check(self._lib.uavtrack_learner_write_priorities(self._h, td.numel(), _ptr(idx), buffer.capacity,
                                                                   _ptr(td), _ptr(buffer.priorities), self._stream()),
                       "uavtrack_learner_write_priorities")

    def update_from_many(self, buffers, batch_size: int, generator: Optional[torch.Generator] = None,
                         importance: bool = False, beta: float = 0.4, beta_final: Optional[float] = None,
                         anneal_calls: int = 0, rho_bar: Optional[float] = None, rho_out=None,
                         clip_eps: Optional[float] = None, ratio_out=None):
        """ONE update from several buffers on this device (the shards of one GPU): one gradient row per buffer from
        min(batch_size, its count) of its rows, the rows applied in list order, each prioritised buffer's priorities
        written back from its own draw.  Returns (actor_loss, critic_loss, [td_delta per buffer]).  The other arguments
        are the fields of replay.DrawSpec, one spec for every buffer (each draw's weights normalised by its own maximum,
        with rho_bar or clip_eps every buffer a behaviour ring), except rho_out and ratio_out: each a sequence of one
        float32 [k] tensor (or None) per buffer."""
        self._kl_refuses_split("update_from_many")
        buffers = list(buffers)
        if not 1 <= len(buffers) <= _lib.LEARNER_MAX_ROWS:
            raise ValueError(f"update_from_many: {len(buffers)} buffers, one apply takes 1 to {_lib.LEARNER_MAX_ROWS} rows")
        spec = DrawSpec(importance=importance, beta=beta, beta_final=beta_final, anneal_calls=anneal_calls,
                        rho_bar=rho_bar, generator=generator, clip_eps=clip_eps)
        rho_outs = [None] * len(buffers) if rho_out is None else list(rho_out)
        if len(rho_outs) != len(buffers):
            raise ValueError(f"update_from_many: rho_out holds {len(rho_outs)} entries for {len(buffers)} buffers")
        ratio_outs = [None] * len(buffers) if ratio_out is None else list(ratio_out)
        if len(ratio_outs) != len(buffers):
            raise ValueError(f"update_from_many: ratio_out holds {len(ratio_outs)} entries for {len(buffers)} buffers")
        return self._update_split(buffers, batch_size,
                                  [spec._replace(rho_out=r, ratio_out=q) for r, q in zip(rho_outs, ratio_outs)])

    def _update_split(self, buffers, batch_size: int, specs, gather=None):
        """The split update behind update_from_many and update_from(group=): a gradient row per buffer, the rows as
        `gather` completes them (the other ranks' rows), one apply, each buffer's priorities from its own draw."""
        rows = self.new_rows(len(buffers))
        drawn = [self._grad_drawn(b, batch_size, s, r) for b, s, r in zip(buffers, specs, rows)]
        al, cl = self.apply(rows if gather is None else gather(rows))
        for b, (_, td, idx) in zip(buffers, drawn):
            self.write_priorities(b, idx, td)
        return al, cl, [td for _, td, _ in drawn]

    def publish_actor(self, env) -> None:
        """The actor's current parameters into env's rollout actor, packed on the device (uavtrack_learner_publish_actor):
        stream-ordered, no host copy, no synchronisation, capturable -- the sync-free form of
        env.set_actor(self.actor_state_dict()), with the same bits.  env's actor must already be installed at this
        hidden_dim (set_actor)."""
        _lib.check(self._lib.uavtrack_learner_publish_actor(self._h, env._h, env._stream()),
                   "uavtrack_learner_publish_actor")

    # ---- weights and optimizer state
    def _module_state(self, module: torch.nn.Module, offset: int) -> "OrderedDict[str, torch.Tensor]":
        names, params = zip(*module.named_parameters())
        return OrderedDict(zip(names, split(self._get_params()[offset:], params)))

    def actor_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """FnnPolicyNet's state_dict (fc1.weight, fc1.bias, fc2.weight, fc2.bias; CPU fp32): loads into ActorMLP,
        the reference's FnnPolicyNet and BatchedUavEnv.set_actor."""
        return self._module_state(self._actor, 0)

    def critic_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """FnnValueNet's state_dict (CPU fp32)."""
        return self._module_state(self._critic, sum(p.numel() for p in self._actor.parameters()))

    def _optim_state(self):
        """(exp_avg [P], exp_avg_sq [P], step [8]) as numpy arrays: the actor's parameters, then the critic's."""
        return adam.read(self._lib.uavtrack_learner_get_optimizer_state, self._h, self.num_params,
                         _lib.LEARNER_TENSORS, self._stream())

    def _set_optim_state(self, exp_avg: np.ndarray, exp_avg_sq: np.ndarray, step: np.ndarray) -> None:
        """_optim_state's inverse."""
        adam.write(self._lib.uavtrack_learner_set_optimizer_state, self._h, np.ascontiguousarray(exp_avg, np.float32),
                   np.ascontiguousarray(exp_avg_sq, np.float32), np.ascontiguousarray(step, np.int64), self._stream())

    def _optimizers(self):
        """(parameters, lr, float span, tensor span) of the actor's and the critic's Adam in the flat state."""
        a = list(self._actor.parameters())
        na, ta = sum(p.numel() for p in a), len(a)
        return ((a, self.actor_lr, slice(0, na), slice(0, ta)),
                (list(self._critic.parameters()), self.critic_lr, slice(na, None), slice(ta, None)))

    def _adam_state_dicts(self):
        """(actor, critic) torch.optim.Adam state dicts, built by torch itself so Adam.load_state_dict accepts them."""
        m, v, steps = self._optim_state()
        return [to_state_dict(params, lr, m[f], v[f], steps[t]) for params, lr, f, t in self._optimizers()]

    def _load_adam(self, actor_sd: Optional[dict], critic_sd: Optional[dict]) -> None:
        m, v, steps = self._optim_state()
        for (params, lr, f, t), sd in zip(self._optimizers(), (actor_sd, critic_sd)):
            if sd is not None:
                m[f], v[f], steps[t] = from_state_dict(params, lr, sd)
        adam.write(self._lib.uavtrack_learner_set_optimizer_state, self._h, m, v, steps, self._stream())

    def _load_module(self, actor_sd: Optional[dict], critic_sd: Optional[dict]) -> None:
        cur = split(self._get_params(), self._params())
        t0 = 0
        for module, sd in ((self._actor, actor_sd), (self._critic, critic_sd)):
            names = [k for k, _ in module.named_parameters()]
            if sd is not None:
                probe = type(module)(_lib.OBS_DIM, self.hidden_dim, *((self.action_dim,) if module is self._actor else ()))
                probe.load_state_dict(sd)             # torch checks keys and shapes
                for i, k in enumerate(names):
                    cur[t0 + i] = probe.state_dict()[k]
            t0 += len(names)
        self._set_params(flat(cur))

    def state_dict(self) -> dict:
        """The four reference entries; while a target critic is enabled also "target_critic" (theta-, FnnValueNet's
        format) and "target" (its settings, as get_target returns them)."""
        a_opt, c_opt = self._adam_state_dicts()
        sd = {"actor": self.actor_state_dict(), "critic": self.critic_state_dict(),
              "actor_optimizer": a_opt, "critic_optimizer": c_opt}
        if self._target_on():
            sd["target_critic"], sd["target"] = self.target_state_dict(), self.get_target()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """state_dict's inverse.  "target" enables the target critic as saved and "target_critic" restores theta-; a
        learner with a target enabled that loads a checkpoint without one hard-syncs theta- to the loaded critic."""
        self._load_module(sd.get("actor"), sd.get("critic"))
        self._load_adam(sd.get("actor_optimizer"), sd.get("critic_optimizer"))
        self._restore_target(sd.get("target"), sd.get("target_critic"))

    def save(self, save_dir: str, epoch_i) -> None:
        """ActorCritic.save (actor_critic.py:181-190): <save_dir>/actor/actor_weights_<epoch>.pth and
        <save_dir>/critic/critic_weights_<epoch>.pth, each {'model_state_dict', 'optimizer_state_dict'}; while a target
        critic is enabled the critic file also holds 'target_state_dict' and 'target' (the settings)."""
        a_opt, c_opt = self._adam_state_dicts()
        extra = {"target_state_dict": self.target_state_dict(), "target": self.get_target()} if self._target_on() else {}
        for sub, model, opt, more in (("actor", self.actor_state_dict(), a_opt, {}),
                                      ("critic", self.critic_state_dict(), c_opt, extra)):
            os.makedirs(os.path.join(save_dir, sub), exist_ok=True)
            torch.save({"model_state_dict": model, "optimizer_state_dict": opt, **more},
                       os.path.join(save_dir, sub, f"{sub}_weights_{epoch_i}.pth"))

    def load(self, actor_path: Optional[str], critic_path: Optional[str]) -> None:
        """ActorCritic.load (actor_critic.py:192-205): each checkpoint that exists replaces that network's weights
        and Adam state.  (The learning rates stay the ones this learner was built with.)  A critic file with a
        'target_state_dict' restores the target critic as load_state_dict does; without one, an enabled target is
        hard-synced to the loaded critic."""
        ck = {}
        for key, path in (("actor", actor_path), ("critic", critic_path)):
            if path and os.path.exists(path):
                ck[key] = torch.load(path, map_location="cpu")
        self._load_module(ck["actor"]["model_state_dict"] if "actor" in ck else None,
                          ck["critic"]["model_state_dict"] if "critic" in ck else None)
        self._load_adam(ck["actor"]["optimizer_state_dict"] if "actor" in ck else None,
                        ck["critic"]["optimizer_state_dict"] if "critic" in ck else None)
        self._restore_target(ck.get("critic", {}).get("target"), ck.get("critic", {}).get("target_state_dict"))


class _TargetCritic:
    """DeviceActorCritic.target: the target critic's values, for whoever takes a `critic` with .values()."""

    def __init__(self, learner: DeviceActorCritic):
        self._learner = learner

    def values(self, states: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """DeviceActorCritic.values with theta- in the critic's place (uavtrack_learner_values_target): bit for bit the
        V(s') an update bootstraps from.  An error while no target is enabled."""
        return self._learner._values("uavtrack_learner_values_target", states, out)
