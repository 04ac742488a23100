#!/usr/bin/env python3
"""End-to-end MAAC training loop on the batched environment (example; the learner is plain PyTorch).

What the reference does per episode (src/train.py:142-196, 199-290): 200 steps x N batch-1 actor calls +
Environment.step, push the N*200 transitions into the replay buffer, sample, one ActorCritic.update
(src/models/actor_critic.py:150-178: TD(0) target r + gamma*V(s'), actor loss -log pi(a|s) * delta, critic MSE).
Here one iteration = B episodes at once: the whole rollout (actor + environment, B x N x T agent-steps) is ONE
launch of the library (uavtrack_run_actor), its [T,B,N] outputs go straight into a device replay ring, the
update is the same rule on a sampled batch, and the new actor weights are re-uploaded (sync_actor), or, with
--publish device, packed into the rollout's actor on the device with no host copy and no synchronisation.

    python examples/train_maac.py --envs 1024 --iters 40
    python examples/train_maac.py --method maac-r --envs 1024 --iters 40     # reciprocal (PMI) reward, PMI net trained too
    python examples/train_maac.py --replay prioritized --learner device --envs 4096 --n-uav 20   # prioritised ring, 32.8 M slots
    python examples/train_maac.py --replay prioritized --learner device --publish device --log-every 10   # no host sync per iteration
    python examples/train_maac.py --replay prioritized --learner device --importance --beta-final 1.0     # train on the importance weights, beta annealed on the device
    python examples/train_maac.py --replay prioritized --learner device --n-step 3                        # 3-step returns folded by the ring's add
    python examples/train_maac.py --replay prioritized --learner device --td-lambda 0.9                   # lambda-returns: critic values + a backward scan in the ring's add
    python examples/train_maac.py --replay prioritized --learner device --rho-bar 1.0 --publish device --log-every 10   # truncated importance ratios: who acted
    python examples/train_maac.py --replay prioritized --learner device --actor-loss per_sample --ppo-clip 0.2   # ... or PPO's clipped surrogate from the same store
    python examples/train_maac.py --replay prioritized --learner device --actor-loss per_sample --ppo-clip 0.2 --normalise-advantage   # ... on batch-standardised advantages
    python examples/train_maac.py --replay uniform-device --learner device --actor-loss per_sample --ppo-clip 0.2 --ppo-epochs 4 --minibatch 65536   # ... over 4 epochs of disjoint minibatches of the new rollout
    python examples/train_maac.py --replay prioritized --learner device --target-tau 0.005                # bootstrap from a Polyak-averaged target critic
    python examples/train_maac.py --replay uniform-device --learner device --actor-loss per_sample --ppo-clip 0.2 --ppo-epochs 4 --minibatch 65536 --target-kl 0.01 --publish device --log-every 10   # ... stopped by a KL latch on the device
    python examples/train_maac.py --replay uniform-device --learner device --actor-loss per_sample --ppo-clip 0.2 --ppo-epochs 4 --minibatch 65536 --gae-lambda 0.95   # ... on fixed GAE advantages and value targets
    python examples/train_maac.py --replay prioritized --learner device --target-period 100 --td-lambda 0.9   # ... or a periodic copy; the lambda add folds with it too
    python examples/train_maac.py --method maac-r --pmi-trainer device --learner device --replay prioritized --publish device --log-every 10
    python examples/train_maac.py --shards 8 --envs 32768 --n-uav 20 --learner device --replay prioritized --publish device   # 8 shard handles, one learner
    python examples/train_maac.py --shards 4 --method maac-r --pmi-trainer device --learner device --replay prioritized --publish device   # ... and one PMI trainer
    python examples/train_maac.py --phase evaluate --envs 256 --eval-episodes 4 --save-dir out   # train.evaluate, batched; csv files
    python examples/train_maac.py --phase run --envs 256                                         # train.run, the C-METHOD baseline

Every phase reports the reference's six per-episode results (train.py:181-196: return, the three reward terms, mean and
maximum of the covered targets) from a uavtrack.EpisodeStats, which folds each rollout's outputs on the device; in
`train` it is fed behind every rollout and read only on printed lines, so --log-every N still means no host
synchronisation in between.  --save-dir writes the lists as data_util.save_csv does (plus the two covered lists).

--method maac-r is the paper's method (configs/MAAC-R.yaml): the reward of every step is mixed in-kernel with the
neighbours' rewards, weighted by the PMI network's scores (uav.py:262-291); that network is trained alongside on
(timestep, uav-pair) samples of the rollout's observations (PMINet.py:74-100, here uavtrack.sample_pmi_pairs +
pmi_contrastive_loss on the device history) and its BatchNorm-folded weights are re-uploaded every iteration -- or, with
--publish device, folded and packed into the scorer on the device (publish_pmi), the index draw of train_pmi on a device
generator and the PMI loss read on printed lines only, so that a MAAC-R iteration too issues no host synchronisation.
"""
import argparse
import copy
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "marl-uavs-targets-tracking_amd")]

import torch  # noqa: E402
import uavtrack  # noqa: E402


class ValueNet(torch.nn.Module):
    """Same shape as the reference's critic FnnValueNet (actor_critic.py:101-112): Linear-ReLU-Linear -> scalar."""

    def __init__(self, state_dim=12, hidden_dim=128):
        super().__init__()
        self.fc1 = torch.nn.Linear(state_dim, hidden_dim)
        self.fc2 = torch.nn.Linear(hidden_dim, 1)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x))).squeeze(-1)


def update(actor, critic, opt_a, opt_c, batch, gamma, weights=None, entropy_coef=0.0, max_grad_norm=None, diag=None,
           rho_bar=None, rho_stats=None, target_critic=None, ppo_clip=None, normalise=False, adv_stats=None, kl_limit=None,
           kl_stats=None):
    """One ActorCritic.update step (actor_critic.py:150-178) on a batch of transitions.  weights (--importance): the
    draw's importance weights, one per row, multiplied into the per-sample losses before the mean.  entropy_coef and
    max_grad_norm: the two terms of DeviceActorCritic.set_regularisation, so that --learner torch and --learner device
    stay comparable; diag (a dict) receives the mean entropy and the two gradient norms before clipping.  A batch from an
    n-step ring (--n-step) carries "discounts", gamma^m per row, which take gamma's place in the target; so does a batch
    from a lambda ring (--td-lambda), whose rewards and discounts make that target the lambda-return.  rho_bar (--rho-bar):
    the batch carries "log_mu" and every row's losses are multiplied by min(rho_bar, pi / mu), a constant of the
    differentiation, as DeviceActorCritic.update_from(rho_bar=) does; rho_stats (a dict) receives the ratios.
    ppo_clip (--ppo-clip EPS): the batch carries "log_mu" and the policy term of a row becomes
    -min(r A, clamp(r, 1 - EPS, 1 + EPS) A) with r = pi / mu differentiated through and A = td_delta, as
    DeviceActorCritic.update_from(clip_eps=) trains; rho_stats receives the ratios.
    normalise (--normalise-advantage): the advantage of the policy term, plain or clipped, is the batch's standardised
    TD error (td - td.mean()) / (td.std() + 1e-8), as DeviceActorCritic.set_advantage("batch") trains; the critic keeps
    the raw TD error.  adv_stats (a dict) receives the mean and std of td_delta.
    target_critic (--target-tau / --target-period): the copy of the critic that V(s') comes from; keeping it in step
    is the caller's (sync_target_critic).
    A batch from a GAE ring (--gae-lambda) carries "advantages", which take td_delta's place as A (normalise applies on
    top), and a reward that is the fixed value target G_t with a discount of 0: the critic regresses on it as it stands.
    kl_limit (--target-kl X: 1.5 X, with ppo_clip): the minibatch's own mean((r - 1) - log r), formed in float64 from the
    float32 ratios before the step, goes to kl_stats["kl"]; where it exceeds kl_limit (compared in float32) nothing steps,
    kl_stats["stopped"] is set and the losses returned are NaN -- the host's `break`, which
    DeviceActorCritic.set_kl_stop latches on the device instead."""
    s, a, r, s2 = batch["states"], batch["actions"].long().unsqueeze(1), batch["rewards"], batch["next_states"]
    if target_critic is None:
        v_next = critic(s2)
    else:
        with torch.no_grad():
            v_next = target_critic(s2)
    td_target = r + batch.get("discounts", gamma) * v_next
    td_delta = td_target - critic(s)
    probs = actor(s)
    log_probs = torch.log(probs.gather(1, a).squeeze(1).clamp_min(1e-12))
    adv = batch["advantages"] if "advantages" in batch else td_delta.detach()
    if adv_stats is not None:
        adv_stats["mean"], adv_stats["std"] = adv.mean(), adv.std()
    if normalise:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    per_row = -log_probs * adv
    if ppo_clip is not None:
        r = torch.exp(log_probs - batch["log_mu"])
        per_row = -torch.min(r * adv, r.clamp(1 - ppo_clip, 1 + ppo_clip) * adv)
        if rho_stats is not None:
            rho_stats["rho"] = r.detach()
        if kl_limit is not None:
            r64 = r.detach().double()
            kl_stats["kl"] = ((r64 - 1.0) - torch.log(r64)).mean().float()
            if bool(kl_stats["kl"] > torch.tensor(kl_limit, dtype=torch.float32)):      # the host's synchronisation
                kl_stats["stopped"] = True
                return float("nan"), float("nan")
    if rho_bar is not None:
        rho = torch.exp(log_probs.detach() - batch["log_mu"]).clamp(max=rho_bar)
        weights = rho if weights is None else weights * rho
        if rho_stats is not None:
            rho_stats["rho"] = rho
    if entropy_coef or diag is not None:
        entropy = -(probs * torch.log(probs.clamp_min(1e-12))).sum(dim=1)
        if entropy_coef:
            per_row = per_row - entropy_coef * entropy
    if weights is None:
        actor_loss = torch.mean(per_row)
        critic_loss = torch.nn.functional.mse_loss(critic(s), td_target.detach())
    else:
        actor_loss = torch.mean(weights * per_row)
        critic_loss = torch.mean(weights * (critic(s) - td_target.detach()) ** 2)
    opt_a.zero_grad(); opt_c.zero_grad()
    actor_loss.backward(); critic_loss.backward()
    if max_grad_norm is not None:
        norms = [torch.nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm) for net in (actor, critic)]
        if diag is not None:
            diag["norms"] = torch.stack(norms).detach()
    if diag is not None:
        diag["entropy"] = entropy.detach().mean()
    opt_a.step(); opt_c.step()
    return float(actor_loss.detach()), float(critic_loss.detach())


def targeted(args):
    return args.target_tau is not None or args.target_period is not None


def sync_target_critic(args, target_critic, critic, updates_done):
    """The torch learner's side of --target-tau / --target-period, behind each update: DeviceActorCritic.set_target's two
    rules on a copy.deepcopy of the critic -- t <- (1 - tau) t + tau w with two float32 multiplies and one add, or a copy
    after every --target-period updates."""
    if args.target_tau is not None:
        tau32 = torch.tensor(args.target_tau, dtype=torch.float32)
        omt, tau = float(1.0 - tau32), float(tau32)                    # both float32 values: formed once, as the library's
    with torch.no_grad():
        for t, w in zip(target_critic.parameters(), critic.parameters()):
            if args.target_tau is not None:
                t.mul_(omt).add_(w * tau)
            elif updates_done % args.target_period == 0:
                t.copy_(w)


def lambda_critic(args, online, target):
    """Whose values the lambda add folds the rewards with (--lambda-critic): the target critic's while one is kept
    (the default then: the tail of a lambda-return bootstraps from the same slowly moving critic as its head, which
    every update takes from the target), else the online critic's."""
    return target if targeted(args) and args.lambda_critic != "online" else online


def device_learner(args, uavtrack, na_total, dev, max_batch):
    """The DeviceActorCritic of --learner device with --entropy-coef / --max-grad-norm; the diagnostics only when one of
    them is on.  A refused setting (--entropy-coef with --actor-loss reference) exits with the library's message.
    --target-tau / --target-period: its target critic (set_target)."""
    try:
        learner = uavtrack.DeviceActorCritic(12, args.hidden, na_total, args.actor_lr, args.critic_lr, args.gamma, dev,
                                             loss=args.actor_loss, max_batch=max_batch,
                                             entropy_coef=args.entropy_coef, max_grad_norm=args.max_grad_norm)
    except RuntimeError as e:
        raise SystemExit(f"train_maac.py: {e}")
    if regularised(args):
        learner.enable_diagnostics(max_batch)
    if targeted(args):
        learner.set_target(tau=args.target_tau, period=args.target_period)
    if args.normalise_advantage:
        learner.set_advantage("batch")                                # each draw standardised by its own statistics
    if args.target_kl is not None:
        learner.set_kl_stop(1.5 * args.target_kl)                     # the latch is cleared beside each sweep.rebind()
    return learner


def kl_field(kl, skipped):
    """The printed lines' extra field under --target-kl: the last evaluated minibatch's KL estimate and the updates that
    were stopped since the previous line."""
    return f"kl {float(kl):.5f} skipped {int(skipped)}  "


def advantage_field(mean, std):
    """The printed lines' extra field under --normalise-advantage: the mean and the standard deviation of the last
    update's TD errors (with --shards, of its last ring's draw)."""
    return f"td mean {float(mean):+.3f} std {float(std):.3f}  "


def nstep_ring(args, ring):
    """--n-step N > 1: the ring stores N-step returns and their discounts (with_nstep); N = 1 leaves it what it was.
    --td-lambda L: the ring stores lambda-returns instead (with_lambda).  --gae-lambda L: fixed GAE advantages and value
    targets (with_gae)."""
    if args.gae_lambda is not None:
        return ring.with_gae(args.gae_lambda, args.gamma)
    if args.td_lambda is not None:
        return ring.with_lambda(args.td_lambda, args.gamma)
    return ring.with_nstep(args.n_step, args.gamma) if args.n_step > 1 else ring


def behavioural(args):
    """--rho-bar or --ppo-clip: the two corrections for who acted, which both read the behaviour log-probabilities."""
    return args.rho_bar is not None or args.ppo_clip is not None


def behaviour_ring(args, ring):
    """--rho-bar / --ppo-clip: the ring keeps the behaviour log-probability of every slot (with_behaviour)."""
    return ring.with_behaviour() if behavioural(args) else ring


def add_rollout(args, ring, obs_in, res, acted, critic):
    """The rollout's outputs into the ring, before the iteration's updates.  --rho-bar / --ppo-clip: with the
    log-probabilities of `acted` -- the device learner, or the PyTorch actor -- whose actor at this moment is the one
    the rollout ran."""
    if not behavioural(args):
        ring.add_rollout(obs_in, res, **critic_kwargs(args, critic))
    else:
        ring.add_rollout_behaviour(obs_in, res, behaviour=acted, **critic_kwargs(args, critic))


def rho_field(rho, rho_bar):
    """The printed lines' extra field under --rho-bar: the mean ratio of the last update's batch and the share of its rows
    at the cap (a read of the device buffer rho_out filled: printed lines only)."""
    return f"rho mean {float(rho.mean()):.4f} at cap {float((rho >= rho_bar).float().mean()):.3f}  "


def ratio_field(r, eps):
    """The printed lines' extra field under --ppo-clip: the mean ratio of the last update's batch, the share of its rows
    with |r - 1| > EPS and the approximate KL mean(-log r) (a read of the device buffer ratio_out filled: printed lines
    only)."""
    return (f"ratio mean {float(r.mean()):.4f} clipped {float(((r - 1).abs() > eps).float().mean()):.3f} "
            f"kl {float(-torch.log(r).mean()):+.5f}  ")


class RatioMeans:
    """--ppo-epochs with --ppo-clip or --rho-bar: the printed lines' ratio statistics as a mean over the iteration's
    minibatches instead of the last update's alone, summed on the device (read on printed lines only)."""

    def __init__(self, args):
        self.args, self.sum, self.n = args, None, 0

    def add(self, r):
        a = self.args
        if a.ppo_clip is not None:
            v = torch.stack([r.mean(), ((r - 1).abs() > a.ppo_clip).float().mean(), -torch.log(r).mean()])
        else:
            v = torch.stack([r.mean(), (r >= a.rho_bar).float().mean()])
        self.sum, self.n = (v if self.sum is None else self.sum + v), self.n + 1

    def field(self):
        m = (self.sum / self.n).tolist()
        if self.args.ppo_clip is not None:
            return f"ratio mean {m[0]:.4f} clipped {m[1]:.3f} kl {m[2]:+.5f} (over {self.n} minibatches)  "
        return f"rho mean {m[0]:.4f} at cap {m[1]:.3f} (over {self.n} minibatches)  "


def epoch_sweeps(args, rings, rows, sweeps):
    """--ppo-epochs E, behind the iteration's adds: one sweep of minibatches of `rows` per ring, made on the first
    iteration and rebound to what the add has just written on every later one (ring.sweep, sweep.rebind: the cursor back
    at call 0), and the E * M update calls the iteration then takes -- M the minibatches of the smallest window, so that no
    ring goes beyond its E epochs."""
    try:
        sweeps = [ring.sweep(rows) for ring in rings] if sweeps is None else [s.rebind() for s in sweeps]
    except ValueError as e:
        raise SystemExit(f"train_maac.py: --minibatch: {e}")
    return sweeps, args.ppo_epochs * min(s.minibatches for s in sweeps)


def ratio_kwargs(args, bufs, rings):
    """update_from_many's arguments under --rho-bar or --ppo-clip, and the views of bufs (one per ring) the ratios land
    in; update_from takes the one view itself."""
    if not behavioural(args):
        return {}, None
    views = [b[:min(b.numel(), ring.count)] for b, ring in zip(bufs, rings)]
    if args.ppo_clip is not None:
        return {"clip_eps": args.ppo_clip, "ratio_out": views}, views
    return {"rho_bar": args.rho_bar, "rho_out": views}, views


def critic_kwargs(args, critic):
    """add_rollout's extra argument under --td-lambda or --gae-lambda: the critic whose values the add folds the rewards
    with (a GAE ring also takes its advantages' baseline from it)."""
    return {} if args.td_lambda is None and args.gae_lambda is None else {"critic": critic}


def regularised(args):
    return bool(args.entropy_coef) or args.max_grad_norm is not None


def regularisation_field(entropy, norms):
    """The printed lines' extra field while --entropy-coef or --max-grad-norm is on: the mean policy entropy of the last
    update's batch and the actor's and critic's gradient norms before clipping (nan without --max-grad-norm)."""
    a, c = (float("nan"), float("nan")) if norms is None else (float(norms[0]), float(norms[1]))
    return f"entropy {float(entropy):.4f}  grad norm {a:.4f} {c:.4f}  "


SIX = ("return_list", "target_tracking_return_list", "boundary_punishment_return_list",
       "duplicate_tracking_punishment_return_list", "average_covered_targets_list", "max_covered_targets_list")


def drain(stats_list, kept):
    """Read and clear every EpisodeStats (a synchronisation each: printed lines only); the records join `kept` (the
    lists --save-dir writes) and their means over the episodes since the previous line come back as a string."""
    reads = []
    for st in stats_list:
        reads.append(st.read())
        st.clear()
    got = {k: [v for r in reads for v in r[k].tolist()] for k in SIX}
    for k in SIX:
        kept[k].extend(got[k])
    n = max(1, len(got[SIX[0]]))
    tt, bp, dp, avg, mx = (sum(got[k]) / n for k in SIX[1:])
    lost = sum(r["dropped"] for r in reads)
    return (f"tracking {tt:+.4f}  boundary {bp:+.4f}  duplicate {dp:+.4f}  covered avg {avg:5.2f} max {mx:5.2f}  "
            f"episodes {len(got[SIX[0]])}" + (f" (+{lost} not logged)" if lost else ""))


def save_results(args, kept):
    if args.save_dir:
        os.makedirs(args.save_dir, exist_ok=True)
        uavtrack.episode_stats.save_csv(kept, args.save_dir, extra=True)


def evaluate_phase(args, env, policy):
    """--phase evaluate (train.evaluate, train.py:298-324) and --phase run (train.run, train.py:372-396), batched: every
    environment plays --eval-episodes episodes; prints the means of the six results, returns the per-episode returns."""
    res = uavtrack.evaluate(env, policy, args.steps, episodes=args.eval_episodes, seed=args.seed,
                            auto_reset=args.rollout_episodes > 1)       # then all the episodes in ONE launch
    n = len(res[SIX[0]])
    print(f"{args.phase}: {n} episodes of {args.steps} steps ({res['path']} path)  " +
          "  ".join(f"{k[:-5]} {res[k].mean():+.4f}" for k in SIX), flush=True)
    save_results(args, res)
    env.close()
    return res["return_list"].tolist()


def importance_kwargs(args):
    """What --importance / --beta / --beta-final mean to update_from, update_from_many and the ring's sample(): nothing
    without --importance (the reference's update drops the weights), else beta and, with --beta-final, the linear
    schedule over every draw of the run (iters x updates), counted on the device."""
    if not args.importance:
        return {}
    kw = {"importance": True, "beta": args.beta}
    if args.beta_final is not None:
        kw.update(beta_final=args.beta_final, anneal_calls=max(1, args.iters * args.updates))
    return kw


def train_sharded(args, timings=None):
    """--shards K: K environment handles over disjoint global environment ids, K rollouts, K prioritised rings, ONE
    device learner.  Every update takes one gradient row from each ring and applies them in shard order
    (update_from_many), each ring gets its own priorities back, and the new actor is published to every handle.
    --method maac-r: ONE device PMI trainer too, trained after the K rollouts on triples drawn over the K observation
    histories (train_pmi_many) and published to every handle's scorer."""
    dev = "cuda:0"
    K = args.shards
    torch.manual_seed(args.seed)
    coop = args.cooperative if args.cooperative is not None else (0.0 if args.method == "maac" else 0.3)
    mode = {"maac": uavtrack.RewardMode.RAW, "maac-g": uavtrack.RewardMode.MEAN, "maac-r": uavtrack.RewardMode.PMI}[args.method]
    envs = []
    for k in range(K):
        off, cnt = uavtrack.shard_range(args.envs, k, K)
        envs.append(uavtrack.BatchedUavEnv(uavtrack.EnvConfig(
            n_envs=cnt, n_uav=args.n_uav, m_targets=args.m_targets, cooperative=coop, reward_mode=mode,
            horizon=args.steps, env_offset=off), dev))
    pmi_dev = pmi_gen = None
    if args.method == "maac-r":                                       # ONE PMI trainer; every handle scores with its network
        pmi_dev = uavtrack.DevicePMINetwork(args.pmi_hidden, args.pmi_b2, dev, max_batch=max(args.pmi_batch, 4096))
        for e in envs:
            e.set_pmi(pmi_dev)
        if args.pmi_draw == "device" or (args.pmi_draw == "auto" and args.publish == "device"):
            pmi_gen = torch.Generator(device=dev)
            pmi_gen.manual_seed(args.seed)
    na_total = envs[0].cfg.na_total
    actor = uavtrack.ActorMLP(hidden_dim=args.hidden, action_dim=na_total).to(dev)
    per_shard = -(-args.batch // K)                                   # rows each ring contributes to one update
    learner = device_learner(args, uavtrack, na_total, dev, per_shard)
    actor.load_state_dict(learner.actor_state_dict())
    rollouts = [uavtrack.BatchedRollout(e, actor, device_actor=True, seed=args.seed) for e in envs]
    if args.replay == "prioritized":
        rings = [uavtrack.PrioritizedReplayRing(2 * e.cfg.n_envs * args.n_uav * args.steps, dev, alpha=args.alpha,
                                                seed=args.seed + 7919 * k, max_batch=per_shard) for k, e in enumerate(envs)]
    else:                                                             # uniform-device
        rings = [uavtrack.ReplayRing(2 * e.cfg.n_envs * args.n_uav * args.steps, dev, seed=args.seed + 7919 * k,
                                     max_batch=per_shard) for k, e in enumerate(envs)]
    rings = [behaviour_ring(args, nstep_ring(args, ring)) for ring in rings]
    rho_bufs = [torch.empty(per_shard, device=dev) for _ in rings] if behavioural(args) else None
    per_iter = args.envs * args.n_uav * args.steps
    stats = [uavtrack.EpisodeStats(e, log_capacity=e.cfg.n_envs * args.log_every, max_steps=args.steps) for e in envs]
    kept = {k: [] for k in SIX}
    history, stamps, outs = [], [], [None] * K
    sweeps = None                                                     # --ppo-epochs: one sweep per ring, made at the first add
    t_log = time.perf_counter()
    for it in range(args.iters):
        log = (it + 1) % args.log_every == 0 or it == args.iters - 1
        t0 = time.perf_counter()
        eps = []
        for k, (ro, ring) in enumerate(zip(rollouts, rings)):
            ro.seed = args.seed + it
            ro.reset(seed=1000 + it)
            obs_in = ro.obs.clone()
            res = ro.run_fused(args.steps, out=outs[k], stats=stats[k])    # done fires at the horizon: one record per episode
            outs[k] = {key: v for key, v in res.items() if key != "ep_sums"}
            add_rollout(args, ring, obs_in, res, learner,
                        lambda_critic(args, learner, learner.target))   # (--td-lambda: every ring, the one learner's values)
            eps.append(res["ep_sums"])
        if log:
            torch.cuda.synchronize()
        t_roll = time.perf_counter() - t0
        sources, n_updates = rings, args.updates
        if args.ppo_epochs:                                           # E epochs over what the adds above wrote
            sweeps, n_updates = epoch_sweeps(args, rings, per_shard, sweeps)
            sources = sweeps
        rho_kw, rhos = ratio_kwargs(args, rho_bufs, sources)          # every ring's ratios, read on printed lines only
        means = RatioMeans(args) if log and rho_kw and args.ppo_epochs else None
        for _ in range(n_updates):
            la_t, lc_t, tds = learner.update_from_many(sources, per_shard, **importance_kwargs(args), **rho_kw)
            if means is not None:
                means.add(torch.cat(rhos))
        la, lc = (float(la_t), float(lc_t)) if log else (la_t, lc_t)
        reg_field = ""
        if log and regularised(args):                                 # the last ring's rows of the last update
            reg_field = regularisation_field(learner.entropy(tds[-1].numel()).mean(), learner.grad_norm)
        if means is not None:
            reg_field += means.field()
        elif log and rho_kw:
            reg_field += rho_field(torch.cat(rhos), args.rho_bar) if args.ppo_clip is None else \
                ratio_field(torch.cat(rhos), args.ppo_clip)
        if log and args.normalise_advantage:
            reg_field += advantage_field(learner.advantage_stats[0], learner.advantage_stats[2])
        if args.publish == "host":
            actor.load_state_dict(learner.actor_state_dict())
            for ro in rollouts:
                ro.sync_actor()
        else:
            for e in envs:
                learner.publish_actor(e)                              # one device pack per handle
        pmi_field = ""
        if pmi_dev is not None:                                       # train_pmi over the K histories, never concatenated
            lp = pmi_dev.train_pmi_many({"pmi": {"batch_size": args.pmi_batch}}, [o["obs"] for o in outs], args.n_uav,
                                        generator=pmi_gen, sync=False)
            for e in envs:
                if args.publish == "device":
                    pmi_dev.publish_pmi(e)                            # no copy to the host, no synchronisation
                else:
                    e.set_pmi(pmi_dev)
            if log:
                pmi_field = f"pmi loss {float(lp):.4f}  "
        ep = torch.cat(eps)                                           # [envs, 5] in global environment order
        history.append(ep[:, 0].mean())
        if not log:
            continue
        ret, cov = float(ep[:, 0].mean()), float(ep[:, 4].mean()) / args.steps
        six = drain(stats, kept)
        torch.cuda.synchronize()
        now = time.perf_counter()
        n_iter = it + 1 - (stamps[-1][0] if stamps else 0)
        stamps.append((it + 1, now))
        print(f"iter {it:3d}  shards {K}  episode return {ret:8.3f}  covered targets/step {cov:5.2f}  actor loss {la:+.4f}  "
              f"critic loss {lc:.4f}  {reg_field}{pmi_field}rollout {t_roll * 1e3:6.1f} ms ({per_iter / t_roll / 1e9:.2f} G agent-steps/s)  "
              f"iteration {((now - t0) if args.log_every == 1 else (now - t_log) / n_iter) * 1e3:6.1f} ms  {six}", flush=True)
        t_log = now
    save_results(args, kept)
    for ring in rings:
        ring.check()                                                  # no draw was refused on the device
    learner.check()                                                   # no update was refused on the device
    if pmi_dev is not None:
        pmi_dev.check()                                               # no train_pmi call was refused on the device
    for e in envs:
        e.close()
    history = [float(r) for r in history]
    if timings is not None:
        timings.extend(stamps)
    return history


def main(argv=None, timings=None):
    """Returns the episode return of every iteration.  timings (a list, optional) receives (iterations done, perf_counter)
    at every printed line, each taken after a synchronisation."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--n-uav", type=int, default=10)        # configs/MAAC.yaml: 10 UAVs, 10 targets
    ap.add_argument("--m-targets", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)       # main.py:128 num_steps
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--updates", type=int, default=8, help="learner updates per iteration")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--hidden", type=int, default=128)      # configs/MAAC.yaml:34
    ap.add_argument("--gamma", type=float, default=0.95)
    ap.add_argument("--actor-lr", type=float, default=1e-4)
    ap.add_argument("--critic-lr", type=float, default=5e-4)
    ap.add_argument("--method", choices=["maac", "maac-g", "maac-r"], default="maac")
    ap.add_argument("--cooperative", type=float, default=None, help="default: 0 for maac, 0.3 for maac-g / maac-r")
    ap.add_argument("--pmi-hidden", type=int, default=128)   # configs/MAAC-R.yaml:39
    ap.add_argument("--pmi-b2", type=int, default=3000)      # PMINetwork b2_size (PMINet.py:21)
    ap.add_argument("--pmi-batch", type=int, default=500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--learner", choices=["torch", "device"], default="torch",
                    help="torch: the PyTorch update below (per-sample actor loss); device: uavtrack.DeviceActorCritic, "
                         "the whole update in one library call")
    ap.add_argument("--actor-loss", choices=["reference", "per_sample"], default="reference",
                    help="--learner device only: the reference's broadcast loss mean(-log p) * mean(delta), or "
                         "mean(-log p * delta) (what the torch learner trains with)")
    ap.add_argument("--entropy-coef", type=float, default=0.0,
                    help="entropy bonus c: actor loss mean(w (-log p delta - c H)), in both learners (--learner device: "
                         "DeviceActorCritic(entropy_coef=c), --actor-loss per_sample only)")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="clip_grad_norm_ of the actor's and of the critic's gradient to this norm before each Adam step, "
                         "in both learners (--learner device: DeviceActorCritic(max_grad_norm=...)); default: no clipping")
    ap.add_argument("--pmi-trainer", choices=["torch", "device"], default="torch",
                    help="--method maac-r only: torch: the PyTorch PMINetwork.train_pmi loop below; device: "
                         "uavtrack.DevicePMINetwork, the whole train_pmi call in one library call")
    ap.add_argument("--replay", choices=["uniform", "uniform-device", "prioritized"], default="uniform",
                    help="uniform: DeviceReplayBuffer (random.sample, train.py:57); uniform-device: uavtrack.ReplayRing, "
                         "the same buffer added to from the rollout and drawn from in HIP (distinct slots, O(batch)); "
                         "prioritized: uavtrack.PrioritizedReplayRing (the reference's PrioritizedReplayBuffer, "
                         "train.py:73-139), added to from the rollout and drawn from in HIP, |td_delta| written back as the "
                         "new priorities")
    ap.add_argument("--n-step", type=int, default=1,
                    help="N > 1: train on N-step targets.  The ring's add folds each transition's next N rewards (never "
                         "across an episode end or the rollout's last step) and keeps gamma^m per slot "
                         "(ring.with_nstep(N, gamma)); both learners bootstrap with that discount.  Needs --replay "
                         "prioritized or uniform-device")
    ap.add_argument("--td-lambda", type=float, default=None,
                    help="L in [0, 1]: train on TD(lambda) targets.  The ring's add evaluates the critic on the rollout's "
                         "observations and walks every agent's chain backwards (ring.with_lambda(L, gamma), "
                         "add_rollout(critic=...)): each slot keeps r + gamma L G' as its reward and gamma (1 - L) as its "
                         "discount, never across an episode end or the rollout's last step.  Needs --replay prioritized or "
                         "uniform-device; not with --n-step > 1")
    ap.add_argument("--gae-lambda", type=float, default=None, metavar="L",
                    help="L in [0, 1], with --ppo-epochs: fixed GAE(L) advantages and value targets per slot.  The ring's add "
                         "evaluates the critic on the rollout's observations and walks every agent's chain backwards "
                         "(ring.with_gae(L, gamma), add_rollout(critic=...)): each slot keeps the lambda-return G as its "
                         "reward, 0 as its discount and G - V(s) as its advantage, never across an episode end or the "
                         "rollout's last step, and every minibatch of the iteration's epochs trains the actor on that "
                         "advantage and the critic on that target (the device learner through "
                         "uavtrack_learner_update_stored, the torch learner from sample()['advantages']).  "
                         "--normalise-advantage, --ppo-clip, --shards and --lambda-critic apply.  Needs --replay prioritized "
                         "or uniform-device, and --actor-loss per_sample with --learner device; not with --n-step > 1 or "
                         "--td-lambda")
    ap.add_argument("--ppo-clip", type=float, default=None, metavar="EPS",
                    help="EPS >= 0: PPO's clipped surrogate instead of --rho-bar.  The ring keeps log mu(a|s) as for "
                         "--rho-bar, and every update trains -min(r A, clip(r, 1 - EPS, 1 + EPS) A) with r = pi / mu "
                         "differentiated through and A the TD error (DeviceActorCritic.update_from(clip_eps=EPS), inside "
                         "the gradient kernel; the torch learner trains the same expression); the printed lines show the "
                         "mean ratio, the share of rows with |r - 1| > EPS and mean(-log r).  Needs --replay prioritized or "
                         "uniform-device, and --actor-loss per_sample with --learner device; not with --rho-bar")
    ap.add_argument("--ppo-epochs", type=int, default=None, metavar="E",
                    help="E >= 1: on-policy epochs in place of --updates.  After each iteration's add the ring's sweep is "
                         "rebound to the slots that add wrote (ring.sweep(K), sweep.rebind()) and the iteration takes E * M "
                         "updates from it, M = window // K: E passes over the new rollout in disjoint minibatches, every "
                         "transition once per pass, in another order each pass (DeviceActorCritic.update_from(sweep, K); the "
                         "torch learner trains on sweep.sample(), and leaves a prioritised ring's priorities alone).  "
                         "--ppo-clip, --rho-bar, --normalise-advantage, --entropy-coef, --n-step, --td-lambda and --shards "
                         "apply as before, and the printed ratio statistics become means over the iteration's minibatches.  "
                         "Needs --replay prioritized or uniform-device; not with --importance (a sweep is uniform)")
    ap.add_argument("--target-kl", type=float, default=None, metavar="X",
                    help="X >= 0, with --ppo-clip and --ppo-epochs: KL early stopping.  Every minibatch's own estimate "
                         "mean((r - 1) - log r) is formed before its step, and once one exceeds 1.5 X the rest of the "
                         "iteration's updates are skipped.  --learner device: DeviceActorCritic.set_kl_stop(1.5 X), a latch on "
                         "the device cleared beside each iteration's sweep.rebind() (kl_reset), so --log-every N still "
                         "means no host synchronisation; --learner torch: the same estimator on the same rows and a host "
                         "break.  Printed lines show the last KL and the updates skipped since the previous line (the "
                         "losses of a line whose last update was stopped are NaN).  Not with --shards K > 1")
    ap.add_argument("--minibatch", type=int, default=None, metavar="K",
                    help="--ppo-epochs only: rows per minibatch (default: --batch; with --shards, split over the rings as "
                         "--batch is); at most what one iteration adds")
    ap.add_argument("--normalise-advantage", action="store_true",
                    help="standardise each batch's TD errors before they multiply grad log p (and gate --ppo-clip): "
                         "A = (td - mean) / (std + 1e-8), in both learners (--learner device: "
                         "DeviceActorCritic.set_advantage(\"batch\"), --actor-loss per_sample only; with --shards each "
                         "ring's draw by its own statistics); the printed lines gain the mean and std of td")
    ap.add_argument("--rho-bar", type=float, default=None,
                    help="R > 0: correct for who acted.  The ring keeps log mu(a|s) of every slot, evaluated by the learner's "
                         "actor over the window each add writes (ring.with_behaviour(), add_rollout_behaviour), and every "
                         "update weighs its rows by the truncated importance ratio min(R, pi / mu) "
                         "(DeviceActorCritic.update_from(rho_bar=R); the torch learner multiplies its per-sample losses by "
                         "the same ratios); the printed lines show the mean ratio and the share of rows at the cap.  With "
                         "--n-step or --td-lambda the ratio corrects the first action only.  Needs --replay prioritized or "
                         "uniform-device")
    tgt = ap.add_mutually_exclusive_group()
    tgt.add_argument("--target-tau", type=float, default=None,
                     help="tau in (0, 1]: bootstrap V(s') from a target critic kept by Polyak averaging, "
                          "t <- (1 - tau) t + tau w after every update (DeviceActorCritic.set_target(tau=...); the torch "
                          "learner keeps a copy.deepcopy of its critic under the same rule)")
    tgt.add_argument("--target-period", type=int, default=None,
                     help="K >= 1: bootstrap V(s') from a target critic that is copied from the critic after every K "
                          "updates (DeviceActorCritic.set_target(period=K), counted on the device; the torch learner "
                          "likewise)")
    ap.add_argument("--lambda-critic", choices=["target", "online"], default=None,
                    help="--td-lambda with a target critic: whose values the ring's add folds the rewards with.  Default "
                         "target: the whole lambda-return then bootstraps from the one slowly moving critic, as the "
                         "update's own V(s') does; online: the critic being trained, as without a target")
    ap.add_argument("--alpha", type=float, default=0.6, help="--replay prioritized: priority exponent (train.py:74)")
    ap.add_argument("--beta", type=float, default=0.4, help="--replay prioritized: importance exponent (train.py:100)")
    ap.add_argument("--importance", action="store_true",
                    help="--replay prioritized only: train on the draw's importance weights (count * P(i))^-beta / max "
                         "(weighted critic and actor losses: DeviceActorCritic.update_from(importance=True), or the torch "
                         "learner's per-sample losses times the weights); default: drop them, as the reference does")
    ap.add_argument("--beta-final", type=float, default=None,
                    help="--importance only: anneal beta linearly from --beta to this value over the run's iters x updates "
                         "draws, on the ring's device call counter (no host value to freeze in a captured update)")
    ap.add_argument("--publish", choices=["host", "device"], default="host",
                    help="host: the learner's actor weights reach the rollout through the host pack (sync_actor); device: "
                         "packed on the device from the learner's parameters (publish_actor), no copy, no synchronisation; "
                         "with --method maac-r the PMI network reaches the scorer the same way (publish_pmi)")
    ap.add_argument("--pmi-draw", choices=["auto", "cpu", "device"], default="auto",
                    help="--pmi-trainer device only: where train_pmi draws its index triples: torch's CPU generator (the "
                         "reference's stream; copies them to the device) or a device generator seeded with --seed (no "
                         "host work); auto: cpu with --publish host, device with --publish device")
    ap.add_argument("--shards", type=int, default=1,
                    help="split --envs into K environment handles (uavtrack.shard_range: disjoint global environment "
                         "ids), each with its own rollout and device ring, and take every update of the ONE learner "
                         "from all K rings (DeviceActorCritic.update_from_many: one gradient row per ring, one apply); "
                         "needs --learner device and --replay prioritized or uniform-device; --method maac-r also needs --pmi-trainer device "
                         "(DevicePMINetwork.train_pmi_many over the K observation histories, un-concatenated), and each "
                         "MAAC-R handle sizes its own scorer scratch")
    ap.add_argument("--log-every", type=int, default=1,
                    help="print (and so synchronise) every N iterations and after the last; the iteration time printed is "
                         "the mean over the iterations since the previous line, and with N > 1 the rollout time of a "
                         "line includes the work still queued from the iterations before it")
    ap.add_argument("--phase", choices=["train", "evaluate", "run"], default="train",
                    help="main.py's three phases: train; evaluate (train.evaluate: the actor, sampled, --eval-episodes "
                         "episodes per environment); run (train.run: the C-METHOD greedy baseline)")
    ap.add_argument("--eval-episodes", type=int, default=1, help="--phase evaluate / run: episodes per environment")
    ap.add_argument("--rollout-episodes", type=int, default=1,
                    help="K > 1: every iteration is ONE launch of K * --steps steps that resets each environment inside the "
                         "kernel at its horizon (BatchedRollout(auto_reset_seed=...)): K episodes per environment without a "
                         "reset launch or an observation copy in between; --phase evaluate / run then play their "
                         "--eval-episodes in one launch too (evaluate(auto_reset=True)).  Not with --shards")
    ap.add_argument("--actor-path", default=None,
                    help="--phase evaluate: a saved FnnPolicyNet / ActorMLP state dict (default: fresh weights)")
    ap.add_argument("--save-dir", default=None,
                    help="write the per-episode result lists there as data_util.save_csv does (return_list.csv, ...), "
                         "plus average_covered_targets_list.csv and max_covered_targets_list.csv; default: nothing is written")
    args = ap.parse_args(argv)
    if args.log_every < 1:
        ap.error("--log-every must be >= 1")
    if args.eval_episodes < 1:
        ap.error("--eval-episodes must be >= 1")
    if args.rollout_episodes < 1:
        ap.error("--rollout-episodes must be >= 1")
    if args.rollout_episodes > 1 and args.shards > 1:
        ap.error("--rollout-episodes K > 1 runs on one environment handle (no --shards)")
    if args.phase == "run" and args.method == "maac-r":
        ap.error("--phase run is the C-METHOD baseline: it runs with the maac / maac-g rewards")
    if not 1 <= args.n_step <= 64:
        ap.error("--n-step must be in [1, 64]")
    if args.n_step > 1 and args.replay == "uniform":
        ap.error("--n-step N > 1 needs --replay prioritized or --replay uniform-device: the n-step returns are folded by "
                 "the device rings' add (the PyTorch buffer of --replay uniform stores one-step transitions)")
    if args.td_lambda is not None:
        if not 0.0 <= args.td_lambda <= 1.0:
            ap.error("--td-lambda must be in [0, 1]")
        if args.n_step > 1:
            ap.error("--td-lambda and --n-step N > 1 exclude each other: a ring stores lambda-returns or n-step returns")
        if args.replay == "uniform":
            ap.error("--td-lambda needs --replay prioritized or --replay uniform-device: the lambda-returns are folded by "
                     "the device rings' add (the PyTorch buffer of --replay uniform stores one-step transitions)")
    if args.gae_lambda is not None:
        if not 0.0 <= args.gae_lambda <= 1.0:
            ap.error("--gae-lambda must be in [0, 1]")
        if args.n_step > 1 or args.td_lambda is not None:
            ap.error("--gae-lambda excludes --n-step N > 1 and --td-lambda: a ring stores n-step returns, lambda-returns or "
                     "GAE advantages, one of the three")
        if args.ppo_epochs is None or args.replay == "uniform":
            ap.error("--gae-lambda needs --ppo-epochs and --replay prioritized or --replay uniform-device: the advantages "
                     "are fixed per slot by the device rings' add, for the epochs over what that add wrote")
        if args.learner == "device" and args.actor_loss != "per_sample":
            ap.error("--gae-lambda with --learner device needs --actor-loss per_sample: the reference form scales the actor's "
                     "gradient sums once by -mean(delta) / N, a factor a per-row advantage cannot share")
    if args.rho_bar is not None and (not args.rho_bar > 0 or args.replay == "uniform"):
        ap.error("--rho-bar must be > 0 and needs --replay prioritized or --replay uniform-device (the device rings keep "
                 "the behaviour log-probabilities)")
    if args.normalise_advantage and args.learner == "device" and args.actor_loss != "per_sample":
        ap.error("--normalise-advantage with --learner device needs --actor-loss per_sample: the reference form scales the "
                 "actor's gradient sums once by -mean(delta) / N, and a standardised advantage has mean 0")
    if args.ppo_clip is not None:
        if not args.ppo_clip >= 0 or args.replay == "uniform":
            ap.error("--ppo-clip must be >= 0 and needs --replay prioritized or --replay uniform-device (the device rings "
                     "keep the behaviour log-probabilities)")
        if args.rho_bar is not None:
            ap.error("--ppo-clip and --rho-bar exclude each other: one correction for who acted, not two")
        if args.learner == "device" and args.actor_loss != "per_sample":
            ap.error("--ppo-clip with --learner device needs --actor-loss per_sample: the reference form scales the actor's "
                     "gradient sums once by -mean(delta) / N, a factor a per-row gate cannot share")
    if args.target_kl is not None:
        if not args.target_kl >= 0:
            ap.error("--target-kl must be >= 0")
        if args.ppo_clip is None or args.ppo_epochs is None:
            ap.error("--target-kl needs --ppo-clip and --ppo-epochs: the estimate is formed from the clipped surrogate's "
                     "ratios, and what it stops is the rest of an iteration's epochs")
        if args.shards > 1:
            ap.error("--target-kl is not for --shards K > 1: the shards' one update is a split update, and a gradient row "
                     "has nowhere to carry a KL sum")
    if args.minibatch is not None and args.ppo_epochs is None:
        ap.error("--minibatch is the minibatch of --ppo-epochs")
    if args.ppo_epochs is not None:
        if args.ppo_epochs < 1 or args.replay == "uniform":
            ap.error("--ppo-epochs must be >= 1 and needs --replay prioritized or --replay uniform-device (the sweep is "
                     "the device rings' draw)")
        if args.importance:
            ap.error("--ppo-epochs and --importance exclude each other: a sweep is a uniform pass and has no importance "
                     "weights")
        if args.minibatch is not None:
            args.batch = args.minibatch                               # what the rings and the learner are sized by
        if not 1 <= args.batch <= args.envs * args.n_uav * args.steps * args.rollout_episodes:
            ap.error("--minibatch (default --batch) must be in [1, envs * n_uav * steps * rollout-episodes]: a minibatch is "
                     "part of what one iteration adds")
    if args.target_tau is not None and not 0.0 < args.target_tau <= 1.0:
        ap.error("--target-tau must lie in (0, 1]")
    if args.target_period is not None and args.target_period < 1:
        ap.error("--target-period must be >= 1")
    if args.lambda_critic is not None and ((args.td_lambda is None and args.gae_lambda is None) or not targeted(args)):
        ap.error("--lambda-critic chooses between two critics: it needs --td-lambda and --target-tau or --target-period")
    if args.importance and args.replay != "prioritized":
        ap.error("--importance needs --replay prioritized (a uniform draw has no importance weights)")
    if args.beta_final is not None and not args.importance:
        ap.error("--beta-final anneals the importance exponent: it needs --importance")
    if args.phase != "train":
        args.shards = 1

    if args.shards < 1 or args.shards > args.envs:
        ap.error("--shards must be in [1, --envs]")
    if args.shards > 1:
        if args.learner != "device" or args.replay == "uniform":
            ap.error("--shards K > 1 needs --learner device and --replay prioritized or uniform-device (one device "
                     "learner updated from K device rings)")
        if args.method == "maac-r" and args.pmi_trainer != "device":
            ap.error("--shards K > 1 with --method maac-r needs --pmi-trainer device (one uavtrack.DevicePMINetwork "
                     "trained over the K observation histories: train_pmi_many)")
        return train_sharded(args, timings)

    dev = "cuda:0"
    torch.manual_seed(args.seed)
    coop = args.cooperative if args.cooperative is not None else (0.0 if args.method == "maac" else 0.3)
    mode = {"maac": uavtrack.RewardMode.RAW, "maac-g": uavtrack.RewardMode.MEAN, "maac-r": uavtrack.RewardMode.PMI}[args.method]
    cfg = uavtrack.EnvConfig(n_envs=args.envs, n_uav=args.n_uav, m_targets=args.m_targets, cooperative=coop,
                             reward_mode=mode, horizon=args.steps)
    env = uavtrack.BatchedUavEnv(cfg, dev)
    pmi = opt_p = pmi_dev = None
    if args.method == "maac-r" and args.pmi_trainer == "device":
        pmi_dev = uavtrack.DevicePMINetwork(args.pmi_hidden, args.pmi_b2, dev, max_batch=max(args.pmi_batch, 4096))
        env.set_pmi(pmi_dev)
    elif args.method == "maac-r":
        pmi = uavtrack.make_pmi_net(args.pmi_hidden).to(dev)
        opt_p = torch.optim.Adam(pmi.parameters(), lr=1e-3)          # PMINet.py:39
        env.set_pmi(pmi.state_dict())
    pmi_gen = None
    if pmi_dev is not None and (args.pmi_draw == "device" or (args.pmi_draw == "auto" and args.publish == "device")):
        pmi_gen = torch.Generator(device=dev)
        pmi_gen.manual_seed(args.seed)
    actor = uavtrack.ActorMLP(hidden_dim=args.hidden, action_dim=cfg.na_total).to(dev)
    if args.phase != "train":
        if args.actor_path:
            actor.load_state_dict(torch.load(args.actor_path, map_location=dev))
        return evaluate_phase(args, env, actor if args.phase == "evaluate" else "greedy")
    critic = ValueNet(hidden_dim=args.hidden).to(dev)
    opt_a = torch.optim.Adam(actor.parameters(), lr=args.actor_lr)
    opt_c = torch.optim.Adam(critic.parameters(), lr=args.critic_lr)
    target_critic = None                                              # the torch learner's target (--learner torch)
    learner = None
    if args.learner == "device":
        learner = device_learner(args, uavtrack, cfg.na_total, dev, args.batch)
        actor.load_state_dict(learner.actor_state_dict())
    elif targeted(args):
        target_critic = copy.deepcopy(critic).requires_grad_(False)
    updates_done = 0
    rollout = uavtrack.BatchedRollout(env, actor, device_actor=True, seed=args.seed)
    K = args.rollout_episodes
    T = K * args.steps                                                # steps of one launch
    per_iter = args.envs * args.n_uav * T
    if args.replay == "prioritized":
        replay = uavtrack.PrioritizedReplayRing(2 * per_iter, dev, alpha=args.alpha, seed=args.seed,
                                                max_batch=args.batch)
    elif args.replay == "uniform-device":
        replay = uavtrack.ReplayRing(2 * per_iter, dev, seed=args.seed, max_batch=args.batch)
    if args.replay != "uniform":
        replay = behaviour_ring(args, nstep_ring(args, replay))
    else:
        replay = uavtrack.DeviceReplayBuffer(capacity=2 * per_iter, device=dev)
    rho_buf = torch.empty(args.batch, device=dev) if behavioural(args) and learner is not None else None
    stats = uavtrack.EpisodeStats(env, log_capacity=args.envs * K * args.log_every, max_steps=T)
    kept = {k: [] for k in SIX}
    history = []
    out = None
    sweeps = None                                                     # --ppo-epochs: the ring's sweep, made at the first add
    kl_stats = {}                                                     # --target-kl: the last evaluated KL ...
    kl_skipped = torch.zeros((), dtype=torch.int64, device=dev)       # ... and the updates stopped since the last line
    t_log = time.perf_counter()
    stamps = []
    for it in range(args.iters):
        log = (it + 1) % args.log_every == 0 or it == args.iters - 1
        t0 = time.perf_counter()
        rollout.seed = args.seed + it
        rollout.reset(seed=1000 + it)
        if K > 1:
            rollout.auto_reset_seed = 1000 + it                       # the in-launch resets continue this iteration's reset stream
        obs_in = rollout.obs.clone()
        res = rollout.run_fused(T, out=out, stats=stats)              # K * B episodes, one launch; done at the horizon closes them
        out = {k: v for k, v in res.items() if k != "ep_sums"}        # reuse the output buffers next time
        if args.replay != "uniform":
            add_rollout(args, replay, obs_in, res, actor if learner is None else learner,
                        lambda_critic(args, critic, target_critic) if learner is None else
                        lambda_critic(args, learner, learner.target))   # straight from the outputs
        else:
            replay.add(uavtrack.transitions_from_rollout(obs_in, res))
        if log:
            torch.cuda.synchronize()
        t_roll = time.perf_counter() - t0
        diag = {} if log and regularised(args) else None              # the torch learner's entropy and norms
        rho_stats = {}                                                # --rho-bar: the last update's ratios, a device tensor
        adv_stats = {} if args.normalise_advantage else None          # the last update's mean and std of td_delta
        reg_kw = dict(entropy_coef=args.entropy_coef, max_grad_norm=args.max_grad_norm, diag=diag, rho_bar=args.rho_bar,
                      rho_stats=rho_stats, target_critic=target_critic, ppo_clip=args.ppo_clip,
                      normalise=args.normalise_advantage, adv_stats=adv_stats)
        if args.target_kl is not None and learner is None:
            reg_kw.update(kl_limit=1.5 * args.target_kl, kl_stats=kl_stats)
        boot = critic if target_critic is None else target_critic     # whose V(s') the torch learner bootstraps from
        source, n_updates = replay, args.updates
        if args.ppo_epochs:                                           # E epochs over what the add above wrote
            sweeps, n_updates = epoch_sweeps(args, [replay], args.batch, sweeps)
            source = sweeps[0]
        means = RatioMeans(args) if log and behavioural(args) and args.ppo_epochs else None
        if args.target_kl is not None and learner is not None:
            learner.kl_reset()                                        # beside the rebind: a new iteration, a clear latch
        if learner is None and args.ppo_epochs:                       # the torch learner on the sweep's minibatches
            for q in range(n_updates):
                la, lc = update(actor, critic, opt_a, opt_c, source.sample(), args.gamma, **reg_kw)
                if means is not None:
                    means.add(rho_stats["rho"])
                if kl_stats.pop("stopped", False):                    # --target-kl: the rest of the iteration is skipped
                    kl_skipped += n_updates - q
                    break
                updates_done += 1
                if target_critic is not None:
                    sync_target_critic(args, target_critic, critic, updates_done)
        elif learner is None and args.replay == "prioritized":        # train.py:250-262
            ikw = importance_kwargs(args)
            for _ in range(args.updates):
                batch, idx, w = replay.sample(args.batch, args.beta, ikw.get("beta_final"), ikw.get("anneal_calls", 0))
                la, lc = update(actor, critic, opt_a, opt_c, batch, args.gamma, w if args.importance else None, **reg_kw)
                with torch.no_grad():
                    s, r, s2 = batch["states"], batch["rewards"], batch["next_states"]
                    replay.update_priorities(idx, (r + batch.get("discounts", args.gamma) * boot(s2) - critic(s)).abs())
                updates_done += 1
                if target_critic is not None:
                    sync_target_critic(args, target_critic, critic, updates_done)
        elif learner is None:
            for _ in range(args.updates):
                la, lc = update(actor, critic, opt_a, opt_c, replay.sample(args.batch), args.gamma, **reg_kw)
                updates_done += 1
                if target_critic is not None:
                    sync_target_critic(args, target_critic, critic, updates_done)
        else:
            rho_kw, views = ratio_kwargs(args, [rho_buf], [source])
            if views:                                                 # one ring: its view itself, not a list
                rho_stats["rho"] = views[0]
                rho_kw = {k: views[0] if k.endswith("_out") else v for k, v in rho_kw.items()}
            for _ in range(n_updates):
                la_t, lc_t, td_t = learner.update_from(source, args.batch, **importance_kwargs(args), **rho_kw)
                if means is not None:
                    means.add(views[0])
            la, lc = (float(la_t), float(lc_t)) if log else (la_t, lc_t)   # (NaN where the last update was stopped)
            if args.target_kl is not None:
                kl_skipped += learner.kl_state[1]                     # device tensors: read on printed lines only
                kl_stats["kl"] = learner.kl[0]
            if diag is not None:
                diag.update(entropy=learner.entropy(td_t.numel()).mean(), norms=learner.grad_norm)
            if args.publish == "host":
                actor.load_state_dict(learner.actor_state_dict())     # the rollout's actor: host pack, as sync_actor
        lp = float("nan")
        if pmi is not None:                                           # PMINetwork.train_pmi on this rollout's observations
            pmi.train()
            sel, _, _ = uavtrack.sample_pmi_pairs(res["obs"], args.n_uav, args.pmi_b2)
            for x12, x13 in uavtrack.pmi_batches(sel, args.pmi_batch):
                loss = uavtrack.pmi_contrastive_loss(pmi(x12), pmi(x13))
                opt_p.zero_grad(); loss.backward(); opt_p.step()
                lp = loss.detach()
            lp = float(lp) if log else lp
            if args.publish == "device":
                env.publish_pmi(pmi)                                  # folded and packed on the device, same bits
            else:
                env.set_pmi(pmi.state_dict())                         # eval-mode (running-stat) BatchNorm is what gets folded
        elif pmi_dev is not None:                                     # the same call, one library call on the device
            lp = pmi_dev.train_pmi({"pmi": {"batch_size": args.pmi_batch}}, res["obs"], args.n_uav, generator=pmi_gen,
                                   sync=False)
            lp = float(lp) if log else lp
            if args.publish == "device":
                pmi_dev.publish_pmi(env)                              # no copy to the host, no synchronisation
            else:
                env.set_pmi(pmi_dev)
        if args.publish == "host":
            rollout.sync_actor()                                      # new weights for the next rollout
        elif learner is not None:
            learner.publish_actor(env)                                # packed on the device: no copy, no synchronisation
        else:
            rollout.publish_actor()                                   # the CUDA ActorMLP, packed on the device
        ep = res["ep_sums"]                                           # [B, 5]: sum_t mean_i reward, 3 terms, covered
        history.append(ep[:, 0].mean() / K)                           # (a device scalar: read once, at the end)
        if not log:
            continue
        ret, cov = float(ep[:, 0].mean()) / K, float(ep[:, 4].mean()) / T
        six = drain([stats], kept)
        torch.cuda.synchronize()
        now = time.perf_counter()
        n_iter = it + 1 - (stamps[-1][0] if stamps else 0)           # iterations since the previous line
        stamps.append((it + 1, now))
        reg_field = regularisation_field(diag["entropy"], diag.get("norms")) if diag else ""
        if means is not None:
            reg_field += means.field()
        elif args.rho_bar is not None:
            reg_field += rho_field(rho_stats["rho"], args.rho_bar)
        elif args.ppo_clip is not None:
            reg_field += ratio_field(rho_stats["rho"], args.ppo_clip)
        if args.target_kl is not None:
            reg_field += kl_field(kl_stats["kl"], kl_skipped)
            kl_skipped.zero_()
        if args.normalise_advantage:
            reg_field += advantage_field(*((adv_stats["mean"], adv_stats["std"]) if learner is None else
                                           (learner.advantage_stats[0], learner.advantage_stats[2])))
        print(f"iter {it:3d}  episode return {ret:8.3f}  covered targets/step {cov:5.2f}  actor loss {la:+.4f}  "
              f"critic loss {lc:.4f}  {reg_field}pmi loss {lp:.4f}  rollout {t_roll * 1e3:6.1f} ms ({per_iter / t_roll / 1e9:.2f} G agent-steps/s)  "
              f"iteration {((now - t0) if args.log_every == 1 else (now - t_log) / n_iter) * 1e3:6.1f} ms  {six}", flush=True)
        t_log = now
    save_results(args, kept)
    if args.replay == "prioritized":
        replay.check()                                                # no draw was refused on the device
    if learner is not None and behavioural(args):
        learner.check()                                               # no update met a slot whose behaviour is unknown
    env.close()
    history = [float(r) for r in history]
    if timings is not None:
        timings.extend(stamps)
    return history


if __name__ == "__main__":
    main()
