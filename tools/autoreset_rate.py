#!/usr/bin/env python3
"""What the in-launch episode turnover of the fused actor rollout buys: `--episodes` (10) episodes of `--horizon` (200)
steps at 1024 x 10 x 10 and 4096 x 20 x 10 (MAAC rewards, actor width 128), measured two ways for the same work --

    autoreset   ONE uavtrack_run_actor_autoreset launch of episodes * horizon steps (with the start_obs output)
    loop        today's loop: per episode uavtrack_reset, the copy of its observation into the driver's buffer, and one
                uavtrack_run_actor launch of horizon steps (bound calls: no per-call Python beyond the ctypes call)

-- and both forms of the ring add on the auto-reset result (episodes * horizon * B * N transitions into a ring that
holds them all): uavtrack_replay_add_rollout and uavtrack_replay_add_rollout_episodes.  Protocol: warm-up, then HIP
events around `--reps` back-to-back repetitions, median of 5 runs.  One JSON line per measurement, times in ms.
Records, gates nothing.

    python tools/autoreset_rate.py [--reps N] [--episodes E] [--horizon H]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd")]

import torch  # noqa: E402
import uavtrack  # noqa: E402

DEV = "cuda:0"
SHAPES = ((1024, 10, 10), (4096, 20, 10))


def timed(fn, reps, runs=5):
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return sorted(ts)[len(ts) // 2], [round(t, 3) for t in ts]


def measure(B, N, M, E, H, reps):
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=0.0, reward_mode=uavtrack.RewardMode.RAW, horizon=H)
    env = uavtrack.BatchedUavEnv(cfg, DEV)
    torch.manual_seed(0)
    env.set_actor(uavtrack.ActorMLP(hidden_dim=128, action_dim=cfg.na_total))
    obs = env.reset(seed=1).clone()
    T = E * H
    agent_steps = B * N * T

    def line(what, ms, runs, **kw):
        print(json.dumps(dict(what=what, envs=B, n_uav=N, m_targets=M, episodes=E, horizon=H, ms=round(ms, 3), runs_ms=runs,
                              **kw)), flush=True)

    # one launch across the E episodes
    big = env.run_actor(T, obs, seed=3, auto_reset_seed=1, want_start_obs=True)
    one = env.bind_run(T, big, "actor", obs_in=obs, seed=3, auto_reset_seed=1, want_start_obs=True)
    one(); torch.cuda.synchronize()
    ms, runs = timed(one, reps)
    line("autoreset", ms, runs, g_agent_steps_per_s=round(agent_steps / ms / 1e6, 2))

    # the loop it replaces
    small = env.run_actor(H, obs, seed=3)
    reset = env.bind_reset(1, obs)
    per_episode = env.bind_run(H, small, "actor", obs_in=obs, seed=3)

    def loop():
        for e in range(E):
            reset(e)                # (writes the driver's obs buffer in place: the copy of the loop is this write)
            per_episode()
    loop(); torch.cuda.synchronize()
    ms_loop, runs = timed(loop, reps)
    line("loop", ms_loop, runs, g_agent_steps_per_s=round(agent_steps / ms_loop / 1e6, 2), loop_over_autoreset=round(ms_loop / ms, 3))

    # the two ring adds on the big result
    n = T * B * N
    ring = uavtrack.PrioritizedReplayRing(n, DEV, seed=0, max_batch=1024)
    plain = {k: big[k] for k in ("obs", "actions", "reward")}
    for what, out in (("add_rollout", plain), ("add_rollout_episodes", big)):
        fn = lambda: ring.add_rollout(obs, out)
        fn(); torch.cuda.synchronize()
        ms_add, runs = timed(fn, max(1, reps // 2))
        line(what, ms_add, runs, transitions=n, gb_per_s=round(n * (2 * 48 + 8) * 2 / ms_add / 1e6, 1))
    env.set_start_obs_output(None)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=200)
    args = ap.parse_args()
    for B, N, M in SHAPES:
        measure(B, N, M, args.episodes, args.horizon, args.reps)


if __name__ == "__main__":
    main()
