#!/usr/bin/env python3
"""Multi-step targets, what they cost: the n-step ring add against the one-step episodes add on the same launch's
outputs, and update_from with a discount store against without.

add: one 1024 envs x 10 UAVs x 200 steps rollout (done fired once, mid-rollout, with its start_obs) into a ring of twice
that size; uavtrack_replay_add_rollout_episodes (a plain ring) against uavtrack_replay_add_rollout_nstep at n_step 1, 3
and 8 (ring.with_nstep).  Expectation: the n-step add reads up to n - 1 more reward lines per transition and one
displaced obs row (each obs row is read twice, as a state and as a next state, where the one-step kernel reads it once).
update: DeviceActorCritic.update_from at n = 65 536, H = 128 from a uniform ring of 2 M slots, with a discount store
(one more float load per batch row) and without.
The compared calls alternate; each figure is the median of 7 runs of back-to-back calls between HIP events.

    python tools/nstep_rate.py [--quick] [--out FILE]     # FILE: the rows as one JSON list
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd")]

import torch  # noqa: E402
import uavtrack  # noqa: E402

DEV = "cuda:0"
GAMMA = 0.95


def once(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternating(calls, reps, runs=7):
    """{name: (median us, [runs])} of several calls, run in turn `runs` times."""
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            ts[k].append(once(fn, reps))
    return {k: (statistics.median(v), sorted(v)) for k, v in ts.items()}


def add_rows(B, N, T, prioritised):
    g = torch.Generator(device=DEV).manual_seed(0)
    obs_in = torch.randn(B, N, 12, device=DEV, generator=g)
    done = torch.zeros(T, B, dtype=torch.uint8, device=DEV)
    done[T // 2] = 1
    out = {"obs": torch.randn(T, B, N, 12, device=DEV, generator=g),
           "actions": torch.randint(0, 12, (T, B, N), device=DEV, generator=g, dtype=torch.int32),
           "reward": torch.randn(T, B, N, device=DEV, generator=g), "done": done,
           "start_obs": torch.randn(T, B, N, 12, device=DEV, generator=g)}
    n = T * B * N
    make = (lambda: uavtrack.PrioritizedReplayRing(2 * n, DEV, seed=1)) if prioritised \
        else (lambda: uavtrack.ReplayRing(2 * n, DEV, seed=1))
    rings = {"episodes": make()}
    for k in (1, 3, 8):
        rings[f"n_step_{k}"] = make().with_nstep(k, GAMMA)
    res = alternating({name: (lambda r=r: r.add_rollout(obs_in, out)) for name, r in rings.items()}, reps=10)
    row = {"what": "add_rollout", "ring": "prioritised" if prioritised else "uniform", "envs": B, "n_uav": N, "steps": T,
           "transitions": n}
    for name, (med, runs) in res.items():
        row[name + "_us"] = round(med, 1)
        row[name + "_runs_us"] = [round(x, 1) for x in runs]
    print(json.dumps(row), flush=True)
    for r in rings.values():
        r.close()
    return row


def update_row(n, H, slots):
    g = torch.Generator(device=DEV).manual_seed(0)
    rings = {"plain": uavtrack.ReplayRing(slots, DEV, seed=1, max_batch=n),
             "discounted": uavtrack.ReplayRing(slots, DEV, seed=1, max_batch=n).with_nstep(3, GAMMA)}
    for r in rings.values():
        r.store["states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
        r.store["next_states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
        r.store["actions"].copy_(torch.randint(0, 12, (slots,), device=DEV, generator=g, dtype=torch.int32))
        r.store["rewards"].copy_(torch.rand(slots, device=DEV, generator=g) * 4 - 2)
        r.pos, r.count = 0, slots
    rings["discounted"].discounts.copy_(torch.rand(slots, device=DEV, generator=g))
    learners = {k: uavtrack.DeviceActorCritic(12, H, 12, 1e-4, 5e-4, GAMMA, DEV, max_batch=n) for k in rings}
    res = alternating({k: (lambda k=k: learners[k].update_from(rings[k], n)) for k in rings}, reps=50)
    row = {"what": "update_from", "n": n, "H": H, "slots": slots}
    for name, (med, runs) in res.items():
        row[name + "_us"] = round(med, 1)
        row[name + "_runs_us"] = [round(x, 1) for x in runs]
    print(json.dumps(row), flush=True)
    for x in list(learners.values()) + list(rings.values()):
        x.check()
        x.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nstep_rate.py measures on the MI355X"
    if args.quick:
        rows = [add_rows(64, 10, 20, False), update_row(4096, 128, 1 << 16)]
    else:
        rows = [add_rows(1024, 10, 200, False), add_rows(1024, 10, 200, True), update_row(65536, 128, 1 << 21)]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
