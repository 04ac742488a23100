#!/usr/bin/env python3
"""TD(lambda) targets, what they cost: the critic-forward kernel over a rollout's rows, the lambda ring add against the
one-step episodes add and the n-step add at n = 8 on the same launch's outputs, and update_from from a lambda ring
against a plain ring.

values: DeviceActorCritic.values over the [T*B*N][12] observation rows of one rollout, H = 128.  Per row the kernel reads
48 bytes, writes 4 and issues 26 H flops (13 fused operations per hidden unit: 12 of layer 1, one of layer 2); the row prints
its share of the 157 TF fp32 vector peak and of the 8 TB/s HBM rate beside the time.
add: one envs x n_uav x 200 steps rollout (done fired once, mid-rollout, with its start_obs) into a ring of twice that
size; uavtrack_replay_add_rollout_episodes (a plain ring), uavtrack_replay_add_rollout_nstep at n_step 8 and
uavtrack_replay_add_rollout_lambda (values given, so the add alone is timed).  The lambda add is the episodes add's write
followed by the scan: one thread per agent chain, 200 dependent steps, the loads eight steps ahead.
update: DeviceActorCritic.update_from at n = 65 536, H = 128 from a uniform ring of 2 M slots, lambda ring against plain.
The compared calls alternate; each figure is the median of 7 runs of back-to-back calls between HIP events.

    python tools/lambda_rate.py [--quick] [--out FILE]     # FILE: the rows as one JSON list
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402
import uavtrack  # noqa: E402
from nstep_rate import DEV, GAMMA, alternating  # noqa: E402

LAMBDA = 0.9
PEAK_FP32_VECTOR = 157e12
PEAK_HBM = 8e12


def put(row, res):
    for name, (med, runs) in res.items():
        row[name + "_us"] = round(med, 1)
        row[name + "_runs_us"] = [round(x, 1) for x in runs]
    print(json.dumps(row), flush=True)
    return row


def rollout(B, N, T):
    g = torch.Generator(device=DEV).manual_seed(0)
    obs_in = torch.randn(B, N, 12, device=DEV, generator=g)
    done = torch.zeros(T, B, dtype=torch.uint8, device=DEV)
    done[T // 2] = 1
    out = {"obs": torch.randn(T, B, N, 12, device=DEV, generator=g),
           "actions": torch.randint(0, 12, (T, B, N), device=DEV, generator=g, dtype=torch.int32),
           "reward": torch.randn(T, B, N, device=DEV, generator=g), "done": done,
           "start_obs": torch.randn(T, B, N, 12, device=DEV, generator=g)}
    return obs_in, out


def values_row(obs, H):
    n = obs.numel() // 12
    learner = uavtrack.DeviceActorCritic(12, H, 12, 1e-4, 5e-4, GAMMA, DEV, max_batch=64)
    v = torch.empty(n, device=DEV)
    res = alternating({"values": lambda: learner.values(obs, out=v)}, reps=10)
    us = res["values"][0]
    row = {"what": "values", "rows": n, "H": H, "flops": 26 * H * n, "bytes": 52 * n,
           "share_of_fp32_vector_peak": round(26 * H * n / (us * 1e-6) / PEAK_FP32_VECTOR, 3),
           "share_of_hbm_rate": round(52 * n / (us * 1e-6) / PEAK_HBM, 3)}
    learner.check()
    learner.close()
    return put(row, res)


def add_rows(B, N, T, prioritised):
    obs_in, out = rollout(B, N, T)
    n = T * B * N
    make = (lambda: uavtrack.PrioritizedReplayRing(2 * n, DEV, seed=1)) if prioritised \
        else (lambda: uavtrack.ReplayRing(2 * n, DEV, seed=1))
    rings = {"episodes": make(), "n_step_8": make().with_nstep(8, GAMMA), "lambda": make().with_lambda(LAMBDA, GAMMA)}
    vals = torch.randn(T, B, N, device=DEV)
    calls = {name: (lambda r=r: r.add_rollout(obs_in, out)) for name, r in rings.items() if name != "lambda"}
    calls["lambda"] = lambda: rings["lambda"].add_rollout(obs_in, out, values=vals)
    row = {"what": "add_rollout", "ring": "prioritised" if prioritised else "uniform", "envs": B, "n_uav": N, "steps": T,
           "transitions": n}
    put(row, alternating(calls, reps=10))
    for r in rings.values():
        r.close()
    return row


def update_row(n, H, slots):
    g = torch.Generator(device=DEV).manual_seed(0)
    rings = {"plain": uavtrack.ReplayRing(slots, DEV, seed=1, max_batch=n),
             "lambda": uavtrack.ReplayRing(slots, DEV, seed=1, max_batch=n).with_lambda(LAMBDA, GAMMA)}
    for r in rings.values():
        r.store["states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
        r.store["next_states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
        r.store["actions"].copy_(torch.randint(0, 12, (slots,), device=DEV, generator=g, dtype=torch.int32))
        r.store["rewards"].copy_(torch.rand(slots, device=DEV, generator=g) * 4 - 2)
        r.pos, r.count = 0, slots
    learners = {k: uavtrack.DeviceActorCritic(12, H, 12, 1e-4, 5e-4, GAMMA, DEV, max_batch=n) for k in rings}
    res = alternating({k: (lambda k=k: learners[k].update_from(rings[k], n)) for k in rings}, reps=50)
    row = put({"what": "update_from", "n": n, "H": H, "slots": slots}, res)
    for x in list(learners.values()) + list(rings.values()):
        x.check()
        x.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lambda_rate.py measures on the MI355X"
    rows = []
    if args.quick:
        rows += [values_row(rollout(64, 10, 20)[1]["obs"], 128), add_rows(64, 10, 20, False), update_row(4096, 128, 1 << 16)]
    else:
        for B, N in ((1024, 10), (4096, 20)):
            rows.append(values_row(rollout(B, N, 200)[1]["obs"], 128))
            rows += [add_rows(B, N, 200, False), add_rows(B, N, 200, True)]
        rows.append(update_row(65536, 128, 1 << 21))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
