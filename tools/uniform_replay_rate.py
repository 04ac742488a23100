#!/usr/bin/env python3
"""Uniform replay rate: uavtrack.ReplayRing (HIP draw and add_rollout) against the plain-PyTorch DeviceReplayBuffer path
(torch.randperm(count)[:k]; transitions_from_rollout + add), both from this build.

update: one draw of k = 65 536 rows plus DeviceActorCritic.update_from, on rings holding 4 096 000 slots (the example's
default: 2 x 1024 x 10 x 200) and 32 768 000 slots (the headline batch: 2 x 4096 x 20 x 200); the draw alone is timed
too.  Both buffers read the same stores.
add: one 200-step rollout of 1024 x 10 and of 4096 x 20 into a ring of twice its size: add_rollout against
add(transitions_from_rollout(...)).

Every figure is a mean us per call over `reps` back-to-back calls between HIP events; the two paths alternate run by
run, after a warm-up of each, and a row reports the median of the runs and their range [min, max].

    python tools/uniform_replay_rate.py [--quick] [--out FILE]     # FILE: the rows as one JSON list
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
RUNS = 7


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def compare(hip, ref, reps, warm=3):
    """{hip_us, torch_us}: [median, min, max] over RUNS alternating windows of `reps` calls each."""
    for fn in (hip, ref):
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {"hip_us": [], "torch_us": []}
    for _ in range(RUNS):
        t["hip_us"].append(window(hip, reps))
        t["torch_us"].append(window(ref, reps))
    out = {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in t.items()}
    out["torch_over_hip"] = round(out["torch_us"][0] / out["hip_us"][0], 2)
    return out


def update_rows(count, k, reps):
    ring = uavtrack.ReplayRing(count, DEV, seed=1, max_batch=k)
    g = torch.Generator(device=DEV).manual_seed(0)
    ring.store["states"].copy_(torch.randn(count, 12, device=DEV, generator=g))
    ring.store["next_states"].copy_(torch.randn(count, 12, device=DEV, generator=g))
    ring.store["actions"].copy_(torch.randint(0, 12, (count,), device=DEV, generator=g, dtype=torch.int32))
    ring.store["rewards"].copy_(torch.randn(count, device=DEV, generator=g))
    ring.count = count
    ref = uavtrack.DeviceReplayBuffer(1, DEV)
    ref.store, ref.capacity, ref.count = ring.store, count, count          # the same rows behind both draws
    torch.manual_seed(0)
    learner = uavtrack.DeviceActorCritic(12, 128, 12, 1e-4, 5e-4, 0.95, DEV, max_batch=k)
    rows = []
    for what, hip, tor in (("draw", lambda: ring._draw_batch(k), lambda: torch.randperm(count, device=DEV)[:k]),
                           ("draw + update_from", lambda: learner.update_from(ring, k),
                            lambda: learner.update_from(ref, k))):
        rows.append({"what": what, "count": count, "k": k, "reps": reps, "runs": RUNS, **compare(hip, tor, reps)})
        print(json.dumps(rows[-1]), flush=True)
    learner.check()
    ring.check()
    idx = ring.draw(k)
    assert idx.unique().numel() == k and int(idx.max()) < count
    ring.close()
    learner.close()
    del ring, ref, learner
    torch.cuda.empty_cache()
    return rows


def add_row(B, N, T, reps):
    g = torch.Generator(device=DEV).manual_seed(0)
    obs_in = torch.randn(B, N, 12, device=DEV, generator=g)
    out = {"obs": torch.randn(T, B, N, 12, device=DEV, generator=g),
           "actions": torch.randint(0, 12, (T, B, N), device=DEV, generator=g, dtype=torch.int32),
           "reward": torch.randn(T, B, N, device=DEV, generator=g)}
    n = T * B * N
    ring = uavtrack.ReplayRing(2 * n, DEV, seed=1)
    ref = uavtrack.DeviceReplayBuffer(2 * n, DEV)
    row = {"what": "add", "envs": B, "n_uav": N, "steps": T, "transitions": n, "capacity": 2 * n, "reps": reps,
           "runs": RUNS, **compare(lambda: ring.add_rollout(obs_in, out),
                                   lambda: ref.add(uavtrack.transitions_from_rollout(obs_in, out)), reps, warm=2)}
    for key in ring.store:
        assert (ring.pos, ring.count) == (ref.pos, ref.count) and torch.equal(ring.store[key], ref.store[key]), key
    print(json.dumps(row), flush=True)
    ring.close()
    del ring, ref, out
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "uniform_replay_rate.py measures on the MI355X"
    if args.quick:
        rows = update_rows(1 << 16, 1024, 5) + [add_row(64, 10, 20, 2)]
    else:
        rows = update_rows(2 * 1024 * 10 * 200, 65536, 50) + update_rows(2 * 4096 * 20 * 200, 65536, 50) \
            + [add_row(1024, 10, 200, 10), add_row(4096, 20, 200, 10)]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
