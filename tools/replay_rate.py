#!/usr/bin/env python3
"""Prioritised replay rate: uavtrack.PrioritizedReplayRing's draw and add_rollout (HIP) against the PyTorch path
(PrioritizedDeviceReplayBuffer: torch.multinomial over fp32 probabilities; transitions_from_rollout + add).

draw: count in {1 M, 2^24 - 8, 2^25} x k in {2000, 2048, 4000}, indices + importance weights, eager (HIP events around
50 back-to-back calls) and graph-replayed (one captured call, replayed 50 times); the torch path where torch can run
it (count <= 2^24).  Bound: the draw reads at least the 4 B priority of every slot once (the per-tile sums).
add: one 4096 x 20 x 200 rollout into a 2^25 ring.  Bound: reads obs_in + obs + actions + reward once plus the 4 B
priorities (the maximum), writes states + next_states (2 x 48 B) + action + reward + priority per transition.
Bounds use HBM_TBS below; each figure is the median of 5 runs.

    python tools/replay_rate.py [--quick] [--out FILE]     # FILE: the rows as one JSON list
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

HBM_TBS = 6.3          # the stream rate the bounds assume, TB/s (6.9 write-only, 4.75 copy)
DEV = "cuda:0"


def timed(fn, reps=50, runs=5):
    """Median over `runs` of the mean us per call of `reps` back-to-back calls, HIP events around them."""
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out)


def torch_draw(prio, count, k, alpha=0.6, beta=0.4):
    """PrioritizedDeviceReplayBuffer.sample without the gather."""
    prob = prio[:count] ** alpha
    prob = prob / prob.sum()
    idx = torch.multinomial(prob, k, replacement=True)
    w = (count * prob[idx]) ** (-beta)
    return idx, w / w.max()


def draw_rows(counts, ks):
    rows = []
    for count in counts:
        ring = uavtrack.PrioritizedReplayRing(count, DEV, seed=1, max_batch=max(ks))
        g = torch.Generator(device=DEV).manual_seed(0)
        ring.priorities.copy_(torch.rand(count, device=DEV, generator=g) + 0.01)
        ring.count = count
        for k in ks:
            idx = torch.empty(k, dtype=torch.int64, device=DEV)
            w = torch.empty(k, device=DEV)
            call = lambda: ring._draw(k, 0.4, idx, w)   # noqa: E731
            for _ in range(3):
                call()
            eager = timed(call)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call()
            graph.replay()
            replayed = timed(graph.replay)
            tt = None
            if count <= 1 << 24:
                for _ in range(3):
                    torch_draw(ring.priorities, count, k)
                tt = timed(lambda: torch_draw(ring.priorities, count, k))
            ring.check()
            bound = count * 4 / (HBM_TBS * 1e12) * 1e6
            rows.append({"what": "draw", "count": count, "k": k, "hip_eager_us": round(eager, 1),
                         "hip_graph_us": round(replayed, 1), "torch_us": None if tt is None else round(tt, 1),
                         "bound_us": round(bound, 1), "bytes": count * 4})
            print(json.dumps(rows[-1]), flush=True)
        ring.close()
        del ring
        torch.cuda.empty_cache()
    return rows


def add_row(B, N, T, cap):
    M = B * N
    g = torch.Generator(device=DEV).manual_seed(0)
    obs_in = torch.randn(B, N, 12, device=DEV, generator=g)
    out = {"obs": torch.randn(T, B, N, 12, device=DEV, generator=g),
           "actions": torch.randint(0, 12, (T, B, N), device=DEV, generator=g, dtype=torch.int32),
           "reward": torch.randn(T, B, N, device=DEV, generator=g)}
    ring = uavtrack.PrioritizedReplayRing(cap, DEV, seed=1)
    hip = timed(lambda: ring.add_rollout(obs_in, out), reps=5)
    ring.close()
    del ring
    torch.cuda.empty_cache()
    ref = uavtrack.PrioritizedDeviceReplayBuffer(cap, DEV)
    ref.add(uavtrack.transitions_from_rollout(obs_in, out))
    tt = timed(lambda: ref.add(uavtrack.transitions_from_rollout(obs_in, out)), reps=5)
    n = T * M
    rd = M * 48 + n * (48 + 4 + 4) + cap * 4
    wr = min(n, cap) * (2 * 48 + 4 + 4 + 4)
    row = {"what": "add_rollout", "transitions": n, "capacity": cap, "hip_us": round(hip, 1), "torch_us": round(tt, 1),
           "read_bytes": rd, "write_bytes": wr, "bound_us": round((rd + wr) / (HBM_TBS * 1e12) * 1e6, 1)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "replay_rate.py measures on the MI355X"
    if args.quick:
        rows = draw_rows([1 << 20], [2000]) + [add_row(64, 20, 20, 1 << 16)]
    else:
        rows = draw_rows([1 << 20, (1 << 24) - 8, 1 << 25], [2000, 2048, 4000]) + [add_row(4096, 20, 200, 1 << 25)]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
