#!/usr/bin/env python3
"""What the per-episode results cost: EpisodeStats.add (uavtrack_episode_stats_add: step sums, done scan, fold) on one
200-step rollout, next to two yardsticks taken in the same run:

  floor   the bytes the add must read (16 per agent-step: reward and the three terms) at 8 TB/s;
  torch   the same six results from the same tensors with torch ops on the device -- means over the UAVs, the sum over
          the steps, the maximum over the steps -- which is the only other way to get them, and only for launches
          that hold exactly one episode.

Each figure is GPU time per call: HIP events around a captured graph of --reps back-to-back calls (no host launch cost
in it), the median of 5 replays.  Shapes: 4096 x 20 and 1024 x 10, T = 200.  The done flags close every episode at the
last step, so each add also writes B records.

    python tools/episode_stats_rate.py
Prints a table and one JSON line; exits non-zero if the add is not faster than the torch formulation at every shape."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "marl-uavs-targets-tracking_amd")]

import torch  # noqa: E402
import uavtrack  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12


def torch_results(out, T):
    """The six results of train.py:187-192 for a launch that is one episode per environment."""
    ret = out["reward"].mean(dim=2).sum(dim=0) / T
    terms = out["terms"].mean(dim=3).sum(dim=0) / T
    cov = out["covered"]
    return ret, terms, cov.sum(dim=0).to(torch.float64) / T, cov.max(dim=0).values


def graph_us(fn, reps, before=None):
    """GPU microseconds per call of fn: a graph of `reps` calls replayed between two events, median of 5."""
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    if before:
        before()
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) / reps * 1e3)
    del g
    return statistics.median(us)


def one_shape(B, N, T, reps):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(B + N)
    out = dict(reward=torch.rand(T, B, N, device=DEV, generator=gen) * 2 - 1,
               terms=torch.rand(T, 3, B, N, device=DEV, generator=gen) * 2 - 1,
               covered=torch.randint(0, N + 1, (T, B), device=DEV, generator=gen, dtype=torch.int32),
               done=torch.zeros(T, B, dtype=torch.uint8, device=DEV))
    out["done"][-1] = 1
    stats = uavtrack.EpisodeStats((B, N), log_capacity=reps * B, max_steps=T, device=DEV)
    add_us = graph_us(lambda: stats.add(out), reps, before=stats.clear)
    res = stats.read()
    assert len(res["return_list"]) == reps * B and res["dropped"] == 0
    # the two formulations agree (fp32 tree sums against fp64 ordered ones: a loose look, the tests do the exact one)
    ret, _, avg, mx = torch_results(out, T)
    assert abs(float(ret[0]) - res["return_list"][0]) < 1e-5 and float(avg[0]) == res["average_covered_targets_list"][0]
    assert float(mx[0]) == res["max_covered_targets_list"][0]
    torch_us = graph_us(lambda: torch_results(out, T), reps)
    stats.destroy()
    nbytes = 16 * B * N * T
    return dict(B=B, N=N, T=T, add_us=add_us, torch_us=torch_us, bytes=nbytes, floor_us=nbytes / HBM_BYTES_PER_S * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    out = dict(device=props.name, arch=getattr(props, "gcnArchName", ""), reps=args.reps, shapes=[])
    print(f"{'B':>6} {'N':>4} {'T':>4} {'MB read':>8} {'8 TB/s floor us':>16} {'add us':>9} {'torch us':>9} {'torch / add':>12}")
    for B, N in ((4096, 20), (1024, 10)):
        r = one_shape(B, N, 200, args.reps)
        out["shapes"].append(r)
        print(f"{B:6d} {N:4d} {r['T']:4d} {r['bytes'] / 1e6:8.1f} {r['floor_us']:16.1f} {r['add_us']:9.1f} {r['torch_us']:9.1f} "
              f"{r['torch_us'] / r['add_us']:12.2f}", flush=True)
    print(json.dumps(out))
    if not all(r["add_us"] < r["torch_us"] for r in out["shapes"]):
        sys.exit("EpisodeStats.add is not faster than the torch formulation at every shape")


if __name__ == "__main__":
    main()
