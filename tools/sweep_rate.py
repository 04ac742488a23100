#!/usr/bin/env python3
"""Sweep rate: the sweep draw (uavtrack.RingSweep, uavtrack_replay_sample_sweep) against the uniform draw
(uavtrack_replay_sample_uniform) of the same ring at the same k, both from this build.

k = 65 536 rows; the sweep's window is the half of the ring one iteration of the example adds, 2 048 000 slots of
4 096 000 (1024 x 10 x 200) and 16 384 000 of 32 768 000 (4096 x 20 x 200), placed across the end of the ring so that
it wraps; the uniform draw ranges over the whole ring.  Each pair is timed eager and as a replayed graph of one call,
the draw alone and the draw plus DeviceActorCritic.update_from.

Every figure is a mean us per call over `reps` back-to-back calls between HIP events; the two paths alternate run by
run, after a warm-up of each, and a row reports the median of the runs and their range [min, max].

    python tools/sweep_rate.py [--quick] [--out FILE]     # FILE: the rows as one JSON list
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


def compare(sweep, uniform, reps, warm=3):
    """{sweep_us, uniform_us}: [median, min, max] over RUNS alternating windows of `reps` calls each."""
    for fn in (sweep, uniform):
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {"sweep_us": [], "uniform_us": []}
    for _ in range(RUNS):
        t["sweep_us"].append(window(sweep, reps))
        t["uniform_us"].append(window(uniform, reps))
    out = {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in t.items()}
    out["sweep_over_uniform"] = round(out["sweep_us"][0] / out["uniform_us"][0], 3)
    return out


def captured(fn):
    """fn as the replay of a graph that holds one call of it."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def rows_for(count, k, reps):
    ring = uavtrack.ReplayRing(count, DEV, seed=1, max_batch=k)
    g = torch.Generator(device=DEV).manual_seed(0)
    ring.store["states"].copy_(torch.randn(count, 12, device=DEV, generator=g))
    ring.store["next_states"].copy_(torch.randn(count, 12, device=DEV, generator=g))
    ring.store["actions"].copy_(torch.randint(0, 12, (count,), device=DEV, generator=g, dtype=torch.int32))
    ring.store["rewards"].copy_(torch.randn(count, device=DEV, generator=g))
    ring.count = count
    W = count // 2
    sweep = ring.sweep(k, (count - W // 2, W))                        # half the ring, across its end
    torch.manual_seed(0)
    learner = uavtrack.DeviceActorCritic(12, 128, 12, 1e-4, 5e-4, 0.95, DEV, max_batch=k)
    pairs = (("draw", lambda: sweep._draw_batch(k), lambda: ring._draw_batch(k)),
             ("draw + update_from", lambda: learner.update_from(sweep, k), lambda: learner.update_from(ring, k)))
    rows = []
    for what, s, u in pairs:
        for mode in ("eager", "graph"):
            fs, fu = (s, u) if mode == "eager" else (captured(s), captured(u))
            rows.append({"what": what, "mode": mode, "count": count, "window": W, "k": k, "reps": reps, "runs": RUNS,
                         **compare(fs, fu, reps)})
            print(json.dumps(rows[-1]), flush=True)
    learner.check()
    ring.check()
    sweep.seek(0)
    epoch = torch.cat([sweep.draw() for _ in range(sweep.minibatches)])
    assert epoch.unique().numel() == epoch.numel() and bool((((epoch - sweep.window[0]) % count) < W).all())
    ring.close()
    learner.close()
    del ring, sweep, learner
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sweep_rate.py measures on the MI355X"
    if args.quick:
        rows = rows_for(1 << 16, 1024, 5)
    else:
        rows = rows_for(2 * 1024 * 10 * 200, 65536, 50) + rows_for(2 * 4096 * 20 * 200, 65536, 50)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
