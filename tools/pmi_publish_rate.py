#!/usr/bin/env python3
"""What publishing the trained PMI network to the MAAC-R scorer costs, host path against device path.

  (a) device publish (DevicePMINetwork.publish_pmi: uavtrack_pmi_trainer_publish, three launches): GPU time by HIP events
      around --reps eager calls, wall time per call including a synchronisation, and the host time of the call alone;
  (b) the host path (BatchedUavEnv.set_pmi(trainer): state to the host, numpy fold, host pack, upload, stream
      synchronisations): wall time per call, and GPU time between events around the same calls;
      each figure is the median of --runs runs of --reps calls, at --hidden 64 128 256;
  (c) examples/train_maac.py --method maac-r --pmi-trainer device --learner device --replay prioritized per-iteration wall
      time, --publish host against --publish device, the mean over --iters iterations between two synchronised stamps,
      after one warm-up stretch.

    python tools/pmi_publish_rate.py                  # everything
    python tools/pmi_publish_rate.py --skip-loop      # (a) and (b) only
Each GPU step belongs under a time limit of its own (`timeout -k 10 300 python tools/pmi_publish_rate.py --skip-loop &&
timeout -k 10 600 python tools/pmi_publish_rate.py --hidden --loop-envs 1024`).  Prints a table and one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "marl-uavs-targets-tracking_amd"), os.path.join(ROOT, "examples")]

import torch  # noqa: E402
import uavtrack  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    """(GPU ms between events around reps calls, wall s of the calls and a final synchronisation, wall s of the calls alone)"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    t1 = time.perf_counter()
    b.synchronize()
    t2 = time.perf_counter()
    return a.elapsed_time(b), t2 - t0, t1 - t0


def publish_costs(H, reps, runs):
    env = uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=4, n_uav=4, m_targets=4), DEV)
    torch.manual_seed(H)
    net = uavtrack.DevicePMINetwork(H, 256, DEV)
    rows = torch.randn(48, 12, device=DEV)
    net.train_pmi({"pmi": {"batch_size": 64}}, rows, 4)
    env.set_pmi(net)
    for _ in range(3):
        net.publish_pmi(env)
    dev = [timed(lambda: net.publish_pmi(env), reps) for _ in range(runs)]
    host = [timed(lambda: env.set_pmi(net), reps) for _ in range(runs)]
    env.close()
    med = lambda rs, k, f: statistics.median(r[k] for r in rs) * f / reps
    return dict(H=H, device_gpu_us=med(dev, 0, 1e3), device_wall_us=med(dev, 1, 1e6), device_call_us=med(dev, 2, 1e6),
                host_gpu_us=med(host, 0, 1e3), host_wall_us=med(host, 1, 1e6))


def loop_cost(envs, publish, iters):
    import train_maac
    stamps = []
    argv = ["--envs", str(envs), "--n-uav", "10", "--steps", "200", "--method", "maac-r", "--pmi-trainer", "device",
            "--learner", "device", "--replay", "prioritized", "--publish", publish, "--iters", str(2 * iters),
            "--log-every", str(iters)]
    with contextlib.redirect_stdout(io.StringIO()):
        train_maac.main(argv, timings=stamps)
    (n0, t0), (n1, t1) = stamps[0], stamps[1]          # the first stretch warms up; the second is measured
    return dict(envs=envs, publish=publish, iteration_ms=(t1 - t0) / (n1 - n0) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="(c): measured iterations per run (after as many warm-up ones)")
    ap.add_argument("--loop-envs", type=int, nargs="*", default=[1024])
    ap.add_argument("--skip-loop", action="store_true")
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    out = dict(device=props.name, arch=getattr(props, "gcnArchName", ""), publish=[], loop=[])
    if args.hidden:
        print(f"{'H':>5} {'device GPU us':>14} {'device wall us':>15} {'device call us':>15} {'host GPU us':>12} {'host wall us':>13}")
    for H in args.hidden:
        r = publish_costs(H, args.reps, args.runs)
        out["publish"].append(r)
        print(f"{H:5d} {r['device_gpu_us']:14.1f} {r['device_wall_us']:15.1f} {r['device_call_us']:15.1f} "
              f"{r['host_gpu_us']:12.1f} {r['host_wall_us']:13.1f}", flush=True)
    if not args.skip_loop:
        print(f"\ntrain_maac --method maac-r, device trainers, prioritised ring, 10 UAVs x 200 steps, {args.iters} iterations measured")
        for envs in args.loop_envs:
            for publish in ("host", "device"):
                r = loop_cost(envs, publish, args.iters)
                out["loop"].append(r)
                print(f"  {envs:5d} envs  --publish {publish:6s}  {r['iteration_ms']:8.2f} ms / iteration", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
