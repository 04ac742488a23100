#!/usr/bin/env python3
"""What publishing the learner's actor weights to the rollout costs, host path against device path.

  (a) device publish (BatchedUavEnv.publish_actor: uavtrack_publish_actor_weights, two launches), GPU time by HIP events
      around a captured graph of --reps publishes (no host launch cost in the figure), and the eager call's host time;
  (b) the host path (BatchedUavEnv.set_actor from CUDA tensors: copy to the host, host pack, upload, two stream
      synchronisations), wall time per call;
  (c) examples/train_maac.py per-iteration wall time, device learner, prioritised ring, --publish host against
      --publish device (the device run issues no synchronisation between its printed lines), at 1024 and 4096 envs x
      10 UAVs x 200 steps: the mean over --iters iterations between two synchronised stamps, after one warm-up stretch.

    python tools/publish_rate.py                  # everything
    python tools/publish_rate.py --skip-loop      # (a) and (b) only
Prints a table and one JSON line."""
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


def make_env(A):
    kw = {} if A == 12 else dict(dim=3, na=12, nc=A // 12, z_max=300.0)
    return uavtrack.BatchedUavEnv(uavtrack.EnvConfig(n_envs=4, n_uav=4, m_targets=4, **kw), DEV)


def publish_costs(H, A, reps):
    env = make_env(A)
    torch.manual_seed(H + A)
    actor = uavtrack.ActorMLP(hidden_dim=H, action_dim=A).to(DEV)
    sd = {k: v.detach() for k, v in actor.state_dict().items()}
    env.set_actor(sd)
    for _ in range(3):
        env.publish_actor(sd)
    torch.cuda.synchronize()
    # (a) GPU time: a graph of `reps` publishes, replayed between two events
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        env.publish_actor(sd)
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            env.publish_actor(sd)
    g.replay()
    torch.cuda.synchronize()
    gpu = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        gpu.append(a.elapsed_time(b) / reps * 1e3)
    # eager call: host time of the call itself (enqueue only), then of the call + a synchronisation
    host_enqueue, eager_sync = [], []
    for _ in range(reps):
        t = time.perf_counter()
        env.publish_actor(sd)
        host_enqueue.append((time.perf_counter() - t) * 1e6)
        torch.cuda.synchronize()
    for _ in range(reps):
        t = time.perf_counter()
        env.publish_actor(sd)
        torch.cuda.synchronize()
        eager_sync.append((time.perf_counter() - t) * 1e6)
    # (b) host path from the same CUDA tensors
    host_path = []
    for _ in range(reps):
        t = time.perf_counter()
        env.set_actor(sd)
        host_path.append((time.perf_counter() - t) * 1e6)
    del g
    env.close()
    return dict(H=H, A=A, device_gpu_us=statistics.median(gpu), device_call_us=statistics.median(host_enqueue),
                device_call_sync_us=statistics.median(eager_sync), host_set_actor_us=statistics.median(host_path))


def loop_cost(envs, publish, iters):
    import train_maac
    stamps = []
    argv = ["--envs", str(envs), "--n-uav", "10", "--steps", "200", "--learner", "device", "--replay", "prioritized",
            "--publish", publish, "--iters", str(2 * iters), "--log-every", str(iters)]
    with contextlib.redirect_stdout(io.StringIO()):
        train_maac.main(argv, timings=stamps)
    (n0, t0), (n1, t1) = stamps[0], stamps[1]          # the first stretch warms up; the second is measured
    return dict(envs=envs, publish=publish, iteration_ms=(t1 - t0) / (n1 - n0) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 128, 256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5, help="(c): measured iterations per run (after as many warm-up ones)")
    ap.add_argument("--loop-envs", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--skip-loop", action="store_true")
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    out = dict(device=props.name, arch=getattr(props, "gcnArchName", ""), publish=[], loop=[])
    print(f"{'H':>6} {'A':>4} {'device GPU us':>14} {'device call us':>15} {'call+sync us':>13} {'host set_actor us':>18}")
    for A in (12, 48):
        for H in args.hidden:
            r = publish_costs(H, A, args.reps)
            out["publish"].append(r)
            print(f"{H:6d} {A:4d} {r['device_gpu_us']:14.1f} {r['device_call_us']:15.1f} {r['device_call_sync_us']:13.1f} "
                  f"{r['host_set_actor_us']:18.1f}", flush=True)
    if not args.skip_loop:
        print(f"\ntrain_maac, device learner, prioritised ring, 10 UAVs x 200 steps, {args.iters} iterations measured")
        for envs in args.loop_envs:
            for publish in ("host", "device"):
                r = loop_cost(envs, publish, args.iters)
                out["loop"].append(r)
                print(f"  {envs:5d} envs  --publish {publish:6s}  {r['iteration_ms']:8.2f} ms / iteration", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
