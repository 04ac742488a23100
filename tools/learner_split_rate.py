#!/usr/bin/env python3
"""Cost of the split learner update (grad + apply + priority write) against the closed update, H = 128, A = 12, with
tools/learner_rate.py's protocol: warm-up, HIP events around 100 back-to-back updates on resident batches, median of 5
runs.  Every call goes straight to the library on preallocated buffers, with an index vector and a priority write on
both sides.  One JSON line per measurement:

    update      uavtrack_learner_update at n = 4096 / 65536 / 262144
    split       uavtrack_learner_grad + _apply (count 1) + _write_priorities at the same n
    many8       8 rings x 8192 rows through DeviceActorCritic.update_from_many against one 65536-row update_from
    gloo2       (--gloo) two processes on this GPU, update_from(..., group=...) at 32768 rows per rank: the round trip of
                the row all-gather through the host.  gloo on a shared GPU: not a forecast for RCCL.

A/B against another build of the library: run the tool once per library, alternating, with UAVTRACK_LIB=<path>
UAVTRACK_LIB_OLDER_OK=1; a library without the split symbols prints only its `update` lines.

    python tools/learner_split_rate.py [--gloo] [--tag NAME]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd")]

import torch  # noqa: E402
import uavtrack  # noqa: E402
from uavtrack._lib import ptr  # noqa: E402

DEV = "cuda:0"
H, A = 128, 12


def timed(fn, reps, runs):
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(ts)[len(ts) // 2], [round(t, 1) for t in ts]


def store_of(n, g):
    return {"states": torch.rand(n, 12, device=DEV, generator=g) * 2 - 1,
            "actions": torch.randint(0, A, (n,), device=DEV, generator=g, dtype=torch.int32),
            "rewards": torch.rand(n, device=DEV, generator=g) * 4 - 2,
            "next_states": torch.rand(n, 12, device=DEV, generator=g) * 2 - 1}


def ring_of(n, seed, g, max_batch):
    ring = uavtrack.PrioritizedReplayRing(n, DEV, seed=seed, max_batch=max_batch)
    ring.add(store_of(n, g))
    return ring


def gloo_worker(rank, port, reps, runs, tag):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    g = torch.Generator(device=DEV); g.manual_seed(rank)
    n = 32768
    ring = ring_of(n, rank, g, n)
    L = uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, DEV, max_batch=n)
    uavtrack.broadcast_learner(L)
    for _ in range(10):
        L.update_from(ring, n, group=dist.group.WORLD)
    t_dp, r_dp = timed(lambda: L.update_from(ring, n, group=dist.group.WORLD), reps, runs)
    t_one, r_one = timed(lambda: L.update_from(ring, n), reps, runs)
    L.check()
    if rank == 0:
        print(json.dumps({"tag": tag, "what": "gloo2", "n_per_rank": n, "group_us": round(t_dp, 1), "group_runs_us": r_dp,
                          "local_update_from_us": round(t_one, 1), "local_runs_us": r_one,
                          "note": "gloo through the host, two processes on one GPU; not a forecast for RCCL"}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tag", default=os.path.basename(os.path.dirname(uavtrack._lib.LIB_PATH)))
    ap.add_argument("--gloo", action="store_true")
    ap.add_argument("--gloo-worker", nargs=2, type=int, metavar=("RANK", "PORT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gloo_worker:
        return gloo_worker(args.gloo_worker[0], args.gloo_worker[1], args.reps, args.runs, args.tag)
    lib = uavtrack._lib.load()
    have_split = hasattr(lib, "uavtrack_learner_grad")
    g = torch.Generator(device=DEV); g.manual_seed(0)
    for n in (4096, 65536, 262144):
        store = store_of(n, g)
        idx = torch.randint(0, n, (n,), device=DEV, generator=g)
        prio = torch.rand(n, device=DEV, generator=g) + 0.1
        L = uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, DEV, max_batch=n)
        losses, td, st = torch.empty(2, device=DEV), torch.empty(n, device=DEV), L._stream()
        row = torch.empty(L.row_floats, device=DEV)
        sp = [ptr(store[k]) for k in ("states", "actions", "rewards", "next_states")]

        def update():
            lib.uavtrack_learner_update(L._h, n, *sp, n, ptr(idx), ptr(losses[0:1]), ptr(losses[1:2]), ptr(td), ptr(prio), st)

        def split():
            lib.uavtrack_learner_grad(L._h, n, *sp, n, ptr(idx), ptr(td), ptr(row), st)
            lib.uavtrack_learner_apply(L._h, ptr(row), 1, ptr(losses[0:1]), ptr(losses[1:2]), st)
            lib.uavtrack_learner_write_priorities(L._h, n, ptr(idx), n, ptr(td), ptr(prio), st)
        for what, fn in (("update", update),) + ((("split", split),) if have_split else ()):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            t, runs = timed(fn, args.reps, args.runs)
            print(json.dumps({"tag": args.tag, "what": what, "n": n, "H": H, "us": round(t, 1), "runs_us": runs}), flush=True)
        L.check()
        L.close()
    if not have_split:
        return
    rings = [ring_of(8192, k, g, 8192) for k in range(8)]
    one = ring_of(65536, 9, g, 65536)
    L = uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, DEV, max_batch=65536)
    for _ in range(10):
        L.update_from_many(rings, 8192); L.update_from(one, 65536)
    torch.cuda.synchronize()
    t8, r8 = timed(lambda: L.update_from_many(rings, 8192), args.reps, args.runs)
    t1, r1 = timed(lambda: L.update_from(one, 65536), args.reps, args.runs)
    L.check()
    print(json.dumps({"tag": args.tag, "what": "many8", "update_from_many_8x8192_us": round(t8, 1), "many_runs_us": r8,
                      "update_from_65536_us": round(t1, 1), "one_runs_us": r1}), flush=True)
    if args.gloo:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        L.close()
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--gloo-worker", str(r), str(port),
                                   "--reps", str(args.reps), "--runs", str(args.runs), "--tag", args.tag]) for r in range(2)]
        codes = []
        for p in procs:
            try:
                codes.append(p.wait(timeout=300))
            except subprocess.TimeoutExpired:
                p.kill()
                codes.append(p.wait())
        if codes != [0, 0]:
            raise SystemExit(f"gloo workers exited with {codes}")


if __name__ == "__main__":
    main()
