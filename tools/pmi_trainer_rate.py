#!/usr/bin/env python3
"""PMI trainer rate: one PMINetwork.train_pmi call on the PyTorch path (uavtrack.train_pmi_epoch: make_pmi_net +
torch.optim.Adam on the device, one loss.item() per mini-batch as in the reference) against DevicePMINetwork.train_pmi
(one library call), eager and replayed from a captured graph, at (b2, batch_size, H) in
{(3000, 128, 128) configs/MAAC-R.yaml, (3000, 500, 128) examples/train_maac.py's default, (3000, 128, 64),
(3000, 128, 256)}.  The history is 200 steps x 20 UAVs of random observations on the device.

Per configuration and path: warm-up, then HIP events around `reps` back-to-back calls ending in a synchronise, median
of `runs` runs, in us per call.  Eager device calls include the index draw on a device generator; the graph replays the
library call on fixed indices.  FLOPs of one mini-batch step (multiply-add = 2), both forwards and the backward:
2 x [2 bs (12 H) + 2 bs (3H H) + 2 bs H] forward, 2 x [2 bs (12 H) + 2 x 2 bs (3H H) + 2 bs H] backward.

    python tools/pmi_trainer_rate.py [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd")]

import torch  # noqa: E402
import uavtrack  # noqa: E402

PEAK_TF = 157.3
CONFIGS = ((3000, 128, 128), (3000, 500, 128), (3000, 128, 64), (3000, 128, 256))


def flops(b2, bs, H):
    fwd = 2 * (2 * bs * 12 * H + 2 * bs * 3 * H * H + 2 * bs * H)
    bwd = 2 * (2 * bs * 12 * H + 2 * 2 * bs * 3 * H * H + 2 * bs * H)
    return (b2 // bs) * (fwd + bwd)


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
    ts.sort()
    return ts[len(ts) // 2], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the MAAC-R.yaml point only")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    n_uav, T = 20, 200
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    hist = torch.rand(T * n_uav, 12, device=dev, generator=g) * 2 - 1
    for b2, bs, H in (CONFIGS[:1] if args.quick else CONFIGS):
        cfg = {"pmi": {"batch_size": bs}}
        net = uavtrack.make_pmi_net(H).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        tr = uavtrack.DevicePMINetwork(H, b2, dev)

        def torch_call():
            uavtrack.train_pmi_epoch(net, opt, hist, n_uav, b2, bs, generator=g)

        def dev_call():
            tr.train_pmi(cfg, hist, n_uav, generator=g, sync=False)
        t_idx = torch.randint(0, T, (b2,), device=dev, generator=g)
        u_idx = torch.randint(0, n_uav, (b2, 2), device=dev, generator=g)
        avg = torch.empty((), device=dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                tr.train_indices(hist, n_uav, t_idx, u_idx, bs, avg_loss=avg)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tr.train_indices(hist, n_uav, t_idx, u_idx, bs, avg_loss=avg)
        for f in (torch_call, dev_call, graph.replay):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        t_torch, torch_runs = timed(torch_call, max(3, args.reps // 4), args.runs)
        t_dev, dev_runs = timed(dev_call, args.reps, args.runs)
        t_graph, graph_runs = timed(graph.replay, args.reps, args.runs)
        tr.check()
        fl = flops(b2, bs, H)
        print(json.dumps({"b2": b2, "batch_size": bs, "H": H, "steps": b2 // bs, "torch_us": round(t_torch, 1),
                          "device_us": round(t_dev, 1), "graph_us": round(t_graph, 1),
                          "speedup_eager": round(t_torch / t_dev, 2), "speedup_graph": round(t_torch / t_graph, 2),
                          "gflop": round(fl / 1e9, 3), "graph_tflops": round(fl / t_graph / 1e6, 3),
                          "frac_of_157TF": round(fl / t_graph / 1e6 / PEAK_TF, 5),
                          "torch_runs_us": [round(x, 1) for x in torch_runs],
                          "device_runs_us": [round(x, 1) for x in dev_runs],
                          "graph_runs_us": [round(x, 1) for x in graph_runs]}), flush=True)
        del graph
        tr.close()


if __name__ == "__main__":
    main()
