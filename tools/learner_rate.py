#!/usr/bin/env python3
"""Learner rate: examples/train_maac.py's PyTorch `update` against DeviceActorCritic.update (one library call) at
n in {4096, 65536, 262144} x H in {64, 128, 256}, A = 12.  Per configuration: warm-up, then HIP events around 100
back-to-back updates on resident batches, median of 5 runs; prints us per update, the speed-up and the fraction of
the 157 TF fp32 peak for the exact FLOP count below.

FLOPs of one update (multiply-add = 2): forwards 2n(12H) x 3 (actor, critic on s and s') + 2n(H A) + 2n(H) x 2;
backwards: actor fc2 weight + input gradients 2 x 2n(H A), fc1 weight gradient 2n(12H); critic fc2 2n H, fc1 2n(12H);
softmax, losses and Adam are not counted.

    python tools/learner_rate.py [--quick]
    python tools/learner_rate.py --regularised [--quick]
    python tools/learner_rate.py --target [--quick]
    python tools/learner_rate.py --clipped
    python tools/learner_rate.py --normalised
    python tools/learner_rate.py --kl

--regularised times the device update alone (loss="per_sample") under four settings of
DeviceActorCritic.set_regularisation: everything off, the entropy bonus on, clipping on, both.  "off" enqueues the
launches of the plain update; the clip adds two small launches and one more pass over P floats.

--target times the device update alone (loss="per_sample") under three settings of DeviceActorCritic.set_target: no
target, Polyak (tau = 0.005) and periodic (period = 100).  "off" enqueues the launches of the plain update; a target
swaps the gradient kernel for the instantiation that forms V(s') over the second critic block and adds one small
launch over 14 H + 1 words behind the Adam kernel.

--clipped times DeviceActorCritic.update_from (loss="per_sample") at n = 65 536, H = 128, A = 12 from a uniform
behaviour ring of 2 M slots, without and with clip_eps = 0.2 (the clipped surrogate: the gradient kernel's
instantiation that gathers log_mu and gates each row; no further launch), the two alternating, medians of 7 runs of 20
back-to-back calls.  A/B against another build of the library: run the tool once per library, alternating, three
processes each, with UAVTRACK_LIB=<path> UAVTRACK_LIB_OLDER_OK=1; a library without the clipped symbols prints only its
"plain" figure.  The plain figure of this build may not lie above the slowest of the other build's three (DESIGN.md
section 4.11's rule); the clipped figure is reported, not a pass mark.

--normalised times the same update_from under the three modes of DeviceActorCritic.set_advantage -- "raw", a given
(mean, inv_std) pair (the gradient kernel's normalising instantiation alone) and "batch" (the TD pass, the statistics and
one sealing launch on top) --, each without and with clip_eps = 0.2, the six alternating.  A/B against another build as
for --clipped; a library without the advantage symbols prints only its "raw" figures, and "raw" is the figure the rule
above holds to.

--kl times the same clipped update_from (clip_eps = 0.2) in three states of DeviceActorCritic.set_kl_stop -- off; on with
limit = inf, which adds the KL pass (two small launches) and never trips; on and latched (the latch written by hand), where
the gradient kernel returns before its first tile and everything behind it is gated off -- each as eager calls and as
replays of a graph that holds the one update_from (draw and update), the six alternating.  A/B against another build as
for --clipped; a library without the KL symbols prints only its "off" figures, and the eager "off" is the figure the rule
above holds to.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd"), os.path.join(ROOT, "examples")]

import torch  # noqa: E402
import uavtrack  # noqa: E402
from train_maac import ValueNet, update as torch_update  # noqa: E402

PEAK_TF = 157.3


def flops(n, H, A=12):
    fwd = 3 * 2 * n * 12 * H + 2 * n * H * A + 2 * 2 * n * H
    bwd = 2 * 2 * n * H * A + 2 * n * 12 * H + 2 * n * H + 2 * n * 12 * H
    return fwd + bwd


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


def make_batch(n, A, dev):
    g = torch.Generator(device=dev); g.manual_seed(0)
    return {"states": torch.rand(n, 12, device=dev, generator=g) * 2 - 1,
            "actions": torch.randint(0, A, (n,), device=dev, generator=g, dtype=torch.int32),
            "rewards": torch.rand(n, device=dev, generator=g) * 4 - 2,
            "next_states": torch.rand(n, 12, device=dev, generator=g) * 2 - 1}


# The settings sweeps: name -> what it does to a fresh learner (None: nothing, so that "off" makes no call an older build of
# the library lacks).  --regularised: 1e-3 is far below the gradient norms of this batch, so both networks are clipped (the
# clip chain costs the same whether it clips or not).
SWEEPS = {
    "regularised": (("off", None), ("entropy", lambda L: L.set_regularisation(0.01, None)),
                    ("clip", lambda L: L.set_regularisation(0.0, 1e-3)), ("both", lambda L: L.set_regularisation(0.01, 1e-3))),
    "target": (("off", None), ("polyak", lambda L: L.set_target(tau=0.005)), ("periodic", lambda L: L.set_target(period=100))),
}


def sweep(args, grid, dev, A, settings):
    """The device update alone (loss="per_sample") under each setting: one JSON line per configuration."""
    for n, H in grid:
        store = {k: v.contiguous() for k, v in make_batch(n, A, dev).items()}
        out = {"n": n, "H": H, "A": A, "loss": "per_sample"}
        for name, apply in settings:
            L = uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, dev, loss="per_sample", max_batch=n)
            if apply is not None:
                apply(L)

            def dstep():
                L._run(n, store, n, None, None)
            for _ in range(10):
                dstep()
            torch.cuda.synchronize()
            t, runs = timed(dstep, args.reps, args.runs)
            L.check()
            out[name + "_us"] = round(t, 1)
            out[name + "_runs_us"] = [round(x, 1) for x in runs]
            L.close()
        print(json.dumps(out), flush=True)


def clipped(n=65536, H=128, A=12, slots=1 << 21):
    """update_from without and with clip_eps from one uniform behaviour ring: one JSON line."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from nstep_rate import alternating
    from offpolicy_rate import filled
    names = ["plain"] + (["clipped"] if hasattr(uavtrack._lib.load(), "uavtrack_learner_update_clipped") else [])
    learners = {k: uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, "cuda:0", loss="per_sample", max_batch=n)
                for k in names}
    ring = filled(uavtrack.ReplayRing(slots, "cuda:0", seed=1, max_batch=n).with_behaviour(), learners["plain"])
    ratio = torch.empty(n, device="cuda:0")
    calls = {"plain": lambda: learners["plain"].update_from(ring, n)}
    if "clipped" in names:
        calls["clipped"] = lambda: learners["clipped"].update_from(ring, n, clip_eps=0.2, ratio_out=ratio)
    res = alternating(calls, reps=20)
    out = {"what": "update_from", "ring": "uniform", "n": n, "H": H, "A": A, "slots": slots,
           "lib": os.environ.get("UAVTRACK_LIB", "this build")}
    for name, (med, runs) in res.items():
        out[name + "_us"] = round(med, 1)
        out[name + "_runs_us"] = [round(x, 1) for x in runs]
    if "clipped" in names:
        out["clipped_share"] = round(float(((ratio - 1).abs() > 0.2).float().mean()), 4)
    for x in list(learners.values()) + [ring]:
        x.check()
        x.close()
    print(json.dumps(out), flush=True)


def normalised(n=65536, H=128, A=12, slots=1 << 21):
    """update_from under set_advantage "raw", a given pair and "batch", without and with clip_eps: one JSON line."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from nstep_rate import alternating
    from offpolicy_rate import filled
    modes = ["raw"] + (["given", "batch"] if hasattr(uavtrack._lib.load(), "uavtrack_learner_set_advantage") else [])
    pair = torch.tensor([3.0, 0.8], device="cuda:0")
    learners, calls = {}, {}
    for mode in modes:
        for clip in (None, 0.2):
            L = uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, "cuda:0", loss="per_sample", max_batch=n)
            if mode != "raw":
                L.set_advantage(pair if mode == "given" else "batch")
            learners[mode + ("_clip" if clip else "")] = (L, clip)
    ring = filled(uavtrack.ReplayRing(slots, "cuda:0", seed=1, max_batch=n).with_behaviour(), learners["raw"][0])
    for name, (L, clip) in learners.items():
        calls[name] = (lambda L=L: L.update_from(ring, n)) if clip is None else (lambda L=L, c=clip: L.update_from(ring, n, clip_eps=c))
    res = alternating(calls, reps=20)
    out = {"what": "update_from", "ring": "uniform", "n": n, "H": H, "A": A, "slots": slots,
           "lib": os.environ.get("UAVTRACK_LIB", "this build")}
    for name, (med, runs) in res.items():
        out[name + "_us"] = round(med, 1)
        out[name + "_runs_us"] = [round(x, 1) for x in runs]
    if "batch" in modes:
        out["batch_stats"] = [round(float(x), 4) for x in learners["batch"][0].advantage_stats]
    for x in [L for L, _ in learners.values()] + [ring]:
        x.check()
        x.close()
    print(json.dumps(out), flush=True)


def kl(n=65536, H=128, A=12, slots=1 << 21):
    """The clipped update_from with the KL stop off, on and latched, eager and as a one-call graph replay: one JSON line."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from nstep_rate import alternating
    from offpolicy_rate import filled
    names = ["off"] + (["on", "latched"] if hasattr(uavtrack._lib.load(), "uavtrack_learner_set_kl_stop") else [])
    learners = {k: uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, "cuda:0", loss="per_sample", max_batch=n)
                for k in names}
    ring = filled(uavtrack.ReplayRing(slots, "cuda:0", seed=1, max_batch=n).with_behaviour(), learners["off"])
    for name in names[1:]:
        learners[name].set_kl_stop(float("inf") if name == "on" else 0.0)
    calls, graphs, held = {}, {}, []
    for name, L in learners.items():
        calls[name] = lambda L=L: L.update_from(ring, n, clip_eps=0.2)
        for _ in range(3):
            calls[name]()
        if name == "latched":
            L.kl_state[:1].fill_(1)                                 # (an on-policy ring never trips it on its own)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            held.append(calls[name]())
        calls[name + "_graph"] = graphs[name].replay
    res = alternating(calls, reps=20)
    out = {"what": "update_from", "ring": "uniform", "n": n, "H": H, "A": A, "slots": slots, "clip_eps": 0.2,
           "lib": os.environ.get("UAVTRACK_LIB", "this build")}
    for name, (med, runs) in res.items():
        out[name + "_us"] = round(med, 1)
        out[name + "_runs_us"] = [round(x, 1) for x in runs]
    if "on" in names:
        out["on_kl"] = float(learners["on"].kl)
        out["on_state"], out["latched_state"] = learners["on"].kl_state.tolist(), learners["latched"].kl_state.tolist()
    for x in list(learners.values()) + [ring]:
        x.check()
        x.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="n 65536, H 128 only")
    ap.add_argument("--regularised", action="store_true",
                    help="time the device update with the entropy bonus and the gradient-norm clip off / on")
    ap.add_argument("--target", action="store_true",
                    help="time the device update without a target critic, with Polyak averaging and with a periodic copy")
    ap.add_argument("--clipped", action="store_true",
                    help="time update_from at n 65536, H 128 from a uniform behaviour ring without and with clip_eps = 0.2")
    ap.add_argument("--normalised", action="store_true",
                    help="time update_from at n 65536, H 128 under set_advantage raw / given / batch, without and with clip_eps")
    ap.add_argument("--kl", action="store_true",
                    help="time the clipped update_from at n 65536, H 128 with the KL stop off, on and latched, eager and replayed")
    ap.add_argument("--settings", default=None, help="--regularised: a comma-separated subset of off,entropy,clip,both; "
                                                     "--target: of off,polyak,periodic")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    if args.clipped:
        return clipped()
    if args.normalised:
        return normalised()
    if args.kl:
        return kl()
    dev = "cuda:0"
    A = 12
    grid = [(65536, 128)] if args.quick else [(n, H) for H in (64, 128, 256) for n in (4096, 65536, 262144)]
    for which in ("regularised", "target"):
        if getattr(args, which):
            names = args.settings.split(",") if args.settings else [name for name, _ in SWEEPS[which]]
            return sweep(args, grid, dev, A, [x for x in SWEEPS[which] if x[0] in names])
    for n, H in grid:
        batch = make_batch(n, A, dev)
        actor, critic = uavtrack.ActorMLP(12, H, A).to(dev), ValueNet(12, H).to(dev)
        oa, oc = torch.optim.Adam(actor.parameters(), lr=1e-4), torch.optim.Adam(critic.parameters(), lr=5e-4)

        def tstep():   # the example's update without its two host reads of the losses
            s, a, r, s2 = batch["states"], batch["actions"].long().unsqueeze(1), batch["rewards"], batch["next_states"]
            td_target = r + 0.95 * critic(s2)
            td_delta = td_target - critic(s)
            lp = torch.log(actor(s).gather(1, a).squeeze(1).clamp_min(1e-12))
            al = torch.mean(-lp * td_delta.detach())
            cl = torch.nn.functional.mse_loss(critic(s), td_target.detach())
            oa.zero_grad(); oc.zero_grad(); al.backward(); cl.backward(); oa.step(); oc.step()
        L = uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, 0.95, dev, max_batch=n)
        store = {k: v.contiguous() for k, v in batch.items()}

        def dstep():
            L._run(n, store, n, None, None)
        for f in (tstep, dstep):
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        t_torch, _ = timed(tstep, args.reps, args.runs)
        t_dev, runs = timed(dstep, args.reps, args.runs)
        L.check()
        fl = flops(n, H, A)
        print(json.dumps({"n": n, "H": H, "A": A, "torch_us": round(t_torch, 1), "device_us": round(t_dev, 1),
                          "speedup": round(t_torch / t_dev, 2), "gflop": round(fl / 1e9, 3),
                          "device_tflops": round(fl / t_dev / 1e6, 2),
                          "frac_of_157TF": round(fl / t_dev / 1e6 / PEAK_TF, 4),
                          "device_runs_us": [round(x, 1) for x in runs]}), flush=True)
        L.close()


if __name__ == "__main__":
    main()
