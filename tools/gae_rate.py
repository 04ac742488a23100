#!/usr/bin/env python3
"""Fixed GAE advantages, what they cost, each against what it replaces.

add: one envs x n_uav x 200 steps rollout (done fired once, mid-rollout, with its start_obs) into a uniform ring of twice
that size: uavtrack_replay_add_rollout_gae against uavtrack_replay_add_rollout_lambda, all value arrays given, so the adds
alone are timed (the write is the same kernel; the scan stores three words per slot in place of two and loads one more).
values: the three critic passes a GAE add's critic= form runs -- over obs (T*B*N rows, what the lambda add runs too), over
obs_in (B*N rows) and over start_obs (T*B*N rows) -- each timed on its own, H = 128.
update: DeviceActorCritic.update_from at n = 65 536, H = 128, loss="per_sample", from a uniform GAE ring of 2 M slots
against a plain ring of the same contents, in three settings: raw, set_advantage("batch"), and clip_eps = 0.2 (both rings
with_behaviour, log_mu = log pi of the actor as it stands).
The compared calls alternate; each figure is the median of 7 runs of back-to-back calls between HIP events
(tools/nstep_rate.py's `alternating`).

    python tools/gae_rate.py [--quick] [--out FILE]     # FILE: the rows as one JSON list
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402
import uavtrack  # noqa: E402
from lambda_rate import LAMBDA, put, rollout  # noqa: E402
from nstep_rate import DEV, GAMMA, alternating  # noqa: E402


def add_row(B, N, T):
    obs_in, out = rollout(B, N, T)
    n = T * B * N
    rings = {"lambda": uavtrack.ReplayRing(2 * n, DEV, seed=1).with_lambda(LAMBDA, GAMMA),
             "gae": uavtrack.ReplayRing(2 * n, DEV, seed=1).with_gae(LAMBDA, GAMMA)}
    vals, v_in, v_so = torch.randn(T, B, N, device=DEV), torch.randn(B, N, device=DEV), torch.randn(T, B, N, device=DEV)
    calls = {"lambda": lambda: rings["lambda"].add_rollout(obs_in, out, values=vals),
             "gae": lambda: rings["gae"].add_rollout_gae(obs_in, out, values=vals, values_in=v_in, values_start=v_so)}
    row = put({"what": "add_rollout", "ring": "uniform", "envs": B, "n_uav": N, "steps": T, "transitions": n},
              alternating(calls, reps=10))
    for r in rings.values():
        r.close()
    return row


def values_row(B, N, T, H):
    obs_in, out = rollout(B, N, T)
    learner = uavtrack.DeviceActorCritic(12, H, 12, 1e-4, 5e-4, GAMMA, DEV, max_batch=64)
    bufs = {k: torch.empty(x.numel() // 12, device=DEV) for k, x in (("obs", out["obs"]), ("obs_in", obs_in),
                                                                     ("start_obs", out["start_obs"]))}
    src = {"obs": out["obs"], "obs_in": obs_in, "start_obs": out["start_obs"]}
    res = alternating({"values_" + k: (lambda k=k: learner.values(src[k], out=bufs[k])) for k in src}, reps=10)
    row = put({"what": "values", "envs": B, "n_uav": N, "steps": T, "H": H}, res)
    learner.check()
    learner.close()
    return row


def update_rows(n, H, slots):
    g = torch.Generator(device=DEV).manual_seed(0)
    rows = []
    for setting in ("raw", "batch", "clip0.2"):
        rings = {"plain": uavtrack.ReplayRing(slots, DEV, seed=1, max_batch=n),
                 "gae": uavtrack.ReplayRing(slots, DEV, seed=1, max_batch=n).with_gae(LAMBDA, GAMMA)}
        learners = {k: uavtrack.DeviceActorCritic(12, H, 12, 1e-4, 5e-4, GAMMA, DEV, loss="per_sample", max_batch=n)
                    for k in rings}
        for k, r in rings.items():
            r.store["states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
            r.store["next_states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
            r.store["actions"].copy_(torch.randint(0, 12, (slots,), device=DEV, generator=g, dtype=torch.int32))
            r.store["rewards"].copy_(torch.rand(slots, device=DEV, generator=g) * 4 - 2)
            r.pos, r.count = 0, slots
            if r.advantages is not None:
                r.advantages.copy_(torch.randn(slots, device=DEV, generator=g))
                r.discounts.zero_()
            if setting == "batch":
                learners[k].set_advantage("batch")
            if setting.startswith("clip"):
                r.with_behaviour()
                learners[k].log_probs_window(r.store["states"], r.store["actions"], 0, slots, r.log_mu)
        kw = {"clip_eps": 0.2} if setting.startswith("clip") else {}
        res = alternating({k: (lambda k=k: learners[k].update_from(rings[k], n, **kw)) for k in rings}, reps=50)
        rows.append(put({"what": "update_from", "setting": setting, "n": n, "H": H, "slots": slots}, res))
        for x in list(learners.values()) + list(rings.values()):
            x.check()
            x.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gae_rate.py measures on the MI355X"
    rows = []
    if args.quick:
        rows += [add_row(64, 10, 20), values_row(64, 10, 20, 128)] + update_rows(4096, 128, 1 << 16)
    else:
        for B, N in ((1024, 10), (4096, 20)):
            rows += [add_row(B, N, 200), values_row(B, N, 200, 128)]
        rows += update_rows(65536, 128, 1 << 21)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
