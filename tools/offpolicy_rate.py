#!/usr/bin/env python3
"""Off-policy correction, what it costs: the actor-forward kernel over the ring window of a rollout's add, the ratio
weights of a batch, and update_from with and without rho_bar.

window: DeviceActorCritic.log_probs_window over all T*B*N slots of a ring the size of one rollout, H = 128, A = 12, beside
DeviceActorCritic.values over the same rows.  Per row the kernel reads 52 bytes, writes 4 and issues 2 (13 + A) H flops
(12 fused operations of layer 1, the max, A of layer 2 per hidden unit) plus A expf and one logf; the row prints its share
of the 157 TF fp32 vector peak and of the 8 TB/s HBM rate beside the time.
ratio: uavtrack_learner_ratio_weights at n = 65 536 through an index vector into a ring of 2 M slots.
update: DeviceActorCritic.update_from at n = 65 536, H = 128 from a ring of 2 M slots, uniform and prioritised
(importance=True), with rho_bar = 1.0 against without.
The compared calls alternate; each figure is the median of 7 runs of back-to-back calls between HIP events.

    python tools/offpolicy_rate.py [--quick] [--out FILE]     # FILE: the rows as one JSON list
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402
import uavtrack  # noqa: E402
from lambda_rate import PEAK_FP32_VECTOR, PEAK_HBM, put  # noqa: E402
from nstep_rate import DEV, GAMMA, alternating  # noqa: E402

A = 12


def filled(ring, learner):
    """Random transitions in every slot, their log_mu the learner's own log-probabilities (rho = 1: nothing is refused)."""
    g = torch.Generator(device=DEV).manual_seed(0)
    slots = ring.capacity
    ring.store["states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
    ring.store["next_states"].copy_(torch.rand(slots, 12, device=DEV, generator=g) * 2 - 1)
    ring.store["actions"].copy_(torch.randint(0, A, (slots,), device=DEV, generator=g, dtype=torch.int32))
    ring.store["rewards"].copy_(torch.rand(slots, device=DEV, generator=g) * 4 - 2)
    if ring.priorities is not None:
        ring.priorities.copy_(torch.rand(slots, device=DEV, generator=g) + 0.1)
    ring.pos, ring.count = 0, slots
    if ring.log_mu is not None:
        learner.log_probs_window(ring.store["states"], ring.store["actions"], 0, slots, ring.log_mu)
    return ring


def window_row(n, H):
    learner = uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, GAMMA, DEV, max_batch=64)
    ring = filled(uavtrack.ReplayRing(n, DEV, seed=1, max_batch=64).with_behaviour(), learner)
    s, a, v = ring.store["states"], ring.store["actions"], torch.empty(n, device=DEV)
    res = alternating({"log_probs_window": lambda: learner.log_probs_window(s, a, n // 3, n, ring.log_mu),
                       "values": lambda: learner.values(s, out=v)}, reps=10)
    us = res["log_probs_window"][0]
    flops = 2 * (13 + A) * H * n
    row = {"what": "log_probs_window", "rows": n, "H": H, "A": A, "flops": flops, "bytes": 56 * n,
           "share_of_fp32_vector_peak": round(flops / (us * 1e-6) / PEAK_FP32_VECTOR, 3),
           "share_of_hbm_rate": round(56 * n / (us * 1e-6) / PEAK_HBM, 3)}
    learner.check()
    for x in (learner, ring):
        x.close()
    return put(row, res)


def update_rows(n, H, slots):
    rows = []
    for kind in ("uniform", "prioritised"):
        cls = uavtrack.ReplayRing if kind == "uniform" else uavtrack.PrioritizedReplayRing
        learners = {k: uavtrack.DeviceActorCritic(12, H, A, 1e-4, 5e-4, GAMMA, DEV, loss="per_sample", max_batch=n)
                    for k in ("plain", "rho_bar")}
        ring = filled(cls(slots, DEV, seed=1, max_batch=n).with_behaviour(), learners["rho_bar"])
        if kind == "uniform":
            idx, _ = ring._draw_batch(n)
            w = torch.empty(n, device=DEV)
            batch = learners["rho_bar"]._Batch(n, ring.store, slots, idx, log_mu=ring.log_mu)
            res = alternating({"ratio_weights": lambda: learners["rho_bar"]._ratio_weights(batch, 1.0, w, None)}, reps=50)
            rows.append(put({"what": "ratio_weights", "n": n, "H": H, "A": A, "slots": slots}, res))
        imp = kind == "prioritised"
        res = alternating({"plain": lambda: learners["plain"].update_from(ring, n, importance=imp),
                           "rho_bar": lambda: learners["rho_bar"].update_from(ring, n, importance=imp, rho_bar=1.0)},
                          reps=20)
        rows.append(put({"what": "update_from", "ring": kind, "n": n, "H": H, "A": A, "slots": slots}, res))
        # (the rho_bar learner moves away from the store's log_mu as it trains: a ratio off 1 costs the same)
        for x in list(learners.values()) + [ring]:
            x.check()
            x.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller sizes (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "offpolicy_rate.py measures on the MI355X"
    rows = []
    if args.quick:
        rows += [window_row(64 * 10 * 20, 128)] + update_rows(4096, 128, 1 << 16)
    else:
        rows += [window_row(1024 * 10 * 200, 128), window_row(4096 * 20 * 200, 128)] + update_rows(65536, 128, 1 << 21)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
