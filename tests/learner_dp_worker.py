"""One rank of the two-process data-parallel learner test (tests/test_hip_learner_dp.py): its own prioritised ring
filled from rank-seeded synthetic transitions, a learner that starts DIFFERENT on every rank until broadcast_learner,
then three update_from(..., group=...) with a batch size that differs between the ranks.  Writes its final blobs to
<out>/rank<r>.npz.  Also the single-process side of the same data (rank_data, ring_for), so both sides build their
inputs with the same code.

    python tests/learner_dp_worker.py <rank> <world> <port> <backend> <out dir>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H, A, LRS, GAMMA, UPDATES, BATCH = 64, 12, (1e-3, 5e-3), 0.95, 3, 4096
COUNTS = (3000, 1777)            # transitions in each rank's ring: below BATCH, so the ranks' n differ


def rank_data(rank):
    import learner_harness as lh
    return lh.batch(np.random.RandomState(500 + rank), COUNTS[rank], A)


def ring_for(rank, dev):
    import torch
    import uavtrack
    s, a, r, s2 = rank_data(rank)
    ring = uavtrack.PrioritizedReplayRing(4000, dev, seed=40 + rank, max_batch=BATCH)
    ring.add({"states": torch.from_numpy(s), "actions": torch.from_numpy(a), "rewards": torch.from_numpy(r),
              "next_states": torch.from_numpy(s2)})
    # distinct priorities, so the draw is not uniform
    ring.priorities[:COUNTS[rank]] = torch.from_numpy(
        np.random.RandomState(600 + rank).uniform(0.1, 2.0, COUNTS[rank]).astype(np.float32)).to(dev)
    return ring


def learner_for(seed, dev):
    import learner_harness as lh
    import uavtrack
    L = uavtrack.DeviceActorCritic(12, H, A, LRS[0], LRS[1], GAMMA, dev, max_batch=BATCH)
    L._set_params(lh.init_blob(H, A, seed))
    return L


def blobs(L, ring, losses, tds):
    m, v, st = L._optim_state()
    return {"params": L._get_params(), "exp_avg": m, "exp_avg_sq": v, "step": st,
            "losses": np.array([[float(a), float(c)] for a, c in losses], np.float32),
            "priorities": ring.priorities.cpu().numpy(),
            **{f"td{k}": t.cpu().numpy() for k, t in enumerate(tds)}}


def main(rank, world, port, backend, out):
    import torch
    import torch.distributed as dist
    import uavtrack
    dev = "cuda:0" if backend == "gloo" else f"cuda:{rank}"      # gloo: both ranks share the one GPU
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    ring = ring_for(rank, dev)
    L = learner_for(7 + rank, dev)                                # rank 1 starts elsewhere ...
    L._run(64, ring.store, ring.capacity, None, None)             # ... and every rank with Adam state of its own
    uavtrack.broadcast_learner(L, None, src=0)
    losses, tds = [], []
    for _ in range(UPDATES):
        al, cl, td = L.update_from(ring, BATCH, group=dist.group.WORLD)
        losses.append((al, cl)); tds.append(td)
    L.check(); ring.check()
    np.savez(os.path.join(out, f"rank{rank}.npz"), **blobs(L, ring, losses, tds))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
