#!/usr/bin/env python3
"""Writes tests/golden/f5_actor_critic_update.npz: what the reference's own learner computes.

Imports the UNMODIFIED reference classes ActorCritic, FnnPolicyNet, FnnValueNet (src/models/actor_critic.py) and
PrioritizedReplayBuffer (src/train.py) from a checkout of the reference (argument 1, default ../reference next to
this repository), on the CPU in fp32, and records per case:
  - the seeded initial weights (w0: the eight parameter tensors flattened in torch order, actor then critic);
  - a transition store (states / actions / rewards / next_states): real transitions of tests/golden/g2_n20m10_raw.npz
    (obs[t] -> obs[t+1] with the action and reward of step t+1) plus synthetic rows within get_local_state's bounds;
  - five batches drawn from it with replacement (idx [5][n], so indices repeat), and after each ActorCritic.update:
    actor_loss, critic_loss, td_delta; after updates 1 and 5: every parameter, Adam's exp_avg / exp_avg_sq and step;
  - for case h128: one PrioritizedReplayBuffer.update_priorities(idx[0], |td_delta|) (train.py:262) on a buffer
    holding the store, and its priorities before and after (duplicate indices: the last occurrence wins).
Cases: h128 (H 128, A 12, n 257), h48 (H 48, n 257), n1 (H 128, n 1).  Generation only: nothing at test time
reads the reference.

    python tools/gen_learner_golden.py /path/to/reference
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "f5_actor_critic_update.npz")
GAMMA, ACTOR_LR, CRITIC_LR = 0.95, 1e-3, 5e-3
CAPACITY, A = 300, 12


def store_rows(rng):
    z = np.load(os.path.join(ROOT, "tests", "golden", "g2_n20m10_raw.npz"))
    obs, act, rew = z["obs"], z["actions"], z["reward"]               # [E, T, N, 12], [E, T, N], [E, T, N]
    s, a, r, s2 = obs[:, :-1].reshape(-1, 12), act[:, 1:].reshape(-1), rew[:, 1:].reshape(-1), obs[:, 1:].reshape(-1, 12)
    pick = rng.choice(len(s), CAPACITY - 40, replace=False)
    s, a, r, s2 = s[pick], a[pick], r[pick], s2[pick]
    meta = json.loads(str(z["meta"]))

    def synth(k):     # get_local_state bounds (uav.py:156-197): offsets within [-1, 1], position / dc, a / Na
        x = rng.uniform(-1, 1, size=(k, 12))
        x[:, 9] = rng.uniform(0, 5, size=k)
        x[:, 10] = rng.uniform(0, 5, size=k)
        x[:, 11] = rng.uniform(0, 1, size=k)
        return x.astype(np.float32)
    s = np.concatenate([s, synth(40)]).astype(np.float32)
    s2 = np.concatenate([s2, synth(40)]).astype(np.float32)
    a = np.concatenate([a, rng.randint(0, A, size=40)]).astype(np.int64)
    r = np.concatenate([r, rng.uniform(-2, 2, size=40)]).astype(np.float32)
    return s, a, r, s2, meta


def flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().ravel() for t in tensors]).astype(np.float32)


def adam_state(agent):
    m, v, step = [], [], []
    for opt, net in ((agent.actor_optimizer, agent.actor), (agent.critic_optimizer, agent.critic)):
        for p in net.parameters():
            st = opt.state[p]
            m.append(st["exp_avg"]); v.append(st["exp_avg_sq"]); step.append(int(float(st["step"])))
    return flat(m), flat(v), np.array(step, np.int64)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    sys.path.insert(0, os.path.join(ref, "src"))
    from models.actor_critic import ActorCritic            # noqa: E402  (the reference, unmodified)
    import importlib
    import types
    for mod in ("imageio", "tensorboardX", "torch.utils.tensorboard", "matplotlib", "matplotlib.pyplot", "tqdm"):
        try:                                               # train.py's plotting / logging imports, unused here
            importlib.import_module(mod)
        except ImportError:
            sys.modules[mod] = types.ModuleType(mod)
            sys.modules[mod].__getattr__ = lambda name: None
    from train import PrioritizedReplayBuffer              # noqa: E402

    torch.set_num_threads(1)
    rng = np.random.RandomState(5)
    s, a, r, s2, src_meta = store_rows(rng)
    out = {"store_states": s, "store_actions": a.astype(np.int32), "store_rewards": r, "store_next_states": s2}
    meta = {"gamma": GAMMA, "actor_lr": ACTOR_LR, "critic_lr": CRITIC_LR, "capacity": CAPACITY, "A": A,
            "cases": {}, "source": "reference ActorCritic.update on CPU fp32, torch " + torch.__version__}
    for case, H, n, seed in (("h128", 128, 257, 11), ("h48", 48, 257, 12), ("n1", 128, 1, 13)):
        torch.manual_seed(seed)
        agent = ActorCritic(12, H, A, ACTOR_LR, CRITIC_LR, GAMMA, "cpu")
        out[f"{case}_w0"] = flat(list(agent.actor.parameters()) + list(agent.critic.parameters()))
        idx = rng.randint(0, CAPACITY, size=(5, n)).astype(np.int64)
        out[f"{case}_idx"] = idx
        al, cl, tds = [], [], []
        for u in range(5):
            i = idx[u]
            sample = {"states": s[i], "actions": a[i], "rewards": r[i], "next_states": s2[i]}
            la, lc, td = agent.update(sample)
            assert la.dim() == 0 and lc.dim() == 0
            al.append(float(la)); cl.append(float(lc)); tds.append(td.detach().numpy().reshape(n).copy())
            if u == 0 and case == "h128":
                buf = PrioritizedReplayBuffer(CAPACITY)
                buf.add({"states": list(s), "actions": list(a), "rewards": list(r), "next_states": list(s2)})
                buf.priorities[:] = rng.uniform(0.1, 1.0, size=CAPACITY).astype(np.float32)
                out["prio_before"] = buf.priorities.copy()
                buf.update_priorities(i, td.abs().detach().cpu().numpy())
                out["prio_after"] = buf.priorities.copy()
                assert len(set(i.tolist())) < n, "the priority case needs repeated indices"
            if u in (0, 4):
                tag = u + 1
                out[f"{case}_params{tag}"] = flat(list(agent.actor.parameters()) + list(agent.critic.parameters()))
                m, v, st = adam_state(agent)
                out[f"{case}_exp_avg{tag}"], out[f"{case}_exp_avg_sq{tag}"], out[f"{case}_step{tag}"] = m, v, st
        out[f"{case}_actor_loss"] = np.array(al, np.float32)
        out[f"{case}_critic_loss"] = np.array(cl, np.float32)
        out[f"{case}_td"] = np.stack(tds).astype(np.float32)
        meta["cases"][case] = {"hidden": H, "n": n, "seed": seed}
    np.savez_compressed(OUT, meta=json.dumps(meta), **out)
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
