"""The rollout, the done patterns and the ring cases that the n-step and the TD(lambda) ring-add tests share
(tests/test_hip_nstep.py, tests/test_hip_lambda.py), and a ring's image: all five stores and the priorities, compared
byte for byte."""
import numpy as np

import learner_harness as lh

STORES = lh.STORES
T, B, N = 7, 3, 2
NTR = T * B * N                                                        # 42 transitions


def done(kind):
    d = np.zeros((T, B), np.uint8)
    if kind == "mid":
        d[3, 1] = 1
    elif kind == "consecutive":
        d[2, 0] = d[3, 0] = 1
    elif kind == "first":
        d[0, 2] = 1
    elif kind == "last":
        d[T - 1, 1] = 1
    elif kind == "every":
        d[:, 1] = 1
    return None if kind == "null" else d


DONES = ("zeros", "null", "mid", "consecutive", "first", "last", "every")
# (capacity, pos, count): roomy; pos three slots before the end; a ring smaller than the rollout
RINGS = {"roomy": (100, 10, 10), "wrap": (100, 97, 100), "small": (17, 5, 17)}
_roll = {}


def rollout():
    if not _roll:
        rng = np.random.default_rng(5)
        _roll.update(obs_in=rng.standard_normal((B, N, 12)).astype(np.float32),
                     obs=rng.standard_normal((T, B, N, 12)).astype(np.float32),
                     actions=rng.integers(0, 12, (T, B, N)).astype(np.int32),
                     reward=(rng.standard_normal((T, B, N)) * 3).astype(np.float32),
                     start_obs=rng.standard_normal((T, B, N, 12)).astype(np.float32))
        _roll["dev"] = {k: lh.dev(v) for k, v in _roll.items()}
    return _roll


def out(done):
    """The result dict add_rollout takes; done None: no done / start_obs at all."""
    d = rollout()["dev"]
    res = {k: d[k] for k in ("obs", "actions", "reward")}
    if done is not None:
        res.update(done=lh.dev(done), start_obs=d["start_obs"])
    return res


def prefill(ring, pos, count, seed=9):
    """Sentinel stores, the ring's host state, and (prioritised) priorities whose maximum over the whole array is 2.5."""
    rng = np.random.default_rng(seed)
    cap = ring.capacity
    ring.store["states"].copy_(lh.dev(rng.standard_normal((cap, 12)).astype(np.float32)))
    ring.store["next_states"].copy_(lh.dev(rng.standard_normal((cap, 12)).astype(np.float32)))
    ring.store["actions"].fill_(-3)
    ring.store["rewards"].fill_(-777.25)
    if ring.discounts is not None:
        ring.discounts.fill_(7.0)
    if ring.priorities is not None:
        p = rng.uniform(0.1, 2.0, cap).astype(np.float32)
        p[count:] = 0.0
        p[count // 2] = 2.5
        ring.priorities.copy_(lh.dev(p))
    ring.pos, ring.count = pos, count


def image(ring):
    img = {k: ring.store[k].cpu().numpy().copy() for k in STORES}
    img["discounts"] = None if ring.discounts is None else ring.discounts.cpu().numpy().copy()
    img["priorities"] = None if ring.priorities is None else ring.priorities.cpu().numpy().copy()
    return img


def same_image(a, b, keys=STORES + ("discounts", "priorities")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].tobytes() == b[k].tobytes(), k
