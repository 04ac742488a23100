"""numpy mirror of the multi-step targets (uavtrack_replay_add_rollout_nstep, uavtrack_learner_update_discounted /
_grad_discounted), restating the definitions of include/uavtrack.h.

A rollout has steps = T and envs * n_uav agents per step; transition (t, b, i) is flattened as
f = t * agents + b * n_uav + i.  n = n_step in [1, 64]; g = float32(gamma), gamma in [0, 1].
  Horizon   m(t, b): the smallest m >= 1 with m == n, t + m == T or done[t + m - 1][b] != 0 (without done: the first two).
  Return    R = reward[t + m - 1]; for k = m - 2 ... 0: R = reward[t + k] + g * R, every operation rounded to fp32.
  Discount  d = g; then d = d * g exactly m - 1 times, in fp32.
  Stored    state as uavtrack_replay_add_rollout_episodes stores it (obs_in at t == 0, start_obs[t - 1] behind a fired
            done, obs[t - 1] otherwise), actions[t], R, next_state = obs[t + m - 1], discount d; the slot, the window
            for T * agents > capacity, the wrap and the priorities as the other adds.
  Target    y_i = r_i + d_i V(s'_i), d_i = discounts[slot of row i]; everything behind it as before (tests/learner_mirror.py
            takes the gathered per-row array as its discount)."""
import numpy as np

MAX_NSTEP = 64
f32 = np.float32


def horizon(steps, envs, n_step, done=None):
    """m [steps][envs] (int64)."""
    m = np.empty((steps, envs), np.int64)
    for t in range(steps):
        for b in range(envs):
            k = 1
            while not (k == n_step or t + k == steps or (done is not None and done[t + k - 1][b] != 0)):
                k += 1
            m[t, b] = k
    return m


def stop_reasons(steps, envs, n_step, done=None):
    """Per (t, b): the set of the three conditions that hold at m(t, b)."""
    m = horizon(steps, envs, n_step, done)
    out = {}
    for t in range(steps):
        for b in range(envs):
            k = int(m[t, b])
            why = set()
            if k == n_step:
                why.add("n")
            if t + k == steps:
                why.add("tail")
            if done is not None and done[t + k - 1][b] != 0:
                why.add("done")
            out[t, b] = why
    return m, out


def fold(rewards, gamma):
    """(R, d) of one window's rewards [m] in fp32: Horner from the far end, the discount by m - 1 products."""
    g = f32(gamma)
    r = np.asarray(rewards, f32)
    R = f32(r[-1])
    d = g
    for k in range(len(r) - 2, -1, -1):
        R = f32(r[k] + f32(g * R))
        d = f32(d * g)
    return R, d


def transitions(obs_in, obs, actions, reward, n_step, gamma, done=None, start_obs=None):
    """The T * agents stored transitions in f order: states [n][12], actions [n], rewards [n], next_states [n][12],
    discounts [n], and the horizon [T][B]."""
    obs = np.asarray(obs, f32)
    T, B, N, D = obs.shape
    reward = np.asarray(reward, f32).reshape(T, B, N)
    assert (done is None) == (start_obs is None)
    m = horizon(T, B, n_step, done)
    states = np.concatenate([np.asarray(obs_in, f32).reshape(1, B, N, D), obs[:-1]], axis=0)
    if done is not None:
        so = np.asarray(start_obs, f32).reshape(T, B, N, D)
        for t in range(1, T):
            for b in range(B):
                if done[t - 1][b] != 0:
                    states[t, b] = so[t - 1, b]
    R = np.empty((T, B, N), f32)
    d = np.empty((T, B, N), f32)
    nxt = np.empty((T, B, N, D), f32)
    for t in range(T):
        for b in range(B):
            k = int(m[t, b])
            nxt[t, b] = obs[t + k - 1, b]
            for i in range(N):
                R[t, b, i], d[t, b, i] = fold(reward[t:t + k, b, i], gamma)
    return {"states": states.reshape(-1, D), "actions": np.asarray(actions, np.int32).reshape(-1),
            "rewards": R.reshape(-1), "next_states": nxt.reshape(-1, D), "discounts": d.reshape(-1)}, m


def nan_max(p):
    """torch.max over the priorities: a NaN wins."""
    return f32(np.nan) if np.isnan(p).any() else p.max()


def ring_add(image, pos, count, trans):
    """The ring image {states, actions, rewards, next_states, discounts, priorities or None} (arrays of `capacity` slots,
    changed in place) after adding trans: only the last min(n, capacity) land, from (pos + max(0, n - capacity)) %
    capacity on, wrapping, at the maximum of the priorities as they stood (1.0 for an empty ring).  Returns (pos, count)."""
    cap = len(image["actions"])
    n = len(trans["actions"])
    skip = max(0, n - cap)
    slots = (pos + skip + np.arange(n - skip)) % cap
    prio = image.get("priorities")
    top = None if prio is None else (f32(1.0) if count == 0 else nan_max(prio))
    for k in ("states", "actions", "rewards", "next_states", "discounts"):
        image[k][slots] = trans[k][skip:]
    if prio is not None:
        prio[slots] = top
    return (pos + n) % cap, min(cap, count + n)

