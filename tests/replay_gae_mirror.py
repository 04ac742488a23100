"""numpy mirror of the GAE add (uavtrack_replay_add_rollout_gae), restating the definitions of include/uavtrack.h.

T steps, agents = envs * n_uav, f = t * agents + b * n_uav + i.  values[t][b][i] = V(obs[t][b][i]), values_in[b][i] =
V(obs_in[b][i]), values_start[t][b][i] = V(start_obs[t][b][i]) (read only where done[t][b] fired).  g = float32(gamma),
l = float32(lambda), gl = g * l, c = g * (1 - l), every operation rounded to fp32 on its own.  Per agent chain (b, i),
t = T - 1 ... 0, carrying G -- the lambda add's fold (lambda_mirror.chain), operation for operation:
    cut(t) = (t == T - 1) or (done is not None and done[t][b] != 0) or (gl == 0)
    cut:     R_t = reward[t][b][i]               d_t = g
    else:    R_t = reward[t][b][i] + gl * G      d_t = c
    G = R_t + d_t * values[t][b][i]
Stored per (t, b, i): state, action, next_state and priority as the lambda add; reward = G_t; discount = +0.0;
advantage = fl(G_t - Vs_t), Vs_t = values_in at t == 0, values_start[t - 1] where done[t - 1][b] fired, values[t - 1]
otherwise.

gae64 is the independent statement: per segment, A_t = sum_k (g l)^k delta_{t+k} with
delta_u = r_u + g V(s_{u+1}) - V(s_u) in float64, V(s_{u+1}) = values[u] and V(s_u) = Vs_u as above."""
import numpy as np

import lambda_mirror as lm
import nstep_mirror as nm

f32 = np.float32


def chain(r, V, Vs, done, lam, gamma):
    """(G, adv) [T] float32 of one agent chain: r, V, Vs [T] float32 (Vs[t] the value of the state step t began in),
    done [T] (its environment's flags) or None."""
    g, gl, c = lm.constants(lam, gamma)
    r, V, Vs = np.asarray(r, f32), np.asarray(V, f32), np.asarray(Vs, f32)
    T = len(r)
    Gs, adv = np.empty(T, f32), np.empty(T, f32)
    G = f32(0.0)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            cut = t == T - 1 or (done is not None and done[t] != 0) or gl == 0
            R, d = (r[t], g) if cut else (f32(r[t] + f32(gl * G)), c)
            G = f32(R + f32(d * V[t]))
            Gs[t] = G
            adv[t] = f32(G - Vs[t])
    return Gs, adv


def state_values(values, values_in, values_start, done):
    """Vs [T][B][N] float32: the value of the state every step began in."""
    values = np.asarray(values, f32)
    T, B, N = values.shape
    Vs = np.concatenate([np.asarray(values_in, f32).reshape(1, B, N), values[:-1]], axis=0)
    if done is not None:
        vso = np.asarray(values_start, f32).reshape(T, B, N)
        for t in range(1, T):
            for b in range(B):
                if done[t - 1][b] != 0:
                    Vs[t, b] = vso[t - 1, b]
    return Vs


def transitions(obs_in, obs, actions, reward, values, values_in, values_start, lam, gamma, done=None, start_obs=None):
    """The T * agents stored transitions in f order: nstep_mirror.transitions' five stores and "advantages"."""
    assert (done is None) == (values_start is None)
    tr, _ = nm.transitions(obs_in, obs, actions, reward, 1, gamma, done, start_obs)
    T, B, N, _ = np.asarray(obs).shape
    reward = np.asarray(reward, f32).reshape(T, B, N)
    values = np.asarray(values, f32).reshape(T, B, N)
    Vs = state_values(values, values_in, values_start, done)
    G, adv = np.empty((T, B, N), f32), np.empty((T, B, N), f32)
    for b in range(B):
        for i in range(N):
            G[:, b, i], adv[:, b, i] = chain(reward[:, b, i], values[:, b, i], Vs[:, b, i],
                                             None if done is None else done[:, b], lam, gamma)
    tr["rewards"], tr["advantages"] = G.reshape(-1), adv.reshape(-1)
    tr["discounts"] = np.zeros(T * B * N, f32)                         # +0.0: "do not bootstrap"
    return tr


def ring_add(image, pos, count, trans):
    """nstep_mirror.ring_add with the seventh store: image["advantages"] is changed in place like the others."""
    cap = len(image["actions"])
    n = len(trans["actions"])
    skip = max(0, n - cap)
    slots = (pos + skip + np.arange(n - skip)) % cap
    image["advantages"][slots] = trans["advantages"][skip:]
    return nm.ring_add(image, pos, count, trans)


# ---- the independent float64 statement

def gae64(r, V, Vs, done, lam, gamma):
    """(A, mag) [T] float64 of one chain.  A_t = sum_{k < L_t} (g l)^k delta_{t+k} over the L_t steps to the segment's
    cut, delta_u = r_u + g V_u - Vs_u, every term formed on its own from the inputs (no recursion); g, l the fp32
    constants read as float64.  mag_t = sum_k (g l)^k (|r| + g |V| + |Vs|)_{t+k}: what the fp32 fold's error scales with."""
    g, l = float(f32(gamma)), float(f32(lam))
    r, V, Vs = (np.asarray(a, np.float64) for a in (r, V, Vs))
    T = len(r)
    L = lm.segment_lengths(T, done)
    A, mag = np.zeros(T), np.zeros(T)
    for t in range(T):
        w = 1.0
        for k in range(int(L[t])):
            u = t + k
            A[t] += w * (r[u] + g * V[u] - Vs[u])
            mag[t] += w * (abs(r[u]) + g * abs(V[u]) + abs(Vs[u]))
            w *= g * l
    return A, mag
