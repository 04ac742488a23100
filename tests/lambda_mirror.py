"""numpy mirror of the TD(lambda) targets (uavtrack_learner_values, uavtrack_replay_add_rollout_lambda), restating the
definitions of include/uavtrack.h.

Critic values.  V(x) of a row x[12]: p_j = b1c[j]; p_j = fma(W1c[j][k], x[k], p_j) for k = 0 .. 11; h_j = max(p_j, 0);
z = b2c[0]; z = fma(W2c[j], h_j, z) for j = 0 .. H - 1; V = z.  The mirror evaluates it in float64 (critic_forward, learner_mirror.values64) and
gives the magnitude bound m(x) = sum_j |W2_j| (sum_k |W1_jk| |x_k| + |b1_j|) + |b2| the fp32 chain's error scales with.

Lambda-return transitions.  T steps, agents = envs * n_uav, f = t * agents + b * n_uav + i; values[t][b][i] is meant to
hold V(obs[t][b][i]).  g = float32(gamma), l = float32(lambda), gl = g * l, c = g * (1 - l), every operation rounded to
fp32 on its own.  Per agent chain (b, i), t = T - 1 ... 0, carrying G:
    cut(t) = (t == T - 1) or (done is not None and done[t][b] != 0) or (gl == 0)
    cut:     R_t = reward[t][b][i]               d_t = g
    else:    R_t = reward[t][b][i] + gl * G      d_t = c
    G = R_t + d_t * values[t][b][i]
The stored transition is the one-step transition of uavtrack_replay_add_rollout_episodes with reward R_t and discount
d_t; slots, window, wrap and priorities as the other adds (nstep_mirror.ring_add)."""
import numpy as np

import learner_mirror as mirror
import nstep_mirror as nm

f32 = np.float32


def constants(lam, gamma):
    """(g, gl, c) in fp32."""
    g, l = f32(gamma), f32(lam)
    return g, f32(g * l), f32(g * f32(f32(1.0) - l))


def chain(r, V, done, lam, gamma):
    """(R, d) [T] float32 of one agent chain: r, V [T] float32, done [T] (its environment's flags) or None."""
    g, gl, c = constants(lam, gamma)
    r, V = np.asarray(r, f32), np.asarray(V, f32)
    T = len(r)
    R, d = np.empty(T, f32), np.empty(T, f32)
    G = f32(0.0)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            cut = t == T - 1 or (done is not None and done[t] != 0) or gl == 0
            if cut:
                R[t], d[t] = r[t], g
            else:
                R[t], d[t] = f32(r[t] + f32(gl * G)), c
            G = f32(R[t] + f32(d[t] * V[t]))
    return R, d


def segment_lengths(T, done):
    """L [T]: steps from t to the cut that ends its segment, the cut included (done: one environment's flags or None)."""
    L = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        L[t] = 1 if (t == T - 1 or (done is not None and done[t] != 0)) else L[t + 1] + 1
    return L


def transitions(obs_in, obs, actions, reward, values, lam, gamma, done=None, start_obs=None):
    """The T * agents stored transitions in f order, as nstep_mirror.transitions returns them (without the horizon)."""
    tr, _ = nm.transitions(obs_in, obs, actions, reward, 1, gamma, done, start_obs)
    T, B, N, _ = np.asarray(obs).shape
    reward = np.asarray(reward, f32).reshape(T, B, N)
    values = np.asarray(values, f32).reshape(T, B, N)
    R, d = np.empty((T, B, N), f32), np.empty((T, B, N), f32)
    for b in range(B):
        for i in range(N):
            R[:, b, i], d[:, b, i] = chain(reward[:, b, i], values[:, b, i], None if done is None else done[:, b], lam, gamma)
    tr["rewards"], tr["discounts"] = R.reshape(-1), d.reshape(-1)
    return tr


# ---- the critic in float64

def critic_of(blob, H, A):
    """(W1 [H][12], b1 [H], W2 [H], b2) of the learner's parameter blob (actor first: 13 H + A H + A floats), float32."""
    o = 13 * H + A * H + A
    blob = np.asarray(blob, f32)
    W1 = blob[o:o + 12 * H].reshape(H, 12)
    b1 = blob[o + 12 * H:o + 13 * H]
    W2 = blob[o + 13 * H:o + 14 * H]
    return W1, b1, W2, blob[o + 14 * H]


def critic_forward(blob, H, A, x):
    """V(x) [n] in float64 for rows x [n][12]."""
    return mirror.values64(mirror.critic_block(np.asarray(blob, f32), H, A), H, x)


def critic_magnitude(blob, H, A, x):
    """m(x) [n] = sum_j |W2_j| (sum_k |W1_jk| |x_k| + |b1_j|) + |b2| in float64."""
    W1, b1, W2, b2 = (np.abs(np.asarray(a, np.float64)) for a in critic_of(blob, H, A))
    return (np.abs(np.asarray(x, np.float64)) @ W1.T + b1) @ W2 + b2


# ---- the textbook lambda-return in float64

def textbook(r, V, done, lam, gamma):
    """y [T] float64: per t, with m the steps to the segment's cut, G^(n) = sum_{k<n} g^k r_{t+k} + g^n V_{t+n-1} and
    y_t = (1 - l) sum_{n=1}^{m-1} l^(n-1) G^(n) + l^(m-1) G^(m); g, l the fp32 constants read as float64.  (V_u is the
    value of the state step u ends in, so the n-step return from t bootstraps from V_{t+n-1}.)"""
    g, l = float(f32(gamma)), float(f32(lam))
    r, V = np.asarray(r, np.float64), np.asarray(V, np.float64)
    T = len(r)
    L = segment_lengths(T, done)
    y = np.empty(T, np.float64)
    for t in range(T):
        m = int(L[t])
        acc, disc, total = 0.0, 1.0, 0.0
        for n in range(1, m + 1):
            acc += disc * r[t + n - 1]
            disc *= g
            Gn = acc + disc * V[t + n - 1]
            total += ((1.0 - l) * l ** (n - 1) if n < m else l ** (m - 1)) * Gn
        y[t] = total
    return y


def fold_bound(r, V, G, L):
    """4 * 2^-24 * L * (max|r| + max|V| + max|G|): the fold's error bound over a segment of length L."""
    return 4.0 * 2.0 ** -24 * L * (np.abs(r).max() + np.abs(V).max() + np.abs(G).max())
