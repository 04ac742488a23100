"""numpy mirror of the device learner's target critic (uavtrack_learner_set_target), restating include/uavtrack.h: the
two sync rules in float32, operation by operation, and the float64 update that bootstraps from a target, built on
tests/learner_mirror.py.  The target theta- is the critic's block of the parameter blob: 14 H + 1 words in torch order,
fc1.weight [H][12], fc1.bias [H], fc2.weight [1][H], fc2.bias [1]."""
import numpy as np

import learner_mirror as mirror


def critic_block(blob, H, A):
    """The critic's 14 H + 1 words of a parameter blob, as a copy."""
    return np.array(blob[mirror.layout(H, A)[1][4]:], copy=True)


def with_critic(blob, H, A, theta):
    """The blob with theta in the critic's place."""
    out = np.array(blob, copy=True)
    out[mirror.layout(H, A)[1][4]:] = theta
    return out


def polyak(t, w, tau):
    """t <- fl(fl(omt * t) + fl(tau32 * w)) per word, tau32 = (float)tau and omt = 1.0f - tau32: two float32 multiplies
    and one float32 add, each rounded on its own."""
    tau32 = np.float32(tau)
    omt = np.float32(np.float32(1.0) - tau32)
    t, w = np.asarray(t, np.float32), np.asarray(w, np.float32)
    a = np.multiply(omt, t, dtype=np.float32)
    b = np.multiply(tau32, w, dtype=np.float32)
    return np.add(a, b, dtype=np.float32)


def periodic(t, w, step, period):
    """t <- w when the critic's step count (already advanced by the update) is a multiple of period."""
    return np.array(w if int(step) % int(period) == 0 else t, np.float32, copy=True)


def values64(theta, H, x):
    """V(x) of the critic block theta in float64."""
    theta = np.asarray(theta, np.float64)
    w1, b1, w2, b2 = theta[:12 * H].reshape(H, 12), theta[12 * H:13 * H], theta[13 * H:14 * H], theta[14 * H]
    return np.maximum(np.asarray(x, np.float64) @ w1.T + b1, 0) @ w2 + b2


def bootstrapped(theta, H, r, s2, discount):
    """r' = r + d V_target(s') in float64: handed to learner_mirror with gamma = 0 it is the target y itself."""
    return np.asarray(r, np.float64) + np.asarray(discount, np.float64) * values64(theta, H, s2)


def losses_and_grads(blob, theta, H, A, s, a, r, s2, gamma, loss="reference"):
    """learner_mirror.losses_and_grads with y = r + gamma V_target(s')."""
    return mirror.losses_and_grads(blob, H, A, s, a, bootstrapped(theta, H, r, s2, gamma), s2, 0.0, loss)


def update(state, theta, H, A, s, a, r, s2, gamma, lrs, loss="reference"):
    """learner_mirror.update with y = r + gamma V_target(s'): (new state, actor_loss, critic_loss, td_delta).  The sync
    rule is not part of it (polyak / periodic above, on the float32 bits)."""
    return mirror.update(state, H, A, s, a, bootstrapped(theta, H, r, s2, gamma), s2, 0.0, lrs, loss)
