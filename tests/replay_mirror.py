"""fp64 numpy mirror of the prioritised replay ring (uavtrack_replay_*, uavtrack.PrioritizedReplayRing): the documented
Philox draw stream (include/uavtrack.h), inverse-CDF selection with searchsorted(side='right') as np.random.choice
(train.py:106), the importance weights (train.py:109-112) and the ring add (train.py:87-96)."""
import numpy as np

from oracle import philox4x32_10

DOMAIN = 0x52504C59          # "RPLY": Philox counter word 3 of the draw stream
TILE = 2048                  # kReplayTile (csrc/internal.h)
M32 = 0xFFFFFFFF


def u53(r0, r1):
    """53 Philox bits -> u in [0, 1 - 2^-53]: ((r0 << 21) | (r1 >> 11)) * 2^-53."""
    return float((int(r0) << 21) | (int(r1) >> 11)) * 2.0 ** -53


def uniforms(seed, call, k):
    """u of draws 0..k-1 of the call-th sample call of a ring keyed by seed."""
    key = [seed & M32, (seed >> 32) & M32]
    out = np.empty(k)
    for j in range(k):
        r = philox4x32_10([j, call & M32, (call >> 32) & M32, DOMAIN], key)
        out[j] = u53(r[0], r[1])
    return out


def weights_fp32(prio, alpha):
    """p^alpha as the reference's float32 `priorities ** alpha`."""
    p = np.asarray(prio, np.float32)
    return p.copy() if alpha == 1.0 else (p ** np.float32(alpha)).astype(np.float32)


def select(w, u):
    """searchsorted(cdf, u * total, side='right') over the fp64 running sum of w; u * total rounded up to total
    takes the last slot with w > 0."""
    cdf = np.cumsum(np.asarray(w, np.float64))
    total = cdf[-1]
    idx = np.searchsorted(cdf, u * total, side="right")
    over = idx >= len(w)
    if over.any():
        idx[over] = np.flatnonzero(np.asarray(w) > 0)[-1]
    return idx.astype(np.int64), cdf


def select_tiled(w, u, tile=TILE, lanes=64):
    """The device's structure: tile sums, their prefix, a search over the tiles, a per-lane rescan of one tile,
    and the clamps to the last slot with w > 0 where the rescan and the coarse prefix disagree."""
    w = np.asarray(w, np.float32)
    n = len(w)
    ntiles = -(-n // tile)
    wp = np.zeros(ntiles * tile, np.float32)
    wp[:n] = w
    tiles = wp.reshape(ntiles, tile).astype(np.float64)
    prefix = np.cumsum(tiles.sum(axis=1))
    total = prefix[-1]
    nz = np.flatnonzero(wp > 0)
    out = np.empty(len(u), np.int64)
    per = tile // lanes
    for j, uj in enumerate(u):
        x = uj * total
        t = int(np.searchsorted(prefix, x, side="right"))
        if t == ntiles:
            out[j] = nz[-1]
            continue
        rem = x - (prefix[t - 1] if t > 0 else 0.0)
        lane_w = tiles[t].reshape(lanes, per)
        incl = np.cumsum(lane_w.sum(axis=1))
        hit = np.flatnonzero(incl > rem)
        tile_nz = t * tile + np.flatnonzero(tiles[t] > 0)
        if len(hit) == 0:
            out[j] = tile_nz[-1]
            continue
        L = hit[0]
        want = rem - (incl[L - 1] if L > 0 else 0.0)
        c = np.cumsum(lane_w[L])
        q = np.flatnonzero(c > want)
        out[j] = t * tile + L * per + (q[0] if len(q) else np.flatnonzero(lane_w[L] > 0)[-1])
    return out


def importance(w, idx, total, count, beta):
    """(count * P(i))^-beta / max over the batch, P(i) = w_i / total, in fp64."""
    P = np.asarray(w, np.float64)[idx] / total
    return (count * P) ** -beta / (count * P.min()) ** -beta


def draw(prio, count, alpha, beta, seed, call, k):
    """(indices, weights, u, cdf) of one sample call, as the device computes them."""
    w = weights_fp32(np.asarray(prio)[:count], alpha)
    u = uniforms(seed, call, k)
    idx, cdf = select(w, u)
    return idx, importance(w, idx, cdf[-1], count, beta), u, cdf


def near_boundary(u, cdf, idx, w, rel=1e-12):
    """Draws whose u * total lies within rel * total of a CDF boundary, or within one fp32 ulp of each weight summed up
    to it (where a 1-ulp difference in the device's powf could move it)."""
    total = cdf[-1]
    x = u * total
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    hi = cdf[idx]
    tol = rel * total + 2.0 ** -23 * hi
    return (np.abs(x - lo) <= tol) | (np.abs(hi - x) <= tol)


def ring_add(store, prio, pos, count, capacity, trans):
    """PrioritizedReplayBuffer.add of n transitions (numpy, in place): only the last `capacity` survive, each at the
    maximum priority before the call (1.0 for an empty ring).  Returns (pos, count)."""
    n = len(trans["actions"])
    top = np.float32(1.0) if count == 0 else prio.max()
    skip = max(0, n - capacity)
    slots = (pos + skip + np.arange(n - skip)) % capacity
    for k in ("states", "actions", "rewards", "next_states"):
        store[k][slots] = trans[k][skip:]
    prio[slots] = top
    return (pos + n) % capacity, min(capacity, count + n)
