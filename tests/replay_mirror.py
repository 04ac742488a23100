"""fp64 numpy mirror of the prioritised replay ring (uavtrack_replay_*, uavtrack.PrioritizedReplayRing): the documented
Philox draw stream (include/uavtrack.h), inverse-CDF selection with searchsorted(side='right') as np.random.choice
(train.py:106), the importance weights (train.py:109-112) and the ring add (train.py:87-96); and draw_device, the
sample kernels' fp64 arithmetic reproduced operation for operation, with gap_ring, which builds priorities on which a
chosen draw falls into a rounding gap."""
import numpy as np

from oracle import philox4x32_10

DOMAIN = 0x52504C59          # "RPLY": Philox counter word 3 of the draw stream
TILE = 2048                  # kReplayTile (csrc/replay.h)
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


def near_boundary(u, cdf, idx, w, rel=1e-12, ulp_slots=None):
    """Draws whose u * total lies within rel * total of a CDF boundary, or within one fp32 ulp of each weight summed up
    to it (where a 1-ulp difference in the device's powf could move it).  ulp_slots: cover a net 1-ulp difference in
    that many slots (of the largest weight) instead of in every slot, where the full sum would cover the whole ring."""
    total = cdf[-1]
    x = u * total
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    hi = cdf[idx]
    drift = hi if ulp_slots is None else np.minimum(hi, ulp_slots * np.max(w))
    tol = rel * total + 2.0 ** -23 * drift
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


# ---- the device's arithmetic, operation for operation (csrc/replay_kernel.hip) ------------------------------------
# Every fp64 sum below is associated as the kernels associate it; np.sum (pairwise) is used nowhere.  Serial sums are
# written as explicit loops over the summands or np.add.accumulate.

SW = 256                     # threads of the tile kernel
PER_THREAD = TILE // SW      # slots summed serially per thread of the tile kernel
LANES = 64
PER_LANE = TILE // LANES     # slots per lane of the draw kernel's rescan
SCAN_W = 1024                # threads of the scan kernel

# the branch a draw takes (draw_device's `branch`)
HIT = 0              # the first slot of lane L whose running sum exceeds rem - excl
LANE_FALLBACK = 1    # lane L holds w > 0 but rem - excl rounded past its own sum: its last slot with w > 0
TILE_FALLBACK = 2    # no lane's scan exceeds rem, tile t holds w > 0: its last slot with w > 0
LANE_GAP = 3         # lane L holds no w > 0 (its scan rounded above its predecessor's): the last slot with w > 0 before it
TILE_GAP = 4         # tile t holds no w > 0 (its prefix rounded above its predecessor's): the last slot with w > 0 before it
OVER = 5             # x >= total: the last slot with w > 0 of the ring (unreachable, see draw_device)

_PM = (0xD2511F53, 0xCD9E8D57)
_PW = (0x9E3779B9, 0xBB67AE85)


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/philox.h) over numpy arrays of counters: (r0, r1, r2, r3) as uint64 arrays < 2^32."""
    c = [np.asarray(v, np.uint64) & np.uint64(M32) for v in (c0, c1, c2, c3)]
    c = [np.broadcast_to(v, np.broadcast(*c).shape).copy() for v in c]
    k0, k1 = int(k0) & M32, int(k1) & M32
    for _ in range(10):
        p0 = np.uint64(_PM[0]) * c[0]
        p1 = np.uint64(_PM[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(M32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(M32)]
        k0, k1 = (k0 + _PW[0]) & M32, (k1 + _PW[1]) & M32
    return c


def uniforms_np(seed, call, k):
    """uniforms(seed, call, k), vectorised: the u of draws 0..k-1."""
    r = philox_np(np.arange(k, dtype=np.uint64), call & M32, (call >> 32) & M32, DOMAIN, seed & M32, (seed >> 32) & M32)
    bits = (r[0] << np.uint64(21)) | (r[1] >> np.uint64(11))
    return bits.astype(np.float64) * 2.0 ** -53


def _serial(cols):
    """((c0 + c1) + c2) + ... over the last axis, from 0.0 (0.0 + c0 is exact for c0 >= 0)."""
    s = cols[..., 0].copy()
    for q in range(1, cols.shape[-1]):
        s += cols[..., q]
    return s


def _hillis_steele(v):
    """wave_inclusive_scan over the last axis (64 lanes): for o = 1, 2, .. 32, lane l >= o adds lane l - o."""
    v = v.copy()
    o = 1
    while o < v.shape[-1]:
        t = v[..., :-o].copy()
        v[..., o:] += t
        o <<= 1
    return v


def padded(w, count):
    """w[:count] as fp64, zero-padded to whole tiles: what the tile kernel reads (slots >= count weigh 0)."""
    out = np.zeros(-(-count // TILE) * TILE)
    out[:count] = np.asarray(w[:count], np.float32)
    return out


def tile_sums(wp):
    """replay_tile_kernel over a zero-padded fp64 weight array of ntiles * TILE slots: (sum [ntiles], last [ntiles]),
    last = the tile's last slot with w > 0, -1 if none."""
    nt = len(wp) // TILE
    s = _serial(wp.reshape(nt, SW, PER_THREAD)).reshape(nt, SW // 64, 64)
    o = 32
    while o:                                   # wave_sum: lane 0's shfl_down tree
        s = s[..., :o] + s[..., o:2 * o]
        o >>= 1
    tot = _serial(s[..., 0])                   # the 4 wave sums added serially from 0.0
    nz = wp.reshape(nt, TILE) > 0
    last = np.where(nz.any(axis=1), np.arange(nt) * TILE + TILE - 1 - np.argmax(nz[:, ::-1], axis=1), -1)
    return tot, last.astype(np.int64)


def scan(sums):
    """replay_scan_kernel: the inclusive prefix of the tile sums as one workgroup of SCAN_W threads computes it
    (serial chunk sums, a Hillis-Steele scan per wave, wave offsets summed serially, then the serial run through each
    chunk)."""
    nt = len(sums)
    chunk = -(-nt // SCAN_W)
    c = np.zeros(SCAN_W * chunk)
    c[:nt] = sums                              # the padding adds 0.0: exact, as the threads that skip those tiles
    c = c.reshape(SCAN_W, chunk)
    incl = _hillis_steele(_serial(c).reshape(SCAN_W // 64, 64))
    off = np.zeros(SCAN_W // 64)
    for w in range(1, SCAN_W // 64):
        off[w] = off[w - 1] + incl[w - 1, 63]
    excl = np.zeros_like(incl)
    excl[:, 1:] = incl[:, :-1]
    run = (off[:, None] + excl).reshape(SCAN_W)
    out = np.empty_like(c)
    for i in range(chunk):
        run = run + c[:, i]
        out[:, i] = run
    return out.reshape(-1)[:nt]


def _search(prefix, x):
    """The draw kernel's binary search for the first tile whose prefix exceeds x.  Unlike np.searchsorted it assumes
    nothing of the order: it ends on a t with prefix[t - 1] <= x < prefix[t] even where rounding made prefix dip."""
    nt = len(prefix)
    lo = np.zeros(len(x), np.int64)
    hi = np.full(len(x), nt, np.int64)
    act = lo < hi
    while act.any():
        mid = (lo + hi) >> 1
        gt = prefix[np.minimum(mid, nt - 1)] > x
        hi = np.where(act & gt, mid, hi)
        lo = np.where(act & ~gt, mid + 1, lo)
        act = lo < hi
    return lo


class DeviceDraw:
    """draw_device's result: indices, weights (fp32, or None), branch per draw, u, total, pdraw and pmin."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def select_device(wp, count, u, parent=False, sums=None):
    """The tile, scan and draw kernels over fp32 weights w (any array of >= count entries; slots >= count weigh 0):
    (indices, branch, total); sums = tile_sums(w zero-padded to whole tiles) if the caller has it.  parent=True models the parent library, whose gap draws (LANE_GAP, TILE_GAP) fall
    through to its slot 0 clamp."""
    nt = -(-count // TILE)
    w = padded(wp, count)
    if sums is None:
        sums = tile_sums(w)
    prefix = scan(sums[0])
    tlast = np.maximum.accumulate(sums[1])     # the last slot with w > 0 in tiles <= t (the draw kernel's walk back)
    total = prefix[-1]
    u = np.asarray(u, np.float64)
    x = u * total
    t = _search(prefix, x)
    idx = np.full(len(u), -1, np.int64)
    branch = np.full(len(u), HIT, np.int64)
    over = t == nt
    idx[over] = tlast[-1]                      # x < total for every u <= 1 - 2^-53: never taken
    branch[over] = OVER
    for d in np.array_split(np.flatnonzero(~over), max(1, -(-int((~over).sum()) // 65536))):
        if not len(d):
            continue
        td = t[d]
        rem = x[d] - np.where(td > 0, prefix[np.maximum(td - 1, 0)], 0.0)
        ut, inv = np.unique(td, return_inverse=True)
        lw = w.reshape(nt, LANES, PER_LANE)[ut]                     # [tiles drawn][64][32]
        incl = _hillis_steele(_serial(lw))[inv]                     # [draws][64]
        lane_nz = (lw > 0).any(axis=2)
        lane_last = np.where(lane_nz, PER_LANE - 1 - np.argmax((lw > 0)[:, :, ::-1], axis=2), -1)
        hit = incl > rem[:, None]
        anyhit = hit.any(axis=1)
        L = np.argmax(hit, axis=1)
        excl = np.where(L > 0, incl[np.arange(len(d)), np.maximum(L - 1, 0)], 0.0)
        want = rem - excl
        mine = lw[inv, L]                                           # [draws][32]: lane L's weights
        c = np.add.accumulate(mine, axis=1)                         # serial, in the lane's order
        past = c > want[:, None]
        found = past.any(axis=1)
        base = td * TILE + L * PER_LANE
        slot = np.where(found, base + np.argmax(past, axis=1), -1)
        own = lane_last[inv, L]
        # lane fallbacks: lane L's own last slot with w > 0, else (fixed) the last one of the lanes before L
        prev_lane = np.where(lane_nz[inv] & (np.arange(LANES) < L[:, None]), np.arange(LANES), -1).max(axis=1)
        prev = np.where(prev_lane >= 0, td * TILE + np.maximum(prev_lane, 0) * PER_LANE
                        + lane_last[inv, np.maximum(prev_lane, 0)], -1)
        lgap = ~found & (own < 0)
        slot = np.where(~found & (own >= 0), base + own, slot)
        slot = np.where(lgap, -1 if parent else prev, slot)
        br = np.where(found, HIT, np.where(lgap, LANE_GAP, LANE_FALLBACK))
        # tile fallback: (parent) the tile's own last slot with w > 0; (fixed) the last one in tiles <= t
        tgap = ~anyhit & (sums[1][td] < 0)
        slot = np.where(~anyhit, sums[1][td] if parent else tlast[td], slot)
        br = np.where(~anyhit, np.where(tgap, TILE_GAP, TILE_FALLBACK), br)
        idx[d] = slot
        branch[d] = br
    idx[(idx < 0) | (idx >= count)] = 0        # the kernel's last guard: reached only by the parent's gap draws
    return idx, branch, total


def draw_device(prio, count, alpha, beta, seed, call, k, parent=False, u=None, weights=True, sums=None):
    """One sample call as the kernels compute it, bit for bit at alpha == 1 (powf is the device's otherwise).
    weights: (count * P(i))^-beta / (count * pmin)^-beta in fp64, then fp32, with P(i) = (double)w_i / total.
    sums: tile_sums of the same weights, when the caller draws from them more than once."""
    w = weights_fp32(np.asarray(prio)[:count], alpha)
    if u is None:
        u = uniforms_np(seed, call, k)
    idx, branch, total = select_device(w, count, u, parent=parent, sums=sums)
    pdraw = w[idx].astype(np.float64) / total
    pmin = pdraw.min()
    wts = None
    if weights:
        n = float(count)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            wts = ((n * pdraw) ** -beta / (n * pmin) ** -beta).astype(np.float32)
    return DeviceDraw(indices=idx, weights=wts, branch=branch, u=u, total=total, pdraw=pdraw, pmin=pmin)


# ---- rings whose draw j falls in a rounding gap (the regression of the zero-weight draw) --------------------------

def _f32_bits_max(pred, hi=0x7F7FFFFF):
    """The largest non-negative fp32 v (by bit pattern, so by value) with pred(v), pred monotone (true, then false)."""
    lo = 0
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if pred(float(np.uint32(mid).view(np.float32))):
            lo = mid
        else:
            hi = mid - 1
    return float(np.uint32(lo).view(np.float32))


def _tune_total(sums, tail, target):
    """Sets the tile sums at the positions `tail` (single-slot tiles, so a tile's sum is its one weight, exactly) one
    after the other, each to the largest fp32 value that keeps scan(sums)[-1] <= target: a coarse, a fine and a finer
    weight.  True if the total then equals target exactly."""
    for p in tail:
        def fits(v, p=p):
            sums[p] = v
            return scan(sums)[-1] <= target
        sums[p] = _f32_bits_max(fits)
    return scan(sums)[-1] == target


def _totals_for(x, u, span=64):
    """The totals T near x / u with fl(u * T) == x."""
    t0 = x / u
    out = []
    t = t0
    for _ in range(span):
        t = np.nextafter(t, -np.inf)
    for _ in range(2 * span + 1):
        if u * t == x:
            out.append(t)
        t = np.nextafter(t, np.inf)
    return out


def gap_ring(kind, seed, call=0, k=256, trials=200, ntiles=4):
    """Priorities (fp32 [count]) on which draw j of call `call` of a ring keyed by `seed` falls in a rounding gap, for
    the kernels as they stand (alpha = 1): (prio, count, j).

    kind 'lane': tile 0 holds wide-range weights with a few whole lanes of zeros; lane L is one of them whose
    Hillis-Steele scan rounds above every scan before it, and x = u_j * total is that largest earlier scan, so the
    rescan sends the draw to lane L, which holds no w > 0.  kind 'tile': ntiles single-slot tiles of wide-range weights,
    30 % of them zero; tile g is a zero tile whose prefix rounds above every prefix before it, and x is that largest
    earlier prefix.  Either way, the last three tiles hold one weight each (coarse, fine, finer), tuned by bisection
    until total is a value with fl(u_j * total) == x.  Slot 0 weighs 0."""
    u = uniforms_np(seed, call, k)
    rng = np.random.RandomState(seed & 0xFFFF)
    for _ in range(trials):
        nt = ntiles if kind == "tile" else 4
        p = np.zeros(nt * TILE, np.float32)
        if kind == "lane":
            lanes = (2.0 ** rng.uniform(-20, 20, (LANES, PER_LANE))).astype(np.float32)
            lanes[rng.choice(np.arange(1, 63), 8, replace=False)] = 0
            lanes[0, 0] = 0
            p[:TILE] = lanes.reshape(-1)
            incl = _hillis_steele(_serial(lanes.astype(np.float64)))
            best = np.maximum.accumulate(incl)
            cand = [L for L in range(1, LANES) if not lanes[L].any() and incl[L] > best[L - 1]]
            if not cand:
                continue
            x = best[cand[-1] - 1]
        else:
            main = nt - 3
            v = (2.0 ** rng.uniform(-20, 20, main)).astype(np.float32)
            v[rng.rand(main) < 0.3] = 0
            v[0] = 0
            pos = rng.randint(1, TILE, main)
            p[np.arange(main) * TILE + pos] = v
            pre = scan(np.concatenate([v, np.zeros(3)]).astype(np.float64))
            best = np.maximum.accumulate(pre)
            cand = [g for g in range(1, main) if v[g] == 0 and pre[g] > best[g - 1]]
            if not cand:
                continue
            x = best[cand[-1] - 1]
        sums = tile_sums(p.astype(np.float64))[0]
        base = scan(sums)[-1]
        order = np.argsort(-u)
        for j in order[u[order] * base < x][:8]:
            for target in _totals_for(x, u[j]):
                s = sums.copy()
                if not _tune_total(s, [nt - 3, nt - 2, nt - 1], target):
                    continue
                q = p.copy()
                q[(nt - 3) * TILE:] = 0
                q[np.arange(nt - 3, nt) * TILE] = s[nt - 3:]
                count = (nt - 1) * TILE + 1
                q = q[:count]
                idx, branch, _ = select_device(q, count, u)
                want = LANE_GAP if kind == "lane" else TILE_GAP
                if branch[j] == want:
                    return q, count, int(j)
    raise RuntimeError(f"no {kind} gap found in {trials} trials")
