"""fp64 mirror of the MAAC-R mix (csrc/pmi_kernel.hip, pmi_mix_kernel; uav.py:262-291, environment.py:222-226), the error
bounds its tests use, hand-placed scenes, the score-spread ladder and a restatement of the LONE slot pool's bookkeeping.
numpy only: test_maacr_mix_cpu.py runs it against the oracle without a GPU, test_hip_maacr_mix.py against the device.

The bounds are derived, never measured.

Leg A (device against the oracle, end to end).  The scorer's own asserted bound is eps = 1e-5 max(1, mag) per score
(test_hip_round3 / test_hip_round4; mag = sum |terms| of the fp32 evaluation, conftest.pmi_forward_fp64(want_scale=True)).
A softmax weight moves by at most a factor exp(+-2 eps) when every score moves by at most eps, so a convex combination
of the neighbours' raw rewards moves by at most (exp(2 eps) - 1) (max_j raw_j - min_j raw_j):
    bound_A(i) = ATOL + coop (exp(2 eps_i) - 1) (max_j raw_j - min_j raw_j),     eps_i = 1e-5 max(1, max_j mag_ij),
ATOL being test_hip_parity's constant for an fp32 reward of O(1).

Leg B (the mix alone: the device's reward against mix_fp64 of the device's OWN scores and raw rewards):
    bound_B(i) = 2^-22 (k_i + 8) R_i + 2^-23,        k_i neighbours, R_i = max(|raw_i|, max_j |raw_j|).
Where it comes from, u = 2^-24: the subtraction s - mx, the rounded log2(e) constant and the product each cost one u
relative in the exponent d log2(e), 3 u together; a weight e^d moves by |d| e^d <= 1/e of that, under 2 u on the scale of
the largest weight (which is exactly 1), and v_exp_f32 adds one ulp (2 u): under 4 u = 2^-22 per term, k terms in the
numerator (each times |raw_j| <= R).  The two k-term fp32 sums (numerator by fused multiply-add, denominator by adds),
the division, the two fused multiply-adds ((1 - a) raw_i, then a * mix on top) and the rounding of 1 - a are at most 2 u
each on values bounded by R: the 8 R.  2^-23 is half an ulp of a result next to the clip at +-1.

Mean and episode sum (rsum = ascending fp32 sum over the N UAVs times fp32(1 / N); ep_sums[:, 0] = 16 slices of every
16th step, each summed ascending, added in order):
    bound_S = 2^-24 (N + ceil(S / 16) + 18) sum |r|,        sum |r| = sum_t sum_i |r_ti| / N:
N - 1 additions, the rounding of 1 / N and the product per step, ceil(S / 16) - 1 additions per slice, 15 for the slices,
to first order in u, rounded up.
"""
import math

import numpy as np

DP = 200.0
MIN_EDGE_MARGIN = 0.01 * DP          # every pair at least 1 % of dp away from dp
MIN_ORIGIN = 50.0                    # no UAV this close to the origin (the f16 range watch stays silent)
# With the reference's reward weights (0.6, 0.2, 0.2) the raw reward lies in [-0.4, 0.6] and no mix can reach the clip at
# +-1; the "clip" scene batches run with these instead
CLIP_WEIGHTS = dict(alpha=2.4, beta=1.0, gamma=1.0)


# ------------------------------------------------------------------------------------------------- the mix

def neighbour_sets(poses, dp=DP):
    """poses: (x, y) or (x, y, z), each [N] -> list of ascending neighbour index arrays (d <= dp, j != i), fp64."""
    p = np.stack([np.asarray(c, dtype=np.float64) for c in poses if c is not None], axis=1)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    nb = (d <= dp) & ~np.eye(len(p), dtype=bool)
    return [np.flatnonzero(r) for r in nb]


def pair_distances(poses):
    p = np.stack([np.asarray(c, dtype=np.float64) for c in poses if c is not None], axis=1)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    return d[np.triu_indices(len(p), 1)]


def mix_fp64(poses, raw, scores_of_pair, dp=DP, coop=0.3, round_weights=False, want_unclipped=False):
    """One environment.  raw [N]; scores_of_pair: callable (i, j) -> score, or a dict keyed by (i, j) (every ordered
    neighbour pair).  -> (reward [N], mean over the UAVs).  round_weights rounds every softmax weight to fp32 the way the
    oracle does (uav_oracle.c, "scipy softmax on fp32"); the device keeps fp32 throughout, so leg B leaves it off."""
    raw = np.asarray(raw, dtype=np.float64)
    get = scores_of_pair if callable(scores_of_pair) else (lambda i, j: scores_of_pair[(i, j)])
    out = np.empty(len(raw))
    for i, nb in enumerate(neighbour_sets(poses, dp)):
        if len(nb) == 0:
            out[i] = (1.0 - coop) * raw[i]
            continue
        s = np.array([get(i, int(j)) for j in nb], dtype=np.float64)
        e = np.exp(s - s.max())
        w = e / e.sum()
        if round_weights:
            w = w.astype(np.float32).astype(np.float64)
        acc = 0.0
        for wj, j in zip(w, nb):          # ascending j, the oracle's order
            acc += raw[j] * wj
        out[i] = (1.0 - coop) * raw[i] + coop * acc
    if want_unclipped:
        return out
    out = np.clip(out, -1.0, 1.0)
    return out, out.mean()


def pair_inputs(obs, nbs, dtype=np.float32):
    """The scorer's inputs la_i * la_j of every ordered neighbour pair -> (keys [(i, j)], x [n, 12] fp32): one IEEE
    multiply in `dtype`, rounded to fp32 (fp32 rows: what the kernels compute; fp64 rows: what the oracle feeds)."""
    obs = np.asarray(obs, dtype=dtype)
    keys = [(i, int(j)) for i, nb in enumerate(nbs) for j in nb]
    if not keys:
        return keys, np.zeros((0, 12), np.float32)
    ii, jj = np.array(keys).T
    return keys, (obs[ii] * obs[jj]).astype(np.float32)


def leg_a_bound(nbs, raw, mag_of_pair, coop, atol):
    raw = np.asarray(raw, dtype=np.float64)
    out = np.full(len(raw), atol)
    for i, nb in enumerate(nbs):
        if len(nb):
            eps = 1e-5 * max(1.0, max(mag_of_pair[(i, int(j))] for j in nb))
            out[i] += coop * math.expm1(2.0 * eps) * (raw[nb].max() - raw[nb].min())
    return out


def leg_a_second_term(nbs, raw, mag_of_pair, coop):
    return leg_a_bound(nbs, raw, mag_of_pair, coop, 0.0)


def leg_b_bound(nbs, raw):
    raw = np.abs(np.asarray(raw, dtype=np.float64))
    k = np.array([len(nb) for nb in nbs], dtype=np.float64)
    R = np.array([max(raw[i], raw[nb].max() if len(nb) else 0.0) for i, nb in enumerate(nbs)])
    return 2.0 ** -22 * (k + 8.0) * R + 2.0 ** -23


def sum_bound(rewards, N, extra_adds=0):
    """rewards [S, N] of one environment (or [N] for one step's mean) -> bound on the fp32 mean / episode sum.
    extra_adds: additions beyond one call's -- a call that scores its steps in several chunks adds each chunk's sum onto
    the running value (the number of chunks), a step-by-step accumulation adds every step's (S): one more rounding each."""
    r = np.abs(np.asarray(rewards, dtype=np.float64)).reshape(-1, N)
    return 2.0 ** -24 * (N + math.ceil(len(r) / 16) + 18 + extra_adds) * r.sum() / N


def in_neighbourhood_spread(nbs, score_of_pair):
    """max over the UAVs with two or more neighbours of max_j s_ij - min_j s_ij (0.0 when there is none)."""
    out = 0.0
    for i, nb in enumerate(nbs):
        if len(nb) >= 2:
            s = [score_of_pair[(i, int(j))] for j in nb]
            out = max(out, max(s) - min(s))
    return out


# ------------------------------------------------------------------------------------------------- the ladder

RUNGS = (0, 1, 64, 4096)             # chosen in test_maacr_mix_cpu.py from the scenes' in-neighbourhood spreads
LEG_A_RUNGS = (0, 1)                 # where leg A's second term stays below 1e-3 (asserted there)
TOP_RUNG = RUNGS[-1]


def spread_ladder(sd, c):
    """`sd` with fc2.weight and fc2.bias times c (0 or a power of two: exact in fp32 and fp64): every score times c."""
    assert c == 0 or (c > 0 and math.log2(c) == int(math.log2(c))), c
    out = {k: np.array(v) for k, v in sd.items()}
    out["fc2.weight"] = (out["fc2.weight"] * np.float32(c)).astype(np.float32)
    out["fc2.bias"] = (out["fc2.bias"] * np.float32(c)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------- launch geometry

def mix_geometry(N):
    """(workgroup, E instances per group, groups per workgroup, WS) of pmi_mix_kernel for N UAVs (launch_pmi_finalize)."""
    if N <= 64 and (64 // N) * N * 10 >= 64 * 9:
        wgs = 64
    else:
        wgs = 256 if N <= 256 else 1024
    return wgs, wgs // N, (4 if N <= 64 else 1), (1 if N <= 32 else 2 if N <= 64 else 0)


# ------------------------------------------------------------------------------------------------- scenes

# (N, M, dim): the rollout's three emitters (specialised pipe: 20x10 10x10 5x3 50x25; generic elsewhere; the multi-word
# records past 64 UAVs, which keep isolated pairs), the mix's three instantiations (WS = 1 up to 32 UAVs, 2 up to 64, 0
# beyond) and its group shapes (E = 9 at 7 UAVs, 256-thread groups with E = 7 at 33, E = 1 at 64 and 130)
SHAPES = ((20, 10, 2), (10, 10, 2), (5, 3, 2), (7, 4, 2), (32, 6, 2), (33, 6, 2), (50, 25, 2), (64, 6, 2), (65, 5, 2),
          (70, 5, 2), (130, 5, 2), (20, 10, 3), (7, 4, 3))
COOPS = (0.0, 0.3, 1.0)
KINDS = ("open", "clip", "dense")
MIN_ORACLE_MARGIN = 0.005      # metres, every range / wall test of a scene's step: 20 times test_hip_parity's MARGIN


def scenes_of(N, M, dim, kind):
    return dense_scenes(N, M, dim=dim) if kind == "dense" else build_scenes(N, M, dim=dim)


def config_kwargs(N, M, dim, kind, coop, B):
    """Environment constants of a scene batch, for OracleConfig and EnvConfig alike."""
    kw = dict(n_envs=B, n_uav=N, m_targets=M, cooperative=coop, dim=dim)
    if dim == 3:
        kw.update(nc=3, z_max=300.0)
    if kind == "dense":
        kw.update(x_max=600.0, y_max=500.0)
    if kind == "clip":
        kw.update(CLIP_WEIGHTS)
    return kw


def poses_of(state, b, dim):
    return (state["ux"][b], state["uy"][b], state["uz"][b] if dim == 3 else None)


HEADING = 0.3
ACTION = 5            # every UAV takes the same action: the swarm translates rigidly, the graph holds over a launch


def rigid_actions(T, B, N, dim=2, na=12):
    """Alternating actions 5 and 6 (-/+ the smallest turn rate; level flight in 3-D) for every UAV."""
    a = np.where(np.arange(T) % 2 == 0, 5, 6) + (na if dim == 3 else 0)
    return np.broadcast_to(a[:, None, None], (T, B, N)).astype(np.int32).copy()


def _lattice():
    pts = [(150.0 + 260.0 * a, 150.0 + 260.0 * b) for a in range(16) for b in range(16)]
    return sorted(pts, key=lambda p: (max(p), p[0]))


def _place(struct, N, keep_clear=()):
    """struct {index: (x, y)} -> [N, 2]: the other UAVs go to lattice points more than 1.15 dp from everything placed
    (and from the points of `keep_clear`)."""
    xy = np.full((N, 2), np.nan)
    for i, p in struct.items():
        xy[i] = p
    placed = [tuple(p) for p in struct.values()] + [tuple(p) for p in keep_clear]
    lat = iter(_lattice())
    for i in range(N):
        if i in struct:
            continue
        while True:
            c = next(lat)
            if all(math.hypot(c[0] - p[0], c[1] - p[1]) > 1.15 * DP for p in placed):
                break
        xy[i] = c
        placed.append(c)
    return xy


def _grid(n, x0, y0, step=5.0):
    w = int(math.ceil(math.sqrt(n)))
    return [(x0 + step * (k % w), y0 + step * (k // w)) for k in range(n)]


def _star(N, hub):
    leaves = min(5, N - 1)
    others = [i for i in range(N) if i != hub]
    pick = [others[(k * len(others)) // leaves] for k in range(leaves)]      # leaves spread over the index range
    c = (800.0, 800.0)
    st = {hub: c}
    for k, i in enumerate(pick):
        a = 2.0 * math.pi * k / max(leaves, 4) + 0.2
        st[i] = (c[0] + 190.0 * math.cos(a), c[1] + 190.0 * math.sin(a))
    edges = {(min(hub, i), max(hub, i)) for i in pick}
    return st, edges


def _clique(idx, x0, y0):
    idx = list(idx)
    st = dict(zip(idx, _grid(len(idx), x0, y0)))
    return st, {(a, b) for a in idx for b in idx if a < b}


def scene_specs(N):
    """name -> ({index: (x, y)}, expected edge set) of the hand-placed graphs for a swarm of N."""
    sc = {}
    sc["empty"] = ({}, set())
    if N >= 2:
        sc["isolated_pair"] = ({0: (700.0, 700.0), 1: (780.0, 700.0)}, {(0, 1)})
        sc["edge_0_last"] = ({0: (700.0, 700.0), N - 1: (780.0, 700.0)}, {(0, N - 1)})
    if N >= 3:
        for name, hub in (("star_hub_first", 0), ("star_hub_middle", N // 2), ("star_hub_last", N - 1)):
            sc[name] = _star(N, hub)
        L = min(N, 10)
        sc["chain"] = ({i: (300.0 + 150.0 * i, 420.0) for i in range(L)}, {(i, i + 1) for i in range(L - 1)})
        sc["clique_all"] = _clique(range(N), 900.0, 900.0)
    if N >= 5:
        # two cliques (lower / upper half of the indices) whose only link is the edge (h - 1, h): each of the two stands
        # 120 m in front of its own clique, 190 m from the other
        h = N // 2
        sa, ea = _clique(range(0, h - 1), 300.0, 900.0)
        ax = 300.0 + 5.0 * (math.ceil(math.sqrt(max(h - 1, 1))) - 1) + 120.0
        sb, eb = _clique(range(h + 1, N), ax + 190.0 + 121.7, 901.9)       # (off the 5 m raster: no distance of exactly 2 dp)
        st = {**sa, **sb, h - 1: (ax, 910.0), h: (ax + 190.0, 911.3)}
        edges = ea | eb | {(i, h - 1) for i in range(h - 1)} | {(h, j) for j in range(h + 1, N)} | {(h - 1, h)}
        sc["two_cliques"] = (st, edges)
    if N > 32:
        # non-isolated edges across the mask words' seams: a clique over bits 0, 30..33 and, from 64 UAVs on, 61..min(65, N - 1)
        st, edges = _clique([0, 30, 31, 32] + ([33] if N > 33 else []), 500.0, 700.0)
        if N >= 64:
            s2, e2 = _clique(range(61, min(66, N)), 1200.0, 700.0)
            st.update(s2); edges |= e2
        sc["word_seams"] = (st, edges)
    return sc


def _targets(xy, M, near=None):
    """M targets, each a few tens of metres from one of the UAVs `near` (default: all), at offsets that all differ."""
    near = sorted(near) if near else list(range(len(xy)))
    t = np.empty((M, 2))
    for k in range(M):
        i = near[(k * 3) % len(near)]
        t[k] = xy[i] + np.array([40.0 + (37.0 * k) % 90.0, -35.0 + (23.0 * k) % 60.0])
    return t


def build_scenes(N, M, dim=2):
    """-> (names, state dict of float32 [B, ...] arrays for set_state, expected edge sets).  One environment per graph
    of scene_specs(N), plus "wall_chain": a chain along the wall x = 0 whose first node starts outside the box and whose
    second and third stand on all M targets (duplicate tracking) -- with CLIP_WEIGHTS its rows leave [-1, 1]."""
    specs = scene_specs(N)
    names, xs, ts, edges = [], [], [], []
    for name, (st, ed) in specs.items():
        xy = _place(st, N)
        names.append(name); xs.append(xy); ts.append(_targets(xy, M, st.keys())); edges.append(ed)
    if N >= 3:
        L = min(N, 4)
        st = {i: (-60.0 + 150.0 * i, 900.0) for i in range(L)}
        xy = _place(st, N)
        t = np.array([[230.0 + 8.0 * (k % 5), 905.0 + 6.0 * (k // 5)] for k in range(M)])
        names.append("wall_chain"); xs.append(xy); ts.append(t); edges.append({(i, i + 1) for i in range(L - 1)})
    return names, _state(np.array(xs), np.array(ts), dim), edges


def dense_scenes(N, M, B=3, dim=2, seed=0, box=(600.0, 500.0)):
    """Bulk: B random swarms in a 600 x 500 box, drawn one UAV at a time so that every pair keeps MIN_EDGE_MARGIN from dp."""
    r = np.random.RandomState(seed + 1000 * N)
    xs = np.empty((B, N, 2))
    for b in range(B):
        for i in range(N):
            while True:
                c = np.array([r.uniform(60.0, box[0] - 10.0), r.uniform(60.0, box[1] - 10.0)])
                d = np.hypot(*(xs[b, :i] - c).T) if i else np.zeros(0)
                if (np.abs(d - DP) > 2.0 * MIN_EDGE_MARGIN).all() and (np.abs(d - 2.0 * DP) > 0.5).all() and (d > 1.0).all():
                    break
            xs[b, i] = c
    ts = np.stack([np.column_stack([r.uniform(30.0, box[0] - 30.0, M), r.uniform(30.0, box[1] - 30.0, M)]) for _ in range(B)])
    return [f"dense{b}" for b in range(B)], _state(xs, ts, dim), None


def _state(xs, ts, dim):
    B, N, M = xs.shape[0], xs.shape[1], ts.shape[1]
    st = dict(ux=xs[..., 0], uy=xs[..., 1], uh=np.full((B, N), HEADING), ua=np.full((B, N), ACTION),
              tx=ts[..., 0], ty=ts[..., 1], th=np.broadcast_to(0.5 + 0.9 * np.arange(M), (B, M)))
    if dim == 3:
        st["uz"] = np.broadcast_to(150.0 + 10.0 * (np.arange(N) % 4), (B, N))
        st["tz"] = np.full((B, M), 150.0)
    return {k: np.ascontiguousarray(v, dtype=np.int32 if k == "ua" else np.float32) for k, v in st.items()}


def edges_of(nbs):
    return {(i, int(j)) for i, nb in enumerate(nbs) for j in nb if i < j}


def emitted_runs(nbs, drop_isolated=True):
    """Per UAV, the pairs it emits (neighbours j > i), isolated pairs left out as step_kernel.hip's drop_isolated does."""
    runs = []
    for i, nb in enumerate(nbs):
        later = [int(j) for j in nb if j > i]
        if drop_isolated and len(nb) == 1 and len(nbs[int(nb[0])]) == 1:
            later = []
        runs.append(len(later))
    return runs


# ------------------------------------------------------------------------------------------------- the slot pool

POOL_BLOCK = 64
POOL_BRANCHES = ("fits", "split_run", "request_too_small", "last_step_exact", "block_never_used")


def pool_branches(runs_per_step):
    """The LONE (single-wavefront) rollout variant's pair-slot pool, restated for one wavefront from step_kernel.hip
    (kPoolEmit): runs_per_step[t] lists, in lane order, how many pairs each of the wavefront's UAVs emits at step t.
    -> (set of branches that ran, slots reserved from the global pair list).  A step whose pairs fit what is left of the
    block takes them ("fits"); otherwise the lanes whose run still fits keep the old block and the others move on as one
    piece ("split_run" when both groups are non-empty), onto the block requested earlier -- unless that request is
    smaller than what moves ("request_too_small": it is filled with dummies and a fresh one made) -- or onto a fresh
    request of max(moved, 64) slots -- but exactly `moved` on the launch's last step ("last_step_exact": recorded only
    where that clause decides, i.e. at most a block moves; more than a block is taken exactly on any step).  After each step a
    block is requested early when less than twice the step's pairs are left and two more steps follow (max(4 total, 64)
    slots); one that is still outstanding at the end was never used ("block_never_used")."""
    T = len(runs_per_step)
    left = 0
    pend, pend_size = False, 0
    seen, reserved = set(), 0
    for t, runs in enumerate(runs_per_step):
        total = sum(runs)
        if total > left:
            slot, moved = 0, 0
            for mine in runs:
                if mine and slot + mine > left:
                    moved += mine
                slot += mine
            if moved < total:
                seen.add("split_run")
            if pend and pend_size < moved:
                seen.add("request_too_small")
                pend = False
            if not pend:
                # `moved > kPoolBlock || t + 1 == p.T`: the last-step clause decides only where at most a block moves
                exact = t + 1 == T and moved <= POOL_BLOCK
                pend_size = moved if (moved > POOL_BLOCK or exact) else POOL_BLOCK
                if exact:
                    seen.add("last_step_exact")
                reserved += pend_size
            left = pend_size - moved
            pend = False
        else:
            if total:
                seen.add("fits")
            left -= total
        if not pend and left < 2 * total and t + 2 < T:
            pend_size = max(4 * total, POOL_BLOCK)
            reserved += pend_size
            pend = True
    if pend:
        seen.add("block_never_used")
    return seen, reserved


# ------------------------------------------------------------------------------------------------- scenes for the pool

POOL_SHAPES = ((20, 10, 3), (10, 10, 6), (5, 3, 12))       # N, M, environments per wavefront
POOL_LAUNCHES = (16, 17, 32, 36)
COLLAPSE_STEP = 31                                         # the step at which the ring's isolated pairs merge
JOIN_STEP = 15                                             # the step at which the "join" scene's third UAV arrives
TURN = (math.pi / 6.0) / 11.0                              # |turn rate| of actions 5 and 6
_RING_PHI = {2: 0.05, 5: 0.01, 10: 0.004}                  # half the angle between the two UAVs of a pair, by pairs on the ring


def _ring(N, t_star=COLLAPSE_STEP, centre=(1000.0, 1000.0)):
    """N // 2 isolated pairs on a ring, every UAV heading for the centre (20 m per step under the alternating actions):
    neighbouring pairs come within dp of each other -- all four cross distances, all around the ring -- between the moves
    of steps t_star - 1 and t_star, the radius centred in the window that leaves both sides the widest margin.  An odd
    UAV out flies away from far outside.  -> (xy [N, 2], heading [N])."""
    K = N // 2
    phi = _RING_PHI[K]
    ang = np.array([2.0 * math.pi * k / K + 0.05 + s * phi for k in range(K) for s in (-1.0, 1.0)])
    unit = np.column_stack([np.cos(ang), np.sin(ang)])
    d = np.sqrt(((unit[:, None] - unit[None]) ** 2).sum(-1))
    pair = np.arange(2 * K) // 2
    adjacent = ((pair[:, None] - pair[None]) % K == 1) | ((pair[None] - pair[:, None]) % K == 1)
    fmax, fmin = d[adjacent].max(), d[adjacent].min()
    step = 20.0 * math.cos(TURN / 2.0)
    r_star = 0.5 * ((DP + 2.0) / fmin - step + (DP - 2.0) / fmax)
    r0 = r_star + step * (t_star + 1)
    xy = np.empty((N, 2)); h = np.empty(N)
    xy[:2 * K] = np.asarray(centre) + r0 * unit
    h[:2 * K] = ang + math.pi + TURN / 2.0
    if N % 2:
        xy[N - 1] = (centre[0], centre[1] - 1700.0)
        h[N - 1] = -math.pi / 2.0
    return xy, (h + math.pi) % (2.0 * math.pi) - math.pi


def pool_scenes(N, M, E):
    """name -> state of E environments (one wavefront of the LONE variant).  "steady": a rigid chain in every environment,
    the same pair count every step.  "collapse": environment 0 holds a chain of three (2 pairs per step: the 64-slot block
    drains slowly and its successor is requested at step 30), the others only isolated pairs on a contracting ring, which
    emit nothing until they merge at COLLAPSE_STEP -- more than 64 pairs at once.  "disperse" and "join": a chain whose
    third UAV drifts out of range (the block requested for it is never used) or into range (the first pairs arrive on a
    launch's last step), see below."""
    L = min(N, 10)
    chain = _place({i: (300.0 + 150.0 * i, 420.0) for i in range(L)}, N)
    three = _place({i: (300.0 + 150.0 * i, 420.0) for i in range(3)}, N)
    ring, ring_h = _ring(N)
    out = {}
    xs = np.stack([chain] * E)
    out["steady"] = _state(xs, np.stack([_targets(x, M) for x in xs]), 2)
    xs = np.stack([three] + [ring] * (E - 1))
    # (the ring's targets wait around the centre, unevenly: when the pairs merge, some of their UAVs track and some do
    # not, so the merged neighbours' raw rewards differ and a score read from the wrong slot shows)
    mid = np.array([[1000.0 + (120.0 + (37.0 * k) % 200.0) * math.cos(2.4 * k),
                     1000.0 + (120.0 + (37.0 * k) % 200.0) * math.sin(2.4 * k)] for k in range(M)])
    st = _state(xs, np.stack([_targets(three, M)] + [mid] * (E - 1)), 2)
    st["uh"][1:] = ring_h.astype(np.float32)
    out["collapse"] = st
    # "disperse": environment 0 holds an L-shaped chain 0 - 1 - 2 whose UAV 2 flies 0.5 rad off the common heading: it
    # drifts past UAV 1 at 9.9 m per step, 80 m to the side, and leaves its range between the moves of steps 30 and 31 (never
    # entering UAV 0's, 150 m to the other side).  2 pairs per step, then none: the pair (0, 1) that is left is isolated.
    # Everything else is isolated throughout, so the block requested at step 30 is never used.
    # "join": the same drift, entering: UAV 2 comes into UAV 1's range between the moves of steps JOIN_STEP - 1 and
    # JOIN_STEP.  Nothing is emitted before (the pair (0, 1) is isolated), so a launch of JOIN_STEP + 1 steps meets its
    # first 2 pairs on its last step with no block in hand and none requested: the exact last-step reservation of 2 slots.
    dh = 0.5
    rel = 40.0 * math.sin(dh / 2.0)
    e1 = np.array([math.cos(HEADING + dh / 2.0 + math.pi / 2.0), math.sin(HEADING + dh / 2.0 + math.pi / 2.0)])
    e2 = np.array([-e1[1], e1[0]])
    p1 = np.array([700.0, 700.0])
    side = 80.0
    x_exit = math.sqrt(DP ** 2 - side ** 2)
    lone = _place({}, N)
    # (0.3 and not 0.5 of a step: under the alternating actions the drift is not quite parallel, UAV 2 comes 4 m closer
    #  to UAV 1's line over 31 steps and leaves later; the CPU test holds both crossings to the 1 % margin)
    for name, x0 in (("disperse", x_exit - rel * (COLLAPSE_STEP + 0.3)), ("join", -x_exit - rel * (JOIN_STEP + 0.5))):
        path = [p1 + (x0 + rel * t) * e1 + side * e2 for t in range(0, 44, 4)]
        ell = _place({0: tuple(p1 - 150.0 * e2), 1: tuple(p1), 2: tuple(path[0])}, N, keep_clear=path)
        xs = np.stack([ell] + [lone] * (E - 1))
        st = _state(xs, np.stack([_targets(x, M) for x in xs]), 2)
        st["uh"][0, 2] = np.float32(HEADING + dh)
        out[name] = st
    return out


def wave_runs(poses_per_env, drop_isolated=True):
    """One wavefront's emitted pairs per lane (environment-major, UAV-minor) from its environments' post-move poses."""
    return [r for p in poses_per_env for r in emitted_runs(neighbour_sets(p), drop_isolated)]
