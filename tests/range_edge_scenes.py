"""Scenes that put ONE range test of the step exactly one fp32 ulp inside, exactly on, or one ulp outside its threshold.

A plain helper (no tests here); it generalises `gen_ulp_edges` of oracle/gen_golden.py (g9: one constants point, one
shape, one role).  tests/test_range_edges_cpu.py checks the premises below for every scene the GPU file uses and pins
the oracle to the reference's recordings of the 2-D scenes (g10); tests/test_hip_range_edges.py runs the scenes on every
kernel form that takes such a decision.

A SCENE is one environment.  One designated pair -- a probe UAV `i` and its partner, a target `k` or a peer `j` -- is
collinear along x (same y, same z) or, in 3-D, separated along z alone (dx = dy = 0: a kernel that drops the altitude
term puts that pair at distance 0).  After the last move of the scene the distance the tested view sees is exactly
K-, K or K+: the threshold K and its two fp32 neighbours.  Everything flies with heading 0 and, in 3-D, the level climb
index (nc = 3, climb 1: cos 0 = 1, sin 0 = 0), so a move adds exactly dt * v to x and nothing else; every coordinate
before and after every move is an fp32 number, and so is every difference the designated test takes.  With
d2 = fl32(dx * dx): K- gives d2 < K^2, K+ gives d2 > K^2 (by one to three ulps of K^2: K^2 is an fp32 number in every
constants set) and K gives d2 == K^2.  A correct fp32 evaluation therefore has no room to differ from fp64: NOTHING of
these scenes may be set aside by margin.

The five thresholds, their view and K:
    dp_target   probe post-move vs target post-move          d <= dp     (observed, tracked)
    dp_cover    the same pair                                d <  dp     (covered: strict)
    dc_peer     probe post-move vs peer on the SEQUENTIAL view (j < i: post-move, j > i: PRE-move)    d <= dc
    2dp_dup     post-move vs post-move                       d <= 2 dp   (duplicate punishment)
    dp_nb       post-move vs post-move                       d <= dp     (cooperative neighbour)
(dp_target and dp_cover are the same placements: `on` is observed and not covered.)

Layout.  G = the power of two above dc + 2 dp.  Fillers -- every agent that is not of the designated pair -- sit on a grid
of pitch G at x = G (1 + col), y = G (2 + row): farther than dc + 2 dp from each other.  The designated pair lives on
the row y = G (a near-origin probe: y = 1/2), around x = 0, where the fp32 grid is fine enough for K- and K+; its x
offset and the side the partner is on are SEARCHED so that every coordinate of every step is an fp32 number.  UAVs may
fly outside the box (the reference has no wall for them, only the boundary term); targets stay strictly inside it, so
none is mirrored.  `check()` asserts all of this in fp64, and that every pair and view other than the designated one
is farther than 1 % of K from each of dp, dc and 2 dp (the designated pair's own other tests, each against the
thresholds its view is compared with: 0.01 % of K, more than 800 fp32 ulps -- `odd` has 2 dp = 362 next to dc = 363, and
`huge` has a 20 m move next to dc = 20480).

Two moves (na = 9, action 4 = zero turn at the first step): peers move in lockstep, so a peer threshold sits on its
knife edge at BOTH steps; a target threshold lands on it at the second.  The state after the first move is exact and
`check()` computes it, so an oracle can be given it directly.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

THRESHOLDS = ("dp_target", "dp_cover", "dc_peer", "2dp_dup", "dp_nb")
SIDES = ("inside", "on", "outside")
# A fourth side where dp^2 is a power of two (`pow2`, `huge`), for the target pair: x separation K- as `inside`, plus a y
# offset of 2^-12 dp.  fl32(dx * dx) is K^2 less TWO of the (halved) spacings below K^2 and the fma adds one back: the
# kernel's d2 is the LAST fp32 number below K^2 -- the smallest positive value the strict form d2 < K^2 ever meets, ulp(K^2) / 2.
# (K- alone gives d2 two spacings below K^2; a scale S one power of two short, `k = 24 - e` in fold_constants, passes that.)
BELOW = "below"

# dt = 1 everywhere.  u_v_max / t_v_max are the reference's 20 / 5 except where one move of 20 m cannot keep a coordinate
# pair one ulp(K) apart: `ratio` (K+ = 3 + 2^-22, and -17 + 2^-22 is no fp32 number) and `tiny` (K = 3/4) move 1 / 0.5 and
# 1/4 / 1/8 per step.
CONSTANTS = {
    "default":       dict(dp=200.0, dc=500.0),            # the yaml constants
    "census":        dict(dp=150.0, dc=400.0),            # the variant census's point
    "pow2":          dict(dp=256.0, dc=640.0),            # dp^2, 4 dp^2 powers of two: the spacing halves below K
    "dc-below-dp":   dict(dp=300.0, dc=120.0),            # kmin = dc^2
    "dc-below-step": dict(dp=48.0, dc=12.0),              # dc < dt * u_v_max = 20: an even lane's own pre-move pose is out of range
    "ratio":         dict(dp=3.0, dc=3000.0, u_v_max=1.0, t_v_max=0.5),      # large S against a large dc^2
    "tiny":          dict(dp=0.75, dc=2.5, u_v_max=0.25, t_v_max=0.125),     # S = 2^26, thresholds below 1
    "huge":          dict(dp=8192.0, dc=20480.0),         # dp^2 = 2^26: the k < 0 clamp, S = 1
    "odd":           dict(dp=181.0, dc=363.0),            # d^2 one ulp from K^2 on both sides
    "quarter":       dict(dp=173.25, dc=411.75),          # d^2 three ulps from K^2
}

Role = namedtuple("Role", "name i j near0")          # j: target index (target thresholds) or peer index
Scene = namedtuple("Scene", "name cs N M dim threshold side role family moves state actions box probe partner K Kside rows")


class NoPlacement(AssertionError):
    """No arrangement of the designated pair keeps every coordinate of every step an fp32 number (dc = 12 with two moves
    of 20 m and a later peer: its pre-move x carries 2^-20, and 32 m further on the grid is 2^-18)."""


def is_f32(v):
    return float(np.float32(v)) == float(v)


def constants(cs):
    """The full constants of a set: dp, dc, u_v_max, t_v_max (dt = 1) -- asserted exact in fp32 together with 2 dp and
    the three squares."""
    c = dict(u_v_max=20.0, t_v_max=5.0)
    c.update(CONSTANTS[cs])
    for k in (c["dp"], c["dc"], 2.0 * c["dp"]):
        assert is_f32(k) and is_f32(k * k), (cs, k)
    assert is_f32(c["u_v_max"]) and is_f32(c["t_v_max"])
    return c


def threshold_k(c, threshold):
    return {"dp_target": c["dp"], "dp_cover": c["dp"], "dc_peer": c["dc"], "2dp_dup": 2.0 * c["dp"], "dp_nb": c["dp"]}[threshold]


def k_side(K, side):
    k = np.float32(K)
    if side in ("inside", BELOW):
        return float(np.nextafter(k, np.float32(0.0)))
    if side == "outside":
        return float(np.nextafter(k, np.float32(np.inf)))
    return float(k)


def grid_pitch(c):
    return float(2.0 ** math.ceil(math.log2(c["dc"] + 2.0 * c["dp"]) + 1e-12))


def box(cs, N, M):
    """(x_max, y_max, z_max, G, cols) of every scene of a (constants set, shape): one configuration serves the batch."""
    c = constants(cs)
    G = grid_pitch(c)
    assert G > c["dc"] + 2.0 * c["dp"]
    cols = int(math.ceil(math.sqrt(N + M)))
    rows = (N + M + cols - 1) // cols
    zmax = max(512.0, 4.0 * max(c["dc"], 2.0 * c["dp"]))
    return G * (cols + 2), G * (rows + 3), zmax, G, cols


def roles(N, M, threshold):
    """The (probe, partner) index pairs of a shape: where the kernels' indexing differs."""
    out = []
    if threshold in ("dp_target", "dp_cover"):
        out += [Role("i-even-k-even", 0, 0, False), Role("i-odd-k-odd", 1, min(1, M - 1), False),
                Role("i-last-k-last", N - 1, M - 1, False)]          # M odd: the last, padded target pair
        if M >= 25:
            out.append(Role("k-second-word", 2, 24, False))            # coverage word 1 (12 target pairs per word)
        if M >= 4:
            out.append(Role("k-mid", 3, 2, False))
    else:
        out += [Role("i-even-j-lo-x", 2, 0, False), Role("i-even-j-lo-y", 2, 1, False),
                Role("i-odd-j-lo-x", 3, 0, False), Role("i-odd-j-same-pair", 3, 2, False),
                Role("i-even-j-same-pair", 2, 3, False),
                Role("i-even-j-hi-x", 0, N - 1 if N % 2 else N - 2, False),       # (N odd: slot .x of the last, padded pair)
                Role("i-odd-j-hi-y", 1, 3, False), Role("i-last-j-first", N - 1, 0, False),
                Role("i-0-j-opposite", 0, N // 2, False)]                        # sym_dup: the peer both ends evaluate (even N)
        if N >= 66:
            out += [Role("j-pair-32", 1, 64, False), Role("j-pair-32-y", 0, 65, False), Role("i-pair-34", 69, 2, False)]
    seen, uniq = set(), []
    for r in out:
        if (r.i, r.j) not in seen and (threshold in ("dp_target", "dp_cover") or r.i != r.j):
            seen.add((r.i, r.j)); uniq.append(r)
    return uniq


def near_origin_roles(N, M, threshold):
    """The probe within 2.5 m of the origin (the literal weighted sweep and its own mask loop)."""
    if threshold in ("dp_target", "dp_cover"):
        return [Role("near0-i-even", 0, 0, True), Role("near0-i-odd", 1, M - 1, True)]
    return [Role("near0-i-even-j-lo", 2, 1, True), Role("near0-i-odd-j-hi", 1, N - 1, True)]


_P_FAR = (4.0, 8.0, 2.0, 1.0, 16.0, 32.0, 0.0, -1.0, -2.0, -4.0, -8.0, -16.0, -32.0, 0.5, -0.5, 0.25, -0.25, 64.0, -64.0)
_P_NEAR = (1.0, 0.5, -0.5, -1.0, 1.5, -1.5, 2.0, -2.0, 0.25, -0.25, 0.0)


def _track(x_last_pre_or_post, v, moves, last_is_pre):
    """x of an agent before the first move and after each move, given where the LAST step sees it."""
    x0 = x_last_pre_or_post - v * ((moves - 1) if last_is_pre else moves)
    return [x0 + v * t for t in range(moves + 1)]


def _place(K, side, vu, vj, moves, partner_pre, target, near0):
    """Probe and partner x tracks with (seen partner x) - (probe post-move x) = +-K(side) and every coordinate an fp32
    number.  The probe's offset and the partner's side of it are the first that serve all three sides of K, so the three
    scenes of a knife edge differ in the partner's x alone."""
    def tracks(P, sgn, Ks):
        pi = _track(P, vu, moves, False)
        pj = _track(P + sgn * Ks, vj, moves, partner_pre)
        seen = pj[moves - 1] if partner_pre else pj[moves]
        ok = all(is_f32(v) for v in pi + pj) and not (target and min(pj) <= 0.0) and abs(seen - pi[moves]) == Ks
        return ok, pi, pj
    for sgn in ((1.0,) if target else (1.0, -1.0)):
        for P in (_P_NEAR if near0 else _P_FAR):
            if all(tracks(P, sgn, k_side(K, sd))[0] for sd in SIDES):
                return tracks(P, sgn, k_side(K, side))[1:]
    raise NoPlacement(f"no fp32 placement for K = {K!r}, moves {moves}")


def build(cs, N, M, dim, threshold, side, role, moves=1, family="x"):
    """One scene.  family "z" (3-D only): the pair is separated along z alone."""
    assert threshold in THRESHOLDS and side in SIDES + (BELOW,) and dim in (2, 3) and moves in (1, 2) and family in ("x", "z")
    assert family == "x" or dim == 3
    c = constants(cs)
    K = threshold_k(c, threshold)
    Ks = k_side(K, side)
    xmax, ymax, zmax, G, cols = box(cs, N, M)
    vu, vt = c["u_v_max"], c["t_v_max"]
    target = threshold in ("dp_target", "dp_cover")
    i, j = role.i, role.j
    assert 0 <= i < N and 0 <= j < (M if target else N) and (target or i != j)
    partner_pre = threshold == "dc_peer" and j > i          # the sequential view shows a later peer before its move

    # fillers on the grid; state = the pose before the first move
    ux = np.empty(N); uy = np.empty(N); tx = np.empty(M); ty = np.empty(M)
    for n in range(N + M):
        x, y = G * (1 + n % cols), G * (2 + n // cols)
        if n < N:
            ux[n], uy[n] = x, y
        else:
            tx[n - N], ty[n - N] = x, y
    uz = np.full(N, 64.0); tz = np.full(M, 64.0)
    ypair = 0.5 if role.near0 else G
    vj = vt if target else vu
    if family == "x":
        pi, pj = _place(K, side, vu, vj, moves, partner_pre, target, role.near0)
        zi = zj = 64.0
    else:           # dx = dy = 0 on the tested view, dz = Ks (z never changes: the level climb index)
        P = (1.0 if role.near0 else 8.0) + (vt * moves if target else 0.0)
        pi = _track(P, vu, moves, False)
        pj = _track(P, vj, moves, partner_pre)
        zi, zj = 0.0, Ks
    ux[i], uy[i], uz[i] = pi[0], ypair, zi
    if target:
        tx[j], ty[j], tz[j] = pj[0], ypair, zj
        if side == BELOW:
            assert family == "x" and has_below(cs)
            ty[j] = ypair + K * 2.0 ** -12
    else:
        ux[j], uy[j], uz[j] = pj[0], ypair, zj

    name = f"{cs}-{N}x{M}-{dim}d-{threshold}-{side}-{role.name}-m{moves}-{family}"
    # (actions and previous actions are drawn per (role, threshold, ...) and shared by the three sides)
    r = np.random.RandomState(zlib.crc32(name.replace(f"-{side}-", "-").encode()) & 0x7FFFFFFF)
    na = 9 if moves == 2 else 12
    turn = r.randint(0, na, size=(moves, N))
    turn[:moves - 1] = 4                                    # zero turn (2 a + 1 - na = 0) wherever another move follows
    actions = (turn + (na if dim == 3 else 0)).astype(np.int32)          # 3-D: climb index 1 of nc = 3 (level)
    state = dict(ux=ux, uy=uy, uh=np.zeros(N), ua=r.randint(0, na * (3 if dim == 3 else 1), size=N).astype(np.int32),
                 tx=tx, ty=ty, th=np.zeros(M))
    if dim == 3:
        state.update(uz=uz, tz=tz)
    # the rows whose outputs the side decides (the probe's; a symmetric test also decides the partner's)
    rows = (i,) if target or threshold == "dc_peer" else (i, j)
    sc = Scene(name, cs, N, M, dim, threshold, side, role, family, moves, state, actions,
               dict(x_max=xmax, y_max=ymax, z_max=zmax, na=na, nc=3 if dim == 3 else 1), i, j, K, Ks, rows)
    check(sc)
    return sc


def has_below(cs):
    """dp^2 is a power of two: the spacing of fp32 halves below it."""
    dp = constants(cs)["dp"]
    return math.frexp(dp * dp)[0] == 0.5


def states(sc):
    """The exact state before each move and after the last one: [moves + 1] dicts (x advances by dt * v, nothing else)."""
    c = constants(sc.cs)
    out = []
    for t in range(sc.moves + 1):
        s = {k: np.array(v, copy=True) for k, v in sc.state.items()}
        s["ux"] = sc.state["ux"] + c["u_v_max"] * t
        s["tx"] = sc.state["tx"] + c["t_v_max"] * t
        if t > 0:
            s["ua"] = sc.actions[t - 1].copy()
        out.append(s)
    return out


def _dist(ax, ay, az, bx, by, bz):
    return np.sqrt((ax - bx) ** 2 + (ay - by) ** 2 + (az - bz) ** 2)


def check(sc):
    """The premises, in fp64 (module docstring).  Raises AssertionError with the scene's name."""
    c = constants(sc.cs)
    dp, dc = c["dp"], c["dc"]
    N, M, i, j = sc.N, sc.M, sc.probe, sc.partner
    target = sc.threshold in ("dp_target", "dp_cover")
    assert not (sc.role.near0 and sc.moves != 1), sc.name
    st = states(sc)
    z = lambda s, k, n: s[k] if sc.dim == 3 else np.zeros(n)      # noqa: E731
    for s in st:
        for k in ("ux", "uy", "tx", "ty") + (("uz", "tz") if sc.dim == 3 else ()):
            assert all(is_f32(v) for v in s[k]), (sc.name, k)
        assert np.all(s["uh"] == 0.0) and np.all(s["th"] == 0.0)
        assert np.all((s["tx"] > 0) & (s["tx"] < sc.box["x_max"]) & (s["ty"] > 0) & (s["ty"] < sc.box["y_max"])), sc.name
    assert abs(c["u_v_max"] - dc) > 0.01 * dc, sc.name             # an even lane's own pre-move pose against dc

    def far(d, mask, ks, lim, what):
        for K in ks:
            rel = np.abs(d[mask] - K) / K
            assert rel.size == 0 or rel.min() > lim, (sc.name, what, K, float(rel.min()))

    for t in range(sc.moves):
        pre, post = st[t], st[t + 1]
        near = np.maximum(np.abs(post["ux"]), np.abs(post["uy"])) < 2.5
        want_near = np.zeros(N, bool)
        if sc.role.near0:
            want_near[i] = True
            if not target and near[j]:
                want_near[j] = True          # (thresholds below 2.5 m: the partner of a near-origin probe is near it too)
        assert np.array_equal(near, want_near), (sc.name, "near-origin lanes", np.nonzero(near)[0])
        ax, ay, az = post["ux"], post["uy"], z(post, "uz", N)
        dT = _dist(ax[:, None], ay[:, None], az[:, None], post["tx"][None], post["ty"][None], z(post, "tz", M)[None])
        dN = _dist(ax[:, None], ay[:, None], az[:, None], ax[None], ay[None], az[None])         # post-move peers
        # sequential view: row i sees column j < i after its move, j > i before it
        lower = np.arange(N)[None, :] < np.arange(N)[:, None]
        sx = np.where(lower, post["ux"][None], pre["ux"][None]); sy = np.where(lower, post["uy"][None], pre["uy"][None])
        sz = np.where(lower, az[None], z(pre, "uz", N)[None])
        dS = _dist(ax[:, None], ay[:, None], az[:, None], sx, sy, sz)
        # peers move in lockstep, so a peer threshold sits on its edge at every step; a target one at the last
        on_edge = (not target) or t == sc.moves - 1
        own_T = np.zeros((N, M), bool); own_N = np.zeros((N, N), bool); tested_T = own_T.copy(); tested_N = own_N.copy()
        tested_S = own_N.copy()
        if target:
            own_T[i, j] = True
            tested_T[i, j] = on_edge
            if on_edge and sc.side == BELOW:
                # the kernels' own d2 -- dx * dx rounded, then one fma -- is the last fp32 number below K^2; fp64 agrees: inside
                dx, dy = np.float32(post["tx"][j] - ax[i]), np.float32(post["ty"][j] - ay[i])
                assert float(dx) == post["tx"][j] - ax[i] and float(dy) == post["ty"][j] - ay[i], sc.name
                d2 = np.float32(float(dy) * float(dy) + float(np.float32(float(dx) * float(dx))))      # (both sums exact in fp64)
                k2 = np.float32(sc.K * sc.K)
                assert d2 == np.nextafter(k2, np.float32(0.0)) and k2 - d2 == np.spacing(k2) / 2, (sc.name, d2)
                assert sc.K - np.spacing(np.float32(sc.K)) < dT[i, j] < sc.K, (sc.name, dT[i, j])
            elif on_edge:
                assert dT[i, j] == sc.Kside, (sc.name, dT[i, j], sc.Kside)
        else:
            own_N[i, j] = own_N[j, i] = True
            if sc.threshold == "dc_peer":
                tested_S[i, j] = True
                assert dS[i, j] == sc.Kside, (sc.name, dS[i, j], sc.Kside)
            else:
                tested_N[i, j] = tested_N[j, i] = True
                assert dN[i, j] == sc.Kside and dN[j, i] == sc.Kside, (sc.name, dN[i, j], sc.Kside)
        off = ~np.eye(N, dtype=bool)
        # every other pair, on every view: 1 % from each of the three thresholds
        far(dT, ~own_T, (dp, dc, 2.0 * dp), 0.01, "target")
        far(dN, off & ~own_N, (dp, dc, 2.0 * dp), 0.01, "post-move peers")
        far(dS, off & ~own_N, (dp, dc, 2.0 * dp), 0.01, "sequential view")
        # the designated pair's own OTHER tests, each against the thresholds its view is compared with: 1e-4 of K,
        # more than 800 fp32 ulps of K
        far(dT, own_T & ~tested_T, (dp,), 1e-4, "pair: target")
        far(dN, own_N & ~tested_N, (dp, 2.0 * dp), 1e-4, "pair: post-move")
        far(dS, own_N & ~tested_S, (dc,), 1e-4, "pair: sequential view")
        if not target and sc.threshold != "dc_peer":          # the tested post-move distance against the OTHER post-move threshold
            other = dp if sc.threshold == "2dp_dup" else 2.0 * dp
            assert abs(dN[i, j] - other) > 1e-4 * other, sc.name
    return True


def all_scenes(cs, N, M, dim, moves=1, thresholds=("dp_target", "dc_peer", "2dp_dup", "dp_nb"), near_origin=False,
               families=None, skipped=None):
    """Every scene of a (constants set, shape, dim): thresholds x sides x roles (x the two families in 3-D).
    dp_cover is dp_target's placements, so it is left out by default: one batch compares the coverage count too.
    skipped: a list that receives the scenes no fp32 placement exists for (NoPlacement); None: such a scene raises."""
    out = []
    for fam in (families or (("x", "z") if dim == 3 else ("x",))):
        for th in thresholds:
            for role in (near_origin_roles if near_origin else roles)(N, M, th):
                for side in SIDES:
                    try:
                        out.append(build(cs, N, M, dim, th, side, role, moves, fam))
                    except NoPlacement:
                        if skipped is None:
                            raise
                        skipped.append((cs, N, M, dim, th, side, role.name, moves, fam))
                if th in ("dp_target", "dp_cover") and fam == "x" and has_below(cs):
                    out.append(build(cs, N, M, dim, th, BELOW, role, moves, fam))
    return out


def batch(scenes):
    """Scenes of one (constants set, shape, dim, moves) stacked: (state dict of [B, ...], actions [moves, B, N])."""
    keys = scenes[0].state.keys()
    st = {k: np.stack([s.state[k] for s in scenes]) for k in keys}
    for k in st:
        st[k] = st[k].astype(np.int32 if k == "ua" else np.float32)
    return st, np.stack([s.actions for s in scenes], axis=1).astype(np.int32)


def config(cs, N, M, dim, moves, n_envs, cooperative=0.0):
    """Keyword arguments shared by EnvConfig and OracleConfig."""
    c = constants(cs)
    xmax, ymax, zmax, _, _ = box(cs, N, M)
    kw = dict(n_envs=n_envs, n_uav=N, m_targets=M, dim=dim, na=9 if moves == 2 else 12, nc=3 if dim == 3 else 1,
              x_max=xmax, y_max=ymax, dt=1.0, u_v_max=c["u_v_max"], t_v_max=c["t_v_max"], dp=c["dp"], dc=c["dc"],
              cooperative=cooperative)
    if dim == 3:
        kw["z_max"] = zmax
    return kw


# ---- the batches the GPU file runs (tests/test_range_edges_cpu.py checks the premises of every scene in them) ---------
SPEC_SHAPES = ((5, 3), (10, 10), (20, 10), (50, 25))      # kSpecShapes (csrc/step_kernel.hip)
LONE_SHAPES = ((20, 10), (10, 10), (5, 3))                # the shapes with single-wavefront variants
GENERIC_SHAPES = ((7, 4), (70, 5))                        # the generic kernel: N <= 64 and N > 64
B_SETS = ("default", "pow2", "dc-below-step")
D_SETS = ("default", "tiny", "pow2")
Batch = namedtuple("Batch", "group cs N M dim moves near0")


def gpu_batches():
    out = []
    for cs in CONSTANTS:                                   # a: the constants axis
        for N, M in ((20, 10), (7, 4)):
            out.append(Batch("a", cs, N, M, 2, 1, False))
    for cs in B_SETS:                                      # b: the shape and dim axes
        for N, M in SPEC_SHAPES + GENERIC_SHAPES:
            for dim in (2, 3):
                if not (dim == 2 and (N, M) in ((20, 10), (7, 4))):      # (those are group a's)
                    out.append(Batch("b", cs, N, M, dim, 1, False))
    for cs in B_SETS:                                      # c: the single-wavefront variants and their forced-size siblings
        for N, M in LONE_SHAPES:
            for moves in (1, 2):
                out.append(Batch("c", cs, N, M, 2, moves, False))
    for cs in D_SETS:                                      # d: the probe within 2.5 m of the origin
        for N, M in ((20, 10), (7, 4)):
            out.append(Batch("d", cs, N, M, 2, 1, True))
    return out


G10_SHAPES = ((5, 3), (4, 2), (6, 3))      # every set: (5, 3) and, alternating, one of the other two


def g10_groups():
    """(group name, constants set, N, M, MAAC-R?) of tests/golden/g10_ulp_edges_constants.npz: the 2-D one-move scenes
    oracle/gen_golden.py records from the reference -- MAAC-G at every set, MAAC-R (H = 64) at B_SETS."""
    out = []
    for n, cs in enumerate(CONSTANTS):
        for N, M in (G10_SHAPES[0], G10_SHAPES[1 + n % 2]):
            out.append((f"{cs}_n{N}m{M}_mean", cs, N, M, False))
        if cs in B_SETS:
            out.append((f"{cs}_n5m3_pmi_h64", cs, 5, 3, True))
    return out


def batch_id(b):
    return f"{b.group}-{b.cs}-{b.N}x{b.M}-{b.dim}d-m{b.moves}{'-near0' if b.near0 else ''}"


_SCENES = {}


def batch_scenes(b):
    """The scenes of a batch (built once per process) and the ones no fp32 placement exists for."""
    key = tuple(b)[1:]
    if key not in _SCENES:
        skipped = []
        _SCENES[key] = (all_scenes(b.cs, b.N, b.M, b.dim, b.moves, near_origin=b.near0, skipped=skipped), skipped)
    return _SCENES[key]


def exact_state(scenes, t):
    """The exact state before move t of every scene, stacked (fp64: every value is an fp32 number)."""
    per = [states(s)[t] for s in scenes]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def oracle_steps(scenes, cooperative, pmi=None, n_threads=8):
    """The fp64 oracle on stacked scenes of one batch: one result dict per move, each from the exact state before it."""
    from oracle import OracleConfig, OracleEnv
    s0 = scenes[0]
    orc = OracleEnv(OracleConfig(**config(s0.cs, s0.N, s0.M, s0.dim, s0.moves, len(scenes), cooperative)), n_threads=n_threads)
    orc.pmi = pmi
    _, acts = batch(scenes)
    out = []
    for t in range(s0.moves):
        orc.set_state(**exact_state(scenes, t))
        out.append(orc.step(acts[t]))
    return out
