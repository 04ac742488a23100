"""Scenes of the greedy baseline policy (UAV.get_action_by_direction, reference src/agent/uav.py:324-369) shared by
tests/test_greedy_cpu.py (the oracle alone) and tests/test_hip_greedy.py (the device against the oracle).  Plain numpy, no
tests here.

(a) SHAPES: the stand-alone kernel's own geometry (csrc/policy_kernel.hip, launch_greedy) -- the 256- and the 512-thread
    path, E = whole environments per workgroup shrunk by the LDS loop, a partly filled last workgroup -- and the counter
    words and action counts the suite never ran.
(b) SCENES: hand-made states whose answer is written down here, derived from uav.py:324-369 line by line.

The rule, restated (uav.py:341-368; find_closest_a_idx as include/uavtrack.h defines it):
    score_k = 1 / d(u, t_k) - 0.8 * #{other UAVs j, compared BY POSITION (uav.py:351), with d(j, t_k) < dc}   (strict <)
    the first best k wins (`>`, uav.py:358);  angle = atan2(ty - y, tx - x) - h, wrapped to [-pi, pi)
    action = the index a of the turn rate w_a = (2a + 1 - na) * dt * h_max / (na - 1) nearest to the angle, lowest on ties
With the defaults (dt = 1, h_max = pi / 6, na = 12): w_a = (2a - 11) * pi / 66, i.e. (2a - 11) * 0.0475999; an angle beyond
+-pi/6 = +-0.5236 is clipped to a = 11 / a = 0, and angle / 0.0476 is rounded to the nearest ODD integer 2a - 11.
"""
from collections import namedtuple

import numpy as np

CAP = 0.10                       # at most this share of a case's scoring-branch decisions may be set aside
POLICY_SEED = 99

# ---- (a) shape cases ---------------------------------------------------------------------------------------------------
# E below is launch_greedy's: wgs = 256 (N <= 256) or 512, E = wgs // N, then --E while E * (8 N + 12 M) > 65536 bytes.
# steps: random-action steps before the comparison (step_count > 0 enters the Philox counter).  B * N * M * N, the
# oracle's pair evaluations, stays below 2e8 (the largest here: 203 * 3 * 4096 * 3 = 7.5e6).
Shape = namedtuple("Shape", "name N M B box seed na env_offset steps")

# na_max: validate() (csrc/api_env.hip) puts no upper bound of its own on na with nc = 1; the bound a handle meets is
# uavtrack_create's on the specialised shapes of up to 64 UAVs, n_uav^2 * na * nc * 4 < 2^24.  At 50 x 25 that is
# na <= 1677 (2500 * 1677 * 4 = 16 770 000 < 16 777 216 <= 2500 * 1678 * 4).  The turn rates are then pi / (6 * 1676) =
# 3.1e-4 apart in halves, three times the angle tolerance, so steering decisions can still be compared.  (At 20 x 10 the
# bound is 10 485 and the half spacing 5e-5 lies below the tolerance: no steering decision inside +-pi/6 would count.)
NA_MAX_50x25 = (1 << 24) // (50 * 50 * 4) - (1 if (1 << 24) % (50 * 50 * 4) == 0 else 0)

SHAPES = [
    Shape("n1", 1, 7, 300, 2000.0, 13, 12, 77, 2),                       # E = 256: one lane per environment
    Shape("m1", 9, 1, 200, 2000.0, 14, 12, 77, 2),                       # E = 28, 200 % 28 != 0
    Shape("dense_20x10", 20, 10, 131, 600.0, 15, 12, 77, 3),             # E = 12, 131 % 12 != 0; penalties decide
    Shape("n256", 256, 12, 5, 2000.0, 16, 12, 77, 1),                    # the last shape of the 256-thread path, E = 1
    Shape("n257", 257, 6, 3, 2000.0, 17, 12, 77, 1),                     # the first of the 512-thread path, E = 1
    Shape("n512", 512, 3, 3, 2000.0, 18, 12, 77, 1),                     # every lane of the largest workgroup
    Shape("n3_m4096", 3, 4096, 203, 2000.0, 19, 12, 77, 1),              # E shrunk from 85 to 1 (49 176 B of LDS)
    # (box: in the 2000 m box half of the 1000 targets are free of every UAV and ~1 km away, their scores 1/d a few 1e-6
    #  apart: 23 % of the decisions have no clear winner.  In 600 m the counts run 14..19 and the nearest of many decides.)
    Shape("n20_m1000", 20, 1000, 13, 600.0, 20, 12, 77, 1),              # E shrunk from 12 to 5, 13 % 5 != 0
    Shape("na2", 7, 4, 99, 1200.0, 21, 2, 77, 2),
    Shape("na3", 7, 4, 99, 1200.0, 22, 3, 77, 2),
    Shape("na9", 7, 4, 99, 1200.0, 23, 9, 77, 2),
    Shape("na12", 7, 4, 99, 1200.0, 24, 12, 77, 2),
    # (box: 2000 m leaves 10 % of the decisions without a clear winner, on top of the third of the steering angles
    #  inside +-pi/6 that lie within the angle tolerance of a boundary at this na; 1000 m leaves 2 %.)
    Shape("na_max", 50, 25, 37, 1000.0, 25, NA_MAX_50x25, 77, 2),
    Shape("offset_2p32", 5, 3, 200, 2000.0, 26, 12, 2 ** 32 + 77, 2),    # the high word of the environment index
]
SHAPE_IDS = [s.name for s in SHAPES]


def greedy_E(N, M):
    """launch_greedy's workgroup size and environments per workgroup, restated from csrc/policy_kernel.hip."""
    wgs = 256 if N <= 256 else 512
    E = wgs // N
    while E > 1 and E * (N * 8 + M * 12) > 64 * 1024:
        E -= 1
    return wgs, E


def shape_config(s):
    """Keyword arguments shared by EnvConfig and OracleConfig."""
    return dict(n_envs=s.B, n_uav=s.N, m_targets=s.M, x_max=s.box, y_max=s.box, na=s.na)


def shape_actions(s):
    """The random actions of the steps before the comparison, [steps, B, N] int32."""
    return np.random.RandomState(s.seed).randint(0, s.na, size=(s.steps, s.B, s.N)).astype(np.int32)


def round32(st):
    """A state as the device holds it: every pose rounded to fp32."""
    return {k: (v if v.dtype.kind == "i" else v.astype(np.float32)) for k, v in st.items()}


def oracle_state(s):
    """The oracle's own reset (bit-exact with the device's) and `steps` random-action steps, rounded to fp32 ->
    (OracleEnv holding that state, step_count [B])."""
    from oracle import OracleConfig, OracleEnv
    orc = OracleEnv(OracleConfig(**shape_config(s)))
    orc.reset_philox(seed=s.seed, env_offset=s.env_offset)
    for act in shape_actions(s):
        orc.step(act)
    st = round32(orc.get_state())
    orc.set_state(st["ux"], st["uy"], st["uh"], st["ua"], st["tx"], st["ty"], st["th"])
    return orc, np.full(s.B, s.steps, np.int32)


def set_aside(aids):
    """(scoring-branch decisions not robust, scoring-branch decisions) of one oracle call."""
    scoring = aids["branch"] == 2
    return int((scoring & ~aids["robust"]).sum()), int(scoring.sum())


# ---- (b) constructed scenes --------------------------------------------------------------------------------------------
# One environment each; `want[i]` is UAV i's action whenever its draws put it on the scoring branch (None: no hand-made
# answer, the oracle's is taken).  Coordinates are small integers, so every distance test below is exact in fp32 and fp64.
Scene = namedtuple("Scene", "name na uav targets want")          # uav: [(x, y, h)], targets: [(x, y)]
TU = np.pi / 66.0                                                # the default turn-rate half spacing, 0.0475999

SCENES = [
    # Two targets mirror-imaged about the UAV: dy = +-300, dx = 0, d^2 = 90000 bitwise equal, nobody else about -> equal
    # scores, `score > best` keeps the FIRST (uav.py:358).  T0 north: atan2(300, 0) = pi/2 > pi/6 -> clipped to a = 11.
    Scene("mirror_first_north", 12, [(1000, 1000, 0.0)], [(1000, 1300), (1000, 700)], [11]),
    # ... and in the other index order the first is the southern one: -pi/2 -> a = 0.
    Scene("mirror_first_south", 12, [(1000, 1000, 0.0)], [(1000, 700), (1000, 1300)], [0]),
    # Two targets ON the UAV: d = 0, 1/d = +inf for both (the reference would divide by zero; defined here as +inf), the
    # first wins, atan2(0, 0) = 0, angle = -h = -0.2: -0.2 / 0.0476 = -4.20 -> nearest odd -5 -> a = 3.  (+h would give 8;
    # the decoy 1 m to the north scores 1.0 and would give 11.)
    Scene("on_target_twice", 12, [(640, 480, 0.2)], [(640, 481), (640, 480), (640, 480)], [3]),
    # d == dc exactly is NOT inside (strict <, uav.py:353).  UAV 0 (1000, 550): T0 (1000, 1000) is 450 m north, 1/450 =
    # 0.00222; T1 (1000, 40) is 510 m south, 0.00196.  UAV 1 (1500, 1000) is exactly 500 m from T0 (and 1082 m from T1) -> no
    # penalty -> T0 wins -> pi/2 -> a = 11 (with <= it would count: T0 drops to -0.798 and a = 0).  UAV 1 itself, h = -2: T0
    # at 500 m with UAV 0 inside dc of it (450 m): 0.002 - 0.8; T1 at 1082 m, UAV 0 510 m from it: 0.00092 wins;
    # atan2(-960, -500) = -2.0510, minus h = -0.0510; / 0.0476 = -1.07 -> odd -1 -> a = 5.
    Scene("exactly_dc", 12, [(1000, 550, 0.0), (1500, 1000, -2.0)], [(1000, 1000), (1000, 40)], [11, 5]),
    # A near target with k = 2 other UAVs inside dc loses to a farther one with 1.  UAV 0 (1000, 1000): T0 100 m north,
    # T1 800 m south.  UAVs 1, 2 at (1300, 1400), (700, 1400): 424 m from T0, > 1200 m from T1.  UAV 3 (1300, 0): 361 m from
    # T1, 1140 m from T0.  T0: 0.01 - 1.6 = -1.59; T1: 0.00125 - 0.8 = -0.79875 -> T1, -pi/2 -> a = 0.
    Scene("crowded_near_loses", 12, [(1000, 1000, 0.0), (1300, 1400, 0.0), (700, 1400, 0.0), (1300, 0, 0.0)],
          [(1000, 1100), (1000, 200)], [0, None, None, None]),
    # ... and with one UAV fewer near T0 (UAV 2 moved to (700, 1900): 854 m from T0) it is 0.01 - 0.8 = -0.79 against
    # -0.79875: the near target wins by 0.00875 -> pi/2 -> a = 11.  (UAV 0 is itself within dc of T0: it is in the count of
    # UAVs near T0 and must be taken out again; if it were not, T0 would stand at -1.59 and lose.)
    Scene("crowded_near_wins", 12, [(1000, 1000, 0.0), (1300, 1400, 0.0), (700, 1900, 0.0), (1300, 0, 0.0)],
          [(1000, 1100), (1000, 200)], [11, None, None, None]),
    # UAVs 0, 1, 2 share one position: they do not count each other (position compare, uav.py:351).  T0 300 m north, the
    # three are INSIDE dc of it: 3 near it, all at my position -> 0 others -> 0.00333.  T1 (1000, 400) 600 m south, the three
    # are OUTSIDE dc of it, UAV 3 (1000, 100) 300 m from it -> 1 other -> 0.00167 - 0.8.  T0 wins -> a = 11 for all three.
    # (Not taking the coincident ones out of T0's count: -1.6 or -2.4 -> T1 -> a = 0.  Taking them out of T1's count although
    #  I am outside dc of T1: 0.00167 + 1.6 -> T1 -> a = 0.)  UAV 3: T1 at 300 m free (0.00333), T0 at 1200 m with 3 (-2.4)
    # -> T1 due north -> a = 11.
    Scene("coincident_inside_and_outside", 12, [(1000, 1000, 0.0), (1000, 1000, 0.0), (1000, 1000, 0.0), (1000, 100, 0.0)],
          [(1000, 1300), (1000, 400)], [11, 11, 11, 11]),
    # A target dead astern, h = 0: atan2(0, -600) = pi, and [-pi, pi) has no pi: it wraps to -pi -> clipped to a = 0
    # (unwrapped it would be a = 11).
    Scene("dead_astern", 12, [(1000, 1000, 0.0)], [(400, 1000)], [0]),
    # A target dead ahead, h = 0: the angle is exactly 0.  Even na: 0 lies midway between the two middle turn rates -+tu, a
    # tie, the LOWER index na/2 - 1 wins.  Odd na: the middle turn rate is exactly 0, index (na - 1) / 2.
    Scene("dead_ahead_na12", 12, [(1000, 1000, 0.0)], [(1500, 1000)], [5]),
    Scene("dead_ahead_na2", 2, [(1000, 1000, 0.0)], [(1500, 1000)], [0]),
    Scene("dead_ahead_na9", 9, [(1000, 1000, 0.0)], [(1500, 1000)], [4]),
    Scene("dead_ahead_na3", 3, [(1000, 1000, 0.0)], [(1500, 1000)], [1]),
    # Headings near +-pi: angle - h leaves [-pi, pi) and needs the wrap.  Target at (-700, +100) from the UAV:
    # atan2(100, -700) = pi - atan(1/7) = 2.99970; h = -3.1: 6.09970 - 2 pi = -0.18349; / 0.0476 = -3.85 -> odd -3 -> a = 4
    # (unwrapped: clipped to 11).
    Scene("heading_minus_pi", 12, [(1000, 1000, -3.1)], [(300, 1100)], [4]),
    # ... mirrored: atan2(-100, -700) = -2.99970, h = +3.1: -6.09970 + 2 pi = +0.18349 -> odd +3 -> a = 7 (unwrapped: 0).
    Scene("heading_plus_pi", 12, [(1000, 1000, 3.1)], [(300, 900)], [7]),
    # ... and a heading of almost pi with the target dead astern of east: pi - 3.1 = 0.04159; / 0.0476 = 0.87 -> odd 1 -> a = 6.
    Scene("heading_3p1_target_west", 12, [(1000, 1000, 3.1)], [(400, 1000)], [6]),
]
SCENE_IDS = [s.name for s in SCENES]

# One pair a hair outside dc (UAV 1 is 500.005 m from T0, inside the 1e-2 tolerance): the old per-environment margin drops
# all three UAVs, the per-UAV verdict only UAV 0.  UAV 0 (1000, 700): T0 300 m north is 0.00333 if UAV 1 is outside dc of
# it, -0.79667 if inside; T1 (1000, 300) 400 m south is 0.0025 -> the pair decides -> NOT robust.  UAV 1 (h = 1): the pair
# is its own distance, not a penalty test of its own; T0 -0.798 (UAV 0 at 300 m), T1 (860 m, UAV 0 at 400 m) -0.79884, T2
# (1527 m, UAV 2 at 1 m) -0.79935: T0 wins by 8e-4, pi - 1 -> a = 11, robust.  UAV 2 (200, 1800): T2 1 m north scores 1.0,
# nothing comes near -> robust.
NEAR_DC = Scene("near_dc_pair", 12, [(1000, 700, 0.0), (1500.005, 1000, 1.0), (200, 1800, 0.0)],
                [(1000, 1000), (1000, 300), (200, 1801)], [11, 11, 11])
NEAR_DC_ROBUST = [False, True, True]


def scene_config(sc, B=1):
    return dict(n_envs=B, n_uav=len(sc.uav), m_targets=len(sc.targets), na=sc.na)


def scene_state(sc, B=1):
    """The scene in every one of B environments (their draws differ), fp32."""
    u = np.asarray(sc.uav, np.float64)
    t = np.asarray(sc.targets, np.float64)
    rep = lambda v, dt=np.float32: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (B, len(v))))
    return dict(ux=rep(u[:, 0]), uy=rep(u[:, 1]), uh=rep(u[:, 2]), ua=rep(np.zeros(len(u)), np.int32),
                tx=rep(t[:, 0]), ty=rep(t[:, 1]), th=rep(np.zeros(len(t))))


def scene_want(sc, oracle_actions):
    """[B, N] expected actions on the scoring branch: the hand-written answer, the oracle's where there is none."""
    want = np.array(oracle_actions, np.int32, copy=True)
    for i, w in enumerate(sc.want):
        if w is not None:
            want[:, i] = w
    return want
