"""The census of rollout kernel variants: every `rollout_kernel<N_, M_, MODE, Z3, POLICY, ALLOUT, EXTRAS, LONE>` the
dispatch of csrc/step_kernel.hip can produce, each with the recipe that reaches it through the public API.

A plain helper (no tests here).  The table is written from the dispatch rules -- `kSpecShapes`, `pick_policy`, `pick_dim`,
`pick_reward`, `select_rollout` -- as they read in the source, NOT by calling the library:
  * shapes: the specialised (N, M) of kSpecShapes, each with or without single-wavefront (LONE) variants, then the
    generic kernel (0, 0), which has none;
  * pick_policy: on a LONE shape, the two LONE families (planar, no extras: the actor; the caller's actions with every
    output); the planar greedy baseline with / without extras; the actor with / without extras in both dims; the caller's
    actions with extras, with every output, or with neither, in both dims;
  * pick_reward: every family in the three reward modes, except that the greedy baseline's PMI slot is the RAW kernel
    (uavtrack_run_greedy refuses MAAC-R), so greedy has two.
tests/test_variant_census_cpu.py holds this table against the symbols of the built library (set equality);
tests/test_hip_variant_census.py runs every entry against the fp64 oracle.
"""
from collections import namedtuple

RAW, MEAN, PMI = 0, 1, 2                  # UAVTRACK_REWARD_* (include/uavtrack.h), uavtrack.RewardMode
GIVEN, GREEDY, ACTOR = 0, 1, 2            # kPolicy* (csrc/env.h)
MODE_NAMES = {RAW: "raw", MEAN: "mean", PMI: "pmi"}
POLICY_NAMES = {GIVEN: "given", GREEDY: "greedy", ACTOR: "actor"}

# kSpecShapes (csrc/step_kernel.hip): (N, M, has LONE variants).  A shape added there must be added here.
SPEC_SHAPES = [(20, 10, True), (50, 25, False), (10, 10, True), (5, 3, True)]
GENERIC_SHAPE = (7, 4)                    # what the generic kernel's entries run on (any shape not in kSpecShapes would do)
LONE_ACTOR_HIDDEN = 128                   # kLoneActorTiles = 4 tiles of 32: the one width the LONE actor rollout is laid out for
OTHER_ACTOR_HIDDEN = 40                   # another width: the non-LONE actor entry on the same geometry
PMI_LONG_T = 16                           # kPmiShortLaunch: MAAC-R launches of at least this many steps take the LONE variant
FORCED_SIZES = (64, 128, 256, 512)        # UAVTRACK_WGS values plan_geometry knows

# One table entry.  key: the template tuple (N_, M_, MODE, Z3, POLICY, ALLOUT, EXTRAS, LONE).  The recipe:
#   N, M        the shape the entry runs on            mode   the configuration's reward mode      dim  2 | 3
#   entry       "step" | "step_many" | "run_greedy" | "run_actor" | "step_host"
#   flags       keyword arguments of that entry point that select the variant (a want_* flag off, want_targets, ...)
#   extra       None | "targets" | "raw" | "auto_reset" | "state_copy": the extra whose own output the case checks
#   hidden      actor width (run_actor)                T      steps per launch
#   B           batch (prime: never a multiple of the environments per workgroup, so the last workgroup is partly filled)
#   own         True: the library's own geometry reaches the entry at this batch (False: only a forced workgroup size
#               does -- with B <= 64 the library's own choice for these launches is their LONE sibling, an entry of its own)
#   sizes       forced workgroup sizes plan_geometry accepts for the shape; infeasible: those it ignores
Entry = namedtuple("Entry", "key N M mode dim entry flags extra hidden T B own sizes infeasible")

CENSUS_B = 37
GIVEN_EXTRAS = ("targets", "raw", "auto_reset", "state_copy")


def feasible_sizes(N):
    """plan_geometry's rule for a forced size at the census shapes: at least one whole environment per workgroup (the
    LDS of a single environment of these shapes is far below the limit)."""
    ok = tuple(w for w in FORCED_SIZES if w // N >= 1)
    return ok, tuple(w for w in FORCED_SIZES if w not in ok)


def _entries():
    out = []
    shapes = [(n, m, lone, n, m) for n, m, lone in SPEC_SHAPES] + [(0, 0, False) + GENERIC_SHAPE]
    for si, (n_, m_, lone_shape, N, M) in enumerate(shapes):
        sizes, infeasible = feasible_sizes(N)

        def add(mode, z3, policy, allout, extras, lone, entry, flags=None, extra=None, hidden=0, T=1, own=True):
            out.append(Entry((n_, m_, mode, int(z3), policy, int(allout), int(extras), int(lone)), N, M, mode,
                             3 if z3 else 2, entry, dict(flags or {}), extra, hidden, T, CENSUS_B, own,
                             () if lone else sizes, () if lone else infeasible))

        for mi, mode in enumerate((RAW, MEAN, PMI)):
            long_t = PMI_LONG_T if mode == PMI else 1
            if lone_shape:
                # the LONE variants: planar, no extras; the 128-wide actor, or the caller's actions with every output
                add(mode, False, ACTOR, False, False, True, "run_actor", hidden=LONE_ACTOR_HIDDEN, T=long_t)
                add(mode, False, GIVEN, True, False, True, "step_many" if mode == PMI else "step", T=long_t)
            if mode != PMI:      # (pick_reward: greedy's PMI slot is the RAW kernel again)
                add(mode, False, GREEDY, False, False, False, "run_greedy")
                add(mode, False, GREEDY, False, True, False, "run_greedy", dict(want_targets=True), "targets")
            for z3 in (False, True):
                add(mode, z3, ACTOR, False, False, False, "run_actor", hidden=OTHER_ACTOR_HIDDEN)
                add(mode, z3, ACTOR, False, True, False, "run_actor", dict(want_targets=True), "targets", hidden=OTHER_ACTOR_HIDDEN)
                extra = GIVEN_EXTRAS[(si + mi + int(z3)) % 4]
                if extra == "state_copy":
                    add(mode, z3, GIVEN, False, True, False, "step_host", extra=extra)
                else:
                    flag = {"targets": dict(want_targets=True), "raw": dict(want_raw=True),
                            "auto_reset": dict(auto_reset_seed=99)}[extra]
                    add(mode, z3, GIVEN, False, True, False, "step_many", flag, extra)
                # every output, no extras: on a LONE shape's planar RAW / MEAN launches the library's own geometry at this
                # batch is the LONE sibling above (MAAC-R's single steps take geo_short, which is never LONE)
                add(mode, z3, GIVEN, True, False, False, "step", own=not (lone_shape and not z3 and mode != PMI))
                add(mode, z3, GIVEN, False, False, False, "step_many", dict(want_terms=False))
    return out


CENSUS = _entries()
TABLE = {e.key: e for e in CENSUS}
assert len(TABLE) == len(CENSUS), "two census entries with one template tuple"


def cases():
    """The (entry, forced workgroup size) cases of the GPU census; size 0 is the library's own geometry.  LONE entries
    exist only there (a forced size switches the LONE variant off, plan_geometry)."""
    out = []
    for e in CENSUS:
        if e.own:
            out.append((e, 0))
        out.extend((e, w) for w in e.sizes)
    return out


def case_id(e, wgs):
    k = e.key
    return (f"{k[0]}x{k[1]}-{MODE_NAMES[k[2]]}-{'3d' if k[3] else '2d'}-{POLICY_NAMES[k[4]]}"
            f"{'-allout' if k[5] else ''}{'-extras' if k[6] else ''}{'-lone' if k[7] else ''}-wgs{wgs or 'own'}")


def family(e):
    """The shape family knife-edge counts are summed over: (N, M, dim)."""
    return (e.N, e.M, e.dim)


# ---- the census scene (non-default constants: fold_constants derives its scales and thresholds from these) ----------
SCENE = dict(x_max=600.0, y_max=500.0, dp=150.0, dc=400.0, dt=0.8, u_v_max=25.0, t_v_max=6.0, alpha=0.5, beta=0.3, gamma=0.2)
SCENE_3D = dict(z_max=400.0, nc=3)


def scene_config(e, **over):
    """Keyword arguments shared by EnvConfig and OracleConfig for a table entry on the census scene."""
    kw = dict(n_envs=e.B, n_uav=e.N, m_targets=e.M, dim=e.dim, cooperative=0.0 if e.mode == RAW else 0.3, **SCENE)
    if e.dim == 3:
        kw.update(SCENE_3D)
    kw.update(over)
    return kw


def scene_state(kw, seed):
    """The census scene's state: swarm and targets uniform over the box (3-D: over the whole altitude band), headings
    uniform, rounded to fp32."""
    import numpy as np
    r = np.random.RandomState(seed)
    B, N, M = kw["n_envs"], kw["n_uav"], kw["m_targets"]
    f = lambda hi, n, lo=0.0: r.uniform(lo, hi, size=(B, n)).astype(np.float32)
    st = dict(ux=f(kw["x_max"], N), uy=f(kw["y_max"], N), uh=f(np.pi, N, -np.pi),
              ua=r.randint(0, kw.get("na", 12) * kw.get("nc", 1), size=(B, N)).astype(np.int32),
              tx=f(kw["x_max"], M), ty=f(kw["y_max"], M), th=f(np.pi, M, -np.pi))
    if kw.get("dim", 2) == 3:
        st["uz"], st["tz"] = f(kw["z_max"], N), f(kw["z_max"], M)
    return st
