"""CPU side of the rollout variant census (tests/variant_census.py): the table against the symbols of the built library,
and the x-z-plane restriction of the 3-D model against the 2-D model on the fp64 oracle alone."""
import re
import shutil
import subprocess

import numpy as np

import variant_census as vc
from oracle import OracleConfig, OracleEnv
from uavtrack import _lib

_SYMBOL = re.compile(r"rollout_kernel<([^<>]*)>")


def instantiated_variants(lib_path):
    """The template tuples of every rollout_kernel instantiation in the library, from its demangled symbol table."""
    nm = shutil.which("nm")
    assert nm, "binutils' nm was not found: the census cannot be checked for completeness (this check does not skip)"
    out = subprocess.run([nm, "-C", lib_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr
    found = set()
    for args in _SYMBOL.findall(out.stdout):
        fields = [a.strip() for a in args.split(",")]
        assert len(fields) == 8, f"rollout_kernel<{args}>: the template no longer has 8 arguments -- the census must follow"
        found.add(tuple({"true": 1, "false": 0}[f] if f in ("true", "false") else int(f) for f in fields))
    return found


def test_census_table_equals_the_instantiated_variants():
    """Set equality, both ways: a rollout_kernel instantiation that the table lacks is a kernel no census case runs; a table
    entry that is not instantiated is a case that cannot reach its kernel.  A shape added to kSpecShapes, or a family added
    to pick_policy, fails here until tests/variant_census.py follows."""
    built = instantiated_variants(_lib.LIB_PATH)
    assert built, "no rollout_kernel symbol in the library: stripped, or the symbol pattern no longer matches"
    table = set(vc.TABLE)
    print(f"rollout_kernel instantiations: {len(built)} in the library, {len(table)} in the census table, "
          f"{len(vc.cases())} (variant, workgroup size) cases")
    missing, stale = sorted(built - table), sorted(table - built)
    assert not missing and not stale, (f"{len(missing)} instantiated variants are missing from the census table: {missing[:6]} ...; "
                                       f"{len(stale)} table entries are not instantiated: {stale[:6]} ...")


def test_census_recipes_are_well_formed():
    """What the GPU census relies on: every extra is exercised in both dims, LONE entries run at the library's own
    geometry only, every non-LONE entry has at least one workgroup size, and the batch leaves the last workgroup partly
    filled (it is prime and above 1, so it is a multiple of no environments-per-workgroup count but 1 and itself)."""
    for dim in (2, 3):
        assert {e.extra for e in vc.CENSUS if e.key[6] and e.dim == dim} == set(vc.GIVEN_EXTRAS)
    for e in vc.CENSUS:
        assert e.key[6] == (e.extra is not None), e
        if e.key[7]:
            assert e.own and not e.sizes and e.dim == 2 and not e.key[6], e
        else:
            assert e.sizes, e
        assert 3 <= e.B <= 64 and all(e.B % d for d in range(2, e.B)), e
        if e.key[4] == vc.GREEDY:
            assert e.mode != vc.PMI and e.dim == 2, e
    assert all(w == 0 or w in e.sizes for e, w in vc.cases())


# ---- the x-z-plane restriction -------------------------------------------------------------------------------------------
# Columns of the 12-d observation that the restriction makes equal, and those it cannot (see the test's docstring)
XZ_OBS_EQUAL = (0, 2, 3, 4, 5, 7, 8, 9, 11)
XZ_OBS_DIFFER = (1, 6, 10)
XZ_Y_MAX_3D, XZ_Y0 = 2000.0, 1000.0
XZ_ATOL = 1e-7


def xz_configs(N, M, B, cooperative):
    """(3-D keywords, 2-D keywords): zero turn rate is action 4 of na = 9, level flight is nc = 1, the targets stand still;
    the 2-D box's y_max is the 3-D box's z_max."""
    base = dict(n_envs=B, n_uav=N, m_targets=M, cooperative=cooperative, na=9, x_max=600.0, dp=150.0, dc=400.0, dt=0.8,
                u_v_max=25.0, t_v_max=0.0, alpha=0.5, beta=0.3, gamma=0.2)
    return dict(base, dim=3, nc=1, y_max=XZ_Y_MAX_3D, z_max=400.0), dict(base, dim=2, y_max=400.0)


def xz_scene(N, M, B, seed):
    """-> (3-D state, its image under (x, z) -> (x, y)): x at least 5 m inside the walls, every y equal and far from the
    y walls, z over the whole band, headings 0 or pi, fp32."""
    r = np.random.RandomState(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    ux, tx = f32(r.uniform(5.0, 595.0, (B, N))), f32(r.uniform(5.0, 595.0, (B, M)))
    uz, tz = f32(r.uniform(0.0, 400.0, (B, N))), f32(r.uniform(0.0, 400.0, (B, M)))
    uh = f32(np.pi) * r.randint(0, 2, (B, N)).astype(np.float32)
    th = f32(r.uniform(-np.pi, np.pi, (B, M)))
    ua = np.full((B, N), 4, np.int32)
    s3 = dict(ux=ux, uy=np.full_like(ux, XZ_Y0), uz=uz, uh=uh, ua=ua, tx=tx, ty=np.full_like(tx, XZ_Y0), tz=tz, th=th)
    s2 = dict(ux=ux, uy=uz, uh=uh, ua=ua, tx=tx, ty=tz, th=th)
    return s3, s2


def xz_separates(s3, dp):
    """UAV-target pairs within dp in x alone but outside it in (x, z): a kernel that dropped the altitude term would see
    them in range."""
    dx = s3["ux"][:, :, None].astype(np.float64) - s3["tx"][:, None, :]
    dz = s3["uz"][:, :, None].astype(np.float64) - s3["tz"][:, None, :]
    return int(((np.abs(dx) <= dp) & (np.hypot(dx, dz) > dp)).sum())


def test_oracle_3d_restricted_to_the_xz_plane_equals_2d():
    """The 3-D model (our own spec, DESIGN.md 4.4: the reference has no 3-D code) against the reference-pinned 2-D model,
    both on the fp64 oracle: UAVs flying along x (headings 0 or pi, zero turn rate) at one y with their altitudes spread
    over the band, standing targets, mapped (x, z) -> (x, y) into a 2-D box whose y_max is the 3-D z_max.  Unlike the
    equal-altitude restriction, dz is busy here: every range is sqrt(dx^2 + 0 + dz^2).

    EQUAL under the mapping (asserted to XZ_ATOL = 1e-7: a heading of fp32 pi has sin = -8.7e-8, which moves the UAV by
    1.7e-6 m a step along y -- out of the plane in 3-D, along the image of z in 2-D -- that is 1.2e-8 of dp):
      the tracking and duplicate terms, the coverage count, the neighbour sets and with them the MAAC-G mix -- all are
      functions of 3-D distances, which the mapping preserves; the boundary term, because the spec ADDS the z walls to
      the x and y walls (min over all six) and the common y sits 1000 m from the y walls of a 2000 m box, so the y walls
      never bind and min(x walls, z walls) is the 2-D box's min(x walls, y walls); hence the raw and the final rewards;
      observation columns 0, 2-4 (peer x offset, heading and action differences), 5, 7, 8 (target x offset and velocity
      differences), 9 (x / dc) and 11 (action): the sets averaged over are equal and the 1 / min(d, 1) weights are 1 in
      both (x >= 5 m keeps the "offset to absolute pose" distance of uav.py:165 above 1).
    NOT EQUAL, by the spec (asserted to differ, so the list stays honest): observation columns 1, 6 and 10 -- the 3-D
      observation keeps the 2-D layout, its y columns carry y, not z: peer and target y offsets are 0 here against the
      2-D image's z offsets, and column 10 is y / dc = 2.5 against z / dc."""
    N, M, B = 20, 10, 48
    for coop in (0.0, 0.3):
        k3, k2 = xz_configs(N, M, B, coop)
        o3, o2 = OracleEnv(OracleConfig(**k3), n_threads=4), OracleEnv(OracleConfig(**k2), n_threads=4)
        act = np.full((B, N), 4, np.int32)
        separated = 0
        for t in range(3):
            s3, s2 = xz_scene(N, M, B, 100 + t)
            separated += xz_separates(s3, k3["dp"])
            o3.set_state(**s3); o2.set_state(**s2)
            r3, r2 = o3.step(act), o2.step(act)
            np.testing.assert_allclose(r3["terms"], r2["terms"], rtol=0, atol=XZ_ATOL)
            np.testing.assert_allclose(r3["raw"], r2["raw"], rtol=0, atol=XZ_ATOL)
            np.testing.assert_allclose(r3["reward"], r2["reward"], rtol=0, atol=XZ_ATOL)
            np.testing.assert_array_equal(r3["covered"], r2["covered"])
            np.testing.assert_allclose(r3["obs"][..., XZ_OBS_EQUAL], r2["obs"][..., XZ_OBS_EQUAL], rtol=0, atol=XZ_ATOL)
            for c in XZ_OBS_DIFFER:
                assert np.abs(r3["obs"][..., c] - r2["obs"][..., c]).max() > 1e-2, c
            assert np.abs(r3["terms"]).max(axis=(1, 2)).min() > 0.05      # every term is busy, the boundary term included
            g3, g2 = o3.get_state(), o2.get_state()
            np.testing.assert_allclose(g3["ux"], g2["ux"], rtol=0, atol=XZ_ATOL)
            np.testing.assert_array_equal(g3["uz"], s3["uz"].astype(np.float64))      # level flight
            assert np.abs(g3["uy"] - XZ_Y0).max() < 1e-5
        assert separated > 100, separated
        if coop:
            assert np.abs(r3["reward"] - r3["raw"]).max() > 1e-3      # the neighbour mix really mixed
