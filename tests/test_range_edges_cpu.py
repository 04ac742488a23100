"""The range-edge scenes (tests/range_edge_scenes.py) on the CPU: their premises, the fp64 oracle against the reference's
recordings of them (g10), and what the two sides of every knife edge change in the oracle's outputs.

tests/test_hip_range_edges.py compares the kernels with the oracle on these scenes WITHOUT a margin filter; that is only
sound if (1) the scenes are what they claim -- every coordinate an fp32 number, one pair on its threshold, nothing else
near one: test_premises_of_every_gpu_scene; (2) the oracle is the reference at every constants set:
test_oracle_reproduces_g10; (3) every scene decides something -- a scene whose two sides give the same oracle output
would pass on any kernel: test_sides_differ_in_exactly_the_designated_outputs.
"""
import numpy as np
import pytest

import range_edge_scenes as res
from conftest import load_golden
from test_oracle_golden import check_episode

SAME = 1e-6        # the sides move one coordinate by an ulp or two: outputs that do not hang on the test move by ~1e-7
DIFFERENT = 1e-3

_BATCHES = res.gpu_batches()


def test_oracle_reproduces_g10(pmi_state_dict_h64):
    """g10 was recorded from the unmodified reference on the builder's 2-D scenes (oracle/gen_golden.py,
    gen_ulp_edges_constants): the oracle must reproduce it at test_oracle_golden's g9 tolerances, at every constants set,
    and the scenes built here must be the recorded ones (same names, same state, same actions)."""
    z, meta = load_golden("g10_ulp_edges_constants")
    groups = res.g10_groups()
    assert [c["name"] for c in meta["cases"]] == [g[0] for g in groups]
    assert {c["constants"] for c in meta["cases"]} == set(res.CONSTANTS)
    assert {c["constants"] for c in meta["cases"] if c["pmi"]} == set(res.B_SETS)
    for case, (name, cs, N, M, use_pmi) in zip(meta["cases"], groups):
        scenes = res.all_scenes(cs, N, M, 2, moves=1)
        assert [s.name for s in scenes] == case["scenes"], name
        pre = name + "__"
        assert int(z[pre + "overstep_prints"].sum()) == 0
        st, acts = res.batch(scenes)
        for k in ("ux", "uy", "uh", "ua", "tx", "ty", "th"):
            np.testing.assert_array_equal(z[pre + k][:, 0], res.exact_state(scenes, 0)[k], err_msg=f"{name} {k}")
        np.testing.assert_array_equal(z[pre + "actions"][:, 0], acts[0], err_msg=name)
        kw = res.config(cs, N, M, 2, 1, 1, cooperative=0.3)
        u = case["cfg"]["uav"]
        assert (u["dp"], u["dc"], u["v_max"], case["cfg"]["target"]["v_max"]) == (kw["dp"], kw["dc"], kw["u_v_max"], kw["t_v_max"])
        for e in range(len(scenes)):
            check_episode(z, pre, e, case, pmi_state_dict_h64, 1)
        # the recordings themselves show the decisions: per (threshold, role) the three sides
        ref = dict(obs=z[pre + "obs"][:, 0], terms=z[pre + "terms"][:, 0], raw=z[pre + "raw"][:, 0],
                   reward=z[pre + "reward"][:, 0], covered=z[pre + "covered"][:, 0])
        if not use_pmi:
            _check_sides(scenes, ref, name)


def test_constants_sets_are_exact_in_fp32():
    assert len(res.CONSTANTS) == 10
    for cs in res.CONSTANTS:
        c = res.constants(cs)          # asserts dp, dc, 2 dp and their squares
        for th in res.THRESHOLDS:
            K = res.threshold_k(c, th)
            lo, hi = res.k_side(K, "inside"), res.k_side(K, "outside")
            k32 = np.float32(K) * np.float32(K)
            # the arithmetic premise: d2 = fl32(dx * dx) is below, on, above K^2
            assert np.float32(lo) * np.float32(lo) < k32 < np.float32(hi) * np.float32(hi), (cs, th)
            assert lo < K < hi and res.k_side(K, "on") == K


@pytest.mark.parametrize("b", _BATCHES, ids=[res.batch_id(b) for b in _BATCHES])
def test_premises_of_every_gpu_scene(b):
    """Building a scene asserts its premises (range_edge_scenes.check).  The only scenes without an fp32 placement: dc = 12
    with two moves of 20 m (a coordinate one ulp(12) = 2^-20 off cannot survive 40 m of travel)."""
    scenes, skipped = res.batch_scenes(b)
    assert len(scenes) >= (24 if b.near0 else 36), (b, len(scenes))
    if b.cs == "dc-below-step" and b.moves == 2:
        assert skipped and all(s[4] == "dc_peer" for s in skipped), skipped
    else:
        assert not skipped, skipped
    # every threshold, side (and 3-D family) is there, the batch has one configuration, names are unique
    assert {(s.threshold, s.side, s.family) for s in scenes} >= {
        (th, sd, f) for th in ("dp_target", "dc_peer", "2dp_dup", "dp_nb") for sd in res.SIDES
        for f in (("x", "z") if b.dim == 3 else ("x",))
        if not (skipped and th == "dc_peer")}
    assert len({s.name for s in scenes}) == len(scenes)
    assert all(s.box == scenes[0].box for s in scenes)
    if b.near0:
        assert all(s.role.near0 for s in scenes)


def test_the_strict_forms_smallest_value_has_its_scene():
    """Where dp^2 is a power of two the batches hold the `below` side: the kernels' d2 one (halved) spacing below dp^2."""
    assert [cs for cs in res.CONSTANTS if res.has_below(cs)] == ["pow2", "huge"]
    for b in _BATCHES:
        scenes, _ = res.batch_scenes(b)
        n = sum(s.side == res.BELOW for s in scenes)
        assert (n >= 2) == res.has_below(b.cs) and (n == 0) != res.has_below(b.cs), (b, n)


def test_roles_reach_the_indexing_cases():
    """The roles of the issue: probe even / odd, partner below / above the probe, slot .x / .y, the padded pair of an odd
    N, a pair index >= 32, target even / odd, the padded target pair, the second coverage word."""
    ij = lambda N, M, th: {(x.i, x.j) for x in res.roles(N, M, th)}      # noqa: E731
    r = ij(20, 10, "dc_peer")
    assert any(i % 2 == 0 and j < i for i, j in r) and any(i % 2 == 1 and j < i for i, j in r)
    assert any(j > i and j % 2 == 0 for i, j in r) and any(j > i and j % 2 == 1 for i, j in r)
    assert any(j < i and j % 2 == 0 for i, j in r) and any(j < i and j % 2 == 1 for i, j in r)
    assert any(i // 2 == j // 2 for i, j in r) and (0, 10) in r
    assert any(j == 4 for i, j in ij(5, 3, "2dp_dup")) and any(i == 4 for i, j in ij(5, 3, "2dp_dup"))
    assert any(j >= 64 for i, j in ij(70, 5, "dp_nb")) and any(i >= 64 for i, j in ij(70, 5, "dp_nb"))
    t = ij(50, 25, "dp_target")
    assert any(k == 24 for _, k in t) and any(k % 2 for _, k in t) and any(k % 2 == 0 for _, k in t)
    assert any(k == 2 for _, k in ij(5, 3, "dp_target"))
    assert all(x.near0 for x in res.near_origin_roles(20, 10, "dc_peer"))


def _changed(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    assert not np.any((d > SAME) & (d < DIFFERENT)), "an output moved by an amount that is neither rounding nor a decision"
    return d >= DIFFERENT


def _check_sides(scenes, ref, what):
    """Per (threshold, role, family): the three sides' outputs differ in exactly the designated rows and columns.
    ref: obs [S, N, 12], terms [S, 3, N], raw [S, N], reward [S, N], covered [S] of a cooperative (MAAC-G) run."""
    by = {}
    for n, s in enumerate(scenes):
        by.setdefault((s.threshold, s.role.name, s.family), {})[s.side] = (n, s)
    assert by
    for key, sides in by.items():
        assert set(sides) - {res.BELOW} == set(res.SIDES), key
        assert (res.BELOW in sides) == (key[0] == "dp_target" and key[2] == "x" and res.has_below(scenes[0].cs)), key
        if res.BELOW in sides:          # the last fp32 d2 below dp^2: observed, tracked AND covered, as `inside`
            nb, sb = sides[res.BELOW]
            assert int(ref["covered"][nb]) == 1 and ref["terms"][nb][0, sb.probe] > 0 and ref["obs"][nb][sb.probe, 6] != -1.0, sb.name
        (ni, sc), (no, _), (nx, _) = sides["inside"], sides["on"], sides["outside"]
        i, j, N = sc.probe, sc.partner, sc.N
        w = f"{what} {sc.name}"
        # inside vs on: only the strict coverage test tells them apart
        for k in ("obs", "terms", "raw", "reward"):
            assert not _changed(ref[k][ni], ref[k][no]).any(), (w, k, "inside vs on")
        if sc.threshold == "dp_target":
            assert int(ref["covered"][ni]) == int(ref["covered"][no]) + 1 == 1, (w, "coverage is strict")
        else:
            assert int(ref["covered"][ni]) == int(ref["covered"][no]), w
        # on vs outside: the inclusive test
        assert int(ref["covered"][no]) == int(ref["covered"][nx]) == 0, w
        obs, terms = _changed(ref["obs"][no], ref["obs"][nx]), _changed(ref["terms"][no], ref["terms"][nx])
        raw, rew = _changed(ref["raw"][no], ref["raw"][nx]), _changed(ref["reward"][no], ref["reward"][nx])
        want_obs, want_terms = np.zeros((N, 12), bool), np.zeros((3, N), bool)
        rows = np.zeros(N, bool)
        rows[list(sc.rows)] = True
        if sc.threshold == "dp_target":
            want_obs[i, 5:9] = True; want_terms[0, i] = True
            assert obs[i, 6] and terms[0, i] and raw[i], w        # dy / dp = 0 against the empty list's -1; the tracking term
            assert ref["terms"][no][0, i] > 0 and ref["terms"][nx][0, i] == 0, w
        elif sc.threshold == "dc_peer":
            want_obs[i, 0:5] = True
            assert obs[i, 1] and not raw.any() and not rew.any(), w
        elif sc.threshold == "2dp_dup":
            want_terms[2, [i, j]] = True
            assert terms[2, i] and terms[2, j] and raw[i] and raw[j], w
            assert ref["terms"][no][2, i] < 0 and ref["terms"][nx][2, i] == 0, w
        else:               # dp_nb: the cooperative reward alone; outside, neither has a neighbour (MAAC-G gives 0)
            assert rew[i] and rew[j] and not raw.any(), w
            assert ref["reward"][nx][i] == 0.0 and ref["reward"][nx][j] == 0.0, w
        assert not (obs & ~want_obs).any(), (w, "obs outside the designated entries", np.argwhere(obs & ~want_obs))
        assert not (terms & ~want_terms).any(), (w, "terms outside the designated entries")
        assert not (raw & ~rows).any() and not (rew & ~rows).any(), (w, "rewards outside the designated rows")


@pytest.mark.parametrize("b", _BATCHES, ids=[res.batch_id(b) for b in _BATCHES])
def test_sides_differ_in_exactly_the_designated_outputs(b):
    """On the oracle (MAAC-G, so that the neighbour test shows): the last move's outputs."""
    scenes, _ = res.batch_scenes(b)
    ref = res.oracle_steps(scenes, 0.3)[-1]
    assert np.all(ref["margin"] <= 2.0 * np.array([s.K for s in scenes]) * 2.0 ** -23), "a scene is not on a knife edge"
    ref = dict(ref, terms=np.moveaxis(ref["terms"], 0, 1))          # [3, S, N] -> [S, 3, N]
    _check_sides(scenes, ref, res.batch_id(b))
