"""The MAAC-R mix mirror (maacr_mix_mirror.py) against the fp64 oracle, and proof that its scenes decide something.  No GPU.

(1) mix_fp64, fed with fp64 scores of the oracle's own observation products, equals OracleEnv.step's reward to 1e-12 on
every scene, every cooperative weight and every rung of the spread ladder.  The oracle rounds every score (uav_oracle.c,
".item() of an fp32 tensor") and every softmax weight ("scipy softmax on fp32") to fp32; the comparison REPRODUCES both
roundings (mix_fp64(round_weights=True) on fp32-rounded scores) instead of allowing their 2^-24.
(2) Every scene keeps its margins (pairs 1 % of dp from dp, UAVs 50 m from the origin, every range test of the oracle away
from its threshold -- 5 mm, twenty times the 0.25 mm an fp32 move can shift a pose by: the GPU tests set nothing aside), shows the graph it was placed for, and the wall scene meets the
clip both ways.
(3) The ladder: c = 0 all scores equal; c = 1 today's regime, in-neighbourhood spread <= 0.25; c = 64 spread in [2, 10];
c = 4096 spread >= 90, past exp's fp32 overflow at 88.7.  Leg A (bound's second term below 1e-3) holds on c = 0 and 1 only.
(4) Swapping two scores of one UAV's run moves its row by more than 100 leg-B bounds on the shape's most telling row, at
every rung but c = 0 (all scores equal: no swap can show): 500 to 5000 bounds at c = 1, 2e4 and more from c = 64 up.
Every single scene that has a run of two or more does so on at least one rung; which one depends on the scene (the cliques'
scores are flat: only the top rung separates them).
(5) The pool scenes reach every branch of the slot pool's bookkeeping at 20x10, 10x10 and 5x3.
"""
import os

import numpy as np
import pytest

import maacr_mix_mirror as mm
from conftest import GOLDEN, PKG, pmi_forward_fp64
from oracle import OracleConfig, OracleEnv, OraclePmi


@pytest.fixture(scope="module")
def sd0():
    z = np.load(os.path.join(GOLDEN, "pmi_h64.npz"))
    return {k: z[k] for k in z.files if k != "meta"}


def oracle_step(N, M, dim, kind, coop, sd, st):
    B = st["ux"].shape[0]
    orc = OracleEnv(OracleConfig(**mm.config_kwargs(N, M, dim, kind, coop, B)), n_threads=4)
    orc.pmi = OraclePmi.from_state_dict(sd)
    orc.set_state(**st)
    ref = orc.step(mm.rigid_actions(1, B, N, dim)[0])
    return ref, orc.get_state()


def best_swap(nbs, raw, sc, coop):
    """max over UAVs i and pairs j1 < j2 of i's run (neighbours above i) of: how far row i moves when s_ij1 and s_ij2 trade
    places, over row i's leg-B bound."""
    bound = mm.leg_b_bound(nbs, raw)
    best = 0.0
    for i, nb in enumerate(nbs):
        run = [int(j) for j in nb if j > i]
        if len(run) < 2:
            continue
        s = np.array([sc[(i, int(j))] for j in nb])
        pos = {int(j): k for k, j in enumerate(nb)}

        def row(scores):
            e = np.exp(scores - scores.max())
            return coop * float((e / e.sum()) @ raw[nb])
        base = row(s)
        order = sorted(run, key=lambda j: s[pos[j]])
        j1, j2 = order[0], order[-1]                 # the two scores of the run that differ most
        t = s.copy()
        t[pos[j1]], t[pos[j2]] = s[pos[j2]], s[pos[j1]]
        best = max(best, abs(row(t) - base) / bound[i])
    return best


@pytest.mark.parametrize("N,M,dim", mm.SHAPES)
def test_mirror_equals_oracle_and_every_scene_decides(sd0, N, M, dim):
    spread = {c: 0.0 for c in mm.RUNGS}
    second = {c: 0.0 for c in mm.RUNGS}
    swap = {c: 0.0 for c in mm.RUNGS}
    scene_swap = {}
    for kind in mm.KINDS:
        names, st, edges = mm.scenes_of(N, M, dim, kind)
        B = len(names)
        ref0, pos = oracle_step(N, M, dim, kind, 0.3, sd0, st)
        assert ref0["margin"].min() >= mm.MIN_ORACLE_MARGIN, (kind, dict(zip(names, ref0["margin"])))
        per_env = []
        for b in range(B):
            poses = mm.poses_of(pos, b, dim)
            nbs = mm.neighbour_sets(poses)
            d = mm.pair_distances(poses)
            assert len(d) == 0 or np.abs(d - mm.DP).min() >= mm.MIN_EDGE_MARGIN, (kind, names[b])
            assert np.hypot(pos["ux"][b], pos["uy"][b]).min() >= mm.MIN_ORIGIN, (kind, names[b])
            if edges is not None:
                assert mm.edges_of(nbs) == edges[b], (kind, names[b])
            keys, x = mm.pair_inputs(ref0["obs"][b], nbs, np.float64)      # the oracle's (double)(float)(la_i * la_j)
            per_env.append((poses, nbs, keys, x))
        if edges is None:          # bulk: many-neighbour rows
            assert max(len(nb) for _, nbs, _, _ in per_env for nb in nbs) >= (8 if N >= 20 else 2), kind
        if edges is not None:      # targets and walls are placed so that neighbours' raw rewards differ
            for b, (poses, nbs, _, _) in enumerate(per_env):
                for i, nb in enumerate(nbs):
                    if len(nb) >= 2 and names[b] != "clique_all":
                        assert np.ptp(ref0["raw"][b][nb]) > 1e-5, (kind, names[b], i)      # (100 ulps and more)
        for c in mm.RUNGS:
            sd = mm.spread_ladder(sd0, c)
            scored = []
            for poses, nbs, keys, x in per_env:
                s, mag = pmi_forward_fp64(sd, x, want_scale=True) if keys else (np.zeros(0), np.zeros(0))
                s = s.astype(np.float32).astype(np.float64)                 # the oracle's fp32 score
                scored.append((dict(zip(keys, s)), dict(zip(keys, mag))))
                spread[c] = max(spread[c], mm.in_neighbourhood_spread(nbs, scored[-1][0]))
                if c == 0:
                    assert len(set(s)) <= 1
            for coop in mm.COOPS:
                ref, _ = oracle_step(N, M, dim, kind, coop, sd, st)
                np.testing.assert_array_equal(ref["raw"], ref0["raw"])
                for b, ((poses, nbs, keys, x), (sc, mg)) in enumerate(zip(per_env, scored)):
                    got, mean = mm.mix_fp64(poses, ref["raw"][b], sc, coop=coop, round_weights=True)
                    err = np.abs(got - ref["reward"][b]).max()
                    assert err <= 1e-12, (kind, names[b], coop, c, err)
                    assert abs(mean - ref["reward"][b].mean()) <= 1e-12
                    second[c] = max(second[c], mm.leg_a_second_term(nbs, ref["raw"][b], mg, coop).max())
                    if coop > 0 and kind != "clip":
                        moved = best_swap(nbs, ref["raw"][b], sc, coop)
                        swap[c] = max(swap[c], moved)
                        if any((nb > i).sum() >= 2 for i, nb in enumerate(nbs)):      # the scene has a run of two or more
                            key = (kind, names[b], coop)
                            scene_swap[key] = max(scene_swap.get(key, 0.0), moved)
                    if kind == "clip" and names[b] == "wall_chain":
                        un = mm.mix_fp64(poses, ref["raw"][b], sc, coop=coop, want_unclipped=True)
                        raw = ref["raw"][b]
                        assert (np.abs(un) > 1.0).any(), (coop, c)                  # the final clip decides these rows
                        if coop == 0.3:  # raw beyond the clip, the mixed result inside it (coop = 0: the result IS raw;
                                         # coop = 1 on the top rung: one neighbour's raw reward, beyond the clip as well)
                            assert ((np.abs(raw) > 1.0) & (np.abs(un) < 1.0)).any(), (coop, c)
    if os.environ.get("UAVTRACK_TEST_REPORT"):
        print(f"[maacr-mix] N{N} M{M} dim{dim}: spread {spread}, leg-A second term {second}, swap / bound {swap}", flush=True)
    assert spread[0] == 0.0
    assert 0.0 < spread[1] <= 0.25, spread                  # today's regime: every weight within a few percent of 1 / k
    assert 2.0 <= spread[64] <= 10.0, spread
    assert spread[4096] >= 90.0, spread                     # exp(90) overflows fp32: a softmax without the shift gives inf
    for c in mm.RUNGS:
        assert (second[c] < 1e-3) == (c in mm.LEG_A_RUNGS), (c, second)
        if c >= 1:
            assert swap[c] > 100.0, (c, swap)
    # ... and every scene that has a run of two or more decides on some rung, at either cooperative weight: the stars, the
    # chain and the dense boxes from c = 64 up (the star whose hub sits in the middle at c = 64 alone: on the top rung the
    # hub's whole weight lies on an earlier neighbour), the flat cliques on the top rung only
    assert scene_swap and min(scene_swap.values()) > 100.0, {k: v for k, v in scene_swap.items() if v <= 100.0}


def test_mix_geometry_restates_the_launch():
    want = {7: (64, 9, 4, 1), 20: (64, 3, 4, 1), 32: (64, 2, 4, 1), 33: (256, 7, 4, 2), 50: (256, 5, 4, 2),
            64: (64, 1, 4, 2), 65: (256, 3, 1, 0), 130: (256, 1, 1, 0), 5: (64, 12, 4, 1), 10: (64, 6, 4, 1)}
    for N, g in want.items():
        assert mm.mix_geometry(N) == g, N
    # The library does not report the mix launch's geometry, so the restatement is tied to the launch code itself: the
    # expressions it restates must stand in launch_pmi_finalize as they do today.  A change there fails here, before the
    # S * B edge cases of test_hip_maacr_mix.py silently stop being edge cases.
    src = open(os.path.join(PKG, "csrc", "pmi_kernel.hip")).read()
    launch = src[src.index("hipError_t launch_pmi_finalize"):src.index("hipError_t launch_ep_reward")]
    for expr in ("constexpr int mix_batch(int ws) { return ws ? 4 : 1; }",):
        assert expr in src, expr
    for expr in ("const int dflt = (c.n_uav <= 64 && (64 / c.n_uav) * c.n_uav * 10 >= 64 * 9) ? 64 : (c.n_uav <= 256 ? 256 : kMaxWorkgroup);",
                 "const int wgs = dflt;", "f.E = wgs / c.n_uav;", "const int kMixBatch = mix_batch(c.n_uav <= 64 ? 1 : 0);",
                 "(f.SB + f.E * kMixBatch - 1) / (f.E * kMixBatch)",
                 "if (c.n_uav <= 32)\n        hipLaunchKernelGGL(pmi_mix_kernel<1>", "else if (c.n_uav <= 64)\n        hipLaunchKernelGGL(pmi_mix_kernel<2>",
                 "else\n        hipLaunchKernelGGL(pmi_mix_kernel<0>"):
        assert expr in launch, expr


def test_pool_restatement_by_hand():
    """The branches on totals small enough to follow by hand (one lane per entry)."""
    assert mm.pool_branches([[2]] * 16) == ({"fits"}, 64)
    # 40 per step: block of 64 (24 left, request 160 at once), 24 < 40: the lanes 30 + 10 split -- no prefix fits (30 > 24)
    seen, _ = mm.pool_branches([[30, 10]] * 3)
    assert "split_run" not in seen
    seen, _ = mm.pool_branches([[10, 30]] * 3)             # 10 <= 24 stays, 30 moves on
    assert "split_run" in seen
    # a last step that does not fit and has no request outstanding takes exactly what moves: 40, where any other step
    # takes a block of 64 -- the last-step clause decides
    seen, reserved = mm.pool_branches([[2], [70 - 8], [40]])
    assert seen == {"fits", "last_step_exact"} and reserved == 64 + 40
    # (one step more and the block of 4 * 62 asked for at step 1 takes them instead)
    assert mm.pool_branches([[2], [70 - 8], [40], [0]]) == ({"fits"}, 64 + 4 * 62)
    # more than a block is taken exactly on any step: the last-step clause is not what decides, and is not recorded
    seen, reserved = mm.pool_branches([[2], [70]])
    assert seen == set() and reserved == 64 + 70
    # the early request (64, made at step 2 with 16 < 2 * 16 left) is smaller than what moves at step 4 (70)
    seen, reserved = mm.pool_branches([[16], [16], [16], [16], [70], [0]])
    assert seen == {"fits", "request_too_small"} and reserved == 64 + 64 + 70
    # requested at step 1 (2 < 2 * 31, two more steps follow), never needed
    seen, _ = mm.pool_branches([[31], [31], [0], [0]])
    assert "block_never_used" in seen


POOL_EXPECT = {      # (scene, T) -> branches, the same at all three shapes
    ("steady", 16): {"fits", "split_run"}, ("steady", 17): {"fits", "split_run"},
    ("steady", 32): {"fits", "split_run"}, ("steady", 36): {"fits", "split_run"},
    ("collapse", 16): {"fits"}, ("collapse", 17): {"fits"},
    # (the merge at step 31 moves 100 / 125 / 66 pairs: more than a block, taken exactly on any step -- not the last-step
    # clause; likewise the 201 pairs of 10x10's step 35)
    ("collapse", 32): {"fits", "split_run"}, ("collapse", 36): {"fits", "split_run", "request_too_small"},
    ("disperse", 16): {"fits"}, ("disperse", 17): {"fits"}, ("disperse", 32): {"fits"},
    ("disperse", 36): {"fits", "block_never_used"},
    # the first 2 pairs arrive at step 15: the last step of a 16-step launch, with no block in hand and none asked for
    ("join", 16): {"last_step_exact"}, ("join", 17): {"fits"}, ("join", 32): {"fits"}, ("join", 36): {"fits"},
}


def pool_oracle_runs(N, M, E, st, T):
    """Per step, the wavefront's emitted pairs per lane and the smallest |d - dp| over every pair, from the oracle."""
    orc = OracleEnv(OracleConfig(n_envs=E, n_uav=N, m_targets=M, cooperative=0.3), n_threads=4)
    orc.set_state(**st)
    act = mm.rigid_actions(T, E, N)
    runs, margin, differ = [], np.inf, []
    for t in range(T):
        raw = orc.step(act[t])["raw"]
        pos = orc.get_state()
        poses = [mm.poses_of(pos, e, 2) for e in range(E)]
        for p in poses:
            margin = min(margin, np.abs(mm.pair_distances(p) - mm.DP).min())
            assert np.hypot(p[0], p[1]).min() >= mm.MIN_ORIGIN
        runs.append(mm.wave_runs(poses))
        # how far the raw rewards of one UAV's later neighbours differ, at most: what a score from the wrong slot can move
        differ.append(max([np.ptp(raw[e][nb[nb > i]]) for e, p in enumerate(poses) for i, nb in enumerate(mm.neighbour_sets(p))
                           if (nb > i).sum() >= 2] or [0.0]))
    return runs, margin, differ


@pytest.mark.parametrize("N,M,E", mm.POOL_SHAPES)
def test_pool_scenes_reach_every_branch(N, M, E):
    """Nothing is missing: with the launch lengths 16, 17, 32 and 36 the four scenes reach all five branches at every
    shape, by legal dynamics (every UAV flies 20 m per step under the alternating actions 5 and 6).  The branch set of
    every scene and launch is asserted exactly; it is the same at all three shapes."""
    reached = set()
    for name, st in mm.pool_scenes(N, M, E).items():
        runs, margin, differ = pool_oracle_runs(N, M, E, st, max(mm.POOL_LAUNCHES))
        assert margin >= mm.MIN_EDGE_MARGIN, (name, margin)
        totals = [sum(r) for r in runs]
        if name == "collapse":        # the chain of three alone, then more than a block at once
            assert totals[:mm.COLLAPSE_STEP] == [2] * mm.COLLAPSE_STEP and totals[mm.COLLAPSE_STEP] > mm.POOL_BLOCK + 2
            assert min(differ[mm.COLLAPSE_STEP:]) > 1e-3, differ      # the merged runs hold raw rewards that differ
                                                                      # (a leg-B bound is a few 1e-6)
        if name == "disperse":
            assert totals == [2] * mm.COLLAPSE_STEP + [0] * (len(totals) - mm.COLLAPSE_STEP)
        if name == "join":
            assert totals == [0] * mm.JOIN_STEP + [2] * (len(totals) - mm.JOIN_STEP)
        for T in mm.POOL_LAUNCHES:
            seen, reserved = mm.pool_branches(runs[:T])
            assert reserved >= sum(totals[:T])
            assert seen == POOL_EXPECT[(name, T)], (name, T, seen)
            reached |= seen
    assert reached == set(mm.POOL_BRANCHES), set(mm.POOL_BRANCHES) - reached
