"""The fp64 oracle of the greedy baseline policy (oracle/uav_oracle.c, orc_greedy_actions) at the edges the reference
recording tests/golden/greedy_ref.npz does not reach, its per-UAV robustness verdict, and the condition the GPU comparison
rests on: on every shape case of tests/greedy_scenes.py at most 10 % of the scoring-branch decisions are set aside.
No GPU: the states come from the oracle's own reset and steps, rounded to fp32.
"""
import numpy as np
import pytest

import greedy_scenes as gs
from oracle import OracleConfig, OracleEnv, greedy_actions


def scene_oracle(sc, B=1):
    orc = OracleEnv(OracleConfig(**gs.scene_config(sc, B)))
    orc.set_state(**gs.scene_state(sc, B))
    return orc


@pytest.mark.parametrize("sc", gs.SCENES + [gs.NEAR_DC], ids=gs.SCENE_IDS + [gs.NEAR_DC.name])
def test_oracle_gives_the_hand_written_action(sc):
    """force_argmax (no draws): every UAV with a hand-written answer takes it.  Then the unforced policy over seeds and
    environments: the same answer wherever the draws select the scoring branch, the middle action (lower of two) on
    keep-straight, anything in range on a random action -- and all three branches occur."""
    orc = scene_oracle(sc)
    act, aid = greedy_actions(orc, 0, np.zeros(1, np.int32), force_argmax=True)
    assert (aid["branch"] == 2).all()
    np.testing.assert_array_equal(act, gs.scene_want(sc, act), err_msg=sc.name)
    B = 8
    orc = scene_oracle(sc, B)
    seen = set()
    for seed in range(6):
        a2, aid2 = greedy_actions(orc, seed, np.full(B, seed, np.int32), env_offset=seed * 1000)
        steer, straight = aid2["branch"] == 2, aid2["branch"] == 1
        np.testing.assert_array_equal(a2[steer], np.broadcast_to(act, a2.shape)[steer], err_msg=f"{sc.name} seed {seed}")
        assert (a2[straight] == (sc.na - 1) // 2).all(), sc.name
        assert a2.min() >= 0 and a2.max() < sc.na
        seen |= set(np.unique(aid2["branch"]).tolist())
    assert seen == {0, 1, 2}, (sc.name, seen)


def test_exact_ties_are_robust_and_knife_edges_are_not():
    """What the verdict says on the constructed scenes: mirror-image and coincident targets tie bitwise in fp32 too, so the
    index decides and the decision is robust; an angle of exactly 0 with even na sits on an action boundary and pi on the
    seam of the wrap, so those are not (the GPU test compares them with the hand-written answer instead)."""
    verdict = {}
    for sc in gs.SCENES:
        _, aid = greedy_actions(scene_oracle(sc), 0, np.zeros(1, np.int32), force_argmax=True)
        verdict[sc.name] = aid["robust"][0].tolist()
    for name in ("mirror_first_north", "mirror_first_south", "on_target_twice", "crowded_near_loses", "crowded_near_wins",
                 "coincident_inside_and_outside", "heading_minus_pi", "heading_plus_pi", "heading_3p1_target_west",
                 "dead_ahead_na9", "dead_ahead_na3"):
        assert all(verdict[name]), (name, verdict[name])
    for name in ("dead_ahead_na12", "dead_ahead_na2", "dead_astern"):
        assert not any(verdict[name]), (name, verdict[name])
    # exactly_dc: |d - dc| = 0 <= 1e-2, the pair is uncertain to the verdict; it decides UAV 0's choice, not UAV 1's
    assert verdict["exactly_dc"] == [False, True]
    # a mirror image that is NOT bitwise equal in fp32 is no exact tie: 0.25 m further south loses by 2.8e-6 < 2e-5
    sc = gs.Scene("mirror_broken", 12, [(1000, 1000, 0.0)], [(1000, 1300), (1000, 699.75)], [11])
    act, aid = greedy_actions(scene_oracle(sc), 0, np.zeros(1, np.int32), force_argmax=True)
    assert act[0, 0] == 11 and not aid["robust"][0, 0]


def test_near_dc_pair_sets_aside_only_the_uav_it_can_affect():
    sc = gs.NEAR_DC
    orc = scene_oracle(sc)
    act, aid = greedy_actions(orc, 0, np.zeros(1, np.int32), force_argmax=True)
    assert 0 < aid["dist"][0] < 1e-2                       # the old rule drops the whole environment
    assert aid["robust"][0].tolist() == gs.NEAR_DC_ROBUST
    # random and keep-straight actions are always robust (bit-exact draws)
    B = 16
    orc = scene_oracle(sc, B)
    for seed in range(4):
        _, aid = greedy_actions(orc, seed, np.zeros(B, np.int32))
        assert aid["robust"][aid["branch"] != 2].all()
        assert not aid["robust"][:, 0][aid["branch"][:, 0] == 2].any()
        assert aid["robust"][:, 1:].all()


def old_rule(aid):
    """The margins the suite used before: per-UAV score and angle, per-ENVIRONMENT distance to dc."""
    return (aid["score"] > 2e-5) & (aid["angle"] > 1e-4) & (aid["dist"][:, None] > 1e-2)


@pytest.fixture(scope="module")
def shape_verdicts():
    """The oracle on every shape case, once: name -> (actions, aids)."""
    out = {}
    for s in gs.SHAPES:
        orc, sc = gs.oracle_state(s)
        out[s.name] = greedy_actions(orc, gs.POLICY_SEED, sc, env_offset=s.env_offset)
    return out


@pytest.mark.parametrize("s", gs.SHAPES, ids=gs.SHAPE_IDS)
def test_set_aside_share_is_capped(shape_verdicts, s):
    """The cap is a condition on the scene, not a measurement of the kernel: computed from the oracle alone."""
    act, aid = shape_verdicts[s.name]
    bad, scoring = gs.set_aside(aid)
    wgs, E = gs.greedy_E(s.N, s.M)
    print(f"\n[greedy set-aside] {s.name}: {bad} / {scoring} = {bad / max(scoring, 1):.4f} of the scoring-branch decisions "
          f"(old per-environment rule: {int(((aid['branch'] == 2) & ~old_rule(aid)).sum())}); workgroup {wgs}, E = {E}")
    assert scoring >= 0.4 * act.size                       # 0.75 * 0.7 of the draws steer
    assert bad <= gs.CAP * scoring, (s.name, bad, scoring)
    assert act.min() >= 0 and act.max() < s.na
    assert set(np.unique(aid["branch"]).tolist()) == {0, 1, 2}


def test_shapes_reach_the_geometry_they_are_there_for():
    """launch_greedy's paths, restated (greedy_scenes.greedy_E): both workgroup sizes on either side of N = 256, E shrunk
    by the LDS loop to 1 and to a value above 1, partly filled last workgroups, several workgroups everywhere."""
    geo = {s.name: gs.greedy_E(s.N, s.M) + (s.B,) for s in gs.SHAPES}
    assert geo["n256"][:2] == (256, 1) and geo["n257"][:2] == (512, 1) and geo["n512"][:2] == (512, 1)
    assert geo["n3_m4096"][:2] == (256, 1) and 256 // 3 > 1
    wgs, E, B = geo["n20_m1000"]
    assert 1 < E < wgs // 20 and B % E != 0
    for name in ("m1", "dense_20x10", "offset_2p32", "na_max"):
        wgs, E, B = geo[name]
        assert B % E != 0 and B > E, name
    for s in gs.SHAPES:
        wgs, E = gs.greedy_E(s.N, s.M)
        assert E >= 1 and E * s.N <= wgs and E * (8 * s.N + 12 * s.M) <= 64 * 1024      # the kernel's LDS stays in bounds
        assert s.B * s.N * s.M * s.N <= 2e8 and s.steps > 0
    assert {s.na for s in gs.SHAPES} >= {2, 3, 9, 12, gs.NA_MAX_50x25} and gs.NA_MAX_50x25 == 1677
    assert any(s.env_offset >= 2 ** 32 for s in gs.SHAPES)


def test_new_verdict_accepts_what_the_old_margins_accepted(shape_verdicts):
    """Wherever the per-environment rule accepted a UAV the per-UAV verdict does too -- with one stated exception: the old
    margins did not know the seam of the wrap at +-pi (index na - 1 on one side, 0 on the other), the verdict keeps 1e-4
    from it.  And it accepts more: on the dense box the old rule compared far fewer decisions."""
    more = 0
    for s in gs.SHAPES:
        act, aid = shape_verdicts[s.name]
        old = old_rule(aid)
        lost = old & ~aid["robust"]
        ang = (aid["best_angle"][lost] + np.pi) % (2 * np.pi) - np.pi
        assert (np.pi - np.abs(ang) <= 1e-4).all(), (s.name, ang)
        assert lost.sum() <= 1e-3 * old.size
        more += int((aid["robust"] & ~old & (aid["branch"] == 2)).sum())
    assert more > 0
    act, aid = shape_verdicts["n20_m1000"]
    steer = aid["branch"] == 2
    assert aid["robust"][steer].mean() > old_rule(aid)[steer].mean()
