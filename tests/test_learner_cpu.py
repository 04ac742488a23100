"""The fp64 mirror of the device learner (tests/learner_mirror.py) against the reference's own fp32 updates
recorded in tests/golden/f5_actor_critic_update.npz (tools/gen_learner_golden.py).  No GPU."""
import numpy as np
import pytest

from conftest import load_golden
import learner_mirror as mirror

CASES = ("h128", "h48", "n1")


def _replay(z, meta, case, loss="reference", upto=5):
    H, A = meta["cases"][case]["hidden"], meta["A"]
    S, Ac, R, S2 = z["store_states"], z["store_actions"], z["store_rewards"], z["store_next_states"]
    P = z[f"{case}_w0"].size
    st = {"params": z[f"{case}_w0"].astype(np.float64), "exp_avg": np.zeros(P), "exp_avg_sq": np.zeros(P),
          "step": np.zeros(8, np.int64)}
    rec = []
    for u in range(upto):
        i = z[f"{case}_idx"][u]
        st, al, cl, td = mirror.update(st, H, A, S[i], Ac[i], R[i], S2[i], meta["gamma"],
                                       (meta["actor_lr"], meta["critic_lr"]), loss)
        rec.append((st, al, cl, td))
    return rec


@pytest.mark.parametrize("case", CASES)
def test_mirror_reproduces_reference_updates(case):
    z, meta = load_golden("f5_actor_critic_update")
    rec = _replay(z, meta, case)
    for u, (st, al, cl, td) in enumerate(rec):
        # the recorded losses are fp32 values whose own rounding (log of an fp32 softmax, a mean over n x n
        # products) reaches ~2e-6 relative: 1e-5 relative for the losses, 1e-6 for td_delta and the parameters
        assert al == pytest.approx(float(z[f"{case}_actor_loss"][u]), rel=1e-5), (u, al)
        assert cl == pytest.approx(float(z[f"{case}_critic_loss"][u]), rel=1e-6, abs=1e-7), (u, cl)
        np.testing.assert_allclose(td, z[f"{case}_td"][u], rtol=1e-6, atol=1e-6)
    for tag, u in ((1, 0), (5, 4)):
        st = rec[u][0]
        np.testing.assert_allclose(st["params"], z[f"{case}_params{tag}"], rtol=0, atol=1e-6)
        np.testing.assert_array_equal(st["step"], z[f"{case}_step{tag}"])
        for k in ("exp_avg", "exp_avg_sq"):      # gradients are sums of cancelling terms: error relative to the largest
            ref = z[f"{case}_{k}{tag}"]
            np.testing.assert_allclose(st[k], ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_reference_loss_is_the_broadcast_product_of_means():
    """The reference's actor loss is mean(-log p) * mean(delta) ([n,1] * [n] broadcasts to [n,n]); the per-sample form
    differs on the fixture's batch, in the loss and in the actor's gradient."""
    z, meta = load_golden("f5_actor_critic_update")
    H, A = meta["cases"]["h128"]["hidden"], meta["A"]
    i = z["h128_idx"][0]
    args = (z["h128_w0"], H, A, z["store_states"][i], z["store_actions"][i], z["store_rewards"][i],
            z["store_next_states"][i], meta["gamma"])
    al_ref, cl_ref, td_ref, g_ref = mirror.losses_and_grads(*args, loss="reference")
    al_ps, cl_ps, td_ps, g_ps = mirror.losses_and_grads(*args, loss="per_sample")
    assert al_ref == pytest.approx(float(z["h128_actor_loss"][0]), rel=1e-6)
    assert abs(al_ps - al_ref) > 1e-3 * abs(al_ref)
    assert cl_ps == cl_ref and np.array_equal(td_ps, td_ref)
    n_actor = 12 * H + H + A * H + A
    assert np.abs(g_ps[:n_actor] - g_ref[:n_actor]).max() > 1e-3 * np.abs(g_ref[:n_actor]).max()
    np.testing.assert_array_equal(g_ps[n_actor:], g_ref[n_actor:])


def test_priority_write_last_occurrence_wins():
    z, meta = load_golden("f5_actor_critic_update")
    idx = z["h128_idx"][0]
    assert len(set(idx.tolist())) < len(idx)
    got = mirror.last_wins(z["prio_before"], idx, np.abs(z["h128_td"][0]))
    np.testing.assert_array_equal(got.astype(np.float32), z["prio_after"])
