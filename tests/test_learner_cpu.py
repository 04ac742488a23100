"""The fp64 mirror of the device learner (tests/learner_mirror.py) against the reference's own fp32 updates
recorded in tests/golden/f5_actor_critic_update.npz (tools/gen_learner_golden.py); the conversion between both device
trainers' flat Adam state and torch.optim.Adam state_dicts (uavtrack/adam.py).  No GPU."""
import numpy as np
import pytest
import torch

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
    al_ref, cl_ref, td_ref, g_ref = mirror.losses_and_grads(*args, loss="reference")[:4]
    al_ps, cl_ps, td_ps, g_ps = mirror.losses_and_grads(*args, loss="per_sample")[:4]
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


# ---- the flat Adam state <-> torch.optim.Adam.state_dict() (uavtrack.adam), shared by both device trainers

def _torch_adam(params, lr, steps, seed):
    """A torch.optim.Adam over params after max(steps) steps, tensor i stepped steps[i] times (a tensor without a
    gradient is skipped by torch and has no state)."""
    g = torch.Generator().manual_seed(seed)
    opt = torch.optim.Adam(params, lr=lr)
    for k in range(max(steps)):
        for p, n in zip(params, steps):
            p.grad = torch.randn(p.shape, generator=g) if k < n else None
        opt.step()
    return opt.state_dict()


def _assert_same_adam_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert sorted(a["state"]) == sorted(b["state"])
    for i, st in a["state"].items():
        assert sorted(st) == sorted(b["state"][i])
        for k, t in st.items():
            assert t.dtype == b["state"][i][k].dtype and torch.equal(t, b["state"][i][k]), (i, k)


def _check_round_trip(params, lr, steps, seed):
    """torch's own dict -> flat arrays -> dict: equal to torch's, absent tensors load as zeros, and Adam takes it."""
    from uavtrack.adam import flat, from_state_dict, split, to_state_dict
    sd = _torch_adam(params, lr, steps, seed)
    m, v, st = from_state_dict(params, lr, sd)
    P = sum(p.numel() for p in params)
    assert m.dtype == v.dtype == np.float32 and m.shape == v.shape == (P,) and st.dtype == np.int64
    np.testing.assert_array_equal(st, steps)
    for i, (mi, vi) in enumerate(zip(split(m, params), split(v, params))):
        if steps[i] == 0:
            assert i not in sd["state"] and not mi.any() and not vi.any()
        else:
            assert torch.equal(mi, sd["state"][i]["exp_avg"]) and torch.equal(vi, sd["state"][i]["exp_avg_sq"])
    back = to_state_dict(params, lr, m, v, st)
    _assert_same_adam_dict(back, sd)
    fresh = [torch.nn.Parameter(torch.zeros_like(p)) for p in params]
    opt = torch.optim.Adam(fresh, lr=lr)
    opt.load_state_dict(back)
    assert len(opt.state) == sum(1 for n in steps if n > 0)
    # a tensor at step 0 has no state, whatever its moments hold
    m2 = m.copy(); m2[:] = 1.0
    zero = [i for i, n in enumerate(steps) if n == 0]
    assert set(to_state_dict(params, lr, m2, v, st)["state"]) == set(range(len(params))) - set(zero)
    assert np.array_equal(flat(split(m, params)), m)
    return m, v, st


def test_adam_state_round_trip_pmi_parameters():
    import uavtrack
    torch.manual_seed(0)
    params = list(uavtrack.make_pmi_net(16).parameters())
    assert len(params) == 18
    steps = [3, 0, 3, 1, 2, 0, 3, 3, 1, 1, 0, 2, 3, 3, 2, 2, 0, 3]
    _check_round_trip(params, 1e-3, steps, seed=1)


def test_adam_state_round_trip_learner_actor_critic_split():
    """Two optimizers (actor, critic) over consecutive spans of one flat state, as DeviceActorCritic keeps them."""
    import uavtrack
    from uavtrack.adam import from_state_dict, to_state_dict
    torch.manual_seed(0)
    actor = list(uavtrack.ActorMLP(12, 24, 7).parameters())
    critic = list(uavtrack.ValueMLP(12, 24).parameters())
    (ma, va, sa), (mc, vc, sc) = (_check_round_trip(actor, 1e-4, [2, 2, 0, 1], seed=2),
                                  _check_round_trip(critic, 5e-4, [0, 4, 4, 3], seed=3))
    m, v, steps = np.concatenate([ma, mc]), np.concatenate([va, vc]), np.concatenate([sa, sc])
    na = sum(p.numel() for p in actor)
    assert m.size == na + sum(p.numel() for p in critic) and steps.size == 8
    for params, lr, f, t, ref in ((actor, 1e-4, slice(0, na), slice(0, 4), (ma, va, sa)),
                                  (critic, 5e-4, slice(na, None), slice(4, None), (mc, vc, sc))):
        sd = to_state_dict(params, lr, m[f], v[f], steps[t])
        for x, y in zip(from_state_dict(params, lr, sd), ref):
            assert np.array_equal(x, y)
