"""The float64 mirror of the device PMI trainer (tests/pmi_trainer_mirror.py) against the reference's own fp32
train_pmi calls recorded in tests/golden/f6_pmi_train.npz (tools/gen_pmi_trainer_golden.py), and its hand-written
train-mode BatchNorm backward against torch autograd in float64.  No GPU."""
import numpy as np
import pytest
import torch

import pmi_trainer_fixture as fixture
import pmi_trainer_mirror as mirror


def _flat(sd, names):
    return np.concatenate([np.asarray(sd[k], np.float64).ravel() for k in names])


@pytest.mark.parametrize("case", ["h64", "h128"])
def test_mirror_reproduces_reference_calls(case):
    """Outputs and losses to the recording's fp32 rounding (measured: 2e-6 and 5e-8); data-determined parameters to
    4e-6, running_var to 2.5e-6.  The noise-driven elements -- the pre-BN biases, whose float64 gradient is zero --
    move in the reference by Adam steps of at most lr (1 - beta1) / sqrt(1 - beta2) each and are not compared."""
    z, meta, rows = fixture.load()
    c = meta["cases"][case]
    H, bs = c["hidden"], c["batch_size"]
    sd = fixture.initial_state(z, meta, case)
    adam = mirror.new_adam()
    for call in range(2):
        t, u = fixture.indices(z, meta, case, call)
        sd, adam, avg, rec = mirror.train_pmi(sd, adam, rows, meta["n_uav"], t, u, bs)
        assert avg == pytest.approx(float(z[f"{case}_c{call}_avg_loss"]), rel=1e-6)
        np.testing.assert_allclose(np.stack(rec["o12"]), z[f"{case}_c{call}_o12"], rtol=1e-5, atol=5e-6)
        np.testing.assert_allclose(np.stack(rec["o13"]), z[f"{case}_c{call}_o13"], rtol=1e-5, atol=5e-6)
        g = np.max([np.abs(_flat(gr, mirror.param_names())) for gr in rec["grads"]], axis=0)
        noise = g < 1e-12
        assert noise.sum() == 4 * H
        nv = fixture.view_flat(noise, H, z, case)
        # the recording's own gradients of the same elements are fp32 noise (stored as float16: below 2e-7, most 0)
        gabs = z[f"{case}_c{call}_gabs"].astype(np.float64)
        assert gabs[nv].max() < 2e-7
        assert gabs[~nv].min() > 1e-6
        d = np.abs(fixture.view(sd, z, case) - fixture.recorded(z, case, call))
        assert d[~nv].max() < 1e-5, d[~nv].max()
        for bn in ("bn_comm", "bn_obs", "bn_boundary_state", "bn1"):
            np.testing.assert_allclose(sd[bn + ".running_var"], z[f"{case}_c{call}_sd_{bn}.running_var"], rtol=1e-5,
                                       atol=5e-6)
            assert sd[bn + ".num_batches_tracked"] == int(z[f"{case}_c{call}_sd_{bn}.num_batches_tracked"])
        assert [adam["step"][k] for k in mirror.param_names()] == list(z[f"{case}_c{call}_step"])
    m = np.concatenate([adam["exp_avg"][k].ravel() for k in mirror.param_names()])
    v = np.concatenate([adam["exp_avg_sq"][k].ravel() for k in mirror.param_names()])
    np.testing.assert_allclose(fixture.view_flat(m, H, z, case)[~nv], z[f"{case}_c1_exp_avg"][~nv], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(fixture.view_flat(v, H, z, case)[~nv], z[f"{case}_c1_exp_avg_sq"][~nv], rtol=1e-4,
                               atol=1e-10)


def test_mirror_first_batch_of_smallest_case():
    """H 48, batch 2: the first batch (before any noise-driven Adam move) matches the recording."""
    z, meta, rows = fixture.load()
    t, u = fixture.indices(z, meta, "h48", 0)
    _, _, _, rec = mirror.train_pmi(fixture.initial_state(z, meta, "h48"), mirror.new_adam(), rows, meta["n_uav"], t,
                                    u, 2)
    np.testing.assert_allclose(rec["o12"][0], z["h48_c0_o12"][0], rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(rec["o13"][0], z["h48_c0_o13"][0], rtol=1e-5, atol=5e-6)


@pytest.mark.parametrize("H,bs", [(1, 2), (7, 3), (48, 16), (64, 64)])
def test_mirror_gradients_match_torch_autograd_fp64(H, bs):
    import uavtrack
    torch.manual_seed(H * 31 + bs)
    net = uavtrack.make_pmi_net(H).double().train()
    rng = np.random.RandomState(H + bs)
    x12, x13 = rng.uniform(-1, 1, size=(bs, 12)), rng.uniform(-1, 1, size=(bs, 12))
    sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    assert list(sd) == mirror.state_names()
    assert [n for n, _ in net.named_parameters()] == mirror.param_names()
    loss, o12, o13, grads, _ = mirror.loss_and_grads(sd, x12, x13)
    o1, o2 = net(torch.from_numpy(x12)), net(torch.from_numpy(x13))
    tl = uavtrack.pmi_contrastive_loss(o1, o2)
    tl.backward()
    assert loss == pytest.approx(float(tl.detach()), rel=1e-12)
    np.testing.assert_allclose(o12, o1.detach().numpy().reshape(-1), rtol=1e-12, atol=1e-12)
    for name, p in net.named_parameters():
        np.testing.assert_allclose(grads[name], p.grad.numpy(), rtol=1e-9, atol=1e-12, err_msg=name)
    # the running statistics the two forwards left behind
    msd = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sd.items()}
    mirror._update_running(msd, mirror.forward(sd, x12)[2], bs)
    mirror._update_running(msd, mirror.forward(sd, x13)[2], bs)
    for k, v in net.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(msd[k], v.numpy(), rtol=1e-12, atol=1e-14, err_msg=k)
