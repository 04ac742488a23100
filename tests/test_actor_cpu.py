"""The device actor's f16 x 3 split (csrc/actor.h) emulated in numpy (tests/actor_mirror.py) against fp64 and against an
fp32 fmaf chain, on the CPU.  What it establishes is the bound tests/test_hip_actor.py holds the kernel to: logits within
2^-20 of the row's magnitude m_row (the largest sum of |terms|), hence probabilities within 1e-5 max(1, m_row) -- and as
accurate as an fp32 forward (2x its worst error, plus one fp32 rounding of m_row) wherever the block scales keep the f16 planes normal."""
import numpy as np
import pytest

import actor_mirror as mirror


def linear_policy(H, A, seed, fc2=5.0, w1=1.0):
    """torch.nn.Linear's default initialisation (uniform +-1/sqrt(fan_in)), fc2 scaled like the GPU tests' policies."""
    r = np.random.RandomState(seed)
    u = lambda shape, fan: r.uniform(-1.0, 1.0, shape) / np.sqrt(fan)
    f = lambda a: np.asarray(a, np.float32)
    return {"fc1.weight": f(u((H, 12), 12) * w1), "fc1.bias": f(u(H, 12)),
            "fc2.weight": f(u((A, H), H) * fc2), "fc2.bias": f(u(A, H))}


def nominal_obs(R, xb, seed, factor=1.0):
    """Uniform within +-factor * xb; every eighth row exactly at the bounds (random signs)."""
    r = np.random.RandomState(seed)
    x = r.uniform(-1.0, 1.0, (R, 12)) * xb * factor
    x[::8] = np.sign(r.uniform(-1.0, 1.0, (len(x[::8]), 12))) * xb * factor
    return x.astype(np.float32)


XB = mirror.actor_xb()
XB_BOX = mirror.actor_xb(x_max=20000.0, y_max=20000.0, dc=50.0)
XB_DC5 = mirror.actor_xb(x_max=20000.0, y_max=20000.0, dc=5.0)
BASE = linear_policy(128, 12, 0)

# name -> (policy, xb, observation scale, fp32-equivalent): the last is False where a small T1 (a wide nominal range)
# puts W1's lo plane among the f16 subnormals -- there the split keeps 2^-20 m_row, not fp32's accuracy
CASES = {
    "nominal": (BASE, XB, 1.0, True),
    "H1": (linear_policy(1, 12, 1), XB, 1.0, True),
    "H33": (linear_policy(33, 12, 2), XB, 1.0, True),
    "H256": (linear_policy(256, 12, 3), XB, 1.0, True),
    "H1000": (linear_policy(1000, 12, 4), XB, 1.0, True),
    "H4096": (linear_policy(4096, 12, 5), XB, 1.0, True),
    "na2": (linear_policy(128, 2, 6), XB, 1.0, True),
    "A48": (linear_policy(200, 48, 7), XB, 1.0, True),
    "T1_at_max": (mirror.at_scale(BASE, XB, t1=mirror.SCALE_EXP), XB, 1.0, True),
    "T2_at_max": (mirror.at_scale(BASE, XB, t2=mirror.SCALE_EXP), XB, 1.0, True),
    "T1_2^-24": (mirror.at_scale(BASE, XB, t1=-24), XB, 1.0, True),
    "T2_2^-24": (mirror.at_scale(BASE, XB, t2=-24), XB, 1.0, True),
    "weights_x2^-20": (mirror.rescale(BASE, 2.0 ** -20, 2.0 ** -20), XB, 1.0, True),
    "weights_x2^12": (mirror.rescale(BASE, 2.0 ** 12, 2.0 ** 12), XB, 1.0, True),
    "b1_large_W1_tiny": (mirror.rescale(BASE, 2.0 ** -10, 2.0 ** -10, sb1=2.0 ** 10), XB, 1.0, True),
    "inputs_x100": (BASE, XB, 100.0, True),
    "box_20km_dc50": (BASE, XB_BOX, 1.0, True),
    "box_20km_dc5_W1x30": (linear_policy(128, 12, 0, w1=30.0), XB_DC5, 1.0, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_actor_split_error_model(name):
    sd, xb, factor, fp32_like = CASES[name]
    x = nominal_obs(256, xb, seed=len(name), factor=factor)
    assert not mirror.cap_reached(sd, x, xb).any()                 # (the saturating forward has its own test)
    s = mirror.split_forward(sd, x, xb)
    lg64, p64, m = mirror.forward_fp64(sd, x)
    chain = mirror.chain_fp32_logits(sd, x)
    e_split = np.abs(s["logits"] - lg64).max(axis=1)
    e_chain = np.abs(chain - lg64).max(axis=1)
    assert (e_split <= 2.0 ** -20 * m).all(), (name, (e_split / m).max())
    dp = np.abs(s["probs"] - p64).max(axis=1)
    assert (dp <= 1e-5 * np.maximum(1.0, m)).all(), (name, (dp / np.maximum(1.0, m)).max())
    if fp32_like:
        assert e_split.max() <= 2.0 * e_chain.max() + 2.0 ** -24 * m.max(), (name, e_split.max(), e_chain.max())
    else:
        assert e_split.max() > 2.0 * e_chain.max()                 # (why this case is listed apart)
    if name.startswith("T") or name.startswith("weights"):
        assert max(s["T1"], s["T2"]) <= 2.0 ** mirror.SCALE_EXP and min(s["T1"], s["T2"]) >= 2.0 ** -mirror.SCALE_EXP
    if name in ("T1_at_max", "T2_at_max", "T1_2^-24", "T2_2^-24"):
        # the same policy with its layers rescaled against each other: the same scaled planes, the same bits
        ref = mirror.split_forward(BASE, x, xb)
        assert np.array_equal(s["logits"], ref["logits"]), name
        T = s["T1"] if name.startswith("T1") else s["T2"]
        assert T == 2.0 ** {"T1_at_max": 60, "T2_at_max": 60, "T1_2^-24": -24, "T2_2^-24": -24}[name]


def test_actor_block_scales_and_saturation():
    """pack_actor_blob's scales for the nominal bounds of uavtrack_set_actor_weights, and the capped forward: inputs beyond
    60000 and hidden values beyond 60000 / T1 saturate in the split exactly as in the fp64 forward with those clamps."""
    T1, T2 = mirror.scales_of(BASE, XB)
    w1, b1, w2, _ = mirror.weights(BASE)
    bound = mirror._act_bound(w1, b1, XB)
    assert 256.0 < T1 * bound <= 512.0 and T2 * np.abs(w2).max() <= 16384.0 < 2 * T2 * np.abs(w2).max()
    assert mirror.scales_of(mirror.rescale(BASE, 0.0, 0.0), XB) == (2.0 ** 24, 2.0 ** 24)       # zero layers: any scale
    r = np.random.RandomState(5)
    x = nominal_obs(256, XB, seed=9)
    hot = r.rand(*x.shape) < 0.1
    x[hot] = (np.sign(r.uniform(-1, 1, hot.sum())) * 10.0 ** r.uniform(3, 9, hot.sum())).astype(np.float32)
    capped = mirror.cap_reached(BASE, x, XB)
    assert 0.2 < capped.mean() < 1.0
    s = mirror.split_forward(BASE, x, XB)
    assert np.isfinite(s["probs"]).all() and np.allclose(s["probs"].sum(axis=1), 1.0, atol=1e-6)
    _, pc, mc = mirror.forward_fp64(BASE, x, XB, capped=True)
    assert (np.abs(s["probs"] - pc).max(axis=1) <= 1e-5 * np.maximum(1.0, mc)).all()
    _, p64, _ = mirror.forward_fp64(BASE, x)
    assert not np.allclose(p64[capped], pc[capped], atol=1e-3)        # the cap matters on those rows


def test_actor_softmax_at_huge_logits():
    """Logits past ~2^30: the max slot's exponent (the rounding residue of m log2 e) would over- or underflow exp2 --
    the kernel redoes such a row shifted by its own maximum, which the mirror restates: finite probabilities, summing
    to 1, the argmax's mass where fp64 puts it."""
    sd = mirror.rescale(BASE, 2.0 ** 20, 2.0 ** 20)
    x = nominal_obs(256, XB, seed=4)
    s = mirror.split_forward(sd, x, XB)
    _, p64, m = mirror.forward_fp64(sd, x)
    assert np.abs(s["logits"]).max() > 2.0 ** 31
    assert np.isfinite(s["probs"]).all() and np.allclose(s["probs"].sum(axis=1), 1.0, atol=1e-6)
    assert (np.abs(s["probs"] - p64).max(axis=1) <= 1e-5 * np.maximum(1.0, m)).all()
