"""The device actor's arithmetic (csrc/actor.h: pack_actor_blob + actor_pick) restated in numpy, with the fp64 forwards it
is judged against.  Nothing here needs a GPU: tests/test_actor_cpu.py holds the split to an fp32 fmaf chain, and
tests/test_hip_actor.py holds the kernel to `forward_fp64` with the bound that comparison justifies.

The split as the kernel runs it (T1, T2: powers of two the host sizes from the weights and the nominal observation bounds
`xb`, clamped to 2^-60 .. 2^60):
  * weights: w' = f32(T w); hi = f16(w') to nearest, lo = f16(w' - hi)
  * inputs: x capped to +-60000; hi = f16(x) toward zero, lo = f16(x - hi) (one rounding); input 12 = 1 carries b1
  * layer 1, one fp32 accumulator, small terms first: z = ((W1l xh) + W1h xl) + W1h xh, T1-scaled
  * hidden: v = med3(z, 0, 60000); hi toward zero, lo = f16(v - hi)
  * layer 2: one fp32 accumulator across every 16-unit k-step of every hidden tile; per k-step W2l vh, W2h vl, W2h vh
  * logits: fmaf(acc, 1 / (T1 T2), b2)
An MFMA is modelled as exact products and one fp32 rounding of (accumulator + the k-step's 16 products)."""
from __future__ import annotations

import numpy as np

CAP = 60000.0                  # kActorCap: inputs and hidden values saturate here
OBS = 12
SCALE_EXP = 60                 # kActorScaleExp: T1, T2 in [2^-60, 2^60]


def actor_xb(x_max=2000.0, y_max=2000.0, dc=500.0, u_v_max=20.0, t_v_max=5.0) -> np.ndarray:
    """The nominal observation bounds uavtrack_set_actor_weights builds (csrc/api_env.hip)."""
    vr = 1.0 + t_v_max / u_v_max
    pos = 4.0 * max(x_max, y_max) / dc
    return np.array([1, 1, 2, 2, 1, 1, 1, vr, vr, pos, pos, 1], np.float64)


def xb_of(cfg) -> np.ndarray:
    """actor_xb of an EnvConfig."""
    return actor_xb(cfg.x_max, cfg.y_max, cfg.dc, cfg.u_v_max, cfg.t_v_max)


def weights(sd):
    """(w1 [H,12], b1 [H], w2 [A,H], b2 [A]) as fp64 copies of their fp32 values, from a state dict or a module."""
    sd = sd.state_dict() if hasattr(sd, "state_dict") else sd

    def g(k):
        v = sd[k]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        return v.astype(np.float32).astype(np.float64)
    return tuple(g(k) for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))


def _act_bound(w1, b1, xb):
    a = np.abs(b1).copy()
    for k in range(OBS):                                      # the host's summation order
        a = a + np.abs(w1[:, k]) * xb[k]
    return float(a.max())


def exponents(w1, b1, w2, xb):
    """(e1, e2): the exponents of T1 and T2 before the 2^+-60 clamp (pack_actor_blob's pow2_below)."""
    w1max = float(max(np.abs(w1).max(), np.abs(b1).max()))
    e = lambda bound, target: int(np.floor(np.log2(target / bound))) if bound > 0.0 and np.isfinite(bound) else 24
    return min(e(_act_bound(w1, b1, xb), 512.0), e(w1max, 16384.0)), e(float(np.abs(w2).max()), 16384.0)


def block_scales(w1, b1, w2, xb):
    """(T1, T2) of pack_actor_blob: T1 (bound of |pre-activation| over |x_k| <= xb_k) <= 512 and T1 max |W1, b1| <= 16384;
    T2 max |W2| <= 16384; each clamped to 2^-60 .. 2^60."""
    return tuple(float(np.ldexp(1.0, min(SCALE_EXP, max(-SCALE_EXP, e)))) for e in exponents(w1, b1, w2, xb))


def scales_of(sd, xb):
    return block_scales(*weights(sd)[:3], xb)


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def rtz16(a):
    """f16 toward zero (v_cvt_pkrtz_f16_f32), as fp64."""
    a = np.asarray(a, np.float32)
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)


def rne16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def split_w(w, T):
    """(hi, lo) f16 planes of T w as pack_actor_blob writes them."""
    s = _r32(T * w)
    hi = rne16(s)
    return hi, rne16(_r32(s - hi))


def split_v(v):
    """(hi, lo) of an fp32 value on the device: toward zero, then the remainder rounded once (v_fma_mix)."""
    hi = rtz16(v)
    return hi, rne16(np.asarray(v, np.float64) - hi)


def _mfma(acc, a, b):
    """acc [R, C] + a [R, 16] @ b [16, C]: exact products, one fp32 rounding."""
    return _r32(acc + a @ b)


def split_forward(sd, x, xb):
    """The kernel's arithmetic on observations x [R, 12] -> dict(logits, probs [R, A], m_row [R], T1, T2)."""
    w1, b1, w2, b2 = weights(sd)
    H, A = w1.shape[0], w2.shape[0]
    T1, T2 = block_scales(w1, b1, w2, xb)
    x = np.asarray(x, np.float32).reshape(-1, OBS)
    R = x.shape[0]
    W1 = np.zeros((H, 16))                                    # K = 16: inputs 0..11, the constant 1 carrying b1, zeros
    W1[:, :OBS] = w1
    W1[:, OBS] = b1
    w1h, w1l = split_w(W1, T1)
    X = np.zeros((R, 16), np.float32)
    X[:, :OBS] = np.clip(x, -CAP, CAP)
    X[:, OBS] = 1.0
    xh, xl = split_v(X)
    z = _mfma(np.zeros((R, H)), xh, w1l.T)
    z = _mfma(z, xl, w1h.T)
    z = _mfma(z, xh, w1h.T)
    vh, vl = split_v(np.clip(z, 0.0, CAP).astype(np.float32))
    Hp = -(-H // 16) * 16                                     # padding units are zero in every plane
    pad = lambda a: np.pad(a, ((0, 0), (0, Hp - H)))
    vh, vl = pad(vh), pad(vl)
    w2h, w2l = (pad(p) for p in split_w(w2, T2))
    acc = np.zeros((R, A))
    for k in range(0, Hp, 16):
        s = slice(k, k + 16)
        acc = _mfma(acc, vh[:, s], w2l[:, s].T)
        acc = _mfma(acc, vl[:, s], w2h[:, s].T)
        acc = _mfma(acc, vh[:, s], w2h[:, s].T)
    inv = float(np.float32(1.0 / (T1 * T2)))
    logits = _r32(acc * inv + b2)                             # fmaf (the product by a power of two is exact)
    return dict(logits=logits, probs=softmax32(logits), m_row=magnitude(sd, x), T1=T1, T2=T2)


def softmax32(logits):
    """The kernel's softmax in fp32 (exp2 of the max-shifted logit times log2 e, one sum, one reciprocal), with exact exp2
    and reciprocal where the device has its approximate ones."""
    lg = np.asarray(logits, np.float32)
    l2e = np.float32(1.44269504088896340736)
    mneg = -lg.max(axis=1, keepdims=True) * l2e
    arg = _r32(lg.astype(np.float64) * l2e + mneg).astype(np.float32)
    with np.errstate(over="ignore"):
        ex = np.exp2(arg)
    S = ex.sum(axis=1, dtype=np.float32)
    redo = ~((S > 0) & (S < np.inf))                          # the max slot's residue over- or underflowed exp2
    ex[redo] = np.exp2(arg[redo] - arg[redo].max(axis=1, keepdims=True))
    S = np.zeros(lg.shape[0], np.float32)
    for q in range(lg.shape[1]):
        S = S + ex[:, q]
    return (ex * (np.float32(1.0) / S)[:, None]).astype(np.float64)


def magnitude(sd, x, hidden_cap=None):
    """m_row = max over actions of |W2| (|W1| |x| + |b1|) + |b2|, per row; hidden_cap bounds the hidden magnitudes."""
    w1, b1, w2, b2 = weights(sd)
    x = np.asarray(x, np.float64).reshape(-1, OBS)
    h = np.abs(x) @ np.abs(w1).T + np.abs(b1)
    if hidden_cap is not None:
        h = np.minimum(h, hidden_cap)
    return (h @ np.abs(w2).T + np.abs(b2)).max(axis=1)


def forward_fp64(sd, x, xb=None, capped=False):
    """FnnPolicyNet.forward in fp64 -> (logits, probs, m_row).  capped (needs xb): the forward of the saturating kernel --
    inputs clamped to +-60000, hidden values to 60000 / T1 -- and m_row of those clamped values."""
    w1, b1, w2, b2 = weights(sd)
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, OBS)
    hcap = None
    if capped:
        x = np.clip(x, -CAP, CAP)
        hcap = CAP / block_scales(w1, b1, w2, xb)[0]
    h = np.maximum(x @ w1.T + b1, 0.0)
    if hcap is not None:
        h = np.minimum(h, hcap)
    lg = h @ w2.T + b2
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return lg, e / e.sum(axis=1, keepdims=True), magnitude(sd, x, hcap)


def cap_reached(sd, x, xb, slack=1.0):
    """[R] True where the kernel may saturate: an input or a T1-scaled pre-activation at or beyond 60000 / slack."""
    w1, b1, w2, _ = weights(sd)
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, OBS)
    T1 = block_scales(w1, b1, w2, xb)[0]
    z = np.clip(x, -CAP, CAP) @ w1.T + b1
    return (np.abs(x) >= CAP / slack).any(axis=1) | (T1 * z >= CAP / slack).any(axis=1)


def chain_fp32_logits(sd, x):
    """The fp32 forward as fmaf chains (b1 + sum_k w1 x, ReLU, b2 + sum_u w2 h): the yardstick of the split."""
    w1, b1, w2, b2 = weights(sd)
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, OBS)
    z = np.broadcast_to(b1, (x.shape[0], b1.size)).copy()
    for k in range(OBS):
        z = _r32(x[:, k:k + 1] * w1[:, k] + z)
    h = np.maximum(z, 0.0)
    lg = np.broadcast_to(b2, (x.shape[0], b2.size)).copy()
    for u in range(w1.shape[0]):
        lg = _r32(h[:, u:u + 1] * w2[:, u] + lg)
    return lg


def rescale(sd, s1=1.0, s2=1.0, sb1=None):
    """W1 times s1, b1 times sb1 (default s1) and W2 times s2, as a new state dict of fp32 numpy arrays."""
    w1, b1, w2, b2 = weights(sd)
    f = lambda a: np.asarray(a, np.float32)
    return {"fc1.weight": f(w1 * s1), "fc1.bias": f(b1 * (s1 if sb1 is None else sb1)), "fc2.weight": f(w2 * s2),
            "fc2.bias": f(b2)}


def at_scale(sd, xb, t1=None, t2=None):
    """The network with the same fp64 logits (W1, b1 x 2^j and W2 x 2^-j, powers of two: ReLU is positively homogeneous)
    whose T1 -- or, given t2, T2 -- is 2^t1 (2^t2) before the clamp.  T1 T2 stays what it was, so the other scale may
    leave the clamp's range."""
    w1, b1, w2, _ = weights(sd)
    e1, e2 = exponents(w1, b1, w2, xb)
    j = (e1 - t1) if t1 is not None else (t2 - e2)            # T1 -> 2^(e1 - j), T2 -> 2^(e2 + j)
    return rescale(sd, 2.0 ** j, 2.0 ** -j)
