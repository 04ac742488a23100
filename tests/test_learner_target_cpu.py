"""The target critic without a GPU: the float64 mirror with theta- = the critic is the mirror without a target; the float32
Polyak rule at tau = 1 returns the critic's bits; DeviceActorCritic.set_target refuses bad arguments before any library
call (on tests/learner_call_trace.py's handle-less learner, whose library is a recorder); and
sharding.pack_learner_state / unpack_learner_state round-trip on a stub learner."""
import numpy as np
import pytest

import learner_call_trace as lt
import learner_harness as lh
import learner_mirror as mirror
from uavtrack import sharding


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("H,A,n", [(1, 9, 1), (33, 12, 65)])
def test_mirror_with_the_critic_as_target_is_the_plain_mirror(H, A, n, loss):
    rng = np.random.RandomState(H + n)
    blob = lh.init_blob(H, A, 3).astype(np.float64)
    s, a, r, s2 = lh.batch(rng, n, A)
    P = blob.size
    state = {"params": blob, "exp_avg": rng.standard_normal(P) * 1e-3, "exp_avg_sq": rng.uniform(0, 1e-4, P),
             "step": np.arange(8, dtype=np.int64)}
    want, wal, wcl, wtd = mirror.update(state, H, A, s, a, r, s2, 0.95, (1e-3, 5e-3), loss)
    got, al, cl, td = mirror.update(state, H, A, s, a, r, s2, 0.95, (1e-3, 5e-3), loss, theta=mirror.critic_block(blob, H, A))
    for k in ("params", "exp_avg", "exp_avg_sq"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12)
    assert np.array_equal(got["step"], want["step"])
    np.testing.assert_allclose(td, wtd, rtol=0, atol=1e-12)
    assert abs(al - wal) <= 1e-12 and abs(cl - wcl) <= 1e-12
    # and another target gives another update
    other = mirror.critic_block(lh.init_blob(H, A, 4), H, A)
    assert np.abs(mirror.update(state, H, A, s, a, r, s2, 0.95, (1e-3, 5e-3), loss, theta=other)[3] - wtd).max() > 1e-6


def test_polyak_at_tau_one_returns_the_critics_bits_and_each_operation_rounds_on_its_own():
    rng = np.random.RandomState(0)
    w = np.concatenate([rng.standard_normal(64), [1e-45, -1e-45, 1e-39, -3e-41, 3.4e38, -3.4e38, 1.0, 0.0]]).astype(np.float32)
    for t in (np.zeros_like(w), -np.zeros_like(w), np.full_like(w, 1e-45), np.full_like(w, -7e-40),
              rng.standard_normal(w.size).astype(np.float32)):
        got = mirror.polyak(t, w, 1.0)
        assert got.dtype == np.float32 and got.tobytes() == w.tobytes()
    assert mirror.periodic(np.zeros_like(w), w, 6, 3).tobytes() == w.tobytes()
    assert mirror.periodic(np.zeros_like(w), w, 7, 3).tobytes() == np.zeros_like(w).tobytes()
    # tau = 0.3: the separately rounded form, which the fused and the float64 forms both miss somewhere
    t = rng.standard_normal(4096).astype(np.float32)
    w = rng.standard_normal(4096).astype(np.float32)
    tau32 = np.float32(0.3)
    omt = np.float32(1.0) - tau32
    got = mirror.polyak(t, w, 0.3)
    assert got.tobytes() == ((omt * t).astype(np.float32) + (tau32 * w).astype(np.float32)).astype(np.float32).tobytes()
    wide = (np.float64(omt) * t + np.float64(tau32) * w).astype(np.float32)
    assert (got != wide).any()


@pytest.mark.parametrize("kw,word", [(dict(tau=0.1, period=3), "not both"), (dict(tau=0.0), "tau"), (dict(tau=-0.5), "tau"),
                                     (dict(tau=1.5), "tau"), (dict(tau=float("nan")), "tau"), (dict(period=0), "period"),
                                     (dict(period=-2), "period"), (dict(period=2.5), "period"), (dict(period=True), "period")])
def test_set_target_refuses_bad_arguments_before_any_library_call(kw, word):
    lt.REC.calls, lt.REC.known, lt.REC.fresh, lt.REC.dump = [], {}, [], False
    L = lt.Learner()
    with pytest.raises(ValueError, match=word):
        L.set_target(**kw)
    assert lt.REC.calls == []


def test_set_target_is_one_library_call_with_the_mode_it_names():
    lt.REC.calls, lt.REC.known, lt.REC.fresh, lt.REC.dump = [], {}, [], False
    L = lt.Learner()
    L.set_target(tau=0.25)
    L.set_target(period=7)
    L.set_target()
    assert lt.REC.calls == ["uavtrack_learner_set_target(learner, 1, 0.25, 0, None)",
                            "uavtrack_learner_set_target(learner, 2, 0.0, 7, None)",
                            "uavtrack_learner_set_target(learner, 0, 0.0, 0, None)"]


class _Stub:
    """The state pack_learner_state reads and unpack_learner_state writes, on the host."""

    def __init__(self, H, A, seed, target):
        rng = np.random.RandomState(seed)
        self.hidden_dim, self.num_params = H, 27 * H + A * H + A + 1
        P = self.num_params
        self.params = rng.standard_normal(P).astype(np.float32)
        self.m, self.v = rng.standard_normal(P).astype(np.float32), rng.uniform(0, 1, P).astype(np.float32)
        self.steps = rng.randint(0, 2 ** 40, 8).astype(np.int64)
        self.reg = (float(rng.uniform()), float("inf"), float(rng.uniform(1, 2)))
        self.tgt = dict(target)
        self.theta = rng.standard_normal(14 * H + 1).astype(np.float32)
        self.theta[0] = -0.0

    def _on(self):
        return self.tgt["tau"] is not None or self.tgt["period"] is not None

    def _get_params(self): return self.params.copy()
    def _optim_state(self): return self.m.copy(), self.v.copy(), self.steps.copy()
    def get_regularisation(self): return self.reg
    def get_target(self): return dict(self.tgt)

    def _get_target_params(self):
        assert self._on()
        return self.theta.copy()

    def _set_params(self, p): self.params = np.array(p, np.float32)
    def _set_optim_state(self, m, v, s): self.m, self.v, self.steps = np.array(m), np.array(v), np.array(s)
    def set_regularisation(self, c, mgn): self.reg = (c, *mgn)

    def set_target(self, tau=None, period=None):
        assert tau is None or period is None
        self.tgt = {"tau": tau, "period": period}

    def _set_target_params(self, t):
        assert self._on()
        self.theta = np.array(t, np.float32)

    def fields(self):
        return {"params": self.params, "m": self.m, "v": self.v, "steps": self.steps, "reg": np.array(self.reg),
                "theta": self.theta if self._on() else None}


@pytest.mark.parametrize("target", [{"tau": None, "period": None}, {"tau": 0.005, "period": None}, {"tau": 1.0, "period": None},
                                    {"tau": None, "period": 3}])
def test_pack_and_unpack_learner_state_round_trip(target):
    H, A = 5, 3
    src = _Stub(H, A, 1, target)
    for other in ({"tau": None, "period": None}, {"tau": 0.5, "period": None}):
        dst = _Stub(H, A, 2, other)
        blk = sharding.pack_learner_state(src)
        assert blk.dtype == np.int32 and blk.size == 3 * src.num_params + 16 + 6 + 4 + 14 * H + 1   # shapes alone
        sharding.unpack_learner_state(dst, blk)
        assert dst.get_target() == src.get_target()
        a, b = src.fields(), dst.fields()
        for k in a:
            assert (a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        assert sharding.pack_learner_state(dst).tobytes() == blk.tobytes()
    with pytest.raises(ValueError, match="block"):
        sharding.unpack_learner_state(_Stub(H + 1, A, 3, target), blk)
