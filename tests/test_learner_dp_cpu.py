"""The split learner update without a GPU: the float64 mirror of gradient rows and their ordered combine
(tests/learner_mirror.py's shard_sums and combine) against the whole-batch update, the rule it must not be mistaken for,
and the new entry points' declarations."""
import os
import re

import numpy as np
import pytest

import learner_harness as lh
import learner_mirror as mirror
from learner_autograd import rel as _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("loss", ["reference", "per_sample"])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_combined_shards_equal_the_whole_batch(K, loss):
    """A batch cut into K uneven shards, the shards' sums combined and one Adam step taken, is learner_mirror.update on
    the whole batch to 1e-12 relative: losses, gradient, parameters and both moments."""
    H, A, n, gamma, lrs = 33, 9, 1000, 0.95, (1e-3, 5e-3)
    rng = np.random.RandomState(K)
    b = lh.batch(rng, n, A)
    blob = lh.init_blob(H, A, 3)
    P = blob.size
    state = {"params": blob, "exp_avg": rng.randn(P) * 1e-3, "exp_avg_sq": rng.rand(P) * 1e-6, "step": np.full(8, 4)}
    pieces = lh.cuts(n, K)
    assert len(pieces) == K and len({hi - lo for lo, hi in pieces}) > 1
    rows = [mirror.shard_sums(blob, H, A, *sh, gamma, loss) for sh in lh.split(b, pieces)]
    got, al, cl = mirror.update_from_rows(state, rows, H, A, lrs, loss)
    want, wal, wcl, wtd = mirror.update(state, H, A, *b, gamma, lrs, loss)
    assert abs(al - wal) <= 1e-12 * abs(wal) and abs(cl - wcl) <= 1e-12 * abs(wcl)
    g = mirror.combine(rows, H, A, loss)[2]
    assert _rel(g, mirror.losses_and_grads(blob, H, A, *b, gamma, loss)[3]) <= 1e-12
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert _rel(got[k], want[k]) <= 1e-12, k
    assert np.array_equal(got["step"], want["step"])
    assert _rel(np.concatenate([r["td"] for r in rows]), wtd) <= 1e-12


@pytest.mark.parametrize("K", [2, 3, 8])
def test_averaging_shard_gradients_is_a_different_rule(K):
    """On the shared batch (rewards ramp across the rows) the average of the shards' own reference-loss gradients is
    further from the combined gradient than 100 x the bound the GPU test applies to the device's gradient, so a device
    path that averaged per-shard gradients could not pass it."""
    c = lh.TEETH
    blob, b = lh.teeth_batch()
    shards = lh.split(b, lh.cuts(c["n"], K))
    md = [mirror.shard_sums(blob, c["H"], c["A"], *sh, c["gamma"])["loss"][1] / len(sh[1]) for sh in shards]
    assert max(md) - min(md) > 1.0                                       # the shards' mean(delta) clearly differ
    g = mirror.combine([mirror.shard_sums(blob, c["H"], c["A"], *sh, c["gamma"]) for sh in shards], c["H"], c["A"])[2]
    assert _rel(g, mirror.losses_and_grads(blob, c["H"], c["A"], *b, c["gamma"])[3]) <= 1e-12
    naive = mirror.averaged_shard_gradients(blob, c["H"], c["A"], shards, c["gamma"])
    na = sum(mirror.layout(c["H"], c["A"])[0][:4])                       # the actor's part: where mean(delta) acts
    tol = lh.tol_g(c["n"], g)
    assert np.abs(naive[:na] - g[:na]).max() > 100 * tol, (np.abs(naive[:na] - g[:na]).max(), tol)


@pytest.mark.parametrize("H,A", [(1, 1), (64, 12), (128, 12), (200, 9), (256, 48)])
def test_row_floats_is_params_plus_tail(H, A):
    import uavtrack.learner as L
    P = sum(mirror.layout(H, A)[0])
    assert L.num_params(H, A) == P
    assert L.row_floats(H, A) == P + 8


def test_header_declares_the_split_entry_points():
    from uavtrack import _lib
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    for name in ("uavtrack_learner_row_floats", "uavtrack_learner_grad", "uavtrack_learner_apply",
                 "uavtrack_learner_write_priorities"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*uavtrack_learner\s*\*", hdr), name
        assert name in _lib.SIGNATURES, name
    m = re.search(r"#define\s+UAVTRACK_LEARNER_MAX_ROWS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.LEARNER_MAX_ROWS == 64
    lib = _lib.load()
    for name in ("uavtrack_learner_grad", "uavtrack_learner_apply", "uavtrack_learner_write_priorities"):
        assert hasattr(lib, name)
