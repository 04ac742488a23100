"""Per-episode results without a GPU: the numpy mirror of uavtrack_episode_stats_* (tests/episode_stats_mirror.py)
against the reference's own arithmetic -- train.py:181-192 in plain Python floats -- on the per-step recordings in
tests/golden, the csv files against csv.writer, and the new structures and symbols of the ABI."""
import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
import episode_stats_mirror as mirror
from uavtrack import _lib
from uavtrack import episode_stats as es

CASES = ["g1_n5m3_raw", "g2_n20m10_raw", "g3_n20m10_mean", "g5a_n50m25_raw"]


def reference_episode(reward, terms, covered):
    """train.operate_epoch's accumulation (train.py:154-158, 181-192) on one episode's per-step lists, Python floats.
    reward [T][N], terms [T][3][N], covered [T] -> the six results, and sum |x| of each of the four sums."""
    num_steps, n_uav = len(reward), len(reward[0])
    episode = [0, 0, 0, 0]
    mags = [0.0, 0.0, 0.0, 0.0]
    covered_targets_list = []
    for i in range(num_steps):
        lists = [reward[i], terms[i][0], terms[i][1], terms[i][2]]
        for p in range(4):
            episode[p] += sum(lists[p])                     # train.py:181-184
            mags[p] += sum(abs(v) for v in lists[p])
        covered_targets_list.append(covered[i])             # train.py:185
    out = [v / (num_steps * n_uav) for v in episode]        # train.py:187-190
    out += [np.mean(covered_targets_list), np.max(covered_targets_list)]   # train.py:191-192
    return out, mags


def golden_fp32(name):
    z, _ = load_golden(name)
    return (z["reward"].astype(np.float32), z["terms"].astype(np.float32), z["covered"].astype(np.int32))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("form", ["done", "close"])
def test_mirror_matches_reference_arithmetic(name, form):
    """The mirror, fed the fp32 casts a launch would hand it, against the reference formulas on the same numbers.
    form "done": one environment plays the E recorded episodes back to back, in adds of uneven length, each closed by
    its done flag.  form "close": the E episodes are E environments of one add, ended by close()."""
    reward, terms, covered = golden_fp32(name)
    E, T, N = reward.shape
    if form == "done":
        m = mirror.EpisodeStatsMirror(1, N, log_capacity=E, env_offset=7)
        flat_r = reward.reshape(E * T, 1, N)
        flat_t = terms.reshape(E * T, 3, 1, N)
        flat_c = covered.reshape(E * T, 1)
        done = np.zeros((E * T, 1), np.uint8)
        done[T - 1::T] = 1
        cuts = [0] + [c for c in (3, T - 1, T, T + 1, 2 * T + 5) if c < E * T] + [E * T]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if b > a:
                m.add(flat_r[a:b], flat_t[a:b], flat_c[a:b], done[a:b])
        want_env, want_ord = [7] * E, list(range(E))
    else:
        m = mirror.EpisodeStatsMirror(E, N, log_capacity=E, env_offset=7)
        m.add(reward.transpose(1, 0, 2), terms.transpose(1, 2, 0, 3), covered.T, None)
        assert len(m.records()) == 0                        # nothing closes without done
        m.close()
        want_env, want_ord = [7 + e for e in range(E)], [0] * E
    rec = m.records()
    assert len(rec) == E and m.dropped == 0
    assert rec["env"].tolist() == want_env and rec["ordinal"].tolist() == want_ord       # the record order, exactly
    assert rec["steps"].tolist() == [T] * E
    for e in range(E):
        ref, mags = reference_episode([[float(v) for v in row] for row in reward[e]],
                                      [[[float(v) for v in pl] for pl in st] for st in terms[e]],
                                      [int(c) for c in covered[e]])
        n = T * N
        for p, f in enumerate(mirror.FIELDS):
            bound = (n - 1) * 2.0 ** -53 * mags[p] / (T * N)          # an n-term recursive fp64 sum, then the division
            print(f"{name} {form} episode {e} {f}: mirror {rec[f][e]!r} reference {ref[p]!r} bound {bound:.3e}")
            assert abs(rec[f][e] - ref[p]) <= bound, (name, e, f, rec[f][e], ref[p], bound)
        assert rec["average_covered"][e] == ref[4]
        assert rec["max_covered"][e] == ref[5]


def test_mirror_overflow_counts_and_restarts():
    """log_capacity 2, five closing episodes: two kept in (t, b) order, three counted, the accumulators restarted."""
    r = np.random.RandomState(0)
    B, N, T = 3, 4, 4
    reward = r.randn(T, B, N).astype(np.float32)
    terms = r.randn(T, 3, B, N).astype(np.float32)
    covered = r.randint(0, 9, (T, B)).astype(np.int32)
    done = np.array([[0, 1, 0], [1, 0, 0], [0, 1, 1], [1, 0, 0]], np.uint8)
    m = mirror.EpisodeStatsMirror(B, N, log_capacity=2)
    m.add(reward, terms, covered, done)
    rec = m.records()
    assert rec["env"].tolist() == [1, 0] and rec["steps"].tolist() == [1, 2] and m.dropped == 3
    assert m.ordinal.tolist() == [2, 2, 1] and m.steps.tolist() == [0, 1, 1]
    m.clear()
    m.close()
    rec = m.records()
    assert rec["env"].tolist() == [1, 2] and rec["ordinal"].tolist() == [2, 1] and m.dropped == 0


@pytest.mark.parametrize("extra", [False, True])
def test_save_csv_bytes(tmp_path, extra):
    """The files of data_util.save_csv: same names, the reference's header rows, one csv.writer row per Python float."""
    reward, terms, covered = golden_fp32("g2_n20m10_raw")
    E, T, N = reward.shape
    m = mirror.EpisodeStatsMirror(E, N, log_capacity=E)
    m.add(reward.transpose(1, 0, 2), terms.transpose(1, 2, 0, 3), covered.T, None)
    m.close()
    res = es.results_from_records(m.records(), m.dropped)
    es.save_csv(res, str(tmp_path), extra=extra)
    headers = {"return_list": "Reward", "target_tracking_return_list": "target_tracking",
               "boundary_punishment_return_list": "boundary_punishment",
               "duplicate_tracking_punishment_return_list": "duplicate_tracking_punishment"}
    if extra:
        headers.update(average_covered_targets_list="average_covered_targets", max_covered_targets_list="max_covered_targets")
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".csv" for k in headers)
    field = dict(es.RESULT_KEYS)
    for key, head in headers.items():
        buf = io.StringIO(newline="")
        w = csv.writer(buf)
        w.writerow([head])
        for v in m.records()[field[key]]:
            w.writerow([float(v)])
        with open(os.path.join(tmp_path, key + ".csv"), "rb") as f:
            assert f.read() == buf.getvalue().encode()


def test_record_and_config_layout():
    assert C.sizeof(_lib.EpisodeRecord) == 64
    assert mirror.RECORD_DTYPE.itemsize == 64 and es.RECORD_DTYPE == mirror.RECORD_DTYPE
    offs = {n: getattr(_lib.EpisodeRecord, n).offset for n, _ in _lib.EpisodeRecord._fields_}
    assert offs == {n: mirror.RECORD_DTYPE.fields[n][1] for n in mirror.RECORD_DTYPE.names}
    assert offs["env"] == 48 and offs["steps"] == 56 and offs["ordinal"] == 60
    # uint32 + int32, int64, int32 + int32 pad, 3 x int64
    assert C.sizeof(_lib.EpisodeStatsConfig) == 8 + 8 + 8 + 3 * 8
    assert _lib.EpisodeStatsConfig.n_envs.offset == 8 and _lib.EpisodeStatsConfig.env_offset.offset == 24


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    declared = set(re.findall(r"\b(uavtrack_episode_stats_[a-z_]+)\s*\(", hdr))
    assert declared == {"uavtrack_episode_stats_" + k for k in ("create", "destroy", "add", "close", "read", "clear")}
    lib = _lib.load()
    for name in declared:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct uavtrack_episode_record" in hdr and "typedef struct uavtrack_episode_stats_config" in hdr
