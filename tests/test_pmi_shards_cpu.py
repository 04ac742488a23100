"""The PMI trainer over several shards and ranks, without a GPU: the source-table select equals indexing the
concatenation (tests/pmi_select_mirror.py), the per-rank selected buffers recompose to the same rows through
t' = owner * b2 + i (mirror and uavtrack.sharding._pmi_owner_triples alike), gather_pmi_selected moves every bit under a
2-rank gloo group, and the two new symbols are declared in include/uavtrack.h and bound in uavtrack/_lib.py with the
header's argument lists."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pmi_select_mirror as sel
from uavtrack import _lib
from uavtrack.sharding import _pmi_owner_triples, gather_pmi_selected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_UAV = 3
COUNTS = [(1, 5, 2), (3,), (1,) * 64]


def _sources(rng, counts, n_uav=N_UAV):
    return [rng.standard_normal((g * n_uav, 12)).astype(np.float32) for g in counts]


def _draws(rng, counts, n_uav=N_UAV, extra=40):
    """The first and last group of every source, both u extremes, then random draws."""
    base = sel.bases(counts)
    t = np.concatenate([base[:-1], base[1:] - 1, rng.integers(0, base[-1], extra)]).astype(np.int64)
    u = rng.integers(0, n_uav, (len(t), 2)).astype(np.int64)
    u[0], u[1 % len(t)] = (0, n_uav - 1), (n_uav - 1, 0)
    return t, u


@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: f"{len(c)}src")
def test_select_through_the_table_is_indexing_the_concatenation(counts):
    rng = np.random.default_rng(len(counts))
    src = _sources(rng, counts)
    t, u = _draws(rng, counts)
    cat = np.concatenate(src)
    got = np.full((len(t), 2, 12), np.nan, np.float32)
    assert sel.select(src, N_UAV, t, u, got)
    want = cat[(t[:, None] * N_UAV + u)]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    base = sel.bases(counts)
    for k in range(len(counts)):                     # locate at both edges of every span
        assert sel.locate(base, base[k]) == k and sel.locate(base, base[k + 1] - 1) == k


def test_select_span_writes_only_its_own_draws_and_refuses_whole_calls():
    rng = np.random.default_rng(7)
    counts = (1, 5, 2)
    src = _sources(rng, counts)
    t, u = _draws(rng, counts)
    cat = np.concatenate(src)
    total = sum(counts)
    got = np.full((len(t), 2, 12), 7.0, np.float32)
    assert sel.select(src[1:], N_UAV, t, u, got, group_base=1, total_groups=total)      # groups [1, 8)
    inside = t >= 1
    assert inside.any() and (~inside).any()
    assert (got[~inside] == 7.0).all()
    assert np.array_equal(got[inside], cat[(t[:, None] * N_UAV + u)][inside])
    assert sel.select(src[:1], N_UAV, t, u, got, group_base=0, total_groups=total)      # the union: every draw
    assert np.array_equal(got, cat[(t[:, None] * N_UAV + u)])
    for bad_t, bad_u in ((total, 0), (-1, 0), (0, N_UAV)):
        t2, u2 = t.copy(), u.copy()
        t2[5], u2[9, 1] = bad_t, bad_u
        keep = np.full_like(got, 3.0)
        assert not sel.select(src, N_UAV, t2, u2, keep) and (keep == 3.0).all()


@pytest.mark.parametrize("counts", [(8,), (5, 3), (2, 5, 1), (4, 1, 3)], ids=str)
def test_rank_recomposition_returns_the_selected_rows(counts):
    """R = 1, 2, 3 with uneven counts; in the last case no draw falls into rank 1's single group."""
    rng = np.random.default_rng(sum(counts) + len(counts))
    hist = _sources(rng, counts)
    t, u = _draws(rng, counts)
    if counts == (4, 1, 3):
        t[t == 4] = 0                                                   # rank 1 owns nothing
    cat, total, b2 = np.concatenate(hist), sum(counts), len(t)
    base = sel.bases(counts)
    blocks = []
    for r, h in enumerate(hist):
        mine = np.zeros((b2, 2, 12), np.float32)
        assert sel.select([h], N_UAV, t, u, mine, group_base=int(base[r]), total_groups=total)
        blocks.append(mine)
    if counts == (4, 1, 3):
        assert not blocks[1].any()
    got, t2 = sel.recompose(blocks, counts, t)
    assert np.array_equal(got, cat[(t[:, None] * N_UAV + u)])
    # the library's own recomposition triples are the mirror's
    lt, lu = _pmi_owner_triples(torch.from_numpy(t), torch.from_numpy(u), list(counts), N_UAV)
    assert np.array_equal(lt.numpy(), t2) and lt.dtype == torch.int64
    for bad_t, bad_u in ((total, 0), (-1, 0), (0, N_UAV), (0, -1)):   # one bad draw refuses the whole call: every t' is -1
        tb, ub = t.copy(), u.copy()
        tb[3], ub[5, 1] = bad_t, bad_u
        bt, _ = _pmi_owner_triples(torch.from_numpy(tb), torch.from_numpy(ub), list(counts), N_UAV)
        assert (bt == -1).all()
    assert np.array_equal(lu.numpy(), np.tile([0, 1], (b2, 1))) and lu.is_contiguous()
    assert np.array_equal(sel.owner(counts, t), np.searchsorted(base[1:], t, side="right"))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _block(rank, b2=6):
    """A selected buffer with NaN payloads and -0.0 among ordinary values, as int32 bits."""
    bits = np.random.default_rng(20 + rank).integers(-2 ** 31, 2 ** 31, (b2, 2, 12), dtype=np.int64).astype(np.int32)
    bits[0, 0, :4] = np.array([0x7FC00001, 0x7F800123, -0x7FFFFF, -2 ** 31], dtype=np.int64).astype(np.int32)
    return bits                                                         # quiet and signalling NaN, -NaN payload, -0.0


def _gather_worker(rank, world, port, q):
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd"), os.path.join(ROOT, "tests")]
    from uavtrack.sharding import gather_pmi_selected as gather
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = torch.from_numpy(_block(rank)).view(torch.float32)
    out = gather(mine, dist.group.WORLD)
    assert out.dtype == torch.float32 and tuple(out.shape) == (world * 6, 2, 12)
    q.put((rank, out.view(torch.int32).numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_pmi_selected_is_rank_major_and_bit_preserving():
    one = torch.from_numpy(_block(0)).view(torch.float32)
    assert gather_pmi_selected(one) is one                              # no process group: the input itself
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.concatenate([_block(0), _block(1)])
    for r in range(2):
        assert np.array_equal(got[r], want), r


ARGS = {
    "uavtrack_pmi_trainer_train_many": "trainer sources count n_uav t_idx u_idx b2 batch_size avg_loss losses outputs stream",
    "uavtrack_pmi_trainer_select": "trainer sources count group_base total_groups n_uav t_idx u_idx b2 selected stream",
}
CTYPE = {"uavtrack_pmi_trainer *": C.c_void_p, "const uavtrack_pmi_source *": C.POINTER(_lib.PmiSource),
         "int32_t": C.c_int32, "int64_t": C.c_int64, "const int64_t *": C.c_void_p, "float *": C.c_void_p,
         "void *": C.c_void_p}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_symbols_are_declared_and_bound_with_the_headers_argument_lists(name):
    hdr = open(os.path.join(ROOT, "include", "uavtrack.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/uavtrack.h"
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", a).group(1) for a in decl]
    assert names == ARGS[name].split()
    types = [a[:-len(n)].strip() for a, n in zip(decl, names)]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [CTYPE[t] for t in types]
    # the source struct and its limit
    s = re.search(r"typedef struct uavtrack_pmi_source \{(.*?)\} uavtrack_pmi_source;", hdr, re.S).group(1)
    assert re.findall(r"(\w+);", s) == [f[0] for f in _lib.PmiSource._fields_] == ["rows", "n_rows"]
    assert C.sizeof(_lib.PmiSource) == 16
    assert int(re.search(r"#define UAVTRACK_PMI_MAX_SOURCES (\d+)", hdr).group(1)) == _lib.PMI_MAX_SOURCES == 64
    assert re.search(r"#define UAVTRACK_ABI_VERSION\s+1\b", hdr)
