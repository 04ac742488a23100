"""The PMI trainer over several shards and ranks on the MI355X (uavtrack_pmi_trainer_train_many / _select,
DevicePMINetwork.train_indices_many / train_pmi_many / train_pmi(group=...), broadcast_pmi_trainer): every claim is
bitwise equality with the existing single-history call on the concatenation, whose own arithmetic
tests/test_hip_pmi_trainer.py checks.  Shapes are the smallest at which the gather can go wrong: sources of (1, 5, 2)
timesteps of 3 UAVs (a source of one group, first and last groups of every span, both u extremes), b2 = 64 in four
mini-batches of 16, H = 16 (and 128 once); a reserve of one mini-batch (one scratch fill per step); a source whose
address is not 16-byte aligned (the gather's scalar form)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import pmi_dp_worker as worker
import pmi_select_mirror as sel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LR = 1e-3
N_UAV, B2, BS = 3, 64, 16
COUNTS = (1, 5, 2)


def _uav():
    import uavtrack
    return uavtrack


def _history(rng, groups, n_uav=N_UAV):
    x = rng.uniform(-1, 1, size=(groups * n_uav, 12)).astype(np.float32)
    x[:, 9:11] = rng.uniform(0, 5, size=(groups * n_uav, 2))
    return x


def _sources(counts, seed=0, unaligned=False):
    rng = np.random.RandomState(seed)
    out = []
    for g in counts:
        x = torch.from_numpy(_history(rng, g))
        if unaligned:                                  # one float behind an aligned address: contiguous, 4-byte aligned
            flat = torch.empty(x.numel() + 1, device=DEV)
            flat[1:] = x.reshape(-1).to(DEV)
            out.append(flat[1:].view(-1, 12))
            assert out[-1].data_ptr() % 16 == 4 and out[-1].is_contiguous()
        else:
            out.append(x.to(DEV))
    return out


def _triples(counts, b2=B2, seed=1, n_uav=N_UAV):
    """Every source's first and last group with both u extremes, then random draws: (t [b2], u [b2, 2]) on the device."""
    rng = np.random.RandomState(seed)
    base = sel.bases(counts)
    edges = np.unique(np.concatenate([base[:-1], base[1:] - 1]))
    assert len(edges) <= b2
    lead = np.repeat(edges, 2) if 2 * len(edges) <= b2 else edges
    t = np.concatenate([lead, rng.randint(0, base[-1], size=b2)])[:b2]
    u = rng.randint(0, n_uav, size=(b2, 2))
    u[0:len(lead):2], u[1:len(lead):2] = (0, n_uav - 1), (n_uav - 1, 0)
    perm = rng.permutation(b2)                          # the edge draws spread over the mini-batches
    return torch.from_numpy(t[perm].astype(np.int64)).to(DEV), torch.from_numpy(u[perm].astype(np.int64)).to(DEV)


def _pair(H, b2=B2, seed=3, max_batch=0):
    """Two trainers that start from one state dict."""
    torch.manual_seed(seed)
    sd = _uav().make_pmi_net(H).state_dict()
    out = []
    for _ in range(2):
        tr = _uav().DevicePMINetwork(H, b2, DEV, lr=LR, max_batch=max_batch)
        tr.load_state_dict(sd)
        out.append(tr)
    return out


def _full_state(tr):
    st, nbt = tr._get()
    m, v, steps = tr.optimizer_state()
    return st, nbt, m, v, steps


def _assert_same(a, b):
    for name, x, y in zip(("state", "num_batches_tracked", "exp_avg", "exp_avg_sq", "step"), _full_state(a), _full_state(b)):
        assert np.array_equal(x.view(np.int32 if x.dtype == np.float32 else x.dtype),
                              y.view(np.int32 if y.dtype == np.float32 else y.dtype)), name


def _bits(t):
    return t.cpu().contiguous().view(torch.int32).numpy()


def _run(tr, many, src, t, u, bs=BS, calls=2):
    nb = t.numel() // bs
    got = []
    for _ in range(calls):
        losses, outs = torch.empty(nb, device=DEV), torch.empty(nb, 2, bs, device=DEV)
        if many:
            avg = tr.train_indices_many(src, N_UAV, t, u, bs, losses=losses, outputs=outs)
        else:
            avg = tr.train_indices(torch.cat([s.reshape(-1, 12) for s in src]), N_UAV, t, u, bs, losses=losses, outputs=outs)
        got.append((_bits(avg.reshape(1)), _bits(losses), _bits(outs)))
    return got


@pytest.mark.parametrize("case", ["h16", "h128", "one_fill_per_step", "unaligned", "k1", "k64"])
def test_many_sources_equal_the_concatenation(case):
    """train_indices_many(sources) against train_indices(cat), two calls each: the full state, both moments, the step
    counts, num_batches_tracked, avg_loss, losses and outputs, bit for bit.  k1: one source (equals train_indices);
    k64: 64 sources of one group each."""
    counts = {"k1": (8,), "k64": (1,) * 64}.get(case, COUNTS)
    a, b = _pair(128 if case == "h128" else 16, max_batch=BS if case == "one_fill_per_step" else 0)
    src = _sources(counts, unaligned=case == "unaligned")
    t, u = _triples(counts)
    tt = t.cpu().numpy()
    for k, (lo, hi) in enumerate(zip(sel.bases(counts)[:-1], sel.bases(counts)[1:])):
        assert lo in tt and hi - 1 in tt, k                       # every source's first and last group is drawn
    got, want = _run(a, True, src, t, u), _run(b, False, src, t, u)
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            assert np.array_equal(x, y)
    assert np.isfinite(got[-1][1].view(np.float32)).all()
    _assert_same(a, b)
    assert np.array_equal(a.optimizer_state()[2], np.full(18, 2 * (B2 // BS)))
    a.check(); b.check()


def test_train_pmi_many_draws_and_trains_as_train_pmi_on_the_concatenation():
    """Under the same seeded generator, flat sources and [T, B_k, N, 12] sources with unequal B_k."""
    cfg = {"pmi": {"batch_size": BS}}
    rng = np.random.RandomState(5)
    shaped = [torch.from_numpy(_history(rng, 4 * bk).reshape(4, bk, N_UAV, 12)).to(DEV) for bk in (3, 1, 2)]
    for src in (_sources(COUNTS, seed=4), shaped):
        a, b = _pair(16)
        la = a.train_pmi_many(cfg, src, N_UAV, generator=torch.Generator().manual_seed(11))
        lb = b.train_pmi(cfg, torch.cat([s.reshape(-1, 12) for s in src]), N_UAV, generator=torch.Generator().manual_seed(11))
        assert la == lb and np.isfinite(la)
        _assert_same(a, b)
        a.check()
    torch.manual_seed(21)                                          # the global generator, as the reference draws
    la = a.train_pmi_many(cfg, shaped, N_UAV)
    torch.manual_seed(21)
    lb = b.train_pmi(cfg, torch.cat([s.reshape(-1, 12) for s in shaped]), N_UAV)
    assert la == lb
    _assert_same(a, b)
    dev_g = torch.Generator(device=DEV)
    dev_g.manual_seed(1)
    out = a.train_pmi_many(cfg, shaped, N_UAV, generator=dev_g, sync=False)
    assert out.device.type == "cuda" and np.isfinite(float(out))


def _raw_train_many(tr, table, count, t, u, avg, n_uav=N_UAV):
    return tr._lib.uavtrack_pmi_trainer_train_many(tr._h, table, count, n_uav, C.c_void_p(t.data_ptr()),
                                                   C.c_void_p(u.data_ptr()), t.numel(), BS, C.c_void_p(avg.data_ptr()),
                                                   None, None, tr._stream())


def test_bad_source_lists_are_refused_with_nothing_enqueued():
    from uavtrack import _lib
    tr, _ = _pair(16)
    before = _full_state(tr)
    src = _sources(COUNTS)
    t, u = _triples(COUNTS)
    avg = torch.full((), 5.0, device=DEV)
    one = _sources((1,))[0]

    def table(entries):
        tb = (_lib.PmiSource * len(entries))()
        for k, (p, n) in enumerate(entries):
            tb[k].rows, tb[k].n_rows = p, n
        return tb
    good = [(s.data_ptr(), s.shape[0]) for s in src]
    cases = {
        "65 sources": (table([(one.data_ptr(), N_UAV)] * 65), 65, r"count = 65 out of range \[1, 64\]"),
        "no source": (table(good), 0, r"count = 0 out of range"),
        "0 rows": (table(good[:1] + [(src[1].data_ptr(), 0)] + good[2:]), 3, r"sources\[1\]\.n_rows = 0 is not a positive multiple"),
        "not a multiple": (table(good[:2] + [(src[2].data_ptr(), 4)]), 3, r"sources\[2\]\.n_rows = 4 is not a positive multiple"),
        "null rows": (table([(None, 3)] + good[1:]), 3, r"sources\[0\]\.rows is null"),
    }
    for name, (tb, count, msg) in cases.items():
        rc = _raw_train_many(tr, tb, count, t, u, avg)
        assert rc != 0, name
        with pytest.raises(RuntimeError, match=msg):
            _lib.check(rc, "uavtrack_pmi_trainer_train_many")
    # what uavtrack_pmi_trainer_train refuses: batch_size 1, b2 < batch_size, a batch above the reserve
    for bs, tt, uu in ((1, t, u), (BS, t[:8].contiguous(), u[:8].contiguous()), (8192, t, u)):
        with pytest.raises(RuntimeError, match="uavtrack_pmi_trainer_train_many"):
            tr.train_indices_many(src, N_UAV, tt, uu, bs)
    # the Python layer's own tests of the list
    for bad in ([], [one] * 65, [one.double()], [one.cpu()], [one[:, :6]], [one.reshape(-1)[:24]]):
        with pytest.raises(ValueError):
            tr.train_indices_many(bad, N_UAV, t, u, BS)
    sel_buf = torch.zeros(B2, 2, 12, device=DEV)
    for base, total in ((-1, 8), (8, 8), (1, 8)):                 # the span [base, base + 8) must lie in [0, total)
        with pytest.raises(RuntimeError, match="uavtrack_pmi_trainer_select"):
            tr._select(src, base, total, N_UAV, t, u, sel_buf)
    torch.cuda.synchronize()
    assert float(avg) == 5.0 and not sel_buf.any()
    for x, y in zip(before, _full_state(tr)):
        assert np.array_equal(x, y)
    tr.check()                                                      # nothing ran, nothing was refused on the device


@pytest.mark.parametrize("which", ["t_total", "t_negative", "u_high"])
def test_out_of_range_draw_is_a_device_side_noop(which):
    tr, _ = _pair(16)
    tr.check()
    before = _full_state(tr)
    src = _sources(COUNTS)
    t, u = _triples(COUNTS)
    if which == "t_total":
        t[50] = sum(COUNTS)
    elif which == "t_negative":
        t[3] = -1
    else:
        u[63, 1] = N_UAV
    losses = torch.zeros(B2 // BS, device=DEV)
    avg = tr.train_indices_many(src, N_UAV, t, u, BS, losses=losses)
    assert np.isnan(float(avg)) and torch.isnan(losses).all()
    for x, y in zip(before, _full_state(tr)):
        assert np.array_equal(x, y)
    with pytest.raises(RuntimeError, match="refused"):
        tr.check()
    tr.check()                                                      # the count restarts
    # select refuses the same draws whole: nothing is written, one more refusal
    buf = torch.full((B2, 2, 12), 9.0, device=DEV)
    tr._select(src, 0, sum(COUNTS), N_UAV, t, u, buf)
    with pytest.raises(RuntimeError, match="1 train call"):
        tr.check()
    assert (buf == 9.0).all()
    good_t, good_u = _triples(COUNTS)
    assert np.isfinite(float(tr.train_indices_many(src, N_UAV, good_t, good_u, BS)))     # the next call works
    tr.check()


@pytest.mark.parametrize("unaligned", [False, True])
def test_select_writes_only_the_draws_of_its_span(unaligned):
    tr, _ = _pair(16)
    src = _sources(COUNTS, seed=8, unaligned=unaligned)
    t, u = _triples(COUNTS)
    cat = torch.cat(src)
    want = cat[(t[:, None] * N_UAV + u)]                            # [b2, 2, 12]
    total = sum(COUNTS)
    buf = torch.full((B2, 2, 12), -7.0, device=DEV)
    tr._select(src[1:], COUNTS[0], total, N_UAV, t, u, buf)         # groups [1, 8)
    inside = t >= COUNTS[0]
    assert inside.any() and (~inside).any()
    assert (buf[~inside] == -7.0).all() and torch.equal(buf[inside], want[inside])
    tr._select(src[:1], 0, total, N_UAV, t, u, buf)                 # the other span: the union is every draw
    assert torch.equal(buf, want)
    mid = torch.full((B2, 2, 12), -7.0, device=DEV)
    tr._select(src[1:2], COUNTS[0], total, N_UAV, t, u, mid)        # a span with timeline on both sides
    inside = (t >= 1) & (t < 6)
    assert (mid[~inside] == -7.0).all() and torch.equal(mid[inside], want[inside])
    tr.check()


def test_graph_capture_replays_as_eager_calls():
    eager, graphed = _pair(16)
    src = _sources(COUNTS, seed=9)
    t, u = _triples(COUNTS)
    e = [float(eager.train_indices_many(src, N_UAV, t, u, BS)) for _ in range(2)]
    avg, losses = torch.empty((), device=DEV), torch.empty(B2 // BS, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            graphed.train_indices_many(src, N_UAV, t, u, BS, avg_loss=avg, losses=losses)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(graphed.optimizer_state()[2], np.zeros(18))     # capture ran nothing
    got = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        got.append(float(avg))
    assert got == e
    _assert_same(graphed, eager)
    graphed.check()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_processes_stay_bitwise_equal(backend, tmp_path):
    """Two fresh child processes (tests/pmi_dp_worker.py), each with its own history: broadcast_pmi_trainer, then two
    train_pmi(group=...).  Both ranks bitwise equal each other and one process training on the concatenated history
    with the triples rank 0 drew."""
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("the nccl leg needs two GPUs")
    port = _free_port()
    script = os.path.join(ROOT, "tests", "pmi_dp_worker.py")
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", str(port), backend, str(tmp_path)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs, failed = [], False
    for p in procs:
        try:
            if failed:
                p.kill()
            outs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            failed = True
            p.kill()
            outs.append(p.communicate()[0])
        failed = failed or p.returncode != 0
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[-3000:] for o in outs)
    z = [dict(np.load(str(tmp_path / f"rank{r}.npz"))) for r in range(2)]
    # the single-process side: rank 0's start state, the concatenated history, rank 0's generator
    tr = worker.trainer_for(7, DEV)
    worker.warm_up(tr, 0, DEV)
    rows = torch.from_numpy(np.concatenate([worker.history(r) for r in range(2)])).to(DEV)
    gen = torch.Generator().manual_seed(worker.DRAW_SEED)
    one = worker.blobs(tr, [tr.train_pmi(worker.CONFIG, rows, worker.N_UAV, generator=gen) for _ in range(worker.CALLS)])
    tr.check()
    steps = (1 + worker.CALLS) * (worker.B2 // worker.BS)
    assert np.array_equal(one["step"], np.full(18, steps)) and np.array_equal(one["nbt"], np.full(4, 2 * steps))
    assert np.isfinite(one["losses"]).all()
    for r in range(2):
        assert one.keys() == z[r].keys()
        for k in one:
            assert np.array_equal(one[k].view(np.int32 if one[k].dtype == np.float32 else one[k].dtype),
                                  z[r][k].view(np.int32 if z[r][k].dtype == np.float32 else z[r][k].dtype)), (r, k)


def _example(args, capsys):
    if os.path.join(ROOT, "examples") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_maac
    hist = train_maac.main(args)
    return hist, [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]


SHARDED = ["--shards", "2", "--learner", "device", "--replay", "prioritized", "--publish", "device", "--envs", "64",
           "--steps", "20", "--iters", "3"]


def test_example_trains_maac_r_from_two_shards(capsys):
    hist, lines = _example(SHARDED + ["--method", "maac-r", "--pmi-trainer", "device"], capsys)
    assert len(hist) == 3 and np.isfinite(hist).all()
    assert len(lines) == 3 and all("shards 2" in ln for ln in lines)
    assert all(np.isfinite(float(ln.split("pmi loss")[1].split()[0])) for ln in lines)


# The history of SHARDED + ["--method", "maac"] as the commit before train_pmi_many printed it on an MI355X, every
# value an fp32 mean widened to a Python float (so each has an exact hex form):
#   iter 0  -0.585310697555542   (-0x1.2badd8p-1)
#   iter 1  -0.6093887090682983  (-0x1.3801ccp-1)
#   iter 2  -0.562912106513977   (-0x1.203604p-1)
# The run is a function of its arguments alone (seeded resets, seeded rings, ordered applies), so equality is asked.
MAAC_SHARDS_BEFORE = [float.fromhex("-0x1.2badd8p-1"), float.fromhex("-0x1.3801ccp-1"), float.fromhex("-0x1.203604p-1")]


def test_example_maac_shards_are_as_before(capsys):
    """--shards 2 --method maac takes no new branch: its history equals, to the bit, the three values recorded from the
    commit before this feature (MAAC_SHARDS_BEFORE), its printed lines carry no new field, and a second run agrees."""
    hist, lines = _example(SHARDED + ["--method", "maac"], capsys)
    assert hist == MAAC_SHARDS_BEFORE, [float.hex(h) for h in hist]
    assert len(lines) == 3 and all("shards 2" in ln for ln in lines) and not any("pmi loss" in ln for ln in lines)
    again, _ = _example(SHARDED + ["--method", "maac"], capsys)
    assert again == hist


def test_example_torch_pmi_trainer_with_shards_names_the_flag(capsys):
    with pytest.raises(SystemExit):
        _example(SHARDED + ["--method", "maac-r"], capsys)
    assert "--pmi-trainer device" in capsys.readouterr().err
