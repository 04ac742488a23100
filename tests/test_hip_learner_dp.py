"""The split learner update on the MI355X (uavtrack_learner_grad / _apply / _write_priorities and what
uavtrack.DeviceActorCritic builds on them): one row is bit for bit the closed update; K rows give the same bits on every
participant and on one accumulating handle, and sit inside the single-update bounds of the fp64 mirror; a refusal is
global; host-side errors enqueue nothing; the chain captures into a graph; two processes on one GPU stay bitwise equal.

"Bitwise" below is np.array_equal on parameters, both Adam moments, the step counts, losses, td_delta and priorities."""
import ctypes as C
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import learner_dp_worker as worker
import learner_harness as lh
import learner_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = lh.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _uav():
    import uavtrack
    return uavtrack


def _store(s, a, r, s2):
    return {k: lh.dev(x) for k, x in zip(lh.STORES, (s, a, r, s2))}


def _prio_target(prio, cap):
    """What write_priorities needs of a buffer."""
    return types.SimpleNamespace(priorities=prio, capacity=cap)


# ---- 1. one row is today's update ------------------------------------------------------------------------------------

# test_sweep_against_fp64_mirror's grid at H 64 / 128 / 200 / 256: n = 1 and 63 below one tile (H 64: 64 rows), 65 and 63
# not a multiple of it (H 128: 32, H 256: 16), 65537 rows at H 256 needing all 256 workgroups (4097 tiles), A 9 / 12 /
# 48, both losses, with and without an index vector (drawn with replacement: repeated slots)
GRID = [c for c in lh.SWEEP if c[0] in (64, 128, 200, 256)]


def test_grid_covers_what_it_must():
    assert {c[0] for c in GRID} >= {64, 128, 256} and {c[1] for c in GRID} >= {12, 48}
    assert {c[3] for c in GRID} == {"reference", "per_sample"} and {c[4] for c in GRID} == {True, False}
    assert (256, 48, 65537) in {c[:3] for c in GRID} and (64, 48, 63) in {c[:3] for c in GRID}
    assert (128, 9, 65) in {c[:3] for c in GRID}


@pytest.mark.parametrize("H,A,n,loss,gather", GRID)
def test_one_row_is_the_closed_update(H, A, n, loss, gather):
    """grad -> apply(count 1) -> write_priorities against update on a twin handle, three consecutive updates: bitwise."""
    rng = np.random.RandomState(H * 1000 + n)
    cap = n + 7 if gather else n
    store = _store(*lh.batch(rng, cap, A))
    blob = lh.init_blob(H, A, H + n)
    closed, split = (lh.learner(H, A, loss=loss, blob=blob, max_batch=n) for _ in range(2))
    prio_c = torch.from_numpy(rng.uniform(0.1, 2, cap).astype(np.float32)).to(DEV)
    prio_s = prio_c.clone()
    for u in range(3):
        idx = torch.from_numpy(rng.randint(0, cap, size=n).astype(np.int64)).to(DEV) if gather else None
        if gather and n > 1:
            idx[n // 2] = idx[0]                                          # at least one repeated slot
        al, cl, td = closed._run(n, store, cap, idx, prio_c)
        row, td2 = split._grad(n, store, cap, idx)
        al2, cl2 = split.apply(row)
        split.write_priorities(_prio_target(prio_s, cap), idx, td2)
        assert torch.equal(al, al2) and torch.equal(cl, cl2), u
        assert torch.equal(td, td2) and torch.equal(prio_c, prio_s), u
        tail = row[-8:].view(torch.int32).cpu().numpy()
        assert tail[4] == n and tail[5] == 0 and tail[6] == 0 and tail[7] == closed.num_params
    closed.check(); split.check()
    lh.same(lh.state(closed), lh.state(split))
    assert np.array_equal(lh.state(split)["step"], np.full(8, 3))


# ---- 2, 3. K rows: data parallelism and accumulation ---------------------------------------------------------------

def _teeth():
    c = lh.TEETH
    blob, b = lh.teeth_batch()
    return c, blob, b


def _k_handles(K):
    """The shared batch cut K ways, one grad per shard on K handles that start equal, every handle applies all rows."""
    c, blob, b = _teeth()
    shards = lh.split(b, lh.cuts(c["n"], K))
    Ls = [lh.learner(c["H"], c["A"], lr=c["lrs"], gamma=c["gamma"], blob=blob, max_batch=c["n"]) for _ in range(K)]
    rows = Ls[0].new_rows(K)
    tds = []
    for k, (L, sh) in enumerate(zip(Ls, shards)):
        tds.append(L._grad(len(sh[1]), _store(*sh), len(sh[1]), None, rows[k])[1])
    losses = [L.apply(rows) for L in Ls]
    for L in Ls:
        L.check()
    out = [dict(lh.state(L), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy()) for L, (al, cl) in zip(Ls, losses)]
    return out, torch.cat(tds).cpu().numpy()


@pytest.mark.parametrize("K", [2, 3, 8])
def test_k_rows_same_bits_everywhere_and_inside_the_single_update_bounds(K):
    """All K handles bitwise equal; against the fp64 mirror on the WHOLE batch within the bounds
    tests/learner_harness.py applies to a single update."""
    c, blob, (s, a, r, s2) = _teeth()
    H, A, n, lr = c["H"], c["A"], c["n"], c["lrs"]
    out, td = _k_handles(K)
    for o in out[1:]:
        lh.same(out[0], o)
    ral, rcl, rtd, g = mirror.losses_and_grads(blob, H, A, s, a, r, s2, c["gamma"], "reference")[:4]
    lh.assert_losses_and_td(out[0]["actor_loss"], out[0]["critic_loss"], td, ral, rcl, rtd)
    lh.assert_step_from_zero(out[0], blob, g, n, H, A, lr=lr)
    # and the rule it must not be: the averaged per-shard gradients are far outside the same bound
    naive = mirror.averaged_shard_gradients(blob, H, A, lh.split((s, a, r, s2), lh.cuts(n, K)), c["gamma"])
    assert np.abs(out[0]["exp_avg"] / 0.1 - naive).max() > 50 * lh.tol_g(n, g)


@pytest.mark.parametrize("K", [2, 3, 8])
def test_accumulation_on_one_handle_and_update_from_many(K):
    """The same K grads issued on ONE handle into K slots, one apply: bitwise the K-handle result.  update_from_many over
    K rings: bitwise the explicit grad_from / apply / write_priorities calls on twin rings, and each ring's priorities
    are learner_mirror.last_wins on that ring's own draw."""
    c, blob, b = _teeth()
    shards = lh.split(b, lh.cuts(c["n"], K))
    want, want_td = _k_handles(K)
    L = lh.learner(c["H"], c["A"], lr=c["lrs"], gamma=c["gamma"], blob=blob, max_batch=c["n"])
    rows = L.new_rows(K)
    tds = [L._grad(len(sh[1]), _store(*sh), len(sh[1]), None, rows[k])[1] for k, sh in enumerate(shards)]
    al, cl = L.apply(rows)
    L.check()
    lh.same(dict(lh.state(L), actor_loss=al.cpu().numpy(), critic_loss=cl.cpu().numpy()), want[0])
    assert np.array_equal(torch.cat(tds).cpu().numpy(), want_td)

    def rings():
        out = []
        for k, sh in enumerate(shards):
            ring = _uav().PrioritizedReplayRing(len(sh[1]) + 5, DEV, seed=90 + k, max_batch=4096)
            ring.add({key: v.cpu() for key, v in _store(*sh).items()})
            ring.priorities[:len(sh[1])] = torch.from_numpy(
                np.random.RandomState(k).uniform(0.1, 2.0, len(sh[1])).astype(np.float32)).to(DEV)
            out.append(ring)
        return out
    many, explicit = (lh.learner(c["H"], c["A"], lr=c["lrs"], gamma=c["gamma"], blob=blob, max_batch=4096) for _ in range(2))
    ra, rb = rings(), rings()
    for u in range(2):
        before = [ring.priorities.cpu().numpy() for ring in ra]
        al, cl, tds = many.update_from_many(ra, 700)
        drawn = [explicit.grad_from(ring, 700) for ring in rb]
        al2, cl2 = explicit.apply([row for row, _, _ in drawn])
        for ring, (_, td, idx) in zip(rb, drawn):
            explicit.write_priorities(ring, idx, td)
        assert torch.equal(al, al2) and torch.equal(cl, cl2) and torch.isfinite(al)
        for k, (x, y, p0) in enumerate(zip(ra, rb, before)):
            kk = min(700, x.count)
            assert torch.equal(tds[k], drawn[k][1]) and torch.equal(x._idx[:kk], y._idx[:kk])
            assert torch.equal(x.priorities, y.priorities)
            wantp = mirror.last_wins(p0, x._idx[:kk].cpu().numpy(), np.abs(tds[k].cpu().numpy()))
            assert np.array_equal(x.priorities.cpu().numpy(), wantp.astype(np.float32)), (u, k)
    many.check(); explicit.check()
    for ring in ra + rb:
        ring.check()
    lh.same(lh.state(many), lh.state(explicit))


# ---- 4. refusal is global --------------------------------------------------------------------------------------------

def test_refusal_is_global():
    c, blob, b = _teeth()
    K, j = 3, 1
    H, A = c["H"], c["A"]
    shards = lh.split(b, lh.cuts(c["n"], K))
    stores = [_store(*sh) for sh in shards]
    ns = [len(sh[1]) for sh in shards]
    Ls = [lh.learner(H, A, blob=blob, max_batch=c["n"]) for _ in range(K)]
    twins = [lh.learner(H, A, blob=blob, max_batch=c["n"]) for _ in range(K)]
    prios = [torch.rand(n, device=DEV) + 0.1 for n in ns]
    prio0 = [p.clone() for p in prios]
    before = [lh.state(L) for L in Ls]

    def round_(learners, sts, prio):
        rows = learners[0].new_rows(K)
        tds = [L._grad(ns[k], sts[k], ns[k], None, rows[k])[1] for k, L in enumerate(learners)]
        losses = [L.apply(rows) for L in learners]
        for k, L in enumerate(learners):
            L.write_priorities(_prio_target(prio[k], ns[k]), None, tds[k])
        return rows, losses

    bad = [dict(st) for st in stores]
    bad[j]["actions"] = stores[j]["actions"].clone()
    bad[j]["actions"][ns[j] // 2] = A                                    # one action out of range, in shard j only
    rows, losses = round_(Ls, bad, prios)
    tails = rows[:, -8:].view(torch.int32).cpu().numpy()
    assert [int(t[6]) for t in tails] == [1 if k == j else 0 for k in range(K)]
    for k, L in enumerate(Ls):
        assert torch.isnan(losses[k][0]) and torch.isnan(losses[k][1])
        with pytest.raises(RuntimeError, match="1 update"):
            L.check()
        L.check()                                                         # the count restarts
        lh.same(lh.state(L), before[k], "refused")
        assert torch.equal(prios[k], prio0[k])
    # the next clean update succeeds and matches twins that never saw the bad one
    _, losses = round_(Ls, stores, prios)
    tprios = [p.clone() for p in prio0]
    _, tlosses = round_(twins, stores, tprios)
    for k in range(K):
        Ls[k].check(); twins[k].check()
        lh.same(lh.state(Ls[k]), lh.state(twins[k]), "after")
        assert torch.equal(losses[k][0], tlosses[k][0]) and torch.isfinite(losses[k][0])
        assert torch.equal(prios[k], tprios[k]) and not torch.equal(prios[k], prio0[k])
    # a row of a learner of another width: its words do not carry this layout's tag
    other = lh.learner(64, A, blob=lh.init_blob(64, A, 1), max_batch=c["n"])
    foreign, _ = other._grad(ns[0], stores[0], ns[0], None)
    other.check()
    L = Ls[0]
    rows = L.new_rows(2).zero_()
    good, td = L._grad(ns[0], stores[0], ns[0], None, rows[0])
    rows[1, :foreign.numel()] = foreign
    state0, p0 = lh.state(L), prios[0].clone()
    al, cl = L.apply(rows)
    L.write_priorities(_prio_target(prios[0], ns[0]), None, td)
    assert torch.isnan(al) and torch.isnan(cl)
    with pytest.raises(RuntimeError, match="1 update"):
        L.check()
    lh.same(lh.state(L), state0, "foreign")
    assert torch.equal(prios[0], p0)
    with pytest.raises(ValueError, match="rows must be"):
        L.apply(foreign)                                                  # the Python layer refuses the shape outright


# ---- 5. host-side errors enqueue nothing ---------------------------------------------------------------------------

def test_host_side_errors_enqueue_nothing():
    from uavtrack import _lib
    lib = _lib.load()
    H, A, n = 64, 12, 500
    rng = np.random.RandomState(2)
    store = _store(*lh.batch(rng, n, A))
    L = lh.learner(H, A, blob=lh.init_blob(H, A, 2), max_batch=n)
    row, td = L._grad(n, store, n, None)
    L.apply(row)
    L.check()
    before = lh.state(L)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    out = torch.full((2,), 7.0, device=DEV)
    row0, td0 = row.clone(), td.clone()
    prio = torch.rand(n, device=DEV)
    prio0 = prio.clone()
    st = (p(store["states"]), p(store["actions"]), p(store["rewards"]), p(store["next_states"]))

    def err(rc, starts):
        assert rc != 0
        msg = lib.uavtrack_last_error().decode()
        assert msg.startswith(starts + ": "), msg
        return msg
    big = torch.zeros(n + 1, device=DEV)
    err(lib.uavtrack_learner_grad(L._h, n, *st, n, None, p(td), None, None), "uavtrack_learner_grad")            # null row
    err(lib.uavtrack_learner_grad(L._h, n, *st, n, None, None, p(row), None), "uavtrack_learner_grad")           # null td_delta
    assert "reserved" in err(lib.uavtrack_learner_grad(L._h, n + 1, *st, n + 1, None, p(big), p(row), None),
                             "uavtrack_learner_grad")                                                          # n above the reserve
    err(lib.uavtrack_learner_grad(L._h, 0, *st, n, None, p(td), p(row), None), "uavtrack_learner_grad")
    err(lib.uavtrack_learner_grad(L._h, n, None, st[1], st[2], st[3], n, None, p(td), p(row), None), "uavtrack_learner_grad")
    err(lib.uavtrack_learner_apply(L._h, None, 1, p(out[0:1]), p(out[1:2]), None), "uavtrack_learner_apply")     # null rows
    assert "count" in err(lib.uavtrack_learner_apply(L._h, p(row), 0, p(out[0:1]), p(out[1:2]), None), "uavtrack_learner_apply")
    assert "count" in err(lib.uavtrack_learner_apply(L._h, p(row), _lib.LEARNER_MAX_ROWS + 1, p(out[0:1]), p(out[1:2]), None),
                          "uavtrack_learner_apply")
    err(lib.uavtrack_learner_apply(L._h, p(row), 1, None, p(out[1:2]), None), "uavtrack_learner_apply")
    err(lib.uavtrack_learner_write_priorities(L._h, n, None, n, None, p(prio), None), "uavtrack_learner_write_priorities")
    err(lib.uavtrack_learner_write_priorities(L._h, n, None, n, p(td), None, None), "uavtrack_learner_write_priorities")
    err(lib.uavtrack_learner_write_priorities(L._h, n + 1, None, n + 1, p(big), p(prio), None), "uavtrack_learner_write_priorities")
    err(lib.uavtrack_learner_row_floats(L._h, None), "uavtrack_learner_row_floats")
    with pytest.raises(ValueError, match="1 to 64"):
        L.update_from_many([], 10)
    L.check()                                                             # nothing ran, so nothing was refused either
    lh.same(lh.state(L), before)
    assert torch.equal(row, row0) and torch.equal(td, td0) and torch.equal(prio, prio0)
    assert torch.equal(out, torch.full((2,), 7.0, device=DEV))
    rf = C.c_int64()
    assert lib.uavtrack_learner_row_floats(L._h, C.byref(rf)) == 0
    assert rf.value == L.row_floats == _uav().learner.row_floats(H, A) == L.num_params + 8


# ---- 6. graph capture --------------------------------------------------------------------------------------------------

def test_graph_capture_of_the_split_chain():
    """draw + grad + apply + write_priorities captured once and replayed three times == three eager rounds, bitwise: the
    ring's device call counter and the Adam step counts advance under replay."""
    H, A, n, k = 128, 12, 5000, 2048
    rng = np.random.RandomState(31)
    data = lh.batch(rng, n, A)
    blob = lh.init_blob(H, A, 31)

    def ring():
        r = _uav().PrioritizedReplayRing(n + 50, DEV, seed=5, max_batch=k)
        r.add({key: v.cpu() for key, v in _store(*data).items()})
        r.priorities[:n] = torch.from_numpy(np.random.RandomState(1).uniform(0.1, 2.0, n).astype(np.float32)).to(DEV)
        return r

    def round_(L, r):
        row, td, idx = L.grad_from(r, k)
        al, cl = L.apply(row)
        L.write_priorities(r, idx, td)
        return al, cl, td
    eager, re_ = lh.learner(H, A, blob=blob, max_batch=k), ring()
    e_out = [tuple(t.clone() for t in round_(eager, re_)) for _ in range(3)]
    graphed, rg = lh.learner(H, A, blob=blob, max_batch=k), ring()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            g_out = round_(graphed, rg)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(lh.state(graphed)["step"], np.zeros(8))           # capture ran nothing
    for u in range(3):
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(e_out[u], g_out):
            assert torch.equal(x, y), u
    assert np.array_equal(lh.state(graphed)["step"], np.full(8, 3))
    assert len({float(o[0]) for o in e_out}) == 3                         # three different draws
    lh.same(lh.state(graphed), lh.state(eager))
    assert torch.equal(re_.priorities, rg.priorities)
    graphed.check(); eager.check(); re_.check(); rg.check()


# ---- 7. two processes, one GPU ---------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_processes_stay_bitwise_equal(backend, tmp_path):
    """Two fresh child processes (tests/learner_dp_worker.py), each with its own ring and learner: broadcast_learner,
    then three update_from(..., group=...) with uneven n.  Both ranks bitwise equal each other and a single-process run
    of update_from_many over the same two rings."""
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("the nccl leg needs two GPUs")
    port = _free_port()
    script = os.path.join(ROOT, "tests", "learner_dp_worker.py")
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
    for k in ("params", "exp_avg", "exp_avg_sq", "step", "losses"):
        assert np.array_equal(z[0][k], z[1][k]), k
    assert np.array_equal(z[0]["step"], np.full(8, 1 + worker.UPDATES))
    assert z[0]["td0"].shape == (worker.COUNTS[0],) and z[1]["td0"].shape == (worker.COUNTS[1],)
    # the single-process side: rank 0's start state, both rings, update_from_many
    rings = [worker.ring_for(r, DEV) for r in range(2)]
    L = worker.learner_for(7, DEV)
    L._run(64, rings[0].store, rings[0].capacity, None, None)
    losses, tds = [], []
    for _ in range(worker.UPDATES):
        al, cl, td = L.update_from_many(rings, worker.BATCH)
        losses.append((al, cl)); tds.append(td)
    L.check()
    for r in range(2):
        one = worker.blobs(L, rings[r], losses, [t[r] for t in tds])
        assert one.keys() == z[r].keys()
        for k in one:
            assert np.array_equal(one[k], z[r][k]), (r, k)


# ---- 8. the example ----------------------------------------------------------------------------------------------------

def test_example_trains_from_two_shards(capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_maac
    common = ["--envs", "256", "--iters", "3", "--learner", "device", "--replay", "prioritized", "--publish", "device"]
    hist = train_maac.main(["--shards", "2"] + common)                   # replay.check() and learner.check() inside
    assert len(hist) == 3 and np.isfinite(hist).all()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
    assert len(lines) == 3 and all("shards 2" in ln for ln in lines)
    assert all(np.isfinite(float(ln.split("critic loss")[1].split()[0])) for ln in lines)
    one = train_maac.main(["--shards", "1"] + common)
    base = train_maac.main(common)
    assert one == base                                                    # --shards 1 is the loop as it was
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iter")]
    assert len(lines) == 6 and not any("shards" in ln for ln in lines)
    with pytest.raises(SystemExit):
        train_maac.main(["--shards", "2", "--envs", "64"])
