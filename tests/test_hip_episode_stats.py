"""uavtrack_episode_stats_* on the MI355X against the numpy mirror (tests/episode_stats_mirror.py), bit for bit on every
field of every record: at the shapes where the kernels change path (a partly filled last tile, UAV segments that
straddle a wavefront or a 32-word LDS row, tiles narrowed by a wide swarm, more than one group of 64 environments, one
environment, one step), with done flags built so that a log filled in arrival order would differ, through overflow,
clear, close, graph capture, and end to end behind the automatic reset in all three reward modes and `evaluate`."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_stats_mirror as mirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (B, N, T): B = 37 x N = 20 leaves the last tile partly filled; N = 5; N = 50 and 70 straddle a wavefront (70 also
# narrows the tile to 56 environments: B = 70 is two tiles and two groups); N = 1, 64, 65 (64, 65: tiles of 62 and 61);
# N = 300: tiles of 13; B = 1; T = 1, 7, 50
SHAPES = [(37, 20, 7), (3, 5, 50), (70, 50, 7), (70, 70, 7), (130, 1, 7), (65, 64, 1), (37, 65, 7), (1, 20, 50),
          (20, 300, 1)]


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def make_stats(B, N, cap, max_steps, env_offset=0):
    import uavtrack
    return uavtrack.EpisodeStats((B, N), log_capacity=cap, max_steps=max_steps, env_offset=env_offset, device=DEV)


def values(rng, shape):
    """fp32 values spanning 2^-20 .. 2^20 with random signs; along the last axis every third value is the exact negative
    of its predecessor, so the sums cancel exactly in places and an order other than the stated one shows."""
    x = (np.exp2(rng.uniform(-20.0, 20.0, shape)) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    if shape[-1] > 1:
        x[..., 1::3] = -x[..., 0:x[..., 1::3].shape[-1] * 3:3]
    return x


def launch_arrays(rng, T, B, N):
    return values(rng, (T, B, N)), values(rng, (T, 3, B, N)), rng.randint(0, 4097, (T, B)).astype(np.int32)


def staggered_done(T, B, shift=0):
    """done[t][b]: environment b closes where (t + 2 b + shift) % 5 == 0 -- so later rows close LOWER environments, which a
    log in arrival order would not reproduce -- plus environment 0 at t = 0 and at T - 1, and environment B - 1 on two
    consecutive steps."""
    t, b = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    d = ((t + 2 * b + shift) % 5 == 0).astype(np.uint8)
    d[0, 0] = d[T - 1, 0] = 1
    d[T // 2, B - 1] = d[min(T - 1, T // 2 + 1), B - 1] = 1
    return d


def feed(stats, m, arrays, done):
    """The same add to the device handle and to the mirror."""
    reward, terms, covered = arrays
    out = dict(reward=torch.from_numpy(reward).to(DEV), terms=torch.from_numpy(terms).to(DEV),
               covered=torch.from_numpy(covered).to(DEV), done=None if done is None else torch.from_numpy(done).to(DEV))
    stats.add(out)
    m.add(reward, terms, covered, done)


def same_log(stats, m):
    rec, dropped = stats.read_records()
    want = m.records()
    assert len(rec) == len(want) and dropped == m.dropped, (len(rec), len(want), dropped, m.dropped)
    for f in want.dtype.names:
        assert rec[f].tobytes() == want[f].tobytes(), (f, rec[f][:8], want[f][:8])
    assert rec.tobytes() == want.tobytes()
    return rec


@pytest.mark.parametrize("B,N,T", SHAPES)
def test_bitwise_against_mirror(B, N, T):
    """One sequence per shape: staggered done; done == NULL; done never; staggered again (the episodes open since the
    first add span three adds of different T); an add whose last row closes some environments, then close (those
    hold zero steps and get no record); read; clear; one more add and close; read."""
    rng = np.random.RandomState(B * 1000 + N)
    Ts = (T, max(1, T // 2), 1)
    stats = make_stats(B, N, cap=8 * T * B, max_steps=T, env_offset=5)
    m = mirror.EpisodeStatsMirror(B, N, 8 * T * B, env_offset=5)
    feed(stats, m, launch_arrays(rng, Ts[0], B, N), staggered_done(Ts[0], B))
    feed(stats, m, launch_arrays(rng, Ts[1], B, N), None)
    feed(stats, m, launch_arrays(rng, Ts[2], B, N), np.zeros((Ts[2], B), np.uint8))
    feed(stats, m, launch_arrays(rng, Ts[0], B, N), staggered_done(Ts[0], B, shift=3))
    last = np.zeros((Ts[1], B), np.uint8)
    last[-1, ::2] = 1
    feed(stats, m, launch_arrays(rng, Ts[1], B, N), last)
    stats.close(); m.close()
    rec = same_log(stats, m)
    assert len(rec) > B // 2 and (B == 1 or not np.all(np.diff(rec["env"]) >= 0))      # the cases did close, out of env order
    stats.clear(); m.clear()
    rec = same_log(stats, m)
    assert len(rec) == 0
    feed(stats, m, launch_arrays(rng, Ts[0], B, N), staggered_done(Ts[0], B, shift=1))
    stats.close(); m.close()
    same_log(stats, m)
    stats.destroy()


def test_overflow_counts_what_it_cannot_write():
    """log_capacity 5, 12 closing episodes (4 environments, 3 steps, every flag set): the first 5 in (t, b) order are
    present, 7 are counted; the mirror alone drops exactly those 7.  After clear the next read is right."""
    rng = np.random.RandomState(1)
    B, N, T = 4, 20, 3
    stats, m = make_stats(B, N, cap=5, max_steps=T), mirror.EpisodeStatsMirror(B, N, 5)
    feed(stats, m, launch_arrays(rng, T, B, N), np.ones((T, B), np.uint8))
    assert m.dropped == 7 and len(m.records()) == 5
    rec = same_log(stats, m)
    assert rec["env"].tolist() == [0, 1, 2, 3, 0] and rec["ordinal"].tolist() == [0, 0, 0, 0, 1]
    stats.clear(); m.clear()
    feed(stats, m, launch_arrays(rng, 2, B, N), np.array([[0, 1, 0, 0], [1, 0, 0, 1]], np.uint8))
    rec = same_log(stats, m)
    assert rec["env"].tolist() == [1, 0, 3] and rec["ordinal"].tolist() == [3, 3, 3] and m.dropped == 0
    stats.destroy()


def test_same_sequence_twice_same_bytes():
    logs = []
    for _ in range(2):
        rng = np.random.RandomState(2)
        B, N, T = 70, 20, 7
        stats, m = make_stats(B, N, cap=4 * T * B, max_steps=T), mirror.EpisodeStatsMirror(B, N, 4 * T * B)
        for shift in range(3):
            feed(stats, m, launch_arrays(rng, T, B, N), staggered_done(T, B, shift))
        stats.close()
        logs.append(stats.read_records()[0].tobytes())
        stats.destroy()
    assert logs[0] == logs[1] and len(logs[0]) > 0


def test_captured_add_replays_like_eager_calls():
    """An add captured with torch.cuda.graph (which refuses a synchronisation or an allocation inside the capture) and
    replayed twice equals two eager adds; the replays leave torch's allocator where it was."""
    rng = np.random.RandomState(3)
    B, N, T = 37, 20, 7
    reward, terms, covered = launch_arrays(rng, T, B, N)
    done = staggered_done(T, B)
    out = dict(reward=torch.from_numpy(reward).to(DEV), terms=torch.from_numpy(terms).to(DEV),
               covered=torch.from_numpy(covered).to(DEV), done=torch.from_numpy(done).to(DEV))
    eager = make_stats(B, N, cap=4 * T * B, max_steps=T)
    eager.add(out); eager.add(out)
    want = eager.read_records()[0]
    captured = make_stats(B, N, cap=4 * T * B, max_steps=T)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured.add(out)
    torch.cuda.synchronize()
    assert len(captured.read_records()[0]) == 0             # capture does not execute
    before = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    g.replay(); g.replay()
    assert (torch.cuda.memory_allocated(), torch.cuda.memory_reserved()) == before
    got = captured.read_records()[0]
    assert got.tobytes() == want.tobytes() and len(got) > 0
    m = mirror.EpisodeStatsMirror(B, N, 4 * T * B)
    m.add(reward, terms, covered, done); m.add(reward, terms, covered, done)
    assert got.tobytes() == m.records().tobytes()
    eager.destroy(); captured.destroy()


@pytest.mark.parametrize("mode", ["RAW", "MEAN", "PMI"])
def test_behind_automatic_reset(mode, pmi_state_dict_h64):
    """8 environments x 20 UAVs x 10 targets, horizon 6, one automatic-reset launch of 16 steps: two finished episodes
    per environment and an open one.  The records equal the mirror applied to that launch's own outputs; env carries
    env_offset = 100, ordinal counts 0, 1."""
    import uavtrack
    B, N, M, H, T = 8, 20, 10, 6, 16
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=0.0 if mode == "RAW" else 0.3,
                             reward_mode=getattr(uavtrack.RewardMode, mode), horizon=H, env_offset=100)
    env = uavtrack.BatchedUavEnv(cfg, DEV)
    if mode == "PMI":
        env.set_pmi(pmi_state_dict_h64)
    env.reset(seed=11)
    acts = torch.from_numpy(np.random.RandomState(4).randint(0, cfg.na_total, (T, B, N)).astype(np.int32)).to(DEV)
    out = env.step_many(acts, auto_reset_seed=23)
    stats = uavtrack.EpisodeStats(env, log_capacity=64, max_steps=T)
    stats.add(out)
    m = mirror.EpisodeStatsMirror(B, N, 64, env_offset=100)
    m.add(out["reward"].cpu().numpy(), out["terms"].cpu().numpy(), out["covered"].cpu().numpy(), out["done"].cpu().numpy())
    rec = same_log(stats, m)
    assert len(rec) == 2 * B and rec["steps"].tolist() == [H] * (2 * B)
    assert rec["env"].tolist() == list(range(100, 100 + B)) * 2 and rec["ordinal"].tolist() == [0] * B + [1] * B
    assert np.all(np.abs(rec["ret"]) <= 1.0) and np.all(rec["max_covered"] >= rec["average_covered"])
    stats.clear(); m.clear()
    stats.close(); m.close()                                # the open episodes: 4 steps each, ordinal 2
    rec = same_log(stats, m)
    assert rec["steps"].tolist() == [T - 2 * H] * B and rec["ordinal"].tolist() == [2] * B
    stats.destroy(); env.close()


@pytest.mark.parametrize("policy", ["greedy", "actor"])
def test_evaluate_sums_back_to_ep_sums(policy):
    """uavtrack.evaluate returns episodes x B records; multiplied back by their step counts they agree with the fp32
    ep_sums of the same launches.  The bound is fp32's alone: ep_sums[b][k] = sum_t mean_i x is a sum of N fp32 values
    (error <= (N - 1) u A), a division by N (u A) and a running sum of T such means ((T - 1) u A), with u = 2^-24 and
    A = sum_t mean_i |x|; the records' own fp64 error is 2^-29 of that.  The covered sum is an integer below 2^24: exact.
    "greedy" runs on a handle whose horizon is num_steps (the done path), the actor on one without horizon (close)."""
    import uavtrack
    B, N, M, T, E = 8, 20, 10, 12, 2
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=0.3, reward_mode=uavtrack.RewardMode.MEAN,
                             horizon=T if policy == "greedy" else 0)
    env = uavtrack.BatchedUavEnv(cfg, DEV)
    if policy == "actor":
        torch.manual_seed(5)
        pol = uavtrack.ActorMLP(hidden_dim=64, action_dim=cfg.na_total)
    else:
        pol = "greedy"
    res = uavtrack.evaluate(env, pol, num_steps=T, episodes=E, seed=9, mode="sample")
    assert res["path"] == ("done" if policy == "greedy" else "close")
    assert len(res["return_list"]) == E * B and res["dropped"] == 0
    assert res["env"].tolist() == list(range(B)) * E and res["steps"].tolist() == [T] * (E * B)
    assert res["ordinal"].tolist() == [e for e in range(E) for _ in range(B)]
    ep = res["ep_sums"].cpu().numpy().astype(np.float64).reshape(E * B, 5)
    keys = ["return_list", "target_tracking_return_list", "boundary_punishment_return_list",
            "duplicate_tracking_punishment_return_list"]
    u = 2.0 ** -24
    for k, key in enumerate(keys):
        back = res[key] * T                                  # sum / (T N) * T = sum_t mean_i
        bound = (N + T) * u * T * 1.0                        # A <= T: every reward and term lies in [-1, 1]
        print(f"{policy} {key}: max |records - ep_sums| = {np.abs(back - ep[:, k]).max():.3e}, bound {bound:.3e}")
        assert np.all(np.abs(back - ep[:, k]) <= bound), (key, np.abs(back - ep[:, k]).max(), bound)
        assert np.any(res[key] != 0.0) or key == "boundary_punishment_return_list"
    assert np.array_equal(res["average_covered_targets_list"] * T, ep[:, 4])
    assert np.all(res["max_covered_targets_list"] >= res["average_covered_targets_list"])
    assert np.all(res["max_covered_targets_list"] <= M)
    env.close()


def test_errors_enqueue_nothing_and_leave_the_log():
    from uavtrack import _lib
    rng = np.random.RandomState(6)
    B, N, T = 5, 20, 4
    stats, m = make_stats(B, N, cap=64, max_steps=T), mirror.EpisodeStatsMirror(B, N, 64)
    feed(stats, m, launch_arrays(rng, T, B, N), staggered_done(T, B))
    before = stats.read_records()[0].tobytes()
    reward, terms, covered = (torch.from_numpy(a).to(DEV) for a in launch_arrays(rng, T + 1, B, N))
    with pytest.raises(ValueError, match="terms"):
        stats.add(dict(reward=reward[:T].contiguous(), covered=covered[:T].contiguous(), terms=None))
    with pytest.raises(ValueError, match="covered"):
        stats.add(dict(reward=reward[:T].contiguous(), terms=terms[:T].contiguous()))
    with pytest.raises(ValueError, match="reward"):
        stats.add(dict(terms=terms[:T].contiguous(), covered=covered[:T].contiguous()))
    with pytest.raises(RuntimeError, match="max_steps"):
        stats.add(dict(reward=reward, terms=terms, covered=covered))          # T + 1 steps
    lib, st = _lib.load(), stats._stream()
    p = _lib.ptr
    assert lib.uavtrack_episode_stats_add(stats._h, T, None, p(terms), p(covered), None, st) != 0
    assert b"null" in lib.uavtrack_last_error()
    assert lib.uavtrack_episode_stats_add(stats._h, T, p(reward), None, p(covered), None, st) != 0
    assert lib.uavtrack_episode_stats_add(stats._h, T, p(reward), p(terms), None, None, st) != 0
    assert lib.uavtrack_episode_stats_add(None, T, p(reward), p(terms), p(covered), None, st) != 0
    assert lib.uavtrack_episode_stats_add(stats._h, 0, p(reward), p(terms), p(covered), None, st) != 0
    n, d = C.c_int64(), C.c_int64()
    assert lib.uavtrack_episode_stats_read(stats._h, None, 4, C.byref(n), C.byref(d), st) != 0
    bad = _lib.EpisodeStatsConfig(struct_size=C.sizeof(_lib.EpisodeStatsConfig), device_id=0, n_envs=4, n_uav=0,
                                  max_steps=4, log_capacity=4)
    h = C.c_void_p()
    assert lib.uavtrack_episode_stats_create(C.byref(bad), C.byref(h)) != 0 and not h.value
    assert b"n_uav" in lib.uavtrack_last_error()
    assert stats.read_records()[0].tobytes() == before
    stats.close(); m.close()                                # and the open episodes are what they were
    same_log(stats, m)
    stats.destroy()
