#!/usr/bin/env python3
"""Experiment (GPU box): in-kernel time stamps of rollout launches (build_variants/stamp.so from stamp_build.py).
usage: stamp_run.py [B]                  -- 20 x 10 MAAC, T in (1, 5, 20): where a short launch's time goes
       stamp_run.py [B] --placement [T]  -- one T-step launch (default 200): which XCD / CU / SIMD every wave ran on, the
                                            per-step time of a wave alone on its SIMD and of one that shares it, by how many
                                            waves its CU holds; then the placement probe (256 workgroups of 512 threads that
                                            cannot share a CU) and the relay model of DESIGN 4.1.3 fed with the measured rates"""
import collections, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd")]
os.environ["UAVTRACK_LIB"] = os.path.join(ROOT, "build_variants", "stamp.so")
import numpy as np, torch, uavtrack
argv = sys.argv[1:]
placement = "--placement" in argv
cut = argv.index("--placement") if placement else len(argv)
B = int(argv[0]) if cut > 0 else 4096
T_placement = int(argv[cut + 1]) if len(argv) > cut + 1 else 200
cfg = uavtrack.EnvConfig(n_envs=B, n_uav=20, m_targets=10)
env = uavtrack.BatchedUavEnv(cfg)
info = env.kernel_info()
G, E = info["workgroups"], info["envs_per_workgroup"]
assert E == 3, info
print(f"B={B}: {G} workgroups of {info['workgroup']} threads, {E} envs each")
G1 = G - 1             # (the last workgroup may hold fewer than 3 environments: its 15 words are not all there)


def stamped_launch(act, out):
    """A few launches back to back, the last one measured (no idle GPU in front of it): event time in us and the
    [G1, 9] stamp words (entry, filled, stepped, exit, HW_ID, XCC_ID, the three quarter marks of the step loop)."""
    env.reset(seed=1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = env.step_many(act, out=out)
    e0.record(); out = env.step_many(act, out=out); e1.record()
    torch.cuda.synchronize()
    st = out["ep_sums"].view(torch.int32).reshape(-1)[: 15 * G1].reshape(G1, 15)[:, :9].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return e0.elapsed_time(e1) * 1e3, st, out


def where(hw, xcc):
    """HW_ID of gfx9: wave slot [3:0], SIMD [5:4], pipe [7:6], CU [11:8], shader array [12], shader engine [15:13];
    XCC_ID [3:0].  Returns (cu key, simd, wave slot); the CU key is everything above the SIMD that names a place."""
    cu = (xcc & 0xF) << 8 | ((hw >> 8) & 0xFF)
    return cu, (hw >> 4) & 3, hw & 0xF


def short_launches():
    for T in (1, 5, 20):
        act = torch.randint(0, 12, (T, B, 20), dtype=torch.int32, device="cuda")
        env.reset(seed=1)
        out = env.step_many(act)
        rows = []
        for rep in range(40):
            us, st, out = stamped_launch(act, out)
            t0, t1, t2, t3 = (st[:, k] * 10.0 for k in range(4))          # ns (100 MHz)
            base = t0.min()
            rows.append([us, (t3.max() - base) / 1e3, (t0.max() - base) / 1e3, np.median(t1 - t0) / 1e3,
                         np.median(t2 - t1) / 1e3, np.median(t3 - t2) / 1e3, np.median(t3 - t0) / 1e3, (np.sort(t3)[G1 // 2] - base) / 1e3])
        r = np.median(np.array(rows), axis=0)
        print(f"T={T:2d}: events {r[0]:.2f} us | first entry -> last exit {r[1]:.2f} | last workgroup enters at {r[2]:.2f} | per workgroup (median): "
              f"load+fill {r[3]:.2f}, steps {r[4]:.2f} ({r[4] / T:.2f}/step), tail {r[5]:.2f}, entry->exit {r[6]:.2f}; median exit at {r[7]:.2f}")


def hist(counter, total_places):
    h = collections.Counter(counter.values())
    h[0] = total_places - len(counter)
    return "  ".join(f"{k} waves: {h[k]}" for k in sorted(h))


def placement_run(T, reps=12):
    act = torch.randint(0, 12, (T, B, 20), dtype=torch.int32, device="cuda")
    env.reset(seed=1)
    out = env.step_many(act)
    for _ in range(150):                        # loaded clocks (tools/drift.py)
        out = env.step_many(act, out=out)
    tq = (T >> 2) & ~1
    events, spans, step_spans = [], [], []
    cols = []                    # per wave and launch: waves on its CU, on its SIMD, XCD, us per step (whole loop, first quarter, last quarter), its last step done at
    pairs = []
    today_cu, relay_cu = [], []  # per launch: when the last CU is through its steps, today and under the per-CU model
    for rep in range(reps):
        us, st, out = stamped_launch(act, out)
        cu, simd, slot = where(st[:, 4], st[:, 5])
        skey = cu * 4 + simd
        per_cu, per_simd = collections.Counter(cu.tolist()), collections.Counter(skey.tolist())
        t = st[:, [0, 1, 2, 3, 6, 7, 8]] * 0.01                # us
        base = t[:, 1].min()
        events.append(us); spans.append(t[:, 3].max() - t[:, 0].min()); step_spans.append(t[:, 2].max() - base)
        if rep < 2 or rep == reps - 1:
            print(f"[launch {rep}] events {us:.1f} us, first entry -> last exit {spans[-1]:.1f} us, first fill -> last step done {step_spans[-1]:.1f} us; "
                  f"{len(set((st[:, 5] & 0xF).tolist()))} XCDs, {len(per_cu)} CUs, {len(per_simd)} SIMDs hold the {G1} stamped waves")
            print(f"    per SIMD (of {4 * len(per_cu)} on the occupied CUs):  {hist(per_simd, 4 * len(per_cu))}")
            print(f"    per CU:    {hist(per_cu, len(per_cu))}")
            shapes = collections.Counter(tuple(sorted((per_simd.get(c * 4 + k, 0) for k in range(4)), reverse=True)) for c in per_cu)
            print("    waves on the four SIMDs of a CU (sorted) -> CUs:  " + "  ".join(f"{k}: {v}" for k, v in sorted(shapes.items())))
            print("    wave slots used: " + "  ".join(f"{k}: {v}" for k, v in sorted(collections.Counter(slot.tolist()).items())))
            perx = collections.Counter((st[:, 5] & 0xF).tolist())
            print("    waves per XCD: " + "  ".join(f"{k}: {v}" for k, v in sorted(perx.items())))
        ncu = np.array([per_cu[int(c)] for c in cu]); nsimd = np.array([per_simd[int(k)] for k in skey])
        whole = (t[:, 2] - t[:, 1]) / T
        q1 = (t[:, 4] - t[:, 1]) / tq if tq > 0 else whole
        q4 = (t[:, 2] - t[:, 6]) / (T - 3 * tq) if tq > 0 else whole
        cols.append(np.stack([ncu, nsimd, st[:, 5] & 0xF, whole, q1, q4, t[:, 2] - base], axis=1))
        # the two waves of a shared SIMD, side by side: (faster, slower) over the loop and in the first quarter; which slot, which entered first
        o = np.argsort(skey, kind="stable"); o = o[nsimd[o] == 2].reshape(-1, 2)
        fast = np.where(whole[o[:, 0]] <= whole[o[:, 1]], o[:, 0], o[:, 1]); slow = o[:, 0] + o[:, 1] - fast
        pairs.append(np.stack([whole[fast], whole[slow], q1[fast], q1[slow], slot[fast] < slot[slow], t[fast, 0] < t[slow, 0]], axis=1))
        # Per CU: the rate R at which it advances while all its waves run (first quarter: sum of 1 / us-per-step), and the model
        # "its n waves' n * T wave-steps at R throughout" -- what moving work between its SIMDs could at best reach -- against
        # when its last wave is through today.
        _, inv = np.unique(cu, return_inverse=True)
        R = np.zeros(inv.max() + 1); np.add.at(R, inv, 1.0 / q1)
        n = np.bincount(inv)
        first = np.full(len(n), np.inf); np.minimum.at(first, inv, t[:, 1] - base)
        last = np.zeros(len(n)); np.maximum.at(last, inv, t[:, 2] - base)
        today_cu.append(last.max()); relay_cu.append((first + n * T / R).max())
        if rep == reps - 1:
            order = np.argsort(t[:, 2])[-12:]
            print("    the last 12 waves through their steps (us after the first fill | waves on CU, on SIMD | XCD | us per step whole, first, last quarter):")
            for w in order:
                print(f"        {t[w, 2] - base:.1f} | {ncu[w]}, {nsimd[w]} | {int(st[w, 5] & 0xF)} | {whole[w]:.3f} {q1[w]:.3f} {q4[w]:.3f}")
    ev = float(np.median(events))
    A = np.concatenate(cols)
    print(f"T={T}: events median {ev:.1f} us (min {min(events):.1f}, max {max(events):.1f}); first entry -> last exit median {np.median(spans):.1f} us; "
          f"step phase of the whole launch (first fill -> last step done) median {np.median(step_spans):.1f} us")
    print(f"us per step of a wave over {reps} launches: whole loop p5 / median / p95 / max | first quarter (its CU still full) median | last quarter median | "
          "last step done, us after the first fill: median / p95 / max")
    med = {}
    for key in sorted(set(zip(A[:, 0].astype(int).tolist(), A[:, 1].astype(int).tolist()))):
        r = A[(A[:, 0] == key[0]) & (A[:, 1] == key[1])]
        med[key] = [float(np.median(r[:, k])) for k in (3, 4, 5)]
        pc = np.percentile(r[:, 3], [5, 50, 95, 100]); fin = np.percentile(r[:, 6], [50, 95, 100])
        print(f"    CU holds {key[0]} waves, SIMD holds {key[1]}: {pc[0]:.3f} / {pc[1]:.3f} / {pc[2]:.3f} / {pc[3]:.3f} | {med[key][1]:.3f} | {med[key][2]:.3f} | "
              f"{fin[0]:.1f} / {fin[1]:.1f} / {fin[2]:.1f}   ({len(r)} waves)")
    P = np.concatenate(pairs)
    print(f"the two waves of a shared SIMD ({len(P)} pairs): us per step over the loop, faster one p5 / median / p95: " + " / ".join(f"{v:.3f}" for v in np.percentile(P[:, 0], [5, 50, 95]))
          + "; slower one: " + " / ".join(f"{v:.3f}" for v in np.percentile(P[:, 1], [5, 50, 95]))
          + f"; first quarter, medians: {np.median(P[:, 2]):.3f} and {np.median(P[:, 3]):.3f}; the faster one has the lower wave slot in {100 * P[:, 4].mean():.0f} %, entered first in {100 * P[:, 5].mean():.0f} % of the pairs")
    print("median us per step (whole loop) of the waves that share a SIMD, by XCD: " +
          "  ".join(f"{x}: {np.median(A[(A[:, 2] == x) & (A[:, 1] == 2)][:, 3]):.3f}" for x in sorted(set(A[:, 2].astype(int).tolist()))))
    print("wave-steps per us of a CU while all its waves run (first quarter): " + "  ".join(
        f"{n} waves: {sum(np.sum(A[:, 0] == n) and np.sum((A[:, 0] == n) & (A[:, 1] == k)) / np.sum(A[:, 0] == n) * n / med[(n, k)][1] for k in (1, 2) if (n, k) in med):.2f}"
        for n in sorted(set(A[:, 0].astype(int).tolist()))))
    # The relay model of the issue: 6 items on the 8 wave slots of a CU, two SIMDs carry two items and two carry
    # one at any time, every item spends the same share alone: the CU advances 4 / r2 + 2 / r1 item-steps per us.
    if (6, 1) in med and (6, 2) in med:
        r1, r2 = med[(6, 1)][1], med[(6, 2)][1]
        steps = 6 * T / (4 / r2 + 2 / r1)
        cu6 = A[(A[:, 0] == 6) & (A[:, 1] == 2)][:, 6]
        print(f"relay model, 6 items per CU, alone {r1:.3f} us, paired {r2:.3f} us per step (first quarter, CU of 6): the CU's step phase {steps:.1f} us; "
              f"today the paired waves of a CU of 6 are through at {np.median(cu6):.1f} us (median; p95 {np.percentile(cu6, 95):.1f}), "
              f"the whole launch at {np.median(step_spans):.1f} us")
    tc, rc = float(np.median(today_cu)), float(np.median(relay_cu))
    print(f"per-CU model (each CU keeps its first-quarter rate to the end): last CU through at {rc:.1f} us against {tc:.1f} us today (medians of {reps} launches): "
          f"predicted launch {ev - tc + rc:.1f} us against {ev:.1f} us = {100 * ((ev - tc + rc) / ev - 1):+.1f} %  (no hand-off cost taken off)")


def probe(blocks=256, threads=512, lds=81 * 1024, hold_us=30):
    lib = ctypes.CDLL(os.environ["UAVTRACK_LIB"])
    lib.uavtrack_stamp_probe.restype = ctypes.c_int
    lib.uavtrack_stamp_probe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p]
    W = threads // 64
    for rep in range(3):
        buf = torch.zeros(blocks * W * 4, dtype=torch.int32, device="cuda")
        rc = lib.uavtrack_stamp_probe(buf.data_ptr(), blocks, threads, lds, hold_us * 100, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        q = buf.cpu().numpy().astype(np.int64).reshape(blocks, W, 4) & 0xFFFFFFFF
        cu, simd, slot = where(q[:, :, 0], q[:, :, 1])
        one_cu = int((cu == cu[:, :1]).all(axis=1).sum())
        per_cu = collections.Counter(cu[:, 0].tolist())
        together = (q[:, :, 2].max() - q[:, :, 2].min()) * 0.01
        pat = collections.Counter("".join(str(int(s)) for s in row) for row in simd)
        spread = collections.Counter(tuple(sorted(collections.Counter(row.tolist()).values(), reverse=True)) for row in simd)
        print(f"[probe {rep}] {blocks} workgroups x {threads} threads, {lds} B of LDS, held {hold_us} us; last wave entered {together:.2f} us after the first "
              f"({'all resident together' if together < hold_us else 'NOT all resident together'})")
        print(f"    workgroups whose {W} waves share one CU: {one_cu} / {blocks};  distinct CUs: {len(per_cu)};  workgroups per CU: "
              + "  ".join(f"{k}: {v}" for k, v in sorted(collections.Counter(per_cu.values()).items())))
        print("    waves per SIMD inside a workgroup (sorted) -> workgroups:  " + "  ".join(f"{k}: {v}" for k, v in sorted(spread.items())))
        print("    SIMD of wave 0..%d -> workgroups:  " % (W - 1) + "  ".join(f"{k}: {v}" for k, v in pat.most_common(8)) + (f"  (+ {len(pat) - 8} more patterns)" if len(pat) > 8 else ""))
        print("    wave slot of wave 0..%d, first workgroups: " % (W - 1) + " | ".join(",".join(str(int(s)) for s in row) for row in slot[:4]))


if placement:
    placement_run(T_placement)
    probe()
else:
    short_launches()
