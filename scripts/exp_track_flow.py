"""Timing of track flow, v1 (himo_amd/track_flow.py) on one MI355X: the apply kernel at 120k rows beside himo_accum_motion on the same
rows in the same process (the nearest streaming pass: it moves 40 bytes a row, the apply kernel 44), both again at 18M rows, and one whole
call of 16 scenes x 150 sweeps x 300 boxes split into plan and apply.  Synthetic tables; sets no bar.

    python scripts/exp_track_flow.py [--out profiles/track_flow.txt]
"""
import argparse
import ctypes
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import trackflow_ref as ref  # noqa: E402
from himo_amd import _lib  # noqa: E402
from himo_amd.track_flow import TrackFlow, ego_transform, prepare  # noqa: E402


def pose(k):
    yaw = 0.01 * k
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0, 0.8 * k], [s, c, 0, 0.02 * k], [0, 0, 1, 0], [0, 0, 0, 1.0]])


def scene(rng, K, F):
    """K sweeps of F boxes: random velocities, label ids 1..F in random order, F tracks of which every sweep misses a tenth"""
    out = []
    for k in range(K):
        b = np.zeros((F, 12), np.float32)
        b[:, 7:10] = rng.uniform(-15, 15, (F, 3))
        b[:, 10] = rng.permutation(F) + 1
        t = np.zeros((F, 6))
        t[:, 0] = np.where(rng.random(F) < 0.1, -1, rng.permutation(F))
        out.append(prepare(b, t, pose(k), pose(0)))
    return out


def timed(fn, batches, per, warm):
    """(median, min, max) over ``batches`` of the device time of one call [us]: ``per`` calls between two events, after ``warm`` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / per)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "track_flow.txt"))
    a = ap.parse_args()
    dev = _lib.require_gpu()
    lib, P = _lib.load(), _lib.ptr
    lines = []

    def say(s):
        print(s)
        lines.append(s)
    fmt = lambda r, unit=1.0, d=2: f"{r[0] / unit:.{d}f} ({r[1] / unit:.{d}f} .. {r[2] / unit:.{d}f})"      # noqa: E731
    say(f"track_flow timing (scripts/exp_track_flow.py): synthetic tables, one {torch.cuda.get_device_name(dev)} (MI355X, gfx950), torch "
        f"{torch.__version__}, one process; HIP events on the stream around batches of calls, median (min .. max) over the batches after warm-up "
        "calls; no bar is set; nothing has been tried on field data")
    say("compiler's resource report (gfx950, -Rpass-analysis=kernel-resource-usage): tf_length_kernel 13 VGPRs, no LDS; tf_plan_kernel 40 VGPRs, 34816 bytes "
        "LDS a block, occupancy 8 waves a SIMD; tf_apply_kernel 82 VGPRs, 22560 bytes LDS a block, occupancy 5 waves a SIMD; no scratch and no spills in any")
    rng = np.random.default_rng(5)
    with torch.cuda.device(dev):
        stream = _lib.stream_handle()
        # ---- against the restatement, small ----------------------------------------------------------------------------------------------
        eng = TrackFlow(dev)
        small = [scene(rng, 6, 40), scene(rng, 3, 17)]
        got, want = eng.plan(small), ref.plan(small)
        same = all(np.asarray(g).tobytes() == w.tobytes() for g, w in zip((got.state, got.m, got.shift, got.disp, got.u), want))
        say(f"against tests/trackflow_ref.py on 2 small scenes (9 sweeps, {len(want[0])} boxes): every plan output identical {same}")

        # ---- 1. the apply kernel at 120k rows beside himo_accum_motion on the same rows ---------------------------------------------------
        N, F = 120_000, 300
        one = scene(rng, 5, F)
        plan = eng.plan([one])
        s = one[2]
        pc0 = torch.from_numpy(rng.uniform(-50, 50, (N, 4)).astype(np.float32)).to(dev)
        flow = torch.from_numpy(rng.normal(0, 1, (N, 3)).astype(np.float32)).to(dev)
        lab_h = np.where(rng.random(N) < 0.6, 0, rng.choice(s.sorted_id, N)).astype(np.int32)
        label = torch.from_numpy(lab_h).to(dev)
        E = ego_transform(pose(2), pose(3))
        E16 = np.concatenate([E, [0, 0, 0, 1]]).astype(np.float32)
        e_ptr = E16.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        d_E = torch.from_numpy(E).to(dev)
        out = torch.empty((N, 3), dtype=torch.float32, device=dev)
        counts = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        h_pt, h_box = np.array([0, N], np.int64), np.array(plan.rows(0, 2), np.int64)
        d_pt, d_box = torch.from_numpy(h_pt).to(dev), torch.from_numpy(h_box).to(dev)
        prm = eng.params.c_struct()
        motion = torch.empty((N, 3), dtype=torch.float32, device=dev)

        def run_apply(mode=0):
            prm.mode = mode
            st = lib.himo_trackflow_apply(1, h_pt.ctypes.data, P(d_pt), P(pc0), 4, P(flow), P(label), P(d_E), h_box.ctypes.data, P(d_box),
                                          int(plan.det_off[-1]), P(plan.tables[0]), P(plan.tables[1]), P(plan.device[0]), P(plan.device[2]),
                                          P(plan.device[3]), ctypes.addressof(prm), P(out), P(counts), stream)
            assert st == 0, st

        def run_motion():
            assert lib.himo_accum_motion(N, P(pc0), 4, P(flow), e_ptr, P(motion), stream) == 0
        run_apply()
        torch.cuda.synchronize()
        want_out, nm, ns = ref.apply_sweep(pc0.cpu().numpy(), flow.cpu().numpy(), lab_h, E, s, ref.Plan(*(x[slice(*plan.rows(0, 2))] for x in
                                                                                                          (plan.state, plan.m, plan.shift, plan.disp, plan.u))), 0)
        say(f"apply at {N} rows (pitch 4), {F} boxes, {int((lab_h > 0).sum())} labelled rows: rewritten {counts.cpu().numpy().tolist()[0]} (moving, static); "
            f"against the restatement: flow identical {out.cpu().numpy().view(np.uint32).tobytes() == want_out.view(np.uint32).tobytes()}, counts "
            f"{[nm, ns] == counts.cpu().numpy().tolist()[0]}")
        res = {}
        for _ in range(3):                                           # the three take turns, three rounds
            for name, fn in (("apply, shift", lambda: run_apply(0)), ("himo_accum_motion", run_motion), ("apply, replace", lambda: run_apply(1))):
                res.setdefault(name, []).append(timed(fn, 21, 20, 5))
        say("per call [us], 3 rounds of 21 batches of 20 calls, the three taking turns ('apply' = himo_trackflow_apply: the memset of the counts + the kernel):")
        for name, r in res.items():
            say(f"    {name:18s} " + "; ".join(fmt(x) for x in r))
        ma, mm = statistics.median(r[0] for r in res["apply, shift"]), statistics.median(r[0] for r in res["himo_accum_motion"])
        say(f"    median of the rounds: apply {ma:.2f} us = {44 * N / ma / 1e3:.0f} GB/s of its 44 bytes a row; himo_accum_motion {mm:.2f} us = "
            f"{40 * N / mm / 1e3:.0f} GB/s of its 40; RATIO {ma / mm:.2f} (the byte ratio is 1.10)")
        lib.himo_prof_enable(1)
        lib.himo_prof_reset()
        for _ in range(200):
            run_apply(0)
            run_motion()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.himo_prof_summary(buf, len(buf))
        lib.himo_prof_enable(0)
        say("    the library's per-kernel scopes over 200 alternating calls (name, calls, total ms, min ms, max ms; events around every single launch):")
        for ln in buf.value.decode().splitlines():
            say("        " + ln)

        # ---- 2. one whole call: 16 scenes x 150 sweeps x 300 boxes ------------------------------------------------------------------------
        S, K, n_pts = 16, 150, 120_000
        t0 = time.perf_counter()
        scenes = [scene(rng, K, F) for _ in range(S)]
        say(f"whole call, {S} scenes x {K} sweeps x {F} boxes: host preparation (rule A, numpy) {(time.perf_counter() - t0) * 1e3:.0f} ms by the host clock")
        walls = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            big = eng.plan(scenes)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        say("    TrackFlow.plan by the host clock (tables packed and uploaded, memset + two launches, synchronised) [ms], 5 calls: " +
            ", ".join(f"{w:.1f}" for w in walls))
        boxes, tid, w, U, sid, srow, sweep_off, det_off, id_off = eng.tables(scenes)
        d = [torch.from_numpy(x).to(dev) for x in (boxes, tid, w, U, sweep_off, det_off, id_off)]
        rows = len(boxes)
        o = (torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros((rows, 3), device=dev),
             torch.zeros((rows, 3), device=dev), torch.zeros((rows, 3), dtype=torch.float64, device=dev))
        need = int(lib.himo_trackflow_workspace_bytes(S, sweep_off.ctypes.data, det_off.ctypes.data, id_off.ctypes.data))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        prm.mode = 0

        def run_plan():
            st = lib.himo_trackflow_plan(S, sweep_off.ctypes.data, P(d[4]), det_off.ctypes.data, P(d[5]), id_off.ctypes.data, P(d[6]), P(d[1]), P(d[2]),
                                         P(d[0]), P(d[3]), ctypes.addressof(prm), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(ws), need, stream)
            assert st == 0, st
        rp = timed(run_plan, 11, 5, 2)
        say(f"    himo_trackflow_plan on resident tables ({rows} box rows, workspace {need} bytes, {S * K} workgroups) [us]: {fmt(rp, 1.0, 1)}")
        # apply: one scene a launch; the point buffers of one scene (150 sweeps x 120k rows) serve every scene
        R = K * n_pts
        g = torch.Generator(device=dev).manual_seed(1)
        pc = (torch.rand((R, 4), device=dev, generator=g) - 0.5) * 100
        fl = torch.randn((R, 3), device=dev, generator=g)
        lb = torch.where(torch.rand(R, device=dev, generator=g) < 0.6, torch.zeros(R, dtype=torch.int64, device=dev),
                         torch.randint(1, F + 1, (R,), device=dev, generator=g)).to(torch.int32)
        Es = torch.from_numpy(np.stack([ego_transform(pose(k), pose(k + 1)) for k in range(K)])).to(dev)
        ob, mo = torch.empty((R, 3), device=dev), torch.empty((R, 3), device=dev)
        cn = torch.zeros((K, 2), dtype=torch.int32, device=dev)
        hp = (np.arange(K + 1) * n_pts).astype(np.int64)
        dp = torch.from_numpy(hp).to(dev)
        hb = [np.ascontiguousarray(big.det_off[int(big.sweep_off[n]):int(big.sweep_off[n + 1]) + 1]) for n in range(S)]
        db = [torch.from_numpy(h).to(dev) for h in hb]

        def run_scene(n):
            st = lib.himo_trackflow_apply(K, hp.ctypes.data, P(dp), P(pc), 4, P(fl), P(lb), P(Es), hb[n].ctypes.data, P(db[n]), int(big.det_off[-1]),
                                          P(big.tables[0]), P(big.tables[1]), P(big.device[0]), P(big.device[2]), P(big.device[3]), ctypes.addressof(prm),
                                          P(ob), P(cn), stream)
            assert st == 0, st

        def run_all():
            for n in range(S):
                run_scene(n)

        def run_motion_big():
            assert lib.himo_accum_motion(R, P(pc), 4, P(fl), e_ptr, P(mo), stream) == 0
        r1 = timed(lambda: run_scene(3), 7, 3, 2)
        torch.cuda.synchronize()
        say(f"    apply of ONE scene in one launch ({K} sweeps x {n_pts} rows = {R} rows; {int(cn.sum())} rewritten) [ms]: {fmt(r1, 1e3, 3)} = "
            f"{44 * R / r1[0] / 1e3:.0f} GB/s")
        r3 = timed(run_motion_big, 7, 3, 2)
        say(f"    himo_accum_motion on the same {R} rows [ms]: {fmt(r3, 1e3, 3)} = {40 * R / r3[0] / 1e3:.0f} GB/s; RATIO {r1[0] / r3[0]:.2f}")
        r2 = timed(run_all, 5, 1, 1)
        say(f"    apply of the whole call ({S} launches, {S * R} rows) [ms]: {fmt(r2, 1e3, 2)}")
        say(f"    the whole call on the device: plan {rp[0] / 1e3:.3f} ms + apply {r2[0] / 1e3:.2f} ms ({r2[0] / (S * K):.2f} us a sweep of {n_pts} rows); "
            "reading the points from the files and writing the flows back are not in it")
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
