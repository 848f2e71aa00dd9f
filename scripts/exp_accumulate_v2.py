"""Timing of sweep accumulation, v2 (himo_amd/csrc/accumulate.hip) on the input of scripts/exp_accumulate.py: one target of 11 sources x
120 000 rows of the synthetic "rings" cloud, pitch 4, rows as generated, at the default grid.

(a) The v1 entry points -- the 11 ``himo_accum_insert`` calls and ``himo_accum_emit``, each between HIP events -- of this build and,
    with ``--baseline_lib``, of another build of libhimo_amd.so (the commit before v2) in the SAME process on the SAME buffers, the two
    taking turns repetition by repetition: the v1 instantiation of the templated kernels must cost what the untemplated kernels cost.
(b) The v2 insert with a motion, an intensity read in place from column 3 and a label per row (``himo_accum_insert_ex``: 16 + 12 + 4
    bytes a row instead of 16, and two more atomics per run of lanes into the same 32-byte slot) and ``himo_accum_emit_ex`` with both
    columns (8 more bytes read per occupied slot, 8 more written per row), and ``himo_accum_motion`` (rule I) for one sweep.
Prints medians, minima and maxima and the ratios; gates nothing.

    python scripts/exp_accumulate_v2.py [--baseline_lib OTHER/libhimo_amd.so] [--reps 30] [--out profiles/accumulate_v2.txt]
"""
import argparse
import ctypes
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

V1 = ("himo_accum_table_bytes", "himo_accum_clear", "himo_accum_insert", "himo_accum_emit", "himo_accum_status")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=11)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--baseline_lib", default="", help="another build of libhimo_amd.so whose v1 entry points are timed beside this build's")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from himo_amd import _lib
    from himo_amd.accumulate import AccumParams, capacity_for
    from himo_amd.synthetic import lidar_rings
    dev = _lib.require_gpu()
    lib = _lib.load()
    libs = {"this build": lib}
    if a.baseline_lib:
        other = ctypes.CDLL(a.baseline_lib)
        for name in V1:
            getattr(other, name).restype, getattr(other, name).argtypes = _lib.SIGNATURES[name]
        libs["baseline"] = other
    rng = np.random.default_rng(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def pose(k):                                                   # 1 m and 0.3 degrees a sweep, as scripts/exp_accumulate.py
        yaw = np.deg2rad(0.3) * k
        c, s = np.cos(yaw), np.sin(yaw)
        return np.array([[c, -s, 0, 1.0 * k], [s, c, 0, 0.02 * k * k], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)

    n, t = a.points, a.sources - 1
    poses = [pose(k) for k in range(a.sources)]
    sweeps, motions, labels = [], [], []
    for k in range(a.sources):
        rows = np.zeros((n, 4), np.float32)
        rows[:, :3] = lidar_rings(rng, n)
        sweeps.append(rows)
    for k in range(a.sources):                                     # (drawn after every sweep: the rows are those of exp_accumulate.py)
        sweeps[k][:, 3] = rng.uniform(0.0, 1.0, n)
        moving = rng.random((n, 1)) < 0.1
        motions.append(torch.from_numpy((rng.uniform(-2.0, 2.0, (n, 3)) * moving).astype(np.float32)).to(dev))
        labels.append(torch.from_numpy((rng.integers(1, 200, n) * moving[:, 0]).astype(np.int32)).to(dev))
        sweeps[k] = torch.from_numpy(sweeps[k]).to(dev)
    params = AccumParams()
    pp = ctypes.addressof(params)
    cap = capacity_for(a.sources * n)
    table = torch.empty(int(lib.himo_accum_table_bytes(cap)) // 4, dtype=torch.int32, device=dev)
    inv_t = np.linalg.inv(poses[t])
    Ts = [np.ascontiguousarray((inv_t @ poses[k]).astype(np.float32)).reshape(16) for k in range(a.sources)]
    Tp = [T.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for T in Ts]
    room = a.sources * n
    keys = torch.empty(room, dtype=torch.int32, device=dev)
    xyz = torch.empty((room, 3), dtype=torch.float32, device=dev)
    lag = torch.empty(room, dtype=torch.uint8, device=dev)
    cnt = torch.empty(room, dtype=torch.int32, device=dev)
    inten = torch.empty(room, dtype=torch.float32, device=dev)
    lab = torch.empty(room, dtype=torch.int32, device=dev)
    n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    stream = _lib.stream_handle()
    min2 = float(np.float32(0.05 * 0.05))

    def v1(which):
        h = libs[which]
        _lib.check(h.himo_accum_clear(table.data_ptr(), cap, stream), "clear")
        ev[0].record()
        for k in range(a.sources):
            _lib.check(h.himo_accum_insert(n, sweeps[k].data_ptr(), 4, None, Tp[k], t - k, pp, table.data_ptr(), cap, stream), "insert")
        ev[1].record()
        _lib.check(h.himo_accum_emit(table.data_ptr(), cap, pp, room, n_rows.data_ptr(), keys.data_ptr(), xyz.data_ptr(), lag.data_ptr(),
                                     cnt.data_ptr(), stream), "emit")
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), int(n_rows.item())

    def v2(_):
        _lib.check(lib.himo_accum_clear(table.data_ptr(), cap, stream), "clear")
        ev[0].record()
        for k in range(a.sources):
            _lib.check(lib.himo_accum_insert_ex(n, sweeps[k].data_ptr(), 4, None, Tp[k], t - k, pp, table.data_ptr(), cap, motions[k].data_ptr(), min2,
                                                sweeps[k].data_ptr() + 12, 4, 255.0, labels[k].data_ptr(), stream), "insert_ex")
        ev[1].record()
        _lib.check(lib.himo_accum_emit_ex(table.data_ptr(), cap, pp, room, n_rows.data_ptr(), keys.data_ptr(), xyz.data_ptr(), lag.data_ptr(),
                                          cnt.data_ptr(), 255.0, inten.data_ptr(), lab.data_ptr(), stream), "emit_ex")
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), int(n_rows.item())

    legs = [(name, v1) for name in libs] + [("v2", v2)]
    times = {name: ([], [], 0) for name, _ in legs}
    for rep in range(a.reps + 3):                                  # the legs take turns, so that drift of the clocks falls on all alike
        for name, fn in legs:
            ins, emit, rows_out = fn(name)
            if rep >= 3:
                times[name][0].append(ins)
                times[name][1].append(emit)
                times[name] = (times[name][0], times[name][1], rows_out)
    med = lambda v: float(np.median(v))                            # noqa: E731
    say(f"--- {a.sources} sources x {n} rows, pitch 4, as generated; grid 1024 x 1024 x 80 voxels of 0.1 m; table capacity {cap} slots; "
        f"{a.reps} timed repetitions after 3, the legs taking turns within a repetition")
    for name, _ in legs:
        ins, emit, rows_out = times[name]
        what = "v2: insert_ex (motion + intensity in place + label), emit_ex (both columns)" if name == "v2" else f"v1 entry points, {name}"
        say(f"{what}: rows out {rows_out}")
        say(f"  insert  median {med(ins):.3f} ms  min {min(ins):.3f}  max {max(ins):.3f}   ({a.sources} calls)")
        say(f"  emit    median {med(emit):.3f} ms  min {min(emit):.3f}  max {max(emit):.3f}")
    mine = times["this build"]
    if "baseline" in times:
        base = times["baseline"]
        say(f"(a) this build / baseline, v1 entry points: insert {med(mine[0]) / med(base[0]):.3f}, emit {med(mine[1]) / med(base[1]):.3f}, "
            f"insert + emit {(med(mine[0]) + med(mine[1])) / (med(base[0]) + med(base[1])):.3f}")
    say(f"(b) v2 / v1 of this build: insert {med(times['v2'][0]) / med(mine[0]):.3f}, emit {med(times['v2'][1]) / med(mine[1]):.3f}")
    # rule I for one sweep
    flow = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).to(dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ms = []
    for rep in range(a.reps + 3):
        ev[0].record()
        _lib.check(lib.himo_accum_motion(n, sweeps[0].data_ptr(), 4, flow.data_ptr(), Tp[0], out.data_ptr(), stream), "motion")
        ev[1].record()
        torch.cuda.synchronize()
        if rep >= 3:
            ms.append(ev[0].elapsed_time(ev[1]))
    say(f"himo_accum_motion, one sweep of {n} rows: median {med(ms):.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}   ({40 * n / med(ms) / 1e6:.0f} GB/s: "
        f"16 + 12 B a row read, 12 written)")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
