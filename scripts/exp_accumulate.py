"""Timing of the sweep accumulator (himo_amd/csrc/accumulate.hip): one target of 11 sources x 120 000 rows of the synthetic "rings"
cloud at the default grid -- clear, the 11 inserts and the emit each between HIP events on the launch stream, then the whole
``accumulate_target`` call (sort, gathers and the one host wait included) by the host clock -- against the stage's algorithmic bytes:
per row 4 * pitch bytes read and, for every run of neighbouring lanes in one voxel, a 32-byte slot touched by five atomics; per slot 32
bytes cleared and 24 read by the emit; per output row 21 bytes written.  Prints times, rows in and out, and achieved bytes/s; gates
nothing.

    python scripts/exp_accumulate.py [--sources 11] [--points 120000] [--pitch 4] [--reps 30] [--out profiles/accumulate.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=11)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--pitch", type=int, default=4, choices=(3, 4))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from himo_amd import _lib
    from himo_amd.accumulate import Accumulator, AccumParams, accumulate_target, capacity_for
    from himo_amd.synthetic import lidar_rings
    dev = _lib.require_gpu()
    rng = np.random.default_rng(0)
    lines = []

    def say(s):
        print(s)
        lines.append(s)

    def pose(k):                                                   # 1 m and 0.3 degrees a sweep
        yaw = np.deg2rad(0.3) * k
        c, s = np.cos(yaw), np.sin(yaw)
        return np.array([[c, -s, 0, 1.0 * k], [s, c, 0, 0.02 * k * k], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)

    poses = [pose(k) for k in range(a.sources)]
    for order in ("as generated (rows of a sweep in random order)", "sorted by azimuth (rows that follow each other are neighbours)"):
        sweeps = []
        for k in range(a.sources):
            pts = lidar_rings(rng, a.points)
            if order.startswith("sorted"):
                pts = pts[np.lexsort((np.hypot(pts[:, 0], pts[:, 1]), np.round(np.arctan2(pts[:, 1], pts[:, 0]), 2)))]
            rows = np.zeros((a.points, a.pitch), np.float32)
            rows[:, :3] = pts
            sweeps.append(torch.from_numpy(rows).to(dev))
        t = a.sources - 1
        params = AccumParams()
        cap = capacity_for(a.sources * a.points)
        acc = Accumulator(dev, params, cap)
        inv_t = np.linalg.inv(poses[t])
        Ts = [(inv_t @ poses[k]).astype(np.float32) for k in range(a.sources)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        clear_ms, insert_ms, emit_ms, wall_ms = [], [], [], []
        rows_out = 0
        for rep in range(a.reps + 3):
            ev[0].record()
            acc.clear()
            ev[1].record()
            for k in range(a.sources):
                acc.add(sweeps[k], Ts[k], t - k)
            ev[2].record()
            out = acc.result()                                     # emit, the host wait, the sort and the gathers
            ev[3].record()
            torch.cuda.synchronize()
            rows_out = int(out[0].shape[0])
            if rep >= 3:
                clear_ms.append(ev[0].elapsed_time(ev[1]))
                insert_ms.append(ev[1].elapsed_time(ev[2]))
        # the emit alone: the kernel between events, the table as the last insert left it
        import ctypes
        keys = torch.empty(acc.rows, dtype=torch.int32, device=dev)
        xyz = torch.empty((acc.rows, 3), dtype=torch.float32, device=dev)
        lag = torch.empty(acc.rows, dtype=torch.uint8, device=dev)
        cnt = torch.empty(acc.rows, dtype=torch.int32, device=dev)
        n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
        for rep in range(a.reps + 3):
            ev[0].record()
            _lib.check(acc.lib.himo_accum_emit(_lib.ptr(acc.table), cap, ctypes.addressof(params), acc.rows, _lib.ptr(n_rows), _lib.ptr(keys),
                                               _lib.ptr(xyz), _lib.ptr(lag), _lib.ptr(cnt), _lib.stream_handle()), "himo_accum_emit")
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 3:
                emit_ms.append(ev[0].elapsed_time(ev[1]))
        for rep in range(a.reps + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            accumulate_target(sweeps, poses, t, a.sources - 1, acc=acc)
            torch.cuda.synchronize()
            if rep >= 3:
                wall_ms.append(1e3 * (time.perf_counter() - t0))
        rows_in = a.sources * a.points
        med = lambda v: float(np.median(v))                        # noqa: E731
        say(f"--- {a.sources} sources x {a.points} rows, pitch {a.pitch}, {order}")
        say(f"grid 1024 x 1024 x 80 voxels of 0.1 m; table capacity {cap} slots ({acc.table.numel() * 4 / 2**20:.0f} MiB); rows in {rows_in}, "
            f"rows out {rows_out}; {a.reps} timed repetitions after 3")
        say(f"clear   median {med(clear_ms):.3f} ms  min {min(clear_ms):.3f}  max {max(clear_ms):.3f}   ({32 * (cap + 1) / med(clear_ms) / 1e6:.0f} GB/s written)")
        ins_bytes = rows_in * 4 * a.pitch
        say(f"insert  median {med(insert_ms):.3f} ms  min {min(insert_ms):.3f}  max {max(insert_ms):.3f}   ({a.sources} calls; {rows_in / med(insert_ms) / 1e6:.2f} G rows/s; "
            f"{ins_bytes / med(insert_ms) / 1e6:.0f} GB/s of rows read, slots not counted)")
        say(f"emit    median {med(emit_ms):.3f} ms  min {min(emit_ms):.3f}  max {max(emit_ms):.3f}   ({(24 * (cap + 1) + 21 * rows_out) / med(emit_ms) / 1e6:.0f} GB/s: 24 B a slot read, "
            f"21 B an output row written)")
        say(f"accumulate_target, host clock: median {med(wall_ms):.3f} ms  min {min(wall_ms):.3f}  max {max(wall_ms):.3f}   (clear, inserts, emit, one host wait, sort "
            f"of {rows_out} keys and four gathers)")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
