"""Timing of the whole-drive free-space map (himo_amd/drivemap.py, csrc/drivemap.hip) on one synthetic scene of 150 sweeps x 120 000
points (``make_scene``, LiDAR-shaped rings): the carve and the query of every sweep, the emit, the clear, the map's size -- and, in the
same process and taking turns with it, ``raymap.dynamic_flags`` ("free-space ray map, v1", window 5) over the same scene, which walks
every sweep up to ten times where this stage walks it once but pays a 64-bit compare-and-swap per mark where v1 pays a 32-bit OR.
Flags only: the clustering behind them is the same call in both programs.  Host clock round work that ends in a synchronise for the
whole-scene figures, device events round every call for the per-sweep ones, the library's event scopes for the kernels, in a pass of
their own.  Sets no bar.

    python scripts/exp_drivemap.py [OUT] [SWEEPS] [POINTS]     # OUT: the file the lines are also written to (profiles/drivemap.txt)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from himo_amd import _lib, raymap                                            # noqa: E402
from himo_amd.drivemap import DriveMap, carve_drive, relative_poses, scene_extent      # noqa: E402
from himo_amd.synthetic import make_scene                                    # noqa: E402

TURNS = 3
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def stats(ms):
    ms = sorted(ms)
    return f"{ms[len(ms) // 2]:.4f} ms (min {ms[0]:.4f} max {ms[-1]:.4f})"


def main():
    n_sweeps = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    n_points = int(sys.argv[3]) if len(sys.argv) > 3 else 120_000
    dev = _lib.require_gpu()
    frames = make_scene(7, n_sweeps, n_points=n_points, cloud="rings")
    poses = [f["pose0"] for f in frames]
    sweeps = [raymap._device_points(f["pc0"], dev) for f in frames]
    masks = [torch.from_numpy(f["gm0"].astype(np.uint8)).to(dev) for f in frames]
    p = scene_extent(poses)
    T = relative_poses(poses)
    dm = DriveMap(p, dev)
    grid = raymap.new_map(raymap.RaymapParams(), dev)
    say(f"{n_sweeps} sweeps x {n_points} points; the drive's map {p.nx} x {p.ny} x {p.nz} voxels of {p.voxel:g} m = "
        f"{8.0 * p.nx * p.ny * p.nz / 2 ** 20:.1f} MiB (v1: 512 x 512 x 30 = 30.0 MiB, cleared per target)")

    def drive():
        dm.clear()
        moved, _ = carve_drive(dm, sweeps, T)
        return [dm.query(moved[k], masks[k])[0] for k in range(n_sweeps)]

    def v1():
        return [raymap.dynamic_flags(sweeps, poses, masks, t, window=5, grid=grid)[0] for t in range(n_sweeps)]

    # whole-scene flags, the two programs taking turns: one warm-up each, then TURNS timed turns
    seconds = {"drive": [], "v1": []}
    for turn in range(TURNS + 1):
        for name, fn in (("drive", drive), ("v1", v1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flags = fn()
            torch.cuda.synchronize()
            if turn:
                seconds[name].append(time.perf_counter() - t0)
            if turn == TURNS:
                share = sum(int(f.sum().item()) for f in flags) / (n_sweeps * n_points)
                say(f"  {name:5s}: {100.0 * share:.2f} % of the points DYNAMIC (ground skipped)")
    d, v = sorted(seconds["drive"])[TURNS // 2], sorted(seconds["v1"])[TURNS // 2]
    say(f"whole-scene flags, host clock, median of {TURNS} turns: whole drive {d:.3f} s ({n_sweeps / d:.1f} sweeps/s; all {['%.3f' % x for x in seconds['drive']]}), "
        f"v1 at window 5 {v:.3f} s ({n_sweeps / v:.1f} sweeps/s; all {['%.3f' % x for x in seconds['v1']]}): v1 / whole drive = {v / d:.2f}")

    # per call, device events
    ev = lambda: torch.cuda.Event(enable_timing=True)
    carve_ms, query_ms, clear_ms, emit_ms = [], [], [], []
    from himo_amd.seflow.ssl_label import _moved
    moved = [_moved(sweeps[k], np.asarray(T[k], np.float32)) for k in range(n_sweeps)]
    src = torch.zeros(n_points, dtype=torch.uint8, device=dev)
    tables = []
    for k in range(n_sweeps):
        t = np.zeros((16, 3), np.float32)
        t[0] = np.asarray(T[k], np.float32)[:3, 3]
        tables.append(torch.from_numpy(t).to(dev))
    for turn in range(TURNS + 1):
        a, b = ev(), ev()
        a.record()
        dm.clear()
        b.record()
        pairs = []
        for k in range(n_sweeps):
            a2, b2 = ev(), ev()
            a2.record()
            dm.carve(moved[k], src, tables[k], k)
            b2.record()
            pairs.append((a2, b2))
        qpairs = []
        for k in range(n_sweeps):
            a2, b2 = ev(), ev()
            a2.record()
            dm.query(moved[k], masks[k])
            b2.record()
            qpairs.append((a2, b2))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, hits, free = dm.emit()
        torch.cuda.synchronize()
        if turn:
            clear_ms.append(a.elapsed_time(b))
            carve_ms += [x.elapsed_time(y) for x, y in pairs]
            query_ms += [x.elapsed_time(y) for x, y in qpairs]
            emit_ms.append(1e3 * (time.perf_counter() - t0))
    say(f"himo_drivemap_carve, one sweep of {n_points} rays (src check + walk): {stats(carve_ms)} over {len(carve_ms)} calls")
    say(f"himo_drivemap_query, one sweep of {n_points} points:                {stats(query_ms)} over {len(query_ms)} calls")
    say(f"the clear (zeroing the map):                                       {stats(clear_ms)}")
    say(f"DriveMap.emit (count call, allocation, write call; host clock):    {stats(emit_ms)} -> {len(rows)} STATIC voxels")

    # the kernels by the library's event scopes, a pass of their own
    _lib.prof_start("drivemap")
    dm.clear()
    for k in range(n_sweeps):
        dm.carve(moved[k], src, tables[k], k)
    for k in range(n_sweeps):
        dm.query(moved[k], masks[k])
    dm.emit()
    torch.cuda.synchronize()
    prof = _lib.prof_stop()
    for name in sorted(prof):
        s = prof[name]
        say(f"  {name}: {1e3 * s['avg_ms']:.1f} us avg (min {1e3 * s['min_ms']:.1f}, max {1e3 * s['max_ms']:.1f}) over {s['count']}")
    _lib.prof_start("raymap")
    targets = list(range(0, n_sweeps, max(n_sweeps // 15, 1)))
    for t in targets:
        raymap.dynamic_flags(sweeps, poses, masks, t, window=5, grid=grid)
    torch.cuda.synchronize()
    prof1 = _lib.prof_stop()
    for name in sorted(prof1):
        s = prof1[name]
        say(f"  {name}: {1e3 * s['avg_ms']:.1f} us avg (min {1e3 * s['min_ms']:.1f}, max {1e3 * s['max_ms']:.1f}) over {s['count']} ({len(targets)} targets)")
    if "drivemap_carve_kernel" in prof and "raymap_carve_kernel" in prof1:
        per_ray = 1e6 * prof["drivemap_carve_kernel"]["total_ms"] / (prof["drivemap_carve_kernel"]["count"] * n_points)
        rays1 = sum(len(raymap.neighbours(t, n_sweeps, 5)) for t in targets) * n_points
        per_ray1 = 1e6 * prof1["raymap_carve_kernel"]["total_ms"] / rays1
        say(f"carve kernel per ray: whole drive {per_ray:.3f} ns, v1 {per_ray1:.3f} ns: ratio {per_ray / per_ray1:.2f}")
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
