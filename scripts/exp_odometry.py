"""Timing of sweep odometry (himo_amd/odometry.py, csrc/odometry.hip): one 120 000-point synthetic sweep (``make_scene``, the clouds
``uniform`` and ``rings``) against the map of the 10 sweeps before it, built with the estimated poses.  Device events around every call, the
median (min, max) of 60 calls after 10 warm-ups: source build, map build, vote, binning, one step (its two kernels also by the library's
event scopes, in a run of their own), the whole registration, and beside the fused step ``himo_rigid_transform`` + ``himo_nn_grid`` on the
same two sets in the same process (that composition rebins both sets and computes no sums).  Sets no bar.

    python scripts/exp_odometry.py [OUT]          # OUT: the file the lines are also written to (profiles/odometry.txt)
"""
import ctypes
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from himo_amd import _lib                                                   # noqa: E402
from himo_amd.accumulate import Accumulator, accumulate_target, capacity_for, device_rows      # noqa: E402
from himo_amd.odometry import SweepOdometry, as44                              # noqa: E402
import himo_amd.seflow.ssl_label                                             # noqa: E402,F401  (registers himo_rigid_transform)
from himo_amd.ssl_loss import GRID_CELL, GRID_H, GRID_W, GRID_X0, GRID_Y0     # noqa: E402
from himo_amd.synthetic import make_scene                                    # noqa: E402

REPS, WARM = 60, 10
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def timed(fn, before=None):
    for _ in range(WARM):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    a = [torch.cuda.Event(enable_timing=True) for _ in range(REPS)]
    b = [torch.cuda.Event(enable_timing=True) for _ in range(REPS)]
    for i in range(REPS):
        if before:
            before()
        a[i].record()
        fn()
        b[i].record()
    torch.cuda.synchronize()
    ms = sorted(x.elapsed_time(y) for x, y in zip(a, b))
    return ms[len(ms) // 2], ms[0], ms[-1]


def main(cloud):
    dev = _lib.require_gpu()
    lib, P, s = _lib.load(), _lib.ptr, _lib.stream_handle
    frames = make_scene(5, 12, n_points=120_000, n_instances=30, cloud=cloud)
    odo = SweepOdometry(dev)
    sweeps = [device_rows(f["pc0"], dev) for f in frames]
    # the estimated chain of the first 11 sweeps, so that the map is what the program would have built
    t0 = time.perf_counter()
    poses, regs = odo.scene(sweeps[:11], None, frames[0]["pose0"])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    gt = np.stack([f["pose0"] for f in frames[:11]])
    from himo_amd.odometry import rpe_table
    r = rpe_table(poses, gt)
    say(f"[{cloud}] scene of 11 x 120k-point sweeps: {wall / 10 * 1e3:.2f} ms wall per sweep (both accumulations, vote where used, registration, host "
        f"waits); iterations {[x.iters for x in regs]}, inlier share {np.mean([x.share for x in regs]):.3f}, RPE max {r['t_max']:.4f} m "
        f"{r['r_max']:.4f} deg, all accepted {all(x.accepted for x in regs)}")
    k = 11
    eye = np.eye(4)
    acc_src = Accumulator(dev, odo._accum, capacity_for(120_000))
    acc_map = Accumulator(dev, odo._accum, capacity_for(10 * 120_000))
    poses = list(poses) + [poses[-1] @ regs[-1].T44]
    build_src = lambda: accumulate_target([sweeps[k]], [eye], 0, 0, acc=acc_src)[0]                       # noqa: E731
    build_map = lambda: accumulate_target(sweeps[:k], poses[:k], k - 1, 9, acc=acc_map)[0]                # noqa: E731
    S, M = build_src().contiguous(), build_map().contiguous()
    n, m = int(S.shape[0]), int(M.shape[0])
    say(f"[{cloud}] source {n} centroids of 120000 rows, map {m} centroids of 10 sweeps")
    say(f"[{cloud}] source build   {'%.3f ms (min %.3f max %.3f)' % timed(build_src)}   (one host wait inside)")
    say(f"[{cloud}] map build      {'%.3f ms (min %.3f max %.3f)' % timed(build_map)}   (one host wait inside)")
    say(f"[{cloud}] vote           {'%.3f ms (min %.3f max %.3f)' % timed(lambda: odo.vote(S, M))}")
    c = ctypes.addressof(odo._c)
    ws = odo.workspace(m)
    binning = lambda: _lib.check(lib.himo_odom_map(m, P(M), c, P(ws), ws.numel(), s()), "map")          # noqa: E731
    say(f"[{cloud}] binning        {'%.3f ms (min %.3f max %.3f)' % timed(binning)}")
    T0 = regs[-1].T44[:3]
    step = lambda: _lib.check(lib.himo_odom_step(n, P(S), 3, m, P(M), c, P(odo.state), None, None, P(ws), ws.numel(), s()), "step")   # noqa: E731
    t_step = timed(step, before=lambda: odo.init_state(T0))
    say(f"[{cloud}] one step       {'%.3f ms (min %.3f max %.3f)' % t_step}   (step kernel + reduce/solve kernel)")
    _lib.prof_start("odom_")
    for _ in range(20):
        odo.init_state(T0)
        step()
    prof = _lib.prof_stop()
    for name, v in sorted(prof.items()):
        say(f"[{cloud}]   {name}: {v['avg_ms'] * 1e3:.1f} us avg (min {v['min_ms'] * 1e3:.1f}) over {v['count']}")
    kern = prof.get("odom_step_kernel", {}).get("min_ms")
    if kern:
        # compulsory traffic: the source rows, every binned map row once, the neighbour gather, the cell offsets
        byts = n * 12 + m * 16 + n * 12 + odo._c.gw * odo._c.gh * 4
        say(f"[{cloud}]   step kernel: {byts / 1e6:.2f} MB compulsory -> {byts / (kern * 1e-3) / 1e12:.3f} TB/s achieved (HBM: 8.0 TB/s peak, 6.29 TB/s "
            "measured copy rate)")
    reg = lambda: _lib.check(lib.himo_odom_register(n, P(S), 3, m, P(M), c, P(odo.state), P(ws), ws.numel(), s()), "register")      # noqa: E731
    t_reg = timed(reg, before=lambda: odo.init_state(T0))
    odo.init_state(T0)
    reg()
    res = odo.result(n)
    say(f"[{cloud}] registration   {'%.3f ms (min %.3f max %.3f)' % t_reg}   (binning + 20 enqueued steps; {res.iters} ran, status {res.status}, "
        f"{res.pairs}/{n} pairs)")
    # the composition the fused step replaces: himo_rigid_transform + himo_nn_grid on the same two sets (rebins both, no sums)
    nn_ws = torch.empty(int(lib.himo_nn_grid_workspace_bytes(max(n, m, 1), GRID_W, GRID_H)), dtype=torch.uint8, device=dev)
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    T32 = torch.from_numpy(np.ascontiguousarray(as44(T0), dtype=np.float32)).to(dev)
    moved = torch.empty((n, 3), dtype=torch.float32, device=dev)

    def composed():
        _lib.check(lib.himo_rigid_transform(n, P(S), 3, P(T32), P(moved), 3, s()), "rigid")
        _lib.check(lib.himo_nn_grid(n, P(moved), m, P(M), GRID_X0, GRID_Y0, GRID_CELL, GRID_W, GRID_H, P(d2), P(idx), P(nn_ws), nn_ws.numel(), s()),
                   "nn_grid")
    t_comp = timed(composed)
    say(f"[{cloud}] rigid_transform + nn_grid {'%.3f ms (min %.3f max %.3f)' % t_comp}   -> the fused step is {t_step[0] / t_comp[0]:.2f} x of it")


if __name__ == "__main__":
    for cloud in ("uniform", "rings"):
        main(cloud)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text("\n".join(out) + "\n")
