"""Measurements behind profiles/eval_flow_accuracy.txt (GPU box, repo root).

    python scripts/exp_eval_flow_accuracy.py kernel [--parent_lib PATH] [R ...]
        32 sweeps x 120 000 points resident on the device (the shape of profiles/eval_flow.txt), R result names (default 1 and 4).
        Timed per build and mode in windows: synchronise, a device event, 20 launches, a device event, synchronise -> us per launch
        (transform prep launch + kernel).  The windows of the builds and modes ALTERNATE, 10 of each:
          v1      himo_flow_metrics_batch of this build
          parent  himo_flow_metrics_batch of the library at PATH (the parent commit's build), when given
          acc     himo_flow_metrics_batch_ex, full mode, accuracy table on
          res     himo_flow_metrics_batch_ex, residual mode on rows of pitch 4, accuracy table on
        Every other round runs them in the reverse order, so that no build always follows the same neighbour.
        The margin for "v1 is no slower than parent" is the spread between the parent's own windows.
"""
from __future__ import annotations

import ctypes
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from exp_eval_flow import sweep  # noqa: E402


def kernel(rs=(1, 4), parent_lib=None, sweeps: int = 32, points: int = 120_000, launches: int = 20, repeats: int = 10):
    import torch
    from himo_amd import _lib
    from himo_amd.eval_flow import FlowBatch, class_lut
    dev = _lib.require_gpu()
    lib = _lib.load()
    libs = {"v1": lib}
    if parent_lib:
        parent = ctypes.CDLL(str(parent_lib))
        res, args = _lib.SIGNATURES["himo_flow_metrics_batch"]
        parent.himo_flow_metrics_batch.restype, parent.himo_flow_metrics_batch.argtypes = res, args
        libs["parent"] = parent
    rng = np.random.default_rng(0)
    names = [f"flow_{k}" for k in range(max(rs))]
    frames = [sweep(rng, points, names) for _ in range(sweeps)]
    lut = class_lut().ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    for r in rs:
        b = FlowBatch.from_frames(frames, names[:r], device=dev)
        z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)      # noqa: E731
        bk, tw, rj, ac = z(r, 5, 51, 3), z(b.sweeps, r, 3, 2), z(r), z(r, 4, 3)
        ws = torch.empty(int(lib.himo_flow_metrics_workspace_bytes(b.sweeps)) + 16, dtype=torch.uint8, device=dev)
        wide = []
        for e in b.ests:                                           # the same values as rows of pitch 4 (what a trainer's head leaves)
            w = torch.zeros((b.total_points, 4), dtype=torch.float32, device=dev)
            w[:, :3] = e
            wide.append(w)
        p3 = (ctypes.c_void_p * r)(*[_lib.ptr(e) for e in b.ests])
        p4 = (ctypes.c_void_p * r)(*[_lib.ptr(w) for w in wide])
        head = (b.sweeps, b.total_points, _lib.ptr(b.offsets), _lib.ptr(b.pose0), _lib.ptr(b.pose1), _lib.ptr(b.pc0), int(b.pc0.stride(0)), _lib.ptr(b.gt))
        mid = (_lib.ptr(b.category), _lib.ptr(b.ground), None, lut, 0.1)
        tables = (_lib.ptr(bk), _lib.ptr(tw), _lib.ptr(rj))
        tail = (_lib.ptr(ws), _lib.stream_handle())

        def v1(which):
            return lambda: which.himo_flow_metrics_batch(*head, p3, r, *mid, 0, *tables, *tail)
        calls = {name: v1(which) for name, which in libs.items()}
        calls["acc"] = lambda: lib.himo_flow_metrics_batch_ex(*head, p3, r, 3, *mid, 0, *tables, _lib.ptr(ac), *tail)
        calls["res"] = lambda: lib.himo_flow_metrics_batch_ex(*head, p4, r, 4, *mid, _lib.FLAG_EST_RESIDUAL, *tables, _lib.ptr(ac), *tail)
        for call in calls.values():                                # warm-up
            for _ in range(5):
                _lib.check(call(), "warm-up")
        torch.cuda.synchronize()
        us = {name: [] for name in calls}
        for k in range(repeats):
            order = list(calls.items())
            for name, call in (order if k % 2 == 0 else order[::-1]):      # the builds and modes alternate, forwards then backwards
                torch.cuda.synchronize()
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    call()
                e.record()
                e.synchronize()
                us[name].append(a.elapsed_time(e) * 1e3 / launches)
        for name, v in us.items():
            print(f"R={r} {name:<6} median {np.median(v):7.1f} us  min {min(v):7.1f}  max {max(v):7.1f}  windows of {launches} launches: "
                  + " ".join(f"{x:.1f}" for x in v), flush=True)
        if "parent" in us:
            lo, hi, med = min(us["parent"]), max(us["parent"]), float(np.median(us["v1"]))
            print(f"R={r} v1 median {med:.1f} us {'inside' if med <= hi else 'ABOVE'} the parent's own spread {lo:.1f} .. {hi:.1f} us", flush=True)


if __name__ == "__main__":
    argv = sys.argv[2:]
    parent_lib = None
    if "--parent_lib" in argv:
        k = argv.index("--parent_lib")
        parent_lib = argv[k + 1]
        del argv[k:k + 2]
    kernel(tuple(int(v) for v in argv) or (1, 4), parent_lib=parent_lib)
