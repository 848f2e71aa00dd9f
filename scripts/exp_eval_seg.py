"""Measurements behind profiles/eval_seg.txt (GPU box, repo root).

    python scripts/exp_eval_seg.py kernel [R]        the 120 000 x 32 packed batch through himo_seg_confusion, R result names
                                                     (default 8): HIP-event time per launch and effective bandwidth.  The same
                                                     command under ``rocprofv3 --kernel-trace --stats`` / ``--pmc FETCH_SIZE``
                                                     (separate runs) gives the profiler's time and the fetched bytes.
    python scripts/exp_eval_seg.py program DIR       write a synthetic .h5 directory (8 scenes x 64 sweeps x 120 000 points,
                                                     seg_raw + seg_flow) under DIR and run ``eval_seg.main`` over it twice
                                                     (second pass: page cache warm): sweeps/s of the evaluation loop.
"""
from __future__ import annotations

import pickle
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def kernel(r: int = 8, launches: int = 50):
    import torch
    from himo_amd import _lib
    from himo_amd.eval_seg import class_lut, seg_confusion
    dev = _lib.require_gpu()
    n = 120_000 * 32
    g = torch.Generator(device="cpu").manual_seed(0)
    mk = lambda hi: torch.randint(0, hi, (n,), dtype=torch.uint8, generator=g).to(dev)          # noqa: E731
    gt, valid, preds = mk(31), mk(2), [mk(31) for _ in range(r)]
    conf = torch.zeros((r, 2, 3, 3), dtype=torch.int64, device=dev)
    lut = class_lut()
    for _ in range(5):
        seg_confusion(conf, gt, preds, valid, lut)
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        seg_confusion(conf, gt, preds, valid, lut)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    assert int(conf[:, 0].sum()) == r * n * (launches + 5)
    med, best = float(np.median(ms)), float(np.min(ms))
    nbytes = (r + 2) * n
    print(f"seg_confusion_kernel R={r} T={n}: median {med * 1e3:.1f} us, min {best * 1e3:.1f} us over {launches} launches (HIP events); "
          f"algorithmic {(r + 2)} B/point = {nbytes / 1e6:.1f} MB -> {nbytes / med / 1e6:.0f} GB/s at the median")


def program(root: Path, scenes: int = 8, sweeps: int = 64, points: int = 120_000):
    from himo_amd import eval_seg, h5lite
    root.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(0)
    index = []
    t0 = time.perf_counter()
    for s in range(scenes):
        tree = {}
        for k in range(sweeps):
            ts = str(1000 * s + k)
            gt = rng.integers(0, 31, points).astype(np.uint8)
            tree[ts] = {"flow_category_indices": gt, "seg_valid": rng.random(points) < 0.7,
                        "seg_raw": np.where(rng.random(points) < 0.6, gt, 0).astype(np.uint8),
                        "seg_flow": np.where(rng.random(points) < 0.85, gt, 0).astype(np.uint8)}
            index.append([f"scene{s}", ts])
        h5lite.write_file(root / f"scene{s}.h5", tree)
    for name in ("index_total.pkl", "index_eval.pkl"):
        with open(root / name, "wb") as fh:
            pickle.dump(index, fh)
    print(f"wrote {len(index)} sweeps of {points} points in {time.perf_counter() - t0:.1f} s")
    for label in ("first pass", "second pass"):
        t0 = time.perf_counter()
        m = eval_seg.main(str(root), res_names=["seg_raw", "seg_flow"], both=True)
        wall = time.perf_counter() - t0
        print(f"{label}: {m.loop['sweeps']} sweeps, loop {m.loop['seconds']:.2f} s = {m.loop['sweeps'] / m.loop['seconds']:.0f} sweeps/s "
              f"(main() wall {wall:.2f} s); {4 * points / 1e6:.2f} MB read per sweep")


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    else:
        program(Path(sys.argv[2]))
