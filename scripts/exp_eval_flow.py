"""Measurements behind profiles/eval_flow.txt (GPU box, repo root).

    python scripts/exp_eval_flow.py kernel [R ...]   32 sweeps x 120 000 points resident on the device through
                                                     himo_flow_metrics_batch with R result names (default 1 and 4): warm-up, then
                                                     the median HIP-event time of 30 launches (prep launch included) and the
                                                     achieved bytes/s at 31 + 12 R bytes per point.
    python scripts/exp_eval_flow.py program DIR      write a synthetic .h5 directory (4 scenes x 33 sweeps x 120 000 points, one
                                                     stored result) under DIR/av2 and run ``eval_flow.main`` over it twice with
                                                     ``<stored>,raw`` (second pass: page cache warm): sweeps/s of the loop.
"""
from __future__ import annotations

import pickle
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def sweep(rng, n, names):
    """a sweep shaped like a real one: nine points in ten are static background, the rest spread over classes and speeds"""
    rad, th = rng.uniform(2, 45, n), rng.uniform(0, 2 * np.pi, n)
    pc0 = np.stack([rad * np.cos(th), rad * np.sin(th), rng.uniform(-2, 3, n), rng.random(n)], axis=1).astype(np.float32)
    moving = rng.random(n) < 0.1
    cat = np.where(moving | (rng.random(n) < 0.05), rng.integers(1, 31, n), 0).astype(np.uint8)
    speed = np.where(moving, rng.uniform(0.0, 2.5, n), rng.uniform(0.0, 0.02, n))
    d = rng.normal(size=(n, 3))
    flow = (speed[:, None] * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    f = {"pc0": pc0, "flow": flow, "flow_category_indices": cat, "gm0": rng.random(n) < 0.3, "flow_is_valid": np.ones(n, np.uint8),
         "pose0": np.eye(4), "pose1": np.eye(4)}
    for name in names:
        f[name] = (flow + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    return f


def kernel(rs=(1, 4), sweeps: int = 32, points: int = 120_000, launches: int = 30):
    import torch
    from himo_amd import _lib
    from himo_amd.eval_flow import FlowBatch, FlowMetrics
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    names = [f"flow_{k}" for k in range(max(rs))]
    frames = [sweep(rng, points, names) for _ in range(sweeps)]
    for r in rs:
        m = FlowMetrics(names[:r], "av2")
        batch = FlowBatch.from_frames(frames, names[:r])
        for _ in range(5):
            m.add_batch(batch)
        torch.cuda.synchronize()
        ms = []
        for _ in range(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            m.add_batch(batch)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        counted = int(m.buckets[0, :, :, 0].sum()) // (launches + 5)
        n = sweeps * points
        med, best = float(np.median(ms)), float(np.min(ms))
        nbytes = (31 + 12 * r) * n
        print(f"flow_metrics_kernel R={r} T={n} ({counted} points in buckets per launch): median {med * 1e3:.1f} us, min {best * 1e3:.1f} us over "
              f"{launches} launches (HIP events around prep + zeroing + kernel); {31 + 12 * r} B/point = {nbytes / 1e6:.1f} MB -> "
              f"{nbytes / med / 1e9:.2f} TB/s at the median", flush=True)


def program(root: Path, scenes: int = 4, sweeps: int = 33, points: int = 120_000):
    from himo_amd import eval_flow, h5lite
    root = root / "av2"
    root.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(0)
    index, per_sweep = [], 0
    t0 = time.perf_counter()
    for s in range(scenes):
        tree = {}
        for k in range(sweeps):
            ts = str(1000 * s + k)
            f = sweep(rng, points, ["flow_a"])
            tree[ts] = {"lidar": f["pc0"], "pose": f["pose0"], "ground_mask": f["gm0"], "flow": f["flow"], "flow_is_valid": f["flow_is_valid"],
                        "flow_category_indices": f["flow_category_indices"], "flow_a": f["flow_a"]}
            per_sweep = sum(np.asarray(v).nbytes for v in tree[ts].values())
            index.append([f"scene{s}", ts])
        h5lite.write_file(root / f"scene{s}.h5", tree)
    evaluable = [e for e in index if int(e[1]) % 1000 != sweeps - 1]           # (the last sweep of a scene has no successor pose)
    for name, entries in (("index_total.pkl", index), ("index_eval.pkl", evaluable)):
        with open(root / name, "wb") as fh:
            pickle.dump(entries, fh)
    print(f"wrote {len(index)} sweeps of {points} points in {time.perf_counter() - t0:.1f} s", flush=True)
    for label in ("first pass", "second pass"):
        t0 = time.perf_counter()
        m = eval_flow.main(str(root), res_names="flow_a,raw")
        wall = time.perf_counter() - t0
        print(f"{label}: {m.loop['sweeps']} sweeps, loop {m.loop['seconds']:.2f} s = {m.loop['sweeps'] / m.loop['seconds']:.0f} sweeps/s "
              f"(main() wall {wall:.2f} s); {per_sweep / 1e6:.2f} MB read per sweep", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel(tuple(int(v) for v in sys.argv[2:]) or (1, 4))
    else:
        program(Path(sys.argv[2]))
