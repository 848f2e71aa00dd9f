"""Measurements behind profiles/extract_sca.txt (GPU box, repo root).

    python scripts/exp_extract_sca.py kernel          32 sweeps x 120 000 points through himo_box_label_batch at 16, 128 and 512 boxes
                                                      per sweep: HIP-event time per launch and achieved bytes/s against the 34 B/point
                                                      design figure; compdis_gt_kernel on the same point count as the yardstick (73
                                                      B/point).  Under ``rocprofv3 --kernel-trace --stats`` (a run of its own) the same
                                                      command gives the profiler's times.
    python scripts/exp_extract_sca.py program DIR     write a synthetic raw tree (4 scenes x 9 superframes x 120 000 points, 64 boxes a
                                                      frame) under DIR and run ``extract_sca.main`` over it twice into fresh output
                                                      directories (second pass: raw files warm): sweeps/s.
    python scripts/exp_extract_sca.py cpu             tests/boxlabel_ref.py on one such sweep (numpy, the machine's threads as they are).
    python scripts/exp_extract_sca.py all DIR         every step above as a process of its own under ``timeout -k 10``, stopping at the
                                                      first that fails; the kernel step once plain and once under rocprofv3.
"""
from __future__ import annotations

import json
import pickle
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

POINTS, SWEEPS = 120_000, 32


def synthetic_sweep(seed: int, n: int, m: int):
    import boxlabel_ref
    rng = np.random.default_rng(seed)
    boxes = np.stack([rng.uniform(-60, 60, m), rng.uniform(-60, 60, m), rng.uniform(-1, 1, m), rng.uniform(2, 10, m), rng.uniform(1, 3, m),
                      rng.uniform(1, 3.5, m), rng.uniform(-np.pi, np.pi, m)], axis=1)
    pts = np.stack([rng.uniform(-75, 75, n), rng.uniform(-75, 75, n), rng.uniform(-2, 6, n), rng.uniform(0, 255, n)], axis=1).astype(np.float32)
    ego = np.eye(4)
    ego[:3, 3] = rng.uniform(-1, 1, 3)
    return pts, ego, (boxlabel_ref.box_constants(boxes), rng.uniform(-1, 1, (m, 3)).astype(np.float32), rng.integers(1, 31, m).astype(np.uint8),
                      np.ones(m, np.uint8))


def timed(fn, launches: int = 30):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def kernel():
    import torch
    from himo_amd import _lib
    from himo_amd.compdis import CompDisEngine, FrameBatch
    from himo_amd.extract_sca import LabelBatch, label_batch, out_layout
    from himo_amd.synthetic import make_frame
    dev = _lib.require_gpu()
    T = POINTS * SWEEPS
    for m in (16, 128, 512):
        batch = LabelBatch([synthetic_sweep(100 * m + k, POINTS, m) for k in range(SWEEPS)], 0, device=dev)
        out = torch.empty(out_layout(T)[1], dtype=torch.uint8, device=dev)
        med, best = timed(lambda: label_batch(batch, out))
        inst = out.cpu().numpy()[out_layout(T)[0][1]:][:4 * T].view(np.uint32)
        print(f"box_label_kernel {SWEEPS} x {POINTS} points, {m} boxes/sweep: median {med * 1e3:.0f} us, min {best * 1e3:.0f} us (HIP events); "
              f"34 B/point = {34 * T / 1e6:.0f} MB -> {34 * T / med / 1e6:.0f} GB/s; {T * m / med / 1e6:.1f} G (point, box) pairs/s; "
              f"{100.0 * (inst > 0).mean():.1f} % of points in a box")
    frames = [make_frame(k, n_points=POINTS) for k in range(SWEEPS)]
    fb = FrameBatch.from_frames(frames, "flow", with_masks=True, with_labels=True, host_ego=True)
    eng = CompDisEngine(max_frames=SWEEPS)
    med, best = timed(lambda: eng.run_gt(fb, "av2"))
    print(f"compdis_gt (frame_prep + compdis_gt_kernel + body allocation) on the same {T} points: median {med * 1e3:.0f} us, min {best * 1e3:.0f} us; "
          f"73 B/point = {73 * T / 1e6:.0f} MB -> {73 * T / med / 1e6:.0f} GB/s")


def write_raw(root: Path, scenes: int = 4, frames: int = 9, boxes: int = 64):
    rng = np.random.default_rng(0)
    lidars = [f"lidar_{k}" for k in range(6)]
    metadata = []
    for s in range(scenes):
        scene = f"batch_{s + 1}"
        seq = {"vehicle": "Bench", "lidars": {f"lidar{k}": {"name": n} for k, n in enumerate(lidars)}, "superframes": []}
        for j in range(frames):
            m = boxes
            speed = rng.uniform(0, 12, m)
            ang = rng.uniform(-np.pi, np.pi, m)
            metadata.append({"sample_idx": scene, "annos": {
                "location": np.stack([rng.uniform(-60, 60, m), rng.uniform(-60, 60, m), rng.uniform(0.5, 1.5, m)], axis=1),
                "dimensions": np.stack([rng.uniform(2, 10, m), rng.uniform(1, 3, m), rng.uniform(1, 3.5, m)], axis=1),
                "heading": rng.uniform(-np.pi, np.pi, m), "speed": speed, "velocity": np.stack([speed * np.cos(ang), speed * np.sin(ang)], axis=1),
                "name": ["Car"] * m, "mean_delta_t": np.zeros(m)}})
            seq["superframes"].append({"timestamp_epoch_ns": str(10**18 + s * 10**10 + j * 10**8),
                                       "smoothPosition": {"smothYaw_rad": 0.01 * j, "smoothX_m": 1.2 * j, "smoothY_m": 0.1 * j}})
            name = f"superframe_{j + 1:04d}"
            d = root / scene / name
            d.mkdir(parents=True, exist_ok=True)
            for attr, lo, hi in (("X", -75, 75), ("Y", -75, 75), ("Z", -2, 6), ("W", 0, 255)):
                rng.uniform(lo, hi, POINTS).astype(np.float32).tofile(d / f"{name}_{attr}.bin")
            rng.integers(1, 7, POINTS).astype(np.int8).tofile(d / f"{name}_sensor.bin")
            rng.integers(0, 10**8, POINTS).astype(np.int32).tofile(d / f"{name}_deltaT.bin")
        (root / scene / f"sequence_{s + 1}.json").write_text(json.dumps(seq))
    with open(root / "metadata.pkl", "wb") as fh:
        pickle.dump(metadata, fh)
    ext = ["parameters:"]
    for k, n in enumerate(lidars):
        ext += [f"  lidarArray_arrayEl{k}:", f"    humanReadableReference: {n}", "    nominalPosition:", f"      x: {k}.0", "      y: 0.5", "      z: 2.0"]
    (root / "bench-generated.yml").write_text("\n".join(ext) + "\n")
    (root / "names.json").write_text(json.dumps({"Car": "REGULAR_VEHICLE", "none": "NONE"}))
    return scenes * frames


def program(root: Path, readers: int = 8):
    from himo_amd import extract_sca
    t0 = time.perf_counter()
    sweeps = write_raw(root / "raw")
    print(f"wrote {sweeps} superframes of {POINTS} points in {time.perf_counter() - t0:.1f} s")
    for label in ("first pass", "second pass (raw files warm)"):
        out = root / f"out_{label.split()[0]}"
        t0 = time.perf_counter()
        extract_sca.main(str(root / "raw"), str(root / "raw" / "metadata.pkl"), str(out), nproc=readers, lidar_ext_dir=str(root / "raw"),
                         name_mapping=str(root / "raw" / "names.json"))
        wall = time.perf_counter() - t0
        print(f"{label}: {sweeps} sweeps in {wall:.2f} s = {sweeps / wall:.1f} sweeps/s ({readers} reader threads, 1 writer thread, "
              f"{sum(p.stat().st_size for p in out.glob('*.h5')) / 1e6:.0f} MB of h5 written)")


def cpu(boxes: int = 128):
    import boxlabel_ref
    pc, ego, table = synthetic_sweep(1, POINTS, boxes)
    boxlabel_ref.label_sweep(pc, ego, *table, 0)
    t0 = time.perf_counter()
    for _ in range(3):
        boxlabel_ref.label_sweep(pc, ego, *table, 0)
    print(f"tests/boxlabel_ref.label_sweep, one sweep of {POINTS} points x {boxes} boxes (numpy): {(time.perf_counter() - t0) / 3:.3f} s per sweep")


def everything(root: Path):
    me = [sys.executable, str(Path(__file__).resolve())]
    steps = [(["timeout", "-k", "10", "240"] + me + ["kernel"]),
             (["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", str(root / "rocprof"), "--"] + me + ["kernel"]),
             (["timeout", "-k", "10", "300"] + me + ["program", str(root)]),
             (["timeout", "-k", "10", "120"] + me + ["cpu"])]
    for cmd in steps:
        print("$", " ".join(cmd), flush=True)
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(rc)                      # nothing more starts on the device after a step that failed


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernel":
        kernel()
    elif mode == "program":
        program(Path(sys.argv[2]))
    elif mode == "cpu":
        cpu()
    else:
        everything(Path(sys.argv[2]))
