"""Throughput of the ground segmenter (himo_amd/csrc/groundseg.hip): 32 sweeps x 120 000 points of the synthetic "rings" cloud
through ``himo_ground_seg_batch``, timed with HIP events on the launch stream, against the stage's algorithmic bytes -- two reads
of xyz and one byte written per point.  Prints sweeps/s, achieved bytes/s and the per-kernel times; gates nothing.

    python scripts/exp_ground_seg.py [--sweeps 32] [--points 120000] [--pitch 4] [--reps 20] [--out profiles/ground_seg.txt]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=32)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--pitch", type=int, default=4, choices=(3, 4))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from himo_amd import _lib
    from himo_amd.ground_seg import GroundParams, segment_batch, workspace_bytes
    from himo_amd.synthetic import GROUND_Z, make_frame
    dev = _lib.require_gpu()
    frames = [make_frame(k, n_points=a.points, cloud="rings") for k in range(a.sweeps)]
    offsets_host = np.arange(a.sweeps + 1, dtype=np.int64) * a.points
    pc = torch.from_numpy(np.ascontiguousarray(np.concatenate([f["pc0"][:, :a.pitch] for f in frames]))).to(dev)
    offsets = torch.from_numpy(offsets_host).to(dev)
    params = GroundParams(sensor_height=-GROUND_Z)
    ws = torch.empty(workspace_bytes(a.sweeps, params), dtype=torch.uint8, device=dev)
    mask = torch.empty(a.sweeps * a.points, dtype=torch.uint8, device=dev)
    for _ in range(3):
        segment_batch(pc, offsets_host, offsets, params, mask=mask, workspace=ws)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        segment_batch(pc, offsets_host, offsets, params, mask=mask, workspace=ws)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e-3)
    _lib.prof_start("ground_")
    for _ in range(a.reps):
        segment_batch(pc, offsets_host, offsets, params, mask=mask, workspace=ws)
    kernels = _lib.prof_stop()
    host = mask.cpu().numpy().astype(bool)
    gm0 = np.concatenate([f["gm0"] for f in frames])
    t = float(np.median(times))
    algo = a.sweeps * a.points * (2 * 4 * a.pitch + 1)
    lines = [f"ground_seg: {a.sweeps} sweeps x {a.points} points, pitch {a.pitch}, {a.reps} launches, HIP events ({torch.cuda.get_device_name(dev)})",
             f"  whole call (key memset + 3 kernels): median {t * 1e6:.1f} us, min {min(times) * 1e6:.1f} us, max {max(times) * 1e6:.1f} us",
             f"  {a.sweeps / t:.0f} sweeps/s, {a.sweeps * a.points / t / 1e9:.2f} G points/s",
             f"  algorithmic bytes (2 reads of xyz + 1 B written per point): {algo / 1e6:.1f} MB -> {algo / t / 1e12:.3f} TB/s achieved",
             f"  workspace {ws.numel() / 1e6:.1f} MB ({ws.numel() / a.sweeps / 1e6:.2f} MB a sweep: 12 B per cell)"]
    for name, k in sorted(kernels.items()):
        lines.append(f"  {name}: avg {k['avg_ms'] * 1e3:.1f} us, min {k['min_ms'] * 1e3:.1f} us over {k['count']} launches")
    lines.append(f"  ground share {100 * host.mean():.2f} %, agreement with the synthetic's own gm0 {100 * (host == gm0).mean():.2f} % (a figure, not a gate)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
