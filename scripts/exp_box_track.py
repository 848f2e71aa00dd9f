"""Timing of the box tracker (himo_amd/track.py, csrc/boxtrack.hip) on synthetic scenes of 150 sweeps: one call of 1, 64 and 256
scenes at 50 and at 300 boxes per sweep (boxes on a jittered grid with constant velocities of 0 to 30 m/s, centre noise 0.05 m, 2 % of
the detections dropped).  HIP events on the stream after warm-up calls: around the launch alone (the tables already on the device) and
around ``BoxTracker.track`` (the upload of the tables, the allocations and the launch); medians.  A small call is first compared with
tests/boxtrack_ref.py.  Beside the timings, the per-sweep cost of making one sweep's boxes as profiles/box_eval.txt records it: the
yardstick for whether tracking is negligible next to what feeds it.  Sets no bar; exits non-zero only when the comparison fails.

    python scripts/exp_box_track.py [--out profiles/box_track.txt]
"""
import argparse
import ctypes
import re
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import boxtrack_ref as ref  # noqa: E402
from himo_amd import _lib  # noqa: E402
from himo_amd.track import BoxTracker  # noqa: E402

SWEEPS = 150
DISTINCT = 8                        # different scenes drawn per size; a batch repeats them (every scene has a workgroup of its own)

# the compiler's resource report for csrc/boxtrack.hip (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off
# -Rpass-analysis=kernel-resource-usage), read before the first run on a GPU
RESOURCES = ("compiler's resource report (gfx950): bt_track_kernel 188 VGPRs, 0 AGPRs, 106 SGPRs (77 SGPR spills, into VGPR lanes), 0 scratch bytes a "
             "lane, no VGPR spills, 24880 bytes LDS a block, occupancy 2 waves a SIMD (one 512-thread block is 2 waves a SIMD)")


def events_ms(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def box_making_ms():
    path = REPO / "profiles" / "box_eval.txt"
    m = re.search(r"= ([0-9.]+) ms wall", path.read_text()) if path.exists() else None
    return float(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "box_track.txt"))
    a = ap.parse_args()
    dev = _lib.require_gpu()
    lib, P = _lib.load(), _lib.ptr
    tracker = BoxTracker(dev)
    # the path is the tested one: a small call against the restatement
    rng = np.random.default_rng(70)
    small = [ref.moving_scene(rng, 50, 10, drop=0.02), ref.moving_scene(rng, 30, 6, drop=0.1)]
    got, want = tracker.track(small), ref.track(small, [[0.1] * len(sc) for sc in small])
    ok = all(g.tobytes() == w.tobytes() for g, w in zip((got.track_id, got.age, got.state, got.iou, got.live, got.scene_info), want))
    lines = ["box_track timing (scripts/exp_box_track.py): synthetic scenes of 150 sweeps in one call, one MI355X, one process; HIP events on the stream, "
             "medians of 7 calls after 2 warm-ups; no bar is set; nothing has been tried on field data",
             RESOURCES,
             f"against tests/boxtrack_ref.py on 2 small scenes (16 sweeps, {len(want[0])} boxes): every output identical {ok}",
             "per call [ms]: median (min .. max); 'launch' = himo_boxtrack alone, the tables on the device; 'track' = BoxTracker.track (upload, allocations, launch)"]
    per_sweep = {}
    for boxes in (50, 300):
        rng = np.random.default_rng(71 + boxes)
        drawn = [ref.moving_scene(rng, boxes, SWEEPS, drop=0.02) for _ in range(DISTINCT)]
        for n in (1, 64, 256):
            scenes = [drawn[k % DISTINCT] for k in range(n)]
            det, sweep_off, det_off, dt = tracker.tables(scenes)
            d_det, d_so, d_do, d_dt = (torch.from_numpy(x).to(dev) for x in (det, sweep_off, det_off, dt))
            rows = len(det)
            out = (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                   torch.empty((rows, 4), dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.float64, device=dev),
                   torch.empty(len(dt), dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev))
            prm = tracker.params.c_struct()
            need = int(lib.himo_boxtrack_workspace_bytes(n, sweep_off.ctypes.data, det_off.ctypes.data, ctypes.addressof(prm)))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)

            def launch():
                st = lib.himo_boxtrack(n, P(d_det), sweep_off.ctypes.data, P(d_so), det_off.ctypes.data, P(d_do), dt.ctypes.data, P(d_dt), ctypes.addressof(prm),
                                       P(out[0]), P(out[1]), P(out[2]), P(out[3]), P(out[4]), P(out[5]), P(ws), ws.numel(), _lib.stream_handle())
                _lib.check(st, "himo_boxtrack")
            t_launch = events_ms(launch)
            info = out[5].cpu().numpy()
            live = out[4].cpu().numpy()
            del ws
            t_track = events_ms(lambda: tracker.track(scenes), warm=1, reps=3)
            per_sweep[(boxes, n)] = t_launch[0] / (SWEEPS * n)
            lines.append(f"  {n:>3} scenes x {SWEEPS} sweeps x {boxes} boxes ({rows} rows, workspace {need / 1e6:.1f} MB): launch {t_launch[0]:.3f} "
                         f"({t_launch[1]:.3f} .. {t_launch[2]:.3f}), track {t_track[0]:.3f} ({t_track[1]:.3f} .. {t_track[2]:.3f}); {t_launch[0] / SWEEPS * 1e3:.1f} us a "
                         f"step of the call, {per_sweep[(boxes, n)] * 1e3:.2f} us a sweep; ids a scene {info[:, 0].mean():.0f}, overflow {int(info[:, 1].sum())}, "
                         f"live tracks at the end {live[SWEEPS - 1]}")
            del d_det, out
    made = box_making_ms()
    alone, batched = per_sweep[(300, 1)], per_sweep[(300, 256)]
    if made is not None:
        lines.append(f"beside it, making the boxes of ONE sweep (profiles/box_eval.txt): {made:.3f} ms wall.  At 300 boxes a sweep of a scene tracked ALONE costs "
                     f"{alone * 1e3:.0f} us ({100 * alone / made:.0f} % of that), a sweep in a batch of 256 scenes {batched * 1e3:.2f} us ({100 * batched / made:.2f} %); "
                     f"at 50 boxes {per_sweep[(50, 1)] * 1e3:.0f} us alone ({100 * per_sweep[(50, 1)] / made:.0f} %) and {per_sweep[(50, 256)] * 1e3:.2f} us in the batch")
    lines.append(f"one workgroup per scene IS the limit at 300 boxes: a call of 1 scene takes {alone * SWEEPS:.1f} ms and a call of 256 scenes {batched * SWEEPS * 256:.1f} "
                 f"ms -- a call lasts as long as one scene's chain of {SWEEPS} steps while the scenes do not outnumber the compute units, so a scene tracked alone "
                 f"leaves the chip idle and pays the whole step ({alone * 1e3:.0f} us at 300 boxes, {per_sweep[(50, 1)] * 1e3:.0f} us at 50), and only a batch makes "
                 f"tracking negligible next to what feeds it.  Not restructured here (splitting a step's pair phase over several workgroups is the open item)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
