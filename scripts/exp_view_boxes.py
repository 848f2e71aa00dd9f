"""Timing of the viewer's line overlay (himo_amd/view.py "line overlay, v1", csrc/renderlines.hip) on one 1024 x 768 panel: 300
synthetic boxes (on a jittered grid in a 120k-point synthetic sweep, speeds of 0 to 30 m/s, every box tracked) seen by the bird's-eye
camera and by a pinhole, without trails and with the trails of ``--trail 10`` (ten earlier positions per box, made here in the
sweep's own frame).  HIP events on the stream after warm-up calls, medians: ``himo_render_lines`` (with the clear before it, so that
the atomics are issued) and ``himo_render_composite``, and beside them the same run's ``himo_render_splat`` (likewise) and
``himo_render_resolve`` for the sweep the boxes sit in -- the yardstick for
whether drawing the boxes is negligible next to drawing the points.  The lines buffer of each case is first compared with
tests/renderlines_ref.py.  Sets no bar; exits non-zero only when the comparison fails.

    python scripts/exp_view_boxes.py [--out profiles/view_boxes.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import render_ref as pref  # noqa: E402
import renderlines_ref as ref  # noqa: E402
from himo_amd import _lib, view  # noqa: E402

W, H, BOXES, TRAIL, POINTS = 1024, 768, 300, 10, 120_000

# the compiler's resource report for csrc/renderlines.hip (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off
# -Rpass-analysis=kernel-resource-usage), read before the first run on a GPU
RESOURCES = ("compiler's resource report (gfx950): render_lines_kernel 45 VGPRs, 0 AGPRs, 30 SGPRs, 0 scratch bytes a lane, no spills, no LDS, occupancy "
             "8 waves a SIMD; render_composite_kernel 8 VGPRs, 0 AGPRs, 13 SGPRs, 0 scratch bytes a lane, no spills, no LDS, occupancy 8 waves a SIMD")


def events_ms(fn, warm=3, reps=15):
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


def fmt(t):
    return f"{t[0]:.4f} ({t[1]:.4f} .. {t[2]:.4f})"


def synthetic_boxes(rng):
    """300 box rows on a jittered 20 x 15 grid over +-50 m x +-37 m, and per box the TRAIL earlier positions of a constant velocity"""
    gx, gy = np.meshgrid(np.linspace(-48, 48, 20), np.linspace(-35, 35, 15))
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-1.0, 1.0, (BOXES, 2))
    yaw = rng.uniform(-np.pi, np.pi, BOXES)
    speed = rng.uniform(0.0, 30.0, BOXES) * (rng.random(BOXES) < 0.7)
    rows = np.zeros((BOXES, 12), np.float32)
    rows[:, 0:2], rows[:, 2] = xy, rng.uniform(-1.6, -0.4, BOXES)
    rows[:, 3:6] = np.where(rng.random(BOXES)[:, None] < 0.8, [4.5, 1.9, 1.6], [10.0, 2.5, 3.2])
    rows[:, 6], rows[:, 7], rows[:, 8] = yaw, speed * np.cos(yaw), speed * np.sin(yaw)
    trail = []
    for f in range(BOXES):
        top = rows[f, 2] + rows[f, 5] / 2
        past = [np.array([rows[f, 0] - rows[f, 7] * 0.1 * k, rows[f, 1] - rows[f, 8] * 0.1 * k, top]) for k in range(TRAIL, -1, -1)]
        trail += [np.concatenate([a, b]) for a, b in zip(past[:-1], past[1:])]
    return rows, np.asarray(trail, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "view_boxes.txt"))
    a = ap.parse_args()
    dev = _lib.require_gpu()
    from himo_amd.synthetic import make_scene
    frame = make_scene(5, 1, n_points=POINTS, scene_id="view_boxes")[0]
    rng = np.random.default_rng(90)
    rows, trail = synthetic_boxes(rng)
    boxes, _ = view.box_segments(rows, 0.1, 0.05, 0.5)
    cases = {"boxes": boxes, f"boxes + trail {TRAIL}": np.concatenate([boxes, trail])}
    cams = {"bird's-eye": view.Camera.bev((0.0, 0.0), 51.2, W, H, z_range=(-5.0, 15.0)),
            "pinhole": view.Camera.look_at((-60.0, -45.0, 40.0), (0.0, 0.0, 0.0), width=W, height=H, far=250.0)}
    r = view.Renderer(W, H, dev)
    pc0, skip = view.frame_skip(frame)
    ids = torch.from_numpy(np.asarray(frame["lidar_id"]).astype(np.int32)).to(dev)
    ok = True
    lines = [f"view_boxes timing (scripts/exp_view_boxes.py): one {W} x {H} panel, {BOXES} synthetic boxes ({len(boxes)} segments; {len(trail)} more with "
             f"--trail {TRAIL}) in a {POINTS}-point synthetic sweep, one MI355X, one process; HIP events on the stream, medians of 15 calls after 3 warm-ups; "
             "no bar is set; parity unpinned: the reference has no such stage; nothing has been tried on field data",
             RESOURCES,
             "per call [ms]: median (min .. max)"]
    for cam_name, cam in cams.items():
        def clear_points():
            _lib.check(r.lib.himo_render_clear(r.visibility().data_ptr(), W, H, _lib.stream_handle()), "himo_render_clear")

        def fresh_splat():                                            # into a CLEARED buffer: a second splat of the same points finds every word
            clear_points()                                            # already at its minimum and issues no atomic at all
            r.splat(pc0, None, skip, 1, 0, cam)

        t_clear = events_ms(clear_points)
        t_splat = events_ms(fresh_splat)
        t_resolve = events_ms(lambda: r.resolve(ids=(ids,)))
        hit = int((r.visibility() != view.EMPTY).sum().item())
        lines.append(f"  {cam_name}: himo_render_clear alone {fmt(t_clear)}; clear + himo_render_splat of the sweep ({int((skip == 0).sum().item())} points drawn, "
                     f"radius 1, {hit} pixels hit) {fmt(t_splat)}; himo_render_resolve (palette by lidar id) {fmt(t_resolve)}")
        for case, segs in cases.items():
            d_segs = torch.from_numpy(segs).to(dev)
            colors = torch.arange(len(segs), dtype=torch.int32, device=dev)
            for half_px in (0, 1):
                r.clear_lines()
                r.lines(d_segs, half_px, 0, cam)
                got = r.line_buffer().cpu().numpy().view(np.uint64)
                want = ref.clear(W, H)
                ref.lines(want, segs, pref.from_ctypes(cam), half_px=half_px)
                same = bool(np.array_equal(got, want))
                ok &= same

                def fresh_lines():                                    # as above: into a cleared buffer
                    r.clear_lines()
                    r.lines(d_segs, half_px, 0, cam)

                t_lines = events_ms(fresh_lines)
                t_top = events_ms(lambda: r.composite(colors, depth_test=False))
                t_depth = events_ms(lambda: r.composite(colors, depth_test=True))
                lines.append(f"    {case}, line_px {half_px}: {len(segs)} segments, {int((want != ref.EMPTY).sum())} line pixels, identical to tests/renderlines_ref.py "
                             f"{same}: clear + himo_render_lines {fmt(t_lines)}, himo_render_composite on top {fmt(t_top)}, with the depth test {fmt(t_depth)}; clear + lines + "
                             f"composite = {100 * (t_lines[0] + t_top[0]) / (t_splat[0] + t_resolve[0]):.0f} % of clear + splat + resolve")
    lines.append("(every splat and every lines call is timed together with the clear before it: a repeated call into a buffer that already holds its keys "
                 "finds every word at its minimum, issues no atomic and would time the plain loads alone)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
