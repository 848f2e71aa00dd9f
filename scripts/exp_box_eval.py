"""Timing of the box evaluation (himo_amd/eval_box.py, csrc/boxeval.hip) on 32 synthetic sweeps of about 300 boxes against the same
boxes jittered (centre +-0.3 m, yaw +-5 degrees, a third of them stretched by up to 3 m along the heading; 20 % further boxes on each
side that overlap nothing), all in one call: wall per call by the host clock around the call and a device synchronise (median of 15
after 3 warm-ups), and the two phases by the library's event scopes in a run of their own.  The result is first compared with
tests/boxeval_ref.py on those very sweeps.  Beside it, the time of making such boxes -- ``himo_boxfit`` and the DBSCAN call before it --
as profiles/box_fit.txt records it.  Sets no bar; exits non-zero only when the comparison fails.

    python scripts/exp_box_eval.py [--out profiles/box_eval.txt]
"""
import argparse
import re
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import boxeval_ref as ref  # noqa: E402
from himo_amd import _lib  # noqa: E402
from himo_amd.eval_box import BoxEvaluator, rects  # noqa: E402

# the compiler's resource report for csrc/boxeval.hip (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off
# -Rpass-analysis=kernel-resource-usage), read before the first run on a GPU
RESOURCES = ("compiler's resource report (gfx950): be_pair_kernel 124 VGPRs, 80 SGPRs, 0 scratch bytes a lane, no spills, 12288 bytes LDS a block, "
             "occupancy 4 waves a SIMD; be_match_kernel 124 VGPRs, 0 scratch bytes, no spills, 16640 bytes LDS; be_list_kernel 114 VGPRs, 0 scratch "
             "bytes, no spills")


def timed(fn, warm=3, reps=15):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def box_fit_times():
    """what profiles/box_fit.txt records for making boxes: (BoxFitter.fit, the DBSCAN call before it) wall per call, ms"""
    path = REPO / "profiles" / "box_fit.txt"
    if not path.exists():
        return None
    text = path.read_text()
    fit = re.search(r"BoxFitter\.fit \(sort by label[^:]*: ([0-9.]+)", text)
    db = re.search(r"ssl_label\.dbscan[^:]*: ([0-9.]+)", text)
    return (float(fit.group(1)), float(db.group(1))) if fit and db else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    rows_a, rows_b = zip(*[ref.jittered_sweep(rng, 250) for _ in range(32)])
    ev = BoxEvaluator(dev)
    res = ev.match(rows_a, rows_b)
    lines = ["box_eval timing (scripts/exp_box_eval.py): 32 synthetic sweeps in one call, one MI355X, one process; medians of 15 calls after 3 warm-ups; "
             "no bar is set",
             f"sweeps: {len(rows_a)} of {len(rows_a[0])} boxes against {len(rows_b[0])} (250 jittered copies and 50 that overlap nothing, a side); "
             f"min_iou {ev.min_iou:g}; candidate store {int(res.off_a[-1]) * max(len(r) for r in rows_b) * 8 / 1e6:.1f} MB",
             RESOURCES]
    # check against the restatement on these very sweeps (bit for bit, as the tests do on small ones)
    ok, kept, ious = True, 0, []
    for s, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        ma, mb, iou_a = ref.match(ra, rb)
        ga, gb, gi = res.sweep(s)
        ok = ok and ga.tobytes() == ma.tobytes() and gb.tobytes() == mb.tobytes() and gi.tobytes() == iou_a.tobytes()
        kept += int((ma >= 0).sum())
        ious.append(iou_a[ma >= 0, 0])
    ious = np.concatenate(ious)
    lines.append(f"against tests/boxeval_ref.py on these sweeps: match_a, match_b and iou_a identical {ok}; {kept} kept pairs, mean iou {ious.mean():.3f}, "
                 f"{int((ious >= 0.5).sum())} at 0.5, {int((ious >= 0.7).sum())} at 0.7")

    rects_only = timed(lambda: [rects(r) for r in rows_a + rows_b])
    call = timed(lambda: ev.match(rows_a, rows_b))
    copies = timed(lambda: ev.match(rows_a, rows_b).iou_a)
    lines.append("wall per call, host clock around the call and a device synchronise [ms]: median (min .. max)")
    for name, t in (("BoxEvaluator.match (rule A on the host, the upload, two launches)", call),
                    ("BoxEvaluator.match(...).iou_a (the same plus the copies back)", copies),
                    ("rule A alone, on the host (rects of the 64 box lists)", rects_only)):
        lines.append(f"  {name}: {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})")
    # the two phases, by the library's event scopes, in a run of their own
    _lib.prof_start("be_")
    for _ in range(10):
        ev.match(rows_a, rows_b)
    torch.cuda.synchronize()
    scopes = _lib.prof_stop()
    total = sum(v["total_ms"] for v in scopes.values()) / 10
    lines.append(f"kernel scopes, per call [ms]: total {total:.3f}: " + ", ".join(f"{k} {v['total_ms'] / 10:.4f}" for k, v in sorted(scopes.items())))
    lines.append(f"per sweep: {call[0] / len(rows_a):.3f} ms wall, {total / len(rows_a):.4f} ms in the kernels")
    made = box_fit_times()
    if made:
        lines.append(f"beside it, making the boxes of ONE sweep (profiles/box_fit.txt): BoxFitter.fit {made[0]:.3f} ms + the DBSCAN call before it "
                     f"{made[1]:.3f} ms = {made[0] + made[1]:.3f} ms wall")
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
