"""Timing of the cluster boxes (himo_amd/box_fit.py, csrc/boxfit.hip) on one synthetic 120 000-point sweep of about 200 L-shaped
objects over a ground plane, beside the DBSCAN call that precedes it in the same process: wall per call by the host clock around
the call and a device synchronise (median of 15 after 3 warm-ups), the kernels' own time by the library's event scopes in a run of
their own, and one cluster of ``max_points`` rows.  The boxes are first compared with tests/boxfit_ref.py on the very sweep.  Sets no
bar; exits non-zero only when that comparison fails.

    python scripts/exp_box_fit.py [--out profiles/box_fit.txt]
"""
import argparse
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import boxfit_ref as ref  # noqa: E402
from himo_amd import _lib  # noqa: E402
from himo_amd.box_fit import BoxFitter  # noqa: E402
from himo_amd.seflow.ssl_label import EPS, MIN_PTS, dbscan  # noqa: E402


def sweep(seed=0, n_total=120_000, n_clusters=210):
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.exp(rng.normal(5.0, 0.9, n_clusters)), 30, 3000).astype(int)
    pts = []
    for i, n in enumerate(sizes):
        centre = (-49.0 + 7.0 * (i % 15), -49.0 + 7.0 * (i // 15))
        xy = ref.lshape(rng, int(n), rng.uniform(0, math.pi / 2), 4.5, 1.9, 0.02, centre)
        pts.append(np.concatenate([xy, rng.uniform(0.2, 1.6, (int(n), 1))], axis=1))
    n_obj = int(sizes.sum())
    ground = np.concatenate([rng.uniform(-51, 51, (n_total - n_obj, 2)), rng.normal(-1.5, 0.02, (n_total - n_obj, 1))], axis=1)
    pts.append(ground)
    pts = np.concatenate(pts).astype(np.float32)
    gm = np.zeros(n_total, bool)
    gm[n_obj:] = True
    order = rng.permutation(n_total)
    motion = rng.normal(0, 0.05, (n_total, 3)).astype(np.float32)
    return pts[order], gm[order], motion[order], sizes


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pts_h, gm_h, motion_h, sizes = sweep()
    pts, gm, motion = torch.from_numpy(pts_h).to(dev), torch.from_numpy(gm_h).to(dev), torch.from_numpy(motion_h).to(dev)
    fitter = BoxFitter(dev)
    labels, count = dbscan(pts, EPS, MIN_PTS, skip=gm)
    C = int(count)
    res = fitter.fit(pts, labels, motion)
    info = res.info
    lines = ["box_fit timing (scripts/exp_box_fit.py): one synthetic sweep, one MI355X, one process; medians of 15 calls after 3 warm-ups; no bar is set",
             f"sweep: {len(pts_h)} points, {int((~gm_h).sum())} non-ground in {len(sizes)} L-shaped objects of {sizes.min()}..{sizes.max()} points "
             f"(median {int(np.median(sizes))}); DBSCAN (eps {EPS}, min_pts {MIN_PTS}) finds {C} clusters",
             f"boxes: {int((info[:, 0] == 0).sum())} fitted, {int((info[:, 0] == 1).sum())} too few, {int((info[:, 0] == 2).sum())} too large; K = 90 directions"]
    # check against the restatement on this very sweep (bit for bit, as the tests do on small ones)
    want_info, want_box = ref.fit(pts_h, labels.cpu().numpy(), C, motion=motion_h)
    ok_info = bool((info == want_info).all())
    ok_box = res.box[:, [0, 1, 2, 3, 4, 5, 9]].tobytes() == want_box[:, [0, 1, 2, 3, 4, 5, 9]].tobytes()
    lines.append(f"against tests/boxfit_ref.py on this sweep: info identical {ok_info}, box columns 0-5 identical {ok_box}, "
                 f"mean motion max abs difference {np.abs(res.box[:, 6:9] - want_box[:, 6:9]).max():.3g}")

    db = timed(lambda: dbscan(pts, EPS, MIN_PTS, skip=gm))
    fit = timed(lambda: fitter.fit(pts, labels, motion))
    fit_rows = timed(lambda: fitter.fit(pts, labels, motion).rows)
    fit_nomotion = timed(lambda: fitter.fit(pts, labels))
    lines.append("wall per call, host clock around the call and a device synchronise [ms]: median (min .. max)")
    for name, t in (("ssl_label.dbscan (the call before it)", db), ("BoxFitter.fit (sort by label, one host wait, one launch)", fit),
                    ("BoxFitter.fit(...).rows (the same plus the copy back and rule H)", fit_rows), ("BoxFitter.fit without motion", fit_nomotion)):
        lines.append(f"  {name}: {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})")
    # the kernels' own time, by the library's event scopes, in a run of its own
    for what, fn in (("dbscan", lambda: dbscan(pts, EPS, MIN_PTS, skip=gm)), ("box_fit", lambda: fitter.fit(pts, labels, motion))):
        _lib.prof_start()
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        scopes = _lib.prof_stop()
        total = sum(v["total_ms"] for v in scopes.values()) / 10
        lines.append(f"kernel scopes of {what}, per call [ms]: total {total:.3f}: " +
                     ", ".join(f"{k} {v['total_ms'] / 10:.4f}" for k, v in sorted(scopes.items(), key=lambda kv: -kv[1]["total_ms"])[:8]))
    # one large cluster: the tail max_points bounds
    big = ref.lshape(np.random.default_rng(1), 8192, 0.3, 40.0, 12.0, 0.02, (0.0, 0.0))
    bp = torch.from_numpy(np.concatenate([big, np.zeros((8192, 1))], axis=1).astype(np.float32)).to(dev)
    bl = torch.ones(8192, dtype=torch.int32, device=dev)
    _lib.prof_start("bf_fit")
    for _ in range(10):
        fitter.fit(bp, bl)
    torch.cuda.synchronize()
    scopes = _lib.prof_stop()
    lines.append("one cluster of 8192 points (max_points): bf_fit_kernel " +
                 ", ".join(f"{v['total_ms'] / 10:.4f} ms" for v in scopes.values()))
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    if not (ok_info and ok_box):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
