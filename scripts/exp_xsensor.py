"""Timing of the cross-sensor consistency score (himo_amd/eval_xsensor.py, csrc/xsensor.hip) on ONE call of 32 synthetic 120 000-point
sweeps under 2 names, about 300 labelled clusters a sweep, three sensors: wall per call by the host clock around the call and a device
synchronise (median of 9 after 2 warm-ups), the sort and the host wait on their own, and the three phases by the library's event scopes
in a run of their own.  Beside the search phase, in the same process: ``himo_nn_search`` in float32 over the same clusters as segments
-- existing code, the same number of distance evaluations, no group test.  The first sweep's records are first compared with
tests/xsensor_ref.py.  Sets no bar; exits non-zero only when that comparison fails.

    python scripts/exp_xsensor.py [--out profiles/xsensor.txt] [--sweeps 32]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import xsensor_ref as ref  # noqa: E402
from himo_amd import _lib  # noqa: E402
from himo_amd.eval_xsensor import STATE_NAMES, XSensorParams, xsensor_labelled  # noqa: E402


def sweep(seed, n_total=120_000, n_clusters=300):
    """one sweep: ``n_clusters`` vehicle-sized blobs of 30..3000 rows seen by three sensors, the rest unlabelled ground"""
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.exp(rng.normal(4.6, 0.9, n_clusters)), 30, 3000).astype(int)
    pts, labels = [], []
    for i, n in enumerate(sizes):
        centre = np.array([-70.0 + 7.0 * (i % 20), -50.0 + 7.0 * (i // 20), 0.0])
        pts.append(ref.vehicle_surface(rng, int(n)) + centre)
        labels.append(np.full(int(n), i + 1, np.int32))
    n_obj = int(sizes.sum())
    pts.append(np.concatenate([rng.uniform(-75, 75, (n_total - n_obj, 2)), rng.normal(-1.5, 0.02, (n_total - n_obj, 1))], axis=1))
    labels.append(np.zeros(n_total - n_obj, np.int32))
    order = rng.permutation(n_total)
    pts, labels = np.concatenate(pts).astype(np.float32)[order], np.concatenate(labels)[order]
    group = rng.integers(1, 4, n_total).astype(np.uint8)
    dt = (np.float32(0.033) * (group - 1)).astype(np.float32)
    motion = np.tile(np.array([1.2, 0.0, 0.0], np.float32), (n_total, 1))
    return pts, labels, group, dt, motion, sizes


def timed(fn, warm=2, reps=9):
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


def scopes_of(fn, reps=5, only=None):
    fn()
    torch.cuda.synchronize()
    _lib.prof_start(only)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return {k: v["total_ms"] / reps for k, v in _lib.prof_stop().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sweeps", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    S, per = a.sweeps, 300
    parts = [sweep(s) for s in range(S)]
    names = []
    for shift in (0.0, 0.3):                                          # the second name: every sensor's copy displaced along x
        for s, (pts, labels, group, dt, motion, _) in enumerate(parts):
            moved = pts.copy()
            moved[:, 0] += np.float32(shift) * (group.astype(np.float32) - 1)
            names.append((moved, np.where(labels > 0, labels + per * (len(names)), 0).astype(np.int32), group, dt, motion))
    C = per * len(names)
    up = lambda k: torch.from_numpy(np.concatenate([n[k] for n in names])).to(dev)      # noqa: E731
    pts, labels, group, dt, motion = (up(k) for k in range(5))
    prm = XSensorParams()
    call = lambda: xsensor_labelled(pts, labels, group, C, prm, dt, motion)            # noqa: E731
    info, rec, mot, _ = call()
    info_h, rec_h, mot_h = info.cpu().numpy(), rec.cpu().numpy(), mot.cpu().numpy()
    sizes = np.concatenate([p[5] for p in parts])
    lines = ["eval_xsensor timing (scripts/exp_xsensor.py): one call, one MI355X, one process; medians of 9 calls after 2 warm-ups; no bar is set",
             f"call: {S} synthetic sweeps of {len(parts[0][0])} points x 2 names = {len(pts)} rows, {int((labels > 0).sum())} of them labelled, in {C} "
             f"clusters of {sizes.min()}..{sizes.max()} rows (median {int(np.median(sizes))}), three sensors",
             "clusters: " + ", ".join(f"{int((info_h[:, 0] == s).sum())} {n}" for s, n in enumerate(STATE_NAMES)) +
             f"; {int(info_h[:, 3].sum())} query rows; distance evaluations (sum of n^2 over the clusters): {float((sizes.astype(np.float64) ** 2).sum() * 2):.3g}"]
    # the first sweep under both names against the restatement
    ok = True
    for r in range(2):
        p = names[r * S]
        want = ref.score(p[0], np.where(p[1] > 0, p[1] - per * r * S, 0), p[2], per, dt=p[3], motion=p[4])
        lo = per * r * S
        ok &= info_h[lo:lo + per].tobytes() == want[0].tobytes() and rec_h[lo:lo + per].tobytes() == want[1].tobytes() and \
            mot_h[lo:lo + per].tobytes() == want[2].tobytes()
    lines.append(f"against tests/xsensor_ref.py on the first sweep under both names: info, rec and mot identical {bool(ok)}")

    wall = timed(call)
    lines.append("wall per call, host clock around the call and a device synchronise [ms]: median (min .. max)")
    lines.append(f"  xsensor_labelled (sort by label, one host wait, one clear and three launches): {wall[0]:.3f} ({wall[1]:.3f} .. {wall[2]:.3f})")

    def sort_only():
        lab = torch.where((labels > 0) & (labels <= C), labels, torch.zeros_like(labels))
        order = torch.argsort(torch.where(lab > 0, lab, torch.iinfo(torch.int32).max), stable=True)
        sizes_d = torch.bincount(lab, minlength=C + 1)[1:C + 1]
        return order, torch.cumsum(sizes_d, 0).cpu()                  # (the copy back stands for the host wait)
    srt = timed(sort_only)
    lines.append(f"  the sort by label, the row ranges and their copy to the host alone (torch): {srt[0]:.3f} ({srt[1]:.3f} .. {srt[2]:.3f})")
    sc = scopes_of(call, only="xs_")
    lines.append("kernel scopes per call [ms]: " + ", ".join(f"{k} {sc.get(k, float('nan')):.4f}" for k in ("xs_count_kernel", "xs_search_kernel", "xs_reduce_kernel")) +
                 f"; total {sum(sc.values()):.4f}")

    # himo_nn_search in float32 over the same clusters as segments: the same distance evaluations, no group test
    lab = torch.where((labels > 0) & (labels <= C), labels, torch.zeros_like(labels))
    order = torch.argsort(torch.where(lab > 0, lab, torch.iinfo(torch.int32).max), stable=True)
    offsets = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(lab, minlength=C + 1)[1:C + 1], 0, out=offsets[1:])
    nc = int(offsets[-1])
    xyz = pts[order[:nc], :3].contiguous()
    d2 = torch.empty(nc, dtype=torch.float32, device=dev)

    def nn():
        _lib.check(lib.himo_nn_search(C, _lib.ptr(offsets), _lib.ptr(offsets), nc, nc, _lib.ptr(xyz), _lib.ptr(xyz), 0, _lib.ptr(d2), None,
                                      _lib.stream_handle()), "himo_nn_search")
    # the two take turns in one process, three rounds: the later rounds show what the clock did
    rounds = []
    for _ in range(3):
        rounds.append((scopes_of(call, only="xs_search")["xs_search_kernel"], scopes_of(nn, only="nn_kernel")["nn_kernel_f32"]))
    mine, theirs = statistics.median(r[0] for r in rounds), statistics.median(r[1] for r in rounds)
    lines.append("search phase beside himo_nn_search (float32, the same clusters as segments, queries = references = the cluster's rows), taking turns, "
                 "three rounds of 5 calls [ms]: " + "; ".join(f"{x:.4f} / {y:.4f}" for x, y in rounds))
    lines.append(f"  xs_search_kernel {mine:.4f} ms against nn_kernel_f32 {theirs:.4f} ms: ratio {mine / theirs:.2f} (expected within 1.5)")
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
