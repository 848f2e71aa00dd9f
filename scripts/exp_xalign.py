"""Timing of cross-sensor alignment (himo_amd/xalign.py, csrc/xalign.hip) in one process on one MI355X: ONE call of 32 synthetic
120 000-point sweeps, about 300 labelled clusters a sweep (moving vehicle surfaces seen by three sensors 33 ms apart); one sweep alone;
and, as the yardstick, the existing entry point on the same inputs: the call of ``himo_xsensor`` over the same clusters.  Wall per call by
the host clock around the call and a device synchronise (median of 9 after 2 warm-ups); the kernels by the library's event scopes in a
run of their own; the cost per pass from the iterations the call reports.  The first sweep's 300 clusters -- the decided ones are where the
timed path runs -- are first compared with tests/xalign_ref.py.  Sets no bar; exits non-zero only when that comparison fails.

    python scripts/exp_xalign.py [--out profiles/xalign.txt] [--sweeps 32]
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

import xalign_ref as ref  # noqa: E402
import xsensor_ref as xs  # noqa: E402
from himo_amd import _lib  # noqa: E402
from himo_amd.eval_xsensor import XSensorParams, xsensor_labelled  # noqa: E402
from himo_amd.xalign import ALIGNED, REJECTED, STATE_NAMES, STATIC, XAlignParams, xalign_labelled  # noqa: E402

CAPTURE = (0.0, 0.033, 0.066)


def sweep(seed, n_total=120_000, n_clusters=300):
    """one sweep: ``n_clusters`` vehicle surfaces of 30..3000 rows, a third of them moving at up to 35 m/s, every row recorded by one of
    three sensors at its capture time; the rest unlabelled ground"""
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.exp(rng.normal(4.6, 0.9, n_clusters)), 30, 3000).astype(int)
    pts, labels, group = [], [], []
    for i, n in enumerate(sizes):
        centre = np.array([-70.0 + 7.0 * (i % 20), -50.0 + 7.0 * (i // 20), 0.0])
        yaw = rng.uniform(0, 2 * np.pi)
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        v = R @ np.array([rng.uniform(5.0, 35.0) if i % 3 == 0 else 0.0, 0.0, 0.0])
        g = rng.integers(0, 3, int(n))
        p = xs.vehicle_surface(rng, int(n)) @ R.T + centre + rng.normal(0, 0.02, (int(n), 3)) + np.asarray(CAPTURE)[g][:, None] * v[None, :]
        pts.append(p), labels.append(np.full(int(n), i + 1, np.int32)), group.append(g + 1)
    n_obj = int(sizes.sum())
    pts.append(np.concatenate([rng.uniform(-75, 75, (n_total - n_obj, 2)), rng.normal(-1.5, 0.02, (n_total - n_obj, 1))], axis=1))
    labels.append(np.zeros(n_total - n_obj, np.int32)), group.append(rng.integers(1, 4, n_total - n_obj))
    order = rng.permutation(n_total)
    pts, labels, group = np.concatenate(pts).astype(np.float32)[order], np.concatenate(labels)[order], np.concatenate(group).astype(np.uint8)[order]
    tau = np.asarray(CAPTURE, np.float32)[group - 1]
    return pts, labels, group, tau, sizes


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
    _lib.load()
    S, per = a.sweeps, 300
    parts = [sweep(s) for s in range(S)]
    C = per * S
    up = lambda k, n: torch.from_numpy(np.concatenate([p[k] for p in parts[:n]])).to(dev)      # noqa: E731
    labels_h = np.concatenate([np.where(p[1] > 0, p[1] + per * s, 0) for s, p in enumerate(parts)]).astype(np.int32)
    pts, group, tau, labels = up(0, S), up(2, S), up(3, S), torch.from_numpy(labels_h).to(dev)
    n1 = len(parts[0][0])
    prm, xprm = XAlignParams(), XSensorParams()
    call = lambda: xalign_labelled(pts, labels, group, tau, C, prm)                    # noqa: E731
    single = lambda: xalign_labelled(pts[:n1], labels[:n1], group[:n1], tau[:n1], per, prm)      # noqa: E731
    yard = lambda: xsensor_labelled(pts, labels, group, C, xprm, tau)                  # noqa: E731
    info, v, x = (t.cpu().numpy() for t in call())
    sizes = np.concatenate([p[4] for p in parts])
    decided = np.isin(info[:, 0], (ALIGNED, REJECTED, STATIC))
    passes = (info[decided, 6].astype(np.float64) + 2)
    pair_evals = float((info[decided, 3].astype(np.float64) ** 2 * passes).sum())
    lines = ["xalign timing (scripts/exp_xalign.py): one MI355X, one process; medians of 9 calls after 2 warm-ups; no bar is set",
             f"call: {S} synthetic sweeps of {n1} points = {len(pts)} rows, {int((labels_h > 0).sum())} of them labelled, in {C} clusters of "
             f"{sizes.min()}..{sizes.max()} rows (median {int(np.median(sizes))}), three sensors 33 ms apart, a third of the clusters moving",
             "clusters: " + ", ".join(f"{int((info[:, 0] == s).sum())} {n}" for s, n in enumerate(STATE_NAMES)) +
             f"; decided clusters (aligned, rejected, static): {int(decided.sum())} of {int(info[decided, 3].sum())} rows, mean iterations "
             f"{float(info[decided, 6].mean()) if decided.any() else float('nan'):.2f}; distance evaluations (sum of rows^2 x (iterations + 2)): {pair_evals:.3g}"]
    # the first sweep against the restatement: all its clusters, of which the decided ones walk the timed path
    p0 = parts[0]
    want = ref.estimate(p0[0], p0[1], p0[2], p0[3], per)
    first = np.isin(want[0][:, 0], (ALIGNED, REJECTED, STATIC))
    ok = info[:per].tobytes() == want[0].tobytes() and v[:per].tobytes() == want[1].tobytes() and x[:per].tobytes() == want[2].tobytes()
    lines.append(f"against tests/xalign_ref.py on the {per} clusters of the first sweep ({int(first.sum())} of them decided, of "
                 f"{int(want[0][first, 3].min()) if first.any() else 0}..{int(want[0][first, 3].max()) if first.any() else 0} rows, "
                 f"{int(want[0][first, 6].sum())} iterations in all): info, v and the sums identical {bool(ok)}")

    wall, one, base = timed(call), timed(single), timed(yard)
    lines.append("wall per call, host clock around the call and a device synchronise [ms]: median (min .. max)")
    lines.append(f"  xalign_labelled, {S} sweeps (sort by label, one host wait, one clear and two launches): {wall[0]:.3f} ({wall[1]:.3f} .. {wall[2]:.3f})")
    lines.append(f"  xalign_labelled, one sweep alone: {one[0]:.3f} ({one[1]:.3f} .. {one[2]:.3f})")
    lines.append(f"  xsensor_labelled (the existing entry point, rules A-B and one search) over the same {S} sweeps: {base[0]:.3f} ({base[1]:.3f} .. {base[2]:.3f})")
    lines.append(f"  ratio xalign / xsensor over the same clusters: {wall[0] / base[0]:.2f}")
    sc = scopes_of(call, only="xa_")
    cl = sc.get("xa_cluster_kernel", float("nan"))
    lines.append("kernel scopes per call [ms]: " + ", ".join(f"{k} {sc.get(k, float('nan')):.4f}" for k in ("xa_count_kernel", "xa_cluster_kernel")))
    lines.append(f"  xa_cluster_kernel per pass over the decided clusters (vote included): {cl / float(passes.mean()) if decided.any() else float('nan'):.4f} ms "
                 f"at a mean of {float(passes.mean()) if decided.any() else float('nan'):.2f} passes; {pair_evals / (cl * 1e-3) / 1e9 if cl == cl else float('nan'):.1f} G distance evaluations / s")
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
