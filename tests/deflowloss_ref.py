"""The rule of "DeFlow loss, v1" (include/himo_amd.h, himo_amd/csrc/deflowloss.hip) in numpy float64: the same operations in the
same order on the float32 inputs, ``math.fsum`` (exactly rounded) for the sums, the gradient rounded once to float32.  Also the
seeded cases the CPU and GPU tests share.  Checker only: never imported by the package."""
from __future__ import annotations

import math

import numpy as np

TERMS = ("slow", "medium", "fast")


def counted_rows(n, gt, pid=None, valid=None):
    c = np.isfinite(np.asarray(gt, np.float32)[:, :3]).all(axis=1) if n else np.zeros(0, bool)
    if pid is not None:
        c = c & (np.asarray(pid) >= 0)
    if valid is not None:
        c = c & (np.asarray(valid) != 0)
    return c


def deflow_loss_ref(pc0, moved, est, gt, pid=None, valid=None, sensor_dt=0.1):
    """-> {"terms" [3] float64, "total", "counts" [3] int64, "grad" (n,3) float32, "band" (n,) int8 (3 = uncounted), "counted"}"""
    p = np.asarray(pc0, np.float32)[:, :3].astype(np.float64)
    m = np.asarray(moved, np.float32)[:, :3].astype(np.float64)
    f = np.asarray(est, np.float32)[:, :3].astype(np.float64)
    gtf = np.asarray(gt, np.float32)[:, :3]
    n = p.shape[0]
    counted = counted_rows(n, gtf, pid, valid)
    dt = float(np.float32(sensor_dt))                       # (double)sensor_dt of the float32 argument
    t0, t1 = 0.4 * dt, 1.0 * dt
    with np.errstate(all="ignore"):
        g = (p + gtf.astype(np.float64)) - m
        s = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        band = np.where(s < t0, 0, np.where(s <= t1, 1, 2)).astype(np.int8)
        band[~counted] = 3
        d = f - g
        e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        counts = np.array([int((band == b).sum()) for b in range(3)], np.int64)
        terms = np.zeros(3, np.float64)
        for b in range(3):
            if counts[b]:
                eb = e[band == b]
                terms[b] = (math.fsum(eb.tolist()) if np.isfinite(eb).all() else float(eb.sum())) / float(counts[b])
        total = (terms[0] + terms[1]) + terms[2]
        grad = np.zeros((n, 3), np.float32)
        for b in range(3):
            rows = (band == b) & (e != 0.0)                  # (a NaN e goes through: that row's gradient is NaN)
            grad[rows] = ((d[rows] / e[rows, None]) / float(counts[b])).astype(np.float32)
    return {"terms": terms, "total": float(total), "counts": counts, "grad": grad, "band": band, "counted": counted, "e": e}


def make_case(n, seed=0, sensor_dt=0.1, bands=(0, 1, 2), with_pid=True, with_valid=True, all_dropped=False, n_exact=0, n_bad_gt=0,
              nan_est_row=None, pc0_cols=3, est_cols=3):
    """Seeded rows with |coordinates| < 60: ``moved`` a small rigid-looking offset of ``pc0``, the ground-truth residual's speed drawn
    from ``bands`` (0: < 0.4 dt, 1: up to dt, 2: above) row by row in turn, so that every listed band is occupied from n = len(bands)
    on, ``est`` = the residual + noise.  ``n_exact`` rows get est == g exactly (those rows have m = p), ``n_bad_gt`` rows a NaN / inf ground truth, ``nan_est_row`` a NaN estimate.  pid < 0 on ~1/7 of the rows, valid == 0 on
    ~1/9.  Returns a dict of numpy arrays (pc0 (n, pc0_cols), est (n, est_cols))."""
    rng = np.random.default_rng(1000 * seed + n % 997)
    dt = float(np.float32(sensor_dt))
    pc0 = np.zeros((n, pc0_cols), np.float32)
    pc0[:, :3] = rng.uniform(-55.0, 55.0, (n, 3)).astype(np.float32)
    if pc0_cols > 3:
        pc0[:, 3:] = rng.uniform(0, 1, (n, pc0_cols - 3))
    moved = (pc0[:, :3].astype(np.float64) + rng.uniform(-1.5, 1.5, 3) + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    which = np.asarray(bands)[np.arange(n) % len(bands)] if n else np.zeros(0, np.int64)
    lo = np.array([0.0, 0.45, 1.1])[which] * dt
    hi = np.array([0.35, 0.95, 30.0])[which] * dt
    speed = rng.uniform(lo, hi)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-9)
    resid = dirs * speed[:, None]
    # gt = m + resid - p in float64, rounded to float32: the residual the kernel re-forms differs from `resid` by ~1e-6 m, far
    # inside the gaps left around the band edges above
    gt = (moved.astype(np.float64) + resid - pc0[:, :3].astype(np.float64)).astype(np.float32)
    est = np.zeros((n, est_cols), np.float32)
    est[:, :3] = (resid + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    if n_exact and n:
        # est == g exactly needs a g that is a float32: with m = p, g = (p + gt) - p = gt (p + gt is exact in double: the two
        # float32 are less than 2^29 apart in magnitude)
        rows = np.unique(np.arange(min(n_exact, n)) * max(1, n // n_exact) % n)
        moved[rows] = pc0[rows, :3]
        gt[rows] = resid[rows].astype(np.float32)
        est[rows, :3] = gt[rows]
    bad_rows = np.zeros(0, np.int64)
    if n_bad_gt and n:
        bad_rows = rng.choice(n, size=min(n_bad_gt, n), replace=False)
        for k, r in enumerate(bad_rows):
            gt[r, k % 3] = [np.nan, np.inf, -np.inf][k % 3]
    pid = valid = None
    if with_pid:
        pid = rng.integers(0, 512 * 512, n).astype(np.int32)
        pid[rng.uniform(size=n) < 1 / 7] = -1
        if all_dropped:
            pid[:] = -1
    if with_valid:
        valid = (rng.uniform(size=n) >= 1 / 9).astype(np.uint8)
    if nan_est_row is not None and n:
        r = int(nan_est_row) % n
        est[r, 1] = np.nan
        if pid is not None:
            pid[r] = 7
        if valid is not None:
            valid[r] = 1
        if np.isin(r, bad_rows):
            gt[r] = 0.0
    return {"pc0": pc0, "moved": moved, "gt": gt, "est": est, "pid": pid, "valid": valid, "sensor_dt": sensor_dt}
