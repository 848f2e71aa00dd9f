"""The checker of sweep odometry: a numpy / Python restatement of rules 0-5 of "sweep odometry, v1" (the module docstring of
``himo_amd/odometry.py`` is the text; parity with the reference is unpinned: it has no such stage).  The move and the distances are
float32 / float64 operation by operation, the neighbour is a search over the 3 x 3 cells (``nearest``) or all map rows masked to
them (``nearest_brute``), the sums are float64 in row order, the solve and the update are Python floats operation by operation.
The downsampling is ``tests/accumulate_ref.py`` and the vote ``tests/icpflow_ref.py``, as the rule says.  Nothing under ``himo_amd/``
imports this file; it imports nothing from there either (parameters come as keywords)."""
import math

import numpy as np

import accumulate_ref
import icpflow_ref

DEFAULTS = dict(voxel=0.5, window=10, max_dist=1.0, gm_scale=0.25, min_pairs=20, iters=20, eps_t2=1e-10, eps_r2=1e-12, min_ratio=0.3,
                bin=0.25, half=16, z_gate=1.0, x0=-64.0, y0=-64.0, z0=-8.0, extent_xy=128.0, extent_z=16.0, init="model")
RUNNING, CONVERGED, FAILED_PAIRS, FAILED_SOLVE = 0, 1, 2, 3

f32, f64 = np.float32, np.float64


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def accum_kw(**kw):
    """rule 1: the ONE grid of both downsamplings, as keywords of accumulate_ref"""
    p = params(**kw)
    v = float(p["voxel"])
    cells = lambda extent, top: max(1, min(top, int(math.ceil(extent / v))))        # noqa: E731
    return dict(x0=p["x0"], y0=p["y0"], z0=p["z0"], voxel=v, nx=cells(p["extent_xy"], 4096), ny=cells(p["extent_xy"], 4096),
                nz=cells(p["extent_z"], 256))


def search_grid(**kw):
    """rule 3: (x0, y0, cell, inv_cell as float32, gw, gh) of the BEV search grid: cell edge max_dist over the accumulation grid's extent"""
    p = params(**kw)
    cell = f32(p["max_dist"])
    g = max(1, int(math.ceil(p["extent_xy"] / float(cell))))
    return f32(p["x0"]), f32(p["y0"]), cell, f32(1.0) / cell, g, g


def source(sweep, skip=None, **kw):
    """rule 1: S_k, float32 [n, 3] in ascending key order"""
    return accumulate_ref.accumulate([(sweep, np.eye(4), 0, skip)], **accum_kw(**kw))[1]


def local_map(sweeps, poses, k, skips=None, **kw):
    """rule 1: M_k, the sweeps max(0, k - window) .. k - 1 in the frame of sweep k - 1"""
    w = int(params(**kw)["window"])
    return accumulate_ref.accumulate_target(sweeps[:k], poses[:k], k - 1, w - 1, skips=None if skips is None else skips[:k], **accum_kw(**kw))[1]


# ---- rule 3 -------------------------------------------------------------------------------------------------------------------------
def move(T, src):
    """m = float32(T p), every component ((T0 x + T1 y) + T2 z) + T3 in float64"""
    T = np.asarray(T, f64).reshape(3, 4)
    p = np.asarray(src, f32)[:, :3].astype(f64)
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1).astype(f32)


def cell_of(v, v0, inv_cell, g):
    """clamp((int)floor((v - v0) * inv_cell), 0, g - 1) in float32; rows outside go to the border cells"""
    with np.errstate(all="ignore"):
        f = np.floor(((np.asarray(v, f32) - v0).astype(f32) * inv_cell).astype(f32))
    return np.clip(np.nan_to_num(f, nan=0.0, posinf=float(g), neginf=-1.0), 0, g - 1).astype(np.int64)


def _d2(m, q):
    with np.errstate(all="ignore"):
        d = (q - m).astype(f32)
        return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def nearest_brute(m, mp, **kw):
    """(d2 float32 [n], row int32 [n]): every map row whose cell is within one cell of m's in x and in y, ties to the lowest row; (+inf,
    -1) without a candidate or for a non-finite m"""
    x0, y0, _, inv, gw, gh = search_grid(**kw)
    m, mp = np.asarray(m, f32).reshape(-1, 3), np.asarray(mp, f32).reshape(-1, 3)
    d2, idx = np.full(len(m), np.inf, f32), np.full(len(m), -1, np.int32)
    if len(mp) == 0 or len(m) == 0:
        return d2, idx
    cxm, cym = cell_of(mp[:, 0], x0, inv, gw), cell_of(mp[:, 1], y0, inv, gh)
    cx, cy = cell_of(m[:, 0], x0, inv, gw), cell_of(m[:, 1], y0, inv, gh)
    for lo in range(0, len(m), 256):
        s = slice(lo, lo + 256)
        dd = _d2(m[s, None, :], mp[None, :, :]).astype(f32)
        near = (np.abs(cx[s, None] - cxm[None, :]) <= 1) & (np.abs(cy[s, None] - cym[None, :]) <= 1) & ~np.isnan(dd)
        dd = np.where(near, dd, f32(np.inf))
        j = dd.argmin(1)                                            # (the first of equals: the lowest row)
        got = near[np.arange(len(j)), j] & np.isfinite(m[s]).all(1)
        d2[s], idx[s] = np.where(got, dd[np.arange(len(j)), j], f32(np.inf)), np.where(got, j, -1)
    return d2, idx


def nearest(m, mp, **kw):
    """``nearest_brute`` by cells: the map rows sorted by cell, then per neighbour cell and per position in it, vectorised over m"""
    x0, y0, _, inv, gw, gh = search_grid(**kw)
    m, mp = np.asarray(m, f32).reshape(-1, 3), np.asarray(mp, f32).reshape(-1, 3)
    d2, idx = np.full(len(m), np.inf, f32), np.full(len(m), -1, np.int64)
    if len(mp) == 0 or len(m) == 0:
        return d2, idx.astype(np.int32)
    cm = cell_of(mp[:, 1], y0, inv, gh) * gw + cell_of(mp[:, 0], x0, inv, gw)
    order = np.argsort(cm, kind="stable")
    start = np.searchsorted(cm[order], np.arange(gw * gh + 1))
    cx, cy = cell_of(m[:, 0], x0, inv, gw), cell_of(m[:, 1], y0, inv, gh)
    ok = np.isfinite(m).all(1)
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            nx, ny = cx + ox, cy + oy
            inside = ok & (nx >= 0) & (nx < gw) & (ny >= 0) & (ny < gh)
            c = np.where(inside, ny * gw + nx, 0)
            lo, cnt = start[c], np.where(inside, start[c + 1] - start[c], 0)
            for j in range(int(cnt.max(initial=0))):
                at = np.flatnonzero(cnt > j)
                row = order[lo[at] + j]
                dd = _d2(m[at], mp[row]).astype(f32)
                better = ~np.isnan(dd) & ((dd < d2[at]) | ((dd == d2[at]) & ((idx[at] < 0) | (row < idx[at]))))
                d2[at[better]], idx[at[better]] = dd[better], row[better]
    return d2, idx.astype(np.int32)


TERMS = 28           # the 21 upper entries of H (row-major), the 6 of g, the cost


def terms(m, q, gm_scale):
    """float64 [n, 28]: every inlier's contribution to the 28 sums, each entry as the rule writes it"""
    m, q = np.asarray(m, f32).astype(f64), np.asarray(q, f32).astype(f64)
    s = f64(f32(gm_scale))
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    r = q - m
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    rr = (rx * rx + ry * ry) + rz * rz
    u = s / (s + rr)
    w = u * u
    o = np.zeros_like(w)
    wx, wy, wz = w * x, w * y, w * z
    cols = [w, o, o, o, wz, -wy,
            w, o, -wz, o, wx,
            w, wy, -wx, o,
            w * (y * y + z * z), -(w * (x * y)), -(w * (x * z)),
            w * (x * x + z * z), -(w * (y * z)),
            w * (x * x + y * y),
            w * rx, w * ry, w * rz, w * (y * rz - z * ry), w * (z * rx - x * rz), w * (x * ry - y * rx),
            w * rr]
    return np.stack(cols, axis=1) if len(w) else np.zeros((0, TERMS))


def row_order_sums(t):
    """float64 [28]: the sums taken row by row"""
    return np.cumsum(t, axis=0)[-1] if len(t) else np.zeros(TERMS)


def cholesky_solve(sums):
    """xi (6 Python floats) of H xi = g by the unpivoted Cholesky of the rule, or None (a pivot not finite or not > 0, xi not finite)"""
    s = [float(v) for v in sums]
    H = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = s[at]
            at += 1
    g = s[21:27]
    L = [[0.0] * 6 for _ in range(6)]
    with np.errstate(all="ignore"):
        for j in range(6):
            d = f64(H[j][j])
            for k in range(j):
                d = d - f64(L[j][k]) * f64(L[j][k])
            if not (np.isfinite(d) and d > 0.0):
                return None
            L[j][j] = np.sqrt(d)
            for i in range(j + 1, 6):
                v = f64(H[j][i])
                for k in range(j):
                    v = v - f64(L[i][k]) * f64(L[j][k])
                L[i][j] = v / L[j][j]
        yv = [f64(0.0)] * 6
        for i in range(6):
            v = f64(g[i])
            for k in range(i):
                v = v - L[i][k] * yv[k]
            yv[i] = v / L[i][i]
        xi = [f64(0.0)] * 6
        for i in range(5, -1, -1):
            v = yv[i]
            for k in range(i + 1, 6):
                v = v - L[k][i] * xi[k]
            xi[i] = v / L[i][i]
    if not all(np.isfinite(v) for v in xi):
        return None
    return [float(v) for v in xi]


def cayley(omega):
    """D, float64 [3, 3], of the rotation vector omega: a = omega / 2, ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a)"""
    ax, ay, az = (f64(0.5) * f64(v) for v in omega)
    bx, by, bz = f64(2.0) * ax, f64(2.0) * ay, f64(2.0) * az
    aa = (ax * ax + ay * ay) + az * az
    one, den = f64(1.0) - aa, f64(1.0) + aa
    return np.array([[(one + bx * ax) / den, (bx * ay - bz) / den, (bx * az + by) / den],
                     [(by * ax + bz) / den, (one + by * ay) / den, (by * az - bx) / den],
                     [(bz * ax - by) / den, (bz * ay + bx) / den, (one + bz * az) / den]], f64)


def compose(T, xi):
    """R <- D R, t <- D t + t_xi on the 3 x 4 transform, every entry (D0 a + D1 b) + D2 c"""
    T = np.asarray(T, f64).reshape(3, 4)
    D = cayley(xi[3:])
    N = np.empty((3, 4), f64)
    for i in range(3):
        for j in range(3):
            N[i, j] = (D[i, 0] * T[0, j] + D[i, 1] * T[1, j]) + D[i, 2] * T[2, j]
        N[i, 3] = ((D[i, 0] * T[0, 3] + D[i, 1] * T[1, 3]) + D[i, 2] * T[2, 3]) + f64(xi[i])
    return N


def new_state(T=None):
    return {"T": np.eye(4)[:3].copy() if T is None else np.asarray(T, f64).reshape(-1)[:12].reshape(3, 4).copy(), "status": RUNNING, "iters": 0,
            "pairs": 0, "cost": 0.0, "xi": [0.0] * 6, "sums": np.zeros(TERMS)}


def finish(state, sums, n, **kw):
    """the end of a pass, given its 28 sums and its count: what the one solving thread does"""
    p = params(**kw)
    st = dict(state)
    st["sums"], st["cost"], st["pairs"], st["iters"] = np.asarray(sums, f64).copy(), float(sums[27]), int(n), state["iters"] + 1
    if n < int(p["min_pairs"]):
        st["status"] = FAILED_PAIRS
        return st
    xi = cholesky_solve(sums)
    if xi is None:
        st["status"] = FAILED_SOLVE
        return st
    st["xi"], st["T"] = xi, compose(state["T"], xi)
    tt = (f64(xi[0]) * f64(xi[0]) + f64(xi[1]) * f64(xi[1])) + f64(xi[2]) * f64(xi[2])
    oo = (f64(xi[3]) * f64(xi[3]) + f64(xi[4]) * f64(xi[4])) + f64(xi[5]) * f64(xi[5])
    if tt < f64(p["eps_t2"]) and oo < f64(p["eps_r2"]):
        st["status"] = CONVERGED
    return st


def pairs_of(src, mp, T, search=None, **kw):
    """(m, d2, idx, inlier) of one pass"""
    p = params(**kw)
    m = move(T, src)
    d2, idx = (search or nearest)(m, mp, **kw)
    md = f32(p["max_dist"])
    return m, d2, idx, (idx >= 0) & (d2 <= f32(md * md))


def step(src, mp, state, search=None, **kw):
    """one iteration; a state that is not RUNNING comes back as it is"""
    if state["status"] != RUNNING:
        return state
    p = params(**kw)
    mp = np.asarray(mp, f32).reshape(-1, 3)
    m, _, idx, inl = pairs_of(src, mp, state["T"], search, **kw)
    t = terms(m[inl], mp[idx[inl]], p["gm_scale"])
    return finish(state, row_order_sums(t), int(inl.sum()), **kw)


def register(src, mp, T_init=None, **kw):
    """rule 4: ``iters`` steps from T_init; (state, accepted)"""
    p = params(**kw)
    st = new_state(T_init)
    for _ in range(int(p["iters"])):
        st = step(src, mp, st, **kw)
    n = len(np.asarray(src).reshape(-1, np.asarray(src).shape[-1])) if np.asarray(src).size else 0
    return st, accepted(st, n, **kw)


def accepted(state, n_src, **kw):
    return state["status"] in (RUNNING, CONVERGED) and n_src > 0 and state["pairs"] / n_src >= float(f32(params(**kw)["min_ratio"]))


def vote_init(src, mp, **kw):
    """rule 2: the peak of the translation vote with S_k as one cluster: the 3 x 4 start, identity rotation"""
    p = params(**kw)
    src = np.asarray(src, f32).reshape(-1, 3)
    _, peaks, _ = icpflow_ref.vote(src, np.ones(len(src), np.int32), 1, mp, bin=p["bin"], half=p["half"], z_gate=p["z_gate"])
    T = np.eye(4)[:3].copy()
    T[0, 3], T[1, 3] = f64(int(peaks[0, 0])) * f64(f32(p["bin"])), f64(int(peaks[0, 1])) * f64(f32(p["bin"]))
    return T


def as44(T):
    out = np.eye(4)
    out[:3] = np.asarray(T, f64).reshape(3, 4)
    return out


def scene(sweeps, skips=None, pose_first=None, **kw):
    """rules 1-5 over a scene: (poses float64 [K, 4, 4], per sweep k >= 1 a dict: status, iters, pairs, rows, accepted, init, T)"""
    p = params(**kw)
    poses = [np.eye(4) if pose_first is None else np.asarray(pose_first, f64).copy()]
    info, prev, failed = [], None, True
    for k in range(1, len(sweeps)):
        S = source(sweeps[k], None if skips is None else skips[k], **kw)
        M = local_map(sweeps, poses, k, skips, **kw)
        use_vote = p["init"] == "vote" or (p["init"] == "model" and (prev is None or failed))
        T0 = vote_init(S, M, **kw) if use_vote else prev[:3]
        st, ok = register(S, M, T0, **kw)
        predicted = np.eye(4) if prev is None else prev
        T = as44(st["T"]) if ok else predicted
        info.append({"status": st["status"], "iters": st["iters"], "pairs": st["pairs"], "rows": len(S), "accepted": ok,
                     "init": "vote" if use_vote else "model", "T": T, "T_init": as44(T0)})
        poses.append(poses[-1] @ T)
        prev, failed = T, not ok
    return np.stack(poses), info


def relative_errors(est, gt):
    """per sweep pair (translation error [m], rotation error [degrees]) of inv(est_{k-1}) est_k against the same of gt"""
    out = []
    for k in range(1, len(est)):
        a = np.linalg.inv(est[k - 1]) @ est[k]
        b = np.linalg.inv(gt[k - 1]) @ gt[k]
        e = np.linalg.inv(b) @ a
        c = min(1.0, max(-1.0, (np.trace(e[:3, :3]) - 1.0) / 2.0))
        out.append((float(np.linalg.norm(e[:3, 3])), math.degrees(math.acos(c))))
    return out


# ---- the drives of the tests ------------------------------------------------------------------------------------------------------------
DRIVE_SEED, DRIVE_SWEEPS, DRIVE_POINTS, DRIVE_INSTANCES = 3, 6, 8000, 8
CLOUDS = ("uniform", "rings")
_drives = {}


def drive(cloud):
    """(frames, gt poses [K, 4, 4], the restatement's poses, its per-sweep info) of the synthetic drive the tests share, computed once"""
    if cloud not in _drives:
        from himo_amd.synthetic import make_scene
        fr = make_scene(DRIVE_SEED, DRIVE_SWEEPS, n_points=DRIVE_POINTS, n_instances=DRIVE_INSTANCES, cloud=cloud)
        poses, info = scene([f["pc0"] for f in fr], pose_first=fr[0]["pose0"])
        _drives[cloud] = (fr, np.stack([f["pose0"] for f in fr]), poses, info)
    return _drives[cloud]


if __name__ == "__main__":
    import sys
    import time
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
    from himo_amd.synthetic import make_scene
    for cloud in ("uniform", "rings"):
        for seed in (3,):
            fr = make_scene(seed, 6, n_points=8000, n_instances=8, cloud=cloud)
            t0 = time.time()
            poses, info = scene([f["pc0"] for f in fr], pose_first=fr[0]["pose0"])
            gt = [f["pose0"] for f in fr]
            for i, e in zip(info, relative_errors(poses, gt)):
                print(cloud, seed, i["init"], i["status"], i["iters"], i["pairs"], i["rows"], i["accepted"], "%.4f m %.4f deg" % e)
            print("seconds", time.time() - t0)
