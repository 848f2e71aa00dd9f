"""numpy float64 restatement of "ego de-skew, v1" (the module docstring of himo_amd/deskew.py is the rule): the reference time, the
per-row move in the rule's written order of operations, the counts and the greatest displacement; the twist of every sweep from a
pose chain (closed-form SE(3) logarithm); and ``skew_scene``, which turns the frames of ``synthetic.make_scene`` into sweeps skewed by
the true ego twist.  It shares no code with the product."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
SMALL_WW = 1e-16
LOG_SMALL = 1e-8
REFS = ("max", "min", "zero")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def t_ref(dt, ref="max") -> np.float32:
    dt = np.asarray(dt, f32)
    fin = dt[np.isfinite(dt)]
    if ref == "zero" or len(fin) == 0:
        return f32(0.0)
    return f32(fin.max() if ref == "max" else fin.min())


def _cross(a, b):
    """a x b with every component as ``a1*b2 - a2*b1`` (a, b: three arrays or scalars each)"""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def displacement(p, s, v, w, inverse=False):
    """the float64 displacement d of rows ``p`` [n, 3] (float64) for the factors ``s`` [n]: p' = p + d, in the rule's order"""
    x = (p[:, 0], p[:, 1], p[:, 2])
    v, w = [f64(c) for c in v], [f64(c) for c in w]
    g = s if inverse else -s
    ww = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if ww < SMALL_WW:
        c = _cross(w, x)
        return np.stack([g * c[k] + g * v[k] for k in range(3)], axis=1)
    theta = np.sqrt(ww)
    n = [w[k] / theta for k in range(3)]
    A = _cross(n, v)
    B = _cross(n, A)
    phi = g * theta
    half = 0.5 * phi
    sh, ch = np.sin(half), np.cos(half)
    sn, k1 = (2.0 * sh) * ch, (2.0 * sh) * sh
    q = _cross(n, x)
    r = _cross(n, q)
    ca, cb = k1 / theta, (phi - sn) / theta
    return np.stack([(((sn * q[k] + k1 * r[k]) + g * v[k]) + ca * A[k]) + cb * B[k] for k in range(3)], axis=1)


def deskew(pts, dt, twist, ref="max", inverse=False, tref=None):
    """one sweep: (rows float32 of the input's shape, counts [moved, passed], max_disp float32, t_ref float32)"""
    pts = np.asarray(pts, f32)
    dt = np.asarray(dt, f32)
    twist = np.asarray(twist, f64)
    v, w, span = twist[:3], twist[3:6], twist[6]
    tr = t_ref(dt, ref) if tref is None else f32(tref)
    out = pts.copy()
    with np.errstate(all="ignore"):
        s = (f64(tr) - dt.astype(f64)) / span
        ok = np.isfinite(pts[:, :3]).all(axis=1) & np.isfinite(dt) & (s != 0.0)
    if not (np.any(v != 0.0) or np.any(w != 0.0)):
        ok[:] = False
    if not ok.any():
        return out, np.array([0, len(pts)], np.int32), f32(0.0), tr
    p = pts[ok, :3].astype(f64)
    d = displacement(p, s[ok], v, w, inverse)
    out[ok, :3] = (p + d).astype(f32)
    disp = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)
    return out, np.array([int(ok.sum()), int((~ok).sum())], np.int32), f32(disp.max()), tr


# ---- SE(3) -------------------------------------------------------------------------------------------------------------------------------
def hat(xi):
    """the 4x4 matrix of the twist (v, w)"""
    v, w = np.asarray(xi[:3], f64), np.asarray(xi[3:6], f64)
    M = np.zeros((4, 4))
    M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M[:3, 3] = v
    return M


def log_se3(T):
    """(v, w) with Exp(v, w) = T, closed form; refuses what the rule refuses"""
    T = np.asarray(T, f64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("a finite [4, 4] pose")
    R, t = T[:3, :3], T[:3, 3]
    r = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = math.sqrt(float(r @ r))
    theta = math.atan2(sn, 0.5 * (float(np.trace(R)) - 1.0))
    if theta >= math.pi / 2:
        raise ValueError(f"a rotation of {theta:.3f} rad per sweep: the rule admits less than pi / 2")
    if theta < LOG_SMALL:
        w, c = r, 1.0 / 12.0
    else:
        w = r * (theta / sn)
        c = (1.0 - (0.5 * theta) / math.tan(0.5 * theta)) / (theta * theta)
    W = hat(np.concatenate([np.zeros(3), w]))[:3, :3]
    v = t - 0.5 * (W @ t) + c * (W @ (W @ t))
    return np.concatenate([v, w])


def twists_from_poses(poses, mode="backward", span=0.1, sensor_dt=0.1):
    """[K, 8] float64: v, w, span, 0 per sweep.  ``span``: seconds (fixed), or the K timestamps in ns (the difference of the pair used)"""
    poses = np.asarray(poses, f64).reshape(-1, 4, 4)
    K = len(poses)
    stamps = None if np.ndim(span) == 0 else np.asarray(span, np.int64)
    out = np.zeros((K, 8))
    rel = {k: log_se3(np.linalg.inv(poses[k - 1]) @ poses[k]) for k in range(1, K)}
    sp = {k: (float(span) if stamps is None else float(int(stamps[k]) - int(stamps[k - 1])) * 1e-9) for k in range(1, K)}
    for k in range(K):
        if K == 1:
            out[k, 6] = float(sensor_dt if stamps is not None else span)
            continue
        back, fwd = (k if k >= 1 else 1), (k + 1 if k + 1 < K else K - 1)
        use = {"backward": [back], "forward": [fwd], "central": [j for j in (k, k + 1) if 1 <= j < K]}[mode]
        out[k, :6] = sum(rel[j] for j in use) / len(use)
        out[k, 6] = sum(sp[j] for j in use) / len(use)
    return out


# ---- skewed drives ----------------------------------------------------------------------------------------------------------------------
def skew_scene(frames, dt_mode="random"):
    """The frames of ``make_scene`` as a sensor that turns while it drives would have recorded them: every row of sweep k moved by
    ``Exp(+s xi_k)`` with the TRUE twist (the logarithm of ``inv(pose0) pose1`` of the frame: the motion is the same in every sweep of
    a synthetic drive) and s = (max lidar_dt - lidar_dt) / 0.1.  ``dt_mode`` "random": the frames' own ``lidar_dt``; "azimuth":
    ``0.1 * (atan2(y, x) + pi) / (2 pi)`` of the true row, written back as ``lidar_dt``.  Returns new frame dicts (``pc0`` and
    ``lidar_dt`` replaced; everything else shared) -- the input frames are the instantaneous sweeps."""
    out = []
    for f in frames:
        pc = np.asarray(f["pc0"], f32)
        if dt_mode == "azimuth":
            dt = (0.1 * (np.arctan2(pc[:, 1].astype(f64), pc[:, 0].astype(f64)) + math.pi) / (2 * math.pi)).astype(f32)
        elif dt_mode == "random":
            dt = np.asarray(f["lidar_dt"], f32)
        else:
            raise ValueError(dt_mode)
        xi = log_se3(np.linalg.inv(f["pose0"]) @ f["pose1"])
        sk = deskew(pc, dt, np.concatenate([xi, [0.1, 0.0]]), "max", inverse=True)[0]
        out.append(dict(f, pc0=sk, lidar_dt=dt))
    return out


def row_errors(a, b):
    """per row |a - b| over x, y, z in float64"""
    return np.linalg.norm(np.asarray(a, f64)[:, :3] - np.asarray(b, f64)[:, :3], axis=1)


# ---- the drives of the tests --------------------------------------------------------------------------------------------------------------
DRIVE_SEED, DRIVE_SWEEPS, DRIVE_POINTS, DRIVE_INSTANCES = 3, 6, 8000, 8
_drives = {}


def drive(cloud, dt_mode):
    """(instantaneous frames, skewed frames) of the synthetic drive the tests share, computed once and never written to"""
    key = (cloud, dt_mode)
    if key not in _drives:
        from himo_amd.synthetic import make_scene
        if cloud not in _drives:
            _drives[cloud] = make_scene(DRIVE_SEED, DRIVE_SWEEPS, n_points=DRIVE_POINTS, n_instances=DRIVE_INSTANCES, cloud=cloud)
        _drives[key] = (_drives[cloud], skew_scene(_drives[cloud], dt_mode))
    return _drives[key]
