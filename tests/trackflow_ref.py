"""Pure-Python / numpy restatement of "track flow, v1" (the module docstring of himo_amd/track_flow.py is the rule): rules A-E, one
operation at a time in the written order, loops over rows where the order matters.  The checker of himo_amd/csrc/trackflow.hip: plan
outputs and flows are compared bit for bit.  It shares no code with the package; ``a = E p`` is tests/accumulate_ref.py's restatement of
``himo_rigid_transform``."""
from collections import namedtuple

import numpy as np

import accumulate_ref as acc

f32, f64 = np.float32, np.float64
NONE, MOVING, STATIC = 0, 1, 2
Sweep = namedtuple("Sweep", "boxes id w U sorted_id sorted_row")
Plan = namedtuple("Plan", "state m shift disp u")


def scene_transform(pose0, pose0_first):
    return np.linalg.inv(np.asarray(pose0_first, f64)) @ np.asarray(pose0, f64)


def prepare(box_rows, track_rows, pose0, pose0_first) -> Sweep:
    """rule A"""
    b = np.ascontiguousarray(box_rows, dtype=f32).reshape(-1, 12)
    tr = np.asarray(track_rows, dtype=f64).reshape(len(b), 6)
    T = scene_transform(pose0, pose0_first)
    U = np.ascontiguousarray(np.linalg.inv(T)[:3, :3]).reshape(9)
    ids, ws, labels = [], [], []
    with np.errstate(all="ignore"):
        for r in range(len(b)):
            tid = int(min(tr[r, 0], 2.0 ** 31 - 1)) if np.isfinite(tr[r, 0]) else -1
            vx, vy, vz = f64(b[r, 7]), f64(b[r, 8]), f64(b[r, 9])
            w = [(T[e, 0] * vx + T[e, 1] * vy) + T[e, 2] * vz for e in range(3)]
            usable = tid >= 0 and all(np.isfinite(c) for c in w)
            ids.append(tid if usable else -1)
            ws.append(w if usable else [np.nan] * 3)
            lab = float(b[r, 10])
            labels.append(int(min(max(lab, -2.0 ** 31), 2.0 ** 31 - 1)) if np.isfinite(lab) else 0)
    order = sorted(range(len(b)), key=lambda r: (labels[r], r))     # ascending and stable: among equal ids the lowest row first
    return Sweep(b, np.asarray(ids, np.int32).reshape(-1), np.asarray(ws, f64).reshape(-1, 3), U,
                 np.asarray([labels[r] for r in order], np.int32).reshape(-1), np.asarray(order, np.int32).reshape(-1))


def plan_scene(sweeps, sensor_dt=0.1, motion_min=0.05, half=2, min_len=3):
    """rules B-D for one scene: a ``Plan`` per sweep"""
    K = len(sweeps)
    L = {}
    for s in sweeps:
        for t in s.id.tolist():
            if t >= 0:
                L[t] = L.get(t, 0) + 1
    dt, mm = f64(sensor_dt), f64(motion_min)
    out = []
    with np.errstate(all="ignore"):
        for k, s in enumerate(sweeps):
            F = len(s.id)
            state, m = np.zeros(F, np.int32), np.zeros(F, np.int32)
            shift, disp, u = np.zeros((F, 3), f32), np.zeros((F, 3), f32), np.zeros((F, 3), f64)
            for r in range(F):
                t = int(s.id[r])
                if t < 0 or L[t] < min_len:
                    continue
                S, cnt = [f64(0.0)] * 3, 0
                for j in range(max(0, k - half), min(K - 1, k + half) + 1):
                    rows = np.flatnonzero(sweeps[j].id == t)
                    if len(rows):
                        S = [S[e] + sweeps[j].w[rows[0], e] for e in range(3)]
                        cnt += 1
                wb = [S[e] / f64(cnt) for e in range(3)]
                ds = []
                for e in range(3):
                    ue = (s.U[3 * e] * wb[0] + s.U[3 * e + 1] * wb[1]) + s.U[3 * e + 2] * wb[2]
                    de = ue * dt
                    db = f64(s.boxes[r, 7 + e]) * dt
                    u[r, e], shift[r, e], disp[r, e] = ue, f32(de - db), f32(de)
                    ds.append(de)
                d2 = (ds[0] * ds[0] + ds[1] * ds[1]) + ds[2] * ds[2]
                state[r], m[r] = (STATIC if d2 < mm * mm else MOVING), cnt
            out.append(Plan(state, m, shift, disp, u))
    return out


def plan(scenes, **params):
    """the packed outputs of a call over several scenes: (state, m, shift, disp, u)"""
    parts = [p for sc in scenes for p in plan_scene(sc, **params)]
    cat = lambda k, tail, dt: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) if parts else np.zeros((0,) + tail, dt)      # noqa: E731
    return cat(0, (), np.int32), cat(1, (), np.int32), cat(2, (3,), f32), cat(3, (3,), f32), cat(4, (3,), f64)


def ego_transform(pose0, pose1):
    E = (np.linalg.inv(np.asarray(pose1, f64)) @ np.asarray(pose0, f64)).astype(f32)
    return np.ascontiguousarray(E[:3]).reshape(12)


def apply_sweep(pc0, flow, label, E, sweep: Sweep, pl: Plan, mode=0):
    """rule E for one sweep: (out float32 [N, 3], rows written as MOVING, rows written as STATIC)"""
    p = np.asarray(pc0, f32)[:, :3]
    fl = np.ascontiguousarray(flow, dtype=f32).reshape(-1, 3)
    lab = np.asarray(label).astype(np.int64).reshape(-1)
    out = fl.copy()
    F, N = len(sweep.sorted_id), len(p)
    if F == 0 or N == 0:
        return out, 0, 0
    T = np.concatenate([np.asarray(E, f32).reshape(3, 4), np.array([[0, 0, 0, 1]], f32)])
    with np.errstate(all="ignore"):
        ego = (acc.rigid_move(p, T) - p).astype(f32)
        sid = sweep.sorted_id.astype(np.int64)
        pos = np.clip(np.searchsorted(sid, lab, side="left"), 0, F - 1)
        hit = (lab > 0) & (sid[pos] == lab)
        row = sweep.sorted_row[pos]
        st = np.where(hit, pl.state[row], NONE)
        ok = (st != NONE) & np.isfinite(fl).all(axis=1)
        static, moving = ok & (st == STATIC), ok & (st != STATIC)
        out[static] = ego[static]
        if mode == 0:
            out[moving] = (fl[moving] + pl.shift[row[moving]]).astype(f32)
        else:
            out[moving] = (ego[moving] + pl.disp[row[moving]]).astype(f32)
    return out, int(moving.sum()), int(static.sum())


# ---- synthetic scenes ------------------------------------------------------------------------------------------------------------------
def ego_pose(k, speed=8.0, turn=0.02, dt=0.1):
    """the pose of sweep k of an ego that drives and turns"""
    yaw = turn * k
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0, speed * dt * k], [s, c, 0.0, 0.3 * k * dt], [0.0, 0.0, 1.0, 0.01 * k], [0.0, 0.0, 0.0, 1.0]])


def constant_velocity_tracks(rng, n_tracks=40, n_sweeps=12, sigma=0.5):
    """(stored box rows, stored track rows, poses, the true sensor-frame velocity [K, n, 3]) of tracks at constant world velocity seen
    from a moving ego, every box velocity with iid Gaussian noise"""
    vel = np.concatenate([rng.uniform(-20, 20, (n_tracks, 2)), rng.uniform(-0.5, 0.5, (n_tracks, 1))], axis=1)
    boxes, tracks, poses, truth = [], [], [], []
    for k in range(n_sweeps):
        pose = ego_pose(k)
        v = vel @ pose[:3, :3]                                      # R^T v per row
        b = np.zeros((n_tracks, 12), f32)
        b[:, 3:6] = (4.5, 1.9, 1.6)
        b[:, 7:10] = v + rng.normal(0.0, sigma, v.shape)
        b[:, 10] = np.arange(1, n_tracks + 1)
        t = np.zeros((n_tracks, 6))
        t[:, 0], t[:, 1] = np.arange(n_tracks), k + 1
        boxes.append(b), tracks.append(t), poses.append(pose), truth.append(v)
    return boxes, tracks, poses, np.asarray(truth)
