"""The restatement of "box tracking, v1" (the rule is the module docstring of himo_amd/track.py): rules A-F in plain Python float64, in
the rule's operation order, one operation a line where the order matters.  The kernel (himo_amd/csrc/boxtrack.hip) is compared with it
bit for bit (tests/test_box_track_gpu.py); it is itself checked against exact expectations (tests/test_box_track_cpu.py).  The BEV IoU
(rules B, C of box evaluation v1) and the sequential greedy matching (rule D) are those of tests/boxeval_ref.py, imported, not copied.
"""
import math

import numpy as np

import boxeval_ref as be

MAX = 512                           # HIMO_BOXTRACK_MAX
DEFAULTS = dict(min_iou=0.1, alpha=0.5, beta=0.5, max_age=2, max_tracks=512, vel_mode=0)
NAN12 = [math.nan] * 12


# ---- rule A ---------------------------------------------------------------------------------------------------------------------------------
def scene_transform(pose0, pose0_first):
    """``T_k = inv(pose0_first) @ pose0_k``, float64 [4, 4]"""
    return np.linalg.inv(np.asarray(pose0_first, dtype=np.float64)) @ np.asarray(pose0, dtype=np.float64)


def detection(row, T):
    """one box row (float32 [12] in ``box_fit``'s layout, widened) -> the twelve floats of its detection row in the scene frame"""
    x, y, z, l, w, h, yaw, vx, vy = (float(v) for v in row[:9])
    if not all(math.isfinite(v) for v in (x, y, z, l, w, h, yaw, vx, vy)) or l < 0 or w < 0 or h < 0:
        return list(NAN12)
    T = [[float(v) for v in r] for r in np.asarray(T, dtype=np.float64)]
    c = math.cos(yaw)
    s = math.sin(yaw)
    out = [((T[0][0] * x + T[0][1] * y) + T[0][2] * z) + T[0][3],
           ((T[1][0] * x + T[1][1] * y) + T[1][2] * z) + T[1][3],
           ((T[2][0] * x + T[2][1] * y) + T[2][2] * z) + T[2][3],
           l, w, h,
           T[0][0] * c + T[0][1] * s,
           T[1][0] * c + T[1][1] * s,
           T[0][0] * vx + T[0][1] * vy,
           T[1][0] * vx + T[1][1] * vy,
           0.0, 0.0]
    return out if all(math.isfinite(v) for v in out) else list(NAN12)


def detections(rows, pose0, pose0_first):
    T = scene_transform(pose0, pose0_first)
    return np.array([detection(r, T) for r in np.asarray(rows)], dtype=np.float64).reshape(-1, 12)


def det_valid(d):
    """the library's side of rule A"""
    return all(math.isfinite(float(v)) for v in d) and d[3] >= 0 and d[4] >= 0 and d[5] >= 0


# ---- rule C2 --------------------------------------------------------------------------------------------------------------------------------
def rect_cs(x, y, z, l, w, h, c, s):
    """rule A of box evaluation v1 with (c, s) given"""
    hl = l * 0.5
    hw = w * 0.5
    out = []
    for dx, dy in ((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw)):
        out += [x + (dx * c - dy * s), y + (dx * s + dy * c)]
    out += [z - h * 0.5, z + h * 0.5, l * w, 0.0]
    return out


# ---- rules B-E: one scene -------------------------------------------------------------------------------------------------------------------
def track_scene(dets, dts, min_iou=0.1, alpha=0.5, beta=0.5, max_age=2, max_tracks=512, vel_mode=0):
    """``dets``: one float64 [F_k, 12] detection table per sweep; ``dts``: one float per sweep (``dts[0]`` is not read).  Returns
    (sweeps, n_ids, overflow) with sweeps = [(track_id int32 [F], age int32 [F], state float64 [F, 4], iou float64 [F], live int)]."""
    table = []                                                      # [x, y, z, l, w, h, c, s, vx, vy, id, hits, misses] per live track, ascending id
    next_id, overflow, out = 0, 0, []
    with np.errstate(all="ignore"):
        for k, D in enumerate(dets):
            D = [[float(v) for v in d] for d in np.asarray(D, dtype=np.float64).reshape(-1, 12)]
            F = len(D)
            if F > MAX:
                raise ValueError("a sweep above the cap")
            # C1
            if k > 0:
                dt = float(dts[k])
                for tr in table:
                    tr[0] = tr[0] + tr[8] * dt
                    tr[1] = tr[1] + tr[9] * dt
            # C2
            ok = [det_valid(d) for d in D]
            RA = [rect_cs(*tr[:8]) for tr in table]
            RB = [rect_cs(*d[:8]) if v else list(NAN12) for d, v in zip(D, ok)]
            # C3, C4
            iou, _ = be.iou_matrix(np.array(RA, dtype=np.float64).reshape(-1, 12), np.array(RB, dtype=np.float64).reshape(-1, 12))
            ma, mb = be.greedy(iou, min_iou)
            ids, age = np.full(F, -1, np.int32), np.zeros(F, np.int32)
            state, ious = np.zeros((F, 4)), np.zeros(F)
            kept = []
            for i, tr in enumerate(table):
                j = int(ma[i])
                if j >= 0:                                          # C5
                    d = D[j]
                    rx = d[0] - tr[0]
                    ry = d[1] - tr[1]
                    if vel_mode == 0:
                        tr[8] = tr[8] + beta * (d[8] - tr[8])
                        tr[9] = tr[9] + beta * (d[9] - tr[9])
                    else:
                        tr[8] = tr[8] + beta * (rx / dt)
                        tr[9] = tr[9] + beta * (ry / dt)
                    tr[0] = tr[0] + alpha * rx
                    tr[1] = tr[1] + alpha * ry
                    tr[2:8] = d[2:8]
                    tr[11] += 1
                    tr[12] = 0
                    ids[j], age[j], state[j], ious[j] = tr[10], tr[11], (tr[0], tr[1], tr[8], tr[9]), iou[i, j]
                    kept.append(tr)
                else:                                               # C6
                    tr[12] += 1
                    if tr[12] <= max_age:
                        kept.append(tr)
            for j in range(F):                                      # C7
                if mb[j] >= 0 or not ok[j]:
                    continue
                if len(kept) >= max_tracks:
                    overflow += 1
                    continue
                d = D[j]
                v = (d[8], d[9]) if vel_mode == 0 else (0.0, 0.0)
                kept.append(d[:8] + [v[0], v[1], next_id, 1, 0])
                ids[j], age[j], state[j] = next_id, 1, (d[0], d[1], v[0], v[1])
                next_id += 1
            table = kept                                            # C8
            out.append((ids, age, state, ious, len(table)))
    return out, next_id, overflow


def track(scenes, dts, **params):
    """a batch: ``scenes`` = [[det table per sweep] per scene], ``dts`` = [[dt per sweep] per scene] -> the packed outputs of the entry
    point: (track_id, age, state, iou, live, scene_info int32 [n, 2])"""
    tid, age, state, iou, live, info = [], [], [], [], [], []
    for dets, dt in zip(scenes, dts):
        sweeps, n_ids, over = track_scene(dets, dt, **params)
        for a, b, c, d, e in sweeps:
            tid.append(a); age.append(b); state.append(c); iou.append(d); live.append(e)
        info.append((n_ids, over))
    cat = lambda parts, shape, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(shape, dtype)      # noqa: E731
    return (cat(tid, (0,), np.int32), cat(age, (0,), np.int32), cat(state, (0, 4), np.float64).reshape(-1, 4), cat(iou, (0,), np.float64),
            np.asarray(live, dtype=np.int32), np.asarray(info, dtype=np.int32).reshape(-1, 2))


# ---- rule F ---------------------------------------------------------------------------------------------------------------------------------
def stored_rows(track_id, age, state, det, pose0, pose0_first):
    """one sweep's ``tracks_<name>`` float64 [F, 6] = id, age, x, y, vx, vy with the state rotated back into the sweep's sensor frame (the
    z that goes with x, y is the detection's)"""
    U = [[float(v) for v in r] for r in np.linalg.inv(scene_transform(pose0, pose0_first))]
    out = np.zeros((len(track_id), 6))
    for j in range(len(track_id)):
        if track_id[j] < 0:
            out[j, 0] = -1.0
            continue
        x, y, vx, vy = (float(v) for v in state[j])
        z = float(det[j][2])
        out[j] = (float(track_id[j]), float(age[j]),
                  ((U[0][0] * x + U[0][1] * y) + U[0][2] * z) + U[0][3],
                  ((U[1][0] * x + U[1][1] * y) + U[1][2] * z) + U[1][3],
                  U[0][0] * vx + U[0][1] * vy,
                  U[1][0] * vx + U[1][1] * vy)
    return out


# ---- shared case builders -------------------------------------------------------------------------------------------------------------------
def moving_scene(rng, n_obj, n_sweeps, dt=0.1, noise=0.05, drop=0.0, spacing=9.0, speed=(0.0, 5.0, 15.0, 30.0)):
    """``n_obj`` boxes on a jittered grid, each with a constant velocity along its heading, seen over ``n_sweeps`` sweeps with centre
    noise; a detection is dropped with probability ``drop``; the order of a sweep's rows is random.  Detection tables in the scene
    frame (identity poses): [float64 [F_k, 12]]."""
    side = max(1, int(math.ceil(math.sqrt(n_obj))))
    k = np.arange(n_obj)
    c0 = np.stack([(k % side - side / 2) * spacing, (k // side - side / 2) * spacing], axis=1) + rng.uniform(-1, 1, (n_obj, 2))
    yaw = rng.uniform(-math.pi, math.pi, n_obj)
    v = rng.choice(speed, n_obj)
    vel = np.stack([v * np.cos(yaw), v * np.sin(yaw)], axis=1)
    size = np.stack([rng.uniform(3.5, 5.5, n_obj), rng.uniform(1.6, 2.2, n_obj)], axis=1)
    out = []
    for s in range(n_sweeps):
        seen = np.flatnonzero(rng.uniform(0, 1, n_obj) >= drop)
        seen = seen[rng.permutation(len(seen))]
        D = np.zeros((len(seen), 12))
        D[:, 0:2] = c0[seen] + vel[seen] * (s * dt) + rng.uniform(-noise, noise, (len(seen), 2))
        D[:, 2], D[:, 3:5], D[:, 5] = 0.5, size[seen], 1.6
        D[:, 6], D[:, 7] = np.cos(yaw[seen]), np.sin(yaw[seen])
        D[:, 8:10] = vel[seen] + rng.uniform(-0.2, 0.2, (len(seen), 2))
        out.append(D)
    return out
