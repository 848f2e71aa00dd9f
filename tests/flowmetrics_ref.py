"""A numpy float64 restatement of "flow metrics, v1" (himo_amd/eval_flow.py, csrc/flowmetrics.hip), rules 1-8, written from the
rule's text: per sweep, with masks, every operation a separate numpy operation in the order the rule gives.  A checker for the
tests only; it shares no code with the product (its class numbers and ego boxes are written out here)."""
import numpy as np

UNIT = 2.0 ** 24
CLOSE = np.float32(35.0)
BOX = {"av2": (np.float32([-1.5, -1.5, -2.0]), np.float32([1.5, 1.5, 2.0])),
       "scania": (np.float32([-9.5, -1.5, 0.0]), np.float32([5.0, 2.760004 / 2, 5.0]))}
# Argoverse-2 category numbers (0 = NONE, then the annotation categories in alphabetical order from 1)
CLASS_OF = {0: 0,                                                   # BACKGROUND
            19: 1,                                                  # CAR: REGULAR_VEHICLE
            2: 2, 6: 2, 7: 2, 11: 2, 18: 2, 20: 2, 25: 2, 26: 2, 27: 2,   # OTHER_VEHICLES
            16: 3, 17: 3, 23: 3, 28: 3,                             # PEDESTRIAN
            3: 4, 4: 4, 14: 4, 15: 4, 29: 4, 30: 4}                 # WHEELED_VRU
KINDS = ("FD", "FS", "BS")


def class_table():
    return np.array([CLASS_OF.get(v, 5) for v in range(256)], dtype=np.uint8)


def quantise(x):
    return np.rint(np.asarray(x, dtype=np.float64) * UNIT).astype(np.int64)


def counted_mask(frame, data_name):
    """rule 1 (float32, as the package's evaluation mask)"""
    p = np.asarray(frame["pc0"], dtype=np.float32)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    lo, hi = BOX[data_name]
    rng = np.sqrt(px * px + py * py)
    inside = (px > lo[0]) & (px < hi[0]) & (py > lo[1]) & (py < hi[1]) & (pz > lo[2]) & (pz < hi[2])
    m = (rng <= CLOSE) & (np.asarray(frame["gm0"]).astype(np.uint8) == 0) & ~inside
    if data_name == "scania":
        m &= np.asarray(frame["flow_is_valid"]).astype(np.uint8) != 0
    return m


def ego_free_flow(frame, pose_is_ego=False):
    """rule 2: g = gt - (T p - p) in float64, [N][3]"""
    T = np.asarray(frame["pose0"], dtype=np.float64) if pose_is_ego else \
        np.linalg.inv(np.asarray(frame["pose1"], dtype=np.float64)) @ np.asarray(frame["pose0"], dtype=np.float64)
    p = np.asarray(frame["pc0"], dtype=np.float32)[:, :3].astype(np.float64)
    gt = np.asarray(frame["flow"], dtype=np.float32).astype(np.float64)
    g = np.empty_like(gt)
    for c in range(3):
        dot = (p[:, 0] * T[c, 0] + p[:, 1] * T[c, 1]) + p[:, 2] * T[c, 2]
        g[:, c] = gt[:, c] - ((dot + T[c, 3]) - p[:, c])
    return g


def norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def speeds(frame, pose_is_ego=False):
    return norm3(ego_free_flow(frame, pose_is_ego))


def bucket_of(speed, sensor_dt=0.1):
    """rule 8: the number of k in 1..50 with speed >= k * w"""
    w = 0.4 * sensor_dt
    speed = np.asarray(speed, dtype=np.float64)
    b = np.zeros(speed.shape, dtype=np.int64)
    for k in range(1, 51):
        b += speed >= k * w
    return b


def flow_metrics_ref(frames, res_names, data_name, sensor_dt=0.1, lut=None, pose_is_ego=False):
    """(buckets int64 [R][5][51][3], threeway int64 [F][R][3][2], rejected int64 [R]) of the sweeps ``frames``"""
    lut = class_table() if lut is None else np.asarray(lut, dtype=np.uint8)
    R = len(res_names)
    buckets = np.zeros((R, 5, 51, 3), dtype=np.int64)
    threeway = np.zeros((len(frames), R, 3, 2), dtype=np.int64)
    rejected = np.zeros(R, dtype=np.int64)
    thr = 0.5 * sensor_dt
    for f, frame in enumerate(frames):
        if np.asarray(frame["pc0"]).shape[0] == 0:
            continue
        counted = counted_mask(frame, data_name)
        g = ego_free_flow(frame, pose_is_ego)
        speed = norm3(g)
        cls = lut[np.asarray(frame["flow_category_indices"]).astype(np.uint8)]
        bucket = bucket_of(speed, sensor_dt)
        dynamic = speed > thr
        kind = np.where(cls != 0, np.where(dynamic, 0, 1), np.where(dynamic, 3, 2))
        qs = quantise(np.where(counted, speed, 0.0))
        gt = np.asarray(frame["flow"], dtype=np.float32).astype(np.float64)
        for r, name in enumerate(res_names):
            if name == "raw":
                d, finite = -g, np.ones(len(g), dtype=bool)
            else:
                est = np.asarray(frame[name], dtype=np.float32)
                finite = np.isfinite(est).all(axis=1)
                with np.errstate(invalid="ignore", over="ignore"):
                    d = est.astype(np.float64) - gt
            with np.errstate(invalid="ignore", over="ignore"):
                epe = norm3(d)
                rej = counted & (~finite | (epe >= 1024.0))
            take = counted & ~rej
            rejected[r] += int(rej.sum())
            qe = quantise(np.where(take, epe, 0.0))
            sel = take & (cls < 5)                                   # class 5 is in no bucket
            where = (cls[sel].astype(np.int64), bucket[sel])
            np.add.at(buckets[r, :, :, 0], where, 1)
            np.add.at(buckets[r, :, :, 1], where, qe[sel])
            np.add.at(buckets[r, :, :, 2], where, qs[sel])
            for k in range(3):                                       # kind 3 (background, dynamic) is in none
                m = take & (kind == k)
                threeway[f, r, k] += (int(m.sum()), int(qe[m].sum()))
    return buckets, threeway, rejected


def means_ref(buckets, threeway):
    """rules 7 and 8 on the integer tables of ONE result: buckets [5][51][3], threeway [S][3][2] in dataset order"""
    nan = float("nan")
    out = {}
    for k, kind in enumerate(KINDS):
        per_sweep = [int(s[k][1]) / int(s[k][0]) / UNIT for s in threeway if s[k][0] > 0]
        out[kind] = sum(per_sweep[1:], per_sweep[0]) / len(per_sweep) if per_sweep else nan
    out["three_way"] = (out["FD"] + out["FS"] + out["BS"]) / 3
    static, dynamic = [], []
    for c in range(5):
        b = buckets[c]
        static.append(int(b[0][1]) / int(b[0][0]) / UNIT if b[0][0] > 0 else nan)
        ratios = [int(b[k][1]) / int(b[k][2]) for k in range(1, 51) if b[k][0] > 0]
        dynamic.append(float(np.mean(ratios)) if ratios else nan)
    out["static"], out["dynamic"] = static, dynamic
    for key, vals in (("mean_static", static), ("mean_dynamic", dynamic)):
        have = [v for v in vals if v == v]
        out[key] = float(np.mean(have)) if have else nan
    return out
