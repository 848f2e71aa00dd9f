"""A numpy float64 restatement of the two additions to "flow metrics, v1" (himo_amd/eval_flow.py, csrc/flowmetrics.hip): rule 3b,
residual estimates, and rule 9, the accuracy table -- written from the rule's text, per sweep, every operation a separate numpy
operation in the order the rule gives.  A checker for the tests only: it shares no code with the product; rules 1, 2, 5-8 come
from tests/flowmetrics_ref.py."""
import numpy as np

import flowmetrics_ref as ref

STRICT, RELAXED = 0.05, 0.1                  # the doubles nearest 0.05 and 0.1
GROUPS = ("ALL", "FD", "FS", "BS")
# the throw-away prototype's table for the fixture below (result ``a`` under av2; the same in residual mode)
FIXTURE_TABLE = [[524, 363, 513], [325, 279, 318], [44, 19, 43], [140, 59, 138]]


def pose_flow(frame, pose_is_ego=False):
    """``T p - p`` in float64, the chain of rule 2: [N][3]"""
    gt = np.asarray(frame["flow"], dtype=np.float32).astype(np.float64)
    return gt - ref.ego_free_flow(frame, pose_is_ego)


def errors(frame, name, residual=False, pose_is_ego=False):
    """(epe float64 [N], finite bool [N]) of result ``name`` (``raw``: no estimate) by rule 3, or by rule 3b with ``residual``"""
    g = ref.ego_free_flow(frame, pose_is_ego)
    if name == "raw":
        return ref.norm3(-g), np.ones(len(g), dtype=bool)
    est = np.asarray(frame[name], dtype=np.float32)
    finite = np.isfinite(est).all(axis=1)
    gt = np.asarray(frame["flow"], dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = est.astype(np.float64) - (g if residual else gt)
        return ref.norm3(d), finite


def flow_accuracy_ref(frames, res_names, data_name, sensor_dt=0.1, residual=False, lut=None, pose_is_ego=False):
    """(buckets int64 [R][5][51][3], threeway int64 [F][R][3][2], rejected int64 [R], accuracy int64 [R][4][3]) of the sweeps
    ``frames``; ``residual``: every stored result is an ego-motion-free residual (rule 3b)"""
    lut = ref.class_table() if lut is None else np.asarray(lut, dtype=np.uint8)
    R = len(res_names)
    buckets = np.zeros((R, 5, 51, 3), dtype=np.int64)
    threeway = np.zeros((len(frames), R, 3, 2), dtype=np.int64)
    rejected = np.zeros(R, dtype=np.int64)
    accuracy = np.zeros((R, 4, 3), dtype=np.int64)
    thr = 0.5 * sensor_dt
    for f, frame in enumerate(frames):
        if np.asarray(frame["pc0"]).shape[0] == 0:
            continue
        counted = ref.counted_mask(frame, data_name)
        speed = ref.speeds(frame, pose_is_ego)
        cls = lut[np.asarray(frame["flow_category_indices"]).astype(np.uint8)]
        bucket = ref.bucket_of(speed, sensor_dt)
        dynamic = speed > thr
        kind = np.where(cls != 0, np.where(dynamic, 0, 1), np.where(dynamic, 3, 2))
        qs = ref.quantise(np.where(counted, speed, 0.0))
        gt = np.asarray(frame["flow"], dtype=np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            gn = ref.norm3(gt)                                       # the STORED ground truth, ego motion included
            lim_strict, lim_relaxed = STRICT * gn, RELAXED * gn
        for r, name in enumerate(res_names):
            epe, finite = errors(frame, name, residual, pose_is_ego)
            with np.errstate(invalid="ignore"):
                rej = counted & (~finite | ~(epe < 1024.0))
                strict = (epe < STRICT) | (epe < lim_strict)
                relaxed = (epe < RELAXED) | (epe < lim_relaxed)
            take = counted & ~rej
            rejected[r] += int(rej.sum())
            qe = ref.quantise(np.where(take, epe, 0.0))
            sel = take & (cls < 5)
            where = (cls[sel].astype(np.int64), bucket[sel])
            np.add.at(buckets[r, :, :, 0], where, 1)
            np.add.at(buckets[r, :, :, 1], where, qe[sel])
            np.add.at(buckets[r, :, :, 2], where, qs[sel])
            for k in range(3):
                m = take & (kind == k)
                threeway[f, r, k] += (int(m.sum()), int(qe[m].sum()))
            for grp in range(4):                                     # 0 = ALL, then rule 7's kinds
                m = take if grp == 0 else take & (kind == grp - 1)
                accuracy[r, grp] += (int(m.sum()), int((m & strict).sum()), int((m & relaxed).sum()))
    return buckets, threeway, rejected, accuracy


def accuracy_means(accuracy_r):
    """({group: strict / count}, {group: relaxed / count}) of ONE result's table [4][3]; nan where count is 0"""
    nan = float("nan")
    strict = {g: int(accuracy_r[k][1]) / int(accuracy_r[k][0]) if accuracy_r[k][0] > 0 else nan for k, g in enumerate(GROUPS)}
    relaxed = {g: int(accuracy_r[k][2]) / int(accuracy_r[k][0]) if accuracy_r[k][0] > 0 else nan for k, g in enumerate(GROUPS)}
    return strict, relaxed


def threshold_margin(frames, name, residual=False):
    """the smallest distance of a counted point's epe from the four thresholds 0.05, 0.1, 0.05 gn, 0.1 gn"""
    worst = np.inf
    for frame in frames:
        if np.asarray(frame["pc0"]).shape[0] == 0:
            continue
        counted = ref.counted_mask(frame, "av2")
        epe, finite = errors(frame, name, residual)
        gn = ref.norm3(np.asarray(frame["flow"], dtype=np.float32).astype(np.float64))
        m = counted & finite & (epe < 1024.0)
        if m.any():
            e, n = epe[m], gn[m]
            worst = min(worst, float(np.min([np.abs(e - STRICT), np.abs(e - RELAXED), np.abs(e - STRICT * n), np.abs(e - RELAXED * n)])))
    return worst


def fixture():
    """the issue's fixture: 3 sweeps of 300 points with FS populated; result ``a`` = the ground truth + N(0, 0.04), ``res`` = its
    residual float32(a - pose_flow)"""
    from himo_amd.synthetic import make_scene
    frames = make_scene(7, 3, n_points=300, scene_id="acc", n_instances=6)
    rng = np.random.default_rng(5)
    for f in frames:
        cat = np.array(f["flow_category_indices"])
        cat[np.flatnonzero(cat == 0)[::4]] = 19
        f["flow_category_indices"] = cat
        f["a"] = np.float32(f["flow"] + rng.normal(0, 0.04, f["flow"].shape))
        f["res"] = np.float32(f["a"] - pose_flow(f))
    return frames
