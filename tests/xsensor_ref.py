"""The numpy restatement of "cross-sensor consistency, v1" (the rule is the module docstring of ``himo_amd/eval_xsensor.py``): rules
A-F in row order, float32 arithmetic for the search, float64 for the per-row terms, Python integers for every sum.  It is the CHECKER
of the HIP kernels (tests/test_xsensor_gpu.py) and of the rule itself (tests/test_xsensor_cpu.py); nothing in the package imports it.
Also here: the synthetic vehicles the rule is tried on -- L-plus-roof surfaces sampled by three sensors, each with its own capture time
inside the sweep."""
import math

import numpy as np

SCORED, TOO_FEW, ONE_SENSOR, TOO_LARGE = 0, 1, 2, 3
DEFAULTS = dict(trunc=4.0, near=0.2, min_group=5, min_points=10, max_points=8192)
GROUPS = 8
UNIT = 1 << 24
CLIP = 1024.0
SENSOR_DT = 0.1


def q(x) -> int:
    """llrint(x * 2^24) of one float64 (ties to even, as the device's rounding mode)"""
    return int(np.rint(np.float64(x) * np.float64(UNIT)))


def sort_rows(labels, C):
    """(order int64 [nc], offsets int64 [C + 1]): the rows whose label is in 1..C, sorted by label, ascending row inside a cluster"""
    labels = np.asarray(labels).astype(np.int64)
    lab = np.where((labels >= 1) & (labels <= C), labels, 0)
    order = np.flatnonzero(lab > 0)
    order = order[np.argsort(lab[order], kind="stable")]
    offsets = np.zeros(C + 1, np.int64)
    np.cumsum(np.bincount(lab, minlength=C + 1)[1:C + 1], out=offsets[1:])
    return order, offsets


def usable_rows(pts, labels, group, C, dt=None):
    """rule A, bool [N]"""
    pts = np.asarray(pts, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64)
    ok = (labels >= 1) & (labels <= C) & np.isfinite(pts[:, :3]).all(axis=1) & (np.asarray(group).astype(np.int64) <= 7)
    if dt is not None:
        ok &= np.isfinite(np.asarray(dt, dtype=np.float32))
    return ok


def min_d2(q_xyz, c_xyz):
    """rule C for one group of queries against their candidates: float32 [nq], every operation rounding on its own"""
    out = np.full(len(q_xyz), np.inf, np.float32)
    with np.errstate(all="ignore"):
        for lo in range(0, len(q_xyz), 256):
            a = q_xyz[lo:lo + 256, None, :]
            d = a - c_xyz[None, :, :]                                 # float32 - float32
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            out[lo:lo + 256] = d2.min(axis=1)
    return out


def score(pts, labels, group, C, dt=None, motion=None, **params):
    """what ``himo_xsensor`` writes: (info int32 [C, 4], rec int64 [C, 8, 4], mot int64 [C, 2], m float32 [nc]); ``m`` is per SORTED
    row (``sort_rows``), +inf for a row that is not a query"""
    prm = dict(DEFAULTS, **params)
    pts = np.asarray(pts, dtype=np.float32)
    group = np.asarray(group).astype(np.int64)
    ok = usable_rows(pts, labels, group, C, dt)
    order, offsets = sort_rows(labels, C)
    info, rec, mot = np.zeros((C, 4), np.int32), np.zeros((C, GROUPS, 4), np.int64), np.zeros((C, 2), np.int64)
    m = np.full(len(order), np.inf, np.float32)
    trunc, near = float(np.float32(prm["trunc"])), float(np.float32(prm["near"]))
    for k in range(C):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        rows = order[lo:hi]
        use = ok[rows]
        n_g = [int((use & (group[rows] == g)).sum()) for g in range(GROUPS)]
        n = sum(n_g)
        live = [g for g in range(GROUPS) if n_g[g] >= prm["min_group"]]
        state = TOO_FEW if n < prm["min_points"] else TOO_LARGE if n > prm["max_points"] else ONE_SENSOR if len(live) < 2 else SCORED
        info[k, :2] = (state, n)
        rec[k, :, 0] = n_g
        if state != SCORED:
            continue
        is_live = use & np.isin(group[rows], live)
        queries = 0
        for g in range(GROUPS):
            mine = use & (group[rows] == g)
            if dt is not None:
                rec[k, g, 1] = sum(q(min(max(float(v), -CLIP), CLIP)) for v in np.asarray(dt, dtype=np.float32)[rows[mine]])
            if g not in live:
                continue
            best = min_d2(pts[rows[mine], :3], pts[rows[is_live & ~mine], :3])
            m[lo:hi][mine] = best
            with np.errstate(all="ignore"):
                d = np.sqrt(best.astype(np.float64))
            rec[k, g, 2] = sum(q(v if v < trunc else trunc) for v in d)
            rec[k, g, 3] = int((d <= near).sum())
            queries += len(best)
        info[k, 2:] = (sum(1 << g for g in live), queries)
        if motion is not None:
            mv = np.asarray(motion, dtype=np.float32)[rows[use]].astype(np.float64)
            mv = mv[np.isfinite(mv).all(axis=1)]
            s = np.sqrt((mv[:, 0] * mv[:, 0] + mv[:, 1] * mv[:, 1]) + mv[:, 2] * mv[:, 2])
            mot[k] = (len(mv), sum(q(min(v, CLIP)) for v in s))
    return info, rec, mot, m


def brute(pts, labels, group, C, dt=None, **params):
    """rules A-C again, written differently: a double loop over rows in Python floats rounded through float32 at every step ->
    (state [C], m per ORIGINAL row float32 [N], +inf where the row is no query)"""
    prm = dict(DEFAULTS, **params)
    f = np.float32
    N = len(pts)
    states, m = [], np.full(N, np.inf, np.float32)
    for k in range(1, C + 1):
        rows = [i for i in range(N) if labels[i] == k and all(math.isfinite(float(v)) for v in pts[i][:3]) and group[i] <= 7 and
                (dt is None or math.isfinite(float(dt[i])))]
        per = {}
        for i in rows:
            per.setdefault(int(group[i]), []).append(i)
        live = {g for g, r in per.items() if len(r) >= prm["min_group"]}
        if len(rows) < prm["min_points"]:
            states.append(TOO_FEW)
        elif len(rows) > prm["max_points"]:
            states.append(TOO_LARGE)
        elif len(live) < 2:
            states.append(ONE_SENSOR)
        else:
            states.append(SCORED)
            for i in rows:
                if int(group[i]) not in live:
                    continue
                best = f(np.inf)
                for j in rows:
                    if int(group[j]) in live and group[j] != group[i]:
                        with np.errstate(all="ignore"):
                            dx, dy, dz = f(pts[i][0]) - f(pts[j][0]), f(pts[i][1]) - f(pts[j][1]), f(pts[i][2]) - f(pts[j][2])
                            d2 = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
                        if d2 < best:
                            best = d2
                m[i] = best
    return np.asarray(states), m


def glue(info, rec, mot, sensor_dt=SENSOR_DT):
    """rule F, float64 on the integer tables: a dict of per-cluster arrays (nan where a value has no rows behind it)"""
    info, rec, mot = np.asarray(info), np.asarray(rec), np.asarray(mot)
    C = len(info)
    out = {"state": info[:, 0].copy(), "n": info[:, 1].copy(), "queries": info[:, 3].copy(), "X": np.full(C, np.nan), "near": np.full(C, np.nan),
           "t": np.full((C, GROUPS), np.nan), "dt_spread": np.full(C, np.nan), "speed": np.full(C, np.nan)}
    for k in range(C):
        for g in range(GROUPS):
            if rec[k, g, 0] > 0:
                out["t"][k, g] = float(int(rec[k, g, 1])) / (float(UNIT) * float(int(rec[k, g, 0])))
        if info[k, 0] != SCORED:
            continue
        nq = int(info[k, 3])
        out["X"][k] = float(int(rec[k, :, 2].sum())) / (float(UNIT) * nq)
        out["near"][k] = float(int(rec[k, :, 3].sum())) / nq
        t_live = [out["t"][k, g] for g in range(GROUPS) if info[k, 2] >> g & 1]
        out["dt_spread"][k] = max(t_live) - min(t_live)
        if mot[k, 0] > 0:
            out["speed"][k] = float(int(mot[k, 1])) / (float(UNIT) * float(int(mot[k, 0]))) / sensor_dt
    return out


# ---- the synthetic drive ---------------------------------------------------------------------------------------------------------
CAPTURE = (0.0, 0.033, 0.066)          # the three sensors' capture times inside the sweep [s]
SENSORS = (1, 2, 3)                    # their ids


def vehicle_surface(rng, n, length=4.5, width=1.9, height=1.5):
    """n points of the two visible sides and the roof of a box at the origin, heading +x: area-weighted draws, float64 [n, 3]"""
    areas = np.array([length * height, width * height, length * width])
    face = rng.choice(3, size=n, p=areas / areas.sum())
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    x = np.where(face == 1, length / 2, (u - 0.5) * length)
    y = np.where(face == 0, -width / 2, np.where(face == 1, (u - 0.5) * width, (v - 0.5) * width))
    z = np.where(face == 2, height, v * height)
    return np.stack([x, y, z], axis=1)


def drive(seed, speeds, points=600, noise=0.02, spacing=30.0):
    """One sweep of ``len(speeds)`` vehicles, vehicle k (label k + 1) of ``points`` rows moving at ``speeds[k]`` m/s along its
    heading, each sensor sampling a third of the rows at its own capture time.  A point captured ``dt0`` seconds after the sweep's
    reference time is RECORDED at ``p - v dt0``; compensation by the true flow puts it back at ``p``.  ``noise`` [m] is added to
    ``p`` before the displacement, so raw and compensated rows of a static vehicle are the same bytes.
    -> dict(raw, comp float32 [N, 3]; labels int32; group uint8; dt float32; motion float32 [N, 3] per sweep period)"""
    rng = np.random.default_rng(seed)
    raw, comp, labels, group, dts, motion = [], [], [], [], [], []
    for k, speed in enumerate(speeds):
        yaw = rng.uniform(0, 2 * math.pi)
        c, s = math.cos(yaw), math.sin(yaw)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        centre = np.array([spacing * (k % 6) - 60.0, spacing * (k // 6) - 60.0, 0.0])
        v = R @ np.array([speed, 0.0, 0.0])
        for g, t in zip(SENSORS, CAPTURE):
            n = points // len(SENSORS)
            p = vehicle_surface(rng, n) @ R.T + centre + rng.normal(0, noise, (n, 3)) * (noise > 0)
            p32 = p.astype(np.float32)
            shift = (v * t).astype(np.float32)
            r32 = p32 - shift
            raw.append(r32)
            comp.append(r32 + shift if speed else r32)
            labels.append(np.full(n, k + 1, np.int32))
            group.append(np.full(n, g, np.uint8))
            dts.append(np.full(n, t, np.float32))
            motion.append(np.tile((v * SENSOR_DT).astype(np.float32), (n, 1)))
    order = rng.permutation(sum(len(a) for a in raw))
    cat = lambda parts: np.concatenate(parts)[order]                  # noqa: E731
    return dict(raw=cat(raw), comp=cat(comp), labels=cat(labels), group=cat(group), dt=cat(dts), motion=cat(motion))
