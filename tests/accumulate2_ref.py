"""The checker of "sweep accumulation, v2": a numpy restatement of rules A2, I, H and E2 (the module docstring of
``himo_amd/accumulate.py`` is the text; parity with the reference is unpinned: it has no such program) on top of the v1 restatement
(``tests/accumulate_ref.py``: rules A-G and the float32 fused multiply-add).  Float32 operation by operation up to the quantisation,
Python integers in a dictionary by key after it, float64 operation by operation for what is emitted.  Nothing under ``himo_amd/``
imports it; it imports nothing from there either."""
import numpy as np

import accumulate_ref as v1

f32, f64 = np.float32, np.float64
LABEL_LIMIT = 1 << 24


def motion_min2(motion_min):
    """rule A2: (float)((double)motion_min * (double)motion_min)"""
    return f32(f64(motion_min) * f64(motion_min))


def advect(xyz, motion, lag, min2):
    """rule A2: (the rows moved where s >= min2, the rows whose motion is finite)"""
    p, m = np.asarray(xyz, f32).reshape(-1, 3), np.asarray(motion, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = (((m[:, 0] * m[:, 0]).astype(f32) + (m[:, 1] * m[:, 1]).astype(f32)).astype(f32) + (m[:, 2] * m[:, 2]).astype(f32)).astype(f32)
        moved = v1.fma32(np.full(m.shape, f32(lag), f32), m, p)
    finite = np.isfinite(m).all(axis=1)
    with np.errstate(all="ignore"):
        go = finite & (s >= f32(min2))
    return np.where(go[:, None], moved, p), finite


def flow_motion(pc0, flow, pose0, pose1):
    """rule I: m = flow - (E p - p), E = inv(pose1) @ pose0 in float64 rounded to float32"""
    p = np.asarray(pc0, f32)[:, :3]
    E = (np.linalg.inv(np.asarray(pose1, f64)) @ np.asarray(pose0, f64)).astype(f32)
    with np.errstate(all="ignore"):
        d = (v1.rigid_move(p, E) - p).astype(f32)
        return (np.asarray(flow, f32).reshape(-1, 3) - d).astype(f32)


def quantise_attr(v, scale):
    """rule H: the attribute in 0..255"""
    with np.errstate(all="ignore"):
        g = (np.asarray(v, f32) * f32(scale)).astype(f32)
        q = np.floor((g + f32(0.5)).astype(f32))
        q = np.where(g >= f32(255.0), 255.0, q)
        q = np.where(g > 0, q, 0.0)                                # NaN, negatives and zero
    return q.astype(np.int64)


def tag_of(label, lag):
    """rule H: ((255 - lag) << 24) | lab"""
    lab = np.asarray(label, np.int64)
    lab = np.where((lab > 0) & (lab < LABEL_LIMIT), lab, 0)
    return ((255 - int(lag)) << 24) | lab


def insert(table, rows, T, lag, skip=None, motion=None, motion_min=0.0, attr=None, attr_scale=1.0, label=None, **kw):
    """rules A, A2, B, C, D and H: add one source sweep to ``table``, a dict key -> [count, Sx, Sy, Sz, lag, Sa, tag].  A call
    without ``attr`` (``label``) leaves Sa (the tag) alone."""
    p = v1.params(**kw)
    assert 0 <= int(lag) <= 255
    rows = np.asarray(rows, f32)
    rows = rows.reshape(-1, rows.shape[-1] if rows.ndim == 2 else 3)
    n = len(rows)
    if n == 0:
        return 0
    part = v1.takes_part(rows, skip, **kw)                          # on the rows as given
    xyz = rows[:, :3]
    if motion is not None:
        xyz, finite = advect(xyz, motion, lag, motion_min2(motion_min))
        part = part & finite
    u, usable = v1.quantise(v1.rigid_move(xyz, T), **kw)
    v, off = u >> 8, u & 255
    dims = np.array([p["nx"], p["ny"], p["nz"]], np.int64)
    keep = part & usable & ((v >= 0) & (v < dims)).all(axis=1)
    qa = quantise_attr(np.asarray(attr, f32).reshape(-1), attr_scale) if attr is not None else np.zeros(n, np.int64)
    tags = tag_of(np.asarray(label).reshape(-1), lag) if label is not None else np.zeros(n, np.int64)
    for (ix, iy, iz), (ox, oy, oz), a, t in zip(v[keep].tolist(), off[keep].tolist(), qa[keep].tolist(), tags[keep].tolist()):
        key = (iz << 24) | (iy << 12) | ix
        e = table.setdefault(key, [0, 0, 0, 0, 255, 0, 0])
        e[0] += 1
        e[1] += ox
        e[2] += oy
        e[3] += oz
        e[4] = min(e[4], int(lag))
        e[5] += a
        e[6] = max(e[6], t)
    return int(keep.sum())


def emit(table, attr_scale=1.0, **kw):
    """rules E and E2: (keys, xyz, lag, count, intensity float32 [M], label int32 [M]) in ascending key order"""
    keys = np.array(sorted(table), np.int64)
    e = np.array([table[k] for k in keys.tolist()], np.int64).reshape(-1, 7)
    _, xyz, lag, count = v1.emit({k: table[k][:5] for k in keys.tolist()}, **kw)
    with np.errstate(all="ignore"):
        intensity = ((e[:, 5].astype(f64) / e[:, 0].astype(f64)) / f64(f32(attr_scale))).astype(f32)
    return keys, xyz, lag, count, intensity, (e[:, 6] & 0xFFFFFF).astype(np.int32)


def accumulate(calls, attr_scale=1.0, **kw):
    """``calls``: dicts of ``insert``'s arguments (rows, T, lag and any of skip, motion, motion_min, attr, attr_scale, label) inserted
    into one fresh table -> ``emit`` at ``attr_scale``"""
    table = {}
    for c in calls:
        insert(table, **c, **kw)
    return emit(table, attr_scale, **kw)


def accumulate_target(sweeps, poses, t, window=10, skips=None, motions=None, intensities=None, labels=None, motion_min=0.0, intensity_scale=1.0,
                      **kw):
    """rule G with v2's per-sweep extras"""
    pick = lambda seq, k: None if seq is None else seq[k]         # noqa: E731
    calls = [dict(rows=sweeps[k], T=v1.relative_pose(poses[t], poses[k]), lag=t - k, skip=pick(skips, k), motion=pick(motions, k),
                  motion_min=motion_min, attr=pick(intensities, k), attr_scale=intensity_scale, label=pick(labels, k))
             for k in v1.sources(t, len(sweeps), window)]
    return accumulate(calls, intensity_scale, **kw)
