"""Checker: a float64 numpy restatement of ``mmcv.ops.points_in_boxes_part`` on double tensors, the one device call
``dataprocess/extract_sca.py`` makes (:117), and of the labelling around it (:95-145).  Never on the product path.

The membership rule is a restatement from mmcv's documented behaviour (mmcv itself is not available to this project):
a box is ``(cx, cy, cz_bottom, dx, dy, dz, rz)``, its centre ``cz_bottom + dz / 2.0``; a point is outside if
``fabs(z - cz_centre) > dz / 2.0``; otherwise ``local_x = sx * cosa + sy * (-sina)``, ``local_y = sx * sina + sy * cosa`` with
``cosa = cos(-rz)``, ``sina = sin(-rz)``, and the point is inside iff ``-dx/2 < local_x < dx/2`` and ``-dy/2 < local_y < dy/2``
(all four strict).  The first box in list order that contains the point wins; a point in no box gets -1.  Every operation
rounds on its own (numpy does not contract), which is what the device kernel is built to reproduce.
"""
from __future__ import annotations

import numpy as np

RECORDED: list = []          # (points float64 [N,3], boxes float64 [M,7]) of every ``points_in_boxes_part`` call, in order


def box_constants(boxes: np.ndarray) -> np.ndarray:
    """float64 [M,8]: cx, cy, cz_centre, dx/2, dy/2, dz/2, cos(-rz), sin(-rz) of ``boxes`` float64 [M,7]"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    out = np.empty((len(b), 8), dtype=np.float64)
    out[:, 0], out[:, 1] = b[:, 0], b[:, 1]
    out[:, 5] = b[:, 5] / 2.0
    out[:, 2] = b[:, 2] + out[:, 5]
    out[:, 3], out[:, 4] = b[:, 3] / 2.0, b[:, 4] / 2.0
    out[:, 6], out[:, 7] = np.cos(-b[:, 6]), np.sin(-b[:, 6])
    return out


def points_in_boxes(points: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """int32 [N]: index of the first box of ``boxes`` [M,7] that contains each of ``points`` [N,3], -1 for none"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    g = box_constants(boxes)
    hit = np.full(len(p), -1, dtype=np.int32)
    for m in range(len(g) - 1, -1, -1):                       # last to first: an earlier box overwrites a later one
        cx, cy, czc, hx, hy, hz, cosa, sina = g[m]
        zin = ~(np.fabs(p[:, 2] - czc) > hz)
        sx, sy = p[:, 0] - cx, p[:, 1] - cy
        lx = sx * cosa + sy * (-sina)
        ly = sx * sina + sy * cosa
        inside = zin & (lx > -hx) & (lx < hx) & (ly > -hy) & (ly < hy)
        hit[inside] = m
    return hit


def face_distance(points: np.ndarray, boxes: np.ndarray) -> float:
    """the smallest distance of a point to the top / bottom face plane of a box whose footprint contains it (inf when no
    footprint contains a point): the golden inputs keep it above 1e-4 m, where a float32 ``fabsf`` on the z distance
    (what mmcv's kernel may apply) cannot change a decision"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    g = box_constants(boxes)
    best = np.inf
    for cx, cy, czc, hx, hy, hz, cosa, sina in g:
        sx, sy = p[:, 0] - cx, p[:, 1] - cy
        lx = sx * cosa + sy * (-sina)
        ly = sx * sina + sy * cosa
        foot = (lx > -hx) & (lx < hx) & (ly > -hy) & (ly < hy)
        if foot.any():
            best = min(best, float(np.abs(np.fabs(p[foot, 2] - czc) - hz).min()))
    return best


def points_in_boxes_part(points, boxes):
    """the stub installed as ``mmcv.ops.points_in_boxes_part``: torch double tensors [1,N,3] and [1,M,7] -> int32 [1,N];
    records what it was handed"""
    import torch
    p = points.detach().cpu().numpy()[0]
    b = boxes.detach().cpu().numpy()[0]
    assert p.dtype == np.float64 and b.dtype == np.float64
    RECORDED.append((p.copy(), b.copy()))
    return torch.from_numpy(points_in_boxes(p, b))[None]


def label_sweep(pc, ego, geom, obj_flow, box_class, vel_finite, background):
    """the per-point outputs of extract_sca.py:95-145 from the prepared box rows (``geom`` [M,8] as ``box_constants`` gives):
    (flow f32 [N,3], valid u8 [N], category u8 [N], instance u32 [N])"""
    pc = np.asarray(pc, dtype=np.float32)
    n = len(pc)
    ego = np.asarray(ego, dtype=np.float64)
    flow = pc[:, :3] @ ego[:3, :3].T + ego[:3, -1] - pc[:, :3]                       # :97
    p = pc[:, :3].astype(np.float64)
    hit = np.full(n, -1, dtype=np.int32)
    for m in range(len(geom) - 1, -1, -1):
        cx, cy, czc, hx, hy, hz, cosa, sina = geom[m]
        zin = ~(np.fabs(p[:, 2] - czc) > hz)
        sx, sy = p[:, 0] - cx, p[:, 1] - cy
        lx = sx * cosa + sy * (-sina)
        ly = sx * sina + sy * cosa
        hit[zin & (lx > -hx) & (lx < hx) & (ly > -hy) & (ly < hy)] = m
    inbox = hit >= 0
    flow[inbox] += np.asarray(obj_flow, dtype=np.float32).reshape(-1, 3)[hit[inbox]]   # :134
    valid = np.ones(n, dtype=np.uint8)
    valid[inbox] = np.asarray(vel_finite, dtype=np.uint8)[hit[inbox]]
    cat = np.full(n, background, dtype=np.uint8)
    cat[inbox] = np.asarray(box_class, dtype=np.uint8)[hit[inbox]]
    return flow.astype(np.float32), valid, cat, (hit + 1).astype(np.uint32)
