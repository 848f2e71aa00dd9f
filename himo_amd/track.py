"""Box tracking: the identity of a box over the sweeps of a scene (``python -m himo_amd.track --data_dir D --res_names raw,seflowpp_best
[--gt flow]`` reads ``<timestamp>/boxes_<name>`` and ``pose0`` of every sweep, scene by scene, writes ``<timestamp>/tracks_<name>`` and
prints one table per result name).  ``box_fit`` gives every cluster one box with a velocity and ``eval_box`` scores the boxes of one
sweep; neither can say that the car of sweep t is the car of sweep t + 1.  That identity is what motion compensation is for: objects of
the right shape at the right place hold together over time -- fewer broken tracks, fewer identity switches, steadier velocities, raw
against compensated.

PARITY UNPINNED.  The reference has no such stage.  Like ``box_fit`` and ``eval_box`` it follows the build's own written rule, below,
and is checked bit for bit against a pure-Python restatement of it (``tests/boxtrack_ref.py``), never against the reference.  No claim
is made about the reference's numbers.  Timing: 113 ms per call of 256 synthetic scenes of 150 sweeps of 300 boxes (2.9 us a sweep, beside
1.06 ms for making ONE sweep's boxes), but 100 ms for one such scene tracked alone (670 us a sweep; 172 us at 50 boxes): one workgroup
per scene is the limit there (profiles/box_track.txt); nothing has been tried on field data.

The rule -- "box tracking, v1" (normative)
==========================================
A scene is a run of sweeps k = 0..K-1 in index order.  Sweep k has ``F_k`` box rows (``box_fit``'s float32 ``[12]`` layout).

A. Host preparation (Python, float64; ``math.cos`` / ``math.sin`` are used here only, the library calls no transcendental).  Every box
   row is widened to float64 and moved into the scene frame W, the sensor frame of the scene's first sweep: ``T_k = inv(pose0_first) @
   pose0_k`` (numpy, float64).  The position is transformed by ``T_k``: ``x' = ((T00*x + T01*y) + T02*z) + T03``, y' and z' likewise with
   rows 1 and 2.  The heading is the unit vector ``(c, s) = (cos yaw, sin yaw)`` rotated by the upper-left 2x2 of ``T_k``: ``c' = T00*c +
   T01*s``, ``s' = T10*c + T11*s`` (not normalised again); the velocity ``(vx, vy)`` is rotated by the same 2x2.  The detection row is
   float64 ``[12]`` = x, y, z, l, w, h, c, s, vx, vy, 0, 0.  A row with any non-finite value (among the nine it reads or the twelve it
   makes), or with ``l < 0``, ``w < 0`` or ``h < 0``, is INVALID and is written as twelve NaN.  The library takes a row as INVALID iff
   one of its twelve values is not finite or an extent is negative.  An INVALID row is never matched, never starts a track and gets id
   -1.  ``dt_k`` (float64, one per sweep) is the time from sweep k-1 to sweep k; ``dt_0`` is not read.  The program fills every ``dt_k``
   with ``sensor_dt`` (default ``box_fit.SENSOR_DT``): it parses no timestamp, as no other stage here does.  Every ``dt_k`` with k > 0
   must be finite and > 0.
B. Track state (float64): x, y, z, l, w, h, c, s, vx, vy; integers id, hits, misses.  The live tracks of a scene form a table in
   ascending id.
C. One step, for sweep k.  Only ``+ - * /`` and comparisons appear; every operation rounds on its own (``himo_amd/csrc/boxtrack.hip``
   is built with ``-ffp-contract=off``).
   C1. Predict (k > 0).  For every live track ``px = x + vx*dt_k``, ``py = y + vy*dt_k``; everything else is unchanged.  For k = 0 the
       table is empty.
   C2. Rect.  The rect of a track at ``(px, py)`` and the rect of a detection are both made by ONE device function from ``(x, y, z, l,
       w, h, c, s)``: the arithmetic is exactly that of rule A of box evaluation v1 (``eval_box``) with ``c, s`` given -- the corner
       order, ``zlo``, ``zhi`` and ``area = l*w``.  (A rect that comes out with a value that is not finite overlaps nothing.)
   C3. IoU.  The BEV IoU of (track i, detection j) is rules B and C of box evaluation v1, the track the subject A and the detection the
       clip polygon B.
   C4. Match.  Rule D of box evaluation v1 with ``min_iou``: greedy by descending IoU, then lower track slot i, then lower detection j.
   C5. Matched track (i <-> j).  With ``rx = dx - px``, ``ry = dy - py``: ``x = px + alpha*rx``, y likewise; z, l, w, h, c, s are
       replaced by the detection's; the velocity, in ``vel_mode`` 0 ("box"): ``vx = vx + beta*(dvx - vx)``, vy likewise; in ``vel_mode``
       1 ("track"): ``vx = vx + beta*(rx / dt_k)``, vy likewise; ``hits += 1``, ``misses = 0``.
   C6. Unmatched track.  ``x = px``, ``y = py``, ``misses += 1``; the track dies iff ``misses > max_age``.
   C7. Unmatched valid detection.  It starts a track: the state is the detection's, the velocity the detection's in mode 0 and zero in
       mode 1, ``hits = 1``, ``misses = 0``.  New tracks are made in ascending j; each takes the scene's next id (ids start at 0 per
       scene and are never reused).  When the table would exceed ``max_tracks`` the detection gets id -1 and the scene's ``overflow``
       count goes up by one.
   C8. The new table: the surviving tracks in their order, then the new ones.
D. Outputs.  Per detection row: ``track_id`` int32 (the id, or -1); ``age`` int32 (the track's ``hits`` after this step, 0 for -1);
   ``state`` float64 ``[4]`` = x, y, vx, vy after C5 or C7, in W (zeros for -1); ``iou`` float64, the matched pair's BEV IoU (0 for new
   tracks and for -1).  Per sweep: ``live`` int32, the table's length after C8.  Per scene: ``n_ids`` int32 and ``overflow`` int32.
E. Parameters (``TrackParams``, mirrored as ``himo_boxtrack_params``, 40 bytes) and limits: ``min_iou`` 0.1 (as in ``eval_box``: finite,
   ``0 < min_iou <= 1``); ``alpha`` 0.5 and ``beta`` 0.5 (finite, in [0, 1]); ``max_age`` 2 (0..255); ``max_tracks`` 512
   (1..``HIMO_BOXTRACK_MAX`` = 512); ``vel_mode`` 0 (0 or 1).  At most ``HIMO_BOXTRACK_MAX`` detections per sweep; any number of sweeps
   per scene and of scenes per call.  Everything else is refused before a launch, with no write.
F. Host glue (Python, float64, on box rows only).  The state is rotated back into each sweep's sensor frame for storage: with ``U =
   inv(T_k)`` (numpy), ``x_s = ((U00*x + U01*y) + U02*z) + U03``, y_s likewise -- z the detection's z in W, which is the track's after the
   step -- and ``(vx, vy)`` by the upper-left 2x2 of U.  ``tracks_<name>`` is float64 ``[F][6]`` = id, age, x, y, vx, vy; a row with id -1
   holds -1 and five zeros.  The tables, per result name over all scenes: ids issued; CONFIRMED tracks (``hits >= min_hits`` at some
   point, default 3); the mean and median length of a confirmed track in sweeps (the sweeps in which a box carried its id: its last
   ``age``); the share of boxes that belong to a confirmed track; the overflow count; the velocity jitter: the mean ``hypot`` of (box
   velocity - track velocity), both in the sensor frame, over boxes with ``age >= min_hits``.
   With ``--gt NAME`` each sweep's ``boxes_<NAME>`` are paired with the name's boxes by ``BoxEvaluator.match`` (box evaluation v1); a
   ground-truth box is MATCHED iff its pair has BEV IoU >= 0.5 and the predicted box carries a track id >= 0.  The ground-truth identity
   is the label id (column 10) of the ground-truth box.  THIS ASSUMES THAT THE LABEL (``flow_instance_id``) IS STABLE OVER A SCENE;
   nothing in the repository states that it is.  Reported: TP (matched ground-truth boxes), FN (the others), FP (predicted boxes less
   TP); identity switches (IDSW): a ground-truth identity whose matched track id differs from the id at its previous matched sweep;
   fragmentations: a ground-truth identity matched, then -- in a later sweep that holds a box of it -- unmatched, then matched again,
   counted at the sweep that matches again; MOTA = 1 - (FN + FP + IDSW) / GT, None when GT is 0.  All of them for all ground-truth
   boxes and per speed bucket of ``eval_box`` (the bucket of the ground-truth box at the sweep that counts); a predicted box without a
   partner has no ground-truth box and so no bucket: FP is counted in "all" only and a bucket's MOTA leaves it out.  Integer tallies on
   the host.

Not part of v1: association by distance when boxes do not overlap, a Kalman covariance, output for coasting tracks, re-identification
after death, smoothing of size or heading.

Python sequences the one launch of a call and owns no arithmetic on pairs of boxes.  ``BoxTracker.track`` uploads the detection tables
and returns without a host wait; the result's host copies are made when asked for.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .box_fit import MOTION_MIN, SENSOR_DT, boxes_key
from .eval_box import MIN_IOU, SPEED_BUCKETS, check_min_iou, speed_bucket
from .stored import fmt, ratio

MAX_BOXES = 512                     # HIMO_BOXTRACK_MAX
MIN_HITS = 3
MOT_IOU = 0.5
VEL_MODES = ("box", "track")


class _CParams(ctypes.Structure):
    """mirror of ``himo_boxtrack_params`` (include/himo_amd.h)"""
    _fields_ = [("min_iou", ctypes.c_double), ("alpha", ctypes.c_double), ("beta", ctypes.c_double), ("max_age", ctypes.c_int32),
                ("max_tracks", ctypes.c_int32), ("vel_mode", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@dataclass(frozen=True)
class TrackParams:
    """the parameters of "box tracking, v1"; refuses what the rule does not admit before anything is launched"""
    min_iou: float = MIN_IOU
    alpha: float = 0.5
    beta: float = 0.5
    max_age: int = 2
    max_tracks: int = MAX_BOXES
    vel_mode: int = 0

    def __post_init__(self):
        check_min_iou(self.min_iou)
        for name in ("alpha", "beta"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not 0 <= v <= 1:
                raise ValueError(f"TrackParams.{name}={v!r}: finite, 0 <= {name} <= 1")
        for name, lo, hi in (("max_age", 0, 255), ("max_tracks", 1, MAX_BOXES), ("vel_mode", 0, 1)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"TrackParams.{name}={v!r}: an integer, {lo}..{hi}")

    def c_struct(self) -> _CParams:
        return _CParams(float(self.min_iou), float(self.alpha), float(self.beta), int(self.max_age), int(self.max_tracks), int(self.vel_mode), 0)


def check_sensor_dt(v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
        raise ValueError(f"sensor_dt={v!r}: finite and > 0")
    return float(v)


# ---- rule A: the host preparation -------------------------------------------------------------------------------------------------------
def scene_transform(pose0, pose0_first) -> np.ndarray:
    """``T_k = inv(pose0_first) @ pose0_k``, float64 [4, 4]"""
    a, b = np.asarray(pose0_first, dtype=np.float64), np.asarray(pose0, dtype=np.float64)
    if a.shape != (4, 4) or b.shape != (4, 4):
        raise ValueError(f"poses are [4, 4], not {b.shape} and {a.shape}")
    return np.linalg.inv(a) @ b


def detections(rows, pose0, pose0_first) -> np.ndarray:
    """Rule A: box rows ``[F, >= 9]`` (x, y, z, l, w, h, yaw, vx, vy[, ...]) of a sweep with pose ``pose0`` -> detection rows float64
    ``[F, 12]`` in the frame of the scene's first sweep (an INVALID row: twelve NaN)."""
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] < 9:
        raise ValueError(f"box rows are x, y, z, l, w, h, yaw, vx, vy[, ...], not {r.shape}")
    T = scene_transform(pose0, pose0_first)
    x, y, z, l, w, h, yaw, vx, vy = np.ascontiguousarray(r[:, :9].T, dtype=np.float64)
    turn = np.isfinite(yaw)
    angle = np.where(turn, yaw, 0.0).tolist()                       # (math.cos refuses an infinity; such a row is INVALID below)
    c = np.fromiter(map(math.cos, angle), dtype=np.float64, count=len(angle))
    s = np.fromiter(map(math.sin, angle), dtype=np.float64, count=len(angle))
    with np.errstate(all="ignore"):
        cols = np.zeros((12, len(x)), dtype=np.float64)
        for k in range(3):
            cols[k] = ((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]
        cols[3], cols[4], cols[5] = l, w, h
        cols[6] = T[0, 0] * c + T[0, 1] * s
        cols[7] = T[1, 0] * c + T[1, 1] * s
        cols[8] = T[0, 0] * vx + T[0, 1] * vy
        cols[9] = T[1, 0] * vx + T[1, 1] * vy
        bad = ~np.isfinite(cols).all(axis=0) | ~turn | ~np.isfinite(vx) | ~np.isfinite(vy) | (l < 0) | (w < 0) | (h < 0)
    out = np.ascontiguousarray(cols.T)
    out[bad] = np.nan
    return out


def stored_rows(track_id, age, state, det, pose0, pose0_first) -> np.ndarray:
    """Rule F: one sweep's ``tracks_<name>`` float64 [F, 6] = id, age, x, y, vx, vy, the state rotated back into the sweep's sensor frame"""
    U = np.linalg.inv(scene_transform(pose0, pose0_first))
    track_id, age = np.asarray(track_id), np.asarray(age)
    state, det = np.asarray(state, dtype=np.float64).reshape(-1, 4), np.asarray(det, dtype=np.float64).reshape(-1, 12)
    out = np.zeros((len(track_id), 6))
    x, y, vx, vy, z = state[:, 0], state[:, 1], state[:, 2], state[:, 3], det[:, 2]
    with np.errstate(all="ignore"):
        out[:, 0], out[:, 1] = track_id, age
        out[:, 2] = ((U[0, 0] * x + U[0, 1] * y) + U[0, 2] * z) + U[0, 3]
        out[:, 3] = ((U[1, 0] * x + U[1, 1] * y) + U[1, 2] * z) + U[1, 3]
        out[:, 4] = U[0, 0] * vx + U[0, 1] * vy
        out[:, 5] = U[1, 0] * vx + U[1, 1] * vy
    out[track_id < 0, 1:] = 0.0
    return out


# ---- rules B-E: the binding -------------------------------------------------------------------------------------------------------------
class TrackResult:
    """What ``BoxTracker.track`` returns, over the scenes of the call in packed order (``sweep_off`` int64 [n + 1]: the scenes' sweep
    ranges; ``det_off`` int64 [sweeps + 1]: the sweeps' row ranges): ``track_id`` int32 [rows], ``age`` int32 [rows], ``state`` float64
    [rows, 4], ``iou`` float64 [rows], ``live`` int32 [sweeps], ``scene_info`` int32 [n, 2] (ids issued, overflow).  Host copies, made when
    first asked for (that is a wait); ``device`` holds the six device tensors in that order.  ``sweep(n, k)`` gives sweep k of scene n:
    (track_id, age, state, iou)."""

    def __init__(self, tensors, sweep_off, det_off):
        self.device, self.sweep_off, self.det_off = tuple(tensors), sweep_off, det_off
        self._host = None

    def _copies(self):
        if self._host is None:
            self._host = tuple(t.cpu().numpy() for t in self.device)
        return self._host

    track_id = property(lambda self: self._copies()[0])
    age = property(lambda self: self._copies()[1])
    state = property(lambda self: self._copies()[2])
    iou = property(lambda self: self._copies()[3])
    live = property(lambda self: self._copies()[4])
    scene_info = property(lambda self: self._copies()[5])

    def __len__(self):
        return len(self.sweep_off) - 1

    def sweeps(self, n: int) -> int:
        return int(self.sweep_off[n + 1] - self.sweep_off[n])

    def sweep(self, n: int, k: int):
        q = int(self.sweep_off[n]) + k
        lo, hi = int(self.det_off[q]), int(self.det_off[q + 1])
        return self.track_id[lo:hi], self.age[lo:hi], self.state[lo:hi], self.iou[lo:hi]


class BoxTracker:
    """``BoxTracker(device, sensor_dt, **params).track(scenes)`` -> a ``TrackResult`` (rules B-E; a batch of scenes in one launch).  A
    scene is a list of detection tables, float64 ``[F_k, 12]`` each, one per sweep in order (``detections`` makes one from box rows and
    poses: rule A).  ``dts``: per scene, the time step of every sweep (default: ``sensor_dt`` everywhere).  There is no CPU path."""

    def __init__(self, device=None, sensor_dt: float = SENSOR_DT, **params):
        from . import _lib
        self.params = TrackParams(**params)
        self.sensor_dt = check_sensor_dt(sensor_dt)
        self.lib = _lib.load()
        if self.lib.himo_abi_sizeof(b"himo_boxtrack_params") != ctypes.sizeof(_CParams):
            raise ImportError("himo_boxtrack_params: the library's layout is not this binding's; rebuild libhimo_amd.so")
        self.device = device if device is not None else _lib.require_gpu()

    def tables(self, scenes, dts=None):
        """the host tables of a call, checked: (det float64 [rows, 12], sweep_off, det_off, dt float64 [sweeps])"""
        scenes = [[np.asarray(d, dtype=np.float64) for d in sc] for sc in scenes]
        counts = []
        for n, sc in enumerate(scenes):
            for k, d in enumerate(sc):
                if d.ndim != 2 or d.shape[1] != 12:
                    raise ValueError(f"scene {n}, sweep {k}: detection rows are float64 [F, 12] (x, y, z, l, w, h, c, s, vx, vy, 0, 0), not {d.shape}")
                if len(d) > MAX_BOXES:
                    raise ValueError(f"scene {n}, sweep {k} holds {len(d)} boxes: at most {MAX_BOXES} per sweep")
                counts.append(len(d))
        sweep_off = np.zeros(len(scenes) + 1, dtype=np.int64)
        np.cumsum([len(sc) for sc in scenes], out=sweep_off[1:])
        det_off = np.zeros(len(counts) + 1, dtype=np.int64)
        np.cumsum(counts, out=det_off[1:])
        if dts is None:
            dt = np.full(len(counts), self.sensor_dt, dtype=np.float64)
        else:
            dts = [np.asarray(v, dtype=np.float64).reshape(-1) for v in dts]
            if len(dts) != len(scenes) or any(len(v) != len(sc) for v, sc in zip(dts, scenes)):
                raise ValueError("dts: one time step per sweep of every scene")
            for n, v in enumerate(dts):
                if len(v) > 1 and not (np.isfinite(v[1:]).all() and (v[1:] > 0).all()):
                    raise ValueError(f"scene {n}: every dt_k with k > 0 is finite and > 0")
            dt = np.concatenate(dts) if dts else np.zeros(0)
        parts = [d for sc in scenes for d in sc if len(d)]
        det = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 12))
        return det, sweep_off, det_off, np.ascontiguousarray(dt, dtype=np.float64)

    def track(self, scenes, dts=None) -> TrackResult:
        import torch
        from . import _lib
        P, dev = _lib.ptr, self.device
        det, sweep_off, det_off, dt = self.tables(list(scenes), dts)
        n, sweeps, rows = len(sweep_off) - 1, len(det_off) - 1, len(det)
        up = lambda a: torch.from_numpy(a).to(dev)                  # noqa: E731
        d_det, d_so, d_do, d_dt = up(det), up(sweep_off), up(det_off), up(dt)
        out = (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
               torch.empty((rows, 4), dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.float64, device=dev),
               torch.empty(sweeps, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev))
        if n:
            prm = self.params.c_struct()
            need = int(self.lib.himo_boxtrack_workspace_bytes(n, sweep_off.ctypes.data, det_off.ctypes.data, ctypes.addressof(prm)))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                st = self.lib.himo_boxtrack(n, P(d_det), sweep_off.ctypes.data, P(d_so), det_off.ctypes.data, P(d_do), dt.ctypes.data, P(d_dt),
                                            ctypes.addressof(prm), P(out[0]), P(out[1]), P(out[2]), P(out[3]), P(out[4]), P(out[5]), P(ws),
                                            ws.numel(), _lib.stream_handle())
            _lib.check(st, "himo_boxtrack")
        return TrackResult(out, sweep_off, det_off)


# ---- rule F: the tables -----------------------------------------------------------------------------------------------------------------
def mot_keys() -> list:
    return ["all"] + [f"speed {b}" for b in SPEED_BUCKETS]


def new_sums() -> dict:
    """the running sums of one result name: integers, floats and lists only, so that ranks' sums add up"""
    return {"ids": 0, "overflow": 0, "boxes": 0, "confirmed_boxes": 0, "lengths": [], "jitter_sum": 0.0, "jitter_n": 0, "pred": 0,
            "mot": {k: {"gt": 0, "tp": 0, "fn": 0, "idsw": 0, "frag": 0} for k in mot_keys()}}


def tally_scene(sums: dict, boxes, tracks, n_ids: int, overflow: int, min_hits: int = MIN_HITS) -> None:
    """add one scene: ``boxes`` = the box rows of every sweep, ``tracks`` = their stored ``tracks_<name>`` rows (rule F)"""
    sums["ids"] += int(n_ids)
    sums["overflow"] += int(overflow)
    last = {}                                                       # id -> its greatest age
    for tr in tracks:
        for i, a in zip(tr[:, 0].astype(np.int64), tr[:, 1].astype(np.int64)):
            if i >= 0:
                last[int(i)] = max(last.get(int(i), 0), int(a))
    confirmed = {i for i, a in last.items() if a >= min_hits}
    sums["lengths"] += [last[i] for i in sorted(confirmed)]
    for b, tr in zip(boxes, tracks):
        b = np.asarray(b, dtype=np.float64)
        sums["boxes"] += len(b)
        sums["confirmed_boxes"] += sum(1 for i in tr[:, 0].astype(np.int64) if int(i) in confirmed)
        for j in np.flatnonzero(tr[:, 1] >= min_hits):              # (in row order: the sums are the restatement's)
            sums["jitter_sum"] += math.hypot(b[j, 7] - tr[j, 4], b[j, 8] - tr[j, 5])
            sums["jitter_n"] += 1


def tally_mot(sums: dict, sweeps, motion_min: float = MOTION_MIN, sensor_dt: float = SENSOR_DT) -> None:
    """add one scene's ground-truth comparison: ``sweeps`` = [(rows_gt, track ids of the predicted boxes, match_gt, iou_gt)] in sweep
    order, ``match_gt`` int [Fa] (the predicted row or -1) and ``iou_gt`` float [Fa] or [Fa, 2] rule D's of box evaluation v1"""
    prev, broken = {}, set()                                        # identity -> the track id at its last matched sweep; identities lost since
    for rows_gt, pred_ids, match_gt, iou_gt in sweeps:
        rows_gt, pred_ids, match_gt = np.asarray(rows_gt, dtype=np.float64).reshape(-1, 12), np.asarray(pred_ids).astype(np.int64), np.asarray(match_gt)
        iou = np.asarray(iou_gt, dtype=np.float64).reshape(len(rows_gt), -1)[:, 0] if len(rows_gt) else np.zeros(0)
        sums["pred"] += int(len(pred_ids))
        for i, g in enumerate(rows_gt):
            keys = ("all", "speed " + speed_bucket(math.hypot(g[7], g[8]), motion_min, sensor_dt))
            j = int(match_gt[i])
            tid = int(pred_ids[j]) if j >= 0 and iou[i] >= MOT_IOU else -1
            ident = int(g[10])
            for k in keys:
                sums["mot"][k]["gt"] += 1
                sums["mot"][k]["tp" if tid >= 0 else "fn"] += 1
            if tid < 0:
                if ident in prev:
                    broken.add(ident)
                continue
            if ident in prev and prev[ident] != tid:
                for k in keys:
                    sums["mot"][k]["idsw"] += 1
            if ident in broken:
                broken.discard(ident)
                for k in keys:
                    sums["mot"][k]["frag"] += 1
            prev[ident] = tid


def add_sums(a: dict, b: dict) -> dict:
    """two ranks' {name: sums} added up: ``distenv.add_sums``, except that ``lengths`` -- one entry per confirmed track -- is joined"""
    from .distenv import add_sums as add
    less = lambda sums: {s: {k: v for k, v in t.items() if k != "lengths"} for s, t in sums.items()}     # noqa: E731
    return {s: dict(t, lengths=a[s]["lengths"] + b[s]["lengths"]) for s, t in add(less(a), less(b)).items()}


def summary(sums: dict, with_gt: bool) -> dict:
    """the numbers of the tables and of ``--json``: {name: {...}}"""
    out = {}
    for name, t in sums.items():
        lengths = sorted(t["lengths"])
        r = {"ids": t["ids"], "confirmed": len(lengths), "mean_length": ratio(sum(lengths), len(lengths)),
             "median_length": float(np.median(lengths)) if lengths else None, "boxes": t["boxes"],
             "confirmed_share": ratio(t["confirmed_boxes"], t["boxes"]), "overflow": t["overflow"], "velocity_jitter": ratio(t["jitter_sum"], t["jitter_n"])}
        if with_gt:
            r["mot"] = {}
            for key, b in t["mot"].items():
                m = {"gt": b["gt"], "tp": b["tp"], "fn": b["fn"], "idsw": b["idsw"], "frag": b["frag"]}
                fp = 0
                if key == "all":
                    fp = m["fp"] = t["pred"] - b["tp"]
                m["mota"] = None if not b["gt"] else 1.0 - (b["fn"] + fp + b["idsw"]) / b["gt"]
                r["mot"][key] = m
        out[name] = r
    return out


def _table(name: str, r: dict, gt: str | None) -> str:
    lines = [f"{name}: {r['ids']} ids, {r['confirmed']} confirmed tracks, length mean {fmt(r['mean_length'], '.2f')} median {fmt(r['median_length'], '.1f')} "
             f"sweeps, {fmt(r['confirmed_share'])} of {r['boxes']} boxes on a confirmed track, overflow {r['overflow']}, velocity jitter "
             f"{fmt(r['velocity_jitter'])} m/s"]
    for key, m in r.get("mot", {}).items():
        line = f"  against {gt} {key:<12} gt {m['gt']:>6} TP {m['tp']} FN {m['fn']}"
        if "fp" in m:
            line += f" FP {m['fp']}"
        lines.append(line + f" IDSW {m['idsw']} frag {m['frag']} MOTA {fmt(m['mota'])}")
    return "\n".join(lines)


def point_labels(point_label, box_rows, track_id) -> np.ndarray:
    """``--point_label_key``: for every point the track id of the box whose label id (column 10) equals the point's label, -1 where
    there is none: int32 [N]"""
    lab = np.asarray(point_label).astype(np.int64)
    out = np.full(len(lab), -1, dtype=np.int32)
    ids = np.asarray(box_rows)[:, 10].astype(np.int64) if len(box_rows) else np.zeros(0, np.int64)
    if len(ids):
        order = np.argsort(ids, kind="stable")
        pos = np.clip(np.searchsorted(ids[order], lab), 0, len(ids) - 1)
        hit = ids[order][pos] == lab
        out[hit] = np.asarray(track_id).astype(np.int32)[order][pos[hit]]
    return out


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def tracks_key(name: str) -> str:
    return f"tracks_{name}"


def track_label_key(name: str) -> str:
    return f"track_label_{name}"


def main(data_dir: str, res_names, gt: str | None = None, json_path: str | None = None, overwrite: bool = False, batch: int = 16,
         min_hits: int = MIN_HITS, sensor_dt: float = SENSOR_DT, point_label_key: str | None = None, motion_min: float = MOTION_MIN, **params) -> dict:
    """The program: for every scene of ``data_dir`` and every name of ``res_names``, the stored ``boxes_<name>`` and ``pose0`` of its
    sweeps in index order through ``BoxTracker.track``, ``batch`` scenes per launch; writes ``<timestamp>/tracks_<name>`` float64 [F, 6]
    (rule F) into the scene files or the npz container, the way ``box_fit`` stores its boxes.  Reads no point data.  Under ``torchrun``
    whole scenes per rank, scene ``i % world``.  Returns what ``--json`` writes: {name: {...}} over every rank."""
    from . import distenv, stored
    from .dataset import open_dataset
    from .eval_box import MAX_BOXES as GT_MAX
    from .sweeps import sharded_scenes
    names = stored.result_names(res_names, raw_ok=False)
    if gt is not None and not gt:
        raise ValueError("--gt: the name whose boxes are the ground truth (`python -m himo_amd.box_fit --res_names flow --label_key flow_instance_id`)")
    if gt in names:
        raise ValueError(f"--gt {gt} is among --res_names {','.join(names)}: the ground truth is not scored against itself")
    prm = TrackParams(**params)
    sensor_dt = check_sensor_dt(sensor_dt)
    stored.at_least_one("batch", batch, " scene per launch")
    stored.at_least_one("min_hits", min_hits)
    stored.check_motion_min(motion_min)
    if point_label_key == "cluster":
        raise ValueError("--point_label_key cluster: clusters made by `box_fit --label_key cluster` are not stored; name the stored per-point key the "
                         "boxes were fitted on")
    root = Path(data_dir)
    box_keys = [boxes_key(s) for s in names] + ([boxes_key(gt)] if gt else [])
    out_keys = [tracks_key(s) for s in names] + ([track_label_key(s) for s in names] if point_label_key else [])
    extra = [point_label_key] if point_label_key else []
    sums = {s: new_sums() for s in names}
    with distenv.process_group() as (rank, world):
        ds = open_dataset(root, vis_name="", eval=False, fields=tuple(box_keys + out_keys + extra + ["pose0"]))
        mine = sharded_scenes(ds)

        def loop():
            # the refusals, before anything touches the GPU or a file is written
            sink = stored.KeySink(ds, root, f"writing '{out_keys[0]}' into the scene files of {data_dir}")
            held = {}
            for sc, items in mine:
                for i in items:
                    where = "/".join(map(str, ds.index[i]))
                    have = held[i] = stored.arrays(ds, i, box_keys + out_keys + extra + ["pose0"])
                    for s, k in zip(names + ([gt] if gt else []), box_keys):
                        if k not in have:
                            raise KeyError(f"{k}: {where} holds no boxes of the name '{s}' (`python -m himo_amd.box_fit --data_dir {data_dir} --res_names "
                                           f"{s} --label_key ...` writes them)")
                        stored.check_box_rows(have[k], k, where, GT_MAX if s == gt else MAX_BOXES)
                    stored.check_pose(have, where)
                    if point_label_key:
                        if point_label_key not in have:
                            raise KeyError(f"{point_label_key}: {where} holds no such per-point label")
                        stored.check_point_labels(have[point_label_key], point_label_key, where)
                    done = [k for k in out_keys if k in have]
                    if done and not overwrite:
                        raise FileExistsError(f"{where} already holds '{done[0]}': pass --overwrite to replace it")
            if not mine:
                return
            tracker = BoxTracker(sensor_dt=sensor_dt, **params)
            ev = None
            if gt:
                from .eval_box import BoxEvaluator
                ev = BoxEvaluator(min_iou=prm.min_iou)
            for lo in range(0, len(mine), int(batch)):
                chunk = mine[lo:lo + int(batch)]
                writes = {}                                         # (scene, timestamp) -> {key: array}
                for s in names:
                    key = boxes_key(s)
                    dets = [[detections(held[i][key], held[i]["pose0"], held[items[0]]["pose0"]) for i in items] for _, items in chunk]
                    res = tracker.track(dets)
                    info = res.scene_info
                    for n, (sc, items) in enumerate(chunk):
                        rows = []
                        for k, i in enumerate(items):
                            tid, age, state, _ = res.sweep(n, k)
                            rows.append(stored_rows(tid, age, state, dets[n][k], held[i]["pose0"], held[items[0]]["pose0"]))
                            w = writes.setdefault((sc, ds.index[i][1]), {})
                            w[tracks_key(s)] = rows[-1]
                            if point_label_key:
                                w[track_label_key(s)] = point_labels(held[i][point_label_key], held[i][key], tid)
                        tally_scene(sums[s], [held[i][key] for i in items], rows, int(info[n, 0]), int(info[n, 1]), min_hits)
                        if gt:
                            g = [held[i][boxes_key(gt)] for i in items]
                            m = ev.match(g, [held[i][key] for i in items])
                            tally_mot(sums[s], [(g[k], rows[k][:, 0]) + m.sweep(k)[0::2] for k in range(len(items))], motion_min, sensor_dt)
                for (sc, ts), arrays in writes.items():             # (scene by scene, in chunk order: the first name's loop made the entries)
                    for k, a in arrays.items():
                        sink.put(sc, ts, k, a)
            sink.close()                                            # (on success only: a failed run leaves its last scene as it was)

        distenv.run_shard(loop, "its share of the scenes", closing=(ds,))
        numbers = summary(distenv.gathered(sums, add_sums), bool(gt))
        distenv.report(rank, "\n".join([f"track (box tracking, v1; parity unpinned), min_iou {prm.min_iou:g}, alpha {prm.alpha:g}, beta {prm.beta:g}, "
                                        f"max_age {prm.max_age}, velocity from the {VEL_MODES[prm.vel_mode]}, min_hits {min_hits}:"] +
                                       [_table(s, numbers[s], gt) for s in names]), numbers, json_path)
    return numbers


def _parser():
    import argparse
    d = TrackParams()
    ap = argparse.ArgumentParser(description="track the stored boxes_<name> of every scene over its sweeps and store <timestamp>/tracks_<name> = id, "
                                             "age, x, y, vx, vy per box (box tracking, v1; parity unpinned: the reference has no such stage; timed on "
                                             "synthetic scenes only, profiles/box_track.txt; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--res_names", required=True, help="comma-separated names whose stored boxes are tracked")
    ap.add_argument("--gt", default=None, help="the name whose stored boxes are the ground truth (box_fit --res_names flow --label_key flow_instance_id): "
                                               "adds TP / FP / FN, identity switches, fragmentations and MOTA")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the tables' numbers to PATH")
    ap.add_argument("--overwrite", action="store_true", help="replace existing tracks_<name> instead of refusing")
    ap.add_argument("--batch", type=int, default=16, help="scenes per launch")
    ap.add_argument("--min_iou", type=float, default=d.min_iou, help="the smallest BEV IoU of a matched pair, 0 < min_iou <= 1")
    ap.add_argument("--alpha", type=float, default=d.alpha, help="position gain, 0..1")
    ap.add_argument("--beta", type=float, default=d.beta, help="velocity gain, 0..1")
    ap.add_argument("--max_age", type=int, default=d.max_age, help="a track dies after more than this many sweeps without a match, 0..255")
    ap.add_argument("--max_tracks", type=int, default=d.max_tracks, help=f"live tracks of a scene, 1..{MAX_BOXES}")
    ap.add_argument("--vel_mode", default="box", choices=VEL_MODES, help="'box': the velocity follows the boxes' own (the default); 'track': it "
                                                                        "follows the position residual")
    ap.add_argument("--min_hits", type=int, default=MIN_HITS, help="a track with this many matched boxes is confirmed")
    ap.add_argument("--sensor_dt", type=float, default=SENSOR_DT, help="seconds between sweeps")
    ap.add_argument("--point_label_key", default=None, metavar="K", help="the stored per-point int key the boxes were fitted on: also writes "
                                                                         "<timestamp>/track_label_<name> int32 [N] (view --color_by label:track_label_<name>)")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.res_names, a.gt, a.json, a.overwrite, a.batch, a.min_hits, a.sensor_dt, a.point_label_key, min_iou=a.min_iou, alpha=a.alpha,
         beta=a.beta, max_age=a.max_age, max_tracks=a.max_tracks, vel_mode=VEL_MODES.index(a.vel_mode))


if __name__ == "__main__":
    _cli()
