"""Track-consistent flow: tracked velocities back into the per-point flow (``python -m himo_amd.track_flow --data_dir D --res_names
seflowpp_best --label_key ray_label`` reads ``boxes_<name>``, ``tracks_<name>``, the poses, ``pc0``, the stored flow ``<name>`` and the
stored per-point key the boxes were fitted on, and writes ``<timestamp>/<name>_track``).  ``box_fit`` gives every cluster a box with a
velocity, ``track`` gives the box an identity over the sweeps of a scene; nothing took that identity back to the flow, so nothing built
on it could be scored by ``eval``, ``eval_flow``, ``save_zip`` or ``score``.  ``rigid_refine`` regularises a flow inside one sweep pair;
this stage regularises it along time: a vehicle's velocity at sweep t becomes the mean over its track around t, not one sweep pair's
estimate.  The output is an ordinary flow key INCLUDING ego motion.

PARITY UNPINNED.  The reference has no such stage (its README says of a segmentation + tracking route to non-ego motion correction that
it "has not been shown to work in practice").  Like ``box_fit``, ``eval_box`` and ``track`` it follows the build's own written rule,
below, and is checked bit for bit against a pure-Python restatement of it (``tests/trackflow_ref.py``), never against the reference.  No
claim is made about the reference's numbers.  Timing: per call of 16 synthetic scenes of 150 sweeps of 300 boxes and 120k points the plan
takes 0.56 ms and the apply 3.87 ms in 16 launches (1.6 us a sweep; 1.96 x ``himo_accum_motion`` on the same rows), one 120k-row sweep applied
alone 11.2 us (profiles/track_flow.txt); nothing has been tried on field data.

The rule -- "track flow, v1" (normative)
========================================
A scene is a run of sweeps k = 0..K-1 in index order.  Sweep k has ``F_k`` box rows (``box_fit``'s float32 ``[12]`` layout: columns 7..9
the velocity in the sensor frame, column 10 the label id) and as many ``tracks_<name>`` rows (float64 ``[6]``, column 0 the track id).
Only ``+ - * /`` and comparisons appear and every operation rounds on its own (``himo_amd/csrc/trackflow.hip`` is built with
``-ffp-contract=off``); where numpy or a shared function is called it is named.

A. Host preparation (Python, float64, box rows only).  ``T_k = inv(pose0_first) @ pose0_k`` (numpy), as rule A of box tracking.  Per box
   row: ``id`` = column 0 of the tracks row as an integer; ``v`` = box columns 7..9 widened to float64; ``w = R_k v`` with ``R_k =
   T_k[:3,:3]``, each component ``((R0*vx + R1*vy) + R2*vz)``.  A row is USABLE iff ``id >= 0`` and ``w`` is finite; a row that is not
   gets id -1 and ``w`` = NaN.  Per sweep: ``U_k = inv(T_k)[:3,:3]`` (numpy), nine float64; the box label ids (box column 10 as int32)
   sorted ascending and stable, each with its row index: among equal ids the lowest row wins.
B. Track length.  ``L(id)`` = the number of USABLE rows of the scene that carry the id.  A track is CONFIRMED iff ``L >= min_len``
   (default 3, ``track.MIN_HITS``).
C. Smoothing, for a USABLE row of sweep k on a CONFIRMED track t.  ``S = +0.0`` per component, ``m = 0``; for ``j = max(0, k - half) ..
   min(K - 1, k + half)`` ascending: if sweep j holds a USABLE row of id t (the lowest such row), ``S += w_j`` and ``m += 1``.  ``wbar =
   S / (double)m``.  Sweep k itself always counts, so ``m >= 1``; sweeps the track missed contribute nothing.
D. Back to the sweep.  ``u = U_k wbar`` in the same written order; ``d_s = u * sensor_dt``; ``d_b = (double)v32 * sensor_dt`` with
   ``v32`` the box's float32 velocity.  The row is STATIC (2) iff ``((d_s.x^2 + d_s.y^2) + d_s.z^2) < motion_min^2`` in float64, else
   MOVING (1).  Rows that are not USABLE or not CONFIRMED are NONE (0).  Per row the plan holds: the state int32; ``m`` int32; ``shift =
   (float)(d_s - d_b)`` and ``disp = (float)d_s``, float32 ``[3]`` each; ``u`` float64 ``[3]`` for the report (NONE: zeros everywhere).
E. Points.  Row i of sweep k has label ``lab_i``; its box is the row whose label id equals ``lab_i``, and ``lab_i > 0`` is required.
   The input bytes stay untouched (NaN payloads included) when the point has no box, the box is NONE, or one of the three stored flow
   values is not finite.  Otherwise, with ``E = inv(pose1) @ pose0`` (numpy float64) as float32 and ``a_i = E p_i`` by exactly the
   sequence of ``csrc/rigid_math.h`` (``himo_rigid_transform``):
     STATIC, both modes:        ``out = a_i - pc0_i`` -- the ego-motion flow, the bits ``rigid_refine`` gives a static cluster;
     MOVING, ``shift`` (default): ``out = flow_i + shift``, one float32 addition per component: every point keeps its deviation from its
                                cluster's mean, so a rotation found by ``rigid_refine`` survives;
     MOVING, ``replace``:       ``out = (a_i - pc0_i) + disp``, two float32 operations per component.
   Per sweep two integer counts: rows written as MOVING, rows written as STATIC.
F. Parameters (``TrackFlowParams``, mirrored as ``himo_trackflow_params``, 32 bytes): ``sensor_dt`` double 0.1 (finite, > 0);
   ``motion_min`` double 0.05 (finite, >= 0); ``half`` int32 2 (0..8); ``min_len`` int32 3 (>= 1); ``mode`` int32 0 (0 = shift, 1 =
   replace); reserved 0.  At most ``HIMO_BOXTRACK_MAX`` = 512 boxes per sweep.  Everything else is refused before a launch, with no
   write.

Not part of v1: a yaw rate or any rotation from the track, smoothing of size or heading, weights by point count, velocities from centre
differences, a Kalman or RTS smoother, flow for sweeps a track coasted through (there is no box there, hence no labelled rows), an
in-line switch of ``save``.

Python sequences launches and owns no arithmetic on point data (rule A's arithmetic is on box rows, as ``track.detections``).
``TrackFlow.plan`` and ``TrackFlow.apply`` return without a host wait; the results' host copies are made when asked for.  There is no
CPU path.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .box_fit import MOTION_MIN, SENSOR_DT, boxes_key
from .stored import fmt, ratio
from .track import MAX_BOXES, MIN_HITS, check_sensor_dt, scene_transform, tracks_key

NONE, MOVING, STATIC = 0, 1, 2
MODES = ("shift", "replace")
MAX_HALF = 8


def track_flow_key(name: str) -> str:
    return f"{name}_track"


class _CParams(ctypes.Structure):
    """mirror of ``himo_trackflow_params`` (include/himo_amd.h)"""
    _fields_ = [("sensor_dt", ctypes.c_double), ("motion_min", ctypes.c_double), ("half", ctypes.c_int32), ("min_len", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@dataclass(frozen=True)
class TrackFlowParams:
    """the parameters of "track flow, v1"; refuses what the rule does not admit before anything is launched"""
    sensor_dt: float = SENSOR_DT
    motion_min: float = MOTION_MIN
    half: int = 2
    min_len: int = MIN_HITS
    mode: int = 0

    def __post_init__(self):
        check_sensor_dt(self.sensor_dt)
        v = self.motion_min
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v >= 0:
            raise ValueError(f"TrackFlowParams.motion_min={v!r}: finite and >= 0")
        for name, lo, hi in (("half", 0, MAX_HALF), ("min_len", 1, 2 ** 31 - 1), ("mode", 0, 1)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"TrackFlowParams.{name}={v!r}: an integer, {lo}..{hi}")

    def c_struct(self) -> _CParams:
        return _CParams(float(self.sensor_dt), float(self.motion_min), int(self.half), int(self.min_len), int(self.mode), 0)


# ---- rule A: the host preparation -------------------------------------------------------------------------------------------------------
SweepBoxes = namedtuple("SweepBoxes", "boxes id w U sorted_id sorted_row")
SweepBoxes.__doc__ = """rule A's tables of one sweep: ``boxes`` float32 [F, 12], ``id`` int32 [F], ``w`` float64 [F, 3], ``U`` float64 [9],
``sorted_id`` / ``sorted_row`` int32 [F]"""


def prepare(box_rows, track_rows, pose0, pose0_first) -> SweepBoxes:
    """Rule A: the stored ``boxes_<name>`` and ``tracks_<name>`` rows of a sweep with pose ``pose0`` -> a ``SweepBoxes``"""
    b = np.ascontiguousarray(box_rows, dtype=np.float32)
    tr = np.asarray(track_rows, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 12:
        raise ValueError(f"box rows are float32 [F, 12], not {b.shape}")
    if tr.ndim != 2 or tr.shape[1] < 1 or len(tr) != len(b):
        raise ValueError(f"track rows are [F, 6] with one row per box ({len(b)}), not {tr.shape}")
    T = scene_transform(pose0, pose0_first)
    U = np.ascontiguousarray(np.linalg.inv(T)[:3, :3]).reshape(9)
    v = b[:, 7:10].astype(np.float64)
    with np.errstate(all="ignore"):
        w = np.stack([(T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]) + T[r, 2] * v[:, 2] for r in range(3)], axis=1) if len(b) else np.zeros((0, 3))
        tid = np.where(np.isfinite(tr[:, 0]), tr[:, 0], -1.0)
        tid = np.clip(tid, -1.0, 2.0 ** 31 - 1).astype(np.int64)
        label = np.clip(np.where(np.isfinite(b[:, 10]), b[:, 10], 0.0).astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64).astype(np.int32)
    usable = (tid >= 0) & np.isfinite(w).all(axis=1)
    tid = np.where(usable, tid, -1).astype(np.int32)
    w = np.ascontiguousarray(np.where(usable[:, None], w, np.nan))
    order = np.argsort(label, kind="stable").astype(np.int32)
    return SweepBoxes(b, tid, w, U, np.ascontiguousarray(label[order]), order)


def ego_transform(pose0, pose1) -> np.ndarray:
    """rule E's ``E``: the first three rows of ``inv(pose1) @ pose0`` as float32 [12]"""
    E = (np.linalg.inv(np.asarray(pose1, dtype=np.float64)) @ np.asarray(pose0, dtype=np.float64)).astype(np.float32)
    return np.ascontiguousarray(E[:3]).reshape(12)


# ---- rules B-E: the binding -------------------------------------------------------------------------------------------------------------
class TrackFlowPlan:
    """What ``TrackFlow.plan`` returns, over the scenes of the call in the packed order of ``BoxTracker.tables`` (``sweep_off`` int64
    [n + 1], ``det_off`` int64 [sweeps + 1]): ``state`` int32 [rows], ``m`` int32 [rows], ``shift`` float32 [rows, 3], ``disp`` float32
    [rows, 3], ``u`` float64 [rows, 3].  Host copies, made when first asked for (that is a wait); ``device`` holds the five device
    tensors in that order, ``tables`` the device tables ``apply`` reads.  ``sweep(n, k)`` gives sweep k of scene n: (state, m, shift,
    disp, u)."""

    def __init__(self, tensors, sweep_off, det_off, tables):
        self.device, self.sweep_off, self.det_off, self.tables = tuple(tensors), sweep_off, det_off, tables
        self._host = None

    def _copies(self):
        if self._host is None:
            self._host = tuple(t.cpu().numpy() for t in self.device)
        return self._host

    state = property(lambda self: self._copies()[0])
    m = property(lambda self: self._copies()[1])
    shift = property(lambda self: self._copies()[2])
    disp = property(lambda self: self._copies()[3])
    u = property(lambda self: self._copies()[4])

    def __len__(self):
        return len(self.sweep_off) - 1

    def sweeps(self, n: int) -> int:
        return int(self.sweep_off[n + 1] - self.sweep_off[n])

    def rows(self, n: int, k: int):
        """the packed row range of sweep k of scene n"""
        q = int(self.sweep_off[n]) + k
        return int(self.det_off[q]), int(self.det_off[q + 1])

    def sweep(self, n: int, k: int):
        lo, hi = self.rows(n, k)
        return self.state[lo:hi], self.m[lo:hi], self.shift[lo:hi], self.disp[lo:hi], self.u[lo:hi]


class AppliedFlow:
    """What ``TrackFlow.apply`` returns: ``flow`` (device float32 [rows, 3], the sweeps' rows packed in the order given), ``pt_off``
    int64 [sweeps + 1], and ``counts`` int32 [sweeps, 2] (rows written as MOVING, as STATIC): a host copy made when asked for"""

    def __init__(self, flow, counts, pt_off):
        self.flow, self.device_counts, self.pt_off = flow, counts, pt_off
        self._counts = None

    @property
    def counts(self) -> np.ndarray:
        if self._counts is None:
            self._counts = self.device_counts.cpu().numpy()
        return self._counts

    def sweep(self, j: int):
        """the device rows of the j-th sweep of the call"""
        return self.flow[int(self.pt_off[j]):int(self.pt_off[j + 1])]


class TrackFlow:
    """``TrackFlow(device, **params)``: ``plan(scenes)`` -> a ``TrackFlowPlan`` (rules B-D; a batch of scenes, three launches) and
    ``apply(plan, sweeps, pc0, flow, label, E)`` -> an ``AppliedFlow`` (rule E; several sweeps in one launch).  A scene is a list of
    ``SweepBoxes``, one per sweep in order (``prepare`` makes one: rule A).  There is no CPU path."""

    def __init__(self, device=None, **params):
        from . import _lib
        self.params = TrackFlowParams(**params)
        self.lib = _lib.load()
        if self.lib.himo_abi_sizeof(b"himo_trackflow_params") != ctypes.sizeof(_CParams):
            raise ImportError("himo_trackflow_params: the library's layout is not this binding's; rebuild libhimo_amd.so")
        self.device = device if device is not None else _lib.require_gpu()

    def tables(self, scenes):
        """the host tables of a plan call, checked: (boxes, id, w, U, sorted_id, sorted_row, sweep_off, det_off, id_off)"""
        scenes = [list(sc) for sc in scenes]
        counts, n_ids = [], []
        for n, sc in enumerate(scenes):
            top = 0
            for k, s in enumerate(sc):
                F = len(s.boxes)
                if np.asarray(s.boxes).shape != (F, 12) or np.asarray(s.id).shape != (F,) or np.asarray(s.w).shape != (F, 3) or \
                        np.asarray(s.U).shape != (9,) or np.asarray(s.sorted_id).shape != (F,) or np.asarray(s.sorted_row).shape != (F,):
                    raise ValueError(f"scene {n}, sweep {k}: not the tables of one sweep (``prepare`` makes them)")
                if F > MAX_BOXES:
                    raise ValueError(f"scene {n}, sweep {k} holds {F} boxes: at most {MAX_BOXES} per sweep")
                counts.append(F)
                if F:
                    top = max(top, int(np.max(s.id)) + 1)
            n_ids.append(top)
        sweep_off = np.zeros(len(scenes) + 1, dtype=np.int64)
        np.cumsum([len(sc) for sc in scenes], out=sweep_off[1:])
        det_off = np.zeros(len(counts) + 1, dtype=np.int64)
        np.cumsum(counts, out=det_off[1:])
        id_off = np.zeros(len(scenes) + 1, dtype=np.int64)
        np.cumsum(n_ids, out=id_off[1:])
        flat = [s for sc in scenes for s in sc]

        def cat(field, dtype, tail):
            parts = [np.asarray(getattr(s, field), dtype=dtype).reshape((-1,) + tail) for s in flat]
            return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0,) + tail, dtype=dtype)
        return (cat("boxes", np.float32, (12,)), cat("id", np.int32, ()), cat("w", np.float64, (3,)), cat("U", np.float64, (9,)),
                cat("sorted_id", np.int32, ()), cat("sorted_row", np.int32, ()), sweep_off, det_off, id_off)

    def plan(self, scenes) -> TrackFlowPlan:
        import torch
        from . import _lib
        P, dev = _lib.ptr, self.device
        boxes, tid, w, U, sid, srow, sweep_off, det_off, id_off = self.tables(list(scenes))
        n, rows = len(sweep_off) - 1, len(boxes)
        up = lambda a: torch.from_numpy(a).to(dev)                  # noqa: E731
        d_boxes, d_id, d_w, d_U, d_sid, d_srow, d_so, d_do, d_io = (up(a) for a in (boxes, tid, w, U, sid, srow, sweep_off, det_off, id_off))
        out = (torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev),
               torch.zeros((rows, 3), dtype=torch.float32, device=dev), torch.zeros((rows, 3), dtype=torch.float32, device=dev),
               torch.zeros((rows, 3), dtype=torch.float64, device=dev))
        if n:
            prm = self.params.c_struct()
            need = int(self.lib.himo_trackflow_workspace_bytes(n, sweep_off.ctypes.data, det_off.ctypes.data, id_off.ctypes.data))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                st = self.lib.himo_trackflow_plan(n, sweep_off.ctypes.data, P(d_so), det_off.ctypes.data, P(d_do), id_off.ctypes.data, P(d_io),
                                                  P(d_id), P(d_w), P(d_boxes), P(d_U), ctypes.addressof(prm), P(out[0]), P(out[1]), P(out[2]),
                                                  P(out[3]), P(out[4]), P(ws), ws.numel(), _lib.stream_handle())
            _lib.check(st, "himo_trackflow_plan")
        return TrackFlowPlan(out, sweep_off, det_off, (d_sid, d_srow))

    def apply(self, plan: TrackFlowPlan, sweeps, pc0, flow, label, E) -> AppliedFlow:
        """Rule E for the sweeps ``sweeps`` = [(scene n, sweep k)] of ``plan``: ``pc0`` / ``flow`` / ``label`` are lists with one array or
        device tensor per sweep ((N, >= 3) float32, (N, 3) float32, (N,) integer), ``E`` one ``ego_transform`` per sweep."""
        import torch
        from . import _lib
        from .accumulate import device_rows
        P, dev = _lib.ptr, self.device
        sweeps = [(int(n), int(k)) for n, k in sweeps]
        if not (len(sweeps) == len(pc0) == len(flow) == len(label) == len(E)):
            raise ValueError("apply: one pc0, flow, label and E per sweep")
        dev_of = lambda x, dt: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dt)   # noqa: E731
        pts = [device_rows(p, dev) for p in pc0]
        fls = [dev_of(f, torch.float32).reshape(-1, 3) for f in flow]
        labs = []
        for j, lab in enumerate(label):
            if not isinstance(lab, torch.Tensor):
                lab = np.asarray(lab)
                if lab.ndim != 1 or lab.dtype.kind not in "iu":
                    raise ValueError(f"sweep {j}: labels are one integer per point, not {lab.dtype} {lab.shape}")
                lab = torch.from_numpy(np.ascontiguousarray(lab if lab.dtype.kind == "i" else np.minimum(lab, 2 ** 31 - 1), dtype=np.int64))
            a = lab
            if a.dim() != 1 or a.dtype.is_floating_point or a.dtype == torch.bool:
                raise ValueError(f"sweep {j}: labels are one integer per point, not {a.dtype} {tuple(a.shape)}")
            labs.append(a.to(dev).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32))
        pitches = {int(p.shape[1]) for p in pts}
        if len(pitches) > 1:
            pts = [p[:, :3].contiguous() for p in pts]
        for j, (p, f, a) in enumerate(zip(pts, fls, labs)):
            if f.shape[0] != p.shape[0] or a.shape[0] != p.shape[0]:
                raise ValueError(f"sweep {j}: flow {tuple(f.shape)} / labels {tuple(a.shape)} are not row-aligned with its {p.shape[0]} points")
        ns = len(sweeps)
        pt_off = np.zeros(ns + 1, dtype=np.int64)
        np.cumsum([int(p.shape[0]) for p in pts], out=pt_off[1:])
        rows = int(pt_off[ns])
        out = torch.empty((rows, 3), dtype=torch.float32, device=dev)
        counts = torch.zeros((ns, 2), dtype=torch.int32, device=dev)
        if ns == 0:
            return AppliedFlow(out, counts, pt_off)
        # the entry point takes ONE offsets table per launch, so a launch covers a run of sweeps whose plan rows follow each other; sweeps
        # that are no neighbours in the plan split the call into several launches
        ranges = [plan.rows(n, k) for n, k in sweeps]
        cat = lambda xs, tail, dt: torch.cat(xs) if len(xs) > 1 else (xs[0] if xs else torch.zeros((0,) + tail, dtype=dt, device=dev))   # noqa: E731
        d_pts, d_fl, d_lab = cat(pts, (3,), torch.float32).contiguous(), cat(fls, (3,), torch.float32).contiguous(), cat(labs, (), torch.int32).contiguous()
        d_E = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(e, dtype=np.float32).reshape(12) for e in E]))).to(dev)
        pitch = int(d_pts.shape[1]) if d_pts.dim() == 2 and d_pts.shape[0] else 3
        prm = self.params.c_struct()
        d_sid, d_srow = plan.tables
        total = int(plan.det_off[-1])
        lo = 0
        while lo < ns:                                              # runs of sweeps whose plan rows follow each other
            hi = lo + 1
            while hi < ns and ranges[hi][0] == ranges[hi - 1][1]:
                hi += 1
            h_pt = np.ascontiguousarray(pt_off[lo:hi + 1] - pt_off[lo])
            h_box = np.asarray([ranges[lo][0]] + [r[1] for r in ranges[lo:hi]], dtype=np.int64)
            d_pt, d_box = torch.from_numpy(h_pt).to(dev), torch.from_numpy(h_box).to(dev)
            r0, es = int(pt_off[lo]), d_pts.element_size()
            with torch.cuda.device(dev):
                st = self.lib.himo_trackflow_apply(hi - lo, h_pt.ctypes.data, P(d_pt), P(d_pts) + r0 * pitch * es, pitch, P(d_fl) + r0 * 3 * es,
                                                   P(d_lab) + r0 * 4, P(d_E) + lo * 48, h_box.ctypes.data, P(d_box), total, P(d_sid), P(d_srow),
                                                   P(plan.device[0]), P(plan.device[2]), P(plan.device[3]), ctypes.addressof(prm),
                                                   P(out) + r0 * 12, P(counts) + lo * 8, _lib.stream_handle())
            _lib.check(st, "himo_trackflow_apply")
            lo = hi
        return AppliedFlow(out, counts, pt_off)


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
def new_sums() -> dict:
    """the running sums of one result name: integers and floats only, so that ranks' sums add up"""
    return {"tracks": 0, "moving": 0, "static": 0, "none": 0, "points_moving": 0, "points_static": 0, "points": 0, "diff_sum": 0.0, "diff_n": 0}


def tally_plan(sums: dict, plan: TrackFlowPlan, scenes, sensor_dt: float) -> None:
    """add a plan call's boxes: the states, the confirmed tracks in use and ``|d_s - d_b|`` over the boxes that are not NONE (float64
    on box rows, in row order)"""
    state, u = plan.state, plan.u
    for n, sc in enumerate(scenes):
        used = set()
        for k, s in enumerate(sc):
            lo, hi = plan.rows(n, k)
            st = state[lo:hi]
            sums["moving"] += int((st == MOVING).sum())
            sums["static"] += int((st == STATIC).sum())
            sums["none"] += int((st == NONE).sum())
            for r in np.flatnonzero(st != NONE):
                used.add(int(s.id[r]))
                d = u[lo + r] * sensor_dt - s.boxes[r, 7:10].astype(np.float64) * sensor_dt
                sums["diff_sum"] += math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                sums["diff_n"] += 1
        sums["tracks"] += len(used)


def summary(sums: dict) -> dict:
    """the numbers of the tables and of ``--json``: {name: {...}}"""
    return {name: {"confirmed_tracks": t["tracks"], "boxes_moving": t["moving"], "boxes_static": t["static"], "boxes_left_alone": t["none"],
                   "points": t["points"], "points_rewritten": t["points_moving"] + t["points_static"], "points_moving": t["points_moving"],
                   "points_static": t["points_static"], "mean_shift": ratio(t["diff_sum"], t["diff_n"])}
            for name, t in sums.items()}


def _table(name: str, r: dict) -> str:
    return (f"{name} -> {track_flow_key(name)}: {r['confirmed_tracks']} confirmed tracks used, boxes MOVING {r['boxes_moving']} STATIC {r['boxes_static']} "
            f"left alone {r['boxes_left_alone']}, {r['points_rewritten']} of {r['points']} points rewritten ({r['points_moving']} moving, "
            f"{r['points_static']} static), mean |d_s - d_b| {fmt(r['mean_shift'], '.4f')} m")


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def main(data_dir: str, res_names, label_key: str, mode: str = "shift", half: int = 2, min_len: int = MIN_HITS, motion_min: float = MOTION_MIN,
         sensor_dt: float = SENSOR_DT, batch: int = 16, json_path: str | None = None, overwrite: bool = False, sweeps_per_launch: int = 32) -> dict:
    """The program: for every scene of ``data_dir`` and every name of ``res_names``, the stored ``boxes_<name>``, ``tracks_<name>`` and
    ``pose0`` of its sweeps through ``TrackFlow.plan`` (``batch`` scenes per call), then every sweep's ``pc0``, ``<name>`` and
    ``label_key`` through ``TrackFlow.apply`` (``sweeps_per_launch`` sweeps per launch); writes ``<timestamp>/<name>_track`` float32
    (N, 3) through ``save``'s sinks (h5 scene files or the npz container).  Under ``torchrun`` whole scenes per rank, scene ``i %
    world``.  Returns what ``--json`` writes: {name: {...}} over every rank."""
    from . import distenv, stored
    from .dataset import NpzDataset, open_dataset
    from .save import H5ResultSink, NpzResultSink
    from .sweeps import sharded_scenes
    names = stored.result_names(res_names, raw_ok=False)
    if "raw" in names:
        raise ValueError("res_names: 'raw' is the zero-motion key, not a stored flow; name the results whose boxes were tracked")
    if mode not in MODES:
        raise ValueError(f"mode={mode!r}: one of {', '.join(MODES)}")
    if not label_key:
        raise ValueError("label_key: the stored per-point integer key the boxes were fitted on (ray_label, flow_instance_id, ...)")
    if label_key == "cluster":
        raise ValueError("--label_key cluster: clusters made by `box_fit --label_key cluster` are not stored; name the stored per-point key the "
                         "boxes were fitted on")
    prm = TrackFlowParams(sensor_dt=sensor_dt, motion_min=motion_min, half=half, min_len=min_len, mode=MODES.index(mode))
    stored.at_least_one("batch", batch)
    stored.at_least_one("sweeps_per_launch", sweeps_per_launch)
    root = Path(data_dir)
    box_keys, trk_keys, out_keys = [boxes_key(s) for s in names], [tracks_key(s) for s in names], [track_flow_key(s) for s in names]
    sums = {s: new_sums() for s in names}
    with distenv.process_group() as (rank, world):
        ds = open_dataset(root, vis_name=names, eval=False, fields=tuple(["pc0", "pose0", "pose1", label_key] + names))
        npz = isinstance(ds, NpzDataset)
        mine = sharded_scenes(ds)

        def loop():
            # the refusals, before anything touches the GPU or a file is written
            held = {}
            for sc, items in mine:
                for i in items:
                    where = "/".join(map(str, ds.index[i]))
                    have = held[i] = stored.arrays(ds, i, box_keys + trk_keys + ["pose0"])
                    present = stored.present(ds, i, names + out_keys + [label_key])
                    for s, bk, tk in zip(names, box_keys, trk_keys):
                        if bk not in have:
                            raise KeyError(f"{bk}: {where} holds no boxes of the name '{s}' (`python -m himo_amd.box_fit --data_dir {data_dir} "
                                           f"--res_names {s} --label_key {label_key}` writes them)")
                        if tk not in have:
                            raise KeyError(f"{tk}: {where} holds no tracks of the name '{s}' (`python -m himo_amd.track --data_dir {data_dir} "
                                           f"--res_names {s}` writes them)")
                        b, t = have[bk], have[tk]
                        stored.check_box_rows(b, bk, where, None)   # (the count is refused after stale tracks, below)
                        stored.check_track_rows(t, b, tk, bk, where, f"python -m himo_amd.track --res_names {s} --overwrite")
                        stored.check_box_rows(b, bk, where, MAX_BOXES)
                        if s not in present:
                            raise KeyError(f"{s}: {where} holds no result of that name")
                    stored.check_pose(have, where)
                    if label_key not in present:
                        raise KeyError(f"{label_key}: {where} holds no such per-point label")
                    done = [k for k in out_keys if k in present]
                    if done and not overwrite:
                        raise FileExistsError(f"{where} already holds '{done[0]}': pass --overwrite to replace it")
            if not mine:
                return
            engine = TrackFlow(**{k: getattr(prm, k) for k in ("sensor_dt", "motion_min", "half", "min_len", "mode")})
            sinks = {s: NpzResultSink(root, track_flow_key(s)) if npz else H5ResultSink(root, track_flow_key(s), before_write=ds.forget)
                     for s in names}
            for lo in range(0, len(mine), int(batch)):
                chunk = mine[lo:lo + int(batch)]
                plans = {}
                for s in names:
                    prep = [[prepare(held[i][boxes_key(s)], held[i][tracks_key(s)], held[i]["pose0"], held[items[0]]["pose0"])
                             for i in items] for _, items in chunk]
                    plans[s] = engine.plan(prep)
                    tally_plan(sums[s], plans[s], prep, prm.sensor_dt)
                for n, (sc, items) in enumerate(chunk):
                    for g in range(0, len(items), int(sweeps_per_launch)):
                        part = items[g:g + int(sweeps_per_launch)]
                        frames = [ds[i] for i in part]
                        for f in frames:
                            stored.check_point_labels(np.asarray(f[label_key]), label_key, f"{f['scene_id']}/{f['timestamp']}", rows=len(f["pc0"]))
                        Es = [ego_transform(f["pose0"], f["pose1"]) for f in frames]
                        for s in names:
                            res = engine.apply(plans[s], [(n, g + j) for j in range(len(part))], [np.asarray(f["pc0"]) for f in frames],
                                               [np.asarray(f[s]) for f in frames], [np.asarray(f[label_key]) for f in frames], Es)
                            host, counts = res.flow.cpu().numpy(), res.counts
                            for j, (i, f) in enumerate(zip(part, frames)):
                                sinks[s](i, f, host[int(res.pt_off[j]):int(res.pt_off[j + 1])])
                            sums[s]["points"] += int(res.pt_off[-1])
                            sums[s]["points_moving"] += int(counts[:, 0].sum())
                            sums[s]["points_static"] += int(counts[:, 1].sum())
            for sink in sinks.values():                             # (on success only: a failed run leaves its last scene as it was)
                if hasattr(sink, "close"):
                    sink.close()

        distenv.run_shard(loop, "its share of the scenes", closing=(ds,))
        numbers = summary(distenv.gathered(sums))
        distenv.report(rank, "\n".join([f"track_flow (track flow, v1; parity unpinned), labels '{label_key}', mode {mode}, half {prm.half}, "
                                        f"min_len {prm.min_len}, motion_min {prm.motion_min:g}, sensor_dt {prm.sensor_dt:g}:"] +
                                       [_table(s, numbers[s]) for s in names]), numbers, json_path)
    return numbers


def _parser():
    import argparse
    d = TrackFlowParams()
    ap = argparse.ArgumentParser(description="move the points of every tracked box by its track's smoothed velocity and store the flow as "
                                             "<timestamp>/<name>_track (track flow, v1; parity unpinned: the reference has no such stage; "
                                             "timing: profiles/track_flow.txt; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--res_names", required=True, help="comma-separated stored flows whose boxes_<name> and tracks_<name> exist")
    ap.add_argument("--label_key", required=True, help="the stored per-point integer key the boxes were fitted on (ray_label, ...; 'cluster' is "
                                                       "refused: such clusters are not stored)")
    ap.add_argument("--mode", default="shift", choices=MODES, help="MOVING rows: 'shift' adds the box's change of displacement to every point's "
                                                                  "flow (the default); 'replace' writes ego motion + the track's displacement")
    ap.add_argument("--half", type=int, default=d.half, help=f"the window is the sweeps k - half .. k + half, 0..{MAX_HALF}")
    ap.add_argument("--min_len", type=int, default=d.min_len, help="a track with this many boxes is confirmed")
    ap.add_argument("--motion_min", type=float, default=d.motion_min, help="a box that moves less than this a sweep is static, metres")
    ap.add_argument("--sensor_dt", type=float, default=d.sensor_dt, help="seconds between sweeps")
    ap.add_argument("--batch", type=int, default=16, metavar="SCENES", help="scenes per plan call")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the tables' numbers to PATH")
    ap.add_argument("--overwrite", action="store_true", help="replace existing <name>_track instead of refusing")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.res_names, a.label_key, a.mode, a.half, a.min_len, a.motion_min, a.sensor_dt, a.batch, a.json, a.overwrite)


if __name__ == "__main__":
    _cli()
