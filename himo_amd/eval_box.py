"""Box evaluation: the rotated IoU of the boxes ``box_fit`` stores, and how many of them find a partner among the boxes of the sweep
compensated by the ground-truth flow (``python -m himo_amd.eval_box --data_dir D --gt flow --res_names raw,seflowpp_best`` reads
``<timestamp>/boxes_flow``, ``boxes_raw`` and ``boxes_seflowpp_best`` and prints one table per result name).  ``box_fit --against`` needs
the same label under both names; this needs none, so it also serves boxes of clusters made per name (``box_fit --label_key cluster``).
The ground truth comes from ``python -m himo_amd.box_fit --res_names flow --label_key flow_instance_id``.

PARITY UNPINNED.  The reference has no such stage.  Like ``box_fit`` it follows the build's own written rule, below, and is checked bit
for bit against a pure-Python restatement of it (``tests/boxeval_ref.py``), never against the reference.  No claim is made about the
reference's numbers.  Timing: 2.06 ms per call of 32 synthetic sweeps of 300 boxes a side, the two launches 0.23 ms of it, beside 1.06 ms for
making ONE sweep's boxes (profiles/box_eval.txt); nothing has been tried on field data.

The rule -- "box evaluation, v1" (normative)
============================================
Two sets of boxes per sweep: A, the ground truth, ``Fa`` boxes, and B, the predicted, ``Fb`` boxes.

A. Rectangles.  The HOST (Python, float64; ``math.cos`` / ``math.sin``; the library calls no transcendental) turns every box row ``x, y, z,
   l, w, h, yaw`` (float32, the row layout of ``box_fit``; every value widened to float64 first) into ``rect`` float64 ``[12]``: with
   ``c = cos(yaw)``, ``s = sin(yaw)``, ``hl = l * 0.5``, ``hw = w * 0.5`` and ``(dx, dy)`` = ``(hl, hw)``, ``(-hl, hw)``, ``(-hl, -hw)``,
   ``(hl, -hw)`` -- counter-clockwise from ``(+l/2, +w/2)`` in the box frame -- corner k is ``x + (dx*c - dy*s)``, ``y + (dx*s + dy*c)``;
   then ``zlo = z - h*0.5``, ``zhi = z + h*0.5``, ``area = l * w``, and one zero.  A rect with any non-finite value, or of a row with
   ``l < 0``, ``w < 0`` or ``h < 0``, is INVALID: the host writes it as twelve NaN.  The library takes a rect as INVALID iff one of its
   twelve values is not finite, ``area < 0`` or ``zhi < zlo``.  The IoU of an INVALID rect with everything is 0 and it is never matched.
   Zero extents are valid (``box_fit`` can produce them).
B. Intersection of the pair (i of A, j of B), in float64, every operation rounding on its own (``himo_amd/csrc/boxeval.hip`` is built
   with ``-ffp-contract=off``); only ``+ - * /`` and comparisons appear.  A is always the subject and B always the clip polygon (the two
   orders differ in the last bits).
   B1. ``P_k = (Ax_k - Ax_0, Ay_k - Ay_0)`` and ``Q_k = (Bx_k - Ax_0, By_k - Ay_0)``, k = 0..3: all eight corners relative to A's
       corner 0.
   B2. With ``axl, axh, ayl, ayh`` the least and greatest x and y of P and ``bxl, ...`` those of Q: ``inter = 0`` if ``axh < bxl`` or
       ``bxh < axl`` or ``ayh < byl`` or ``byh < ayl``.
   B3. Otherwise the polygon V = P (n = 4 vertices) is clipped by B's edges e = 0..3 in turn, edge e running from ``p = Q_e`` to
       ``q = Q_(e+1 mod 4)``: ``ex = qx - px``, ``ey = qy - py``; the side value of a vertex v is ``d(v) = ex*(vy - py) - ey*(vx - px)``
       (two differences, two products, one difference); v is inside iff ``d(v) >= 0``.
   B4. A pass walks m = 0..n-1 with ``s = V_m``, ``e = V_(m+1 mod n)``: if s is inside, s is emitted; then, if exactly one of s, e is
       inside, the crossing is emitted: ``t = ds / (ds - de)``, ``(sx + t*(ex_ - sx), sy + t*(ey_ - sy))`` with ``(ex_, ey_)`` the
       coordinates of e.  Pass e keeps at most ``5 + e`` vertices -- a convex polygon gains at most one per pass, so at most 8 in all; a
       vertex beyond that (rounding alone can make one) is dropped.  The emitted vertices, in order, are the next V.
   B5. With fewer than 3 vertices after the four passes, ``inter = 0``.
   B6. Otherwise ``acc = 0``; for m = 1..n-2 in turn ``acc = acc + ((Vx_m - Vx_0)*(Vy_(m+1) - Vy_0) - (Vx_(m+1) - Vx_0)*(Vy_m - Vy_0))``;
       ``inter = 0.5 * acc``; if not ``inter >= 0`` then ``inter = 0``; if ``inter > min(areaA, areaB)`` then ``inter`` is that minimum.
C. IoU.  ``union = (areaA + areaB) - inter``; ``iou = inter / union`` if ``union > 0``, else 0.  ``dz = min(zhiA, zhiB) - max(zloA,
   zloB)``; ``hz = dz`` if ``dz > 0``, else 0; ``inter3 = inter * hz``; ``den = (areaA*(zhiA - zloA) + areaB*(zhiB - zloB)) - inter3``;
   ``iou3 = inter3 / den`` if ``den > 0``, else 0.
D. Matching, per sweep: greedy by descending BEV IoU.  The candidates are the pairs with ``iou >= min_iou`` (``min_iou``: a parameter,
   default 0.1, admitted iff finite and ``0 < min_iou <= 1``).  They are taken in the total order: greater ``iou`` first, then lower i,
   then lower j; a candidate is kept iff neither its i nor its j has been kept before.  Outputs: ``match_a`` int32 ``[Fa]`` (j or -1),
   ``match_b`` int32 ``[Fb]`` (i or -1), ``iou_a`` float64 ``[Fa][2]`` (iou and iou3 of the kept pair, zeros otherwise).  Because the
   order is descending, the matching at any threshold ``tau >= min_iou`` is the subset of the kept pairs with ``iou >= tau``: a pair
   below ``tau`` is taken after every pair at or above it and so never displaces one.
E. Limits.  At most ``HIMO_BOXEVAL_MAX_BOXES`` = 1024 boxes per side and sweep; any number of sweeps per call.  Anything else is refused
   before a launch, with no write.
F. Host glue (Python, float64, on box rows only).  Per result name, over all sweeps: for ``tau`` in (0.3, 0.5, 0.7) TP (kept pairs with
   ``iou >= tau``), FP (predicted boxes without a partner at ``tau``), FN (ground-truth boxes without one), precision, recall and F1 (None
   where a denominator is zero); the mean iou and mean iou3 of the pairs kept at ``min_iou``; and for those pairs the mean ``|dl|``,
   ``|dw|``, centre distance and folded yaw difference exactly as ``box_fit.tally_against`` forms them.  Each is reported for all
   ground-truth boxes and per bucket of the GROUND-TRUTH box: by speed ``hypot(vx, vy)`` -- ``static`` (below ``motion_min / sensor_dt``),
   then ``0-10`` (below 10), ``10-20``, ``20-30``, ``30+`` m/s, an edge belonging to the bucket above it (the edges of the reference
   evaluator) -- and by range ``hypot(x, y)`` with the same four edges.  A predicted box without a partner has no ground-truth box and
   counts as FP in "all" only; the buckets report TP, FN and recall.
G. ``--pair_by label``: instead of matching, the boxes that carry the same label id (column 10) under both names are paired, and their
   iou and iou3 are reported with the same bucket tables.  No TP / FP / FN: every pair is given.  ``--pair_by iou`` (the default) is
   rule D.

Not part of v1: association over time, AP with a confidence score (cluster boxes have none), 3-D rotation.

Python sequences launches and owns no arithmetic on pairs of boxes.  ``BoxEvaluator.match`` makes the rects on the host, uploads them
and returns without a host wait; the result's host copies are made when asked for.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from pathlib import Path

import numpy as np

from .box_fit import MOTION_MIN, SENSOR_DT, boxes_key
from .stored import fmt, ratio

MAX_BOXES = 1024                    # HIMO_BOXEVAL_MAX_BOXES
TILE = 128                          # HIMO_BOXEVAL_TILE
MIN_IOU = 0.1
TAUS = (0.3, 0.5, 0.7)
EDGES = (10.0, 20.0, 30.0)
SPEED_BUCKETS = ("static", "0-10", "10-20", "20-30", "30+")
RANGE_BUCKETS = ("0-10", "10-20", "20-30", "30+")


class _CParams(ctypes.Structure):
    """mirror of ``himo_boxeval_params`` (include/himo_amd.h)"""
    _fields_ = [("min_iou", ctypes.c_double), ("reserved", ctypes.c_int32 * 2)]


def check_min_iou(v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not 0 < v <= 1:
        raise ValueError(f"min_iou={v!r}: finite, 0 < min_iou <= 1")
    return float(v)


def rects(rows) -> np.ndarray:
    """Rule A: box rows ``[F, >= 7]`` -> rects float64 ``[F, 12]`` on the host (an INVALID rect: twelve NaN)."""
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] < 7:
        raise ValueError(f"box rows are x, y, z, l, w, h, yaw[, ...], not {r.shape}")
    x, y, z, l, w, h, yaw = np.ascontiguousarray(r[:, :7].T, dtype=np.float64)      # (one contiguous float64 vector a column)
    turn = np.isfinite(yaw)
    angle = np.where(turn, yaw, 0.0).tolist()                       # (math.cos refuses an infinity; such a row is INVALID below)
    c = np.fromiter(map(math.cos, angle), dtype=np.float64, count=len(angle))
    s = np.fromiter(map(math.sin, angle), dtype=np.float64, count=len(angle))
    with np.errstate(all="ignore"):
        hl, hw = l * 0.5, w * 0.5
        cols = np.zeros((12, len(x)), dtype=np.float64)
        for k, (dx, dy) in enumerate(((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw))):
            cols[2 * k] = x + (dx * c - dy * s)
            cols[2 * k + 1] = y + (dx * s + dy * c)
        cols[8] = z - h * 0.5
        cols[9] = z + h * 0.5
        cols[10] = l * w
        bad = ~np.isfinite(cols).all(axis=0) | ~turn | (l < 0) | (w < 0) | (h < 0)
    out = np.ascontiguousarray(cols.T)
    out[bad] = np.nan
    return out


class MatchResult:
    """What ``BoxEvaluator.match`` returns, over the sweeps of the call in packed order (``off_a`` / ``off_b`` int64 [S + 1] are the
    sweeps' row ranges): ``match_a`` int32 [rows of A] (the j within the sweep or -1), ``match_b`` int32 [rows of B], ``iou_a`` float64
    [rows of A, 2] (iou, iou3 of the kept pair).  Host copies, made when first asked for (that is a wait); ``device_match_a``,
    ``device_match_b`` and ``device_iou_a`` are the device tensors.  ``sweep(s)`` gives one sweep's three host arrays."""

    def __init__(self, match_a, match_b, iou_a, off_a, off_b):
        self.device_match_a, self.device_match_b, self.device_iou_a, self.off_a, self.off_b = match_a, match_b, iou_a, off_a, off_b
        self._host = None

    def _copies(self):
        if self._host is None:
            self._host = (self.device_match_a.cpu().numpy(), self.device_match_b.cpu().numpy(), self.device_iou_a.cpu().numpy())
        return self._host

    match_a = property(lambda self: self._copies()[0])
    match_b = property(lambda self: self._copies()[1])
    iou_a = property(lambda self: self._copies()[2])

    def __len__(self):
        return len(self.off_a) - 1

    def sweep(self, s: int):
        a0, a1, b0, b1 = int(self.off_a[s]), int(self.off_a[s + 1]), int(self.off_b[s]), int(self.off_b[s + 1])
        return self.match_a[a0:a1], self.match_b[b0:b1], self.iou_a[a0:a1]


class BoxEvaluator:
    """``BoxEvaluator(device, min_iou).match(list_of_rows_a, list_of_rows_b)`` -> a ``MatchResult`` (rules A-E; a batch of sweeps in one
    call); ``.iou_pairs(rows_a, rows_b, pairs)`` -> device float64 [n, 2] (rules A-C for listed pairs).  There is no CPU path."""

    def __init__(self, device=None, min_iou: float = MIN_IOU):
        from . import _lib
        self.min_iou = check_min_iou(min_iou)
        self.lib = _lib.load()
        if self.lib.himo_abi_sizeof(b"himo_boxeval_params") != ctypes.sizeof(_CParams):
            raise ImportError("himo_boxeval_params: the library's layout is not this binding's; rebuild libhimo_amd.so")
        self.device = device if device is not None else _lib.require_gpu()

    def match(self, rows_a, rows_b) -> MatchResult:
        import torch
        from . import _lib
        P, dev = _lib.ptr, self.device
        rows_a, rows_b = list(rows_a), list(rows_b)
        if len(rows_a) != len(rows_b):
            raise ValueError(f"{len(rows_a)} sweeps of A but {len(rows_b)} of B")
        S = len(rows_a)
        sides = []
        for rows, side in ((rows_a, "A"), (rows_b, "B")):
            rows = [np.asarray(r) for r in rows]
            for k, r in enumerate(rows):
                if r.ndim != 2 or r.shape[1] < 7:
                    raise ValueError(f"sweep {k} of {side}: box rows are x, y, z, l, w, h, yaw[, ...], not {r.shape}")
                if len(r) > MAX_BOXES:
                    raise ValueError(f"sweep {k} of {side} holds {len(r)} boxes: at most {MAX_BOXES} per side and sweep")
            off = np.zeros(S + 1, dtype=np.int64)
            np.cumsum([len(r) for r in rows], out=off[1:])
            table = rects(np.concatenate([r[:, :7] for r in rows])) if rows else np.zeros((0, 12))      # rule A once for the side
            sides.append((np.ascontiguousarray(table), off))
        (ta, off_a), (tb, off_b) = sides
        na, nb = int(off_a[S]), int(off_b[S])
        d_ra, d_rb = torch.from_numpy(ta).to(dev), torch.from_numpy(tb).to(dev)
        d_oa, d_ob = torch.from_numpy(off_a).to(dev), torch.from_numpy(off_b).to(dev)
        match_a = torch.empty(na, dtype=torch.int32, device=dev)
        match_b = torch.empty(nb, dtype=torch.int32, device=dev)
        iou_a = torch.empty((na, 2), dtype=torch.float64, device=dev)
        if S and (na or nb):
            need = int(self.lib.himo_boxeval_workspace_bytes(S, off_a.ctypes.data, off_b.ctypes.data))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            prm = _CParams(self.min_iou)
            with torch.cuda.device(dev):
                st = self.lib.himo_boxeval_match(S, P(d_ra), off_a.ctypes.data, P(d_oa), P(d_rb), off_b.ctypes.data, P(d_ob), ctypes.addressof(prm),
                                                 P(match_a), P(match_b), P(iou_a), P(ws), ws.numel(), _lib.stream_handle())
            _lib.check(st, "himo_boxeval_match")
        return MatchResult(match_a, match_b, iou_a, off_a, off_b)

    def iou_pairs(self, rows_a, rows_b, pairs):
        import torch
        from . import _lib
        P, dev = _lib.ptr, self.device
        ta, tb = rects(rows_a), rects(rows_b)
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        out = torch.empty((len(pr), 2), dtype=torch.float64, device=dev)
        if len(pr):
            d_ra, d_rb, d_pr = torch.from_numpy(ta).to(dev), torch.from_numpy(tb).to(dev), torch.from_numpy(pr).to(dev)
            with torch.cuda.device(dev):
                st = self.lib.himo_box_iou_pairs(len(pr), P(d_ra), len(ta), P(d_rb), len(tb), P(d_pr), P(out), _lib.stream_handle())
            _lib.check(st, "himo_box_iou_pairs")
        return out


# ---- rule F: the host glue --------------------------------------------------------------------------------------------------------------
def speed_bucket(v: float, motion_min: float = MOTION_MIN, sensor_dt: float = SENSOR_DT) -> str:
    if v < motion_min / sensor_dt:
        return "static"
    return "0-10" if v < EDGES[0] else "10-20" if v < EDGES[1] else "20-30" if v < EDGES[2] else "30+"


def range_bucket(r: float) -> str:
    return "0-10" if r < EDGES[0] else "10-20" if r < EDGES[1] else "20-30" if r < EDGES[2] else "30+"


def bucket_keys() -> list:
    return ["all"] + [f"speed {b}" for b in SPEED_BUCKETS] + [f"range {b}" for b in RANGE_BUCKETS]


def buckets_of(rows_gt: np.ndarray, motion_min: float = MOTION_MIN, sensor_dt: float = SENSOR_DT) -> list:
    """per ground-truth row, the bucket keys it counts in: "all", its speed bucket, its range bucket"""
    g = np.asarray(rows_gt, dtype=np.float64)
    return [("all", "speed " + speed_bucket(math.hypot(r[7], r[8]), motion_min, sensor_dt), "range " + range_bucket(math.hypot(r[0], r[1])))
            for r in g]


def new_sums() -> dict:
    """the running sums of one result name: integers and floats only, so that ranks' sums add up"""
    from .box_fit import new_against
    out = {"pred": 0, "buckets": {}}
    for key in bucket_keys():
        out["buckets"][key] = {"gt": 0, "pairs": 0, "sum_iou": 0.0, "sum_iou3": 0.0, "tp": [0] * len(TAUS), "shape": new_against()["all"]}
    return out


def tally(sums: dict, rows_gt, rows_pred, match_gt, iou_gt, motion_min: float = MOTION_MIN, sensor_dt: float = SENSOR_DT) -> None:
    """add one sweep to a result's sums: ``match_gt`` int [Fa] (the predicted row or -1) and ``iou_gt`` float64 [Fa, 2] are rule D's
    ``match_a`` and ``iou_a`` -- or, for ``--pair_by label``, the given pairs and their IoUs"""
    from .box_fit import tally_against
    rows_gt, rows_pred, match_gt, iou_gt = np.asarray(rows_gt), np.asarray(rows_pred), np.asarray(match_gt), np.asarray(iou_gt, dtype=np.float64)
    sums["pred"] += int(len(rows_pred))
    keys = buckets_of(rows_gt, motion_min, sensor_dt)
    members = {}
    for i, ks in enumerate(keys):
        for k in ks:
            members.setdefault(k, []).append(i)
    for k, rows in members.items():
        b = sums["buckets"][k]
        rows = np.asarray(rows, dtype=np.int64)
        kept = rows[match_gt[rows] >= 0]
        b["gt"] += int(len(rows))
        b["pairs"] += int(len(kept))
        for i in kept:                                              # (in row order: the sums are the restatement's)
            b["sum_iou"] += float(iou_gt[i, 0])
            b["sum_iou3"] += float(iou_gt[i, 1])
        for n, tau in enumerate(TAUS):
            b["tp"][n] += int((iou_gt[kept, 0] >= tau).sum())
        if len(kept):
            ids = np.arange(len(kept))
            on = np.ones(len(kept), dtype=bool)
            acc = {"all": b["shape"], "moving": dict(b["shape"])}
            tally_against(acc, rows_gt[kept], on, ids, rows_pred[match_gt[kept]], on, ids)


def summary(sums: dict, pair_by: str = "iou") -> dict:
    """the numbers of the tables and of ``--json``: {name: {bucket: {...}}}"""
    out = {}
    for name, t in sums.items():
        out[name] = {"pred": t["pred"], "buckets": {}}
        for key, b in t["buckets"].items():
            sh = b["shape"]
            r = {"gt": b["gt"], "pairs": b["pairs"], "mean_iou": ratio(b["sum_iou"], b["pairs"]), "mean_iou3": ratio(b["sum_iou3"], b["pairs"]),
                 "mean_dl": ratio(sh["sum_dl"], sh["pairs"]), "mean_dw": ratio(sh["sum_dw"], sh["pairs"]),
                 "mean_centre": ratio(sh["sum_centre"], sh["pairs"]), "mean_yaw_deg": ratio(sh["sum_yaw_deg"], sh["pairs"])}
            if pair_by == "iou":
                r["at"] = {}
                for n, tau in enumerate(TAUS):
                    tp = b["tp"][n]
                    fn = b["gt"] - tp
                    at = {"tp": tp, "fn": fn, "recall": ratio(tp, tp + fn)}
                    if key == "all":
                        fp = t["pred"] - tp
                        p, rc = ratio(tp, tp + fp), at["recall"]
                        at.update(fp=fp, precision=p, f1=None if p is None or rc is None or p + rc == 0 else 2 * p * rc / (p + rc))
                    r["at"][f"{tau:g}"] = at
            out[name]["buckets"][key] = r
    return out


def _table(name: str, r: dict, gt: str, pair_by: str) -> str:
    lines = [f"{name} against {gt} ({'greedy matching by BEV IoU' if pair_by == 'iou' else 'pairs by label'}): {r['pred']} predicted boxes, "
             f"{r['buckets']['all']['gt']} ground-truth boxes"]
    for key, b in r["buckets"].items():
        line = (f"  {key:<12} gt {b['gt']:>6} pairs {b['pairs']:>6}  iou {fmt(b['mean_iou'])} iou3 {fmt(b['mean_iou3'])}  |dl| {fmt(b['mean_dl'])} m "
                f"|dw| {fmt(b['mean_dw'])} m centre {fmt(b['mean_centre'])} m yaw {fmt(b['mean_yaw_deg'], '.2f')} deg")
        for tau, at in b.get("at", {}).items():
            line += f"  @{tau}: TP {at['tp']} FN {at['fn']} R {fmt(at['recall'])}"
            if "fp" in at:
                line += f" FP {at['fp']} P {fmt(at['precision'])} F1 {fmt(at['f1'])}"
        lines.append(line)
    return "\n".join(lines)


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def label_pairs(rows_gt: np.ndarray, rows_pred: np.ndarray):
    """rule G: (rows of gt, rows of pred) that carry the same label id in column 10, in ascending id (the first row of an id on a side)"""
    ia = np.unique(rows_gt[:, 10], return_index=True)
    ib = np.unique(rows_pred[:, 10], return_index=True)
    _, ka, kb = np.intersect1d(ia[0], ib[0], assume_unique=True, return_indices=True)
    return ia[1][ka].astype(np.int64), ib[1][kb].astype(np.int64)


def main(data_dir: str, gt: str, res_names, pair_by: str = "iou", min_iou: float = MIN_IOU, batch: int = 32, json_path: str | None = None,
         motion_min: float = MOTION_MIN) -> dict:
    """The program: the stored ``boxes_<name>`` of every sweep of ``data_dir``, for every name of ``res_names``, against ``boxes_<gt>``;
    ``batch`` sweeps per launch.  Reads nothing but the boxes.  Under ``torchrun`` sweeps ``i % world`` per rank.  Returns what ``--json``
    writes: {name: {"pred", "buckets": {bucket: {...}}}} over every rank."""
    from . import distenv, stored
    from .dataset import open_dataset
    from .sweeps import sharded_items
    names = stored.result_names(res_names, raw_ok=False)
    if not gt:
        raise ValueError("--gt: the name whose boxes are the ground truth (`python -m himo_amd.box_fit --res_names flow --label_key flow_instance_id`)")
    if gt in names:
        raise ValueError(f"--gt {gt} is among --res_names {','.join(names)}: the ground truth is not scored against itself")
    if pair_by not in ("iou", "label"):
        raise ValueError(f"pair_by={pair_by!r}: 'iou' or 'label'")
    min_iou = check_min_iou(min_iou)
    stored.at_least_one("batch", batch, " sweep per launch")
    stored.check_motion_min(motion_min)
    keys = [boxes_key(s) for s in [gt] + names]
    sums = {s: new_sums() for s in names}
    with distenv.process_group() as (rank, world):
        ds = open_dataset(Path(data_dir), vis_name="", eval=False, fields=tuple(keys))
        mine = sharded_items(ds, whole_scenes=False)

        def loop():
            # the refusals, before anything touches the GPU
            held = {}
            for i in mine:
                where = "/".join(map(str, ds.index[i]))
                have = held[i] = stored.arrays(ds, i, keys)
                for s, k in zip([gt] + names, keys):
                    if k not in have:
                        raise KeyError(f"{k}: {where} holds no boxes of the name '{s}' (`python -m himo_amd.box_fit --res_names {s} ...` writes them)")
                    stored.check_box_rows(have[k], k, where, MAX_BOXES)
            if not mine:
                return
            ev = BoxEvaluator(min_iou=min_iou)
            for lo in range(0, len(mine), int(batch)):
                chunk = mine[lo:lo + int(batch)]
                for s in names:
                    g = [held[i][boxes_key(gt)] for i in chunk]
                    p = [held[i][boxes_key(s)] for i in chunk]
                    if pair_by == "iou":
                        res = ev.match(g, p)
                        for k in range(len(chunk)):
                            ma, _, ia = res.sweep(k)
                            tally(sums[s], g[k], p[k], ma, ia, motion_min)
                    else:
                        for k in range(len(chunk)):
                            ig, ip = label_pairs(g[k], p[k])
                            iou = ev.iou_pairs(g[k], p[k], np.stack([ig, ip], axis=1)).cpu().numpy()
                            ma, ia = np.full(len(g[k]), -1, dtype=np.int64), np.zeros((len(g[k]), 2))
                            ma[ig], ia[ig] = ip, iou
                            tally(sums[s], g[k], p[k], ma, ia, motion_min)

        distenv.run_shard(loop, "its share of the boxes", closing=(ds,))
        numbers = summary(distenv.gathered(sums), pair_by)
        distenv.report(rank, "\n".join([f"eval_box (box evaluation, v1; parity unpinned), min_iou {min_iou:g}:"] +
                                       [_table(s, numbers[s], gt, pair_by) for s in names]), numbers, json_path)
    return numbers


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="score the stored boxes_<name> of every sweep against those of the ground-truth flow: rotated IoU, "
                                             "greedy matching, TP / FP / FN at IoU 0.3, 0.5, 0.7 by speed and range (box evaluation, v1; parity "
                                             "unpinned: the reference has no such stage; timed on synthetic sweeps only, profiles/box_eval.txt; "
                                             "MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--gt", required=True, help="the name whose stored boxes are the ground truth (box_fit --res_names flow --label_key flow_instance_id)")
    ap.add_argument("--res_names", required=True, help="comma-separated names whose stored boxes are scored")
    ap.add_argument("--pair_by", default="iou", choices=("iou", "label"), help="'iou': greedy matching by BEV IoU (the default); 'label': the boxes "
                                                                              "of the same label id under both names")
    ap.add_argument("--min_iou", type=float, default=MIN_IOU, help="the smallest BEV IoU of a matched pair, 0 < min_iou <= 1")
    ap.add_argument("--batch", type=int, default=32, help="sweeps per launch")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the tables' numbers to PATH")
    ap.add_argument("--motion_min", type=float, default=MOTION_MIN, help="a ground-truth box slower than this per sweep is static, metres a sweep")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.gt, a.res_names, a.pair_by, a.min_iou, a.batch, a.json, a.motion_min)


if __name__ == "__main__":
    _cli()
