"""Cluster boxes: one oriented box -- a size, a heading and a velocity -- per cluster of labelled points (``python -m himo_amd.box_fit
--data_dir D --res_names raw,seflowpp_best --label_key ray_label`` writes ``<timestamp>/boxes_raw`` and ``<timestamp>/boxes_seflowpp_best``).
Everything this project scores is a per-instance shape error; a box fitted to the same cluster before and after compensation is the shape
feedback a user has where no ground truth ships: a vehicle at 30 m/s is about 3 m longer raw than compensated.

PARITY UNPINNED.  The reference has no such stage.  Like ``icpflow``, ``ground_seg``, ``raymap``, ``hdbscan``, ``rigid_refine`` and
``accumulate`` it follows the build's own written rule, below, and is checked against a numpy restatement of it
(``tests/boxfit_ref.py``), never against the reference.  No claim is made about the reference's numbers.  Timing: 0.67 ms per
120k-point synthetic sweep of 296 clusters, the one launch 0.10 ms of it, beside 0.39 ms for the DBSCAN call before it
(profiles/box_fit.txt); nothing has been tried on field data (the rule was tried on synthetic L-shapes only: tests/test_box_fit_cpu.py).

The method is the search-based L-shape fit: every heading of a fixed table is tried and the one that best explains the visible sides is
kept.  The criterion is the count of EDGE INLIERS, not the area: a LiDAR sees two sides of a car from one corner, and the minimum-area
rectangle of such an L is often a diagonal one (tests/test_box_fit_cpu.py shows both on the same draws).

The rule -- "cluster boxes, v1" (normative)
===========================================
Inputs per call: ``pts [N][pitch >= 3]`` float32 (raw or compensated: the caller decides), ``labels [N]`` int32 (0 = none, else 1..C),
optionally ``motion [N][3]`` float32, a displacement per sweep period, and a direction table ``dirs [K][2]`` int32, ``1 <= K <= 128``,
every ``|a|, |b| <= 4096`` and ``a*a + b*b > 0``.

Parameters (``BoxParams``, mirrored as ``himo_boxfit_params``, 16 bytes): ``scale`` float32, 128 sub-units per metre (admitted: finite,
> 0); ``tol_q`` int32, 13 sub-units, about 0.10 m (0..1024); ``min_points`` int32, 8 = ``ssl_label.MIN_PTS`` (>= 1); ``max_points``
int32, 8192 (``min_points``..2^20).  Anything else is refused before a launch, with no write.

The default table: ``directions(K=90)`` gives ``a_k = rint(4096 cos t_k)``, ``b_k = rint(4096 sin t_k)``, ``t_k = k (pi/2) / K``, computed
in float64 on the host, in Python.  The library never calls ``cos``.

A. Quantisation.  A row is USABLE iff its label is > 0, its x, y and z are finite, and ``|x*scale|`` and ``|y*scale|``, each ONE float32
   multiplication, are below 4194304.  Then ``X = (int)floorf(x*scale)``, ``Y`` likewise.  The cluster's rows are its usable rows; ``n``
   is their count.
B. State, tested in this order: TOO_FEW (1) if ``n < min_points``; TOO_LARGE (2) if ``n > max_points`` or ``Xmax - Xmin >= 16384`` or
   ``Ymax - Ymin >= 16384``; FITTED (0) otherwise.  Only FITTED clusters run C-E; the others write their state and ``n``, zeros elsewhere.
C. Per direction k, all integers: ``X' = X - Xmin``, ``Y' = Y - Ymin``; ``u = a X' + b Y'``, ``v = -b X' + a Y'`` (every value fits int32
   under rule B); ``umin, umax, vmin, vmax`` over the cluster; ``d_i = min(u_i - umin, umax - u_i, v_i - vmin, vmax - v_i)``; a row is an
   EDGE INLIER iff ``d_i <= tol_q << 12``; ``S_k`` is the inlier count, ``A_k = (umax - umin) (vmax - vmin)`` in int64.
D. Choice: the k with the largest ``S_k``; ties go to the smaller ``A_k``; remaining ties to the lowest k.
E. Box, in float64, every operation rounding on its own (``himo_amd/csrc/boxfit.hip`` is built with ``-ffp-contract=off``; only sqrt
   and division appear): ``n2 = (double)(a*a + b*b)``, ``r = sqrt(n2)``; ``su = (double)(umin + umax) * 0.5``, ``sv`` likewise;
   ``px = ((double)a*su - (double)b*sv) / n2``, ``py = ((double)b*su + (double)a*sv) / n2``; ``cx = (((double)Xmin + px) + 0.5) /
   (double)scale``, ``cy`` likewise; ``eu = (double)(umax - umin) / (r * (double)scale)``, ``ev`` likewise; ``zmin``, ``zmax`` the float32
   minimum and maximum of z over the cluster (-0 orders below +0); ``cz = ((double)zmin + (double)zmax) * 0.5``, ``h = (double)zmax -
   (double)zmin``.
F. Motion.  With ``motion`` the box carries the float64 mean of the cluster's motion rows; rows with a non-finite motion value are left
   out of both the sum and its count (no row left: zeros).  The ORDER of the sum is not part of the rule: the device takes it in a fixed
   shape with the ``blockops.h`` sums (the same bytes on every run), the restatement in row order; they agree to rounding.  Without
   ``motion`` the mean is zeros.
G. Outputs of the entry point: ``info int32 [C][12]`` = state, n, k, S_k, Xmin, Ymin, umin, umax, vmin, vmax, motion row count, 0;
   ``box float64 [C][10]`` = cx, cy, cz, eu, ev, h, mx, my, mz, 0.
H. Host glue (Python, float64, on C rows, no point data): ``l = max(eu, ev)``, ``w = min(eu, ev)``; ``yaw0 = t_k``, plus pi/2 when
   ``ev > eu``.  If a motion was given and ``hypot(mx, my) >= motion_min`` (0.05 m, as ``--motion_min`` of ``accumulate``): the heading
   is ``yaw0`` or ``yaw0 + pi``, the one whose dot product with ``(mx, my)`` is non-negative -- ``yaw0 + pi`` iff ``cos(yaw0) mx +
   sin(yaw0) my < 0``, so ``yaw0`` when the two products are equal -- and the box is MOVING.  ``yaw`` is wrapped into (-pi, pi].  The
   final row per FITTED cluster is float32 ``[12]`` = x, y, z, l, w, h, yaw, vx, vy, vz, label id, n; ``v`` is the mean motion divided
   by ``sensor_dt``.  (float32 holds an id exactly up to 2^24; ``BoxResult.ids`` holds every id exactly.)

Not part of v1: a closeness or variance criterion, a refinement between table angles, a 3-D rotation, ground-plane snapping of z, box
association over time, rotated IoU or AP, boxes drawn by ``view``.

Python sequences launches and owns no arithmetic on point data.  ``fit_labelled`` has one host wait per sweep: the cluster count, the
clusters' row ranges and their ids, read through pinned memory behind an event (as ``RigidRefine.refine`` reads them).
``BoxFitter.fit`` compacts the ids with ``torch.unique`` first, which waits on its own (the size of its result depends on the data):
two waits for arbitrary ids, both inside the measured time; the result's host copies are made when asked for, a further wait.  There
is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .stored import fmt, ratio

FITTED, TOO_FEW, TOO_LARGE = 0, 1, 2
STATE_NAMES = ("fitted", "too few", "too large")
MAX_DIRS = 128
MOTION_MIN = 0.05                   # rule H: the project's static threshold [m a sweep] (accumulate's --motion_min)
SENSOR_DT = 0.1


class _CParams(ctypes.Structure):
    """mirror of ``himo_boxfit_params`` (include/himo_amd.h)"""
    _fields_ = [("scale", ctypes.c_float), ("tol_q", ctypes.c_int32), ("min_points", ctypes.c_int32), ("max_points", ctypes.c_int32)]


@dataclass(frozen=True)
class BoxParams:
    """the parameters of "cluster boxes, v1"; refuses what the rule does not admit before anything is launched"""
    scale: float = 128.0
    tol_q: int = 13
    min_points: int = 8
    max_points: int = 8192

    def __post_init__(self):
        v = self.scale
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
            raise ValueError(f"BoxParams.scale={v!r}: a finite, positive number")
        with np.errstate(all="ignore"):
            as32 = float(np.float32(v))
        if not math.isfinite(as32) or not as32 > 0:
            raise ValueError(f"BoxParams.scale={v!r}: not a positive float32")
        for name in ("tol_q", "min_points", "max_points"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"BoxParams.{name}={v!r}: an integer")
        if not 0 <= self.tol_q <= 1024:
            raise ValueError(f"BoxParams.tol_q={self.tol_q}: 0..1024")
        if self.min_points < 1:
            raise ValueError(f"BoxParams.min_points={self.min_points}: at least 1")
        if not self.min_points <= self.max_points <= 1 << 20:
            raise ValueError(f"BoxParams.max_points={self.max_points}: min_points..2^20")

    def c_struct(self) -> _CParams:
        return _CParams(self.scale, int(self.tol_q), int(self.min_points), int(self.max_points))


def angles(K: int = 90) -> np.ndarray:
    """``t_k = k (pi/2) / K``, float64 [K]: the headings of the default table (rule H reads them)"""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= MAX_DIRS:
        raise ValueError(f"K={K!r}: 1..{MAX_DIRS} directions")
    return np.arange(int(K), dtype=np.float64) * ((math.pi / 2) / int(K))


def directions(K: int = 90) -> np.ndarray:
    """the default direction table, int32 [K, 2]: ``rint(4096 cos t_k), rint(4096 sin t_k)`` in float64 on the host"""
    t = angles(K)
    return np.stack([np.rint(4096.0 * np.cos(t)), np.rint(4096.0 * np.sin(t))], axis=1).astype(np.int32)


def check_directions(dirs) -> np.ndarray:
    """``dirs`` as the C-contiguous int32 [K, 2] table the entry point reads; refuses what the rule does not admit"""
    d = np.asarray(dirs)
    if d.ndim != 2 or d.shape[1] != 2 or not 1 <= d.shape[0] <= MAX_DIRS or d.dtype.kind not in "iu":
        raise ValueError(f"dirs: an integer table [K, 2] with 1 <= K <= {MAX_DIRS}, not {d.dtype} {d.shape}")
    d = d.astype(np.int64)
    if (np.abs(d) > 4096).any() or ((d * d).sum(axis=1) == 0).any():
        raise ValueError("dirs: every |a|, |b| <= 4096 and a*a + b*b > 0")
    return np.ascontiguousarray(d, dtype=np.int32)


def glue(info: np.ndarray, box: np.ndarray, ids, theta: np.ndarray, with_motion: bool, motion_min: float = MOTION_MIN,
         sensor_dt: float = SENSOR_DT):
    """Rule H on host copies: (rows float32 [F, 12], moving bool [F]) of the FITTED clusters, in cluster order."""
    rows, moving = [], []
    for c in np.flatnonzero(info[:, 0] == FITTED):
        cx, cy, cz, eu, ev, h, mx, my, mz = (float(v) for v in box[c, :9])
        yaw, mov = float(theta[info[c, 2]]) + (math.pi / 2 if ev > eu else 0.0), False
        if with_motion and math.hypot(mx, my) >= motion_min:
            mov = True
            if math.cos(yaw) * mx + math.sin(yaw) * my < 0:
                yaw += math.pi
        yaw = math.fmod(yaw, 2 * math.pi)
        if yaw > math.pi:
            yaw -= 2 * math.pi
        elif yaw <= -math.pi:
            yaw += 2 * math.pi
        rows.append([cx, cy, cz, max(eu, ev), min(eu, ev), h, yaw, mx / sensor_dt, my / sensor_dt, mz / sensor_dt, float(ids[c]), float(info[c, 1])])
        moving.append(mov)
    return np.asarray(rows, dtype=np.float32).reshape(-1, 12), np.asarray(moving, dtype=bool)


def fit_labelled(pts, labels, n_clusters: int, dirs, params: BoxParams | None = None, motion=None, upper_bound: bool = False, extra=None):
    """Rules A-G through ``himo_boxfit`` on the current stream: ``pts`` device float32 (N, >= 3) rows (any row pitch), ``labels`` device
    int32 [N] (0 and anything outside 1..C: none), ``motion`` None or device float32 [N, 3] -> (info int32 [C, 12], box float64
    [C, 10]) device tensors, and what the one host wait read besides the row ranges.  ``n_clusters`` is C; with ``upper_bound`` it is
    only the most there can be and C is the greatest label, read in the one wait.  ``extra``: a device integer vector to bring to the
    host in the same read (``BoxFitter.fit`` passes the ids).  Sorts the rows by label as ``RigidRefine.refine`` does; one host
    wait, through pinned memory behind an event."""
    import torch
    from . import _lib
    from .icpflow import pinned_words
    lib, P = _lib.load(), _lib.ptr
    params = params if params is not None else BoxParams()
    table = check_directions(dirs)
    dev = pts.device
    if pts.dim() != 2 or pts.shape[1] < 3 or pts.dtype != torch.float32 or (pts.shape[0] > 0 and pts.stride(1) != 1) or \
            (pts.shape[0] > 1 and pts.stride(0) < 3):                # (an empty tensor's strides say nothing)
        raise ValueError(f"points are float32 rows of x, y, z[, ...], not {pts.dtype} {tuple(pts.shape)} with strides {pts.stride()}")
    n = int(pts.shape[0])
    pitch = int(pts.stride(0)) if n > 1 else int(pts.shape[1])
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    if labels.shape != (n,):
        raise ValueError(f"labels {tuple(labels.shape)} are not row-aligned with the {n} points")
    if motion is not None:
        motion = motion.to(device=dev, dtype=torch.float32).contiguous()
        if motion.shape != (n, 3):
            raise ValueError(f"motion is [{n}, 3], not {tuple(motion.shape)}")
    top = int(n_clusters)                                          # the most clusters there can be: sizes the device-side tables
    if top < 0:
        raise ValueError(f"n_clusters={n_clusters}: not negative")
    # the labelled rows sorted by label (stable: ascending row inside a cluster) and every label's first sorted row
    lab = torch.where((labels > 0) & (labels <= top), labels, torch.zeros_like(labels))
    order = torch.argsort(torch.where(lab > 0, lab, torch.iinfo(torch.int32).max), stable=True)
    sizes = torch.bincount(lab, minlength=top + 1)[1:top + 1]
    offsets = torch.zeros(top + 1, dtype=torch.int64, device=dev)
    if top:
        torch.cumsum(sizes, 0, out=offsets[1:])
    count = (lab.max().to(torch.int64) if n else torch.zeros((), dtype=torch.int64, device=dev)).reshape(1)
    words = [count, offsets] + ([extra.to(torch.int64).reshape(-1)] if extra is not None else [])
    total = sum(int(w.numel()) for w in words)
    host = pinned_words(total)
    host[:total].copy_(torch.cat(words), non_blocking=True)
    landed = torch.cuda.Event()
    landed.record(torch.cuda.current_stream(dev))
    landed.synchronize()                                            # the sweep's one host wait
    C = int(host[0]) if upper_bound else top
    h_off = host[1:1 + C + 1].numpy().copy()
    brought = host[2 + top:total].numpy().copy() if extra is not None else None
    nc = int(h_off[C])
    info = torch.zeros((C, 12), dtype=torch.int32, device=dev)
    box = torch.zeros((C, 10), dtype=torch.float64, device=dev)
    if C:
        ws = torch.empty(max(int(lib.himo_boxfit_workspace_bytes(nc, C, len(table))), 16), dtype=torch.uint8, device=dev)
        c_params = params.c_struct()
        with torch.cuda.device(dev):
            st = lib.himo_boxfit(n, P(pts), pitch, P(lab), nc, P(order), C, h_off.ctypes.data, P(offsets), P(motion), table.ctypes.data,
                                 len(table), ctypes.addressof(c_params), P(info), P(box), P(ws), ws.numel(), _lib.stream_handle())
        _lib.check(st, "himo_boxfit")
    return info, box, brought


class BoxResult:
    """What ``BoxFitter.fit`` returns.  ``info`` (int32 [C, 12]) and ``box`` (float64 [C, 10]) are rule G's outputs, ``ids`` (int64 [C])
    the original id of every cluster, ``rows`` (float32 [F, 12]) and ``moving`` (bool [F]) rule H's over the FITTED clusters, ``labels``
    (int64 [F]) their ids.  Host copies, made when first asked for (that is a wait of its own); ``device_info`` / ``device_box`` are
    the device tensors."""

    def __init__(self, info, box, ids, theta, with_motion, motion_min, sensor_dt):
        self.device_info, self.device_box, self.ids = info, box, ids
        self._glue = (theta, with_motion, motion_min, sensor_dt)
        self._host = None

    def _copies(self):
        if self._host is None:
            info, box = self.device_info.cpu().numpy(), self.device_box.cpu().numpy()
            rows, moving = glue(info, box, self.ids, *self._glue)
            self._host = (info, box, rows, moving)
        return self._host

    info = property(lambda self: self._copies()[0])
    box = property(lambda self: self._copies()[1])
    rows = property(lambda self: self._copies()[2])
    moving = property(lambda self: self._copies()[3])

    @property
    def labels(self) -> np.ndarray:
        return self.ids[self.info[:, 0] == FITTED]


class BoxFitter:
    """``BoxFitter(device, params, K).fit(pts, labels, motion=None)`` -> a ``BoxResult`` (module docstring).  ``labels`` may hold
    arbitrary integer ids such as ``flow_instance_id`` (0 = none): they are compacted to 1..C in ascending order and come back in
    column 10 of the rows and, exactly, in ``BoxResult.ids``.  There is no CPU path."""

    def __init__(self, device=None, params: BoxParams | None = None, K: int = 90, motion_min: float = MOTION_MIN, sensor_dt: float = SENSOR_DT):
        from . import _lib
        self.params = params if params is not None else BoxParams()
        self.dirs, self.theta = directions(K), angles(K)
        if not (math.isfinite(motion_min) and motion_min >= 0):
            raise ValueError(f"motion_min={motion_min}: finite and >= 0")
        if not (math.isfinite(sensor_dt) and sensor_dt > 0):
            raise ValueError(f"sensor_dt={sensor_dt}: finite and > 0")
        self.motion_min, self.sensor_dt = float(motion_min), float(sensor_dt)
        self.lib = _lib.load()
        if self.lib.himo_abi_sizeof(b"himo_boxfit_params") != ctypes.sizeof(_CParams):
            raise ImportError("himo_boxfit_params: the library's layout is not this binding's; rebuild libhimo_amd.so")
        self.device = device if device is not None else _lib.require_gpu()

    def fit(self, pts, labels, motion=None) -> BoxResult:
        import torch
        dev = self.device
        up = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))       # noqa: E731
        p = up(pts).to(device=dev, dtype=torch.float32)
        if p.dim() != 2 or p.shape[1] < 3:
            raise ValueError(f"points are rows of x, y, z[, ...], not {tuple(p.shape)}")
        if p.stride(1) != 1 or (p.shape[0] > 1 and p.stride(0) < 3):
            p = p.contiguous()
        if not isinstance(labels, torch.Tensor):                      # (uint32 ids: through int64, which holds every one of them)
            labels = np.asarray(labels)
            if labels.dtype.kind not in "iu":
                raise ValueError(f"labels are one integer id per row, not {labels.dtype}")
            labels = labels.astype(np.int64)
        raw = up(labels)
        if raw.dtype.is_floating_point or raw.dtype == torch.bool or raw.dim() != 1 or raw.shape[0] != p.shape[0]:
            raise ValueError(f"labels are one integer id per row, not {raw.dtype} {tuple(raw.shape)} for {p.shape[0]} rows")
        ids = raw.to(device=dev).to(torch.int64)
        uniq, inverse = torch.unique(ids, return_inverse=True)       # ascending
        nonzero = uniq != 0
        rank = torch.cumsum(nonzero.to(torch.int64), 0) * nonzero     # 0 stays 0, the others 1..C in ascending order
        compact = rank[inverse].to(torch.int32)
        mo = None if motion is None else up(motion).to(device=dev, dtype=torch.float32)
        in_order = uniq[torch.argsort((~nonzero).to(torch.int8), stable=True)]      # the C ids in ascending order, then the 0 if there is one
        info, box, brought = fit_labelled(p, compact, int(uniq.numel()), self.dirs, self.params, mo, upper_bound=True, extra=in_order)
        C = int(info.shape[0])
        return BoxResult(info, box, brought[:C].astype(np.int64), self.theta, motion is not None, self.motion_min, self.sensor_dt)


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def boxes_key(name: str) -> str:
    return f"boxes_{name}"


def new_totals() -> dict:
    return {"boxes": 0, "moving": 0, "sum_l_moving": 0.0, "sum_w_moving": 0.0}


def new_against() -> dict:
    zero = lambda: {"pairs": 0, "sum_dl": 0.0, "sum_dw": 0.0, "sum_centre": 0.0, "sum_yaw_deg": 0.0}      # noqa: E731
    return {"all": zero(), "moving": zero()}


def tally(totals: dict, rows: np.ndarray, moving: np.ndarray) -> None:
    """add one sweep's boxes to a result's running totals"""
    totals["boxes"] += int(len(rows))
    totals["moving"] += int(moving.sum())
    totals["sum_l_moving"] += float(np.sum(rows[moving, 3], dtype=np.float64))
    totals["sum_w_moving"] += float(np.sum(rows[moving, 4], dtype=np.float64))


def tally_against(acc: dict, rows, moving, labels, rows_b, moving_b, labels_b) -> None:
    """``--against``: the boxes of one sweep against those of the same labels under another name (labels FITTED in both; "moving":
    MOVING in both)"""
    _, ia, ib = np.intersect1d(labels, labels_b, assume_unique=True, return_indices=True)
    a, b = rows[ia].astype(np.float64), rows_b[ib].astype(np.float64)
    both = moving[ia] & moving_b[ib]
    fold = np.abs(np.degrees(a[:, 6] - b[:, 6])) % 90.0
    fold = np.minimum(fold, 90.0 - fold)                            # [0, 45] degrees: a box turned by 90 degrees is the same rectangle
    centre = np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1])
    for key, sel in (("all", np.ones(len(ia), dtype=bool)), ("moving", both)):
        t = acc[key]
        t["pairs"] += int(sel.sum())
        t["sum_dl"] += float(np.abs(a[sel, 3] - b[sel, 3]).sum())
        t["sum_dw"] += float(np.abs(a[sel, 4] - b[sel, 4]).sum())
        t["sum_centre"] += float(centre[sel].sum())
        t["sum_yaw_deg"] += float(fold[sel].sum())


def summary(totals: dict, against: dict | None, against_name: str | None) -> dict:
    """the numbers of the table and of ``--json``, per result"""
    out = {}
    for name, t in totals.items():
        out[name] = {"boxes": t["boxes"], "moving": t["moving"], "mean_l_moving": ratio(t["sum_l_moving"], t["moving"]),
                     "mean_w_moving": ratio(t["sum_w_moving"], t["moving"])}
        if against is not None:
            out[name]["against"] = {"name": against_name}
            for key, a in against[name].items():
                out[name]["against"][key] = {"pairs": a["pairs"], "mean_dl": ratio(a["sum_dl"], a["pairs"]), "mean_dw": ratio(a["sum_dw"], a["pairs"]),
                                             "mean_centre": ratio(a["sum_centre"], a["pairs"]), "mean_yaw_deg": ratio(a["sum_yaw_deg"], a["pairs"])}
    return out


def _table(numbers: dict) -> str:
    lines = []
    for name, r in numbers.items():
        line = f"{name}: {r['boxes']} boxes, {r['moving']} moving, mean l {fmt(r['mean_l_moving'])} m, mean w {fmt(r['mean_w_moving'])} m (moving)"
        if "against" in r:
            for key in ("all", "moving"):
                a = r["against"][key]
                line += (f"; against {r['against']['name']} ({key}, {a['pairs']} pairs): |dl| {fmt(a['mean_dl'])} m, |dw| {fmt(a['mean_dw'])} m, "
                         f"centre {fmt(a['mean_centre'])} m, yaw {fmt(a['mean_yaw_deg'], '.2f')} deg")
        lines.append(line)
    return "\n".join(lines)


def sweep_boxes(fitter: BoxFitter, engine, frame: dict, name: str, label_key: str, motion_key: str | None, cluster: str = "dbscan",
                min_cluster_size: int | None = None, min_samples: int | None = None) -> BoxResult:
    """The boxes of one sweep under one name: the points compensated by the stored flow ``name`` through ``CompDisEngine`` (``raw``: as
    recorded), the motion the stored flow ``name`` (``raw``: ``motion_key``, or none) less the ego motion (``himo_accum_motion``), the
    labels the stored ``label_key`` or, for ``cluster``, a clustering of the compensated non-ground in-range points."""
    import torch
    from .accumulate import device_rows, flow_motion
    dev = fitter.device
    pc0 = device_rows(frame["pc0"], dev)
    if name == "raw":
        pts = pc0
    else:
        flow = torch.from_numpy(np.ascontiguousarray(frame[name], dtype=np.float32)).to(dev)
        dt = torch.from_numpy(np.ascontiguousarray(frame["lidar_dt"], dtype=np.float32)).to(dev)
        pts = engine.run_frame(pc0, flow, dt, frame["pose0"], frame["pose1"], refined=True)[1]
    mkey = motion_key if name == "raw" else name
    motion = flow_motion(pc0, frame[mkey], frame["pose0"], frame["pose1"]) if mkey else None
    if label_key == "cluster":
        from .seflow.ssl_label import EPS, HDB_MIN_CLUSTER, HDB_MIN_SAMPLES, MIN_PTS, RANGE_NET, cluster_points
        xyz = pts[:, :3]
        skip = torch.from_numpy(np.ascontiguousarray(frame["gm0"]).astype(bool)).to(dev) | ~torch.isfinite(xyz).all(dim=1) | \
            ~(xyz[:, :2].abs().amax(dim=1) <= RANGE_NET)
        ids, _ = cluster_points(xyz.contiguous(), skip, cluster, EPS, MIN_PTS, HDB_MIN_CLUSTER if min_cluster_size is None else min_cluster_size,
                                HDB_MIN_SAMPLES if min_samples is None else min_samples)
    else:
        ids = np.asarray(frame[label_key])
    return fitter.fit(pts, ids, motion)


def main(data_dir: str, res_names, label_key: str, cluster: str = "dbscan", against: str | None = None, json_path: str | None = None,
         overwrite: bool = False, params: BoxParams | None = None, K: int = 90, motion_key: str | None = None,
         motion_min: float = MOTION_MIN, min_cluster_size: int | None = None, min_samples: int | None = None) -> dict:
    """The program: for every sweep of ``data_dir`` and every name of ``res_names``, ``<timestamp>/boxes_<name>`` float32 [F, 12] (rule
    H's rows) into the scene file -- the writer ``raymap.label_scene`` uses; for this package's npz container, into the sweep's npz.
    An existing ``boxes_<name>`` is refused unless ``overwrite``.  ``raw`` has no stored flow: its boxes take their motion from
    ``motion_key`` (default: the first stored name of ``res_names``; none when there is none, and no box is MOVING then).  Under
    ``torchrun`` whole scenes per rank (h5).  Returns what ``--json`` writes: {name: {"boxes", "moving", "mean_l_moving",
    "mean_w_moving"[, "against"]}} over every rank."""
    from . import distenv, stored
    from .dataset import NpzDataset, open_dataset
    from .seflow.ssl_label import CLUSTERINGS
    from .sweeps import sharded_items
    names = stored.result_names(res_names, raw_ok=True)
    if not label_key:
        raise ValueError("label_key: a stored integer key (ray_label, flow_instance_id, ...) or 'cluster'")
    if against and label_key == "cluster":
        raise ValueError("--against with --label_key cluster: the clusters are made per name, so no label names the same object under two names")
    if against and against not in names:
        raise ValueError(f"--against {against}: not one of --res_names {','.join(names)}")
    if cluster not in CLUSTERINGS:
        raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
    params = params if params is not None else BoxParams()
    angles(K)
    flows_of = [s for s in names if s != "raw"]
    if motion_key == "raw":
        raise ValueError("--motion_key raw: 'raw' is the zero-motion key, not a stored flow")
    if motion_key is None and "raw" in names and flows_of:
        motion_key = flows_of[0]
    flows = list(dict.fromkeys(flows_of + ([motion_key] if motion_key and "raw" in names else [])))
    root = Path(data_dir)
    needs = ["gm0"] if label_key == "cluster" else [label_key]
    keys = [boxes_key(s) for s in names]
    sums = {"totals": {s: new_totals() for s in names}, "against": {s: new_against() for s in names} if against else None}
    with distenv.process_group() as (rank, world):
        ds = open_dataset(root, vis_name=flows, eval=False, fields=tuple(["pc0", "pose0", "pose1", "lidar_dt"] + needs + flows))
        npz = isinstance(ds, NpzDataset)
        mine = sharded_items(ds, whole_scenes=not npz)              # whole scenes per rank: every scene file has one writer

        def loop():
            # the refusals, before anything touches the GPU or a file is written
            sink = stored.KeySink(ds, root, f"writing '{keys[0]}' into the scene files of {data_dir}")
            for i in mine:
                where = "/".join(map(str, ds.index[i]))
                have = stored.present(ds, i, flows + needs + keys)
                for s in flows:
                    if s not in have:
                        raise KeyError(f"{s}: {where} holds no result of that name (--res_names / --motion_key name stored flows; 'raw' needs none)")
                if label_key == "cluster" and "gm0" not in have:
                    raise KeyError("gm0: --label_key cluster needs the sweep's ground mask (`python -m himo_amd.ground_seg` writes it)")
                if label_key != "cluster" and label_key not in have:
                    raise KeyError(f"{label_key}: {where} holds no such label (`python -m himo_amd.raymap` writes ray_label)")
                if label_key != "cluster":
                    count_key = "pc0" if npz else "lidar_dt"        # a sweep's number of points: the cheapest array that has one row each
                    got = stored.arrays(ds, i, (label_key, count_key))
                    stored.check_point_labels(got[label_key], label_key, where, rows=len(got[count_key]))
                done = [k for k in keys if k in have]
                if done and not overwrite:
                    raise FileExistsError(f"{where} already holds '{done[0]}': pass --overwrite to replace it")
            if not mine:
                return
            from .compdis import CompDisEngine
            fitter = BoxFitter(params=params, K=K, motion_min=motion_min)
            engine = CompDisEngine()
            for i in mine:
                f = ds[i]
                got = {}
                for s in names:
                    r = got[s] = sweep_boxes(fitter, engine, f, s, label_key, motion_key, cluster, min_cluster_size, min_samples)
                    tally(sums["totals"][s], r.rows, r.moving)
                    sink.put(f["scene_id"], f["timestamp"], boxes_key(s), r.rows)
                if against:
                    b = got[against]
                    for s in names:
                        tally_against(sums["against"][s], got[s].rows, got[s].moving, got[s].labels, b.rows, b.moving, b.labels)
            sink.close()                                            # (on success only: a failed run leaves its last scene as it was)

        distenv.run_shard(loop, "its share of the boxes", closing=(ds,))
        total = distenv.gathered(sums)
        numbers = summary(total["totals"], total["against"], against)
        distenv.report(rank, f"box_fit (cluster boxes, v1; parity unpinned), labels '{label_key}':\n{_table(numbers)}", numbers, json_path)
    return numbers


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="fit one oriented box per cluster of every sweep and store them as <timestamp>/boxes_<name> (cluster "
                                             "boxes, v1; parity unpinned: the reference has no such stage; timed on synthetic sweeps only, profiles/box_fit.txt; "
                                             "MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--res_names", required=True, help="comma-separated: 'raw' (the points as recorded) and / or stored flows to compensate by")
    ap.add_argument("--label_key", required=True, help="a stored integer label per point (ray_label, flow_instance_id, ...; 0 = none), or "
                                                       "'cluster': cluster the compensated non-ground in-range points (needs ground_mask)")
    ap.add_argument("--cluster", default="dbscan", help="--label_key cluster: 'dbscan' (the default) or 'hdbscan'")
    ap.add_argument("--min_cluster_size", type=int, default=None, help="--cluster hdbscan: the smallest cluster (ssl_label.HDB_MIN_CLUSTER)")
    ap.add_argument("--min_samples", type=int, default=None, help="--cluster hdbscan: the core neighbour count, 1..32 (ssl_label.HDB_MIN_SAMPLES)")
    ap.add_argument("--against", default=None, metavar="NAME", help="compare every result's boxes with those of NAME, label by label "
                                                                    "(refused with --label_key cluster)")
    ap.add_argument("--motion_key", default=None, help="the stored flow the boxes of 'raw' take their motion from (default: the first stored name)")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the table's numbers to PATH")
    ap.add_argument("--overwrite", action="store_true", help="replace existing boxes_<name> instead of refusing")
    d = BoxParams()
    ap.add_argument("--directions", type=int, default=90, help=f"table size K over a quarter turn, 1..{MAX_DIRS}")
    ap.add_argument("--tol_q", type=int, default=d.tol_q, help="edge-inlier tolerance, sub-units of 1 / scale metres")
    ap.add_argument("--min_points", type=int, default=d.min_points, help="fewer usable points: no box")
    ap.add_argument("--max_points", type=int, default=d.max_points, help="more usable points: no box")
    ap.add_argument("--motion_min", type=float, default=MOTION_MIN, help="a box whose mean motion is at least this is moving, metres a sweep")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.res_names, a.label_key, a.cluster, a.against, a.json, a.overwrite,
         BoxParams(tol_q=a.tol_q, min_points=a.min_points, max_points=a.max_points), a.directions, a.motion_key, a.motion_min,
         a.min_cluster_size, a.min_samples)


if __name__ == "__main__":
    _cli()
