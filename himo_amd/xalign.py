"""Cross-sensor alignment: the velocity of an object from the capture times inside ONE sweep (``python -m himo_amd.xalign --data_dir D
--label_key ray_label`` writes it as the flow key ``xalign``).  The distortion this project removes is a multi-LiDAR effect: several
sensors see the same vehicle at different instants of one sweep, so its recorded points form several displaced copies, ``r_i = P + v
tau_i``.  The ``v`` that lays the copies on top of one another is the object's velocity -- no second sweep, no network, no training.  It
is the one compensation that works on the first sweep of a drive, on a logger that dropped the neighbouring sweeps, or on an object seen
once, and it is the second route the reference's README names ("dynamic segmentation + ICP alignment across LiDARs", of which it says
that it "has not been shown to work in practice") and ships no program for.  The chain is ``ground_seg -> raymap -> xalign``;
``eval_xsensor`` measures what it gained.

PARITY UNPINNED.  The reference has no such stage.  Like ``eval_xsensor``, ``box_fit`` and ``track`` it follows the build's own written
rule, below, and is checked against a numpy restatement of it (``tests/xalign_ref.py``), never against the reference.  Timing: 9.3 ms per
call of 32 synthetic 120k-point sweeps in 9600 clusters and 8.7 ms for one sweep alone (the workgroup of the largest cluster sets the
time), 11.0 x the ``himo_xsensor`` call over the same clusters, 1.03 ms per pass (profiles/xalign.txt); nothing has been tried on
field data.  What the rule does on synthetic vehicles (``tests/xsensor_ref.py::drive``, seeds 0..3, 600 points, three sensors 33 ms apart, 0.02
m noise; tests/test_xalign_cpu.py): no static vehicle and no vehicle at 2 m/s is ALIGNED (their ``v`` is exactly zero); every vehicle at
5, 10, 20, 30 and 35 m/s is ALIGNED, the worst ``|v - v_true|`` 0.47 m/s at 5 m/s, 0.80 at 10, 0.49 at 20, 0.37 at 30 and 0.32 at 35 (0.8
m/s is 5 cm over the 66 ms between the first and last sensor, where the raw displacement at 35 m/s is 2.3 m); compensated by the written
flow, the cross-sensor distance of these vehicles is at most 1.0003 of what the true flow leaves (0.111 m against 0.299 m raw at 35 m/s;
static vehicles sit at 0.112 m).  LIMITS.  A vehicle is unreliable below about 600 points: at 300 the float64 prototype was wrong by up to
11.8 m/s at 10 m/s, hence ``min_points = 600``.  With a third of each outer sensor's view cut away (a harsh partial overlap) the prototype
stayed within 1.1 m/s at 600 points and 1 m/s bins, but at 150-300 points, or with coarser bins, it ACCEPTED a few velocities that were
wrong by 50 m/s: the acceptance test of rule F does not catch a wrong alignment that happens to overlap well.  Field data will be worse:
clusters merge objects and the overlap is partial.  Plain nearest-neighbour ICP from ``v = 0`` does not work (the points slide along the
vehicle's side); the vote of rule C is what makes it work and is not optional.

The rule -- "cross-sensor alignment, v1" (normative)
===================================================
Inputs per call, exactly those of ``himo_xsensor``: ``pts [N][pitch >= 3]`` float32, ``labels [N]`` int32 (0 = none, else 1..C),
``group [N]`` uint8 (the loader's ``lidar_id``), ``tau [N]`` float32 (the loader's ``lidar_dt``, the CAPTURE TIME; required).  An object
with velocity ``v`` is recorded at ``r_i = P + v tau_i``.  The labelled rows sorted by label; the clusters of several sweeps laid end to
end in one call.

Parameters (``XAlignParams``, mirrored as ``himo_xalign_params``, 52 bytes; anything else is refused before a launch, with no write):
``min_group`` 5 (>= 1); ``min_points`` 600 (>= 2); ``max_points`` 4096 (``min_points``..16384); ``v_max`` 60 m/s (finite, > 0, <= 1024);
``bin`` 1.0 m/s (finite, > 0; the table side ``nb = 2 ceil(v_max / bin) + 1`` must give ``nb^2 <= 15360``, the cells that fit in LDS:
``nb <= 123``); ``tau_min`` 0.010 s, ``sigma`` 0.3 m, ``trunc`` 2.0 m (each finite, > 0, <= 1024); ``z_gate`` 0.2 m (finite, > 0);
``iters`` 30 (1..100, and ``iters * max_points^2 <= 2^32``: one workgroup walks a cluster, so its work is bounded); ``tol`` 0.02 m/s and
``static_speed`` 0.5 m/s (finite, >= 0); ``min_gain`` 0.1 (finite, in [0, 1)).  The float parameters are float32; where the rule says
float64 they are widened.

A-B. Usable rows, live groups and the states TOO_FEW (1), TOO_LARGE (3) and ONE_SENSOR (2) are those of ``eval_xsensor`` rules A-B, word
   for word and in the same order (``himo_amd/csrc/xsensor_rows.h`` states them once for both kernels; ``tau`` is its ``dt``).  One state
   is added, tested after them: NO_BASELINE (4) iff ``max t_g - min t_g < tau_min`` over the live groups -- no two live groups have mean
   times at least ``tau_min`` apart -- with ``t_g = (sum of q24(tau clipped to +-1024 s) over the group's usable rows) / (2^24 n_g)`` in
   float64, ``q24(x) = llrint(x 2^24)``.  A cluster in one of these states writes its state, ``n`` (NO_BASELINE: also the live mask and
   the rows), ``v = 0`` and zeros elsewhere.  A cluster that ends as NO_BASELINE later (rule C: no vote; rule D: ``A == 0``) writes ``v =
   0`` and zero sums too, but keeps in ``info`` what it had counted by then: the votes and the winning bin, and after ``A == 0`` the
   iterations used and the pairs of the last one.  Only the usable rows of live groups take part in C-F: the ROWS.
C. Vote.  Every pair of rows (i, j) of different live groups with group(i) < group(j), ``|tau_i - tau_j| >= tau_min`` and ``|z_i - z_j|
   < z_gate`` (both differences and tests in float32) votes for the planar velocity ``(dx / dtau, dy / dtau)``, float64 from the float32
   inputs.  The bin per axis is ``floor(v / bin + nb / 2)`` (``nb`` is odd: bin ``(nb - 1) / 2`` is centred on zero); a vote outside the
   table is dropped; counts are integers.  The score of a bin is the sum of the counts over its 3 x 3 neighbourhood, clipped at the
   table's edge.  The start ``v_0`` is the centre ``((b - (nb - 1) / 2) bin`` per axis) of the bin with the greatest score; ties go to
   the smallest flat index ``bx nb + by``.  A table with no vote gives NO_BASELINE.  ``v_z = 0`` throughout v1.
D. Iteration k = 0 .. iters - 1.  The moved rows are ``x_i = r_x - (float32)v_x tau_i``, y likewise, z as recorded: float32, every
   operation rounding on its own (``xalign.hip`` is built with ``-ffp-contract=off``).  For each row, the nearest moved row of ANOTHER
   live group by ``d2 = (dx*dx + dy*dy) + dz*dz`` in float32 -- the minimum of the 64-bit key ``(bits of d2 << 32) | sorted row``: ties go
   to the smallest sorted row, and a NaN (from an overflow) orders as 0x7fc00000, after +inf.  Float64 from here: ``d = sqrt(d2)``; the
   pair is dropped unless ``d <= trunc`` (so ``d`` exactly at ``trunc`` is kept, a NaN is dropped); ``w = (sigma^2 / (sigma^2 + d^2))^2``;
   ``dtau = tau_i - tau_j``; ``dp = r_i - r_j`` on the RECORDED rows.  ``A = sum q40((w dtau) dtau)``, ``b = sum q40((w dtau) dp_{x,y})``
   with ``q40(x) = llrint(x 2^40)``, every term clipped to +-256 first so that the int64 sums of 16384 rows fit: no order is part of the
   rule.  ``A == 0`` ends the cluster as NO_BASELINE.  ``v_{k+1} = (b_x / A, b_y / A, 0)`` in float64.  The loop ends after the step in
   which ``|v_{k+1} - v_k| < tol``.  The iterations used and the pairs kept in the last one are reported.
E. Score.  ``X(v)`` is the mean over the rows of ``min(d, trunc)`` at ``v`` (a NaN counts as ``trunc``), kept as the int64 sum of
   ``q24``, as ``eval_xsensor`` does; taken at ``v = 0`` (``X0``) and at the final ``v`` (``X1``).
F. Decision.  REJECTED (5), with ``v = 0``, if ``|v| > v_max`` or ``X1 > (1 - min_gain) X0`` (float64 on the two sums); STATIC (6), with
   ``v = 0``, if ``|v| < static_speed``; ALIGNED (0) otherwise.  Only ALIGNED clusters carry a non-zero ``v``; the reported ``v`` is
   float32: ``v_x, v_y, 0, |v|``.
G. Apply.  The output flow row of a row in an ALIGNED cluster is the ego-motion flow + ``v * sensor_dt`` (float32, every operation
   rounding on its own): all its labelled rows, usable or not, as long as x, y, z are finite.  The ego-motion flow is ``E p - p`` with
   ``E = inv(pose1) @ pose0`` (numpy float64) as float32 and ``E p`` by the arithmetic of ``himo_rigid_transform``: the very expression
   ``himo_trackflow_apply``'s ``replace`` mode and ``rigid_refine``'s static snap use.  Every other row keeps the bytes of the base flow
   (``raw``: the ego-motion flow itself).

Outputs of the entry point, written whole: ``info int32 [C][8]`` = state, n, live-group bit mask, rows, votes cast, winning flat bin,
iterations, pairs of the last iteration; ``v float32 [C][4]``; ``x int64 [C][2]`` = the two score sums.

Not part of v1: a yaw rate or any rotation, ``v_z``, point-to-plane or normals, subsampling of clusters above ``max_points``,
per-sensor-pair results, any use of ``SensorsCenter``, a prior from a stored flow or a track, an in-line switch of ``save``.

Python sequences launches and owns no arithmetic on point data.  ``xalign_labelled`` sorts the rows by label exactly as
``xsensor_labelled`` does and has one host wait per call.  ``XAlign.estimate`` compacts arbitrary ids with ``torch.unique`` first, which
waits on its own.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, fields
from pathlib import Path

import numpy as np

from .stored import fmt, ratio

ALIGNED, TOO_FEW, ONE_SENSOR, TOO_LARGE, NO_BASELINE, REJECTED, STATIC = range(7)
STATE_NAMES = ("aligned", "too few", "one sensor", "too large", "no baseline", "rejected", "static")
GROUPS = 8
UNIT = 1 << 24
SENSOR_DT = 0.1
TABLE_CELLS = 15360                                  # HIMO_XALIGN_TABLE_CELLS
MAX_POINTS = 16384                                   # HIMO_XALIGN_MAX_POINTS
MAX_ITERS = 100                                      # HIMO_XALIGN_MAX_ITERS
MAX_WORK = 1 << 32                                   # HIMO_XALIGN_MAX_WORK: iters * max_points^2 at the most
SPEED_BUCKETS = ("0-10", "10-20", "20-30", "30+")    # the ladder of eval.py [m/s]; an ALIGNED cluster is never static
_ID_BITS = 40


class _CParams(ctypes.Structure):
    """mirror of ``himo_xalign_params`` (include/himo_amd.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("min_group", "min_points", "max_points", "iters")] + \
               [(k, ctypes.c_float) for k in ("v_max", "bin", "tau_min", "z_gate", "sigma", "trunc", "tol", "min_gain", "static_speed")]


def table_side(v_max: float, bin: float) -> int:
    """``nb = 2 ceil(v_max / bin) + 1`` on the float32 values"""
    return 2 * int(math.ceil(float(np.float32(v_max)) / float(np.float32(bin)))) + 1


@dataclass(frozen=True)
class XAlignParams:
    """the parameters of "cross-sensor alignment, v1"; refuses what the rule does not admit before anything is launched"""
    min_group: int = 5
    min_points: int = 600
    max_points: int = 4096
    v_max: float = 60.0
    bin: float = 1.0
    tau_min: float = 0.010
    z_gate: float = 0.2
    sigma: float = 0.3
    trunc: float = 2.0
    iters: int = 30
    tol: float = 0.02
    min_gain: float = 0.1
    static_speed: float = 0.5

    def __post_init__(self):
        positive = ("v_max", "bin", "tau_min", "z_gate", "sigma", "trunc")
        for name in positive + ("tol", "min_gain", "static_speed"):
            v = getattr(self, name)
            low_ok = (lambda x: x > 0) if name in positive else (lambda x: x >= 0)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not low_ok(v):
                raise ValueError(f"XAlignParams.{name}={v!r}: a finite number, {'> 0' if name in positive else '>= 0'}")
            with np.errstate(all="ignore"):
                as32 = float(np.float32(v))
            if not math.isfinite(as32) or not low_ok(as32):
                raise ValueError(f"XAlignParams.{name}={v!r}: not such a float32")
        for name in ("v_max", "tau_min", "sigma", "trunc"):
            if float(np.float32(getattr(self, name))) > 1024:
                raise ValueError(f"XAlignParams.{name}={getattr(self, name)!r}: at most 1024")
        if not float(np.float32(self.min_gain)) < 1:
            raise ValueError(f"XAlignParams.min_gain={self.min_gain!r}: below 1")
        if float(np.float32(self.v_max)) / float(np.float32(self.bin)) > 4096 or table_side(self.v_max, self.bin) ** 2 > TABLE_CELLS:
            raise ValueError(f"XAlignParams.bin={self.bin!r} with v_max={self.v_max!r}: the vote table of 2 ceil(v_max / bin) + 1 bins a side "
                             f"does not fit its {TABLE_CELLS} cells")
        for name in ("min_group", "min_points", "max_points", "iters"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"XAlignParams.{name}={v!r}: an integer")
        if self.min_group < 1:
            raise ValueError(f"XAlignParams.min_group={self.min_group}: at least 1")
        if self.min_points < 2:
            raise ValueError(f"XAlignParams.min_points={self.min_points}: at least 2")
        if not self.min_points <= self.max_points <= MAX_POINTS:
            raise ValueError(f"XAlignParams.max_points={self.max_points}: min_points..{MAX_POINTS}")
        if not 1 <= self.iters <= MAX_ITERS or int(self.iters) * int(self.max_points) ** 2 > MAX_WORK:
            raise ValueError(f"XAlignParams.iters={self.iters}: 1..{MAX_ITERS}, and iters * max_points^2 at most 2^32 (one workgroup walks a "
                             f"cluster; max_points={self.max_points})")

    def c_struct(self) -> _CParams:
        return _CParams(**{k: (int if t is ctypes.c_int32 else float)(getattr(self, k)) for k, t in _CParams._fields_})


def glue(info, x) -> dict:
    """host glue on copies of the integer tables: {"state", "n", "rows", "iters" int [C]; "X0", "X1" float64 [C] in metres, nan where
    the sums were not taken}"""
    info, x = np.asarray(info), np.asarray(x)
    if info.ndim != 2 or info.shape[1] != 8 or x.shape != (len(info), 2):
        raise ValueError(f"info [C, 8] and x [C, 2], not {info.shape}, {x.shape}")
    took = np.isin(info[:, 0], (ALIGNED, REJECTED, STATIC))
    with np.errstate(all="ignore"):
        rows = info[:, 3].astype(np.float64)
        X0 = np.where(took, x[:, 0].astype(np.float64) / (float(UNIT) * rows), np.nan)
        X1 = np.where(took, x[:, 1].astype(np.float64) / (float(UNIT) * rows), np.nan)
    return {"state": info[:, 0].copy(), "n": info[:, 1].copy(), "rows": info[:, 3].copy(), "iters": info[:, 6].copy(), "X0": X0, "X1": X1}


def _rows_of(pts):
    import torch
    if pts.dim() != 2 or pts.shape[1] < 3 or pts.dtype != torch.float32 or (pts.shape[0] > 0 and pts.stride(1) != 1) or \
            (pts.shape[0] > 1 and pts.stride(0) < 3):
        raise ValueError(f"points are float32 rows of x, y, z[, ...], not {pts.dtype} {tuple(pts.shape)} with strides {pts.stride()}")
    n = int(pts.shape[0])
    return n, (int(pts.stride(0)) if n > 1 else int(pts.shape[1]))


def xalign_labelled(pts, labels, group, tau, n_clusters: int, params: XAlignParams | None = None):
    """Rules A-F through ``himo_xalign`` on the current stream: ``pts`` device float32 (N, >= 3) rows (any row pitch), ``labels`` device
    int32 [N] (0 and anything outside 1..C: none), ``group`` device uint8 [N], ``tau`` device float32 [N] -> (info int32 [C, 8], v
    float32 [C, 4], x int64 [C, 2]) device tensors.  Sorts the rows by label as ``xsensor_labelled`` does; one host wait, through pinned
    memory behind an event."""
    import torch
    from . import _lib
    from .icpflow import pinned_words
    lib, P = _lib.load(), _lib.ptr
    params = params if params is not None else XAlignParams()
    dev = pts.device
    n, pitch = _rows_of(pts)
    if tau is None:
        raise ValueError("tau: the capture time per point is required")
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    group = group.to(device=dev, dtype=torch.uint8).contiguous()
    tau = tau.to(device=dev, dtype=torch.float32).contiguous()
    if labels.shape != (n,) or group.shape != (n,) or tau.shape != (n,):
        raise ValueError(f"labels {tuple(labels.shape)}, group {tuple(group.shape)} and tau {tuple(tau.shape)} are not row-aligned with the {n} points")
    C = int(n_clusters)
    if C < 0:
        raise ValueError(f"n_clusters={n_clusters}: not negative")
    # the labelled rows sorted by label (stable: ascending row inside a cluster) and every label's first sorted row
    lab = torch.where((labels > 0) & (labels <= C), labels, torch.zeros_like(labels))
    order = torch.argsort(torch.where(lab > 0, lab, torch.iinfo(torch.int32).max), stable=True)
    sizes = torch.bincount(lab, minlength=C + 1)[1:C + 1]
    offsets = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    if C:
        torch.cumsum(sizes, 0, out=offsets[1:])
    host = pinned_words(C + 1)
    host[:C + 1].copy_(offsets, non_blocking=True)
    landed = torch.cuda.Event()
    landed.record(torch.cuda.current_stream(dev))
    landed.synchronize()                                            # the call's one host wait
    h_off = host[:C + 1].numpy().copy()
    nc = int(h_off[C])
    info = torch.zeros((C, 8), dtype=torch.int32, device=dev)
    v = torch.zeros((C, 4), dtype=torch.float32, device=dev)
    x = torch.zeros((C, 2), dtype=torch.int64, device=dev)
    if C:
        ws = torch.empty(max(int(lib.himo_xalign_workspace_bytes(nc, C)), 16), dtype=torch.uint8, device=dev)
        c_params = params.c_struct()
        with torch.cuda.device(dev):
            st = lib.himo_xalign(n, P(pts), pitch, P(lab), P(group), P(tau), nc, P(order), C, h_off.ctypes.data, P(offsets),
                                 ctypes.addressof(c_params), P(info), P(v), P(x), P(ws), ws.numel(), _lib.stream_handle())
        _lib.check(st, "himo_xalign")
    return info, v, x


def ego_transform(pose0, pose1) -> np.ndarray:
    """rule G's ``E``: the first three rows of ``inv(pose1) @ pose0`` as float32 [12]"""
    E = (np.linalg.inv(np.asarray(pose1, dtype=np.float64)) @ np.asarray(pose0, dtype=np.float64)).astype(np.float32)
    return np.ascontiguousarray(E[:3]).reshape(12)


def xalign_apply(pts, labels, info, v, pt_off, E, base=None, sensor_dt: float = SENSOR_DT):
    """Rule G through ``himo_xalign_apply`` on the current stream, over one point buffer of sweeps laid end to end: ``pts`` device float32
    (N, >= 3), ``labels`` device int32 [N] in 1..C (the compact labels ``info`` / ``v`` were made for), ``pt_off`` int64 [S + 1] on the
    host, ``E`` float32 [S, 12] on the host (``ego_transform`` per sweep), ``base`` None (``raw``) or device float32 [N, 3] -> the flow,
    device float32 [N, 3].  No host wait."""
    import torch
    from . import _lib
    lib, P = _lib.load(), _lib.ptr
    dev = pts.device
    n, pitch = _rows_of(pts)
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    if labels.shape != (n,):
        raise ValueError(f"labels {tuple(labels.shape)} are not row-aligned with the {n} points")
    h_off = np.ascontiguousarray(pt_off, dtype=np.int64)
    S = len(h_off) - 1
    h_E = np.ascontiguousarray(E, dtype=np.float32).reshape(-1, 12)
    if S < 0 or len(h_E) != S:
        raise ValueError(f"pt_off [S + 1] and E [S, 12], not {h_off.shape} and {h_E.shape}")
    if base is not None:
        base = base.to(device=dev, dtype=torch.float32).contiguous()
        if base.shape != (n, 3):
            raise ValueError(f"base is [{n}, 3], not {tuple(base.shape)}")
    C = int(info.shape[0])
    if tuple(info.shape) != (C, 8) or tuple(v.shape) != (C, 4) or info.dtype != torch.int32 or v.dtype != torch.float32:
        raise ValueError(f"info int32 [C, 8] and v float32 [C, 4], not {info.dtype} {tuple(info.shape)}, {v.dtype} {tuple(v.shape)}")
    info, v = info.contiguous(), v.contiguous()
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_off = torch.from_numpy(h_off).to(dev)
    d_E = torch.from_numpy(h_E).to(dev)
    with torch.cuda.device(dev):
        st = lib.himo_xalign_apply(n, P(pts), pitch, P(labels), C, P(info), P(v), S, h_off.ctypes.data, P(d_off), P(d_E), P(base),
                                   float(sensor_dt), P(out), _lib.stream_handle())
    _lib.check(st, "himo_xalign_apply")
    return out


class XAlignResult:
    """What ``XAlign.estimate`` returns.  ``info`` (int32 [C, 8]), ``v`` (float32 [C, 4]) and ``x`` (int64 [C, 2]) are the entry point's
    outputs, ``ids`` (int64 [C]) the original id of every cluster, ``glue`` the host glue's dict.  Host copies, made when first asked for
    (that is a wait of its own); ``device_info`` / ``device_v`` / ``device_x`` are the device tensors, ``labels`` the device int32 [N]
    compact label (1..C, 0 = none) of every row, which ``xalign_apply`` takes."""

    def __init__(self, info, v, x, ids, labels):
        self.device_info, self.device_v, self.device_x, self.ids, self.labels = info, v, x, ids, labels
        self._host = None

    def _copies(self):
        if self._host is None:
            info, v, x = self.device_info.cpu().numpy(), self.device_v.cpu().numpy(), self.device_x.cpu().numpy()
            self._host = (info, v, x, glue(info, x))
        return self._host

    info = property(lambda self: self._copies()[0])
    v = property(lambda self: self._copies()[1])
    x = property(lambda self: self._copies()[2])
    glue = property(lambda self: self._copies()[3])


class XAlign:
    """``XAlign(device, params).estimate(pts, ids, group, tau)`` -> an ``XAlignResult`` (module docstring).  ``ids`` may hold arbitrary
    integer ids such as ``ray_label`` (0 = none): they are compacted to 1..C in ascending order and come back, exactly, in
    ``XAlignResult.ids``.  ``apply(result, pts, pt_off, E, base)`` is rule G.  There is no CPU path."""

    def __init__(self, device=None, params: XAlignParams | None = None, sensor_dt: float = SENSOR_DT):
        from . import _lib
        self.params = params if params is not None else XAlignParams()
        if not (math.isfinite(sensor_dt) and sensor_dt > 0):
            raise ValueError(f"sensor_dt={sensor_dt}: finite and > 0")
        self.sensor_dt = float(sensor_dt)
        self.lib = _lib.load()
        if self.lib.himo_abi_sizeof(b"himo_xalign_params") != ctypes.sizeof(_CParams):
            raise ImportError("himo_xalign_params: the library's layout is not this binding's; rebuild libhimo_amd.so")
        self.device = device if device is not None else _lib.require_gpu()

    def _points(self, pts):
        import torch
        p = (pts if isinstance(pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pts))).to(device=self.device, dtype=torch.float32)
        if p.dim() != 2 or p.shape[1] < 3:
            raise ValueError(f"points are rows of x, y, z[, ...], not {tuple(p.shape)}")
        if p.stride(1) != 1 or (p.shape[0] > 1 and p.stride(0) < 3):
            p = p.contiguous()
        return p

    def estimate(self, pts, ids, group, tau) -> XAlignResult:
        import torch
        dev = self.device
        up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))       # noqa: E731
        p = self._points(pts)
        if tau is None:
            raise ValueError("tau: the capture time per point is required")
        if not isinstance(ids, torch.Tensor):                         # (uint32 ids: through int64, which holds every one of them)
            ids = np.asarray(ids)
            if ids.dtype.kind not in "iu":
                raise ValueError(f"ids are one integer id per row, not {ids.dtype}")
            ids = ids.astype(np.int64)
        raw = up(ids)
        if raw.dtype.is_floating_point or raw.dtype == torch.bool or raw.dim() != 1 or raw.shape[0] != p.shape[0]:
            raise ValueError(f"ids are one integer id per row, not {raw.dtype} {tuple(raw.shape)} for {p.shape[0]} rows")
        if not isinstance(group, torch.Tensor):
            group = np.asarray(group)
            if group.dtype.kind not in "iu" or group.shape != (p.shape[0],):
                raise ValueError(f"group is one sensor id per row, not {group.dtype} {group.shape}")
            group = np.where((group < 0) | (group > 255), 255, group).astype(np.uint8)       # (an id the rule does not admit stays one)
        uniq, inverse = torch.unique(raw.to(device=dev).to(torch.int64), return_inverse=True)       # ascending; waits
        nonzero = uniq != 0
        rank = torch.cumsum(nonzero.to(torch.int64), 0) * nonzero     # 0 stays 0, the others 1..C in ascending order
        host_ids = uniq[nonzero].cpu().numpy()
        labels = rank[inverse].to(torch.int32)
        info, v, x = xalign_labelled(p, labels, up(group), up(tau), len(host_ids), self.params)
        return XAlignResult(info, v, x, host_ids.astype(np.int64), labels)

    def apply(self, res: XAlignResult, pts, pt_off, E, base=None):
        import torch
        if base is not None and not isinstance(base, torch.Tensor):
            base = torch.from_numpy(np.ascontiguousarray(base, dtype=np.float32))
        return xalign_apply(self._points(pts), res.labels, res.device_info, res.device_v, pt_off, E, base, self.sensor_dt)


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def speed_bucket(speed: float) -> str:
    """0-10 / 10-20 / 20-30 / 30+ m/s"""
    return SPEED_BUCKETS[min(int(speed // 10.0), 3)]


def new_totals() -> dict:
    return {"sweeps": 0, "points": 0, "points_moved": 0, "states": [0] * len(STATE_NAMES), "speed": {b: 0 for b in SPEED_BUCKETS},
            "decided": 0, "sum_iters": 0, "sum_X0": 0.0, "sum_X1": 0.0}


def tally(totals: dict, info, v, x) -> None:
    """add the clusters of one call to the running totals"""
    g = glue(info, x)
    for s in range(len(STATE_NAMES)):
        totals["states"][s] += int((g["state"] == s).sum())
    for c in np.flatnonzero(g["state"] == ALIGNED):
        totals["speed"][speed_bucket(float(v[c, 3]))] += 1
    took = np.isin(g["state"], (ALIGNED, REJECTED, STATIC))
    totals["decided"] += int(took.sum())
    totals["sum_iters"] += int(g["iters"][took].sum())
    totals["sum_X0"] += float(g["X0"][took].sum())
    totals["sum_X1"] += float(g["X1"][took].sum())


def summary(t: dict) -> dict:
    """the numbers of the report and of ``--json``: the derived values and, under "totals", the raw sums"""
    return {"sweeps": t["sweeps"], "points": t["points"], "points_moved": t["points_moved"], "states": dict(zip(STATE_NAMES, t["states"])),
            "speed": dict(t["speed"]), "mean_iters": ratio(t["sum_iters"], t["decided"]), "mean_X0": ratio(t["sum_X0"], t["decided"]),
            "mean_X1": ratio(t["sum_X1"], t["decided"]), "ratio": ratio(t["sum_X1"], t["sum_X0"]), "totals": t}


def _table(n: dict) -> str:
    return "\n".join([f"  {n['sweeps']} sweeps, {n['points']} points, {n['points_moved']} moved; clusters " +
                      ", ".join(f"{k} {v}" for k, v in n["states"].items()),
                      "  aligned by speed [m/s]: " + ", ".join(f"{k} {v}" for k, v in n["speed"].items()),
                      f"  over the decided clusters (aligned, rejected, static): mean iterations {fmt(n['mean_iters'], '.2f')}, "
                      f"X0 {fmt(n['mean_X0'], '.4f')} m, X1 {fmt(n['mean_X1'], '.4f')} m, X1 / X0 {fmt(n['ratio'], '.3f')}"])


def align_batch(engine: XAlign, frames: list, packed: dict, label_key: str, base: str, cluster: str = "dbscan", min_cluster_size=None,
                min_samples=None):
    """One ``himo_xalign`` call and one ``himo_xalign_apply`` call for the sweeps of ``frames`` laid end to end: the cluster of sweep s
    with stored id v has the key ``((s + 1) << 40) | v``.  ``packed``: the batch's device tensors (``pc0``, ``lidar_dt``, ``lidar_id``,
    ``offsets`` on the host, the base flow unless ``raw``, and ``ids`` unless ``label_key`` is ``cluster``).  -> (XAlignResult, the flow
    device float32 [rows, 3])"""
    import torch
    from .eval_xsensor import cluster_ids
    off, pc0 = packed["offsets"], packed["pc0"]
    keys = []
    for s, f in enumerate(frames):
        lo, hi = int(off[s]), int(off[s + 1])
        if label_key == "cluster":
            ids = cluster_ids(pc0[lo:hi, :3], packed["gm0"][lo:hi], cluster, min_cluster_size, min_samples)
        else:
            ids = packed["ids"][lo:hi]
        keys.append(torch.where(ids != 0, ids + ((s + 1) << _ID_BITS), torch.zeros_like(ids)))
    res = engine.estimate(pc0, torch.cat(keys), packed["lidar_id"], packed["lidar_dt"])
    E = np.stack([ego_transform(f["pose0"], f["pose1"]) for f in frames])
    return res, engine.apply(res, pc0, off, E, None if base == "raw" else packed[base])


def main(data_dir: str, label_key: str, base: str = "raw", out_name: str = "xalign", cluster: str = "dbscan",
         params: XAlignParams | None = None, batch: int = 8, json_path: str | None = None, overwrite: bool = False,
         sensor_dt: float = SENSOR_DT, min_cluster_size: int | None = None, min_samples: int | None = None, overlap: bool = True) -> dict:
    """The program: for every sweep of ``data_dir`` the velocity of every cluster of ``label_key`` from the sweep's own capture times,
    ``batch`` sweeps per ``himo_xalign`` call, and ``<timestamp>/<out_name>`` float32 (N, 3) = the base flow (``raw``: the ego-motion
    flow) with the rows of ALIGNED clusters replaced by ego motion + ``v * sensor_dt``, written through ``save``'s sinks.  Under
    ``torchrun`` sweep i is done by rank i % world (npz) or whole scenes per rank (h5) and the totals are gathered.  Returns what
    ``--json`` writes."""
    from . import distenv, stored
    from .dataset import NpzDataset, open_dataset
    from .save import H5ResultSink, NpzResultSink
    from .seflow.ssl_label import CLUSTERINGS
    from .eval_xsensor import pack_sweeps
    from .sweeps import MissingKey, fed, raise_missing, sharded_items
    if not label_key:
        raise ValueError("label_key: a stored integer key (ray_label, flow_instance_id, ...) or 'cluster'")
    if not base:
        raise ValueError("base: 'raw' (the ego-motion flow) or a stored flow")
    if not out_name or out_name == "raw":
        raise ValueError(f"out_name={out_name!r}: 'raw' means zero motion downstream; name the key to write")
    if out_name == base:
        raise ValueError(f"out_name={out_name!r} is the base: the aligned flow goes under a key of its own")
    if cluster not in CLUSTERINGS:
        raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
    stored.at_least_one("batch", batch, " sweep a call")
    params = params if params is not None else XAlignParams()
    if not (math.isfinite(sensor_dt) and sensor_dt > 0):
        raise ValueError(f"sensor_dt={sensor_dt}: finite and > 0")
    flows = [] if base == "raw" else [base]
    needs = ["lidar_id", "lidar_dt"] + (["gm0"] if label_key == "cluster" else [label_key])
    root = Path(data_dir)
    sums = new_totals()
    with distenv.process_group() as (rank, world):
        ds = open_dataset(root, vis_name=flows + [out_name], eval=False, fields=tuple(["pc0", "pose0", "pose1"] + needs + flows))
        npz = isinstance(ds, NpzDataset)
        sink = None

        def loop():
            nonlocal sink
            mine = sharded_items(ds, whole_scenes=not npz)          # whole scenes per rank: every scene file has one writer
            # the refusals, before anything touches the GPU or a file is written
            try:
                for i in mine:
                    where = "/".join(map(str, ds.index[i]))
                    have = stored.present(ds, i, flows + needs + [out_name])
                    for key, hint in [("lidar_id", "the sensor id per point: the extractors write it"),
                                      ("lidar_dt", "the capture time per point: the extractors write it")] + \
                            [(s, "--base names a stored flow; 'raw' needs none") for s in flows] + \
                            [("gm0", "--label_key cluster needs the sweep's ground mask: `python -m himo_amd.ground_seg` writes it")
                             if label_key == "cluster" else (label_key, "`python -m himo_amd.raymap` writes ray_label")]:
                        if key not in have:
                            raise MissingKey(key, [f"[Warning]: No {key} in {where} ({hint}), check the data."])
                    if out_name in have and not overwrite:
                        raise FileExistsError(f"{where} already holds '{out_name}': pass --overwrite to replace it")
            except MissingKey as e:
                raise_missing(e)
            if not mine:
                return
            import torch
            engine = XAlign(params=params, sensor_dt=sensor_dt)
            sink = NpzResultSink(root, out_name) if npz else H5ResultSink(root, out_name, before_write=ds.forget)
            dev = engine.device

            def build(idx, upload):
                return (idx,) + pack_sweeps(ds, idx, upload, dev, flows, label_key)

            batches = [mine[lo:lo + int(batch)] for lo in range(0, len(mine), int(batch))]
            for idx, frames, packed in fed(iter(batches), build, device=dev, overlap=overlap):
                res, flow = align_batch(engine, frames, packed, label_key, base, cluster, min_cluster_size, min_samples)
                host, off = flow.cpu().numpy(), packed["offsets"]
                info, v = res.info, res.v
                tally(sums, info, v, res.x)
                if len(info):                                       # rule G moves the finite rows of ALIGNED clusters
                    lab = res.labels.long()
                    hit = (res.device_info[:, 0] == ALIGNED)[(lab - 1).clamp(min=0)] & (lab > 0)
                    sums["points_moved"] += int((hit & torch.isfinite(packed["pc0"][:, :3]).all(dim=1)).sum())
                for j, (i, f) in enumerate(zip(idx, frames)):
                    sink(i, f, host[int(off[j]):int(off[j + 1])])
                sums["sweeps"] += len(frames)
                sums["points"] += int(off[len(frames)])
            if hasattr(sink, "close"):                              # (on success only: a failed run leaves its last scene as it was)
                sink.close()

        distenv.run_shard(loop, "its share of the sweeps", closing=(ds,))
        numbers = summary(distenv.gathered(sums))
        distenv.report(rank, f"xalign (cross-sensor alignment, v1; parity unpinned), labels '{label_key}', base '{base}' -> '{out_name}':\n"
                             f"{_table(numbers)}", numbers, json_path)
    return numbers


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="per cluster, the velocity that lays the sensors' copies of an object on top of one another, "
                                             "from the capture times inside one sweep, stored as a flow (cross-sensor alignment, v1; parity "
                                             "unpinned: the reference has no such stage; timed on synthetic sweeps only, profiles/xalign.txt; "
                                             "nothing tried on field data; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--label_key", required=True, help="a stored integer label per point (ray_label, flow_instance_id, ...; 0 = none), or "
                                                       "'cluster': cluster the non-ground in-range points (needs ground_mask)")
    ap.add_argument("--base", default="raw", help="the flow every row that is not moved keeps: 'raw' (the ego-motion flow) or a stored flow")
    ap.add_argument("--out_name", default="xalign", help="the key to write")
    ap.add_argument("--cluster", default="dbscan", help="--label_key cluster: 'dbscan' (the default) or 'hdbscan'")
    d = XAlignParams()
    helps = {"min_group": "a sensor with fewer usable points in a cluster takes no part there", "min_points": "fewer usable points: not tried",
             "max_points": "more usable points: not tried", "v_max": "the vote covers, and the result may reach, this speed, m/s",
             "bin": "m/s per vote bin", "tau_min": "the smallest difference of capture times that counts, s",
             "z_gate": "a voting pair lies closer than this in z, metres", "sigma": "the scale of the weight, metres",
             "trunc": "a pair farther apart is dropped, metres", "iters": "the most iterations", "tol": "the loop ends when v changes by less, m/s",
             "min_gain": "rejected unless the cross-sensor distance falls by this share", "static_speed": "slower: static, m/s"}
    for f in fields(XAlignParams):
        ap.add_argument(f"--{f.name}", type=int if f.type == "int" else float, default=getattr(d, f.name), help=helps[f.name])
    ap.add_argument("--batch", type=int, default=8, metavar="SWEEPS", help="sweeps per call")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the report's numbers and the raw totals to PATH")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing <out_name> instead of refusing")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    return main(a.data_dir, a.label_key, a.base, a.out_name, a.cluster, XAlignParams(**{f.name: getattr(a, f.name) for f in fields(XAlignParams)}),
                a.batch, a.json, a.overwrite)


if __name__ == "__main__":
    _cli()
