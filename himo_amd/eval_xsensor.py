"""Cross-sensor consistency: a score that needs no ground truth (``python -m himo_amd.eval_xsensor --data_dir D --res_names
raw,seflowpp_best --label_key ray_label`` prints it per name).  The distortion this project removes is a multi-LiDAR effect: several
sensors see the same vehicle at different instants of one sweep, so its raw points form several displaced copies.  Inside each cluster,
take the distance from every point to the nearest point recorded by ANOTHER sensor: it is large when the copies are displaced and falls
to the sampling spacing when they are laid on top of one another.  The loader's ``lidar_id`` and ``lidar_dt`` are all it reads besides
the points and a per-point cluster label, so it completes the label-free chain ``ground_seg -> raymap -> save -> eval_xsensor`` for
field data whose ground truth does not ship.

PARITY UNPINNED.  The reference has no such stage.  Like ``box_fit``, ``eval_box`` and ``track`` it follows the build's own written
rule, below, and is checked against a numpy restatement of it (``tests/xsensor_ref.py``), never against the reference.  No claim is made
about the reference's numbers.  Timing: 1.43 ms per call of 32 synthetic 120k-point sweeps x 2 names in 19200 clusters -- the sort and
the host wait 0.66 ms, count 0.22 ms, search 0.36 ms (1.03 x ``himo_nn_search`` in float32 over the same clusters), reduce 0.12 ms
(profiles/xsensor.txt); nothing has been tried on field data.  On synthetic vehicles of 600 points sampled by three sensors 33 ms apart
under 0.02 m noise, compensation by the true flow brings the summed distance to 0.53 of raw's at 20 m/s and to 0.37 at 35 m/s, and
static vehicles give byte-identical records (tests/test_xsensor_cpu.py).  The floor of the number is the point spacing, which is the
same on both sides of a paired comparison.

The rule -- "cross-sensor consistency, v1" (normative)
======================================================
Inputs per call: ``pts [N][pitch >= 3]`` float32 (raw or compensated: the caller decides), ``labels [N]`` int32 (0 = none, else 1..C),
``group [N]`` uint8 (the sensor id), ``dt [N]`` float32 or none (the capture time), ``motion [N][3]`` float32 or none (a displacement
per sweep period).

Parameters (``XSensorParams``, mirrored as ``himo_xsensor_params``, 20 bytes): ``trunc`` float32, 4.0 m (admitted: finite, > 0 and, so
that ``q`` of it fits an integer, <= 1024); ``near`` float32, 0.2 m (finite, >= 0); ``min_group`` int32, 5 (>= 1); ``min_points`` int32,
10, the evaluator's instance floor (>= 2); ``max_points`` int32, 8192, as ``box_fit`` (``min_points``..2^20).  Anything else is refused
before a launch, with no write.

A. Usable rows.  A row is USABLE iff its label is in 1..C, its x, y and z are finite, its group is <= 7 and, where ``dt`` is given, its
   ``dt`` is finite.  ``n`` is the cluster's usable rows, ``n_g`` its usable rows of group g.
B. State, tested in this order: TOO_FEW (1) if ``n < min_points``; TOO_LARGE (3) if ``n > max_points``; group g is LIVE iff ``n_g >=
   min_group``, and the cluster is ONE_SENSOR (2) if fewer than two groups are live; SCORED (0) otherwise.  Only SCORED clusters run
   C-D; the others write their state, ``n`` and the ``n_g``, and zeros elsewhere.
C. Search.  A QUERY row is a usable row of a live group.  Its candidates are the usable rows of the same cluster in a DIFFERENT live
   group.  For query i and candidate j, all float32, every operation rounding on its own (``himo_amd/csrc/xsensor.hip`` is built with
   ``-ffp-contract=off``): ``dx = x_i - x_j``, ``dy`` and ``dz`` likewise; ``d2 = (dx*dx + dy*dy) + dz*dz``.  ``m_i`` is the minimum of
   ``d2`` over the candidates.  The minimum is order-free, so the per-row result is defined bit for bit.  No index is reported.
D. Per-row terms, in float64: ``d_i = sqrt((double)m_i)``; ``c_i = d_i < (double)trunc ? d_i : (double)trunc`` (a ``+inf`` from
   overflow clips); row i is NEAR iff ``d_i <= (double)near``; ``q(x) = llrint(x * 2^24)``, the unit of ``eval_flow``.  Every sum is an
   int64 sum, so block and lane order are not part of the rule.
E. Outputs of the entry point: ``info int32 [C][4]`` = state, n, live-group bit mask, query rows; ``rec int64 [C][8][4]``, per group =
   ``n_g``, the sum of ``q(dt)`` over the group's usable rows (``dt`` clipped to +-1024 s so that ``q`` fits; 0 without ``dt``), the
   sum of ``q(c_i)`` over its query rows, its NEAR count; ``mot int64 [C][2]`` = the usable rows with a finite motion, and the sum of
   ``q(s_i)`` over them, ``s_i = sqrt(((double)mx*mx + (double)my*my) + (double)mz*mz)`` clipped at 1024 m (zeros without ``motion``);
   optionally ``m float32 [n_sorted]``: ``m_i`` per sorted row, ``+inf`` for a row that is not a query.
F. Host glue (Python, float64, on C rows only, no point data): the cluster distance ``X_c = sum_g sum q(c) / (2^24 * query rows)``; the
   near share, NEAR rows / query rows; per group the mean time ``t_g = sum q(dt) / (2^24 n_g)``; the time spread over the live groups
   ``dt_c = max t_g - min t_g``; the speed, ``mean s / sensor_dt``.

Not part of v1: a per-point stored key, a range bucket, weighting by overlap, normals or point-to-plane distance, a split by time for
single-sensor data, pairs of sensors reported separately, any use of ``SensorsCenter``.

Python sequences launches and owns no arithmetic on point data.  ``xsensor_labelled`` sorts the rows by label exactly as
``box_fit.fit_labelled`` does and has one host wait per call: the clusters' row ranges, read through pinned memory behind an event.
``XSensor.score`` compacts arbitrary ids with ``torch.unique`` first, which waits on its own.  The clusters of several sweeps and several
results go into ONE call: more segments over one point buffer.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .stored import check_point_labels, fmt, ratio

SCORED, TOO_FEW, ONE_SENSOR, TOO_LARGE = 0, 1, 2, 3
STATE_NAMES = ("scored", "too few", "one sensor", "too large")
GROUPS = 8
UNIT = 1 << 24
SENSOR_DT = 0.1
STATIC_SPEED = 0.5                                   # below this [m/s] a cluster is static
SPEED_BUCKETS = ("static", "0-10", "10-20", "20-30", "30+")           # the ladder of eval.py [m/s]
DT_BUCKETS = ("<10ms", "10-30ms", ">30ms")
_ID_BITS = 40                                        # the program's keys: (name, sweep) above, the stored id below


class _CParams(ctypes.Structure):
    """mirror of ``himo_xsensor_params`` (include/himo_amd.h)"""
    _fields_ = [("trunc", ctypes.c_float), ("near", ctypes.c_float), ("min_group", ctypes.c_int32), ("min_points", ctypes.c_int32),
                ("max_points", ctypes.c_int32)]


@dataclass(frozen=True)
class XSensorParams:
    """the parameters of "cross-sensor consistency, v1"; refuses what the rule does not admit before anything is launched"""
    trunc: float = 4.0
    near: float = 0.2
    min_group: int = 5
    min_points: int = 10
    max_points: int = 8192

    def __post_init__(self):
        for name, low_ok in (("trunc", lambda v: v > 0), ("near", lambda v: v >= 0)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not low_ok(v):
                raise ValueError(f"XSensorParams.{name}={v!r}: a finite number, {'> 0' if name == 'trunc' else '>= 0'}")
            with np.errstate(all="ignore"):
                as32 = float(np.float32(v))
            if not math.isfinite(as32) or not low_ok(as32):
                raise ValueError(f"XSensorParams.{name}={v!r}: not such a float32")
        if self.trunc > 1024:
            raise ValueError(f"XSensorParams.trunc={self.trunc!r}: at most 1024 m")
        for name in ("min_group", "min_points", "max_points"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"XSensorParams.{name}={v!r}: an integer")
        if self.min_group < 1:
            raise ValueError(f"XSensorParams.min_group={self.min_group}: at least 1")
        if self.min_points < 2:
            raise ValueError(f"XSensorParams.min_points={self.min_points}: at least 2")
        if not self.min_points <= self.max_points <= 1 << 20:
            raise ValueError(f"XSensorParams.max_points={self.max_points}: min_points..2^20")

    def c_struct(self) -> _CParams:
        return _CParams(self.trunc, self.near, int(self.min_group), int(self.min_points), int(self.max_points))


def glue(info, rec, mot, sensor_dt: float = SENSOR_DT) -> dict:
    """Rule F on host copies of the integer tables: {"state", "n", "queries" int [C]; "X", "near", "dt_spread", "speed" float64 [C];
    "t" float64 [C, 8]}, nan where a value has no rows behind it (a cluster that is not SCORED, a group without rows, no motion)."""
    info, rec, mot = np.asarray(info), np.asarray(rec), np.asarray(mot)
    if info.ndim != 2 or info.shape[1] != 4 or rec.shape != (len(info), GROUPS, 4) or mot.shape != (len(info), 2):
        raise ValueError(f"info [C, 4], rec [C, 8, 4] and mot [C, 2], not {info.shape}, {rec.shape}, {mot.shape}")
    if not (math.isfinite(sensor_dt) and sensor_dt > 0):
        raise ValueError(f"sensor_dt={sensor_dt}: finite and > 0")
    C = len(info)
    scored = info[:, 0] == SCORED
    nan = lambda *shape: np.full(shape, np.nan)                       # noqa: E731
    with np.errstate(all="ignore"):
        n_g = rec[:, :, 0].astype(np.float64)
        t = np.where(rec[:, :, 0] > 0, rec[:, :, 1].astype(np.float64) / (float(UNIT) * n_g), np.nan)
        nq = info[:, 3].astype(np.float64)
        X = np.where(scored, rec[:, :, 2].sum(axis=1).astype(np.float64) / (float(UNIT) * nq), np.nan)
        near = np.where(scored, rec[:, :, 3].sum(axis=1).astype(np.float64) / nq, np.nan)
        live = (info[:, 2:3] >> np.arange(GROUPS)[None, :] & 1).astype(bool) & scored[:, None]
        spread = nan(C)
        if scored.any():
            spread[scored] = np.where(live[scored], t[scored], -np.inf).max(axis=1) - np.where(live[scored], t[scored], np.inf).min(axis=1)
        speed = np.where(scored & (mot[:, 0] > 0), mot[:, 1].astype(np.float64) / (float(UNIT) * mot[:, 0].astype(np.float64)) / sensor_dt, np.nan)
    return {"state": info[:, 0].copy(), "n": info[:, 1].copy(), "queries": info[:, 3].copy(), "X": X, "near": near, "t": t,
            "dt_spread": spread, "speed": speed}


def xsensor_labelled(pts, labels, group, n_clusters: int, params: XSensorParams | None = None, dt=None, motion=None, want_rows: bool = False):
    """Rules A-E through ``himo_xsensor`` on the current stream: ``pts`` device float32 (N, >= 3) rows (any row pitch), ``labels``
    device int32 [N] (0 and anything outside 1..C: none), ``group`` device uint8 [N], ``dt`` None or device float32 [N], ``motion``
    None or device float32 [N, 3] -> (info int32 [C, 4], rec int64 [C, 8, 4], mot int64 [C, 2], rows) device tensors; ``rows`` is None,
    or with ``want_rows`` the pair (m float32 [n_sorted], order int64 [n_sorted]): rule E's per-row minimum and the row of ``pts``
    behind every sorted row.  Sorts the rows by label as ``box_fit.fit_labelled`` does; one host wait, through pinned memory behind an
    event."""
    import torch
    from . import _lib
    from .icpflow import pinned_words
    lib, P = _lib.load(), _lib.ptr
    params = params if params is not None else XSensorParams()
    dev = pts.device
    if pts.dim() != 2 or pts.shape[1] < 3 or pts.dtype != torch.float32 or (pts.shape[0] > 0 and pts.stride(1) != 1) or \
            (pts.shape[0] > 1 and pts.stride(0) < 3):
        raise ValueError(f"points are float32 rows of x, y, z[, ...], not {pts.dtype} {tuple(pts.shape)} with strides {pts.stride()}")
    n = int(pts.shape[0])
    pitch = int(pts.stride(0)) if n > 1 else int(pts.shape[1])
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    group = group.to(device=dev, dtype=torch.uint8).contiguous()
    if labels.shape != (n,) or group.shape != (n,):
        raise ValueError(f"labels {tuple(labels.shape)} and group {tuple(group.shape)} are not row-aligned with the {n} points")
    if dt is not None:
        dt = dt.to(device=dev, dtype=torch.float32).contiguous()
        if dt.shape != (n,):
            raise ValueError(f"dt is [{n}], not {tuple(dt.shape)}")
    if motion is not None:
        motion = motion.to(device=dev, dtype=torch.float32).contiguous()
        if motion.shape != (n, 3):
            raise ValueError(f"motion is [{n}, 3], not {tuple(motion.shape)}")
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
    info = torch.zeros((C, 4), dtype=torch.int32, device=dev)
    rec = torch.zeros((C, GROUPS, 4), dtype=torch.int64, device=dev)
    mot = torch.zeros((C, 2), dtype=torch.int64, device=dev)
    m = torch.full((nc,), float("inf"), dtype=torch.float32, device=dev) if want_rows else None
    if C:
        ws = torch.empty(max(int(lib.himo_xsensor_workspace_bytes(nc, C)), 16), dtype=torch.uint8, device=dev)
        c_params = params.c_struct()
        with torch.cuda.device(dev):
            st = lib.himo_xsensor(n, P(pts), pitch, P(lab), P(group), P(dt), P(motion), nc, P(order), C, h_off.ctypes.data, P(offsets),
                                  ctypes.addressof(c_params), P(info), P(rec), P(mot), P(m), P(ws), ws.numel(), _lib.stream_handle())
        _lib.check(st, "himo_xsensor")
    return info, rec, mot, ((m, order[:nc]) if want_rows else None)


class XSensorResult:
    """What ``XSensor.score`` returns.  ``info`` (int32 [C, 4]), ``rec`` (int64 [C, 8, 4]) and ``mot`` (int64 [C, 2]) are rule E's
    outputs, ``ids`` (int64 [C]) the original id of every cluster, ``glue`` rule F's dict.  Host copies, made when first asked for
    (that is a wait of its own); ``device_info`` / ``device_rec`` / ``device_mot`` are the device tensors, ``device_rows`` None or
    (m, order) as ``xsensor_labelled`` returns them."""

    def __init__(self, info, rec, mot, rows, ids, sensor_dt):
        self.device_info, self.device_rec, self.device_mot, self.device_rows, self.ids = info, rec, mot, rows, ids
        self.sensor_dt = sensor_dt
        self._host = None

    def _copies(self):
        if self._host is None:
            info, rec, mot = self.device_info.cpu().numpy(), self.device_rec.cpu().numpy(), self.device_mot.cpu().numpy()
            self._host = (info, rec, mot, glue(info, rec, mot, self.sensor_dt))
        return self._host

    info = property(lambda self: self._copies()[0])
    rec = property(lambda self: self._copies()[1])
    mot = property(lambda self: self._copies()[2])
    glue = property(lambda self: self._copies()[3])


class XSensor:
    """``XSensor(device, params).score(pts, ids, group, dt=None, motion=None)`` -> an ``XSensorResult`` (module docstring).  ``ids`` may
    hold arbitrary integer ids such as ``ray_label`` or ``flow_instance_id`` (0 = none): they are compacted to 1..C in ascending order
    and come back, exactly, in ``XSensorResult.ids``.  There is no CPU path."""

    def __init__(self, device=None, params: XSensorParams | None = None, sensor_dt: float = SENSOR_DT):
        from . import _lib
        self.params = params if params is not None else XSensorParams()
        if not (math.isfinite(sensor_dt) and sensor_dt > 0):
            raise ValueError(f"sensor_dt={sensor_dt}: finite and > 0")
        self.sensor_dt = float(sensor_dt)
        self.lib = _lib.load()
        if self.lib.himo_abi_sizeof(b"himo_xsensor_params") != ctypes.sizeof(_CParams):
            raise ImportError("himo_xsensor_params: the library's layout is not this binding's; rebuild libhimo_amd.so")
        self.device = device if device is not None else _lib.require_gpu()

    def score(self, pts, ids, group, dt=None, motion=None, want_rows: bool = False) -> XSensorResult:
        import torch
        dev = self.device
        up = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))       # noqa: E731
        p = up(pts).to(device=dev, dtype=torch.float32)
        if p.dim() != 2 or p.shape[1] < 3:
            raise ValueError(f"points are rows of x, y, z[, ...], not {tuple(p.shape)}")
        if p.stride(1) != 1 or (p.shape[0] > 1 and p.stride(0) < 3):
            p = p.contiguous()
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
        info, rec, mot, rows = xsensor_labelled(p, rank[inverse].to(torch.int32), up(group), len(host_ids), self.params,
                                                None if dt is None else up(dt), None if motion is None else up(motion), want_rows)
        return XSensorResult(info, rec, mot, rows, host_ids.astype(np.int64), self.sensor_dt)


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def bucket_keys(with_motion: bool) -> list:
    return ["all"] + ([f"speed:{b}" for b in SPEED_BUCKETS] if with_motion else []) + [f"dt:{b}" for b in DT_BUCKETS]


def speed_bucket(speed: float) -> str:
    """static below 0.5 m/s, then 0-10 / 10-20 / 20-30 / 30+ m/s"""
    return SPEED_BUCKETS[0] if speed < STATIC_SPEED else SPEED_BUCKETS[1 + min(int(speed // 10.0), 3)]


def dt_bucket(spread: float) -> str:
    return DT_BUCKETS[0] if spread < 0.010 else DT_BUCKETS[1] if spread <= 0.030 else DT_BUCKETS[2]


def cluster_buckets(g: dict, c: int, with_motion: bool) -> list:
    """the buckets SCORED cluster ``c`` of a glue dict counts in (a cluster without a finite motion row is in no speed bucket)"""
    keys = ["all"]
    if with_motion and not math.isnan(g["speed"][c]):
        keys.append(f"speed:{speed_bucket(float(g['speed'][c]))}")
    keys.append(f"dt:{dt_bucket(float(g['dt_spread'][c]))}")
    return keys


def new_totals(with_motion: bool) -> dict:
    return {"states": [0, 0, 0, 0], "buckets": {k: {"clusters": 0, "queries": 0, "sum_qc": 0, "near": 0, "sum_X": 0.0} for k in bucket_keys(with_motion)}}


def new_against(with_motion: bool) -> dict:
    return {k: {"pairs": 0, "sum_X": 0.0, "sum_X_against": 0.0} for k in bucket_keys(with_motion)}


def tally(totals: dict, g: dict, rec, with_motion: bool) -> None:
    """add the clusters of one call (a glue dict and its ``rec``) to a name's running totals"""
    for s in range(4):
        totals["states"][s] += int((g["state"] == s).sum())
    for c in np.flatnonzero(g["state"] == SCORED):
        for key in cluster_buckets(g, c, with_motion):
            b = totals["buckets"][key]
            b["clusters"] += 1
            b["queries"] += int(g["queries"][c])
            b["sum_qc"] += int(rec[c, :, 2].sum())
            b["near"] += int(rec[c, :, 3].sum())
            b["sum_X"] += float(g["X"][c])


def tally_against(acc: dict, g: dict, keys, g_b: dict, keys_b, with_motion: bool) -> None:
    """``--against``: the clusters SCORED under both names, matched by their (sweep, id) keys; bucketed as under the first name"""
    sc, sc_b = np.flatnonzero(g["state"] == SCORED), np.flatnonzero(g_b["state"] == SCORED)
    _, ia, ib = np.intersect1d(keys[sc], keys_b[sc_b], assume_unique=True, return_indices=True)
    for c, cb in zip(sc[ia], sc_b[ib]):
        for key in cluster_buckets(g, c, with_motion):
            acc[key]["pairs"] += 1
            acc[key]["sum_X"] += float(g["X"][c])
            acc[key]["sum_X_against"] += float(g_b["X"][cb])


def summary(totals: dict, against: dict | None, against_name: str | None) -> dict:
    """the numbers of the table and of ``--json``, per name: the derived values and, under "totals", the raw sums"""
    out = {}
    for name, t in totals.items():
        res = {"states": dict(zip(STATE_NAMES, t["states"])), "buckets": {}, "totals": t}
        for key, b in t["buckets"].items():
            res["buckets"][key] = {"clusters": b["clusters"], "queries": b["queries"], "mean_X": ratio(b["sum_X"], b["clusters"]),
                                   "mean_X_rows": ratio(b["sum_qc"] / float(UNIT), b["queries"]), "near_share": ratio(b["near"], b["queries"])}
        if against is not None:
            res["against"] = {"name": against_name, "buckets": {key: {"pairs": a["pairs"], "ratio": ratio(a["sum_X"], a["sum_X_against"])}
                                                                for key, a in against[name].items()}, "totals": against[name]}
        out[name] = res
    return out


def _table(numbers: dict) -> str:
    lines = []
    for name, r in numbers.items():
        lines.append(f"{name}: clusters " + ", ".join(f"{k} {v}" for k, v in r["states"].items()))
        for key, b in r["buckets"].items():
            line = (f"  {key:<14} {b['clusters']:>7} clusters {b['queries']:>9} rows  X {fmt(b['mean_X'], '.4f')} m  by rows {fmt(b['mean_X_rows'], '.4f')} m  "
                    f"near {fmt(b['near_share'], '.3f')}")
            if "against" in r:
                a = r["against"]["buckets"][key]
                line += f"  / {r['against']['name']} {fmt(a['ratio'], '.3f')} ({a['pairs']} pairs)"
            lines.append(line)
    return "\n".join(lines)


def _ids_host(a, where: str, key: str, rows: int) -> np.ndarray:
    a = np.asarray(a)
    check_point_labels(a, key, where, rows=rows)
    a = a.astype(np.int64)
    if len(a) and (a.min() < 0 or a.max() >= 1 << _ID_BITS):
        raise ValueError(f"{key}: {where} holds an id outside 0..2^{_ID_BITS} - 1")
    return a


def cluster_ids(xyz, gm0, cluster: str = "dbscan", min_cluster_size=None, min_samples=None):
    """``--label_key cluster``: the ids (device int64 [n], 0 = none) of a clustering of one sweep's points ``xyz`` (device float32 [n, 3]):
    the points that are not ground (``gm0``), finite and inside the network's range, clustered as ``ssl_label.cluster_points`` does"""
    import torch
    from .seflow.ssl_label import EPS, HDB_MIN_CLUSTER, HDB_MIN_SAMPLES, MIN_PTS, RANGE_NET, cluster_points
    xyz = xyz.contiguous()
    skip = gm0.bool() | ~torch.isfinite(xyz).all(dim=1) | ~(xyz[:, :2].abs().amax(dim=1) <= RANGE_NET)
    return cluster_points(xyz, skip, cluster, EPS, MIN_PTS, HDB_MIN_CLUSTER if min_cluster_size is None else min_cluster_size,
                          HDB_MIN_SAMPLES if min_samples is None else min_samples)[0].to(torch.int64)


def pack_sweeps(ds, idx, upload, dev, flows, label_key: str):
    """The sweeps ``idx`` of ``ds`` laid end to end on ``dev`` for a per-cluster program: (frames, packed) with ``packed`` = ``offsets``
    (host), ``pc0``, ``lidar_dt``, ``lidar_id``, every stored flow of ``flows`` and ``gm0`` (``label_key`` "cluster") or ``ids``"""
    from .sweeps import SweepPacker
    frames = [ds[i] for i in idx]
    pk = SweepPacker(frames, upload=upload, device=dev)
    packed = {"offsets": pk.offsets_host, "pc0": pk.cat("pc0", np.float32), "lidar_dt": pk.cat("lidar_dt", np.float32),
              "lidar_id": pk.cat("lidar_id", np.uint8)}
    if packed["pc0"].dim() != 2 or packed["pc0"].shape[1] not in (3, 4):
        raise ValueError(f"pc0 is rows of x, y, z[, intensity], not {tuple(packed['pc0'].shape)}")
    for s in flows:
        packed[s] = pk.cat(s, np.float32, width=3)
    if label_key == "cluster":
        packed["gm0"] = pk.cat("gm0", np.uint8)
    else:
        ids = [_ids_host(f[label_key], f"{f['scene_id']}/{f['timestamp']}", label_key, n) for f, n in zip(frames, pk.counts)]
        packed["ids"] = pk.upload(ids, np.int64)
    return frames, packed


def score_batch(scorer: XSensor, engine, frames: list, packed: dict, names: list, label_key: str, motion_key: str | None,
                cluster: str = "dbscan", min_cluster_size=None, min_samples=None):
    """One ``himo_xsensor`` call for the sweeps of ``frames`` under every name of ``names``: the point buffer is the sweeps laid end to
    end once per name (compensated by that name's stored flow through ``CompDisEngine`` with ``refined=True``; ``raw``: as recorded),
    the cluster of sweep s with stored id v under name r has the key ``((r S + s + 1) << 40) | v``.  ``packed``: the batch's device
    tensors (``pc0``, ``lidar_dt``, ``lidar_id``, ``offsets`` on the host, the stored flows, and ``ids`` unless ``label_key`` is
    ``cluster``).  -> (XSensorResult, name index int64 [C], key without the name int64 [C])"""
    import torch
    from .accumulate import flow_motion
    S, off = len(frames), packed["offsets"]
    pc0 = packed["pc0"]
    parts, keys = [], []
    for r, name in enumerate(names):
        for s, f in enumerate(frames):
            lo, hi = int(off[s]), int(off[s + 1])
            rows = pc0[lo:hi]
            if name == "raw":
                pts = rows[:, :3]
            else:
                pts = engine.run_frame(rows, packed[name][lo:hi], packed["lidar_dt"][lo:hi], f["pose0"], f["pose1"], refined=True)[1]
            parts.append(pts)
            if label_key == "cluster":
                ids = cluster_ids(pts, packed["gm0"][lo:hi], cluster, min_cluster_size, min_samples)
            else:
                ids = packed["ids"][lo:hi]
            keys.append(torch.where(ids != 0, ids + ((r * S + s + 1) << _ID_BITS), torch.zeros_like(ids)))
    motion = None
    if motion_key:
        motion = torch.cat([flow_motion(pc0[int(off[s]):int(off[s + 1])], packed[motion_key][int(off[s]):int(off[s + 1])], f["pose0"], f["pose1"])
                            for s, f in enumerate(frames)]).repeat(len(names), 1)
    R = len(names)
    res = scorer.score(torch.cat(parts), torch.cat(keys), packed["lidar_id"].repeat(R), packed["lidar_dt"].repeat(R), motion)
    which = (res.ids >> _ID_BITS) - 1
    return res, which // S, ((which % S) << _ID_BITS) | (res.ids & ((1 << _ID_BITS) - 1))


def main(data_dir: str, res_names, label_key: str, motion_key: str | None = None, against: str | None = None, cluster: str = "dbscan",
         params: XSensorParams | None = None, batch: int = 8, json_path: str | None = None, sensor_dt: float = SENSOR_DT,
         min_cluster_size: int | None = None, min_samples: int | None = None, overlap: bool = True) -> dict:
    """The program: for every sweep of ``data_dir`` and every name of ``res_names`` the cross-sensor distance of every cluster, ``batch``
    sweeps and all names per ``himo_xsensor`` call.  The motion that buckets a cluster by speed is ONE key for all names
    (``motion_key``, default the first stored name of ``res_names``), so a cluster lands in the same bucket under every name; with no
    stored name there is no motion and the speed buckets are omitted.  Writes nothing into the scene files.  Under ``torchrun`` sweep i
    is scored by rank i % world and the totals are gathered.  Returns what ``--json`` writes."""
    from . import distenv, stored
    from .dataset import open_dataset
    from .seflow.ssl_label import CLUSTERINGS
    from .sweeps import MissingKey, fed, raise_missing, sharded_batches
    names = stored.result_names(res_names, raw_ok=True)
    if not label_key:
        raise ValueError("label_key: a stored integer key (ray_label, flow_instance_id, ...) or 'cluster'")
    if against and against not in names:
        raise ValueError(f"--against {against}: not one of --res_names {','.join(names)}")
    if against and label_key == "cluster":
        raise ValueError("--against with --label_key cluster: the clusters are made per name, so no label names the same object under two names")
    if cluster not in CLUSTERINGS:
        raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"batch={batch!r}: at least one sweep a call")
    params = params if params is not None else XSensorParams()
    flows_of = [s for s in names if s != "raw"]
    if motion_key == "raw":
        raise ValueError("--motion_key raw: 'raw' is the zero-motion key, not a stored flow")
    if motion_key is None and flows_of:
        motion_key = flows_of[0]
    with_motion = bool(motion_key)
    flows = list(dict.fromkeys(flows_of + ([motion_key] if motion_key else [])))
    needs = ["lidar_id"] + (["gm0"] if label_key == "cluster" else [label_key])
    sums = {"totals": {s: new_totals(with_motion) for s in names}, "against": {s: new_against(with_motion) for s in names} if against else None}
    with distenv.process_group() as (rank, world):
        ds = open_dataset(Path(data_dir), vis_name=flows, eval=False, fields=tuple(["pc0", "pose0", "pose1", "lidar_dt"] + needs + flows))

        def loop():
            mine = sharded_batches(ds, int(batch))
            # the refusals, before anything touches the GPU
            try:
                for i in (i for b in mine for i in b):
                    where = "/".join(map(str, ds.index[i]))
                    have = stored.present(ds, i, flows + needs)
                    for key, hint in [("lidar_id", "the sensor id per point: the extractors write it")] + \
                            [(s, "--res_names / --motion_key name stored flows; 'raw' needs none") for s in flows] + \
                            [("gm0", "--label_key cluster needs the sweep's ground mask: `python -m himo_amd.ground_seg` writes it")
                             if label_key == "cluster" else (label_key, "`python -m himo_amd.raymap` writes ray_label")]:
                        if key not in have:
                            raise MissingKey(key, [f"[Warning]: No {key} in {where} ({hint}), check the data."])
            except MissingKey as e:
                raise_missing(e)
            if not mine:
                return
            from .compdis import CompDisEngine
            scorer = XSensor(params=params, sensor_dt=sensor_dt)
            engine = CompDisEngine()
            dev = scorer.device

            def build(idx, upload):
                return pack_sweeps(ds, idx, upload, dev, flows, label_key)

            for frames, packed in fed(iter(mine), build, device=dev, overlap=overlap):
                res, which, keys = score_batch(scorer, engine, frames, packed, names, label_key, motion_key, cluster, min_cluster_size,
                                               min_samples)
                g, rec = res.glue, res.rec
                per = {}
                for r, s in enumerate(names):
                    sel = np.flatnonzero(which == r)
                    per[s] = ({k: v[sel] for k, v in g.items()}, rec[sel], keys[sel])
                    tally(sums["totals"][s], per[s][0], per[s][1], with_motion)
                if against:
                    for s in names:
                        tally_against(sums["against"][s], per[s][0], per[s][2], per[against][0], per[against][2], with_motion)

        distenv.run_shard(loop, "its share of the sweeps", closing=(ds,))
        total = distenv.gathered(sums)
        numbers = summary(total["totals"], total["against"], against)
        distenv.report(rank, f"eval_xsensor (cross-sensor consistency, v1; parity unpinned), labels '{label_key}'"
                             f"{', speed from ' + repr(motion_key) if motion_key else ''}:\n{_table(numbers)}", numbers, json_path)
    return numbers


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="per cluster, the distance from every point to the nearest point another sensor recorded: a score "
                                             "that needs no ground truth (cross-sensor consistency, v1; parity unpinned: the reference has no "
                                             "such stage; timed on synthetic sweeps only, profiles/xsensor.txt; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--res_names", required=True, help="comma-separated: 'raw' (the points as recorded) and / or stored flows to compensate by")
    ap.add_argument("--label_key", required=True, help="a stored integer label per point (ray_label, flow_instance_id, ...; 0 = none), or "
                                                       "'cluster': cluster the compensated non-ground in-range points (needs ground_mask)")
    ap.add_argument("--motion_key", default=None, help="the stored flow that buckets every name's clusters by speed (default: the first stored name)")
    ap.add_argument("--against", default=None, metavar="NAME", help="also the ratio of summed X_c to NAME's, over the clusters scored under both")
    ap.add_argument("--cluster", default="dbscan", help="--label_key cluster: 'dbscan' (the default) or 'hdbscan'")
    d = XSensorParams()
    ap.add_argument("--min_group", type=int, default=d.min_group, help="a sensor with fewer usable points in a cluster takes no part there")
    ap.add_argument("--min_points", type=int, default=d.min_points, help="fewer usable points: not scored")
    ap.add_argument("--max_points", type=int, default=d.max_points, help="more usable points: not scored")
    ap.add_argument("--trunc", type=float, default=d.trunc, help="a point's distance is clipped here, metres")
    ap.add_argument("--near", type=float, default=d.near, help="a point at most this far from another sensor's is near, metres")
    ap.add_argument("--batch", type=int, default=8, metavar="SWEEPS", help="sweeps per call")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the table's numbers and the raw totals to PATH")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    return main(a.data_dir, a.res_names, a.label_key, a.motion_key, a.against, a.cluster,
                XSensorParams(trunc=a.trunc, near=a.near, min_group=a.min_group, min_points=a.min_points, max_points=a.max_points), a.batch, a.json)


if __name__ == "__main__":
    _cli()
