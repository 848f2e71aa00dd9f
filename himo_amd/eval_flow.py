"""The scene-flow evaluator: three-way and bucketed end-point error of ``<res_name>`` against the ground-truth ``flow``.

    python -m himo_amd.eval_flow --data_dir D --res_names seflowpp_best,fastnsf,nsfp,icpflow,raw

PARITY UNPINNED.  The reference scores flow in its absent ``OpenSceneFlow`` submodule (``eval.py:21`` imports the tables of
``src.utils.av2_eval``), so there is no source to hold this against.  What runs here is this package's own written rule,
"flow metrics, v1", which follows the published three-way EPE and the Argoverse-2 bucketed normalised EPE; no claim is made about
the numbers the reference's program would print.

The rule.  All arithmetic is IEEE double on the float32 inputs, every operation rounded on its own.  For sweep f with
``T = inv(pose1) @ pose0`` and point i:
  1. counted: the package's evaluation mask (BEV range <= 35 m, not ground, outside the ego box; Scania: ``flow_is_valid`` too).
  2. ``g = gt - pose_flow`` (``pose_flow = T p - p``), ``speed = sqrt((gx gx + gy gy) + gz gz)``.
  3. result r: ``d = est_r - gt`` (``raw``: no estimate, ego motion only: ``d = -g``), ``epe = sqrt((dx dx + dy dy) + dz dz)``.
  4. a counted point whose estimate has a non-finite component or whose ``epe >= 1024 m`` (or is NaN) is *rejected* for r:
     counted in ``rejected[r]``, part of nothing else.
  5. ``q(x) = llrint(x * 2^24)``; every sum is an int64 sum of ``q(epe)`` / ``q(speed)``: the unit is 2^-24 m, and block order,
     batch size and rank count cannot change a digit.
  6. classes 0..4 = BACKGROUND, CAR, OTHER_VEHICLES, PEDESTRIAN, WHEELED_VRU (``eval.BUCKETED_METACATAGORIES``); 5 = every other
     category: foreground, in no bucket.
  7. three-way, per sweep: dynamic = ``speed > 0.5 sensor_dt``; FD / FS = foreground dynamic / static, BS = background static.
     A kind's value is the mean over the sweeps that have such points of the sweep's mean EPE; ``three_way`` the mean of the three.
  8. buckets, over the run: bucket = #{k in 1..50: speed >= k * 0.4 sensor_dt}.  Static EPE of a class = mean EPE of bucket 0;
     dynamic normalised EPE = mean over the occupied buckets b >= 1 of sum(epe) / sum(speed).

Two additions, both PARITY UNPINNED like the rest (this package's own rule, no claim about the absent submodule's numbers):
  3b. residual estimates (``residual=True``): a result may be handed over as its ego-motion-free part ``res`` (float32): the
     network's own output rows, before ``pose_flow`` is added.  Its error is ``d = (double)res - g`` with ``g`` of rule 2; it is
     rejected if a component of ``res`` is non-finite or not ``epe < 1024``.  An all-zero residual is by construction the ``raw``
     result (``d = -g``).
  9. accuracy table, v1 (``accuracy=True``): for every counted, non-rejected point of result r, ``gn = sqrt((gx gx + gy gy) + gz gz)``
     of the STORED ground-truth flow (ego motion included), in double; *strict* iff ``epe < 0.05 || epe < 0.05 * gn``, *relaxed* iff
     ``epe < 0.1 || epe < 0.1 * gn`` (the doubles nearest 0.05 and 0.1, every product rounded once).  Groups: 0 = ALL (every counted
     non-rejected point, class 5 and dynamic background included), 1 = FD, 2 = FS, 3 = BS (rule 7's kinds).  ``accuracy`` int64
     [R][4][3] = (count, strict, relaxed) summed over the run; ``acc_strict[group] = strict / count``, ``acc_relaxed`` likewise, NaN
     where count is 0.
The angle error is not built: an ``acos`` does not round identically on device and host, so it cannot enter integer tables that
must not change a digit.

What runs where: rules 1-6, 3b, 9 and the sums run in one HIP kernel per packed batch of sweeps for up to 8 results at once
(csrc/flowmetrics.hip, ``himo_flow_metrics_batch`` / ``himo_flow_metrics_batch_ex``); the means of rules 7-9 are pure numpy on the
integer tables and work without a GPU (``FlowMetrics.from_counts``).  With ``torch.distributed`` initialised sweep i runs on rank i % world.
"""
from __future__ import annotations

import ctypes
import json
import os
import time

import numpy as np

from . import _lib
from .eval import BUCKETED_METACATAGORIES, CATEGORY_TO_INDEX
from .eval_seg import parse_res_names  # noqa: F401  (parse_res_names is part of this module's interface)
from .sweeps import MissingKey, SweepPacker, fed, raise_missing, sharded_batches, timed

CLASS_NAMES = ("BACKGROUND", "CAR", "OTHER_VEHICLES", "PEDESTRIAN", "WHEELED_VRU")
KINDS = ("FD", "FS", "BS")
MAX_RESULTS = 8                      # HIMO_FLOWM_MAX_RESULTS
CLASSES = len(CLASS_NAMES)           # HIMO_FLOWM_CLASSES
BUCKETS = 51                         # HIMO_FLOWM_BUCKETS
OTHER_FOREGROUND = 5
GROUPS = ("ALL",) + KINDS            # rule 9's groups
UNIT = float(2 ** 24)                # quantisation units per metre


def class_lut() -> np.ndarray:
    """uint8[256]: category index -> 0..4 (``CLASS_NAMES``) | 5 (any other category: foreground, in no bucket)"""
    lut = np.full(256, OTHER_FOREGROUND, dtype=np.uint8)
    seen = set()
    for cid, name in enumerate(CLASS_NAMES):
        idx = [CATEGORY_TO_INDEX[c] for c in BUCKETED_METACATAGORIES[name]]
        if seen & set(idx):
            raise ValueError("the meta-categories of eval.BUCKETED_METACATAGORIES overlap: no single class table stands for them")
        seen |= set(idx)
        lut[idx] = cid
    return lut


def data_name_of(data_dir: str) -> str:
    """the package's substring sniff (``utils.check_valid``: a match at position 0 does not count)"""
    hit = lambda s: str(data_dir).find(s) > 0      # noqa: E731
    if hit("Scania") or hit("scania"):
        return "scania"
    if hit("av2") or hit("AV2"):
        return "av2"
    raise ValueError("Unknown dataset name in data_dir.")


def flow_metrics(buckets, threeway, rejected, offsets, pose0, pose1, pc0, gt, ests, category, ground, valid=None, lut=None,
                 sensor_dt: float = 0.1, scania: bool = False, pose_is_ego: bool = False, workspace=None, accuracy=None,
                 residual: bool = False) -> None:
    """One launch on the current stream: the device int64 tables ``buckets`` [R][5][51][3], ``threeway`` [F][R][3][2] and
    ``rejected`` [R] += the packed batch (``offsets`` int64 [F+1], poses float64 [F][4][4], ``pc0`` float32 [T][S] rows,
    ``gt`` float32 [T][3], ``ests``: R float32 [T][3] tensors or None for ``raw``, ``category`` / ``ground`` / ``valid`` uint8 [T]).
    ``ests`` may be row views of wider buffers (``stride(0) >= 3``, ``stride(1) == 1``, one pitch for all of them): they are read in
    place.  ``accuracy``: the device int64 table [R][4][3] of rule 9, += ; None: not computed.  ``residual``: every estimate is an
    ego-motion-free residual (rule 3b).  Never synchronises."""
    import torch
    from .compdis import CLOSE_DISTANCE_DEFAULT, CLOSE_DISTANCE_THRESHOLD
    if CLOSE_DISTANCE_THRESHOLD != CLOSE_DISTANCE_DEFAULT:
        raise ValueError(f"flow metrics v1 count points within {CLOSE_DISTANCE_DEFAULT:g} m; HIMO_CLOSE_DISTANCE_THRESHOLD is set to another range")
    lib = _lib.load()
    lut = class_lut() if lut is None else np.ascontiguousarray(lut, dtype=np.uint8)
    if lut.shape != (256,):
        raise ValueError("the class table has 256 entries")
    r, n_frames, total = len(ests), int(offsets.numel()) - 1, int(pc0.shape[0])
    if not 1 <= r <= MAX_RESULTS:
        raise ValueError(f"{r} results: himo_flow_metrics_batch takes 1..{MAX_RESULTS}")
    if pc0.dim() != 2 or pc0.shape[1] < 3 or pc0.dtype != torch.float32 or (total and (pc0.stride(1) != 1 or pc0.stride(0) < 3)):
        raise ValueError("pc0 must be float32 rows of at least 3 unit-stride columns")
    pc_stride = int(pc0.stride(0)) if total else int(pc0.shape[1])        # (an empty tensor's strides say nothing)
    for name, t, shape, dtype in ([("gt", gt, (total, 3), torch.float32), ("category", category, (total,), torch.uint8),
                                   ("ground", ground, (total,), torch.uint8), ("buckets", buckets, (r, CLASSES, BUCKETS, 3), torch.int64),
                                   ("threeway", threeway, (n_frames, r, 3, 2), torch.int64), ("rejected", rejected, (r,), torch.int64),
                                   ("pose0", pose0, (n_frames, 4, 4), torch.float64)]
                                  + ([("pose1", pose1, (n_frames, 4, 4), torch.float64)] if pose1 is not None else [])
                                  + ([("valid", valid, (total,), torch.uint8)] if valid is not None else [])
                                  + ([("accuracy", accuracy, (r, len(GROUPS), 3), torch.int64)] if accuracy is not None else [])):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape}, not {t.dtype} {tuple(t.shape)}")
    est_stride = 3
    pitches = set()
    for k, e in enumerate(ests):
        if e is None:
            continue
        if tuple(e.shape) != (total, 3) or e.dtype != torch.float32 or (total and (e.stride(1) != 1 or e.stride(0) < 3)):
            raise ValueError(f"result {k} must be float32 rows of shape {(total, 3)} with unit-stride columns, not {e.dtype} {tuple(e.shape)}")
        if total:
            pitches.add(int(e.stride(0)))
    if len(pitches) > 1:
        raise ValueError(f"the results' rows have different pitches {sorted(pitches)}: one call reads them all at one est_stride")
    if pitches:
        est_stride = pitches.pop()
    if scania and valid is None:
        raise KeyError("flow_is_valid")
    need = int(lib.himo_flow_metrics_workspace_bytes(n_frames))
    if workspace is None:
        workspace = torch.empty(need + 16, dtype=torch.uint8, device=pc0.device)
    if workspace.numel() < need:
        raise ValueError("workspace smaller than himo_flow_metrics_workspace_bytes")
    flags = (_lib.FLAG_SCANIA if scania else 0) | (_lib.FLAG_POSE_IS_EGO if pose_is_ego else 0)
    ptrs = (ctypes.c_void_p * r)(*[_lib.ptr(e) if total else None for e in ests])
    if accuracy is None and not residual and est_stride == 3:
        _lib.check(lib.himo_flow_metrics_batch(
            n_frames, total, _lib.ptr(offsets), _lib.ptr(pose0), _lib.ptr(pose1), _lib.ptr(pc0), pc_stride, _lib.ptr(gt), ptrs, r,
            _lib.ptr(category), _lib.ptr(ground), _lib.ptr(valid), lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), float(sensor_dt), flags,
            _lib.ptr(buckets), _lib.ptr(threeway), _lib.ptr(rejected), _lib.ptr(workspace), _lib.stream_handle()), "himo_flow_metrics_batch")
        return
    flags |= _lib.FLAG_EST_RESIDUAL if residual else 0
    _lib.check(lib.himo_flow_metrics_batch_ex(
        n_frames, total, _lib.ptr(offsets), _lib.ptr(pose0), _lib.ptr(pose1), _lib.ptr(pc0), pc_stride, _lib.ptr(gt), ptrs, r, est_stride,
        _lib.ptr(category), _lib.ptr(ground), _lib.ptr(valid), lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), float(sensor_dt), flags,
        _lib.ptr(buckets), _lib.ptr(threeway), _lib.ptr(rejected), _lib.ptr(accuracy), _lib.ptr(workspace), _lib.stream_handle()),
        "himo_flow_metrics_batch_ex")


class FlowBatch:
    """A packed batch of sweeps on the device (sweep k owns rows ``offsets_host[k]:offsets_host[k + 1]``); ``ests[r]`` is None for
    ``raw``; ``keys[k]`` is sweep k's dataset index."""

    def __init__(self, offsets_host, offsets, pose0, pose1, pc0, gt, ests, category, ground, valid, keys, pose_is_ego=False):
        self.offsets_host, self.offsets, self.pose0, self.pose1, self.pc0, self.gt = offsets_host, offsets, pose0, pose1, pc0, gt
        self.ests, self.category, self.ground, self.valid, self.keys, self.pose_is_ego = ests, category, ground, valid, list(keys), pose_is_ego

    @property
    def sweeps(self) -> int:
        return len(self.offsets_host) - 1

    @property
    def total_points(self) -> int:
        return int(self.offsets_host[-1])

    @classmethod
    def from_device(cls, pc0, gt, ests, category, ground, pose0, pose1=None, valid=None, offsets_host=None, keys=None,
                    pose_is_ego=False) -> "FlowBatch":
        """A batch of tensors that are already resident (a trainer's output: no host trip): ``pc0`` float32 [T][S] rows, ``gt``
        float32 [T][3], ``ests`` as in ``flow_metrics`` (row views allowed), ``category`` / ``ground`` / ``valid`` uint8 [T].  The
        poses may be host arrays ([4][4] or [F][4][4]; 256 bytes a sweep go up) or device float64 tensors.  ``offsets_host``: the
        sweeps' row bounds (default: ONE sweep of all T rows); the device copy is filled without a host copy for one sweep."""
        import torch
        dev = pc0.device
        total = int(pc0.shape[0])
        one = offsets_host is None
        offsets_host = np.array([0, total], dtype=np.int64) if one else np.ascontiguousarray(offsets_host, dtype=np.int64)
        if offsets_host.ndim != 1 or offsets_host.size < 2 or offsets_host[0] != 0 or offsets_host[-1] != total or (np.diff(offsets_host) < 0).any():
            raise ValueError("offsets_host must rise from 0 to the number of rows of pc0")
        if one:
            offsets = torch.zeros(2, dtype=torch.int64, device=dev)
            offsets[1:].fill_(total)
        else:
            offsets = torch.from_numpy(offsets_host).to(dev)
        n = offsets_host.size - 1

        def pose(p):
            if p is None or isinstance(p, torch.Tensor):
                return p
            return torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64).reshape(n, 4, 4)).to(dev)
        return cls(offsets_host, offsets, pose(pose0), pose(pose1), pc0, gt, list(ests), category, ground, valid,
                   keys if keys is not None else range(n), pose_is_ego=pose_is_ego)

    @classmethod
    def from_frames(cls, frames, res_names, device=None, upload=None, keys=None) -> "FlowBatch":
        """``frames``: dicts with ``pc0``, ``pose0``, ``pose1``, ``gm0``, ``flow``, ``flow_category_indices``, every stored name of
        ``res_names`` (``raw`` packs nothing) and, for Scania, ``flow_is_valid`` (packed when every frame has it).  A missing key
        is a ``KeyError``; an array whose length differs from ``pc0``'s raises ``ValueError`` naming the sweep.
        ``upload(parts, dtype)``: the feeder's staging (``feeder.BatchFeeder``); None: one plain copy per array."""
        p = SweepPacker(frames, upload, device)
        cat = p.cat
        return cls(p.offsets_host, p.offsets, p.stack("pose0", np.float64), p.stack("pose1", np.float64),
                   cat("pc0", np.float32), cat("flow", np.float32, 3),
                   [None if name == "raw" else cat(name, np.float32, 3) for name in res_names],
                   cat("flow_category_indices", np.uint8, labels=True), cat("gm0", np.uint8, labels=True),
                   cat("flow_is_valid", np.uint8, labels=True) if all("flow_is_valid" in f for f in p.frames) else None,
                   keys if keys is not None else range(len(p.frames)))


def _nanmean(values) -> float:
    v = [x for x in values if not np.isnan(x)]
    return float(np.mean(v)) if v else float("nan")


class FlowMetrics:
    """The batched evaluator: the integer tables of ``res_names`` -- ``buckets`` int64 [R][5][51][3] (count, sum q(epe),
    sum q(speed)), ``threeway`` {dataset index: int64 [R][3][2]} (count, sum q(epe) of FD, FS, BS) and ``rejected`` int64 [R] --
    fed whole batches of sweeps, and the float64 means made of them.  The three are host views: reading one waits for the
    device and folds its tables in; assigning one replaces the counts.  ``accuracy=True`` adds rule 9's table, ``accuracy`` int64
    [R][4][3] (count, strict, relaxed of ALL, FD, FS, BS), a fourth such view; ``residual=True``: the batches' estimates are
    ego-motion-free residuals (rule 3b)."""

    def __init__(self, res_names, data_name: str, sensor_dt: float = 0.1, device=None, accuracy: bool = False, residual: bool = False):
        self.res_names = parse_res_names(res_names)
        if len(self.res_names) > MAX_RESULTS:
            raise ValueError(f"{len(self.res_names)} result names: at most {MAX_RESULTS} are evaluated in one pass")
        if data_name not in ("av2", "scania"):
            raise ValueError(f"data_name {data_name!r}: 'av2' or 'scania'")
        self.data_name, self.sensor_dt, self.device = data_name, float(sensor_dt), device
        self.with_accuracy, self.residual = bool(accuracy), bool(residual)
        self.lut = class_lut()
        self._dev = self._ws = None
        self.reset()

    @classmethod
    def from_counts(cls, res_names, data_name: str, buckets, threeway, rejected=None, sensor_dt: float = 0.1, accuracy=None) -> "FlowMetrics":
        """the evaluator holding host-set tables (no GPU involved); ``accuracy``: rule 9's table, which turns its means on"""
        m = cls(res_names, data_name, sensor_dt, accuracy=accuracy is not None)
        m.buckets, m.threeway = buckets, threeway
        if accuracy is not None:
            m.accuracy = accuracy
        if rejected is not None:
            m.rejected = rejected
        m.frame_cnt = len(m._threeway)
        return m

    def reset(self) -> None:
        r = len(self.res_names)
        self._buckets = np.zeros((r, CLASSES, BUCKETS, 3), dtype=np.int64)
        self._rejected = np.zeros(r, dtype=np.int64)
        self._accuracy = np.zeros((r, len(GROUPS), 3), dtype=np.int64)
        self._threeway = {}
        self._pending = []                    # (dataset indices, device [F][R][3][2]) of the launches not folded in yet
        if self._dev is not None:
            for t in self._dev:
                t.zero_()
        self.frame_cnt = 0
        self._next_key = 0

    # ---- device side -----------------------------------------------------------------------------------------------
    def add_batch(self, batch: FlowBatch) -> None:
        import torch
        r = len(self.res_names)
        if len(batch.ests) != r:
            raise ValueError(f"the batch packs {len(batch.ests)} results, the evaluator has {r} names")
        if self._dev is None:
            self.device = self.device if self.device is not None else _lib.require_gpu()
            self._dev = (torch.zeros(self._buckets.shape, dtype=torch.int64, device=self.device),
                         torch.zeros(r, dtype=torch.int64, device=self.device)) + \
                        ((torch.zeros(self._accuracy.shape, dtype=torch.int64, device=self.device),) if self.with_accuracy else ())
        need = int(_lib.load().himo_flow_metrics_workspace_bytes(batch.sweeps))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + 16, dtype=torch.uint8, device=self.device)
        tw = torch.zeros((batch.sweeps, r, 3, 2), dtype=torch.int64, device=self.device)
        flow_metrics(self._dev[0], tw, self._dev[1], batch.offsets, batch.pose0, batch.pose1, batch.pc0, batch.gt, batch.ests,
                     batch.category, batch.ground, batch.valid, self.lut, self.sensor_dt, scania=self.data_name == "scania",
                     pose_is_ego=batch.pose_is_ego, workspace=self._ws, accuracy=self._dev[2] if self.with_accuracy else None,
                     residual=self.residual)
        self._pending.append((list(batch.keys), tw))
        self.frame_cnt += batch.sweeps

    def add(self, frames, keys=None) -> None:
        """the sweeps of ``frames`` (host dicts) as one packed batch, one launch; ``keys``: their dataset indices (default: the
        running count of sweeps added)"""
        frames = list(frames)
        if not frames:
            return
        if keys is None:
            keys = range(self._next_key, self._next_key + len(frames))
        keys = [int(k) for k in keys]
        self._next_key = max(self._next_key, max(keys) + 1)
        self.add_batch(FlowBatch.from_frames(frames, self.res_names, device=self.device, keys=keys))

    def _fold(self) -> None:
        if self._dev is not None and self._pending:
            self._buckets = self._buckets + self._dev[0].cpu().numpy()
            self._rejected = self._rejected + self._dev[1].cpu().numpy()
            if self.with_accuracy:
                self._accuracy = self._accuracy + self._dev[2].cpu().numpy()
            for t in self._dev:
                t.zero_()
            for keys, tw in self._pending:
                self._merge_threeway(zip(keys, tw.cpu().numpy()))
            self._pending = []

    def _merge_threeway(self, items) -> None:
        for key, words in items:
            have = self._threeway.get(int(key))
            self._threeway[int(key)] = np.array(words, dtype=np.int64) if have is None else have + words

    # ---- host views ------------------------------------------------------------------------------------------------
    @property
    def buckets(self) -> np.ndarray:
        self._fold()
        return self._buckets

    @buckets.setter
    def buckets(self, value):
        self._fold()
        self._buckets = np.array(value, dtype=np.int64).reshape(self._buckets.shape)

    @property
    def rejected(self) -> np.ndarray:
        self._fold()
        return self._rejected

    @rejected.setter
    def rejected(self, value):
        self._fold()
        self._rejected = np.array(value, dtype=np.int64).reshape(self._rejected.shape)

    @property
    def accuracy(self) -> np.ndarray:
        """int64 [R][4][3]: count, strict, relaxed of ALL, FD, FS, BS (zeros unless the evaluator was built with ``accuracy=True``)"""
        self._fold()
        return self._accuracy

    @accuracy.setter
    def accuracy(self, value):
        self._fold()
        self._accuracy = np.array(value, dtype=np.int64).reshape(self._accuracy.shape)

    @property
    def threeway(self) -> dict:
        """{dataset index: int64 [R][3][2]}, in dataset order"""
        self._fold()
        self._threeway = dict(sorted(self._threeway.items()))
        return self._threeway

    @threeway.setter
    def threeway(self, value):
        self._fold()
        r = len(self.res_names)
        self._threeway = {int(k): np.array(v, dtype=np.int64).reshape(r, 3, 2) for k, v in dict(value).items()}

    def gather(self) -> None:
        """Over the ranks of the process group: ONE all-reduce of the bucket, rejected and (with ``accuracy=True``) accuracy integers and one gather of the per-sweep
        three-way words, which every rank then holds ordered by dataset index.  Integer sums: every rank ends with exactly the
        single-process tables."""
        import torch
        import torch.distributed as dist
        self._fold()
        if not (dist.is_available() and dist.is_initialized()):
            return
        acc = [self._accuracy.reshape(-1)] if self.with_accuracy else []
        t = torch.from_numpy(np.concatenate([self._buckets.reshape(-1), self._rejected] + acc + [[self.frame_cnt]]).astype(np.int64))
        if dist.get_backend() == "nccl":
            t = t.to(torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        flat = t.cpu().numpy()
        nb, nr = self._buckets.size, self._rejected.size
        self._buckets = flat[:nb].reshape(self._buckets.shape).copy()
        self._rejected = flat[nb:nb + nr].copy()
        if self.with_accuracy:
            self._accuracy = flat[nb + nr:-1].reshape(self._accuracy.shape).copy()
        self.frame_cnt = int(flat[-1])
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, sorted(self._threeway.items()))
        self._threeway = {}
        self._merge_threeway(sorted((item for part in parts for item in part), key=lambda kv: kv[0]))

    # ---- rules 7 and 8: float64 on the integers ---------------------------------------------------------------------
    def results(self) -> dict:
        """{name: {"three_way", "FD", "FS", "BS", "static": {class: m}, "dynamic": {class: ratio}, "mean_static", "mean_dynamic",
        "counted", "rejected"}}; a kind or class with nothing counted is nan.  ``counted`` = the points that entered the sums.
        With ``accuracy=True`` also "acc_strict" and "acc_relaxed": {"ALL", "FD", "FS", "BS": strict (relaxed) / count, nan for an
        empty group}."""
        buckets, rejected, threeway = self.buckets, self.rejected, self.threeway
        accuracy = self.accuracy
        out = {}
        for r, name in enumerate(self.res_names):
            tw = np.stack([v[r] for v in threeway.values()]) if threeway else np.zeros((0, 3, 2), dtype=np.int64)
            res = {}
            for k, kind in enumerate(KINDS):
                has = tw[:, k, 0] > 0
                per_sweep = tw[has, k, 1].astype(np.float64) / tw[has, k, 0].astype(np.float64) / UNIT
                res[kind] = float(per_sweep.mean()) if per_sweep.size else float("nan")
            res["three_way"] = float(np.mean([res[k] for k in KINDS]))
            static, dynamic = {}, {}
            for c, cname in enumerate(CLASS_NAMES):
                b = buckets[r, c]
                static[cname] = float(np.float64(b[0, 1]) / np.float64(b[0, 0]) / UNIT) if b[0, 0] > 0 else float("nan")
                has = np.flatnonzero(b[1:, 0] > 0) + 1
                ratios = b[has, 1].astype(np.float64) / b[has, 2].astype(np.float64)
                dynamic[cname] = float(ratios.mean()) if ratios.size else float("nan")
            res["static"], res["dynamic"] = static, dynamic
            res["mean_static"], res["mean_dynamic"] = _nanmean(static.values()), _nanmean(dynamic.values())
            res["counted"] = int(buckets[r, 0, :, 0].sum() + tw[:, :2, 0].sum())
            res["rejected"] = int(rejected[r])
            res = {k: res[k] for k in ("three_way",) + KINDS + ("static", "dynamic", "mean_static", "mean_dynamic", "counted", "rejected")}
            if self.with_accuracy:
                for col, key in ((1, "acc_strict"), (2, "acc_relaxed")):
                    res[key] = {g: float(np.float64(accuracy[r, k, col]) / np.float64(accuracy[r, k, 0])) if accuracy[r, k, 0] > 0 else float("nan")
                                for k, g in enumerate(GROUPS)}
            out[name] = res
        return out

    def table(self) -> str:
        """one text block per result name: the five classes' static EPE [m] and dynamic normalised EPE, then the three-way line
        (and, with ``accuracy=True``, the strict and the relaxed accuracy of ALL, FD, FS, BS)"""
        fmt = lambda v: "-" if np.isnan(v) else f"{v:.6f}"      # noqa: E731
        width = max(len(c) for c in CLASS_NAMES) + 2
        out = []
        for name, res in self.results().items():
            out.append(f"\nFlow metrics (v1) for {name} in {self.data_name}: {self.frame_cnt} sweeps, {res['counted']} points, "
                       f"{res['rejected']} rejected")
            out.append(f"{'':<9}" + "".join(f"{c:>{width}}" for c in CLASS_NAMES) + f"{'mean':>{width}}")
            for row in ("static", "dynamic"):
                out.append(f"{row:<9}" + "".join(f"{fmt(res[row][c]):>{width}}" for c in CLASS_NAMES) + f"{fmt(res['mean_' + row]):>{width}}")
            out.append(f"three-way {fmt(res['three_way'])}  FD {fmt(res['FD'])}  FS {fmt(res['FS'])}  BS {fmt(res['BS'])}")
            if self.with_accuracy:
                for key, label in (("acc_strict", "accuracy strict "), ("acc_relaxed", "accuracy relaxed")):
                    out.append(label + "".join(f"  {g} {fmt(res[key][g])}" for g in GROUPS))
        return "\n".join(out) + "\n"


def merge_json(path, results: dict) -> dict:
    """``{res_name: results}`` merged into the JSON object of ``path`` (created when absent; nan is written as NaN)"""
    data = {}
    if os.path.exists(path):
        try:
            with open(path) as f:
                data = json.load(f)
        except json.JSONDecodeError:
            data = {}
    data.update(results)
    with open(path, "w") as f:
        json.dump(data, f, indent=4)
    return data


def run_dataset(dataset, metrics: FlowMetrics, batch_frames: int = 32, overlap: bool = True) -> int:
    """Shared body of ``main``: sweep i of ``dataset`` on rank i % world, ``batch_frames`` sweeps per launch.  A sweep without
    ``flow`` or ``flow_category_indices`` is skipped with a warning line; one that lacks a stored result name (or another array
    the rule reads) raises ``KeyError`` naming it.  With ``overlap`` the batches are read, packed and copied two ahead by
    ``feeder.BatchFeeder``.  Returns the sweeps this rank evaluated."""
    names = metrics.res_names
    required = ["pc0", "pose0", "pose1", "gm0"] + (["flow_is_valid"] if metrics.data_name == "scania" else []) + [n for n in names if n != "raw"]

    def batches():
        for mine in sharded_batches(dataset, batch_frames):
            frames, keys, lines = [], [], []
            for i in mine:
                f = dataset[i]
                lacking = [k for k in ("flow", "flow_category_indices") if k not in f]
                if lacking:
                    lines += [f"[Warning]: No {k} in {f['scene_id']} at {f['timestamp']}, check the data." for k in lacking]
                    continue
                for key in required:
                    if key not in f:
                        lines.append(f"[Warning]: No {key} in {f['scene_id']} at {f['timestamp']}, check the data.")
                        raise MissingKey(key, lines)
                frames.append(f)
                keys.append(i)
            yield frames, keys, lines

    if overlap and metrics.device is None:
        metrics.device = _lib.require_gpu()

    def build(item, upload):
        frames, keys, lines = item
        return (FlowBatch.from_frames(frames, names, device=metrics.device, upload=upload, keys=keys) if frames else None), lines
    done = 0
    try:
        for batch, lines in fed(batches(), build, device=metrics.device, overlap=overlap):
            for line in lines:
                print(line)
            if batch is not None:
                metrics.add_batch(batch)
                done += batch.sweeps
    except MissingKey as e:
        raise_missing(e)
    return done


def main(data_dir: str = "/home/kin/data/av2/h5py/sensor/himo", res_names="seflowpp_best,raw", data_name: str = "auto",
         batch_frames: int = 32, json_path: str = "", dataset=None, accuracy: bool = False):
    """Evaluate ``res_names`` over the sweeps of ``index_eval.pkl``.  ``data_name``: "av2" | "scania" | "auto" (sniffed from
    ``data_dir``).  Under ``torchrun`` sweep i is counted by rank i % world on its own GPU; rank 0 prints the tables and, with
    ``json_path``, merges ``{res_name: results}`` into that file.  ``accuracy``: rule 9's table too (two more lines per result, two
    more keys in the JSON).  Returns the ``FlowMetrics``."""
    from . import distenv
    from .dataset import FLOW_EVAL_FIELDS, open_dataset

    names = parse_res_names(res_names)
    if data_name == "auto":
        data_name = data_name_of(data_dir)

    def loop():
        t0 = time.perf_counter()
        data = dataset
        if data is None:
            stored = [n for n in names if n != "raw"]
            data = open_dataset(data_dir, vis_name=stored, eval=True, fields=FLOW_EVAL_FIELDS + tuple(stored), zero_copy=True)
        done = run_dataset(data, metrics, batch_frames=batch_frames)
        metrics.buckets                                          # (wait for the device: the loop's time includes its kernels)
        metrics.loop = {"seconds": time.perf_counter() - t0, "sweeps": done}
    with distenv.process_group() as (rank, world):
        metrics = FlowMetrics(names, data_name, accuracy=accuracy)
        distenv.run_shard(loop, "its sweeps, but no table was printed")
        metrics.gather()
        if rank == 0:
            print(metrics.table(), end="")
            if json_path:
                merge_json(json_path, metrics.results())
    return metrics


def _cli(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="three-way and bucketed EPE of <res_name> against the ground-truth flow (MI355X path)")
    ap.add_argument("--data_dir", default="/home/kin/data/av2/h5py/sensor/himo")
    ap.add_argument("--res_names", default="seflowpp_best,raw", help="seflowpp_best,fastnsf,raw  or  \"['seflowpp_best','raw']\"")
    ap.add_argument("--data_name", default="auto", choices=["auto", "av2", "scania"])
    ap.add_argument("--batch_frames", type=int, default=32)
    ap.add_argument("--json", dest="json_path", default="", help="merge {res_name: results} into this JSON file")
    ap.add_argument("--accuracy", action="store_true", help="also the strict / relaxed accuracy table (accuracy table, v1; parity unpinned)")
    a = ap.parse_args(argv)
    return main(a.data_dir, parse_res_names(a.res_names), data_name=a.data_name, batch_frames=a.batch_frames, json_path=a.json_path,
                accuracy=a.accuracy)


if __name__ == "__main__":
    timed(_cli)
