"""Host side of the fused flow -> comp_dis path (stages a1-a6 of SURVEY.md section 8).

Mirrors the body of the reference's per-frame loops (save_zip.py:112-121, eval.py:281-299) but
works on a ragged BATCH of sweeps resident in HBM, because one 120k-point sweep is ~5 MB --
less than a microsecond of HBM time on an MI355X.  The arithmetic is in
himo_amd/csrc/compdis.hip behind the C ABI of include/himo_amd.h.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .sweeps import SweepPacker, host_upload  # noqa: F401  (host_upload: scripts import it from here)

# `CLOSE_DISTANCE_THRESHOLD` comes from the reference's absent OpenSceneFlow submodule (eval.py:21 / save_zip.py:26 import it from
# `src.utils.av2_eval`); 35 m is the Argoverse-2 convention, recorded as unverified in SURVEY.md 0.1.  THIS is the one place the
# product takes it from: the kernels receive it as an argument (`himo_compdis_batch(..., close_dist, ...)`), `eval.py` / `score.py`
# import this name.  The day the value is readable: change this line (or export HIMO_CLOSE_DISTANCE_THRESHOLD), the oracle's copy
# (oracle/himo_oracle.py:31) and the stub in tests/golden/make_golden.py:76, and regenerate the a6 / a7 fixtures.
import os as _os
CLOSE_DISTANCE_DEFAULT = 35.0
CLOSE_DISTANCE_THRESHOLD = float(_os.environ.get("HIMO_CLOSE_DISTANCE_THRESHOLD", str(CLOSE_DISTANCE_DEFAULT)))
if CLOSE_DISTANCE_THRESHOLD != CLOSE_DISTANCE_DEFAULT:       # an exported variable changes every eval.py / save_zip.py figure: say so, once
    import warnings as _warnings
    _warnings.warn(f"HIMO_CLOSE_DISTANCE_THRESHOLD={CLOSE_DISTANCE_THRESHOLD:g} m replaces the default {CLOSE_DISTANCE_DEFAULT:g} m: evaluation masks, "
                   f"metrics and submissions of this process are not comparable with default runs (recorded in res-*.json)", stacklevel=2)
# ego boxes: utils/__init__.py:26 (Scania default) and eval.py:296 (everything else)
EGO_BOX = {
    "scania": ([-9.5, -3 / 2, 0], [5, 2.760004 / 2, 5]),
    "av2": ([-1.5, -1.5, -2.0], [1.5, 1.5, 2.0]),
}


@dataclass
class FrameBatch:
    """Ragged batch of sweeps laid end to end in HBM (frame f owns rows offsets[f]:offsets[f+1])."""
    offsets_host: np.ndarray                 # int64 [F+1]
    offsets: torch.Tensor                    # int64 [F+1]  (device)
    pose0: torch.Tensor                      # float64 [F,4,4]
    pose1: torch.Tensor                      # float64 [F,4,4]
    pc0: torch.Tensor                        # float32 [T,S]
    lidar_dt: torch.Tensor                   # float32 [T]
    flow: torch.Tensor | None = None         # float32 [T,3]  (None => "raw")
    gm0: torch.Tensor | None = None          # uint8 [T]
    flow_is_valid: torch.Tensor | None = None
    category: torch.Tensor | None = None     # uint8 [T]   flow_category_indices (``with_labels``)
    instance: torch.Tensor | None = None     # int32 [T] holding the uint32 bits of flow_instance_id (``with_labels``)
    gt_offsets_host: np.ndarray | None = None  # int64 [F+1] byte offset of every sweep's record-batch body (``with_labels``)
    gt_offsets: torch.Tensor | None = None     # ... on the device, uploaded with the rest of the batch
    f32_chain: bool = False                  # numpy would have computed in float32 (float32 poses)
    pose_is_ego: bool = False                # pose0 holds ego_pose = inv(pose1) @ pose0 computed by numpy (``host_ego``)
    meta: list = field(default_factory=list)  # (scene_id, timestamp) per frame

    @property
    def n_frames(self) -> int:
        return len(self.offsets_host) - 1

    @property
    def total_points(self) -> int:
        return int(self.offsets_host[-1])

    def split(self, t: torch.Tensor) -> list[torch.Tensor]:
        """Per-frame views of a per-point tensor."""
        o = self.offsets_host
        return [t[int(o[i]):int(o[i + 1])] for i in range(self.n_frames)]

    @classmethod
    def from_frames(cls, frames, res_name: str | None = "seflowpp_best", device=None, with_masks: bool = False, upload=None,
                    with_labels: bool = False, host_ego: bool = False):
        """Pack reference-style frame dicts.  ``res_name`` "raw"/None => no flow (save_zip.py:117).
        A missing result key raises ``KeyError`` exactly where the reference's ``data[res_name]`` does.
        ``upload(parts, dtype) -> device tensor`` of the row-wise concatenation of ``parts`` converted to ``dtype``: optional
        staging hook (feeder.EvalFeeder concatenates straight into pinned memory and copies on its own stream).
        ``with_labels``: also ``flow_category_indices`` / ``flow_instance_id``, each when EVERY frame of the batch carries it (the
        ground-truth writer decides per sweep whether a column exists, tools/test/save_zip_gt.py:172-173: it packs one batch per schema).
        ``host_ego``: ``ego_pose = inv(pose1) @ pose0`` of every frame comes from numpy in the poses' own dtype -- the very expression of
        save_zip.py:115, so the 4x4 bits are the reference's and a singular pose raises numpy's ``LinAlgError`` -- instead of the library's
        float64 LU (within 1 ulp of it in the results; ``run_frame`` has the same switch)."""
        p = SweepPacker(frames, upload, device)
        frames, cat, to_dev = p.frames, p.cat, p.upload
        raw = res_name in (None, "raw")
        stride = int(np.asarray(frames[0]["pc0"]).shape[1])
        if host_ego:
            egos = [np.linalg.inv(np.asarray(f["pose1"])) @ np.asarray(f["pose0"]) for f in frames]      # save_zip.py:115
            f32_chain = all(e.dtype == np.float32 for e in egos)
            pose0 = pose1 = to_dev([np.stack([e.astype(np.float64) for e in egos])], np.float64)
        else:
            pose_dtypes = {np.asarray(f[k]).dtype for f in frames for k in ("pose0", "pose1")}
            f32_chain = all(dt == np.float32 for dt in pose_dtypes)
            pose0, pose1 = p.stack("pose0", np.float64), p.stack("pose1", np.float64)
        b = cls(
            offsets_host=p.offsets_host, offsets=p.offsets,
            pose0=pose0, pose1=pose1,
            pc0=cat("pc0", np.float32, stride),
            lidar_dt=cat("lidar_dt", np.float32),
            flow=None if raw else cat(res_name, np.float32, 3),
            f32_chain=f32_chain, pose_is_ego=host_ego,
            meta=[(f.get("scene_id"), f.get("timestamp")) for f in frames],
        )
        if with_masks:
            b.gm0 = cat("gm0", np.uint8)
            if all("flow_is_valid" in f for f in frames):
                b.flow_is_valid = cat("flow_is_valid", np.uint8)
        if with_labels:
            if all("flow_category_indices" in f for f in frames):
                b.category = cat("flow_category_indices", np.uint8)
            if all("flow_instance_id" in f for f in frames):
                b.instance = cat("flow_instance_id", np.int32)             # (the uint32 column's bits: ``astype(np.uint32)`` wraps alike)
            from . import feather
            b.gt_offsets_host = gt_body_offsets(p.offsets_host, feather.gt_schema(b.category is not None, b.instance is not None)[1])
            b.gt_offsets = to_dev([b.gt_offsets_host], np.int64)            # rides in the batch's one upload: no copy at launch time
        return b


def gt_body_offsets(offsets_host, dtypes) -> np.ndarray:
    """int64 [F+1]: where each sweep's record batch body starts in a batch's body buffer (bytes; bodies are multiples of 8)"""
    from . import feather
    out = np.zeros(len(offsets_host), dtype=np.int64)
    for k in range(len(offsets_host) - 1):
        out[k + 1] = out[k] + feather.body_layout(dtypes, int(offsets_host[k + 1] - offsets_host[k]))[0]
    return out


class CompDisEngine:
    """Owns the (tiny) workspace and launches the two kernels of the fused path."""

    def __init__(self, device=None, max_frames: int = 1):
        self.lib = _lib.load()
        self.device = device if device is not None else _lib.require_gpu()
        self._ws = None
        self._reserve(max_frames)

    def _reserve(self, n_frames: int):
        need = int(self.lib.himo_compdis_workspace_bytes(n_frames))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + 64, dtype=torch.uint8, device=self.device)
        return need

    def run(self, batch: FrameBatch, sensor_dt: float = 0.1, refined: bool = False, data_name: str | None = None,
            out: dict | None = None) -> dict:
        """comp_dis (T,3) f32 [+ refined (T,3) f32] [+ eval_mask (T,) uint8 when ``data_name`` is given].
        Asynchronous on the current stream; ``out`` may carry preallocated tensors to reuse."""
        b = batch
        self._reserve(b.n_frames)
        T = b.total_points
        out = {} if out is None else out
        cd = out.get("comp_dis")
        if cd is None:
            cd = out["comp_dis"] = torch.empty((T, 3), dtype=torch.float32, device=self.device)
        rf = None
        if refined:
            rf = out.get("refined")
            if rf is None:
                rf = out["refined"] = torch.empty((T, 3), dtype=torch.float32, device=self.device)
        flags = (_lib.FLAG_F32_CHAIN if b.f32_chain else 0) | (_lib.FLAG_RAW if b.flow is None else 0)
        flags |= _lib.FLAG_POSE_IS_EGO if b.pose_is_ego else 0
        mask = valid = bounds = None
        if data_name is not None:
            if b.gm0 is None:
                raise KeyError("gm0")                                  # eval.py:290 reads data['gm0']
            mask = out.get("eval_mask")
            if mask is None:
                mask = out["eval_mask"] = torch.empty(T, dtype=torch.uint8, device=self.device)
            lo, hi = EGO_BOX["scania" if data_name == "scania" else "av2"]
            bounds = (ctypes.c_float * 6)(*[float(v) for v in lo + hi])
            if data_name == "scania":
                if b.flow_is_valid is None:
                    raise KeyError("flow_is_valid")                    # eval.py:294
                flags |= _lib.FLAG_SCANIA
                valid = b.flow_is_valid
        st = self.lib.himo_compdis_batch(
            b.n_frames, T, _lib.ptr(b.offsets), _lib.ptr(b.pose0), _lib.ptr(b.pose1), _lib.ptr(b.pc0), b.pc0.shape[1],
            _lib.ptr(b.flow), _lib.ptr(b.lidar_dt), float(sensor_dt), flags, _lib.ptr(cd), _lib.ptr(rf), _lib.ptr(mask),
            _lib.ptr(b.gm0), _lib.ptr(valid), bounds, float(CLOSE_DISTANCE_THRESHOLD), _lib.ptr(self._ws),
            self._ws.numel(), _lib.stream_handle())
        _lib.check(st, "himo_compdis_batch")
        return out

    def run_gt(self, batch: FrameBatch, data_name: str, sensor_dt: float = 0.1):
        """The batch's ground-truth sweeps (tools/test/save_zip_gt.py:143-178; ``batch.flow`` is the frames' ``flow``) as Arrow record
        batch BODIES: ``(body, body_offsets, (names, dtypes))`` -- ``body`` a uint8 device tensor, sweep ``k``'s bytes at
        ``body_offsets[k]:body_offsets[k + 1]`` (host int64), laid out as ``feather.framing(names, dtypes, rows)`` says, so that its file
        is ``head + body + tail``.  The label columns exist when the batch carries them.  Asynchronous on the current stream."""
        from . import feather
        b = batch
        if b.flow is None:
            raise KeyError("flow")                                     # save_zip_gt.py:167
        if b.gm0 is None:
            raise KeyError("gm0")                                      # save_zip_gt.py:148
        self._reserve(b.n_frames)
        names, dtypes = feather.gt_schema(b.category is not None, b.instance is not None)
        columns = (_lib.GT_HAS_CATEGORY if b.category is not None else 0) | (_lib.GT_HAS_INSTANCE if b.instance is not None else 0)
        if b.gt_offsets is None:                                       # a batch packed without ``with_labels``
            b.gt_offsets_host = gt_body_offsets(b.offsets_host, dtypes)
            b.gt_offsets = torch.from_numpy(b.gt_offsets_host).to(self.device)
        body_offsets, d_body_offsets = b.gt_offsets_host, b.gt_offsets
        body = torch.empty(max(int(body_offsets[-1]), 8), dtype=torch.uint8, device=self.device)
        flags = (_lib.FLAG_F32_CHAIN if b.f32_chain else 0) | (_lib.FLAG_POSE_IS_EGO if b.pose_is_ego else 0)
        valid = None
        lo, hi = EGO_BOX["scania" if data_name == "scania" else "av2"]
        bounds = (ctypes.c_float * 6)(*[float(v) for v in lo + hi])
        if data_name == "scania":
            if b.flow_is_valid is None:
                raise KeyError("flow_is_valid")                        # save_zip_gt.py:152
            flags |= _lib.FLAG_SCANIA
            valid = b.flow_is_valid
        st = self.lib.himo_compdis_gt_batch(
            b.n_frames, b.total_points, _lib.ptr(b.offsets), _lib.ptr(b.pose0), _lib.ptr(b.pose1), _lib.ptr(b.pc0), b.pc0.shape[1],
            _lib.ptr(b.flow), _lib.ptr(b.lidar_dt), float(sensor_dt), flags, _lib.ptr(b.gm0), _lib.ptr(valid), _lib.ptr(b.category),
            _lib.ptr(b.instance), columns, bounds, float(CLOSE_DISTANCE_THRESHOLD), _lib.ptr(d_body_offsets), _lib.ptr(body),
            _lib.ptr(self._ws), self._ws.numel(), _lib.stream_handle())
        _lib.check(st, "himo_compdis_gt_batch")
        return body[:int(body_offsets[-1])], body_offsets, (names, dtypes)

    def run_frame(self, pc0: torch.Tensor, flow: torch.Tensor | None, lidar_dt: torch.Tensor, pose0, pose1,
                  sensor_dt: float = 0.1, refined: bool = False, host_ego: bool = True):
        """One sweep with host poses -- the loop body of save_zip.py:113-121.

        ``host_ego=True`` computes ``ego_pose = inv(pose1) @ pose0`` with numpy in the poses' own dtype, the
        very expression of save_zip.py:115 (so a singular pose raises numpy's own ``LinAlgError`` and the
        4x4 bits are the reference's); ``False`` leaves the inverse to the library (float64 LU)."""
        self._reserve(1)
        n = pc0.shape[0]
        p0 = np.asarray(pose0)
        p1 = np.asarray(pose1)
        flags = _lib.FLAG_RAW if flow is None else 0
        dptr = ctypes.POINTER(ctypes.c_double)
        if host_ego:
            ego = np.linalg.inv(p1) @ p0                                  # save_zip.py:115
            f32_chain = ego.dtype == np.float32
            a = np.ascontiguousarray(ego, dtype=np.float64).ravel()
            b_ptr = None
            flags |= _lib.FLAG_POSE_IS_EGO
        else:
            f32_chain = p0.dtype == np.float32 and p1.dtype == np.float32
            a = np.ascontiguousarray(p0, dtype=np.float64).ravel()
            b = np.ascontiguousarray(p1, dtype=np.float64).ravel()
            b_ptr = b.ctypes.data_as(dptr)
        flags |= _lib.FLAG_F32_CHAIN if f32_chain else 0
        cd = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        rf = torch.empty((n, 3), dtype=torch.float32, device=self.device) if refined else None
        st = self.lib.himo_compdis_frame(n, a.ctypes.data_as(dptr), b_ptr, _lib.ptr(pc0), pc0.shape[1],
                                         _lib.ptr(flow), _lib.ptr(lidar_dt), float(sensor_dt), flags, _lib.ptr(cd),
                                         _lib.ptr(rf), _lib.ptr(self._ws), self._ws.numel(), _lib.stream_handle())
        _lib.check(st, "himo_compdis_frame")
        return (cd, rf) if refined else cd


_default_engine: CompDisEngine | None = None


def default_engine() -> CompDisEngine:
    global _default_engine
    if _default_engine is None:
        _default_engine = CompDisEngine()
    return _default_engine


def comp_dis_frame(data: dict, res_name: str, sensor_dt: float = 0.1, host_ego: bool = True) -> np.ndarray:
    """Drop-in for the body of the loop at save_zip.py:113-121: frame dict -> (N,3) float32
    ``comp_dis`` as a numpy array (what the reference hands to ``write_output_file``)."""
    eng = default_engine()
    dev = eng.device
    pc0 = torch.from_numpy(np.ascontiguousarray(data["pc0"], dtype=np.float32)).to(dev)
    dt = torch.from_numpy(np.ascontiguousarray(data["lidar_dt"], dtype=np.float32)).to(dev)
    flow = None
    if res_name != "raw":
        flow = torch.from_numpy(np.ascontiguousarray(data[res_name], dtype=np.float32)).to(dev)   # KeyError as the reference
        if flow.shape != (pc0.shape[0], 3):
            raise ValueError(f"operands could not be broadcast together with shapes {tuple(flow.shape)} {(pc0.shape[0], 3)}")
    if dt.shape[0] != pc0.shape[0]:
        raise ValueError(f"operands could not be broadcast together with shapes {(pc0.shape[0], 3)} {tuple(dt.shape)}")
    cd = eng.run_frame(pc0, flow, dt, data["pose0"], data["pose1"], sensor_dt=sensor_dt, host_ego=host_ego)
    return cd.cpu().numpy()
