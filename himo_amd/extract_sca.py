"""Drop-in for the reference's ``dataprocess/extract_sca.py``: raw Scania superframes + annotation boxes + a metadata pickle
-> ``<scene>.h5`` with pseudo-ground-truth ``flow``, ``flow_is_valid``, ``flow_category_indices``, ``flow_instance_id`` and
``ego_motion`` -- the scene files every other program of this package consumes.

Same public names as the reference:
    check_data(pts_filename)                                              extract_sca.py:36-43
    get_pc(pts_filename)                                                  extract_sca.py:45-61
    get_pose_and_timestamp(sequence_meta, frame_idx)                      extract_sca.py:63-73
    process_one(origin_data, output_dir, scene_id, scene_meta)            extract_sca.py:75-235
    main(origin_data, metadata_pkl, output_dir, nproc, create_index_only) extract_sca.py:240-284

The labelling (extract_sca.py:95-145: pose flow, ``mmcv.ops.points_in_boxes_part`` on double tensors, object flow, validity,
classes, instance ids) runs on the device, one launch per batch of sweeps (himo_amd/csrc/boxlabel.hip); the box table it reads is
prepared here in the reference's order (:104-114).  There is no CPU path.

Three things the reference takes from its absent ``OpenSceneFlow`` submodule are not in its tree:
  * ``BOUNDING_BOX_EXPANSION``: 0.2 here (Argoverse 2's value), an UNVERIFIED default; ``HIMO_BOUNDING_BOX_EXPANSION`` overrides it
    (with a warning, as ``HIMO_CLOSE_DISTANCE_THRESHOLD`` does in ``compdis.py``);
  * ``NameMapping``: annotation name -> AV2 category, ``'none'`` included -- a REQUIRED ``--name_mapping`` JSON / YAML file;
  * ``create_reading_index``: its source is absent; ``create_reading_index`` below writes ``index_total.pkl`` in the structure
    ``dataset.HDF5Dataset`` reads and ``tools/pkl_extract.py:5-19`` handles (a list of ``[scene_id, timestamp]`` pairs).
``CATEGORY_TO_INDEX`` is the package's table (``eval_seg.py``).  The extrinsics YAML directory is ``--lidar_ext_dir`` (the
reference's default lies inside the absent submodule).  The membership rule itself is a restatement of mmcv's documented behaviour;
its parity with mmcv's kernel is not pinned.
"""
from __future__ import annotations

import json
import os
import pickle
import threading
import time
import warnings
from pathlib import Path

import numpy as np

from .eval_seg import CATEGORY_TO_INDEX
from .sweeps import SweepPacker, draining, fed, sweep_offsets

BOUNDING_BOX_EXPANSION_DEFAULT = 0.2
BOUNDING_BOX_EXPANSION = float(os.environ.get("HIMO_BOUNDING_BOX_EXPANSION", str(BOUNDING_BOX_EXPANSION_DEFAULT)))
if BOUNDING_BOX_EXPANSION != BOUNDING_BOX_EXPANSION_DEFAULT:      # an exported variable changes every label this process writes: say so, once
    warnings.warn(f"HIMO_BOUNDING_BOX_EXPANSION={BOUNDING_BOX_EXPANSION:g} m replaces the default {BOUNDING_BOX_EXPANSION_DEFAULT:g} m: the "
                  f"scene files of this process are not comparable with default runs", stacklevel=2)

ATTRS = ("X", "Y", "Z", "W", "sensor", "deltaT")
SWEEP_INTERVAL = 0.1                                              # the hard-coded 0.1 s of extract_sca.py:111 and :133


# --------------------------------------------------------------------------------------------------------------------------
# raw reading (extract_sca.py:36-73)
# --------------------------------------------------------------------------------------------------------------------------
def check_data(pts_filename):
    """the first of the six ``<pts_filename>_<attr>.bin`` files that is missing, or None"""
    for attr in ATTRS:
        path = f"{pts_filename}_{attr}.bin"
        if not os.path.isfile(path):
            return path
    return None


def get_pc(pts_filename):
    """([X, Y, Z, W] float32 arrays, sensor ids int8, deltaT in seconds float64 = int32 nanoseconds * 1e-9)"""
    columns, lidar_id, lidar_dt = [], None, None
    for attr in ATTRS:
        path = f"{pts_filename}_{attr}.bin"
        if attr == "sensor":
            lidar_id = np.fromfile(path, np.int8)
        elif attr == "deltaT":
            lidar_dt = np.fromfile(path, np.int32) * 1e-9
        else:
            columns.append(np.fromfile(path, np.float32))
    return columns, lidar_id, lidar_dt


def get_pose_and_timestamp(sequence_meta, frame_idx):
    """(4x4 float64 pose from the smoothed yaw / x / y, int timestamp) of superframe ``frame_idx`` (0-based)"""
    frame = sequence_meta["superframes"][frame_idx]
    smooth = frame["smoothPosition"]
    yaw = float(smooth["smothYaw_rad"])
    pose = np.eye(4)
    pose[:3, :3] = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    pose[0, 3] = float(smooth["smoothX_m"])
    pose[1, 3] = float(smooth["smoothY_m"])
    return pose, int(frame["timestamp_epoch_ns"])


def read_extrinsics(lidar_ext_dir, vehicle: str) -> dict:
    """{lidar name: [x, y, z]} from ``<lidar_ext_dir>/<vehicle>-generated.yml`` (extract_sca.py:167-175; up to ten lidars)"""
    import yaml
    with open(Path(lidar_ext_dir) / f"{vehicle.lower()}-generated.yml") as fh:
        params = yaml.safe_load(fh)["parameters"]
    out = {}
    for k in range(10):
        entry = params.get(f"lidarArray_arrayEl{k}")
        if entry is None:
            continue
        c = entry["nominalPosition"]
        out[entry["humanReadableReference"]] = [c["x"], c["y"], c["z"]]
    return out


def sensors_center(lidar_id, sequence_meta, extrinsics) -> np.ndarray:
    """[n lidars present, 3]: the centre of every sensor id of the sweep, in ``np.unique`` order (extract_sca.py:191-194)"""
    return np.array([extrinsics[sequence_meta["lidars"][f"lidar{k - 1}"]["name"]] for k in np.unique(lidar_id)])


def load_name_mapping(path) -> dict:
    """annotation name -> AV2 category from a JSON or YAML file; must name ``'none'`` and map into ``CATEGORY_TO_INDEX``"""
    if path is None:
        raise ValueError("--name_mapping is required: the reference's NameMapping lives in its absent OpenSceneFlow submodule")
    text = Path(path).read_text()
    if str(path).endswith((".yml", ".yaml")):
        import yaml
        mapping = yaml.safe_load(text)
    else:
        mapping = json.loads(text)
    if not isinstance(mapping, dict) or "none" not in mapping:
        raise ValueError(f"{path}: a name mapping is a dict that also maps 'none'")
    unknown = sorted({str(v) for v in mapping.values()} - set(CATEGORY_TO_INDEX))
    if unknown:
        raise ValueError(f"{path}: not AV2 categories: {unknown}")
    return {str(k): str(v) for k, v in mapping.items()}


# --------------------------------------------------------------------------------------------------------------------------
# the box table (extract_sca.py:104-114, :120-140 per box instead of per point)
# --------------------------------------------------------------------------------------------------------------------------
def prepared_boxes(annos, expansion: float | None = None) -> np.ndarray:
    """float64 [M,7] ``(cx, cy, cz_bottom, dx, dy, dz, rz)``: what the reference hands to ``points_in_boxes_part``.  The
    arithmetic runs in the annotations' own dtype in the reference's order, then widens (its ``.double()``)."""
    e = BOUNDING_BOX_EXPANSION if expansion is None else expansion
    box = np.concatenate([np.asarray(annos["location"]), np.asarray(annos["dimensions"]),
                          np.asarray(annos["heading"]).reshape(-1, 1)], axis=1)
    box[:, 2] -= box[:, 5] / 2                                     # :105 centre -> ground, by half the UNEXPANDED height
    speed = np.asarray(annos["speed"]).reshape(-1)
    finite = speed != np.inf
    box[finite, 3] += speed[finite] * SWEEP_INTERVAL * 2 + e       # :111 along the heading, where the speed is finite
    box[:, 4] += 0.4                                               # :113
    box[:, 5] += e                                                 # :114
    return box.astype(np.float64)


def box_geometry(boxes: np.ndarray) -> np.ndarray:
    """float64 [M,8] cx, cy, cz_centre, dx/2, dy/2, dz/2, cos(-rz), sin(-rz): the constants of the membership rule, so that
    no device transcendental takes part in a decision"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    g = np.empty((len(b), 8), dtype=np.float64)
    g[:, 0], g[:, 1] = b[:, 0], b[:, 1]
    g[:, 5] = b[:, 5] / 2.0
    g[:, 2] = b[:, 2] + g[:, 5]
    g[:, 3], g[:, 4] = b[:, 3] / 2.0, b[:, 4] / 2.0
    g[:, 6], g[:, 7] = np.cos(-b[:, 6]), np.sin(-b[:, 6])
    return g


def class_bytes(names, name_mapping: dict) -> np.ndarray:
    return np.array([CATEGORY_TO_INDEX[name_mapping[n]] for n in names], dtype=np.uint8).reshape(-1)


def box_table(annos, name_mapping: dict, expansion: float | None = None):
    """(geometry f64 [M,8], object flow f32 [M,3], class u8 [M], velocity-is-finite u8 [M]) of one annotated frame"""
    geom = box_geometry(prepared_boxes(annos, expansion))
    vel = np.asarray(annos["velocity"]).reshape(-1, 2)
    vel3 = np.hstack([vel, np.zeros(len(vel)).reshape(-1, 1)])                  # :121
    infinite = np.isinf(vel3).any(axis=1)                                        # :125
    vel3[infinite, :] = 0.0                                                      # :126
    obj_flow = (vel3 * SWEEP_INTERVAL).astype(np.float32)                        # :133-134
    names = [n for n in annos["name"]][:len(vel)]                                # (the reference appends 'none' to this list: :137)
    return geom, obj_flow, class_bytes(names, name_mapping), (~infinite).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------------
# the device half
# --------------------------------------------------------------------------------------------------------------------------
class LabelBatch:
    """A packed, ragged batch of sweeps and their box rows on the device (``upload(parts, dtype)`` as ``FrameBatch``)."""

    def __init__(self, sweeps, background: int, device=None, upload=None):
        """``sweeps``: [(pc f32 [N,4], ego1_SE3_ego0 f64 [4,4] or [3,4], (geom, obj_flow, cls, vel_finite))]"""
        p = SweepPacker([{"pc": pc, "ego": np.asarray(ego, dtype=np.float64)[:3, :4], "scene_id": "sweep", "timestamp": k}
                         for k, (pc, ego, _) in enumerate(sweeps)], upload, device, count_key="pc")
        up = p.upload
        self.n = len(sweeps)
        self.background = int(background)
        self.offsets_host, self.offsets = p.offsets_host, p.offsets
        self.box_offsets_host = sweep_offsets(len(t[0]) for _, _, t in sweeps).astype(np.int32)
        self.box_offsets = up([self.box_offsets_host], np.int32)
        self.ego = p.stack("ego", np.float64)
        self.pc = p.cat("pc", np.float32, 4)
        self.geom = up([t[0].reshape(-1, 8) for _, _, t in sweeps], np.float64)
        self.obj_flow = up([t[1].reshape(-1, 3) for _, _, t in sweeps], np.float32)
        self.box_class = up([t[2] for _, _, t in sweeps], np.uint8)
        self.vel_finite = up([t[3] for _, _, t in sweeps], np.uint8)

    @property
    def total_points(self) -> int:
        return int(self.offsets_host[-1])


def out_layout(total: int):
    """byte offsets of (flow, instance, valid, category) inside one output buffer, and its size: 16-byte aligned columns"""
    def up16(v):
        return (v + 15) // 16 * 16
    at_flow = 0
    at_inst = up16(at_flow + 12 * total)
    at_valid = up16(at_inst + 4 * total)
    at_cat = up16(at_valid + total)
    return (at_flow, at_inst, at_valid, at_cat), max(up16(at_cat + total), 16)


def label_batch(batch: LabelBatch, out=None):
    """Launch ``himo_box_label_batch`` on the current stream: a uint8 device buffer laid out by ``out_layout`` (one device ->
    host copy carries all four columns).  Asynchronous."""
    import torch
    from . import _lib
    lib = _lib.load()
    T = batch.total_points
    (a_flow, a_inst, a_valid, a_cat), size = out_layout(T)
    if out is None:
        out = torch.empty(size, dtype=torch.uint8, device=batch.pc.device)
    base = out.data_ptr()
    st = lib.himo_box_label_batch(
        batch.n, T, batch.offsets_host.ctypes.data, _lib.ptr(batch.offsets), _lib.ptr(batch.ego), _lib.ptr(batch.pc),
        int(batch.box_offsets_host[-1]), batch.box_offsets_host.ctypes.data, _lib.ptr(batch.box_offsets), _lib.ptr(batch.geom),
        _lib.ptr(batch.obj_flow), _lib.ptr(batch.box_class), _lib.ptr(batch.vel_finite), batch.background,
        base + a_flow, base + a_valid, base + a_cat, base + a_inst, _lib.stream_handle())
    _lib.check(st, "himo_box_label_batch")
    return out


def split_outputs(host: np.ndarray, offsets_host: np.ndarray) -> list:
    """per sweep (flow f32 [N,3], valid bool [N], category u8 [N], instance u32 [N]) views of a host copy of the output buffer"""
    T = int(offsets_host[-1])
    (a_flow, a_inst, a_valid, a_cat), _ = out_layout(T)
    flow = host[a_flow:a_flow + 12 * T].view(np.float32).reshape(T, 3)
    inst = host[a_inst:a_inst + 4 * T].view(np.uint32)
    valid = host[a_valid:a_valid + T]
    cat = host[a_cat:a_cat + T]
    out = []
    for k in range(len(offsets_host) - 1):
        lo, hi = int(offsets_host[k]), int(offsets_host[k + 1])
        out.append((flow[lo:hi], valid[lo:hi].astype(bool), cat[lo:hi], inst[lo:hi]))
    return out


class GroundBatch:
    """Every sweep of a batch -- also the ones without labels -- packed for the ground segmenter (``himo_amd/ground_seg.py``;
    parity with the reference's own segmenter unpinned), uploaded with the batch that labels the boxes."""

    def __init__(self, pcs, params, device=None, upload=None):
        p = SweepPacker([{"pc": pc} for pc in pcs], upload, device, count_key="pc")
        self.params, self.offsets_host, self.offsets, self.pc = params, p.offsets_host, p.offsets, p.cat("pc", np.float32)

    @property
    def total_points(self) -> int:
        return int(self.offsets_host[-1])


def ground_batch(gb: GroundBatch, mask=None):
    """Launch ``himo_ground_seg_batch`` on the current stream: the uint8 device mask of every point of ``gb``.  Asynchronous."""
    from .ground_seg import segment_batch
    return segment_batch(gb.pc, gb.offsets_host, gb.offsets, gb.params, mask=mask)


def label_sweeps(sweeps, background: int, device=None) -> list:
    """``compute_flow`` of extract_sca.py:95-145 for a list of sweeps, synchronously: per sweep (flow, valid, category, instance)"""
    import torch
    if not sweeps:
        return []
    batch = LabelBatch(sweeps, background, device=device)
    out = label_batch(batch)
    torch.cuda.synchronize()
    return split_outputs(out.cpu().numpy(), batch.offsets_host)


# --------------------------------------------------------------------------------------------------------------------------
# scene planning, reading and writing (extract_sca.py:147-235)
# --------------------------------------------------------------------------------------------------------------------------
_H5_LOCK = threading.Lock()          # the HDF5 C library is not re-entrant: planning (feeder thread) and writing (drain thread) take turns


def _h5():
    """the module whose ``File(path, mode)`` writes scene files: ``h5py`` when importable, else the HDF5 C library (``h5c``)"""
    try:
        import h5py
        return h5py
    except ImportError:
        from . import h5c
        h5c.load()
        return h5c


def superframes_of(origin_data, scene_id) -> list:
    return sorted(d for d in os.listdir(os.path.join(origin_data, scene_id)) if d.startswith("superframe_"))


def scene_plan(origin_data, output_dir, scene_id, scene_meta, lidar_ext_dir):
    """What ``process_one`` will do for a scene, decided before any point is read: None when the scene is skipped (its h5 already
    holds one group per superframe, or it has no sequence JSON: :157-164), else ``(sequence_meta, extrinsics, jobs)`` with one job
    ``(group name, points file stem, 0-based frame index, successor's frame index or None, annotations or None)`` per superframe up
    to the first one with a missing ``.bin`` file (the reference's ``break``).  Like the reference it opens ``<scene>.h5`` for
    appending first, so a skipped scene without a file leaves an empty one."""
    frames = superframes_of(origin_data, scene_id)
    with _H5_LOCK, _h5().File(Path(output_dir) / f"{scene_id}.h5", "a") as f:
        done = len(f.keys()) == len(frames)
    if done:
        print(f"{scene_id} already exist, skip. and the total timestamp is correct.")
        return None
    meta_json = os.path.join(origin_data, scene_id, f"sequence_{int(scene_id.split('_')[1])}.json")
    if not os.path.exists(meta_json):
        print(f"{scene_id} has no meta file, skip.")
        return None
    with open(meta_json) as fh:
        sequence_meta = json.load(fh)
    if lidar_ext_dir is None:
        raise ValueError("--lidar_ext_dir is required: the reference reads the extrinsics from its absent OpenSceneFlow submodule")
    extrinsics = read_extrinsics(lidar_ext_dir, sequence_meta["vehicle"])
    jobs = []
    for i, one in enumerate(frames):
        stem = os.path.join(origin_data, scene_id, one, one)
        lack = check_data(stem)
        if lack is not None:
            print(f"{scene_id} has no data file: {lack}")
            break
        idx = int(one.split("_")[-1]) - 1                              # :184 the JSON is 0-based, superframe_* names are 1-based
        if i >= len(scene_meta) - 1:                                   # :200 the last annotated frame (and any after it): no flow
            jobs.append((one.split("_")[-1], stem, idx, None, None))
            continue
        nxt = frames[i + 1]
        lack = check_data(os.path.join(origin_data, scene_id, nxt, nxt))
        if lack is not None:
            print(f"{scene_id} has no data file: {lack}")
            break
        jobs.append((one.split("_")[-1], stem, idx, int(nxt.split("_")[-1]) - 1, scene_meta[i]["annos"]))
    return sequence_meta, extrinsics, jobs


def read_sweep(job, sequence_meta, extrinsics, name_mapping) -> dict:
    """one superframe from disk (a reader worker): its arrays, pose, and -- for an annotated frame with a successor -- the
    transform and box table the device needs"""
    group, stem, idx, idx1, annos = job
    columns, lidar_id, lidar_dt = get_pc(stem)
    pc = np.array(columns).T                                           # [N,4]
    pose, timestamp = get_pose_and_timestamp(sequence_meta, idx)
    rec = {"group": group, "pc": np.ascontiguousarray(pc, dtype=np.float32), "lidar_id": lidar_id, "lidar_dt": lidar_dt,
           "SensorsCenter": sensors_center(lidar_id, sequence_meta, extrinsics), "pose": pose, "timestamp": timestamp, "label": None}
    if annos is not None:
        pose1, _ = get_pose_and_timestamp(sequence_meta, idx1)
        ego = np.linalg.inv(pose1) @ pose                              # cal_pose0to1Numpy (absent submodule; save_zip.py:115's expression)
        rec["label"] = (ego, box_table(annos, name_mapping))
    return rec


def write_group(f, rec, labels=None, ground=None) -> None:
    """one superframe's group with the dataset names, dtypes and conditions of extract_sca.py:76-93, :200-235"""
    g = f.create_group(rec["group"])
    g.create_dataset("lidar", data=rec["pc"].astype(np.float32))
    g.create_dataset("lidar_id", data=rec["lidar_id"].astype(np.uint8))
    g.create_dataset("lidar_dt", data=rec["lidar_dt"].astype(np.float32))
    g.create_dataset("SensorsCenter", data=rec["SensorsCenter"].astype(np.float32))
    pose = rec["pose"] if labels is None else rec["pose"].astype(np.float32)    # :232 a labelled frame's pose passes through float32
    g.create_dataset("pose", data=pose.astype(np.float64))
    g.create_dataset("timestamp", data=np.asarray(rec["timestamp"], dtype=np.int64))
    if labels is not None:
        flow, valid, cat, inst = labels
        g.create_dataset("flow", data=np.asarray(flow, dtype=np.float32))
        g.create_dataset("flow_is_valid", data=np.asarray(valid).astype(bool))
        g.create_dataset("flow_category_indices", data=np.asarray(cat).astype(np.uint8))
        g.create_dataset("flow_instance_id", data=np.asarray(inst).astype(np.uint32))
        g.create_dataset("ego_motion", data=rec["label"][0].astype(np.float32))  # :234
    if ground is not None:                                             # (--ground_mask: not one of the reference extractor's datasets)
        g.create_dataset("ground_mask", data=np.asarray(ground).astype(bool))


def process_one(origin_data, output_dir: Path, scene_id, scene_meta, lidar_ext_dir=None, name_mapping=None, ground_params=None):
    """One scene, serially: plan, read every superframe, label the annotated ones in ONE launch, write ``<scene_id>.h5``.
    ``ground_params`` (a ``ground_seg.GroundParams``): also write every sweep's ``ground_mask``."""
    plan = scene_plan(origin_data, output_dir, scene_id, scene_meta, lidar_ext_dir)
    if plan is None:
        return
    if not isinstance(name_mapping, dict):
        name_mapping = load_name_mapping(name_mapping)
    sequence_meta, extrinsics, jobs = plan
    recs = [read_sweep(j, sequence_meta, extrinsics, name_mapping) for j in jobs]
    todo = [r for r in recs if r["label"] is not None]
    background = CATEGORY_TO_INDEX[name_mapping["none"]]
    labels = iter(label_sweeps([(r["pc"], r["label"][0], r["label"][1]) for r in todo], background))
    ground = [None] * len(recs)
    if ground_params is not None and recs:
        from .ground_seg import ground_masks
        ground = ground_masks([r["pc"] for r in recs], ground_params)
    with _h5().File(Path(output_dir) / f"{scene_id}.h5", "a") as f:
        for r, gm in zip(recs, ground):
            write_group(f, r, next(labels) if r["label"] is not None else None, gm)


def create_reading_index(output_dir) -> list:
    """``index_total.pkl``: the sorted list of ``[scene_id, timestamp]`` pairs (group names) of every ``*.h5`` under ``output_dir``.
    The reference's function of this name lives in its absent OpenSceneFlow submodule; this writes the structure
    ``dataset.load_index`` reads and ``tools/pkl_extract.py:5-19`` iterates."""
    from .dataset import h5_reader
    output_dir = Path(output_dir)
    index = []
    for path in sorted(output_dir.glob("*.h5")):
        with h5_reader().File(path, "r") as f:
            index.extend([path.stem, str(k)] for k in sorted(f.keys()))
    with open(output_dir / "index_total.pkl", "wb") as fh:
        pickle.dump(index, fh)
    return index


def select_scenes(origin_data, metadata) -> list:
    """[(scene_id, its metadata entries)] of the ``*batch*`` folders that have any (extract_sca.py:257-268)"""
    out = []
    for scene_id in sorted(os.listdir(origin_data)):
        if not os.path.isdir(os.path.join(origin_data, scene_id)) or "batch" not in scene_id:
            continue
        meta = [m for m in metadata if m["sample_idx"] == scene_id]
        if meta:
            out.append((scene_id, meta))
    return out


def run_scenes(scenes, origin_data, output_dir, lidar_ext_dir, name_mapping: dict, nproc: int = 4, batch_sweeps: int = 32,
               ground_params=None) -> int:
    """The program's loop: ``nproc`` reader threads read superframes ahead (``np.fromfile`` releases the interpreter lock), sweeps
    of consecutive scenes are packed ``batch_sweeps`` at a time (``feeder.BatchFeeder`` stages and uploads two batches ahead), each
    batch is ONE launch, and its four columns come back as one copy through ``feeder.ResultDrain`` to a writer thread that appends
    the groups in order (one writer: the HDF5 library serialises its calls anyway).  Returns the sweeps written.
    ``ground_params``: the batch also carries ALL its sweeps packed for the ground segmenter (the labelled ones a second time: the
    labelling kernel wants them contiguous), the masks are computed on the same stream right after the labels and come back in the
    same copy, behind the four label columns."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from . import _lib
    from .feeder import ResultDrain
    dev = _lib.require_gpu()
    background = CATEGORY_TO_INDEX[name_mapping["none"]]
    readers = ThreadPoolExecutor(max_workers=max(1, int(nproc)), thread_name_prefix="himo-sca-read")
    ahead = max(2 * batch_sweeps, 2 * int(nproc))

    def records():
        pending = deque()
        for scene_id, meta in scenes:
            plan = scene_plan(origin_data, output_dir, scene_id, meta, lidar_ext_dir)
            if plan is None:
                continue
            sequence_meta, extrinsics, jobs = plan
            for k, job in enumerate(jobs):
                pending.append((scene_id, k == len(jobs) - 1, readers.submit(read_sweep, job, sequence_meta, extrinsics, name_mapping)))
                while len(pending) >= ahead:
                    s, last, fut = pending.popleft()
                    yield s, last, fut.result()
        while pending:
            s, last, fut = pending.popleft()
            yield s, last, fut.result()

    def batches():
        group = []
        for item in records():
            group.append(item)
            if len(group) == batch_sweeps:
                yield group
                group = []
        if group:
            yield group

    def build(group, upload):
        todo = [r for _, _, r in group if r["label"] is not None]
        batch = LabelBatch([(r["pc"], r["label"][0], r["label"][1]) for r in todo], background, device=dev, upload=upload) if todo else None
        gb = GroundBatch([r["pc"] for _, _, r in group], ground_params, device=dev, upload=upload) if ground_params is not None else None
        return group, batch, gb

    files = {}
    written = [0]

    def sink(key, host):                                               # (the writer thread; ``host`` is a view of a pinned buffer)
        group, offsets_host, ground_offsets = key
        labels = iter(split_outputs(host, offsets_host)) if offsets_host is not None else iter(())
        at_ground = out_layout(int(offsets_host[-1]))[1] if offsets_host is not None else 0
        for k, (scene_id, last, rec) in enumerate(group):
            gm = None
            if ground_offsets is not None:
                gm = host[at_ground + int(ground_offsets[k]):at_ground + int(ground_offsets[k + 1])]
            with _H5_LOCK:
                f = files.get(scene_id)
                if f is None:
                    f = files[scene_id] = _h5().File(Path(output_dir) / f"{scene_id}.h5", "a")
                write_group(f, rec, next(labels) if rec["label"] is not None else None, gm)
                if last:
                    files.pop(scene_id).close()
            written[0] += 1

    drain = ResultDrain(sink, device=dev, threads=1, copy=False)
    feed = fed(batches(), build, device=dev)
    try:
        with draining(feed, drain):
            for group, batch, gb in feed:
                size = out_layout(batch.total_points)[1] if batch is not None else 0
                extra = gb.total_points if gb is not None else 0
                out = torch.empty(max(size + extra, 16), dtype=torch.uint8, device=dev)
                if batch is not None:
                    label_batch(batch, out)
                if gb is not None and extra:
                    ground_batch(gb, out[size:size + extra])
                drain.put((group, batch.offsets_host if batch is not None else None, gb.offsets_host if gb is not None else None), out)
    finally:
        readers.shutdown(wait=False, cancel_futures=True)
    for f in files.values():
        f.close()
    return written[0]


def main(origin_data: str = "/home/kin/data/Scania/val", metadata_pkl: str = "/home/kin/data/Scania/scania_pseudo_infos.pkl",
         output_dir: str = "/home/kin/data/Scania/preprocess/val_debuging", nproc: int = 4, create_index_only: bool = False,
         lidar_ext_dir: str | None = None, name_mapping: str | None = None, batch_sweeps: int = 32, ground_mask: bool = False,
         sensor_height: float = 0.0):
    """extract_sca.py:240-284.  Under ``torchrun`` (one rank per GPU) the scenes are sharded i % world, every rank writes its own
    scene files, and rank 0 writes the index once all of them are on disk.  ``ground_mask``: also write every sweep's
    ``ground_mask`` (``himo_amd/ground_seg.py``, with ``sensor_height``); off by default, so the output is the reference's."""
    from . import distenv
    if create_index_only:
        create_reading_index(Path(output_dir))
        return
    mapping = name_mapping if isinstance(name_mapping, dict) else load_name_mapping(name_mapping)
    with open(metadata_pkl, "rb") as f:
        metadata = pickle.load(f)
    Path(output_dir).mkdir(parents=True, exist_ok=True)
    scenes = select_scenes(origin_data, metadata)
    with distenv.process_group() as (rank, world):
        mine = scenes[rank::world]
        print(f"Using {nproc} readers for creating {len(mine)} of {len(scenes)} scene.")

        def loop():
            ground_params = None
            if ground_mask:
                from .ground_seg import GroundParams
                ground_params = GroundParams(sensor_height=sensor_height)
            run_scenes(mine, origin_data, output_dir, lidar_ext_dir, mapping, nproc=nproc, batch_sweeps=batch_sweeps, ground_params=ground_params)
        distenv.run_shard(loop, "its scene files, but no index was written")
        if rank == 0:
            create_reading_index(Path(output_dir))
        if world > 1:
            distenv.all_ranks_ok(True)                                 # nobody leaves before the index exists


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="raw Scania superframes + boxes + metadata pickle -> <scene>.h5 with pseudo ground truth (MI355X path)")
    ap.add_argument("--origin_data", default="/home/kin/data/Scania/val")
    ap.add_argument("--metadata_pkl", default="/home/kin/data/Scania/scania_pseudo_infos.pkl")
    ap.add_argument("--output_dir", default="/home/kin/data/Scania/preprocess/val_debuging")
    ap.add_argument("--nproc", type=int, default=4, help="reader threads that read superframes ahead of the device")
    ap.add_argument("--create_index_only", action="store_true")
    ap.add_argument("--lidar_ext_dir", default=None, help="directory of the <vehicle>-generated.yml extrinsics files")
    ap.add_argument("--name_mapping", default=None, help="JSON / YAML file: annotation name -> AV2 category, 'none' included (required)")
    ap.add_argument("--batch_sweeps", type=int, default=32, help="sweeps per launch")
    ap.add_argument("--ground_mask", action="store_true",
                    help="also write <timestamp>/ground_mask for every sweep (himo_amd.ground_seg's rule; parity with the reference's "
                         "segmenter unpinned); off by default: the output is then the reference extractor's")
    ap.add_argument("--sensor_height", type=float, default=0.0,
                    help="with --ground_mask: the ground is expected at z = -sensor_height; the default 0.0 is an UNVERIFIED assumption "
                         "about the Scania vehicle frame")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.origin_data, a.metadata_pkl, a.output_dir, a.nproc, a.create_index_only, a.lidar_ext_dir, a.name_mapping, a.batch_sweeps, a.ground_mask,
         a.sensor_height)


if __name__ == "__main__":
    start_time = time.time()
    _cli()
    print(f"\nRunning {__file__} used: {(time.time() - start_time) / 60:.2f} mins")
