"""Generate the Scania extractor's fixtures by RUNNING THE REFERENCE'S OWN ``dataprocess/extract_sca.py``.

Run once in the build container (needs /root/reference and libhdf5; never runs on the GPU box):

    python tests/golden/make_extract_golden.py

What it does
  * writes a synthetic raw tree under ``tests/golden/sca/raw/``: two scenes (``batch_11``, ``batch_12``) of four superframes
    with six lidars, 8-20 annotation boxes per annotated frame -- overlapping pairs, rotated boxes, one box per scene whose speed
    and velocity are infinite, one frame with a single box -- the sequence JSONs, ``metadata.pkl`` and, beside it,
    ``lidar_ext/testtruck-generated.yml`` and ``name_mapping.json``.  ``batch_12`` has three annotated frames for four
    superframes (two frames without flow).  Superframes hold 1.0-2.3 k points rather than 2-3 k each, so that a scene's h5
    (39 bytes a labelled point) stays under the 250 KB every committed fixture keeps to;
  * imports ``dataprocess/extract_sca.py`` unmodified, with only what is missing stubbed: ``fire``; ``h5py`` (``File`` served by
    ``himo_amd.h5c``, the C library h5py wraps); ``dataprocess.misc_data`` (``cal_pose0to1Numpy = inv(pose1) @ pose0``, a
    recording ``create_reading_index``); ``src.utils.av2_eval`` (``CATEGORY_TO_INDEX`` of ``himo_amd.eval_seg``, the committed
    name mapping, ``BOUNDING_BOX_EXPANSION = 0.2``); ``mmcv.ops.points_in_boxes_part`` (the float64 restatement of
    ``tests/boxlabel_ref.py``, which records the points and boxes it is handed); the module's ``BASE_DIR`` pointed at a
    temporary tree that holds the extrinsics YAML where :167 looks for it;
  * runs ``main(nproc=1)`` and stores the h5 files the reference wrote (``sca/h5/``) and the box tensors it handed to the op
    (``sca/recorded_boxes.npz``, in call order: scenes sorted, labelled frames in order).

Asserted here and again by tests/test_extract_sca_cpu.py: no point lies within 1e-4 m of the top or bottom face plane of a box
whose footprint contains it, so a single-precision ``fabsf`` in mmcv's kernel could not change a golden value.
Only data is written -- no reference source is copied.
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import json
import pickle
import shutil
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
REF = Path("/root/reference")
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import boxlabel_ref  # noqa: E402
from himo_amd import h5c  # noqa: E402
from himo_amd.eval_seg import CATEGORY_TO_INDEX  # noqa: E402

OUT = HERE / "sca"
SEED = 20240417
EXPANSION = 0.2
VEHICLE = "Testtruck"
LIDARS = ["front_left", "front_right", "rear_left", "rear_right", "roof_front", "roof_rear"]
NAME_MAPPING = {"Car": "REGULAR_VEHICLE", "Truck": "TRUCK", "Bus": "BUS", "Pedestrian": "PEDESTRIAN", "Trailer": "VEHICULAR_TRAILER",
                "none": "NONE"}
# scene -> (points per superframe, annotated frames, boxes per annotated frame)
SCENES = {"batch_11": ([2049, 1300, 1023, 1601], 4, [12, 1, 20, 8]),
          "batch_12": ([1531, 2300, 2047, 1200], 3, [9, 17, 8])}
LIMIT = 250_000


def make_boxes(rng, m: int, with_inf: bool) -> dict:
    loc = np.stack([rng.uniform(-35, 35, m), rng.uniform(-20, 20, m), rng.uniform(0.5, 1.5, m)], axis=1)
    dims = np.stack([rng.uniform(1.0, 9.0, m), rng.uniform(0.6, 2.6, m), rng.uniform(1.2, 3.5, m)], axis=1)
    heading = rng.uniform(-np.pi, np.pi, m)
    heading[::5] = 0.0                                            # some axis-aligned ones among the rotated
    for k in range(1, m, 4):                                      # overlapping pairs: box k sits on box k - 1
        loc[k] = loc[k - 1] + rng.uniform(-0.6, 0.6, 3) * [1, 1, 0.2]
        heading[k] = heading[k - 1] + rng.uniform(-0.5, 0.5)
    speed = rng.uniform(0.0, 14.0, m)
    ang = rng.uniform(-np.pi, np.pi, m)
    vel = np.stack([speed * np.cos(ang), speed * np.sin(ang)], axis=1)
    if with_inf:
        k = m // 2
        speed[k] = np.inf
        vel[k] = [np.inf, -np.inf]
    names = [str(n) for n in rng.choice([n for n in NAME_MAPPING if n != "none"], m)]
    return {"location": loc, "dimensions": dims, "heading": heading, "speed": speed, "velocity": vel, "name": names,
            "mean_delta_t": rng.uniform(0.0, 0.1, m)}


def make_points(rng, n: int, annos) -> np.ndarray:
    pts = np.stack([rng.uniform(-45, 45, n), rng.uniform(-25, 25, n), rng.uniform(-1.0, 4.0, n), rng.uniform(0, 255, n)], axis=1)
    if annos is not None and n > 1:
        m = len(annos["heading"])
        near = rng.random(n) < 0.45
        b = rng.integers(0, m, n)
        # local coordinates reach beyond the (expanded) faces, so that points fall on both sides of every face
        local = rng.uniform(-0.75, 0.75, (n, 3)) * (annos["dimensions"][b] + [2.0, 0.6, 0.4])
        c, s = np.cos(annos["heading"][b]), np.sin(annos["heading"][b])
        world = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2]], axis=1) + annos["location"][b]
        pts[near, :3] = world[near]
    return pts.astype(np.float32)


def write_raw(root: Path, rng) -> list:
    """the raw tree; returns the metadata list"""
    metadata = []
    t0 = 1_700_000_000_000_000_000
    for scene, (sizes, annotated, n_boxes) in SCENES.items():
        num = int(scene.split("_")[1])
        seq = {"vehicle": VEHICLE, "lidars": {f"lidar{k}": {"name": name} for k, name in enumerate(LIDARS)}, "superframes": []}
        for j, n in enumerate(sizes):
            annos = None
            if j < annotated:
                annos = make_boxes(rng, n_boxes[j], with_inf=j == 0)
                metadata.append({"sample_idx": scene, "frame_idx": j, "annos": annos})
            seq["superframes"].append({"timestamp_epoch_ns": str(t0 + num * 10**10 + j * 10**8),
                                       "smoothPosition": {"smothYaw_rad": float(rng.uniform(-3, 3)), "smoothX_m": float(1000 + 1.3 * j + rng.normal()),
                                                          "smoothY_m": float(-500 + 0.4 * j + rng.normal())}})
            pts = make_points(rng, n, annos)
            name = f"superframe_{j + 1:04d}"                       # 1-based folder names, 0-based JSON entries (:184)
            d = root / scene / name
            d.mkdir(parents=True)
            for col, attr in enumerate("XYZW"):
                pts[:, col].tofile(d / f"{name}_{attr}.bin")
            rng.integers(1, len(LIDARS) + 1, n).astype(np.int8).tofile(d / f"{name}_sensor.bin")
            rng.integers(0, 10**8, n).astype(np.int32).tofile(d / f"{name}_deltaT.bin")
        (root / scene / f"sequence_{num}.json").write_text(json.dumps(seq, indent=1) + "\n")
    with open(root / "metadata.pkl", "wb") as fh:
        pickle.dump(metadata, fh)
    return metadata


def write_extrinsics(path: Path, rng) -> None:
    lines = ["parameters:"]
    for k, name in enumerate(LIDARS):
        x, y, z = (round(float(v), 3) for v in rng.uniform(-3, 3, 3))
        lines += [f"  lidarArray_arrayEl{k}:", f"    humanReadableReference: {name}", "    nominalPosition:", f"      x: {x}", f"      y: {y}",
                  f"      z: {z}"]
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


def install_stubs(indexed: list):
    fire = types.ModuleType("fire")
    fire.Fire = lambda fn=None, *a, **k: None
    h5py = types.ModuleType("h5py")
    h5py.File = lambda path, mode="r": h5c.File(path, mode)
    mods = {"fire": fire, "h5py": h5py}
    for name in ("mmcv", "mmcv.ops", "dataprocess", "dataprocess.misc_data", "src", "src.utils", "src.utils.av2_eval"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
    mods["mmcv.ops"].points_in_boxes_part = boxlabel_ref.points_in_boxes_part
    mods["dataprocess.misc_data"].cal_pose0to1Numpy = lambda pose0, pose1: np.linalg.inv(pose1) @ pose0
    mods["dataprocess.misc_data"].create_reading_index = lambda d: indexed.append(Path(d))
    mods["src.utils.av2_eval"].CATEGORY_TO_INDEX = dict(CATEGORY_TO_INDEX)
    mods["src.utils.av2_eval"].NameMapping = dict(NAME_MAPPING)
    mods["src.utils.av2_eval"].BOUNDING_BOX_EXPANSION = EXPANSION
    sys.modules.update(mods)


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_extract_sca", REF / "dataprocess/extract_sca.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_extract_sca"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    rng = np.random.default_rng(SEED)
    if OUT.exists():
        shutil.rmtree(OUT)
    raw = OUT / "raw"
    write_raw(raw, rng)
    ext = OUT / "lidar_ext" / f"{VEHICLE.lower()}-generated.yml"
    write_extrinsics(ext, rng)
    (OUT / "name_mapping.json").write_text(json.dumps(NAME_MAPPING, indent=1) + "\n")

    indexed = []
    install_stubs(indexed)
    ref = load_reference()
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(tmp) / "OpenSceneFlow"
        (base / "assets/private/lidar_ext").mkdir(parents=True)
        shutil.copy(ext, base / "assets/private/lidar_ext" / ext.name)
        ref.BASE_DIR = str(base)
        h5dir = OUT / "h5"
        out, err = io.StringIO(), io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            ref.main(str(raw), str(raw / "metadata.pkl"), str(h5dir), nproc=1)
    assert indexed == [h5dir], indexed
    calls = boxlabel_ref.RECORDED
    assert len(calls) == sum(a - 1 for _, a, _ in SCENES.values()), len(calls)
    total = inside = 0
    worst = np.inf
    for pts, boxes in calls:
        worst = min(worst, boxlabel_ref.face_distance(pts, boxes))
        hit = boxlabel_ref.points_in_boxes(pts, boxes)
        total += len(hit)
        inside += int((hit >= 0).sum())
    assert worst > 1e-4, f"a golden point lies {worst:g} m from a top / bottom face: choose another SEED"
    np.savez(OUT / "recorded_boxes.npz", **{f"boxes_{k}": b for k, (_, b) in enumerate(calls)},
             **{f"n_points_{k}": np.int64(len(p)) for k, (p, _) in enumerate(calls)})
    sizes = {str(p.relative_to(OUT)): p.stat().st_size for p in sorted(OUT.rglob("*")) if p.is_file()}
    assert max(sizes.values()) < LIMIT, {k: v for k, v in sizes.items() if v >= LIMIT}
    print(f"wrote {len(sizes)} files, {sum(sizes.values())} bytes, largest {max(sizes.values())}; {len(calls)} labelled sweeps, "
          f"{inside} of {total} points in a box, nearest z face {worst:.3g} m")


if __name__ == "__main__":
    main()
