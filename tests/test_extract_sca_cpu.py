"""The Scania extractor's host half (dataprocess/extract_sca.py) against the fixtures the reference itself wrote
(tests/golden/make_extract_golden.py): the raw readers, the box tables, class bytes, the index, the command line -- and the
checker ``tests/boxlabel_ref.py`` on hand-built cases.  No GPU."""
import importlib
import pickle
import re
import warnings
from pathlib import Path

import numpy as np
import pytest

import boxlabel_ref
from conftest import GOLDEN

SCA = GOLDEN / "sca"
RAW = SCA / "raw"
REPO = Path(__file__).resolve().parents[1]


def _h5():
    from himo_amd.dataset import h5_reader
    return h5_reader()


@pytest.fixture(scope="module")
def metadata():
    with open(RAW / "metadata.pkl", "rb") as fh:
        return pickle.load(fh)


@pytest.fixture(scope="module")
def mapping():
    from himo_amd import extract_sca
    return extract_sca.load_name_mapping(SCA / "name_mapping.json")


def labelled_frames(metadata):
    """[(scene, group, annos)] in the order the reference called the op: scenes sorted, all annotated frames but the last"""
    out = []
    for scene in sorted({m["sample_idx"] for m in metadata}):
        meta = [m for m in metadata if m["sample_idx"] == scene]
        out += [(scene, f"{j + 1:04d}", m["annos"]) for j, m in enumerate(meta[:-1])]
    return out


def test_bin_reader_pose_and_timestamp_match_the_golden_h5():
    import json
    from himo_amd import extract_sca as ex
    for scene in ("batch_11", "batch_12"):
        seq = json.loads((RAW / scene / f"sequence_{scene.split('_')[1]}.json").read_text())
        ext = ex.read_extrinsics(SCA / "lidar_ext", seq["vehicle"])
        with _h5().File(SCA / "h5" / f"{scene}.h5", "r") as f:
            groups = sorted(f.keys())
            assert groups == ["0001", "0002", "0003", "0004"]
            for g in groups:
                stem = str(RAW / scene / f"superframe_{g}" / f"superframe_{g}")
                assert ex.check_data(stem) is None
                cols, lidar_id, lidar_dt = ex.get_pc(stem)
                assert lidar_dt.dtype == np.float64 and lidar_id.dtype == np.int8
                assert np.array_equal(np.array(cols).T.astype(np.float32), np.asarray(f[g]["lidar"]))
                assert np.array_equal(lidar_id.astype(np.uint8), np.asarray(f[g]["lidar_id"]))
                assert np.array_equal(lidar_dt.astype(np.float32), np.asarray(f[g]["lidar_dt"]))
                pose, ts = ex.get_pose_and_timestamp(seq, int(g) - 1)                   # folder names are 1-based
                stored = np.asarray(f[g]["pose"])
                assert stored.dtype == np.float64
                labelled = "flow" in f[g]
                want = pose.astype(np.float32).astype(np.float64) if labelled else pose
                assert np.array_equal(stored, want)
                assert int(np.asarray(f[g]["timestamp"])) == ts
                assert np.array_equal(ex.sensors_center(lidar_id, seq, ext).astype(np.float32), np.asarray(f[g]["SensorsCenter"]))
    assert ex.check_data(str(RAW / "batch_11" / "superframe_0009" / "superframe_0009")).endswith("superframe_0009_X.bin")


def test_box_tables_are_the_tensors_the_reference_handed_to_the_op(metadata, mapping):
    from himo_amd import extract_sca as ex
    rec = np.load(SCA / "recorded_boxes.npz")
    frames = labelled_frames(metadata)
    assert len(frames) == 5 and f"boxes_{len(frames)}" not in rec.files
    single = 0
    for k, (scene, group, annos) in enumerate(frames):
        mine = ex.prepared_boxes(annos, 0.2)
        want = rec[f"boxes_{k}"]
        assert mine.dtype == np.float64 and mine.tobytes() == want.tobytes(), (scene, group)
        single += len(want) == 1
        geom, obj_flow, cls, finite = ex.box_table(annos, mapping, 0.2)
        assert geom.tobytes() == boxlabel_ref.box_constants(want).tobytes()
        inf = np.isinf(np.asarray(annos["velocity"])).any(axis=1)
        assert np.array_equal(finite, (~inf).astype(np.uint8)) and obj_flow.dtype == np.float32
        assert not obj_flow[inf].any() and np.array_equal(obj_flow[~inf, :2], (np.asarray(annos["velocity"])[~inf] * 0.1).astype(np.float32))
        # an infinite speed leaves the length unexpanded (:111); width and height always grow
        raw_dims = np.asarray(annos["dimensions"])
        sp = np.asarray(annos["speed"])
        assert np.array_equal(want[~np.isfinite(sp), 3], raw_dims[~np.isfinite(sp), 0])
        assert np.array_equal(want[:, 4], raw_dims[:, 1] + 0.4)
    assert single == 1
    assert any(np.isinf(np.asarray(a["speed"])).any() for _, _, a in frames)


def test_golden_points_keep_clear_of_the_z_faces(metadata):
    """the condition under which mmcv's possible single-precision fabsf cannot change a golden value"""
    rec = np.load(SCA / "recorded_boxes.npz")
    for k, (scene, group, _) in enumerate(labelled_frames(metadata)):
        with _h5().File(SCA / "h5" / f"{scene}.h5", "r") as f:
            pts = np.asarray(f[group]["lidar"])[:, :3].astype(np.float64)
        assert len(pts) == int(rec[f"n_points_{k}"])
        assert boxlabel_ref.face_distance(pts, rec[f"boxes_{k}"]) > 1e-4


def test_name_mapping_and_class_bytes(metadata, mapping, tmp_path):
    from himo_amd import extract_sca as ex
    from himo_amd.eval_seg import CATEGORY_TO_INDEX
    assert ex.CATEGORY_TO_INDEX is CATEGORY_TO_INDEX
    assert CATEGORY_TO_INDEX[mapping["none"]] == 0
    rec = np.load(SCA / "recorded_boxes.npz")
    for k, (scene, group, annos) in enumerate(labelled_frames(metadata)):
        with _h5().File(SCA / "h5" / f"{scene}.h5", "r") as f:
            inst = np.asarray(f[group]["flow_instance_id"])
            cat = np.asarray(f[group]["flow_category_indices"])
        cls = ex.class_bytes(annos["name"][:len(rec[f"boxes_{k}"])], mapping)
        assert cls.dtype == np.uint8
        assert np.array_equal(cat, np.where(inst > 0, cls[np.maximum(inst, 1) - 1], 0))
    (tmp_path / "m.yaml").write_text("Car: REGULAR_VEHICLE\nnone: NONE\n")
    assert ex.load_name_mapping(tmp_path / "m.yaml") == {"Car": "REGULAR_VEHICLE", "none": "NONE"}
    (tmp_path / "bad.json").write_text('{"Car": "REGULAR_VEHICLE"}')
    with pytest.raises(ValueError, match="none"):
        ex.load_name_mapping(tmp_path / "bad.json")
    (tmp_path / "bad2.json").write_text('{"Car": "SPACESHIP", "none": "NONE"}')
    with pytest.raises(ValueError, match="SPACESHIP"):
        ex.load_name_mapping(tmp_path / "bad2.json")
    with pytest.raises(ValueError, match="required"):
        ex.load_name_mapping(None)


def test_index_file(tmp_path):
    import shutil
    from himo_amd import extract_sca as ex
    from himo_amd.dataset import load_index
    for p in (SCA / "h5").glob("*.h5"):
        shutil.copy(p, tmp_path / p.name)
    ex.main(output_dir=str(tmp_path), create_index_only=True)
    with open(tmp_path / "index_total.pkl", "rb") as fh:
        index = pickle.load(fh)
    assert index == [[s, g] for s in ("batch_11", "batch_12") for g in ("0001", "0002", "0003", "0004")]
    assert load_index(tmp_path) == index
    for scene_id, timestamps in index:                     # the loop of tools/pkl_extract.py:14
        assert isinstance(scene_id, str) and isinstance(timestamps, str)


def test_cli_arguments_and_expansion_override(monkeypatch):
    from himo_amd import extract_sca as ex
    a = ex._parser().parse_args(["--origin_data", "o", "--metadata_pkl", "m", "--output_dir", "d", "--nproc", "3", "--lidar_ext_dir", "e",
                                 "--name_mapping", "n.json", "--create_index_only"])
    assert (a.origin_data, a.metadata_pkl, a.output_dir, a.nproc, a.lidar_ext_dir, a.name_mapping, a.create_index_only) == \
        ("o", "m", "d", 3, "e", "n.json", True)
    d = ex._parser().parse_args([])
    assert d.create_index_only is False and d.name_mapping is None and d.batch_sweeps == 32
    import inspect
    assert list(inspect.signature(ex.main).parameters)[:5] == ["origin_data", "metadata_pkl", "output_dir", "nproc", "create_index_only"]
    assert ex.BOUNDING_BOX_EXPANSION == ex.BOUNDING_BOX_EXPANSION_DEFAULT == 0.2
    monkeypatch.setenv("HIMO_BOUNDING_BOX_EXPANSION", "0.35")
    try:
        with pytest.warns(UserWarning, match="HIMO_BOUNDING_BOX_EXPANSION=0.35"):
            importlib.reload(ex)
        assert ex.BOUNDING_BOX_EXPANSION == 0.35
    finally:
        monkeypatch.delenv("HIMO_BOUNDING_BOX_EXPANSION")
        with warnings.catch_warnings():
            warnings.simplefilter("error")                 # the default warns about nothing
            importlib.reload(ex)
    assert ex.BOUNDING_BOX_EXPANSION == 0.2


def test_export_is_declared_in_the_header_and_bound():
    from himo_amd import _lib
    header = (REPO / "include" / "himo_amd.h").read_text()
    m = re.search(r"int himo_box_label_batch\(([^;]*)\);", header)
    assert m, "include/himo_amd.h does not declare himo_box_label_batch"
    assert "extract_sca.py:117" in header
    restype, argtypes = _lib.SIGNATURES["himo_box_label_batch"]
    assert len(argtypes) == len(m.group(1).split(","))
    assert "FLAGS_boxlabel := -ffp-contract=off" in (REPO / "himo_amd" / "csrc" / "Makefile").read_text()


# ---- the checker itself -----------------------------------------------------------------------------------------------------
# an axis-aligned box with exactly representable coordinates: centre (2, -1), bottom 0.5, size 4 x 2 x 1
BOX = np.array([[2.0, -1.0, 0.5, 4.0, 2.0, 1.0, 0.0]])
FACE_POINTS = np.array([
    [2.0, -1.0, 1.0],      # the centre: inside
    [4.0, -1.0, 1.0],      # +x face: outside (strict)
    [0.0, -1.0, 1.0],      # -x face: outside
    [2.0, 0.0, 1.0],       # +y face: outside
    [2.0, -2.0, 1.0],      # -y face: outside
    [2.0, -1.0, 1.5],      # top face: inside (`>` rejects)
    [2.0, -1.0, 0.5],      # bottom face: inside
    [3.9999999, -1.0, 1.0],
    [2.0, -1.0, 1.5000001],
])
FACE_WANT = np.array([0, -1, -1, -1, -1, 0, 0, 0, -1], dtype=np.int32)


def test_checker_faces_are_strict_in_xy_and_closed_in_z():
    assert np.array_equal(boxlabel_ref.points_in_boxes(FACE_POINTS, BOX), FACE_WANT)
    assert np.array_equal(boxlabel_ref.box_constants(BOX)[0], [2.0, -1.0, 1.0, 2.0, 1.0, 0.5, 1.0, 0.0])


def test_checker_first_box_wins_and_none_is_minus_one():
    boxes = np.array([[10.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0],
                      [2.0, -1.0, 0.5, 1.0, 1.0, 1.0, 0.0],          # inside BOX's copy below, listed first
                      [2.0, -1.0, 0.5, 4.0, 2.0, 1.0, 0.0],
                      [2.0, -1.0, 0.5, 4.0, 2.0, 1.0, 0.5]])
    pts = np.array([[2.0, -1.0, 1.0], [3.5, -1.0, 1.0], [10.5, 0.5, 1.0], [50.0, 0.0, 1.0], [2.0, -1.0, 3.0]])
    assert boxlabel_ref.points_in_boxes(pts, boxes).tolist() == [1, 2, 0, -1, -1]
    assert boxlabel_ref.points_in_boxes(pts, boxes[::-1]).tolist() == [0, 0, 3, -1, -1]
    assert boxlabel_ref.points_in_boxes(pts, np.zeros((0, 7))).tolist() == [-1] * 5
    assert boxlabel_ref.points_in_boxes(np.zeros((0, 3)), boxes).shape == (0,)


def test_checker_rotation_sign():
    """a box turned by +90 degrees: its LENGTH lies along y"""
    box = np.array([[0.0, 0.0, 0.0, 6.0, 2.0, 2.0, np.pi / 2]])
    assert boxlabel_ref.points_in_boxes(np.array([[0.0, 2.5, 1.0], [2.5, 0.0, 1.0]]), box).tolist() == [0, -1]
