"""The segmentation evaluator's host side (himo_amd/eval_seg.py) against the reference's own recorded results
(tests/golden/seg_golden.json, written by tests/golden/make_seg_golden.py from downstream/eval_seg.py).  No GPU."""
import json
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
SEG = GOLDEN / "seg"


@pytest.fixture(scope="module")
def seg_gold():
    return json.loads((GOLDEN / "seg_golden.json").read_text())


def test_public_names_match_the_reference_tables(seg_gold):
    from himo_amd import eval_seg
    assert eval_seg.CATEGORY_TO_INDEX == seg_gold["category_to_index"]
    assert eval_seg.INDEX_TO_CATEGORY == {v: k for k, v in seg_gold["category_to_index"].items()}
    assert eval_seg.CAR == ["REGULAR_VEHICLE"] and len(eval_seg.OTHER_VEHICLES) == 9
    for name in ("iouEval", "SegMetrics", "main"):
        assert hasattr(eval_seg, name)


def test_class_lut_is_the_reference_three_step_remap_for_every_byte(seg_gold):
    from himo_amd import eval_seg
    lut = eval_seg.class_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    assert lut.tolist() == seg_gold["remap_gt"]           # eval_seg.py:255-257 applied to 0..255 by the reference itself
    assert lut.tolist() == seg_gold["remap_pred"]         # eval_seg.py:261-263
    assert lut[eval_seg.CATEGORY_TO_INDEX["REGULAR_VEHICLE"]] == 1 and lut[1] == 0 and lut[2] == 2


def test_class_lut_refuses_a_table_the_three_steps_do_not_collapse_for(monkeypatch):
    from himo_amd import eval_seg
    shifted = dict(eval_seg.CATEGORY_TO_INDEX)
    shifted["BUS"], shifted["ANIMAL"] = 1, shifted["BUS"]       # index 1 in OTHER_VEHICLES: step 3 would catch the cars
    monkeypatch.setattr(eval_seg, "CATEGORY_TO_INDEX", shifted)
    with pytest.raises(ValueError, match="collapse"):
        eval_seg.class_lut()


@pytest.mark.parametrize("text", ["seg_raw,seg_flow", "['seg_raw','seg_flow']", '["seg_raw", "seg_flow"]', " seg_raw , seg_flow ",
                                  "(seg_raw,seg_flow)"])
def test_res_names_parser_accepts_both_spellings(text):
    from himo_amd.eval_seg import parse_res_names
    assert parse_res_names(text) == ["seg_raw", "seg_flow"]


def test_res_names_parser_lists_and_errors():
    from himo_amd.eval_seg import parse_res_names
    assert parse_res_names(["a", "b"]) == ["a", "b"] and parse_res_names("seg_raw") == ["seg_raw"]
    with pytest.raises(ValueError):
        parse_res_names("[]")


def test_labels_outside_a_byte_count_as_class_zero():
    from himo_amd.eval_seg import as_labels_u8
    got = as_labels_u8(np.array([[0, 1, 2, 255], [256, -1, 1000, 19]], dtype=np.int64))
    assert got.dtype == np.uint8 and got.tolist() == [0, 1, 2, 255, 0, 0, 0, 19]
    assert as_labels_u8(np.array([True, False])).tolist() == [1, 0]
    u8 = np.arange(5, dtype=np.uint8)
    assert np.shares_memory(as_labels_u8(u8), u8)                 # uint8 goes through without a copy


def test_hdf5_dataset_serves_requested_datasets_with_their_disk_dtypes():
    from himo_amd.dataset import SEG_FIELDS, HDF5Dataset
    names = ["seg_raw", "seg_flow"]
    ds = HDF5Dataset(SEG, vis_name=names, eval=True, fields=SEG_FIELDS + tuple(names), need_next=False)
    assert len(ds) == 5                                   # the last sweeps of both scenes stay: nothing here needs a successor
    seen_unlabelled = 0
    for i in range(len(ds)):
        f = ds[i]
        n = len(f["seg_valid"])
        assert f["seg_valid"].dtype == np.bool_ and f["seg_raw"].dtype == np.uint8 and f["seg_flow"].dtype == np.uint8
        assert f["seg_raw"].shape == f["seg_flow"].shape == (n,) and n > 2000
        assert "pc0" not in f and "pose0" not in f and "gm0" not in f
        if "flow_category_indices" in f:
            assert f["flow_category_indices"].dtype == np.uint8 and set(f["flow_category_indices"].tolist()) == set(range(31))
        else:
            seen_unlabelled += 1
    assert seen_unlabelled == 1
    f = ds.read(0, fields=("seg_valid",))
    assert set(f) == {"scene_id", "timestamp", "seg_valid"}
    ds.close()


def test_hdf5_dataset_existing_callers_get_what_they_got():
    """the default index still drops sweeps without a successor, and a read without the new names holds none of them"""
    from himo_amd.dataset import EVAL_FIELDS, HDF5Dataset
    ds = HDF5Dataset(GOLDEN / "h5", eval=False, fields=EVAL_FIELDS)
    assert len(ds) == 6
    f = ds[0]
    assert "seg_valid" not in f and "SensorsCenter" not in f and "ego_motion" not in f
    assert set(f) == {"scene_id", "timestamp"} | set(EVAL_FIELDS)
    ds.close()
    with pytest.raises(KeyError):
        HDF5Dataset(SEG, eval=True)                           # the evaluation list names last sweeps: refused unless need_next=False


def test_npz_dataset_carries_the_same_keys(tmp_path):
    from himo_amd.dataset import SEG_FIELDS, HDF5Dataset, NpzDataset, open_dataset
    names = ["seg_raw", "seg_flow"]
    src = HDF5Dataset(SEG, vis_name=names, eval=False, fields=SEG_FIELDS + tuple(names), need_next=False)
    frames = [src[i] for i in range(len(src))]
    NpzDataset.write(tmp_path, frames, eval_subset=[0, 4])
    ds = open_dataset(tmp_path, vis_name=names, eval=True, fields=SEG_FIELDS + tuple(names), need_next=False)
    assert isinstance(ds, NpzDataset) and len(ds) == 2
    for got, want in zip((ds[0], ds[1]), (frames[0], frames[4])):
        assert set(got) == set(want)
        for k in ("seg_valid", "seg_raw", "seg_flow"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k])


@pytest.mark.parametrize("mode", ["All", "Mask only"])
def test_get_iou_on_the_golden_matrices_is_bit_equal(seg_gold, mode):
    from himo_amd.eval_seg import iouEval
    for name in seg_gold["res_names"]:
        ev = iouEval(n_classes=3, ignore=[])
        assert ev.num_classes() == 3 and ev.conf_matrix.sum() == 0
        ev.conf_matrix = np.array(seg_gold[mode]["conf"][name], dtype=np.int64)
        mean, per_class = ev.getIoU()
        assert float(mean).hex() == seg_gold[mode]["iou_mean"][name]
        assert [float(v).hex() for v in per_class] == seg_gold[mode]["iou"][name]
        tp, fp, fn = ev.getStats()
        conf = np.array(seg_gold[mode]["conf"][name], dtype=np.float64)
        assert np.array_equal(tp, np.diag(conf)) and np.array_equal(fp, conf.sum(1) - tp) and np.array_equal(fn, conf.sum(0) - tp)
        ev.reset()
        assert ev.conf_matrix.sum() == 0


def test_ignore_list_enters_stats_and_mean_as_in_the_reference(seg_gold):
    from himo_amd.eval_seg import iouEval
    conf = np.array(seg_gold["All"]["conf"]["seg_raw"], dtype=np.int64)
    ev = iouEval(n_classes=3, ignore=[0])
    ev.conf_matrix = conf
    c = conf.astype(np.float64)
    c[:, [0]] = 0
    tp = np.diag(c)
    union = tp + (c.sum(1) - tp) + (c.sum(0) - tp) + 1e-15
    mean, per_class = ev.getIoU()
    assert np.array_equal(per_class, tp / union) and mean == (tp[1:] / union[1:]).mean()
    with pytest.raises(ValueError):
        iouEval(n_classes=2)


@pytest.mark.parametrize("mode", ["All", "Mask only"])
def test_table_text_on_the_golden_matrices_is_the_reference_block(seg_gold, mode):
    from himo_amd.eval_seg import SegMetrics
    m = SegMetrics(seg_gold["res_names"])
    for r, name in enumerate(seg_gold["res_names"]):
        m.host[r, 0 if mode == "All" else 1] = np.array(seg_gold[mode]["conf"][name])
    text = seg_gold[mode]["stdout"]
    assert m.table(mode) == text[text.index("\n  ====="):]
    assert m.table(0 if mode == "All" else 1) == m.table(mode)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_matrix(rank):
    rng = np.random.default_rng(40 + rank)
    return rng.integers(0, 2 ** 40, (2, 2, 3, 3)).astype(np.int64)


def _worker_gather(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, str(REPO))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from himo_amd.eval_seg import SegMetrics
    m = SegMetrics(["seg_raw", "seg_flow"])
    m.host = _rank_matrix(rank)
    m.frame_cnt, m.points = 3 + rank, 1000 * (rank + 1)
    m.gather()
    np.save(Path(out_dir, f"conf{rank}.npy"), m.conf)
    Path(out_dir, f"cnt{rank}").write_text(f"{m.frame_cnt} {m.points}")
    dist.destroy_process_group()


def test_gather_sums_host_matrices_over_two_gloo_ranks_exactly(tmp_path):
    mp.spawn(_worker_gather, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    want = _rank_matrix(0) + _rank_matrix(1)
    for rank in range(2):
        got = np.load(tmp_path / f"conf{rank}.npy")
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert (tmp_path / f"cnt{rank}").read_text() == "7 3000"


def test_gather_without_a_process_group_leaves_the_matrices():
    from himo_amd.eval_seg import SegMetrics
    m = SegMetrics("seg_raw")
    m.host[0, 0] = np.arange(9).reshape(3, 3)
    m.gather()
    assert m.conf[0, 0].tolist() == np.arange(9).reshape(3, 3).tolist()


def test_sweep_warnings_are_the_reference_lines(seg_gold):
    from himo_amd.eval_seg import sweep_warnings
    f = {"scene_id": "seg-scene-01", "timestamp": 315970000400000000, "seg_valid": 0, "seg_raw": 0, "seg_flow": 0}
    lines = sweep_warnings(f, ["seg_raw", "seg_flow"])
    assert lines == ["[Warning]: No flow_category_indices in seg-scene-01 at 315970000400000000, check the data."]
    assert seg_gold["All"]["stdout"].startswith(lines[0] + "\n" + lines[0] + "\n")
    assert sweep_warnings({"scene_id": "s", "timestamp": 1}, ["a"]) == [
        "[Warning]: No seg_valid in s at 1, check the data.", "[Warning]: No flow_category_indices in s at 1, check the data.",
        "[Warning]: No a in s at 1, check the data."]


def test_fixture_files_are_small():
    for p in list(SEG.iterdir()) + [GOLDEN / "seg_golden.json"]:
        assert p.stat().st_size < 512 << 10, p
