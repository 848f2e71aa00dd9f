"""The segmentation evaluator on the device (csrc/segiou.hip, himo_amd/eval_seg.py): integer results, so every comparison is
exact -- against the reference's own recorded matrices and text (tests/golden/seg_golden.json) and against ``np.bincount``."""
import json
import pickle
import shutil
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
SEG = GOLDEN / "seg"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg_gold():
    return json.loads((GOLDEN / "seg_golden.json").read_text())


def _bincount_conf(pred_cls, gt_cls):
    """rows = prediction, columns = ground truth"""
    return np.bincount(3 * pred_cls.astype(np.int64) + gt_cls.astype(np.int64), minlength=9).reshape(3, 3)


@pytest.mark.parametrize("overlap_both", [(False, False), (False, True), (True, False)])
def test_main_over_the_golden_scenes_matches_the_reference(gpu, seg_gold, capsys, overlap_both):
    from himo_amd import eval_seg
    mask_only, both = overlap_both
    m = eval_seg.main(str(SEG), res_names=list(seg_gold["res_names"]), mask_only=mask_only, both=both)
    out = capsys.readouterr().out
    for k, mode in enumerate(("All", "Mask only")):
        for r, name in enumerate(seg_gold["res_names"]):
            assert m.conf[r, k].tolist() == seg_gold[mode]["conf"][name], (mode, name)
    assert m.frame_cnt == seg_gold["sweeps_counted"] and m.points == seg_gold["points"]
    assert int(m.conf[:, 0].sum()) == len(seg_gold["res_names"]) * seg_gold["points"]
    assert int(m.conf[:, 1].sum()) == len(seg_gold["res_names"]) * seg_gold["valid_points"]
    if both:
        text = seg_gold["Mask only"]["stdout"]
        assert out == seg_gold["All"]["stdout"] + text[text.index("\n  ====="):]
    else:
        assert out == seg_gold["Mask only" if mask_only else "All"]["stdout"]        # character for character


def test_serial_loop_and_small_batches_give_the_same_matrices(gpu, seg_gold):
    from himo_amd import eval_seg
    from himo_amd.dataset import SEG_FIELDS, open_dataset
    names = seg_gold["res_names"]
    for overlap, batch_frames in ((False, 32), (True, 1), (False, 2)):
        ds = open_dataset(SEG, vis_name=names, eval=True, fields=SEG_FIELDS + tuple(names), need_next=False)
        m = eval_seg.SegMetrics(names)
        assert eval_seg.run_dataset(ds, m, batch_frames=batch_frames, overlap=overlap) == seg_gold["sweeps_counted"]
        for r, name in enumerate(names):
            assert m.conf[r, 0].tolist() == seg_gold["All"]["conf"][name]
            assert m.conf[r, 1].tolist() == seg_gold["Mask only"]["conf"][name]


def test_cli_accepts_the_reference_list_spelling(gpu, seg_gold, capsys):
    from himo_amd import eval_seg
    eval_seg._cli(["--data_dir", str(SEG), "--res_names", "['seg_raw','seg_flow']"])
    assert capsys.readouterr().out == seg_gold["All"]["stdout"]
    eval_seg._cli(["--data_dir", str(SEG), "--res_names", "seg_flow", "--mask_only"])
    text = capsys.readouterr().out
    want = seg_gold["Mask only"]["stdout"]
    assert "seg_raw" not in text and text.endswith(want[want.index("seg_flow 100 frames"):])


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
def test_add_batch_against_bincount(gpu, n):
    from himo_amd.eval_seg import iouEval
    rng = np.random.default_rng(n)
    pred, gt = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 3, n).astype(np.uint8)
    ev = iouEval(n_classes=3, ignore=[])
    ev.addBatch(pred, gt)
    want = _bincount_conf(pred, gt)
    assert ev.conf_matrix.dtype == np.int64 and np.array_equal(ev.conf_matrix, want) and ev.conf_matrix.sum() == n
    ev.addBatch(pred.astype(np.int64), gt.astype(np.int32))                       # a second call accumulates; other dtypes are cast
    assert np.array_equal(ev.conf_matrix, 2 * want)
    ev.reset()
    assert ev.conf_matrix.sum() == 0
    ev.addBatch(pred, gt)
    assert np.array_equal(ev.conf_matrix, want)


def test_add_batch_casts_and_sends_stray_values_to_class_zero(gpu):
    import torch
    from himo_amd.eval_seg import iouEval
    pred = np.array([0, 1, 2, 3, 255, 256, -1, 2, 1], dtype=np.int64)
    gt = np.array([1, 1, 2, 2, 0, 1, 2, 1000, 1], dtype=np.int64)
    clean = lambda a: np.where((a >= 0) & (a <= 2), a, 0)                          # noqa: E731
    ev = iouEval()
    ev.addBatch(pred, gt)
    assert np.array_equal(ev.conf_matrix, _bincount_conf(clean(pred), clean(gt)))
    dev = iouEval()
    dev.addBatch(torch.from_numpy(clean(pred).astype(np.uint8)).to(gpu)[1:], torch.from_numpy(clean(gt).astype(np.uint8)).to(gpu)[1:])
    assert np.array_equal(dev.conf_matrix, _bincount_conf(clean(pred)[1:], clean(gt)[1:]))      # (an unaligned device view)
    mean, per_class = ev.getIoU()
    c = ev.conf_matrix.astype(np.float64)
    tp = np.diag(c)
    assert np.array_equal(per_class, tp / (tp + (c.sum(1) - tp) + (c.sum(0) - tp) + 1e-15)) and mean == per_class.mean()


def _sweeps(rng, sizes, names):
    frames = []
    for k, n in enumerate(sizes):
        f = {"scene_id": "s", "timestamp": k, "flow_category_indices": rng.integers(0, 31, n).astype(np.uint8),
             "seg_valid": rng.random(n) < 0.6}
        for name in names:
            f[name] = rng.integers(0, 31, n).astype(np.uint8)
        frames.append(f)
    return frames


def _expected(frames, names, lut):
    want = np.zeros((len(names), 2, 3, 3), dtype=np.int64)
    gt = lut[np.concatenate([f["flow_category_indices"] for f in frames])] if frames else np.zeros(0, np.uint8)
    valid = np.concatenate([f["seg_valid"] for f in frames]) if frames else np.zeros(0, bool)
    for r, name in enumerate(names):
        pred = lut[np.concatenate([f[name] for f in frames])] if frames else np.zeros(0, np.uint8)
        want[r, 0] = _bincount_conf(pred, gt)
        want[r, 1] = _bincount_conf(pred[valid], gt[valid])
    return want, int(gt.size), int(valid.sum())


@pytest.mark.parametrize("n_results", [1, 2, 8])
@pytest.mark.parametrize("sizes", [[0], [1], [15], [16], [17], [4097], [5, 0, 16, 33, 1, 4097, 250], [120_000] * 32],
                         ids=["0", "1", "15", "16", "17", "4097", "ragged", "120000x32"])
def test_packed_sweeps_against_bincount(gpu, n_results, sizes):
    """sweeps of odd sizes packed back to back (their starts are not 16-byte aligned), R result names, a random seg_valid"""
    from himo_amd.eval_seg import SegMetrics, class_lut
    names = [f"seg_{k}" for k in range(n_results)]
    rng = np.random.default_rng(1000 * n_results + len(sizes) + sum(sizes) % 977)
    if len(sizes) == 32:
        sizes = [n - 7 * k for k, n in enumerate(sizes)]      # 120 000 points, less a few: every later sweep starts unaligned
    frames = _sweeps(rng, sizes, names)
    want, points, valid_points = _expected(frames, names, class_lut())
    m = SegMetrics(names)
    m.add(frames)
    got = m.conf
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert all(int(got[r, 0].sum()) == points and int(got[r, 1].sum()) == valid_points for r in range(n_results))
    assert m.points == points and m.frame_cnt == len(frames)
    m.add(frames)                                              # two calls accumulate
    assert np.array_equal(m.conf, 2 * want)
    m.reset()                                                  # reset() zeroes
    assert m.conf.sum() == 0 and m.points == 0
    m.add(frames[:1])
    assert np.array_equal(m.conf, _expected(frames[:1], names, class_lut())[0])


def test_unaligned_base_pointers_take_the_point_by_point_path(gpu):
    import torch
    from himo_amd.eval_seg import class_lut, seg_confusion
    rng = np.random.default_rng(5)
    n = 10_001
    lut = class_lut()
    gt, pred, valid = (rng.integers(0, 31, n + 3).astype(np.uint8), rng.integers(0, 31, n + 3).astype(np.uint8),
                       (rng.random(n + 3) < 0.5).astype(np.uint8))
    d = lambda a, off: torch.from_numpy(a).to(gpu)[off:off + n]                    # noqa: E731
    conf = torch.zeros((1, 2, 3, 3), dtype=torch.int64, device=gpu)
    seg_confusion(conf, d(gt, 1), [d(pred, 3)], d(valid, 2), lut)
    g, p, v = lut[gt[1:1 + n]], lut[pred[3:3 + n]], valid[2:2 + n].astype(bool)
    assert np.array_equal(conf[0, 0].cpu().numpy(), _bincount_conf(p, g))
    assert np.array_equal(conf[0, 1].cpu().numpy(), _bincount_conf(p[v], g[v]))
    none = torch.zeros((1, 2, 3, 3), dtype=torch.int64, device=gpu)
    seg_confusion(none, d(gt, 0), [d(pred, 0)], None, lut)                         # no seg_valid: the masked matrix stays empty
    assert int(none[0, 0].sum()) == n and int(none[0, 1].sum()) == 0
    with pytest.raises(ValueError):
        seg_confusion(none, d(gt, 0), [d(pred, 0)] * 9, None, lut)
    with pytest.raises(ValueError):
        seg_confusion(none, d(gt, 0), [d(pred, 0)[:-1]], None, lut)


def _copy_fixture(tmp_path, index_eval):
    root = tmp_path / "seg"
    shutil.copytree(SEG, root)
    with open(root / "index_eval.pkl", "wb") as fh:
        pickle.dump(index_eval, fh)
    return root


def test_sweep_without_labels_is_skipped_with_the_reference_warning(gpu, tmp_path, capsys):
    from himo_amd import eval_seg
    with open(SEG / "index_total.pkl", "rb") as fh:
        total = pickle.load(fh)
    root = _copy_fixture(tmp_path, [total[4]])                                    # only the sweep that has no flow_category_indices
    m = eval_seg.main(str(root), res_names=["seg_raw"])
    out = capsys.readouterr().out
    line = f"[Warning]: No flow_category_indices in {total[4][0]} at {total[4][1]}, check the data.\n"
    assert out.startswith(line + line + "\n  ====") and m.frame_cnt == 0 and m.conf.sum() == 0
    assert "IoU avg 0.000" in out


@pytest.mark.parametrize("overlap", [True, False])
def test_missing_result_name_is_a_key_error(gpu, capsys, overlap):
    from himo_amd import eval_seg
    from himo_amd.dataset import SEG_FIELDS, open_dataset
    names = ["seg_raw", "seg_nowhere"]
    with pytest.raises(KeyError, match="seg_nowhere"):
        if overlap:
            eval_seg.main(str(SEG), res_names=names)
        else:
            ds = open_dataset(SEG, vis_name=names, eval=True, fields=SEG_FIELDS + tuple(names), need_next=False)
            eval_seg.run_dataset(ds, eval_seg.SegMetrics(names), overlap=False)
    out = capsys.readouterr().out
    assert out.startswith("[Warning]: No seg_nowhere in seg-scene-00 at ") and "RESULTS" not in out
