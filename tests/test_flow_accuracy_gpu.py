"""Rules 3b (residual estimates) and 9 (accuracy table) of "flow metrics, v1" on the device (``himo_flow_metrics_batch_ex``,
csrc/flowmetrics.hip) against the numpy restatement (tests/flowaccuracy_ref.py) and against the v1 entry point.

What is compared, and how tightly.  The v1 tables of the new entry must be BIT-EQUAL to ``himo_flow_metrics_batch``'s on the same
inputs: it is the same arithmetic.  The accuracy table must EQUAL the restatement's: a stored result's error involves no
transform (identical inputs, correctly rounded operations in the same order), group membership rests on the 1e-4 m margin of
every speed from the dynamic threshold, and where an error does involve the transform (``raw``, residual mode) its distance from
the four thresholds is asserted first -- the kernel's chain is within a few ulp (1e-15 m) of numpy's."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))

import flowaccuracy_ref as acc  # noqa: E402
import flowmetrics_ref as ref  # noqa: E402
from test_flow_metrics_gpu import H5, SIZES, assert_clear_of_edges, make_frames  # noqa: E402

pytestmark = pytest.mark.gpu


def _tables(gpu, n_frames, n_results):
    import torch
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=gpu)      # noqa: E731
    return z(n_results, 5, 51, 3), z(n_frames, n_results, 3, 2), z(n_results), z(n_results, 4, 3)


def _launch(gpu, b, ests=None, accuracy=True, residual=False):
    """one thin launch on fresh tables -> (buckets, threeway, rejected, accuracy or None) on the device"""
    from himo_amd.eval_flow import flow_metrics
    ests = b.ests if ests is None else ests
    bk, tw, rj, ac = _tables(gpu, b.sweeps, len(ests))
    flow_metrics(bk, tw, rj, b.offsets, b.pose0, b.pose1, b.pc0, b.gt, ests, b.category, b.ground,
                 accuracy=ac if accuracy else None, residual=residual)
    return bk, tw, rj, (ac if accuracy else None)


def _full_mode(gpu, frames, names):
    """the new entry with a table beside the v1 entry on the same packed batch; the accuracy table against the restatement"""
    import torch
    from himo_amd.eval_flow import FlowBatch
    assert_clear_of_edges(frames, 1e-4)
    for name in names:
        margin = acc.threshold_margin(frames, name)
        print(f"{name}: epe stays {margin:.3g} m from the accuracy thresholds")
        assert margin >= 1e-9
    b = FlowBatch.from_frames(frames, names, device=gpu)
    old = _launch(gpu, b, accuracy=False)                          # himo_flow_metrics_batch
    new = _launch(gpu, b)                                          # himo_flow_metrics_batch_ex, d_accuracy != NULL
    for x, y in zip(old[:3], new[:3]):
        assert torch.equal(x, y)
    wb, wt, wr, wa = acc.flow_accuracy_ref(frames, names, "av2")
    got = new[3].cpu().numpy()
    assert np.array_equal(got, wa), (got.tolist(), wa.tolist())
    assert np.array_equal(new[2].cpu().numpy(), wr) and np.array_equal(new[0].cpu().numpy()[..., 0], wb[..., 0])
    return wa, wr


@pytest.mark.parametrize("case", list(SIZES))
def test_full_mode_keeps_the_v1_bits_and_counts_the_restatements_table(gpu, case):
    names = ["flow_a", "raw"]
    frames = make_frames(211 + sum(SIZES[case]), SIZES[case], names, bad="flow_a")
    wa, wr = _full_mode(gpu, frames, names)
    if sum(SIZES[case]) >= 1023:
        assert (wa[..., 0] > 0).all() and wr[0] > 0 and (wa[0, :, 1] < wa[0, :, 2]).all()       # every group, strict < relaxed
        assert wa[0, 0, 0] + wr[0] == wa[1, 0, 0]                   # rejected points are in no group


@pytest.mark.parametrize("n_results", [1, 2, 8])
def test_result_counts_with_raw_and_a_result_of_bad_rows(gpu, n_results):
    names = (["flow_0", "raw"] + [f"flow_{k}" for k in range(2, 8)])[:n_results]
    frames = make_frames(270 + n_results, [700, 0, 300], names, bad="flow_0")
    wa, wr = _full_mode(gpu, frames, names)
    assert wr[0] > 0 and not wr[1:].any() and (wa[1:, 0, 0] == wa[0, 0, 0] + wr[0]).all()


def test_two_large_sweeps_take_the_capped_grid(gpu):
    """more than 1024 x 256 points: every block walks several steps and the sweep boundary falls inside a block's run"""
    names = ["flow_a", "raw"]
    frames = make_frames(6, [140_000, 139_993], names, bad="flow_a")
    assert sum(f["pc0"].shape[0] for f in frames) > 1024 * 256
    wa, wr = _full_mode(gpu, frames, names)
    assert wr[0] > 1000 and (wa[..., 0] > 1000).all()


@pytest.fixture(scope="module")
def fixture_frames():
    return acc.fixture()


def _pitch4(gpu, rows):
    """[T][3] float32 -> an [T][3] view of rows four floats apart on the device (column 3 holds a value that must not be read)"""
    import torch
    wide = torch.full((rows.shape[0], 4), float("nan"), dtype=torch.float32, device=gpu)
    wide[:, :3] = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(gpu)
    view = wide[:, :3]
    assert view.stride(0) == 4 and not view.is_contiguous()
    return view


def test_residual_rows_of_pitch_four_against_the_restatement(gpu, fixture_frames):
    import torch
    from himo_amd.eval_flow import FlowBatch, FlowMetrics
    frames, names = fixture_frames, ["res", "raw"]
    margin = acc.threshold_margin(frames, "res", residual=True)
    print(f"residual fixture: epe stays {margin:.3g} m from the accuracy thresholds")
    assert margin >= 1e-6
    assert min(np.abs(ref.speeds(f) - 0.05).min() for f in frames) >= 1e-4         # group membership: the dynamic threshold
    assert_clear_of_edges(frames, 1e-5)                                           # (the fixture's speeds stay 3.7e-5 m from the bucket edges)
    wb, wt, wr, wa = acc.flow_accuracy_ref(frames, names, "av2", residual=True)
    assert wa[0].tolist() == acc.FIXTURE_TABLE
    b = FlowBatch.from_frames(frames, names, device=gpu)
    b.ests = [_pitch4(gpu, np.concatenate([f["res"] for f in frames])), None]
    m = FlowMetrics(names, "av2", accuracy=True, residual=True)
    m.add_batch(b)

    def check(times):
        bk, rj, ac = m.buckets, m.rejected, m.accuracy
        tw = np.stack(list(m.threeway.values()))
        assert np.array_equal(ac, times * wa), ac.tolist()
        assert np.array_equal(bk[..., 0], times * wb[..., 0]) and np.array_equal(tw[..., 0], times * wt[..., 0]) and np.array_equal(rj, times * wr)
        for got, want, count in ((bk[..., 1], wb[..., 1], wb[..., 0]), (bk[..., 2], wb[..., 2], wb[..., 0]), (tw[..., 1], wt[..., 1], wt[..., 0])):
            assert np.all(np.abs(got - times * want) <= times * count)             # one unit per counted point
    check(1)
    res = m.results()["res"]
    strict, relaxed = acc.accuracy_means(wa[0])
    assert res["acc_strict"] == strict and res["acc_relaxed"] == relaxed
    m.add_batch(b)                                                  # a second call accumulates
    check(2)
    m.reset()
    assert m.accuracy.sum() == 0 and m.buckets.sum() == 0 and m.threeway == {}
    m.add_batch(b)
    check(1)
    # an all-zero residual is the raw result, bit for bit, through the same entry
    zero = _pitch4(gpu, np.zeros((b.total_points, 3), np.float32))
    bk, tw, rj, ac = _launch(gpu, b, ests=[zero, None], residual=True)
    assert torch.equal(bk[0], bk[1]) and torch.equal(tw[:, 0], tw[:, 1]) and torch.equal(ac[0], ac[1]) and int(rj.sum()) == 0
    assert np.array_equal(ac[1].cpu().numpy(), wa[1])
    # ... and a residual with NaN / inf / 2000 m rows is rejected there, for that result only
    bad = np.concatenate([f["res"] for f in frames]).copy()
    bad[0::9, 0], bad[1::9, 1], bad[2::9, 2] = np.nan, np.inf, 2000.0
    bad_frames = [dict(f, res=bad[lo:hi]) for f, lo, hi in zip(frames, b.offsets_host[:-1], b.offsets_host[1:])]
    _, _, wr2, wa2 = acc.flow_accuracy_ref(bad_frames, names, "av2", residual=True)
    _, _, rj, ac = _launch(gpu, b, ests=[_pitch4(gpu, bad), None], residual=True)
    assert wr2[0] > 0 and np.array_equal(rj.cpu().numpy(), wr2) and np.array_equal(ac.cpu().numpy(), wa2)


def test_refusals_and_the_call_without_a_table(gpu, fixture_frames):
    import torch
    from himo_amd import _lib
    from himo_amd.eval_flow import FlowBatch, class_lut, flow_metrics
    frames, names = fixture_frames, ["a", "raw"]
    b = FlowBatch.from_frames(frames, names, device=gpu)
    lib = _lib.load()
    ws = torch.empty(int(lib.himo_flow_metrics_workspace_bytes(b.sweeps)) + 16, dtype=torch.uint8, device=gpu)
    lut = class_lut()

    def raw_call(est_stride, tables):
        bk, tw, rj, ac = tables
        ptrs = (ctypes.c_void_p * 2)(_lib.ptr(b.ests[0]), None)
        return lib.himo_flow_metrics_batch_ex(b.sweeps, b.total_points, _lib.ptr(b.offsets), _lib.ptr(b.pose0), _lib.ptr(b.pose1), _lib.ptr(b.pc0),
                                              int(b.pc0.stride(0)), _lib.ptr(b.gt), ptrs, 2, est_stride, _lib.ptr(b.category), _lib.ptr(b.ground),
                                              None, lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 0.1, 0, _lib.ptr(bk), _lib.ptr(tw),
                                              _lib.ptr(rj), _lib.ptr(ac), _lib.ptr(ws), _lib.stream_handle())
    for stride in (2, 0, -4):
        tables = _tables(gpu, b.sweeps, 2)
        assert raw_call(stride, tables) == _lib.ERR_INVALID_ARGUMENT                # a status ...
        assert all(int(t.abs().sum()) == 0 for t in tables)                        # ... and no write
    tables = _tables(gpu, b.sweeps, 2)
    assert raw_call(3, tables) == _lib.OK and int(tables[3].sum()) > 0
    with pytest.raises(ValueError):                                               # the evaluator refuses such rows itself
        wide = torch.zeros((b.total_points, 4), dtype=torch.float32, device=gpu)
        _launch(gpu, b, ests=[wide[:, :2], None])
    with pytest.raises(ValueError):                                               # two pitches in one call
        _launch(gpu, b, ests=[_pitch4(gpu, np.zeros((b.total_points, 3))), b.ests[0]])
    with pytest.raises(ValueError):                                               # a table of another result count
        bk, tw, rj, _ = _tables(gpu, b.sweeps, 2)
        flow_metrics(bk, tw, rj, b.offsets, b.pose0, b.pose1, b.pc0, b.gt, b.ests, b.category, b.ground, accuracy=_tables(gpu, 1, 3)[3])
    # a null d_accuracy computes the v1 tables alone: rows of pitch 4 in full mode, and residual mode
    old = _launch(gpu, b, accuracy=False)
    new = _launch(gpu, b, ests=[_pitch4(gpu, np.concatenate([f["a"] for f in frames])), None], accuracy=False)
    for x, y in zip(old[:3], new[:3]):
        assert torch.equal(x, y)
    with_table = _launch(gpu, b, ests=[_pitch4(gpu, np.concatenate([f["res"] for f in frames])), None], residual=True)
    without = _launch(gpu, b, ests=[_pitch4(gpu, np.concatenate([f["res"] for f in frames])), None], accuracy=False, residual=True)
    for x, y in zip(with_table[:3], without[:3]):
        assert torch.equal(x, y)
    assert int(without[0].sum()) > 0


def test_a_batch_of_resident_tensors_needs_no_host_trip(gpu, fixture_frames):
    import torch
    from himo_amd.eval_flow import FlowBatch, FlowMetrics
    f = fixture_frames[1]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(gpu)      # noqa: E731
    b = FlowBatch.from_device(up(f["pc0"], np.float32), up(f["flow"], np.float32), [_pitch4(gpu, f["res"])], up(f["flow_category_indices"], np.uint8),
                              up(f["gm0"], np.uint8), f["pose0"], f["pose1"], keys=[7])
    assert b.sweeps == 1 and b.total_points == 300 and b.offsets.cpu().tolist() == [0, 300] and b.pose0.shape == (1, 4, 4)
    m = FlowMetrics(["val"], "av2", accuracy=True, residual=True)
    m.add_batch(b)
    _, wt, _, wa = acc.flow_accuracy_ref([f], ["res"], "av2", residual=True)
    assert list(m.threeway) == [7] and np.array_equal(m.accuracy, wa) and np.array_equal(m.threeway[7][..., 0], wt[0][..., 0])
    with pytest.raises(ValueError):
        FlowBatch.from_device(b.pc0, b.gt, b.ests, b.category, b.ground, f["pose0"], f["pose1"], offsets_host=[0, 299])


def test_program_with_the_accuracy_flag_over_the_golden_scenes(gpu, capsys, tmp_path):
    from himo_amd import eval_flow
    from himo_amd.dataset import FLOW_EVAL_FIELDS, open_dataset
    names = ["seflowpp_best", "raw"]
    ds = open_dataset(H5, vis_name=["seflowpp_best"], eval=True, fields=FLOW_EVAL_FIELDS + ("seflowpp_best",))
    frames = [ds[i] for i in range(len(ds))]
    assert_clear_of_edges(frames, 1e-9)
    assert min(acc.threshold_margin(frames, n) for n in names) >= 1e-9
    _, _, _, wa = acc.flow_accuracy_ref(frames, names, "av2")
    assert wa[0, 0, 0] > 0
    path = tmp_path / "flow.json"
    m = eval_flow._cli(["--data_dir", str(H5), "--res_names", "seflowpp_best,raw", "--data_name", "av2", "--json", str(path), "--accuracy"])
    out = capsys.readouterr().out
    assert out == m.table() and out.count("accuracy strict ") == 2 and out.count("accuracy relaxed") == 2
    assert np.array_equal(m.accuracy, wa)
    back = json.loads(path.read_text())
    same = lambda x, y: (x != x and y != y) or x == y             # noqa: E731  (nan round-trips as nan)
    for r, name in enumerate(names):
        strict, relaxed = acc.accuracy_means(wa[r])
        for g in acc.GROUPS:
            assert same(back[name]["acc_strict"][g], strict[g]) and same(back[name]["acc_relaxed"][g], relaxed[g])
    # without the flag: what the program printed and wrote before
    plain_path = tmp_path / "plain.json"
    plain = eval_flow._cli(["--data_dir", str(H5), "--res_names", "seflowpp_best,raw", "--data_name", "av2", "--json", str(plain_path)])
    out = capsys.readouterr().out
    assert "accuracy" not in out and out == plain.table()
    written = json.loads(plain_path.read_text())
    assert all("acc_strict" not in written[n] and "acc_relaxed" not in written[n] for n in names)
    assert all(set(back[n]) - set(written[n]) == {"acc_strict", "acc_relaxed"} for n in names)
    assert np.array_equal(plain.buckets, m.buckets) and np.array_equal(plain.rejected, m.rejected)
