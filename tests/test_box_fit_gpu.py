"""Cluster boxes on the GPU: ``himo_boxfit`` against the numpy restatement of the rule (tests/boxfit_ref.py) at the sizes and inputs where
the kernel takes another path.  ``info`` matches bit for bit; ``box`` matches bit for bit except columns 6-8, the mean motion, whose
summation order is not part of the rule: they agree within 1e-12 relative, and a mean that is exactly 0 in the restatement is
exactly 0 on the device.  Small sweeps: every case is a few thousand rows."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest

import boxfit_ref as ref

pytestmark = pytest.mark.gpu

CHUNK = 1024                                    # HIMO_BOXFIT_CHUNK: the points the kernel stages in LDS at a time


def blob(rng, n, centre, yaw=None, spread=1.0):
    """n points of an L-shape (or, for tiny n, whatever of it n draws give) about ``centre``, with z and a fourth column"""
    yaw = rng.uniform(0, math.pi / 2) if yaw is None else yaw
    xy = ref.lshape(rng, n, yaw, 4.5 * spread, 1.9 * spread, 0.02, centre)
    return np.concatenate([xy, rng.uniform(-0.5, 1.5, (n, 1)), rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)


def sweep(sizes, seed, loose=200, shuffle=True):
    """clusters of the given sizes (label i + 1) on a grid of centres, ``loose`` rows of label 0 among them, rows in random order:
    (pts float32 [N, 4], labels int32 [N], motion float32 [N, 3])"""
    rng = np.random.default_rng(seed)
    pts, labels = [], []
    for i, n in enumerate(sizes):
        centre = (-40.0 + 12.0 * (i % 8) + rng.uniform(-1, 1), -40.0 + 12.0 * (i // 8) + rng.uniform(-1, 1))
        pts.append(blob(rng, n, centre))
        labels.append(np.full(n, i + 1, np.int32))
    pts.append(np.concatenate([rng.uniform(-50, 50, (loose, 2)), rng.uniform(-1, 2, (loose, 2))], axis=1).astype(np.float32))
    labels.append(np.zeros(loose, np.int32))
    pts, labels = np.concatenate(pts), np.concatenate(labels)
    order = rng.permutation(len(pts)) if shuffle else np.arange(len(pts))
    pts, labels = pts[order], labels[order]
    motion = (rng.normal(0, 0.3, (len(pts), 3)) + np.array([1.5, -0.7, 0.0])).astype(np.float32)
    return pts, labels, motion


def device_fit(gpu, pts, labels, C, dirs=None, motion=None, pitch_view=None, **params):
    """(info, box) host copies of one ``himo_boxfit`` call on the current stream"""
    import torch
    from himo_amd import box_fit
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(gpu) if not isinstance(pts, torch.Tensor) else pts
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(gpu)
    mo = None if motion is None else torch.from_numpy(np.ascontiguousarray(motion)).to(gpu)
    info, box, _ = box_fit.fit_labelled(p, lab, C, ref.directions() if dirs is None else dirs, box_fit.BoxParams(**params), mo)
    return info, box


def same(info, box, want_info, want_box, motion=None):
    info, box = info.cpu().numpy(), box.cpu().numpy()
    assert info.dtype == np.int32 and box.dtype == np.float64 and info.shape == want_info.shape and box.shape == want_box.shape
    bad = np.flatnonzero((info != want_info).any(axis=1))
    assert len(bad) == 0, (bad[:5], info[bad[:1]], want_info[bad[:1]])
    exact = [0, 1, 2, 3, 4, 5, 9]
    assert box[:, exact].tobytes() == want_box[:, exact].tobytes(), np.abs(box[:, exact] - want_box[:, exact]).max()
    err = np.abs(box[:, 6:9] - want_box[:, 6:9])
    assert (err <= 1e-12 * np.abs(want_box[:, 6:9])).all(), (err.max(), (err / np.maximum(np.abs(want_box[:, 6:9]), 1e-300)).max())


# ---- cluster sizes: wave, block and chunk edges -------------------------------------------------------------------------------------------
SIZES = (8, 7, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 1)


@functools.lru_cache(maxsize=None)
def sizes_case():
    pts, labels, motion = sweep(SIZES, seed=11)
    return pts, labels, motion, ref.fit(pts, labels, len(SIZES), motion=motion)


def test_cluster_sizes_at_the_wave_block_and_chunk_edges(gpu):
    pts, labels, motion, (want_info, want_box) = sizes_case()
    assert want_info[:, 0].tolist() == [ref.FITTED, ref.TOO_FEW] + [ref.FITTED] * 10 + [ref.TOO_FEW] and want_info[:, 1].tolist() == list(SIZES)
    info, box = device_fit(gpu, pts, labels, len(SIZES), motion=motion)
    same(info, box, want_info, want_box, motion)
    assert (want_info[want_info[:, 0] == ref.FITTED, 10] == want_info[want_info[:, 0] == ref.FITTED, 1]).all()      # every motion row counted


def test_max_points_and_the_extent_bound(gpu):
    rng = np.random.default_rng(12)
    sizes = (300, 301, 40, 40, 40, 40)
    pts, labels, motion = sweep(sizes, seed=12)
    # clusters 3 .. 6: two rows pinned so that the extent is 16383 / 16384 sub-units in x, then in y
    for lab, axis, span in ((3, 0, 16383), (4, 0, 16384), (5, 1, 16383), (6, 1, 16384)):
        rows = np.flatnonzero(labels == lab)
        pts[rows, axis] = rng.uniform(-20.0, 20.0, len(rows)).astype(np.float32)
        pts[rows[0], axis], pts[rows[1], axis] = -64.0, np.float32(-64.0 + span / 128.0)
    want_info, want_box = ref.fit(pts, labels, len(sizes), motion=motion, max_points=300)
    assert want_info[:, 0].tolist() == [ref.FITTED, ref.TOO_LARGE, ref.FITTED, ref.TOO_LARGE, ref.FITTED, ref.TOO_LARGE]
    same(*device_fit(gpu, pts, labels, len(sizes), motion=motion, max_points=300), want_info, want_box, motion)


# ---- labels -------------------------------------------------------------------------------------------------------------------------------
def test_one_cluster_and_three_hundred(gpu):
    pts, labels, motion = sweep((500,), seed=13, loose=300)
    same(*device_fit(gpu, pts, labels, 1, motion=motion), *ref.fit(pts, labels, 1, motion=motion), motion)
    sizes = tuple(8 + (i * 7) % 13 for i in range(300))
    pts, labels, motion = sweep(sizes, seed=14, loose=500)
    dirs = ref.directions(16)
    want = ref.fit(pts, labels, 300, dirs, motion)
    assert (want[0][:, 0] == ref.FITTED).all()
    same(*device_fit(gpu, pts, labels, 300, dirs, motion), *want, motion)


def test_labels_without_usable_rows_and_rows_in_label_order(gpu):
    pts, labels, motion = sweep((50, 20, 30, 60), seed=15, shuffle=False)
    pts[labels == 2, 0] = np.nan                                   # a label with rows, none of them usable
    labels[labels == 3] = 0                                        # a label with no row at all
    want_info, want_box = ref.fit(pts, labels, 6, motion=motion)   # ... and two labels beyond the greatest one present
    assert want_info[:, :2].tolist() == [[ref.FITTED, 50], [ref.TOO_FEW, 0], [ref.TOO_FEW, 0], [ref.FITTED, 60], [ref.TOO_FEW, 0], [ref.TOO_FEW, 0]]
    same(*device_fit(gpu, pts, labels, 6, motion=motion), want_info, want_box, motion)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def test_rows_that_are_not_usable_and_motion_rows_that_are_not_finite(gpu):
    rng = np.random.default_rng(16)
    pts, labels, motion = sweep((120, 90, 200), seed=16)
    one, two, three = (np.flatnonzero(labels == k) for k in (1, 2, 3))
    pts[one[0], 0], pts[one[1], 1], pts[one[2], 2] = np.nan, np.inf, -np.inf
    pts[one[3], 0], pts[one[4], 1] = 32768.0, -32768.0             # |x * 128| == 4194304: not below the bound
    pts[one[5], 0] = 3.0e38                                        # x * scale overflows
    motion[two[0], 0], motion[two[1], 1], motion[two[2], 2] = np.nan, np.inf, -np.inf
    motion[three] = np.nan                                         # no motion row left: the mean is zeros, the count 0
    # cluster 2 sits just inside the bound, in the negative quadrant of y: the largest |X|, floors of negative values
    pts[two, 0] = (32767.5 + rng.uniform(0, 0.4, len(two))).astype(np.float32)
    pts[two, 1] = (-32767.5 - rng.uniform(0, 0.4, len(two))).astype(np.float32)
    want_info, want_box = ref.fit(pts, labels, 3, motion=motion)
    assert want_info[:, [0, 1, 10]].tolist() == [[ref.FITTED, 114, 114], [ref.FITTED, 90, 87], [ref.FITTED, 200, 0]]
    assert want_info[1, 4] > 4194000 and want_info[1, 5] < -4194000 and not want_box[2, 6:9].any()
    same(*device_fit(gpu, pts, labels, 3, motion=motion), want_info, want_box, motion)
    want = ref.fit(pts, labels, 3)                                 # motion absent
    assert not want[1][:, 6:9].any() and not want[0][:, 10].any()
    same(*device_fit(gpu, pts, labels, 3), *want)


def test_signed_zeros_in_z(gpu):
    pts, labels, _ = sweep((16, 16, 16), seed=17, loose=0)
    pts[labels == 1, 2] = np.where(np.arange(16) % 2 == 0, 0.0, -0.0).astype(np.float32)
    pts[labels == 2, 2] = np.float32(-0.0)
    pts[labels == 3, 2] = np.where(np.arange(16) % 2 == 0, -0.0, 1.0).astype(np.float32)
    want_info, want_box = ref.fit(pts, labels, 3)
    assert np.signbit(want_box[1, 2]) and not np.signbit(want_box[0, 2])
    same(*device_fit(gpu, pts, labels, 3), want_info, want_box)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def test_pitches_and_streams(gpu):
    import torch
    pts, labels, motion, want = sizes_case()
    C = len(SIZES)
    same(*device_fit(gpu, pts[:, :3].copy(), labels, C, motion=motion), *want, motion)                       # pitch 3
    wide = np.zeros((len(pts), 7), np.float32)
    wide[:, 2:6] = pts
    gapped = torch.from_numpy(wide).to(gpu)[:, 2:5]                                                          # pitch 7, an offset start
    assert gapped.stride() == (7, 1)
    same(*device_fit(gpu, gapped, labels, C, motion=motion), *want, motion)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        got = device_fit(gpu, pts, labels, C, motion=motion)
    side.synchronize()
    same(*got, *want, motion)


def test_two_calls_in_flight_on_two_streams(gpu):
    import torch
    pts, labels, motion, want = sizes_case()
    pts2, labels2, motion2 = sweep((700, 33, 1500), seed=18)
    want2 = ref.fit(pts2, labels2, 3, motion=motion2)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s1):
        got = device_fit(gpu, pts, labels, len(SIZES), motion=motion)
    with torch.cuda.stream(s2):
        got2 = device_fit(gpu, pts2, labels2, 3, motion=motion2)
    s1.synchronize()
    s2.synchronize()
    same(*got, *want, motion)
    same(*got2, *want2, motion2)


# ---- tables and parameters ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case():
    return sweep((8, 100, 333, 1100), seed=19)


@pytest.mark.parametrize("K", [1, 90, 128])
def test_table_sizes(gpu, K):
    pts, labels, motion = small_case()
    dirs = ref.directions(K)
    same(*device_fit(gpu, pts, labels, 4, dirs, motion), *ref.fit(pts, labels, 4, dirs, motion), motion)


def test_a_table_of_equal_entries_chooses_k_0_and_signed_entries_work(gpu):
    pts, labels, motion = small_case()
    dirs = np.tile(np.array([[3000, 1000]], np.int32), (77, 1))
    want = ref.fit(pts, labels, 4, dirs, motion)
    assert (want[0][:, 2] == 0).all()
    same(*device_fit(gpu, pts, labels, 4, dirs, motion), *want, motion)
    signed = np.array([[-4096, 0], [0, -4096], [4096, 4096], [-4096, 4096], [1, 0], [-2896, -2896], [0, 1]], np.int32)
    same(*device_fit(gpu, pts, labels, 4, signed, motion), *ref.fit(pts, labels, 4, signed, motion), motion)


@pytest.mark.parametrize("params", [dict(tol_q=0), dict(tol_q=1024), dict(scale=64.0), dict(scale=256.0), dict(min_points=1, max_points=1 << 20)],
                         ids=["tol0", "tol1024", "scale64", "scale256", "widest"])
def test_parameters(gpu, params):
    pts, labels, motion = small_case()
    want = ref.fit(pts, labels, 4, motion=motion, **params)
    same(*device_fit(gpu, pts, labels, 4, motion=motion, **params), *want, motion)
    if params.get("tol_q") == 1024:
        assert (want[0][:, 3] == want[0][:, 1]).all()              # 8 m of tolerance: every row is an edge inlier


# ---- empty calls, refusals, determinism -----------------------------------------------------------------------------------------------------
def test_empty_calls(gpu):
    import torch
    info, box = device_fit(gpu, np.zeros((0, 3), np.float32), np.zeros(0, np.int32), 0)
    assert tuple(info.shape) == (0, 12) and tuple(box.shape) == (0, 10)
    info, box = device_fit(gpu, np.zeros((0, 4), np.float32), np.zeros(0, np.int32), 3)       # clusters without a row
    assert info.cpu().numpy().tolist() == [[ref.TOO_FEW] + [0] * 11] * 3 and not box.cpu().numpy().any()
    pts, labels, _ = small_case()
    info, box = device_fit(gpu, pts, np.zeros_like(labels), 0)                                # rows, none of them labelled
    assert tuple(info.shape) == (0, 12)
    torch.cuda.synchronize()


def test_refusals_leave_the_outputs_untouched(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.box_fit import BoxParams
    lib, P = _lib.load(), _lib.ptr
    pts, labels, motion = small_case()
    n, C = len(pts), 4
    p, lab, mo = (torch.from_numpy(a).to(gpu) for a in (pts, labels, motion))
    order = torch.argsort(torch.where(lab > 0, lab, 1 << 30), stable=True)
    off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C + 1)[1:])]).astype(np.int64)
    d_off, nc = torch.from_numpy(off).to(gpu), int(off[C])
    info = torch.full((C, 12), 7, dtype=torch.int32, device=gpu)
    box = torch.full((C, 10), 7.0, dtype=torch.float64, device=gpu)
    ws = torch.zeros(int(lib.himo_boxfit_workspace_bytes(nc, C, 90)), dtype=torch.uint8, device=gpu)
    dirs, prm = ref.directions(90), BoxParams().c_struct()

    def call(**kw):
        a = dict(n=n, pts=P(p), pitch=4, labels=P(lab), nc=nc, rows=P(order), C=C, h_off=off.ctypes.data, d_off=P(d_off), motion=P(mo),
                 dirs=dirs.ctypes.data, K=90, prm=ctypes.addressof(prm), info=P(info), box=P(box), ws=P(ws), ws_bytes=ws.numel())
        a.update(kw)
        return lib.himo_boxfit(a["n"], a["pts"], a["pitch"], a["labels"], a["nc"], a["rows"], a["C"], a["h_off"], a["d_off"], a["motion"],
                               a["dirs"], a["K"], a["prm"], a["info"], a["box"], a["ws"], a["ws_bytes"], _lib.stream_handle())
    short, zero_dir = off.copy(), dirs.copy()
    short[C] -= 1
    zero_dir[5] = 0
    bad = [BoxParams().c_struct() for _ in range(4)]
    bad[0].scale, bad[1].tol_q, bad[2].min_points, bad[3].max_points = float("inf"), 1025, 0, 1
    refused = [dict(pitch=2), dict(K=0), dict(K=129), dict(nc=n + 1), dict(h_off=short.ctypes.data), dict(dirs=zero_dir.ctypes.data), dict(pts=None),
               dict(info=None), dict(C=-1), dict(motion=P(mo) + 2)] + [dict(prm=ctypes.addressof(b)) for b in bad]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    for kw in (dict(ws=None), dict(ws_bytes=ws.numel() - 256), dict(ws=P(ws) + 4)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    torch.cuda.synchronize()
    assert (info == 7).all() and (box == 7.0).all() and not ws.any()
    assert call() == _lib.OK                                        # the same call, admitted, writes
    torch.cuda.synchronize()
    same(info, box, *ref.fit(pts, labels, C, motion=motion), motion)


def test_two_runs_give_the_same_bytes(gpu):
    pts, labels, motion, _ = sizes_case()
    a, b = device_fit(gpu, pts, labels, len(SIZES), motion=motion), device_fit(gpu, pts, labels, len(SIZES), motion=motion)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


# ---- BoxFitter.fit -------------------------------------------------------------------------------------------------------------------------
def test_fitter_keeps_arbitrary_ids(gpu):
    from himo_amd.box_fit import BoxFitter
    pts, labels, motion = sweep((60, 5, 90, 40, 120), seed=20)
    names = np.array([0, 4000000000, 7, 16777216, 3, 2 ** 31 + 5], dtype=np.uint32)        # 0 = none; ids far from 1..C, out of order
    ids = names[labels]
    got = BoxFitter(gpu).fit(pts, ids, motion)
    rows, moving, info, box, uniq = ref.fit_rows(pts, ids, motion)
    assert got.ids.tolist() == uniq.tolist() == sorted(int(v) for v in names[1:])
    same(got.device_info, got.device_box, info, box, motion)
    assert got.info.tobytes() == got.device_info.cpu().numpy().tobytes() and got.box.shape == (5, 10)
    assert got.rows.shape == rows.shape == (4, 12) and got.rows.dtype == np.float32
    assert got.labels.tolist() == [3, 16777216, 2 ** 31 + 5, 4000000000]                    # the cluster of 5 rows has no box
    assert got.rows[:, 10].tolist() == [3.0, 16777216.0, float(np.float32(2 ** 31 + 5)), 4000000000.0]   # column 10: the id as float32
    assert got.rows[:, [0, 1, 2, 3, 4, 5, 6, 10, 11]].tobytes() == rows[:, [0, 1, 2, 3, 4, 5, 6, 10, 11]].tobytes()
    assert np.allclose(got.rows[:, 7:10], rows[:, 7:10], rtol=1e-6, atol=0) and got.moving.tolist() == moving.tolist() == [True] * 4
    # signed ids, a tensor on the device, no motion
    import torch
    signed = torch.from_numpy(np.where(labels > 0, labels.astype(np.int64) * 1000 - 2500, 0)).to(gpu)
    got = BoxFitter(gpu, K=45).fit(torch.from_numpy(pts).to(gpu), signed)
    rows, moving, info, box, uniq = ref.fit_rows(pts, signed.cpu().numpy(), None, K=45)
    assert got.ids.tolist() == uniq.tolist() == [-1500, -500, 500, 1500, 2500]
    assert got.rows.tobytes() == rows.tobytes() and not got.moving.any()


# ---- the program ----------------------------------------------------------------------------------------------------------------------------
def _drive(root, sweeps=2):
    """an npz directory of ``sweeps`` sweeps: one vehicle at 30 m/s swept over dt in [0, 0.1), one parked car, loose points; the stored
    flow ``flow`` is the true one, the poses are the identity"""
    from himo_amd.dataset import NpzDataset
    frames = []
    for k in range(sweeps):
        rng = np.random.default_rng(30 + k)
        yaw = 0.4 + 0.1 * k
        heading = np.array([math.cos(yaw), math.sin(yaw), 0.0])
        n_fast, n_parked, n_loose = 300, 150, 100
        fast = blob(rng, n_fast, (15.0, 5.0), yaw)[:, :3].astype(np.float64)
        parked = blob(rng, n_parked, (-12.0, -9.0))[:, :3]
        loose = np.concatenate([rng.uniform(-40, 40, (n_loose, 2)), rng.uniform(0, 2, (n_loose, 1))], axis=1)
        n = n_fast + n_parked + n_loose
        dt = rng.uniform(0, 0.1, n).astype(np.float32)
        fast = fast + 30.0 * dt[:n_fast, None].astype(np.float64) * heading
        flow = np.zeros((n, 3), np.float32)
        flow[:n_fast] = (3.0 * heading).astype(np.float32)
        ids = np.concatenate([np.full(n_fast, 901), np.full(n_parked, 17), np.zeros(n_loose)]).astype(np.int32)
        order = rng.permutation(n)
        pc0 = np.concatenate([fast, parked, loose]).astype(np.float32)[order]
        frames.append({"scene_id": "s0", "timestamp": 1000 + k, "pc0": pc0, "pose0": np.eye(4), "pose1": np.eye(4), "lidar_dt": dt[order],
                       "flow": flow[order], "ids": ids[order]})
    NpzDataset.write(root, frames)
    return frames


def test_program_writes_boxes_and_its_numbers_are_the_restatements(gpu, tmp_path, monkeypatch, capsys):
    import torch
    from himo_amd import box_fit
    from himo_amd.accumulate import flow_motion
    from himo_amd.compdis import CompDisEngine
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "drive"
    frames = _drive(root)
    out = tmp_path / "boxes.json"
    numbers = box_fit.main(str(root), "raw,flow", "ids", against="raw", json_path=str(out))
    assert json.loads(out.read_text()) == numbers
    assert "cluster boxes, v1; parity unpinned" in capsys.readouterr().out
    # the same numbers from the restatement, on the points and motions the package's own earlier stages give
    engine = CompDisEngine()
    totals = {s: box_fit.new_totals() for s in ("raw", "flow")}
    versus = {s: box_fit.new_against() for s in ("raw", "flow")}
    for f in frames:
        pc0 = torch.from_numpy(f["pc0"]).to(gpu)
        comp = engine.run_frame(pc0, torch.from_numpy(f["flow"]).to(gpu), torch.from_numpy(f["lidar_dt"]).to(gpu), f["pose0"], f["pose1"],
                                refined=True)[1].cpu().numpy()
        motion = flow_motion(pc0, f["flow"], f["pose0"], f["pose1"]).cpu().numpy()
        want = {"raw": ref.fit_rows(f["pc0"], f["ids"], motion), "flow": ref.fit_rows(comp, f["ids"], motion)}
        with np.load(root / "s0" / f"{f['timestamp']}.npz") as z:
            for s in ("raw", "flow"):
                rows, moving = want[s][0], want[s][1]
                got = z[f"boxes_{s}"]
                assert got.dtype == np.float32 and got.shape == rows.shape == (2, 12)
                assert got[:, [0, 1, 2, 3, 4, 5, 6, 10, 11]].tobytes() == rows[:, [0, 1, 2, 3, 4, 5, 6, 10, 11]].tobytes()
                assert np.allclose(got[:, 7:10], rows[:, 7:10], rtol=1e-6, atol=1e-9)
                assert got[:, 10].tolist() == [17.0, 901.0] and moving.tolist() == [False, True]
                box_fit.tally(totals[s], rows, moving)
                labels = want[s][4][want[s][2][:, 0] == ref.FITTED]
                box_fit.tally_against(versus[s], rows, moving, labels, want["raw"][0], want["raw"][1], labels)
            # the vehicle: smeared by up to 3 m as recorded, its true size once compensated; it heads where it moves
            raw_l, comp_l = z["boxes_raw"][1, 3], z["boxes_flow"][1, 3]
            assert raw_l - comp_l > 1.0 and abs(comp_l - 4.5) <= 0.2 and abs(z["boxes_flow"][1, 4] - 1.9) <= 0.2
            assert abs(z["boxes_flow"][1, 6] - (0.4 + 0.1 * (f["timestamp"] - 1000))) <= math.radians(2.0)
            true_yaw = 0.4 + 0.1 * (f["timestamp"] - 1000)
            assert np.allclose(z["boxes_flow"][1, 7:10], [30.0 * math.cos(true_yaw), 30.0 * math.sin(true_yaw), 0.0], atol=1e-3)
    recomputed = box_fit.summary(totals, versus, "raw")
    for s in ("raw", "flow"):
        a, b = numbers[s], recomputed[s]
        assert (a["boxes"], a["moving"]) == (b["boxes"], b["moving"]) == (4, 2)
        assert a["mean_l_moving"] == pytest.approx(b["mean_l_moving"], rel=1e-9) and a["mean_w_moving"] == pytest.approx(b["mean_w_moving"], rel=1e-9)
        for key in ("all", "moving"):
            assert a["against"][key]["pairs"] == b["against"][key]["pairs"] == (4 if key == "all" else 2)
            for col in ("mean_dl", "mean_dw", "mean_centre", "mean_yaw_deg"):
                assert a["against"][key][col] == pytest.approx(b["against"][key][col], rel=1e-9, abs=1e-12), (s, key, col)
    assert numbers["raw"]["against"]["all"]["mean_dl"] == 0.0 and numbers["flow"]["against"]["moving"]["mean_dl"] > 1.0
    # a second run is refused, and leaves the files alone; --overwrite replaces
    with pytest.raises(FileExistsError, match="boxes_raw.*--overwrite"):
        box_fit.main(str(root), "raw,flow", "ids")
    box_fit._cli(["--data_dir", str(root), "--res_names", "flow", "--label_key", "ids", "--overwrite", "--directions", "45"])
    with np.load(root / "s0" / "1000.npz") as z:
        assert z["boxes_flow"].shape == (2, 12) and z["boxes_raw"].shape == (2, 12)


def test_program_clusters_when_asked(gpu, tmp_path, monkeypatch):
    from himo_amd import box_fit
    from himo_amd.dataset import NpzDataset
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "drive"
    frames = _drive(root, sweeps=1)
    for f in frames:
        f["gm0"] = np.zeros(len(f["pc0"]), bool)
        f["pc0"][:, 2] *= 0.25                                     # 0.5 m tall: every object is far denser than min_pts within eps
    NpzDataset.write(root, frames)
    numbers = box_fit.main(str(root), "raw,flow", "cluster")
    # compensated, the vehicle and the parked car are one dense cluster each (the loose points are no cluster at eps = 0.5 m)
    assert numbers["flow"]["boxes"] == 2 and numbers["flow"]["moving"] == 1 and "against" not in numbers["flow"]
    assert abs(numbers["flow"]["mean_l_moving"] - 4.5) <= 0.2 and numbers["raw"]["boxes"] >= 1
    with np.load(root / "s0" / "1000.npz") as z:
        assert z["boxes_flow"].shape[1] == 12 and z["boxes_raw"].dtype == np.float32


def test_program_on_h5_scene_files(gpu, tmp_path, monkeypatch):
    """the scene-file branch: boxes held back per scene, written into <scene>.h5 once its reads are done, refused when there"""
    import warnings
    from himo_amd import box_fit, synthetic
    from himo_amd.accumulate import flow_motion
    from himo_amd.dataset import HDF5Dataset, h5_reader
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "scenes"
    root.mkdir()
    synthetic.write_h5_scenes(root, [synthetic.make_scene(s, 3, n_points=3000, n_instances=4, scene_id=f"sc{s}") for s in (1, 2)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # (the last sweep of a scene has no successor)
        numbers = box_fit.main(str(root), "raw,flow", "flow_instance_id", against="raw")
        ds = HDF5Dataset(root, vis_name="", fields=("pc0", "pose0", "pose1", "flow", "flow_instance_id"))
    assert len(ds) == 4
    boxes = 0
    for i in range(len(ds)):
        f = ds[i]
        motion = flow_motion(f["pc0"], f["flow"], f["pose0"], f["pose1"]).cpu().numpy()
        rows, moving, _, _, _ = ref.fit_rows(np.asarray(f["pc0"])[:, :3], np.asarray(f["flow_instance_id"]), motion)
        with h5_reader().File(root / f"{f['scene_id']}.h5", "r") as h:
            got = np.asarray(h[str(f["timestamp"])]["boxes_raw"][:])
            comp = np.asarray(h[str(f["timestamp"])]["boxes_flow"][:])
        assert got.dtype == np.float32 and got.shape == rows.shape and got.shape[1] == 12 and comp.shape == got.shape and len(got) >= 1
        assert got[:, [0, 1, 2, 3, 4, 5, 6, 10, 11]].tobytes() == rows[:, [0, 1, 2, 3, 4, 5, 6, 10, 11]].tobytes()
        assert np.allclose(got[:, 7:10], rows[:, 7:10], rtol=1e-6, atol=1e-9)
        boxes += len(rows)
    ds.close()
    assert numbers["raw"]["boxes"] == numbers["flow"]["boxes"] == boxes and numbers["flow"]["against"]["all"]["pairs"] == boxes
    with h5_reader().File(root / "sc1.h5", "r") as h:               # the sweep without a successor holds none
        assert not [k for k in h[sorted(h.keys())[-1]].keys() if k.startswith("boxes_")]
    with pytest.raises(FileExistsError, match="boxes_raw.*--overwrite"):
        box_fit.main(str(root), "raw", "flow_instance_id")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        again = box_fit.main(str(root), "raw", "flow_instance_id", overwrite=True)
    assert again["raw"]["boxes"] == boxes
