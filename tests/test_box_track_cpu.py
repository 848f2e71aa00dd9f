"""Box tracking without a GPU: the restatement of the rule (tests/boxtrack_ref.py) against exact expectations, and the host glue of
himo_amd/track.py (rule A, rule F, the tables, the refusals) against the restatement and hand-written arrays."""
import ctypes
import math

import numpy as np
import pytest

import boxtrack_ref as ref
from himo_amd import track

DT = 0.1


def det_row(x, y, yaw=0.0, v=(0.0, 0.0), l=4.5, w=1.9, z=0.5, h=1.6):
    return [x, y, z, l, w, h, math.cos(yaw), math.sin(yaw), v[0], v[1], 0.0, 0.0]


def table(*rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 12)


# ---- constant velocity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_constant_velocity_keeps_one_id_each(mode):
    speeds, yaws = (0.0, 5.0, 30.0), (0.3, -2.0, 1.1)
    vel = [(v * math.cos(a), v * math.sin(a)) for v, a in zip(speeds, yaws)]
    start = [(-20.0, 0.0), (0.0, 15.0), (25.0, -30.0)]
    dets = [table(*[det_row(p[0] + u[0] * (k * DT), p[1] + u[1] * (k * DT), a, u) for p, u, a in zip(start, vel, yaws)]) for k in range(20)]
    out, n_ids, overflow = ref.track_scene(dets, [DT] * 20, vel_mode=mode)
    assert n_ids == 3 and overflow == 0
    for k, (tid, age, state, iou, live) in enumerate(out):
        assert tid.tolist() == [0, 1, 2] and age.tolist() == [k + 1] * 3 and live == 3
        if mode == 0:                                               # prediction and detection differ by rounding only
            assert np.abs(state[:, 0:2] - dets[k][:, 0:2]).max() <= 1e-9
            assert np.abs(state[:, 2:4] - np.array(vel)).max() <= 1e-9
            if k:
                assert (iou > 0.999999).all()
    if mode == 1:                                                   # the velocity is learnt from the residuals
        assert np.abs(out[-1][2][:, 2:4] - np.array(vel)).max() < 0.1


def test_crossing_boxes_keep_their_ids():
    # one box along +x, one along +y, through the same point at the same time
    dets = [table(det_row(-10.0 + 10.0 * k * DT, 0.0, 0.0, (10.0, 0.0)), det_row(0.0, -10.0 + 10.0 * k * DT, math.pi / 2, (0.0, 10.0))) for k in range(21)]
    order = [k % 2 for k in range(21)]                              # the rows swap places every other sweep
    shown = [d[::-1].copy() if o else d for d, o in zip(dets, order)]
    out, n_ids, _ = ref.track_scene(shown, [DT] * 21)
    assert n_ids == 2
    for (tid, _, _, _, live), o in zip(out, order):
        assert tid.tolist() == ([1, 0] if o else [0, 1]) and live == 2


# ---- coasting, births, deaths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_age", [0, 2])
def test_coasting_through_max_age(max_age):
    def scene(gap):
        rows = [table(det_row(5.0 * k * DT, 0.0, 0.0, (5.0, 0.0)), det_row(0.0, 20.0)) for k in range(4 + gap + 2)]
        for k in range(4, 4 + gap):
            rows[k] = rows[k][1:].copy()                            # the moving box is not seen
        return rows
    kept, n_ids, _ = ref.track_scene(scene(max_age), [DT] * 20, max_age=max_age)
    assert n_ids == 2 and kept[-1][0].tolist() == [0, 1] and kept[-1][1].tolist() == [6, 6 + max_age]
    assert [o[4] for o in kept] == [2] * len(kept)                  # the coasting track stays in the table
    lost, n_ids, _ = ref.track_scene(scene(max_age + 1), [DT] * 20, max_age=max_age)
    assert n_ids == 3 and lost[-1][0].tolist() == [2, 1] and lost[-1][1].tolist() == [2, 7 + max_age]
    assert [o[4] for o in lost] == [2] * (4 + max_age) + [1] + [2, 2]


def test_births_in_ascending_j_and_overflow_at_max_tracks_plus_one():
    rows = table(*[det_row(10.0 * j, 0.0) for j in range(6)])
    out, n_ids, overflow = ref.track_scene([rows[[3, 1, 5, 0, 4, 2]], rows], [DT, DT], max_tracks=5)
    assert out[0][0].tolist() == [0, 1, 2, 3, 4, -1] and out[0][4] == 5 and n_ids == 5 and overflow == 2
    assert out[1][0].tolist() == [3, 1, -1, 0, 4, 2] and out[1][1].tolist() == [2, 2, 0, 2, 2, 2] and out[1][4] == 5
    exact, n_ids, overflow = ref.track_scene([rows[:5]], [DT], max_tracks=5)
    assert exact[0][0].tolist() == [0, 1, 2, 3, 4] and overflow == 0 and n_ids == 5
    # a death makes room: ids are never reused
    out, n_ids, overflow = ref.track_scene([rows[:5], rows[1:6]], [DT, DT], max_tracks=5, max_age=0)
    assert out[1][0].tolist() == [1, 2, 3, 4, 5] and n_ids == 6 and overflow == 0


def test_invalid_rows_get_minus_one_and_disturb_nothing():
    good = [table(det_row(3.0 * k * DT, 0.0, 0.0, (3.0, 0.0)), det_row(20.0, 5.0, 0.7)) for k in range(5)]
    want, n_ids, _ = ref.track_scene(good, [DT] * 5)
    bad = []
    for k, d in enumerate(good):
        junk = table(det_row(3.0 * k * DT, 0.0), det_row(20.0, 5.0, 0.7), det_row(1.0, 1.0), det_row(-30.0, 0.0))
        junk[0, 3], junk[1, 0], junk[2, 11], junk[3] = -1.0, math.inf, math.nan, math.nan
        bad.append(np.concatenate([junk[:2], d[:1], junk[2:], d[1:]]))
    got, n2, over = ref.track_scene(bad, [DT] * 5)
    assert n2 == n_ids == 2 and over == 0
    for (tid, age, state, iou, live), (wt, wa, ws, wi, wl) in zip(got, want):
        assert tid.tolist() == [-1, -1, wt[0], -1, -1, wt[1]] and live == wl
        assert age[[2, 5]].tolist() == wa.tolist() and not age[[0, 1, 3, 4]].any()
        assert state[[2, 5]].tobytes() == ws.tobytes() and iou[[2, 5]].tobytes() == wi.tobytes() and not state[[0, 1, 3, 4]].any()


def test_exact_ties_go_to_the_lower_track_then_the_lower_detection():
    one = det_row(0.0, 0.0)
    # two tracks on the same box (born from duplicate rows), then ONE detection: the lower slot takes it
    out, n_ids, _ = ref.track_scene([table(one, one), table(one), table(one, one, one)], [DT] * 3)
    assert out[0][0].tolist() == [0, 1] and out[1][0].tolist() == [0] and out[1][4] == 2
    assert out[2][0].tolist() == [0, 1, 2] and out[2][1].tolist() == [3, 2, 1] and n_ids == 3
    # one track, two detections mirror-symmetric about it: equal IoUs, the lower j is matched, the other is born
    out, _, _ = ref.track_scene([table(det_row(0.0, 0.0, l=4.0, w=2.0)), table(det_row(1.0, 0.0, l=4.0, w=2.0), det_row(-1.0, 0.0, l=4.0, w=2.0))], [DT, DT])
    assert out[1][0].tolist() == [0, 1] and out[1][3].tolist() == [0.6, 0.0]


# ---- rule A and rule F: the host glue ----------------------------------------------------------------------------------------------------
def pose(x, y, yaw, z=0.0):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, z], [0.0, 0.0, 0.0, 1.0]])


def test_moving_ego_with_static_objects():
    import boxeval_ref as be
    world = [(12.0, 4.0, 0.3), (-8.0, -15.0, 1.9), (30.0, 22.0, -2.5)]
    poses = [pose(1.2 * k, 0.1 * k * k, 0.02 * k, 0.01 * k) for k in range(12)]
    rows = []
    for P in poses:
        inv = np.linalg.inv(P)
        ego_yaw = math.atan2(P[1, 0], P[0, 0])
        c = np.array([inv @ [x, y, 0.5, 1.0] for x, y, _ in world])
        r = be.box_rows(c[:, :2], np.tile([4.5, 1.9], (3, 1)), [a - ego_yaw for _, _, a in world]).astype(np.float64)
        r[:, 0:2], r[:, 6] = c[:, :2], [a - ego_yaw for _, _, a in world]      # (float64 rows: rounding alone separates the sweeps)
        rows.append(r)
    dets = [track.detections(r, P, poses[0]) for r, P in zip(rows, poses)]
    for r, P, d in zip(rows, poses, dets):
        assert d.tobytes() == ref.detections(r, P, poses[0]).tobytes()       # the vectorised rule A is the restatement's
    for mode in (0, 1):
        out, n_ids, _ = ref.track_scene(dets, [DT] * 12, vel_mode=mode)
        assert n_ids == 3
        for k, (tid, age, state, _, _) in enumerate(out):
            assert tid.tolist() == [0, 1, 2]
            assert np.abs(state[:, 2:4]).max() < 1e-9
            got = track.stored_rows(tid, age, state, dets[k], poses[k], poses[0])
            assert got.tobytes() == ref.stored_rows(tid, age, state, dets[k], poses[k], poses[0]).tobytes()
            assert np.abs(got[:, 2:4] - rows[k][:, 0:2]).max() < 1e-9      # back in the sensor frame: the boxes' own centres
    # the round trip alone, on float64: W and back
    d = dets[5]
    back = track.stored_rows(np.arange(3), np.ones(3), d[:, [0, 1, 8, 9]], d, poses[5], poses[0])
    assert np.abs(back[:, 2:4] - rows[5][:, 0:2]).max() < 1e-12


def test_rule_a_invalid_rows_and_shapes():
    import boxeval_ref as be
    rows = be.box_rows([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [9.0, 1.0]], np.tile([4.0, 2.0], (5, 1)), [0.1, 0.2, 0.3, 0.4, 0.5], vel=np.ones((5, 2)))
    rows[0, 3], rows[1, 6], rows[2, 7], rows[3, 2] = -1.0, np.inf, np.nan, np.inf
    got = track.detections(rows, np.eye(4), np.eye(4))
    assert np.isnan(got[:4]).all() and np.isfinite(got[4]).all() and got.tobytes() == ref.detections(rows, np.eye(4), np.eye(4)).tobytes()
    assert got[4].tolist() == [9.0, 1.0, 0.5, 4.0, 2.0, float(np.float32(1.6)), math.cos(0.5), math.sin(0.5), 1.0, 1.0, 0.0, 0.0]
    assert track.detections(np.zeros((0, 12), np.float32), np.eye(4), np.eye(4)).shape == (0, 12)
    with pytest.raises(ValueError, match="box rows"):
        track.detections(np.zeros((3, 7)), np.eye(4), np.eye(4))
    with pytest.raises(ValueError, match="poses"):
        track.detections(rows, np.eye(3), np.eye(4))


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------
def gt_rows(ids, speed=0.0):
    import boxeval_ref as be
    r = be.box_rows(np.zeros((len(ids), 2)), np.tile([4.0, 2.0], (len(ids), 1)), np.zeros(len(ids)), ids=ids)
    r[:, 7] = speed
    return r


def test_mot_tallies_on_hand_written_arrays():
    sums = track.new_sums()
    # identity 7: track 0, 0, (unmatched), 0 -> one fragmentation; identity 9 (at 15 m/s): track 1, 2 -> one switch; then IoU 0.4: FN
    sweeps = [(gt_rows([7, 9], [0.0, 15.0]), [0, 1, 5], [0, 1], [0.9, 0.8]),
              (gt_rows([7, 9], [0.0, 15.0]), [2, 0], [1, 0], [0.7, 0.6]),
              (gt_rows([7]), [0], [-1], [0.0]),
              (gt_rows([7, 9], [0.0, 15.0]), [0, 2, -1], [0, 1], [0.5, 0.4]),
              (gt_rows([11]), [-1], [0], [0.9])]                    # a partner without a track id does not match
    track.tally_mot(sums, sweeps)
    a, s, f = sums["mot"]["all"], sums["mot"]["speed static"], sums["mot"]["speed 10-20"]
    assert a == {"gt": 8, "tp": 5, "fn": 3, "idsw": 1, "frag": 1} and sums["pred"] == 10
    assert s == {"gt": 5, "tp": 3, "fn": 2, "idsw": 0, "frag": 1} and f == {"gt": 3, "tp": 2, "fn": 1, "idsw": 1, "frag": 0}
    out = track.summary({"x": sums}, True)["x"]["mot"]
    assert out["all"]["fp"] == 5 and out["all"]["mota"] == 1.0 - (3 + 5 + 1) / 8 and "fp" not in out["speed static"]
    assert out["speed 10-20"]["mota"] == 1.0 - (1 + 1) / 3 and out["speed 30+"] == {"gt": 0, "tp": 0, "fn": 0, "idsw": 0, "frag": 0, "mota": None}
    # an identity absent from a sweep is not "unmatched" there; a second scene starts afresh
    sums = track.new_sums()
    track.tally_mot(sums, [(gt_rows([7]), [0], [0], [0.9]), (gt_rows([8]), [1], [0], [0.9]), (gt_rows([7]), [0], [0], [0.9])])
    track.tally_mot(sums, [(gt_rows([7]), [4], [0], [[0.9, 0.5]])])
    assert sums["mot"]["all"] == {"gt": 4, "tp": 4, "fn": 0, "idsw": 0, "frag": 0}


def test_track_tables_on_hand_written_arrays():
    T = lambda *rows: np.array(rows, dtype=np.float64).reshape(-1, 6)       # noqa: E731
    boxes = [gt_rows([1, 2], 3.0), gt_rows([1, 2], 3.0), gt_rows([1, 2, 3], 3.0), gt_rows([1], 3.0)]
    tracks = [T([0, 1, 0, 0, 3, 0], [1, 1, 0, 0, 3, 0]), T([0, 2, 0, 0, 3, 0], [2, 1, 0, 0, 0, 0]), T([0, 3, 0, 0, 0, 4], [2, 2, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0]),
              T([0, 4, 0, 0, 3, 0])]
    sums = track.new_sums()
    track.tally_scene(sums, boxes, tracks, 3, 1, min_hits=3)
    assert (sums["ids"], sums["overflow"], sums["boxes"], sums["confirmed_boxes"], sums["lengths"], sums["jitter_n"]) == (3, 1, 8, 4, [4], 2)
    assert sums["jitter_sum"] == 5.0                                # hypot(3 - 0, 0 - 4) + 0
    two = track.add_sums({"x": sums}, {"x": {**track.new_sums(), "ids": 2, "lengths": [3, 9], "boxes": 2}})
    out = track.summary(two, False)["x"]
    assert out == {"ids": 5, "confirmed": 3, "mean_length": 16 / 3, "median_length": 4.0, "boxes": 10, "confirmed_share": 0.4, "overflow": 1,
                   "velocity_jitter": 2.5}
    empty = track.summary({"x": track.new_sums()}, True)["x"]
    assert empty["mean_length"] is None and empty["median_length"] is None and empty["confirmed_share"] is None and empty["mot"]["all"]["mota"] is None
    assert "box tracking" not in track._table("x", out, None) and "confirmed tracks" in track._table("x", empty, "flow")


def test_point_labels():
    rows = gt_rows([40, 7, 9])
    got = track.point_labels(np.array([7, 0, 9, 40, 8, 41, 7], dtype=np.int32), rows, np.array([5, -1, 3]))
    assert got.dtype == np.int32 and got.tolist() == [-1, -1, 3, 5, -1, -1, -1]
    assert track.point_labels(np.array([1, 2]), np.zeros((0, 12), np.float32), np.zeros(0)).tolist() == [-1, -1]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(min_iou=0.0), dict(min_iou=1.5), dict(min_iou=math.nan), dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=math.nan),
                                dict(beta=math.inf), dict(beta=True), dict(max_age=-1), dict(max_age=256), dict(max_age=1.0), dict(max_tracks=0),
                                dict(max_tracks=513), dict(vel_mode=2), dict(vel_mode=-1), dict(sensor_dt=0.0), dict(sensor_dt=math.nan)])
def test_parameters_are_refused_before_the_gpu_is_touched(kw, monkeypatch):
    from himo_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    with pytest.raises(ValueError):
        track.BoxTracker(**kw)


def test_binding_refuses_tables_before_the_gpu_is_touched():
    t = track.BoxTracker.__new__(track.BoxTracker)                  # (no device: the checks are the host's)
    t.params, t.sensor_dt = track.TrackParams(), 0.1
    with pytest.raises(ValueError, match="513 boxes"):
        t.tables([[np.zeros((513, 12))]])
    with pytest.raises(ValueError, match=r"float64 \[F, 12\]"):
        t.tables([[np.zeros((3, 7))]])
    with pytest.raises(ValueError, match="one time step per sweep"):
        t.tables([[np.zeros((1, 12))]], dts=[[0.1, 0.1]])
    for bad in (0.0, -0.1, math.nan, math.inf):
        with pytest.raises(ValueError, match="finite and > 0"):
            t.tables([[np.zeros((1, 12)), np.zeros((1, 12))]], dts=[[0.1, bad]])
    det, so, do, dt = t.tables([[np.zeros((2, 12)), np.zeros((0, 12))], [], [np.ones((1, 12))]], dts=[[math.nan, 0.2], [], [0.0]])
    assert det.shape == (3, 12) and so.tolist() == [0, 2, 2, 3] and do.tolist() == [0, 2, 2, 3] and dt.tolist()[1:] == [0.2, 0.0]


def _drive(root, sweeps=3, **more):
    import boxeval_ref as be
    from himo_amd.dataset import NpzDataset
    frames = []
    for k in range(sweeps):
        f = {"scene_id": "s0", "timestamp": 1000 + k, "pc0": np.zeros((5, 3), np.float32), "pose0": np.eye(4), "pose1": np.eye(4),
             "boxes_raw": be.box_rows([[1.0 + k, 2.0]], [[4.0, 2.0]], [0.0], vel=[[10.0, 0.0]]), "ids": np.array([1, 1, 0, 0, 1], np.int32)}
        f.update({key: v[k] if isinstance(v, list) else v for key, v in more.items()})
        frames.append(f)
    NpzDataset.write(root, frames)
    return frames


def test_program_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from himo_amd import _lib
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    root = tmp_path / "d"
    _drive(root)
    for kw, exc, text in ((dict(res_names=""), ValueError, "res_names"), (dict(res_names="raw,raw"), ValueError, "res_names"),
                          (dict(res_names="raw", gt="raw"), ValueError, "--gt raw is among"), (dict(res_names="raw", gt=""), ValueError, "--gt"),
                          (dict(res_names="raw", alpha=2.0), ValueError, "alpha"), (dict(res_names="raw", batch=0), ValueError, "batch"),
                          (dict(res_names="raw", min_hits=0), ValueError, "min_hits"), (dict(res_names="raw", sensor_dt=-1.0), ValueError, "sensor_dt"),
                          (dict(res_names="raw", point_label_key="cluster"), ValueError, "cluster"),
                          (dict(res_names="est"), KeyError, "boxes_est.*box_fit.*--res_names est"),
                          (dict(res_names="raw", gt="flow"), KeyError, "boxes_flow.*box_fit"),
                          (dict(res_names="raw", point_label_key="nope"), KeyError, "nope")):
        with pytest.raises(exc, match=text):
            track.main(str(root), **kw)
    import boxeval_ref as be
    many = be.box_rows(np.zeros((513, 2)), np.tile([4.0, 2.0], (513, 1)), np.zeros(513))
    for more, exc, text in ((dict(boxes_raw=np.zeros((2, 12))), ValueError, r"float64 \(2, 12\), not float32"),
                            (dict(boxes_raw=np.zeros((2, 7), np.float32)), ValueError, "not float32"),
                            (dict(boxes_raw=many), ValueError, "513 boxes: at most 512"),
                            (dict(tracks_raw=np.zeros((1, 6))), FileExistsError, "tracks_raw.*--overwrite"),
                            (dict(pose0=np.eye(3)), ValueError, "pose0"),
                            (dict(ids=np.zeros((5, 2), np.int32)), ValueError, "one integer per point")):
        root = tmp_path / ("d_" + "_".join(more))
        _drive(root, **more)
        with pytest.raises(exc, match=text):
            track.main(str(root), "raw", point_label_key="ids")
        with np.load(root / "s0" / "1000.npz") as z:                # nothing was written
            assert "track_label_raw" not in z.files and ("tracks_raw" in more or "tracks_raw" not in z.files)
    with pytest.raises(SystemExit):
        track._cli(["--data_dir", str(root), "--res_names", "raw", "--vel_mode", "both"])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_has_the_c_struct_size():
    from himo_amd import _lib
    assert ctypes.sizeof(track._CParams) == 40
    if _lib.LIB_PATH.exists():
        assert _lib.load().himo_abi_sizeof(b"himo_boxtrack_params") == ctypes.sizeof(track._CParams)
