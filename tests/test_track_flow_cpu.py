"""Track flow without a GPU: the parameters' and the program's refusals, the host preparation (rule A) against the restatement on
hand-made rows, and the restatement itself (tests/trackflow_ref.py) on the cases that say why the rule exists."""
import ctypes
import math

import numpy as np
import pytest

import trackflow_ref as ref

f32 = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


# ---- parameters and layout ----------------------------------------------------------------------------------------------------------------
def test_params_defaults_and_refusals():
    from himo_amd import track, track_flow
    from himo_amd.track_flow import TrackFlowParams
    d = TrackFlowParams()
    assert (d.sensor_dt, d.motion_min, d.half, d.min_len, d.mode) == (0.1, 0.05, 2, track.MIN_HITS, 0)
    assert track_flow.track_flow_key("seflowpp_best") == "seflowpp_best_track" and track_flow.MODES == ("shift", "replace")
    c = TrackFlowParams(sensor_dt=0.2, motion_min=0.0, half=8, min_len=1, mode=1).c_struct()
    assert (c.sensor_dt, c.motion_min, c.half, c.min_len, c.mode, c.reserved) == (0.2, 0.0, 8, 1, 1, 0)
    TrackFlowParams(half=0)
    bad = [dict(sensor_dt=0.0), dict(sensor_dt=-0.1), dict(sensor_dt=math.nan), dict(sensor_dt=math.inf), dict(sensor_dt=True), dict(sensor_dt="0.1"),
           dict(motion_min=-1e-9), dict(motion_min=math.nan), dict(motion_min=math.inf), dict(motion_min=False), dict(motion_min=None),
           dict(half=-1), dict(half=9), dict(half=2.0), dict(half=True), dict(min_len=0), dict(min_len=-3), dict(min_len=3.0), dict(min_len=2 ** 31),
           dict(mode=2), dict(mode=-1), dict(mode="shift"), dict(mode=True)]
    for kw in bad:
        with pytest.raises(ValueError, match=next(iter(kw))):
            TrackFlowParams(**kw)


def test_the_mirror_has_the_c_struct_size():
    from himo_amd import _lib
    from himo_amd.track_flow import _CParams
    assert ctypes.sizeof(_CParams) == 32 == _lib.load().himo_abi_sizeof(b"himo_trackflow_params")


# ---- rule A on hand-made rows ---------------------------------------------------------------------------------------------------------------
def hand_made():
    b = np.zeros((7, 12), f32)
    b[:, 7:10] = [[3.0, -1.5, 0.25], [1.0, 2.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [3.0e38, 3.0e38, 0.0], [0.1, 0.2, 0.3], [7.0, 7.0, 7.0]]
    b[:, 10] = [9, 4, 4, 12, 9, 1, 4]                               # duplicate label ids: 4 on rows 1, 2, 6 and 9 on rows 0, 4
    t = np.zeros((7, 6))
    t[:, 0] = [5, -1, 2, 3, 0, 7, -1]
    return b, t


def test_preparation_equals_the_restatement_on_hand_made_rows():
    from himo_amd.track_flow import ego_transform, prepare
    b, t = hand_made()
    first, pose = ref.ego_pose(0), ref.ego_pose(9)
    got, want = prepare(b, t, pose, first), ref.prepare(b, t, pose, first)
    for g, w, name in zip(got, want, got._fields):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and bits(g).tobytes() == bits(w).tobytes(), name
    assert got.id.tolist() == [5, -1, -1, -1, 0, 7, -1]             # id -1, a velocity that is not finite (NaN, inf); 3e38 stays finite in float64
    assert np.isnan(got.w[[1, 2, 3, 6]]).all() and np.isfinite(got.w[[0, 4, 5]]).all()
    assert got.sorted_id.tolist() == [1, 4, 4, 4, 9, 9, 12] and got.sorted_row.tolist() == [5, 1, 2, 6, 0, 4, 3]      # the lowest row first
    T = np.linalg.inv(first) @ pose
    assert got.w[0].tobytes() == np.array([(T[e, 0] * 3.0 + T[e, 1] * -1.5) + T[e, 2] * 0.25 for e in range(3)]).tobytes()
    assert got.U.tobytes() == np.ascontiguousarray(np.linalg.inv(T)[:3, :3]).tobytes()
    empty = prepare(np.zeros((0, 12), f32), np.zeros((0, 6)), pose, first)
    assert empty.id.shape == (0,) and empty.w.shape == (0, 3) and empty.sorted_row.shape == (0,)
    with pytest.raises(ValueError, match="one row per box"):
        prepare(b, t[:5], pose, first)
    with pytest.raises(ValueError, match=r"\[F, 12\]"):
        prepare(b[:, :9], t, pose, first)
    E = ego_transform(first, pose)
    assert E.dtype == np.float32 and E.tobytes() == ref.ego_transform(first, pose).tobytes()


def test_duplicate_label_ids_the_lowest_row_wins():
    b, t = hand_made()
    t[:, 0] = [0, 1, 2, 3, 4, 5, 6]
    b[2, 7:10] = (0.0, 0.0, 0.0)
    b[3, 7:10] = (0.0, 1.0, 0.0)
    s = ref.prepare(b, t, np.eye(4), np.eye(4))
    pl = ref.plan_scene([s], min_len=1)[0]
    assert pl.state.tolist() == [1, 1, 2, 1, 1, 2, 1]               # (row 5 moves 0.037 m a sweep: STATIC, as the zero velocity of row 2)
    pc0 = np.zeros((4, 3), f32)
    flow = np.full((4, 3), 0.5, f32)
    out, nm, ns = ref.apply_sweep(pc0, flow, [4, 9, 12, 3], np.eye(4, dtype=f32)[:3], s, pl, mode=1)
    assert (nm, ns) == (3, 0)
    assert out[0].tobytes() == pl.disp[1].tobytes() and out[1].tobytes() == pl.disp[0].tobytes() and out[2].tobytes() == pl.disp[3].tobytes()
    assert out[3].tobytes() == flow[3].tobytes()                    # a label that no box carries


# ---- the restatement: why the rule exists -----------------------------------------------------------------------------------------------------
def test_smoothing_cuts_the_velocity_noise():
    """40 tracks of 12 sweeps at constant velocity under a moving ego pose, iid Gaussian noise on every box velocity: the windows hold 3,
    4, 5, ... 5, 4, 3 boxes, so the RMS error falls to sqrt((2/3 + 2/4 + 8/5) / 12) = 0.48 of the boxes'; 0.6 leaves the sampling margin
    of 1440 components."""
    boxes, tracks, poses, truth = ref.constant_velocity_tracks(np.random.default_rng(71))
    sweeps = [ref.prepare(b, t, p, poses[0]) for b, t, p in zip(boxes, tracks, poses)]
    plans = ref.plan_scene(sweeps)
    assert [int(p.m[0]) for p in plans] == [3, 4] + [5] * 8 + [4, 3] and all((p.state == ref.MOVING).all() for p in plans)
    box_err = np.concatenate([b[:, 7:10].astype(np.float64) - v for b, v in zip(boxes, truth)])
    smooth_err = np.concatenate([p.u - v for p, v in zip(plans, truth)])
    assert box_err.size == 1440
    rms = lambda e: math.sqrt(float((e * e).mean()))                # noqa: E731
    ratio = rms(smooth_err) / rms(box_err)
    print(f"rms box {rms(box_err):.4f} smoothed {rms(smooth_err):.4f} ratio {ratio:.3f}")
    assert 0.35 < ratio < 0.6
    # and the plan's vectors are the rule's: disp = (float)(u dt), shift = (float)(u dt - (double)v32 dt)
    p, b = plans[5], boxes[5]
    assert p.disp.tobytes() == (p.u * 0.1).astype(f32).tobytes()
    assert p.shift.tobytes() == (p.u * 0.1 - b[:, 7:10].astype(np.float64) * 0.1).astype(f32).tobytes()


def test_half_zero_counts_the_sweep_alone_and_one_sweep_works():
    boxes, tracks, poses, _ = ref.constant_velocity_tracks(np.random.default_rng(72), n_tracks=5, n_sweeps=4)
    sweeps = [ref.prepare(b, t, p, poses[0]) for b, t, p in zip(boxes, tracks, poses)]
    for p, s in zip(ref.plan_scene(sweeps, half=0), sweeps):
        assert (p.m == 1).all() and (p.state == ref.MOVING).all()
        # m = 1: wbar = w / 1, so u is the box's own velocity up to the two rotations' rounding, and the shift is tiny
        assert np.abs(p.u - s.boxes[:, 7:10]).max() < 1e-5 and np.abs(p.shift).max() < 1e-6
    one = ref.plan_scene(sweeps[:1], min_len=1)
    assert len(one) == 1 and (one[0].m == 1).all() and (one[0].state == ref.MOVING).all()
    short = ref.plan_scene(sweeps[:2])                              # two sweeps under min_len 3: nothing is confirmed
    assert all((p.state == ref.NONE).all() and (p.m == 0).all() and not p.shift.any() and not p.u.any() for p in short)


def test_track_length_missed_sweeps_and_static_boxes():
    K = 6
    boxes = [np.zeros((3, 12), f32) for _ in range(K)]
    tracks = [np.zeros((3, 6)) for _ in range(K)]
    for k in range(K):
        boxes[k][:, 7] = (10.0 + k, 0.2, 4.0)                       # track 0 speeds up; track 1 crawls; track 2 is short
        boxes[k][:, 10] = (1, 2, 3)
        tracks[k][:, 0] = (0, 1, 2 if k < 2 else -1)
    tracks[3][0, 0] = -1                                            # track 0 misses sweep 3
    sweeps = [ref.prepare(b, t, np.eye(4), np.eye(4)) for b, t in zip(boxes, tracks)]
    plans = ref.plan_scene(sweeps, half=1)
    assert [int(p.m[0]) for p in plans] == [2, 3, 2, 0, 2, 2]       # the ends are clipped; sweep 3 contributes nothing and has no row
    assert plans[2].u[0, 0] == (11.0 + 12.0) / 2.0 and plans[4].u[0, 0] == (14.0 + 15.0) / 2.0
    assert [int(p.state[0]) for p in plans] == [1, 1, 1, 0, 1, 1]
    assert all(int(p.state[1]) == ref.STATIC for p in plans)        # 0.2 m/s * 0.1 s = 0.02 m < 0.05 m
    assert all(int(p.state[2]) == ref.NONE for p in plans)          # length 2 < min_len 3
    assert all(int(p.state[2]) == ref.MOVING for p in ref.plan_scene(sweeps, half=1, min_len=2)[:2])
    assert int(ref.plan_scene(sweeps, motion_min=0.0)[0].state[1]) == ref.MOVING       # nothing is below zero


def test_points_of_the_restatement():
    b = np.zeros((2, 12), f32)
    b[:, 7] = (5.0, 0.1)
    b[:, 10] = (7, 3)
    t = np.zeros((2, 6))
    t[:, 0] = (0, 1)
    pose0, pose1 = ref.ego_pose(3), ref.ego_pose(4)
    s = ref.prepare(b, t, pose0, pose0)
    pl = ref.plan_scene([s], min_len=1)[0]
    assert pl.state.tolist() == [ref.MOVING, ref.STATIC]
    rng = np.random.default_rng(73)
    pc0 = rng.uniform(-30, 30, (8, 4)).astype(f32)
    flow = rng.normal(0, 1, (8, 3)).astype(f32)
    flow[2, 1] = np.nan
    flow.view(np.uint32)[3, 0] = 0x7FC12345                        # a NaN with a payload
    label = np.array([7, 3, 7, 3, 0, -7, 5, 7])
    E = ref.ego_transform(pose0, pose1)
    T = np.concatenate([E.reshape(3, 4), [[0, 0, 0, 1]]]).astype(f32)
    ego = (ref.acc.rigid_move(pc0[:, :3], T) - pc0[:, :3]).astype(f32)
    for mode in (0, 1):
        out, nm, ns = ref.apply_sweep(pc0, flow, label, E, s, pl, mode)
        assert (nm, ns) == (2, 1)
        assert out[1].tobytes() == ego[1].tobytes()                 # STATIC in both modes: the ego-motion flow
        for i in (2, 3, 4, 5, 6):                                   # a flow that is not finite, label 0, negative, absent: the input bytes
            assert out[i].tobytes() == flow[i].tobytes()
        want = (flow[[0, 7]] + pl.shift[0]).astype(f32) if mode == 0 else (ego[[0, 7]] + pl.disp[0]).astype(f32)
        assert out[[0, 7]].tobytes() == want.tobytes()


# ---- the program's refusals: before any launch or write ---------------------------------------------------------------------------------------
def small_dataset(root, with_tracks=True, with_out=False, stale=False):
    from himo_amd.dataset import NpzDataset
    frames = []
    for k in range(2):
        b = np.zeros((2, 12), f32)
        b[:, 10] = (1, 2)
        f = {"scene_id": "s0", "timestamp": 100 + k, "pc0": np.zeros((5, 3), f32), "pose0": np.eye(4), "pose1": np.eye(4), "res": np.zeros((5, 3), f32),
             "ids": np.array([1, 2, 0, 1, 2], np.int32), "boxes_res": b}
        if with_tracks:
            f["tracks_res"] = np.zeros((3 if stale and k == 1 else 2, 6))
        if with_out and k == 1:
            f["res_track"] = np.zeros((5, 3), f32)
        frames.append(f)
    NpzDataset.write(root, frames)
    return root


def snapshot(root):
    return {p: p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_program_refusals_come_before_any_launch_or_write(tmp_path, monkeypatch):
    from himo_amd import track_flow
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    made = []
    monkeypatch.setattr(track_flow, "TrackFlow", lambda *a, **kw: made.append(1))      # no engine is ever asked for
    good = small_dataset(tmp_path / "good")
    before = snapshot(good)
    with pytest.raises(ValueError, match="--label_key cluster: clusters made by `box_fit --label_key cluster` are not stored"):
        track_flow.main(str(good), "res", "cluster")
    with pytest.raises(KeyError, match="boxes_nope"):
        track_flow.main(str(good), "nope", "ids")
    with pytest.raises(KeyError, match="no_label"):
        track_flow.main(str(good), "res", "no_label")
    for kw, what in ((dict(mode="both"), "mode"), (dict(half=9), "half"), (dict(min_len=0), "min_len"), (dict(motion_min=-1.0), "motion_min"),
                     (dict(sensor_dt=0.0), "sensor_dt"), (dict(batch=0), "batch")):
        with pytest.raises(ValueError, match=what):
            track_flow.main(str(good), "res", "ids", **kw)
    with pytest.raises(ValueError, match="raw"):
        track_flow.main(str(good), "raw", "ids")
    with pytest.raises(ValueError, match="different names"):
        track_flow.main(str(good), "res,res", "ids")
    assert snapshot(good) == before
    no_tracks = small_dataset(tmp_path / "no_tracks", with_tracks=False)
    with pytest.raises(KeyError, match="tracks_res.*himo_amd.track"):
        track_flow.main(str(no_tracks), "res", "ids")
    stale = small_dataset(tmp_path / "stale", stale=True)
    before = snapshot(stale)
    with pytest.raises(ValueError, match="tracks_res.*3 rows for the 2 boxes.*stale tracks"):
        track_flow.main(str(stale), "res", "ids")
    assert snapshot(stale) == before
    done = small_dataset(tmp_path / "done", with_out=True)
    before = snapshot(done)
    with pytest.raises(FileExistsError, match="res_track.*--overwrite"):
        track_flow.main(str(done), "res", "ids")
    assert snapshot(done) == before and not made
    a = track_flow._parser().parse_args(["--data_dir", "D", "--res_names", "a,b", "--label_key", "ray_label"])
    assert (a.mode, a.half, a.min_len, a.motion_min, a.sensor_dt, a.batch, a.json, a.overwrite) == ("shift", 2, 3, 0.05, 0.1, 16, None, False)
