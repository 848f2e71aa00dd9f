"""Ego de-skew without a GPU: the restatement (tests/deskew_ref.py) checked against scipy's matrix exponential and logarithm and against
its own algebra, the product's pose logarithm and twist modes, the round trip on the synthetic drives, and every refusal of
``DeskewParams`` and of the program that needs no library."""
import math

import numpy as np
import pytest

import deskew_ref as ref

f32, f64 = np.float32, np.float64

TWISTS = {
    "zero_rotation": [9.0, -0.4, 0.1, 0.0, 0.0, 0.0],
    "theta_1e-9": [1.0, 0.2, -0.1, 0.0, 6e-10, 8e-10],
    "theta_7e-3": [1.0, 0.1, 0.02, 0.0, 0.0, 7e-3],
    "theta_0.5": [0.8, -0.3, 0.2, 0.0, 0.0, 0.5],
    "axis_off_z": [1.1, 0.3, -0.2, 0.12, -0.2, 0.15],
    "above_switch": [1.0, -1.0, 0.5, 0.0, 1.2e-8, 0.0],
}


def _rows(n=400, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-36.9, 36.9, (n, 3))                        # |p| <= 64 m
    p[0], p[1] = (64.0, 0.0, 0.0), (0.0, -64.0, 0.0)
    return p


@pytest.mark.parametrize("name", sorted(TWISTS))
def test_closed_form_equals_the_matrix_exponential(name):
    from scipy.linalg import expm
    xi = np.array(TWISTS[name], f64)
    p = _rows()
    rng = np.random.default_rng(1)
    s = rng.uniform(-1.0, 1.0, len(p))
    worst = 0.0
    for inverse in (False, True):
        d = ref.displacement(p, s, xi[:3], xi[3:], inverse)
        for k in range(0, len(p), 7):
            E = expm((s[k] if inverse else -s[k]) * ref.hat(xi))
            want = E[:3, :3] @ p[k] + E[:3, 3]
            worst = max(worst, float(np.abs(p[k] + d[k] - want).max()))
    print(f"{name}: worst |closed form - expm| = {worst:.3g} m")
    theta = float(np.linalg.norm(xi[3:]))
    if 0 < theta < 1e-8:
        # the rule's FIRST-ORDER form, not the closed form: what it leaves out is the second order of the series,
        # s^2 / 2 (w x v + w x (w x p)), at most theta / 2 (|v| + theta |p|) for |s| <= 1 (and 1e-12 for the rest)
        assert worst <= 0.5 * theta * (float(np.linalg.norm(xi[:3])) + theta * 64.0) + 1e-12
    else:
        assert worst <= 1e-12


@pytest.mark.parametrize("theta", (0.0, 0.9e-8, 1.1e-8, 1e-5, 7e-3, 0.5, 1.5))
def test_the_products_log_equals_logm(theta):
    from scipy.linalg import expm, logm
    from himo_amd.deskew import se3_log
    axis = np.array([0.2, -0.3, 0.93])
    axis /= np.linalg.norm(axis)
    xi = np.concatenate([[0.9, -0.2, 0.05], theta * axis])
    T = expm(ref.hat(xi))
    got = se3_log(T)
    L = np.real(logm(T)) if theta > 0 else ref.hat(np.concatenate([T[:3, 3], np.zeros(3)]))
    want = np.array([L[0, 3], L[1, 3], L[2, 3], L[2, 1], L[0, 2], L[1, 0]])
    print(f"theta {theta:g}: |log - logm| = {np.abs(got - want).max():.3g}, |log - xi| = {np.abs(got - xi).max():.3g}")
    assert np.abs(got - xi).max() <= 1e-12                      # the twist the pose was made from
    assert np.abs(got - want).max() <= 1e-9                     # scipy's own logarithm (its error near the identity is the larger)
    assert np.abs(ref.log_se3(T) - got).max() <= 1e-15          # the restatement's own closed form


def test_log_refusals():
    from scipy.linalg import expm
    from himo_amd.deskew import se3_log, twists_from_poses
    with pytest.raises(ValueError, match="pi / 2"):
        se3_log(expm(ref.hat([0, 0, 0, 0, 0, 1.6])))
    bad = np.eye(4)
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        se3_log(bad)
    with pytest.raises(ValueError, match="finite"):
        twists_from_poses(np.stack([np.eye(4), bad]))
    with pytest.raises(ValueError, match="pi / 2"):
        twists_from_poses(np.stack([np.eye(4), expm(ref.hat([1, 0, 0, 0, 0, 2.0]))]))
    with pytest.raises(ValueError, match="span"):
        twists_from_poses(np.stack([np.eye(4), np.eye(4)]), "backward", [200, 100])
    with pytest.raises(ValueError, match="one of"):
        twists_from_poses(np.stack([np.eye(4), np.eye(4)]), "sideways")
    with pytest.raises(ValueError, match="4, 4"):
        twists_from_poses(np.zeros((3, 3, 4)))


def test_a_whole_span_is_the_inverse_relative_pose():
    """s = 1: the row is moved by inv(rel), the whole motion of the sweep"""
    from scipy.linalg import expm
    xi = np.array(TWISTS["axis_off_z"], f64)
    rel = expm(ref.hat(xi))
    p = _rows(50).astype(f32)
    dt = np.zeros(len(p), f32)
    dt[-1] = f32(0.1)                                           # t_ref = 0.1 (max): every other row has s = 1 with the span of its own bits
    out = ref.deskew(p, dt, np.concatenate([xi, [float(f32(0.1)), 0]]))[0]
    inv = np.linalg.inv(rel)
    want = p[:-1].astype(f64) @ inv[:3, :3].T + inv[:3, 3]
    assert np.abs(out[:-1] - want).max() <= 4e-6                # float32 rounding at 64 m
    assert out[-1].tobytes() == p[-1].tobytes()


def test_rows_that_keep_their_bytes():
    xi = np.concatenate([TWISTS["theta_7e-3"], [0.1, 0]])
    p = _rows(12).astype(f32)
    p = np.concatenate([p, np.linspace(0, 1, 12, dtype=f32)[:, None]], axis=1)
    dt = np.linspace(0, 0.09, 12).astype(f32)
    dt[3] = dt.max()                                            # s == 0 twice
    p[3, 1] = f32(-0.0)
    p[4, 0], p[5, 2], p[6, 1] = np.nan, np.inf, -np.inf
    dt[7], dt[8] = np.nan, np.inf
    out, counts, disp, tr = ref.deskew(p, dt, xi)
    keep = [3, 4, 5, 6, 7, 8, 11]
    for k in keep:
        assert out[k].tobytes() == p[k].tobytes(), k
    assert tr == f32(0.09) and counts.tolist() == [12 - len(keep), len(keep)]
    moved = [k for k in range(12) if k not in keep]
    assert all(out[k, :3].tobytes() != p[k, :3].tobytes() for k in moved) and np.array_equal(out[:, 3], p[:, 3])
    assert disp > 0
    # a zero twist, all lidar_dt equal, and no finite lidar_dt: every byte unchanged
    for tw, d in ((np.array([0, 0, 0, 0, 0, 0, 0.1, 0.0]), dt), (xi, np.full(12, 0.05, f32)), (xi, np.full(12, np.nan, f32))):
        out, counts, disp, tr = ref.deskew(p, d, tw)
        assert out.tobytes() == p.tobytes() and counts.tolist() == [0, 12] and disp == 0
    assert ref.t_ref(np.full(3, np.nan, f32)) == 0 and ref.t_ref(dt, "min") == 0 and ref.t_ref(dt, "zero") == 0
    assert ref.t_ref(np.array([-0.02, -0.05, np.nan], f32), "max") == f32(-0.02)


@pytest.mark.parametrize("dt_mode", ("random", "azimuth"))
@pytest.mark.parametrize("cloud", ("uniform", "rings"))
def test_round_trip_of_the_drives_with_true_poses(cloud, dt_mode):
    """8e-6 m: two float32 roundings (the skew's and the de-skew's), each at most half an ulp of 64 m = 3.8e-6 m a coordinate, that is
    2 * sqrt(3) * 1.9e-6 = 6.6e-6 m a row in the worst case, plus the float64 work (1e-14)"""
    from himo_amd.deskew import twists_from_poses
    frames, skewed = ref.drive(cloud, dt_mode)
    reach = max(float(np.abs(f["pc0"][:, :3]).max()) for f in skewed)
    print(f"{cloud} {dt_mode}: greatest |coordinate| {reach:.2f} m")          # (a few rows of `rings` lie past 64 m in x: still within the bound)
    poses = np.stack([f["pose0"] for f in frames])
    tw = twists_from_poses(poses, "backward", 0.1)
    assert np.abs(tw - ref.twists_from_poses(poses, "backward", 0.1)).max() <= 1e-15
    skew_mean, skew_max, worst = [], 0.0, 0.0
    for f, sk, t in zip(frames, skewed, tw):
        e = ref.row_errors(sk["pc0"], f["pc0"])
        skew_mean.append(e.mean())
        skew_max = max(skew_max, e.max())
        out, counts, disp, _ = ref.deskew(sk["pc0"], sk["lidar_dt"], t)
        assert counts.sum() == len(out) and abs(float(disp) - e.max()) <= 1e-5
        assert np.array_equal(out[:, 3], f["pc0"][:, 3])
        worst = max(worst, float(ref.row_errors(out, f["pc0"]).max()))
    print(f"{cloud} {dt_mode}: skew mean {np.mean(skew_mean):.3f} m max {skew_max:.3f} m; after de-skew worst row {worst:.3g} m")
    assert np.mean(skew_mean) > 0.1 and worst <= 8e-6


def test_twist_modes_at_the_ends_of_a_scene():
    from scipy.linalg import expm
    from himo_amd.deskew import twists_from_poses
    xis = [np.array([1.0, 0.0, 0.0, 0, 0, 0.01]), np.array([1.2, 0.1, 0.0, 0, 0, 0.02]), np.array([0.9, -0.1, 0.0, 0, 0.01, -0.01])]
    poses = [np.eye(4)]
    for x in xis:
        poses.append(poses[-1] @ expm(ref.hat(x)))
    poses = np.stack(poses)
    stamps = [1000, 1000 + 100_000_000, 1000 + 210_000_000, 1000 + 300_000_000]
    for fn in (twists_from_poses, ref.twists_from_poses):
        b, f, c = fn(poses, "backward", 0.1), fn(poses, "forward", 0.1), fn(poses, "central", 0.1)
        for got, want in ((b, [0, 0, 1, 2]), (f, [0, 1, 2, 2])):
            assert np.abs(got[:, :6] - np.stack([xis[j] for j in want])).max() <= 1e-12
        assert np.abs(c[:, :6] - np.stack([xis[0], (xis[0] + xis[1]) / 2, (xis[1] + xis[2]) / 2, xis[2]])).max() <= 1e-12
        assert (b[:, 6] == 0.1).all() and (c[:, 6] == 0.1).all() and (b[:, 7] == 0).all()
        s = fn(poses, "backward", stamps)
        assert np.allclose(s[:, 6], [0.1, 0.1, 0.11, 0.09], rtol=0, atol=1e-15)
        s = fn(poses, "central", stamps)
        assert np.allclose(s[:, 6], [0.1, 0.105, 0.1, 0.09], rtol=0, atol=1e-15)
        one = fn(poses[:1], "central", 0.1)
        assert one.shape == (1, 8) and (one[0, :6] == 0).all() and one[0, 6] == 0.1
        one = fn(poses[:1], "backward", stamps[:1], 0.05)
        assert (one[0, :6] == 0).all() and one[0, 6] == 0.05
        two = fn(poses[:2], "forward", 0.1)
        assert np.abs(two[:, :6] - np.stack([xis[0], xis[0]])).max() <= 1e-12
    assert twists_from_poses(np.zeros((0, 4, 4))).shape == (0, 8)


def test_params_refuse_what_the_rule_does_not_admit():
    from himo_amd.deskew import DeskewParams
    d = DeskewParams()
    assert (d.ref, d.twist, d.span, d.sensor_dt, d.ref_mode) == ("max", "backward", "fixed", 0.1, 0)
    assert DeskewParams(ref="zero").ref_mode == 2 and DeskewParams(ref="min").ref_mode == 1
    for kw in (dict(ref="mean"), dict(ref=None), dict(twist="sideways"), dict(span="clock"), dict(sensor_dt=0.0), dict(sensor_dt=-0.1),
               dict(sensor_dt=float("nan")), dict(sensor_dt=float("inf")), dict(sensor_dt="0.1"), dict(sensor_dt=True), dict(batch=0),
               dict(batch=-2), dict(batch=1.5), dict(batch=True), dict(batch=5000)):
        with pytest.raises(ValueError, match="DeskewParams"):
            DeskewParams(**kw)
    with pytest.raises(Exception):
        d.ref = "min"                                           # frozen


def test_program_refusals_that_need_no_library(tmp_path):
    from himo_amd import deskew
    from himo_amd.dataset import NpzDataset
    from himo_amd.synthetic import make_scene, write_h5_scenes
    frames = make_scene(5, 2, n_points=200, n_instances=1, scene_id="tiny")
    src, npz, out = tmp_path / "src", tmp_path / "npz", tmp_path / "out"
    src.mkdir()
    write_h5_scenes(src, [frames])
    NpzDataset.write(npz, frames)
    with pytest.raises(ValueError, match="equals --data_dir"):
        deskew.main(str(src), str(src))
    with pytest.raises(ValueError, match="equals --data_dir"):
        deskew.main(str(src), str(src / "." / ""))
    with pytest.raises(ValueError, match="npz container"):
        deskew.main(str(npz), str(out))
    with pytest.raises(FileNotFoundError, match="no <scene>.h5"):
        deskew.main(str(tmp_path / "out"), str(tmp_path / "out2"))
    for kw in (dict(ref="mean"), dict(twist="x"), dict(span="y"), dict(sensor_dt=0.0), dict(batch=0)):
        with pytest.raises(ValueError, match="DeskewParams"):
            deskew.main(str(src), str(out), **kw)
    out.mkdir()
    (out / "tiny.h5").write_bytes(b"")
    with pytest.raises(FileExistsError, match="--overwrite"):
        deskew.main(str(src), str(out))
    (out / "tiny.h5").unlink()
    with pytest.raises(KeyError, match="pose_odom"):
        deskew.main(str(src), str(out), pose_key="pose_odom")
    with pytest.raises(KeyError, match="--inverse re-skews"):
        deskew.main(str(src), str(out), inverse=True)
    assert not list(out.iterdir())                              # nothing was written
    with pytest.raises(SystemExit):
        deskew._parser().parse_args(["--data_dir", "a", "--out_dir", "b", "--ref", "mean"])
    a = deskew._parser().parse_args(["--data_dir", "a", "--out_dir", "b"])
    assert (a.pose_key, a.twist, a.ref, a.span, a.sensor_dt, a.inverse, a.overwrite, a.json) == ("pose", "backward", "max", "fixed", 0.1, False,
                                                                                               False, None)
