"""Sweep odometry on the CPU: the restatement of the rule (tests/odometry_ref.py) recovers the poses of the synthetic drives, the Cayley
update, the refusals of ``OdomParams``, the arithmetic of the RPE table, the ``pose_key`` switch of the loaders and the ctypes mirrors."""
import ctypes
import math

import numpy as np
import pytest

import odometry_ref as ref

RPE_T_MAX, RPE_R_MAX = 0.02, 0.02          # metres, degrees: a condition on the restatement alone (the issue's bound)


# ---- recovery on the synthetic drives ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloud", ref.CLOUDS)
def test_restatement_recovers_the_poses(cloud):
    frames, gt, poses, info = ref.drive(cloud)
    p = ref.params()
    assert len(info) == len(frames) - 1
    for i in info:
        assert i["accepted"] and i["status"] == ref.CONVERGED and i["iters"] <= p["iters"], i
    errs = ref.relative_errors(poses, gt)
    print(cloud, [(round(t, 5), round(r, 5)) for t, r in errs])
    assert max(t for t, _ in errs) <= RPE_T_MAX and max(r for _, r in errs) <= RPE_R_MAX, errs
    # the k = 1 vote lands within one bin of the true translation
    assert info[0]["init"] == "vote" and all(i["init"] == "model" for i in info[1:])
    true = np.linalg.inv(gt[0]) @ gt[1]
    assert np.all(np.abs(info[0]["T_init"][:2, 3] - true[:2, 3]) <= p["bin"]), (info[0]["T_init"][:3, 3], true[:3, 3])
    assert np.array_equal(info[0]["T_init"][:3, :3], np.eye(3)) and info[0]["T_init"][2, 3] == 0.0


def test_search_by_cells_equals_the_masked_brute_force():
    rng = np.random.default_rng(5)
    mp = rng.uniform(-70, 70, (900, 3)).astype(np.float32)
    mp[:, 2] = rng.uniform(-2, 2, 900)
    mp[100:110] = mp[90:100]                                   # duplicate rows: the lowest row wins
    m = np.concatenate([mp[:300] + rng.normal(0, 0.3, (300, 3)).astype(np.float32), rng.uniform(-80, 80, (200, 3)).astype(np.float32),
                        np.array([[np.nan, 0, 0], [np.inf, 1, 1], [0, 0, 0]], np.float32)])
    a, b = ref.nearest(m, mp), ref.nearest_brute(m, mp)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    assert a[1][500] == -1 and a[1][501] == -1 and np.isinf(a[0][500])
    assert set(a[1][90:100].tolist()) <= set(range(90, 100)) | {-1}
    for empty in (ref.nearest(m, mp[:0]), ref.nearest_brute(m, mp[:0])):
        assert (empty[1] == -1).all() and np.isinf(empty[0]).all()


# ---- the Cayley update ---------------------------------------------------------------------------------------------------------------------
def test_cayley_update():
    rng = np.random.default_rng(0)
    for scale in (1e-6, 1e-2, 0.5, 3.0):
        for _ in range(20):
            D = ref.cayley(rng.normal(0, scale, 3))
            assert np.abs(D @ D.T - np.eye(3)).max() <= 8 * 2.0 ** -52
            assert abs(np.linalg.det(D) - 1.0) <= 16 * 2.0 ** -52
    Z = ref.cayley([0.0, 0.0, 0.0])
    assert Z.tobytes() == np.eye(3).tobytes()                  # the zero motion: the identity bit for bit (no negative zero)
    # a small rotation about z by omega: tan(angle / 2) = omega / 2
    D = ref.cayley([0.0, 0.0, 0.02])
    assert math.isclose(math.atan2(D[1, 0], D[0, 0]), 2 * math.atan(0.01), rel_tol=1e-14)
    # composition: R <- D R, t <- D t + t_xi (the update is applied on the LEFT)
    T = np.concatenate([ref.cayley([0.3, -0.2, 0.5]), [[1.0], [2.0], [3.0]]], axis=1)
    xi = [0.1, -0.2, 0.3, 0.05, 0.4, -0.3]
    N, D = ref.compose(T, xi), ref.cayley(xi[3:])
    assert np.allclose(N[:, :3], D @ T[:, :3], rtol=0, atol=4e-16) and np.allclose(N[:, 3], D @ T[:, 3] + xi[:3], rtol=0, atol=2e-15)
    assert np.abs(N[:, :3] - T[:, :3] @ D).max() > 1e-3
    same = ref.compose(T, [0.0] * 6)
    assert same.tobytes() == T.tobytes()


def test_cholesky_solves_and_refuses():
    rng = np.random.default_rng(1)
    A = rng.normal(size=(40, 6))
    H, x = A.T @ A, rng.normal(size=6)
    sums = np.concatenate([H[np.triu_indices(6)], H @ x, [0.0]])
    assert np.allclose(ref.cholesky_solve(sums), x, rtol=1e-10)
    H[3:, :] = 0
    H[:, 3:] = 0                                                 # rank 3: the fourth pivot is exactly 0
    assert ref.cholesky_solve(np.concatenate([H[np.triu_indices(6)], np.zeros(7)])) is None
    assert ref.cholesky_solve(np.concatenate([np.full(21, np.nan), np.zeros(7)])) is None


# ---- OdomParams ----------------------------------------------------------------------------------------------------------------------------
BAD = [("voxel", 0), ("voxel", -0.5), ("voxel", float("nan")), ("voxel", float("inf")), ("voxel", 0.05), ("voxel", "0.5"), ("voxel", True),
       ("window", 0), ("window", 32), ("window", 2.5), ("window", True), ("max_dist", 0), ("max_dist", 0.1), ("max_dist", float("inf")),
       ("max_dist", 1e-50), ("gm_scale", 0), ("gm_scale", -1), ("gm_scale", float("nan")), ("min_pairs", 0), ("min_pairs", 1.5), ("iters", 0),
       ("iters", 1025), ("eps_t2", 0), ("eps_t2", float("nan")), ("eps_r2", -1e-12), ("eps_r2", float("inf")), ("min_ratio", 0),
       ("min_ratio", 1.5), ("init", "icp"), ("init", None), ("bin", 0), ("half", 0), ("half", 65), ("z_gate", float("nan")),
       ("data_name", "kitti")]


@pytest.mark.parametrize("name,value", BAD)
def test_odom_params_refuse(name, value):
    from himo_amd.odometry import OdomParams
    with pytest.raises(ValueError, match=name):
        OdomParams(**{name: value})


def test_odom_params_defaults_and_grids():
    from himo_amd.odometry import OdomParams
    p = OdomParams()
    d = ref.params()
    for k in ("voxel", "window", "max_dist", "gm_scale", "min_pairs", "iters", "eps_t2", "eps_r2", "min_ratio", "init", "bin", "half", "z_gate"):
        assert getattr(p, k) == d[k], k
    c = p.c_struct()
    g = ref.search_grid()
    assert (c.x0, c.y0, c.max_dist, c.gw, c.gh) == (float(g[0]), float(g[1]), float(g[2]), g[4], g[5]) and c.gw * c.gh <= 1 << 20
    a, kw = p.accum_params(), ref.accum_kw()
    assert (a.x0, a.y0, a.z0, a.voxel, a.nx, a.ny, a.nz) == (kw["x0"], kw["y0"], kw["z0"], kw["voxel"], kw["nx"], kw["ny"], kw["nz"])
    assert a.nx * a.voxel >= 128 and a.nz * a.voxel >= 16 and a.x0 <= -64 and a.z0 <= -8          # +-64 m in x and y, +-8 m in z
    OdomParams(voxel=0.0625, max_dist=0.125, window=31, iters=1024, half=64, min_ratio=1.0, init="vote")
    with pytest.raises(Exception):
        p.voxel = 1.0                                           # frozen


def test_ctypes_mirrors_have_the_c_struct_sizes():
    from himo_amd import _lib
    from himo_amd.odometry import _CParams, _CState
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_odom_params") == ctypes.sizeof(_CParams) == 48
    assert lib.himo_abi_sizeof(b"himo_odom_state") == ctypes.sizeof(_CState) == 392
    for name in ("himo_odom_workspace_bytes", "himo_odom_init", "himo_odom_map", "himo_odom_step", "himo_odom_register"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


# ---- the RPE table -------------------------------------------------------------------------------------------------------------------------
def _yaw(deg, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    T[:2, :2], T[:3, 3] = [[c, -s], [s, c]], t
    return T


def _chain(steps, first=None):
    out = [np.eye(4) if first is None else first]
    for s in steps:
        out.append(out[-1] @ s)
    return np.stack(out)


def test_rpe_table_arithmetic():
    from himo_amd.odometry import fold_sums, new_sums, numbers_of, rpe_table
    steps = [_yaw(1.0, (1.0, 0.1, 0.0)), _yaw(-0.5, (0.9, 0.0, 0.02)), _yaw(0.2, (1.1, -0.1, 0.0))]
    gt = _chain(steps, first=_yaw(30.0, (5.0, -3.0, 1.0)))
    same = rpe_table(gt, gt)
    assert same["pairs"] == 3 and same["t_max"] < 1e-12 and same["r_max"] < 1e-6 and same["drift"] < 1e-12
    assert math.isclose(same["path"], sum(np.linalg.norm(s[:3, 3]) for s in steps), rel_tol=1e-12)
    # the same relative motion from another first pose: still zero (the error is relative)
    assert rpe_table(_chain(steps), gt)["t_max"] < 1e-12
    # a known yaw offset of 0.25 degrees a step, and a known translation offset in the second step
    off = [s @ _yaw(0.25) for s in steps]
    off[1] = off[1] @ _yaw(0.0, (0.0, 0.03, 0.04))
    t = rpe_table(_chain(off), _chain(steps))
    assert math.isclose(t["r_sum"], 0.75, rel_tol=1e-7) and math.isclose(t["r_max"], 0.25, rel_tol=1e-7)
    assert math.isclose(t["t_max"], 0.05, rel_tol=1e-9) and math.isclose(t["t_sum"], 0.05, rel_tol=1e-9)
    assert t["drift"] > 0.0
    with pytest.raises(ValueError):
        rpe_table(gt, gt[:-1])
    both = fold_sums(dict(new_sums(), **t, sweeps=3, accepted=3, iters=12, share=2.4, scenes=1),
                     dict(new_sums(), **same, sweeps=3, accepted=2, fallen=1, iters=30, share=1.2, scenes=1))
    n = numbers_of(both, True)
    assert n["sweeps"] == 6 and n["accepted"] == 5 and n["fallen_back"] == 1 and n["mean_iters"] == 7.0 and math.isclose(n["mean_inlier_share"], 0.6)
    assert n["rpe_pairs"] == 6 and math.isclose(n["rpe_r_max_deg"], 0.25, rel_tol=1e-7) and math.isclose(n["rpe_t_mean_m"], 0.05 / 6, rel_tol=1e-9)
    assert math.isclose(n["drift_share"], both["drift"] / both["path"])
    assert numbers_of(new_sums(), True)["rpe_t_mean_m"] is None


# ---- pose_key ------------------------------------------------------------------------------------------------------------------------------
def _scenes():
    from himo_amd.synthetic import make_scene
    return [make_scene(40 + s, 3, n_points=60, n_instances=1, scene_id=f"sc{s}") for s in range(2)]


def _odom_pose(f):
    """a second pose of a sweep, different from the stored one"""
    return np.asarray(f["pose0"]) @ _yaw(0.5, (0.25, 0.0, 0.0))


def _h5_with_second_key(root, scenes, skip=()):
    from himo_amd import h5lite, save, stored
    from himo_amd.synthetic import write_h5_scenes
    write_h5_scenes(root, scenes)
    mod, _ = save.h5_writer()
    for frames in scenes:
        path = root / f"{frames[0]['scene_id']}.h5"
        keys = {str(f["timestamp"]): {"pose_odom": _odom_pose(f)} for f in frames if f["timestamp"] not in skip}
        if mod is not None:
            with mod.File(path, "a") as h:
                for ts, arrays in keys.items():
                    stored.put_keys(h, ts, arrays)
        else:                                                   # no HDF5 library to modify a file with: the same tree written whole
            with h5lite.File(path) as h:
                tree = {ts: {k: np.asarray(h[ts][k][:]) for k in h[ts]} for ts in h}
            for ts, arrays in keys.items():
                tree[ts].update(arrays)
            h5lite.write_file(path, tree)


def test_pose_key_on_scene_files(tmp_path, monkeypatch):
    from himo_amd.dataset import HDF5Dataset, open_dataset
    monkeypatch.delenv("HIMO_POSE_KEY", raising=False)
    scenes = _scenes()
    _h5_with_second_key(tmp_path, scenes)
    flat = [f for frames in scenes for f in frames[:-1]]
    with pytest.warns(UserWarning):
        plain = open_dataset(tmp_path)
    assert len(plain) == len(flat) and plain.pose_key == "pose"
    for i, f in enumerate(flat):                                # neither set: today's frames, byte for byte
        d = plain[i]
        assert d["pose0"].tobytes() == np.asarray(f["pose0"]).tobytes() and d["pose1"].tobytes() == np.asarray(f["pose1"]).tobytes()
        assert d["pc0"].tobytes() == f["pc0"].tobytes() and "pose_odom" not in d
    with pytest.warns(UserWarning):
        named = open_dataset(tmp_path, pose_key="pose_odom")
    monkeypatch.setenv("HIMO_POSE_KEY", "pose_odom")
    with pytest.warns(UserWarning):
        by_env = open_dataset(tmp_path)
        explicit = HDF5Dataset(tmp_path, pose_key="pose")       # a name given wins over the environment
    assert by_env.pose_key == "pose_odom" and explicit.pose_key == "pose"
    for ds in (named, by_env):
        for frames in scenes:
            for k, f in enumerate(frames[:-1]):
                d = ds[[s for s, _ in ds.index].index(f["scene_id"]) + k]
                assert d["timestamp"] == f["timestamp"]
                assert np.array_equal(d["pose0"], _odom_pose(f)) and np.array_equal(d["pose1"], _odom_pose(frames[k + 1]))
                assert d["pc0"].tobytes() == f["pc0"].tobytes()
    assert explicit[0]["pose0"].tobytes() == np.asarray(flat[0]["pose0"]).tobytes()
    # the last sweep of a scene: kept without need_next, and then it has no successor to ask for
    alone = HDF5Dataset(tmp_path, need_next=False, pose_key="pose_odom", fields=("pc0", "pose0"))
    assert len(alone) == sum(len(frames) for frames in scenes)
    last = alone[len(scenes[0]) - 1]
    assert last["timestamp"] == scenes[0][-1]["timestamp"] and np.array_equal(last["pose0"], _odom_pose(scenes[0][-1])) and "pose1" not in last
    with pytest.raises(KeyError):
        alone.read(len(scenes[0]) - 1, fields=("pose1",))
    monkeypatch.setenv("HIMO_POSE_KEY", "")
    with pytest.warns(UserWarning):
        assert open_dataset(tmp_path).pose_key == "pose"
    with pytest.raises(ValueError, match="pose_key"):
        HDF5Dataset(tmp_path, pose_key="")


def test_pose_key_missing_is_a_worded_keyerror(tmp_path, monkeypatch):
    from himo_amd.dataset import open_dataset
    monkeypatch.delenv("HIMO_POSE_KEY", raising=False)
    scenes = _scenes()
    _h5_with_second_key(tmp_path, scenes, skip=(scenes[0][1]["timestamp"],))
    with pytest.warns(UserWarning):
        ds = open_dataset(tmp_path, pose_key="pose_odom")
    with pytest.raises(KeyError, match=r"pose_odom.*python -m himo_amd\.odometry"):
        ds[0]                                                   # its successor lacks the key
    with pytest.raises(KeyError, match=r"pose_odom.*python -m himo_amd\.odometry"):
        ds[1]                                                   # the sweep itself lacks it
    assert np.array_equal(ds[2]["pose0"], _odom_pose(scenes[1][0]))
    with pytest.warns(UserWarning):
        other = open_dataset(tmp_path, pose_key="pose_icp")
    with pytest.raises(KeyError, match="pose_icp"):
        other[2]


def test_pose_key_on_the_npz_container(tmp_path, monkeypatch):
    from himo_amd import stored
    from himo_amd.dataset import NpzDataset, open_dataset
    monkeypatch.delenv("HIMO_POSE_KEY", raising=False)
    frames = [f for sc in _scenes() for f in sc]
    NpzDataset.write(tmp_path, frames)
    for f in frames[:-1]:
        stored.put_npz(tmp_path, f["scene_id"], f["timestamp"], {"pose_odom": _odom_pose(f), "pose_odom_next": np.asarray(f["pose1"]) @ _yaw(0.5, (0.25, 0, 0))})
    stored.put_npz(tmp_path, frames[-1]["scene_id"], frames[-1]["timestamp"], {"pose_odom": _odom_pose(frames[-1])})    # no successor pose
    plain = open_dataset(tmp_path)
    assert isinstance(plain, NpzDataset) and plain.pose_key == "pose"
    for i, f in enumerate(frames):
        assert plain[i]["pose0"].tobytes() == np.asarray(f["pose0"]).tobytes() and plain[i]["pose1"].tobytes() == np.asarray(f["pose1"]).tobytes()
    monkeypatch.setenv("HIMO_POSE_KEY", "pose_odom")
    for ds in (open_dataset(tmp_path), NpzDataset(tmp_path, pose_key="pose_odom")):
        for i, f in enumerate(frames[:-1]):
            d = ds[i]
            assert np.array_equal(d["pose0"], _odom_pose(f)) and np.array_equal(d["pose1"], np.asarray(f["pose1"]) @ _yaw(0.5, (0.25, 0, 0)))
            assert d["pc0"].tobytes() == f["pc0"].tobytes()
        with pytest.raises(KeyError, match=r"pose_odom_next.*python -m himo_amd\.odometry"):
            ds[len(frames) - 1]
    assert NpzDataset(tmp_path, pose_key="pose")[0]["pose0"].tobytes() == np.asarray(frames[0]["pose0"]).tobytes()


def test_program_refuses_before_any_gpu_work(tmp_path):
    from himo_amd import odometry
    with pytest.raises(ValueError, match="out_key"):
        odometry.main(str(tmp_path), out_key="pose")
    with pytest.raises(ValueError, match="out_key"):
        odometry.main(str(tmp_path), out_key="pose_odom_next")
    with pytest.raises(ValueError, match="window"):
        odometry.main(str(tmp_path), window=0)
    with pytest.raises(ValueError, match="init"):
        odometry.main(str(tmp_path), init="imu")
    a = odometry._parser().parse_args(["--data_dir", "D"])
    assert (a.out_key, a.window, a.voxel, a.init, a.gt_key, a.skip_label, a.overwrite) == ("pose_odom", 10, 0.5, "model", None, None, False)
