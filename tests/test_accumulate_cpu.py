"""The sweep accumulator without a GPU: the numpy restatement of its written rule (tests/accumulate_ref.py; parity with the reference
is unpinned) against hand-worked cases, its float32 fused multiply-add against the C library's, the refusals of ``AccumParams``, the
argument parser, the ctypes signatures against the header, the window rule at a scene's start, and what the feature says about
itself."""
import ctypes
import ctypes.util
import re

import numpy as np
import pytest

import accumulate_ref as ref
from conftest import REPO

UNIT = dict(x0=0.0, y0=0.0, z0=0.0, voxel=1.0, nx=8, ny=8, nz=4, ego_min=(2.0, 2.0, 1.0), ego_max=(3.0, 3.0, 2.0))      # 8 x 8 x 4 voxels of 1 m
EYE = np.eye(4, dtype=np.float32)
f32 = np.float32


def key(ix, iy, iz):
    return (iz << 24) | (iy << 12) | ix


def one(rows, lag=0, T=EYE, skip=None, **kw):
    return ref.accumulate([(np.asarray(rows, f32).reshape(-1, 3), T, lag, skip)], **{**UNIT, **kw})


def test_the_hand_worked_point():
    keys, xyz, lag, count = one([(0.5, 0.5, 0.5)])
    u, usable = ref.quantise(np.array([[0.5, 0.5, 0.5]], f32), **UNIT)
    assert usable.all() and u.tolist() == [[128, 128, 128]]
    assert keys.tolist() == [0] and count.tolist() == [1] and lag.tolist() == [0]
    assert xyz.dtype == np.float32 and xyz.tolist() == [[0.501953125] * 3]          # (0 + 0.5 + 128) / 256


def test_two_points_in_one_voxel():
    keys, xyz, lag, count = one([(1.25, 2.0, 3.5), (1.75, 2.5, 3.5)])
    assert keys.tolist() == [key(1, 2, 3)] and count.tolist() == [2]
    # offsets 64 and 192 -> mean 128; 0 and 128 -> 64; 128 and 128 -> 128
    assert xyz.tolist() == [[1 + 128.5 / 256, 2 + 64.5 / 256, 3 + 128.5 / 256]]


def test_faces_of_voxels_and_of_the_grid():
    keys, xyz, _, count = one([(3.0, 0.25, 0.25), (8.0, 0.25, 0.25), (0.25, 0.25, 4.0), (np.nextafter(f32(8.0), f32(0)), 0.25, 0.25),
                               (-0.001, 0.25, 0.25)])
    # a point on a voxel's face belongs to the voxel above it; the grid's upper face and anything below 0 are outside
    assert keys.tolist() == [key(3, 0, 0), key(7, 0, 0)] and count.tolist() == [1, 1]
    assert xyz[0, 0] == f32(3 + 0.5 / 256) and xyz[1, 0] == f32(7 + 255.5 / 256)


def test_the_ego_box_is_open():
    inside, on_it = (2.5, 2.5, 1.5), (2.0, 2.5, 1.5)
    part = ref.takes_part(np.array([inside, on_it, (3.0, 3.0, 2.0), (2.5, 2.5, 2.5)], f32), **UNIT)
    assert part.tolist() == [False, True, True, True]
    keys, _, _, _ = one([inside, on_it])
    assert keys.tolist() == [key(2, 2, 1)]
    # the box is tested on the row as given, not on the moved point
    T = EYE.copy()
    T[0, 3] = 3.0
    keys, _, _, _ = one([inside, (-0.5, 2.5, 1.5)], T=T)                            # the second row lands where the first one was
    assert keys.tolist() == [key(2, 2, 1)]
    assert one([inside], skip=None)[0].size == 0


def test_the_quantisation_limit_and_non_finite_rows():
    big = dict(UNIT, voxel=256.0)                                                     # scale 1: f = c
    assert ref.scale_of(256.0) == 1.0
    edge = f32(4194304.0)
    u, usable = ref.quantise(np.array([[edge, 1, 1], [np.nextafter(edge, f32(0)), 1, 1], [-edge, 1, 1], [1, np.nan, 1], [1, 1, np.inf]], f32), **big)
    assert usable.tolist() == [False, True, False, False, False]
    rows = np.array([(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (1.5, 1.5, 1.5)], f32)
    assert ref.takes_part(rows, **UNIT).tolist() == [False, False, False, True]
    keys, _, _, count = one(rows)
    assert keys.tolist() == [key(1, 1, 1)] and count.tolist() == [1]
    # a finite row that the transform sends past the limit
    T = EYE.copy()
    T[1, 3] = 3.0e38
    assert one(rows, T=T)[0].size == 0
    assert one(np.zeros((0, 3), f32))[0].size == 0


def test_the_least_lag_of_a_voxel():
    p = np.array([[4.5, 4.5, 0.5]], f32)
    keys, _, lag, count = ref.accumulate([(p, EYE, 3), (p, EYE, 1), (p + f32(1.0), EYE, 7)], **UNIT)
    assert keys.tolist() == [key(4, 4, 0), key(5, 5, 1)] and lag.tolist() == [1, 7] and count.tolist() == [2, 1]
    keys, _, lag, _ = ref.accumulate([(p, EYE, 3, np.array([0])), (p, EYE, 1, np.array([1]))], **UNIT)       # the lag-1 row is skipped
    assert lag.tolist() == [3]


def test_keys_order_and_the_last_voxel_of_the_largest_grid():
    wide = dict(UNIT, nx=4096, ny=4096, nz=256)
    keys, xyz, _, _ = one([(4095.5, 4095.5, 255.5), (0.5, 0.5, 128.5), (0.5, 0.5, 0.5)], **wide)
    assert keys.tolist() == [0, 128 << 24, 0xFFFFFFFF]                               # the last key is the all-ones word
    assert xyz[2].tolist() == [4095.501953125, 4095.501953125, 255.501953125]


def test_the_float32_fma_of_the_restatement_is_the_c_librarys():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(f32) * f32(50)
    b = rng.standard_normal(4000).astype(f32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * rng.choice([1.0, 1.0 + 2.0 ** -20, 0.5, -3.0], 4000)).astype(f32)      # cancellations
    # ties of the float32 rounding that only the product's low bits break: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24
    a[:4], b[:4], c[:4] = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12), [0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** 30]
    a[4], b[4], c[4] = f32(1 + 2.0 ** -23), f32(1 + 2.0 ** -23), f32(2.0 ** 60)           # the float64 sum itself is inexact
    a[5], b[5], c[5] = f32(3 + 2.0 ** -20), f32(5 - 2.0 ** -21), f32(-2.0 ** 40 - 2.0 ** 17)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], f32)
    got = ref.fma32(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got != (a * b + c).astype(f32)).any()                                    # ... and it is not the twice-rounded expression
    # the move: a pure translation and the identity are exact
    T = EYE.copy()
    T[:3, 3] = (1.0, -2.0, 0.5)
    p = rng.uniform(-8, 8, (50, 3)).astype(f32)
    assert np.array_equal(ref.rigid_move(p, EYE), p) and np.array_equal(ref.rigid_move(p, T), p + T[:3, 3])


def test_the_window_rule_at_a_scenes_start():
    from himo_amd import accumulate as acc
    for t, window, want in ((0, 10, [0]), (3, 10, [0, 1, 2, 3]), (12, 10, list(range(2, 13))), (5, 0, [5]), (40, 31, list(range(9, 41)))):
        assert acc.sources(t, 50, window) == ref.sources(t, 50, window) == want
    with pytest.raises(ValueError):
        acc.sources(3, 10, 32)
    with pytest.raises(ValueError):
        acc.sources(3, 10, -1)
    with pytest.raises(IndexError):
        acc.sources(10, 10, 2)
    assert [acc.capacity_for(n) for n in (0, 8, 9, 1000, 1_320_000, 1 << 30)] == [16, 16, 32, 2048, 1 << 22, 1 << 26]
    poses = [np.eye(4), np.eye(4)]
    poses[1][0, 3] = 2.0
    assert ref.relative_pose(poses[1], poses[0])[0, 3] == -2.0 and ref.relative_pose(poses[1], poses[0]).dtype == np.float32


def test_params_mirror_and_refusals():
    from himo_amd.accumulate import AccumParams
    from himo_amd.compdis import EGO_BOX
    p = AccumParams().check()
    assert ctypes.sizeof(AccumParams) == 56
    assert (p.nx, p.ny, p.nz) == (1024, 1024, 80) and p.voxel == f32(0.1) and p.scale == ref.scale_of(0.1) == f32(256.0 / float(f32(0.1)))
    assert list(p.ego_min) == [f32(v) for v in EGO_BOX["av2"][0]] and list(p.ego_max) == [f32(v) for v in EGO_BOX["av2"][1]]
    s = AccumParams(data_name="scania")
    assert list(s.ego_min) == [f32(v) for v in EGO_BOX["scania"][0]] and list(s.ego_max) == [f32(v) for v in EGO_BOX["scania"][1]]
    assert {k: (tuple(v) if isinstance(v, list) else v) for k, v in ref.DEFAULTS.items()} == \
           dict(x0=-51.2, y0=-51.2, z0=-3.0, voxel=0.1, nx=1024, ny=1024, nz=80, ego_min=tuple(EGO_BOX["av2"][0]), ego_max=tuple(EGO_BOX["av2"][1]))
    AccumParams(nx=4096, ny=4096, nz=256).check()
    AccumParams(nx=1, ny=1, nz=1, voxel=1e-3).check()
    bad = [dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(voxel=1e-40), dict(x0=float("inf")),
           dict(z0=float("nan")), dict(nx=0), dict(nx=4097), dict(ny=0), dict(ny=4097), dict(nz=0), dict(nz=257),
           dict(ego_min=(float("nan"), 0, 0)), dict(ego_max=(0, float("inf"), 0))]
    for kw in bad:
        with pytest.raises(ValueError):
            AccumParams(**kw).check()
    q = AccumParams()
    q.scale = 2559.0                                                                  # not (float)(256.0 / voxel)
    with pytest.raises(ValueError):
        q.check()


def test_the_argument_parser():
    from himo_amd.accumulate import _parser
    a = _parser().parse_args(["--data_dir", "D", "--out_dir", "O"])
    assert (a.data_dir, a.out_dir, a.res_name, a.window, a.voxel, a.drop_ground, a.drop_label, a.data_name, a.overwrite) == \
           ("D", "O", "seflowpp_best", 10, 0.1, False, None, "av2", False)
    a = _parser().parse_args("--data_dir D --out_dir O --res_name raw --window 5 --voxel 0.2 --drop_ground --drop_label ray_label "
                             "--data_name scania --overwrite".split())
    assert (a.res_name, a.window, a.voxel, a.drop_ground, a.drop_label, a.data_name, a.overwrite) == ("raw", 5, 0.2, True, "ray_label", "scania", True)
    for argv in (["--out_dir", "O"], ["--data_dir", "D"], ["--data_dir", "D", "--out_dir", "O", "--data_name", "kitti"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(argv)


def test_main_refuses_before_it_touches_a_gpu(tmp_path):
    from himo_amd import accumulate as acc
    with pytest.raises(ValueError):
        acc.main(str(tmp_path), str(tmp_path / "o"), window=32)
    with pytest.raises(ValueError):
        acc.main(str(tmp_path), str(tmp_path / "o"), voxel=0.0)
    with pytest.raises(ValueError):
        acc.main(str(tmp_path), str(tmp_path / "o"), data_name="kitti")
    with pytest.raises(FileNotFoundError):
        acc.main(str(tmp_path), str(tmp_path / "o"))
    assert not (tmp_path / "o").exists()


def test_exports_are_declared_in_the_header_and_bound():
    from himo_amd import _lib
    header = (REPO / "include" / "himo_amd.h").read_text()
    for name in ("himo_accum_table_bytes", "himo_accum_clear", "himo_accum_insert", "himo_accum_emit", "himo_accum_status"):
        m = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert m, f"include/himo_amd.h does not declare {name}"
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    lib = _lib.load()
    assert lib.himo_abi_version() == 1
    from himo_amd.accumulate import AccumParams
    assert lib.himo_abi_sizeof(b"himo_accum_params") == ctypes.sizeof(AccumParams)
    assert "FLAGS_accumulate := -ffp-contract=off" in (REPO / "himo_amd" / "csrc" / "Makefile").read_text()
    # what needs no device: capacities
    assert lib.himo_accum_table_bytes(16) == 32 * 17 and lib.himo_accum_table_bytes(1 << 26) == 32 * ((1 << 26) + 1)
    for cap in (0, 8, 15, 17, 24, -16, 1 << 27):
        assert lib.himo_accum_table_bytes(cap) == 0, cap


def test_parity_is_said_to_be_unpinned_everywhere():
    from himo_amd import accumulate
    for words in ("sweep accumulation, v1", "PARITY UNPINNED", "bit for bit", "0.501953125", "Not part of v1", "a world-frame output"):
        assert words in accumulate.__doc__, words
    assert "PARITY UNPINNED" in (REPO / "include" / "himo_amd.h").read_text().split("Multi-sweep accumulation")[1][:600]
    assert "PARITY UNPINNED" in (REPO / "himo_amd" / "csrc" / "accumulate.hip").read_text()[:400]
    assert "sweep accumulation, v1; parity unpinned" in (REPO / "README.md").read_text()
    design = (REPO / "DESIGN.md").read_text()
    assert "accumulate.hip" in design and "sweep accumulation, v1" in design
    assert "himo_accum_insert" in (REPO / "INTEGRATION.md").read_text()
    assert "accumulate.txt" in (REPO / "profiles" / "README.md").read_text()
    # both entry points that move points share one device function
    for unit in ("fastnsf.hip", "accumulate.hip"):
        assert "rigid_apply(" in (REPO / "himo_amd" / "csrc" / unit).read_text(), unit
