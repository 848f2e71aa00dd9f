"""Cluster boxes without a GPU: the rule itself (tests/boxfit_ref.py, the numpy restatement of the rule in ``himo_amd/box_fit.py``) on the
synthetic L-shapes it was designed on and on its degenerate cases, the host glue of the package against the restatement's, and the host
logic of the package (parameters, the direction table, the struct mirror, the binding, the program's refusals)."""
import ctypes
import math
import re

import numpy as np
import pytest

import boxfit_ref as ref
from conftest import REPO

SEEDS = (0, 1, 2)
L, W = 4.5, 1.9


# ---- the rule on L-shapes: a 4.5 x 1.9 m shape, two sides visible, 0.02 m noise, random yaw ------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_yaw_of_sparse_and_dense_l_shapes(seed):
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(40):
        yaw, n = rng.uniform(0, math.pi / 2), int(rng.integers(30, 401))
        info, _ = ref.one_box(ref.lshape(rng, n, yaw, L, W))
        assert info[0] == ref.FITTED and info[1] == n
        worst = max(worst, ref.yaw_error_deg(info[2], 90, yaw))
    print(f"\nseed {seed}: n in 30..400, worst yaw error {worst:.3f} deg")
    assert worst <= 2.0                                            # one table step plus noise


@pytest.mark.parametrize("seed", SEEDS)
def test_dense_l_shapes_give_the_size_and_beat_the_minimum_area_choice(seed):
    rng = np.random.default_rng(100 + seed)
    rule = area = dl = dw = 0.0
    for _ in range(40):
        yaw, n = rng.uniform(0, math.pi / 2), int(rng.integers(200, 401))
        xy = ref.lshape(rng, n, yaw, L, W)
        info, box = ref.one_box(xy)
        by_area, _ = ref.one_box(xy, pick=ref.choose_min_area)
        rule, area = max(rule, ref.yaw_error_deg(info[2], 90, yaw)), max(area, ref.yaw_error_deg(by_area[2], 90, yaw))
        dl, dw = max(dl, abs(max(box[3], box[4]) - L)), max(dw, abs(min(box[3], box[4]) - W))
    print(f"\nseed {seed}: n in 200..400, worst yaw error {rule:.3f} deg (minimum area: {area:.3f} deg), |dl| {dl:.3f} m, |dw| {dw:.3f} m")
    assert rule <= 2.0 and dl <= 0.2 and dw <= 0.2
    assert rule < area


# ---- smear: the same vehicle at 30 m/s, swept over dt in [0, 0.1) ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_smear_lengthens_the_raw_box_and_the_true_flow_takes_it_back(seed):
    rng = np.random.default_rng(200 + seed)
    yaw, n, speed, period = rng.uniform(0, math.pi / 2), 300, 30.0, 0.1
    heading = np.array([math.cos(yaw), math.sin(yaw)])
    at_rest = ref.lshape(rng, n, yaw, L, W)
    dt = rng.uniform(0, period, n)
    raw = (at_rest + speed * dt[:, None] * heading).astype(np.float32)
    flow = np.tile((speed * period * heading).astype(np.float32), (n, 1))           # the true displacement per sweep period
    dt0 = (dt.max() - dt).astype(np.float32)
    comp = raw + flow / np.float32(period) * dt0[:, None]                          # p + flow / 0.1 * dt0
    _, box_raw = ref.one_box(raw)
    _, box_comp = ref.one_box(comp)
    l_raw, l_comp = max(box_raw[3], box_raw[4]), max(box_comp[3], box_comp[4])
    print(f"\nseed {seed}: l raw {l_raw:.3f} m, compensated {l_comp:.3f} m")
    assert l_raw - l_comp > 1.0 and abs(l_comp - L) <= 0.2


# ---- degenerate cases -----------------------------------------------------------------------------------------------------------------------
def test_identical_points_give_k_0_and_zero_extents():
    info, box = ref.one_box(np.tile([[3.0, 4.0]], (10, 1)), z=np.full(10, 0.5, np.float32))
    assert info.tolist() == [ref.FITTED, 10, 0, 10, 384, 512, 0, 0, 0, 0, 0, 0]
    assert box[3] == 0 and box[4] == 0 and box[5] == 0 and box[2] == 0.5
    assert box[0] == (384 + 0.5) / 128 and box[1] == (512 + 0.5) / 128


def test_points_on_an_exact_45_degree_line_give_k_half_and_no_width():
    t = np.arange(40) * 0.25 + 5.0
    info, box = ref.one_box(np.stack([t, t], 1))
    assert info[0] == ref.FITTED and info[2] == 45 and info[3] == 40
    rows, _ = ref.glue(info[None], box[None], [1], ref.thetas(90), False)
    assert rows[0, 4] == 0 and abs(rows[0, 3] - 39 * 0.25 * math.sqrt(2)) < 1e-5 and abs(rows[0, 6] - math.pi / 4) < 1e-6


def test_ties_go_to_the_smaller_area_then_to_the_lower_k():
    stats = np.array([[5, 10, 0, 0, 0, 0], [5, 8, 0, 0, 0, 0], [5, 8, 0, 0, 0, 0], [4, 1, 0, 0, 0, 0], [6, 99, 0, 0, 0, 0]])
    assert ref.choose(stats) == 4 and ref.choose(stats[:4]) == 1 and ref.choose(stats[[0, 3]]) == 0 and ref.choose(stats[2:4]) == 0
    # a table whose entries are all equal: every direction ties on both, the choice is k = 0
    rng = np.random.default_rng(5)
    xy = ref.lshape(rng, 60, 0.3)
    pts = np.zeros((60, 3), np.float32)
    pts[:, :2] = xy
    info, _ = ref.fit(pts, np.ones(60, np.int32), 1, np.tile([[3000, 1000]], (7, 1)))
    assert info[0, 0] == ref.FITTED and info[0, 2] == 0
    # the same area in two directions that are not the same direction: (a, b) and (-b, a) swap u and v
    info, _ = ref.fit(pts, np.ones(60, np.int32), 1, np.array([[-1000, 3000], [3000, 1000]]))
    assert info[0, 2] == 0


def test_an_aligned_rectangle_is_recovered_exactly():
    # sides along x and y on the sub-unit grid: 4.5 x 2.0 m from (1, 2)
    edge = lambda a, b, n: np.linspace(a, b, n)                      # noqa: E731
    xs, ys = edge(1.0, 5.5, 37), edge(2.0, 4.0, 17)                  # steps of 0.125 m: exact in float32 and on the grid
    xy = np.concatenate([np.stack([xs, np.full_like(xs, 2.0)], 1), np.stack([xs, np.full_like(xs, 4.0)], 1),
                         np.stack([np.full_like(ys, 1.0), ys], 1), np.stack([np.full_like(ys, 5.5), ys], 1)])
    info, box = ref.one_box(xy)
    assert info[:4].tolist() == [ref.FITTED, len(xy), 0, len(xy)]
    assert box[3] == 4.5 and box[4] == 2.0
    assert box[0] == 3.25 + 0.5 / 128 and box[1] == 3.0 + 0.5 / 128            # the centre of the sub-unit cells that hold the corners
    # sides along the two diagonals: corners on the integer grid, table angle k = K/2
    s = np.arange(0, 33)
    d = np.concatenate([np.stack([s, s], 1), np.stack([s - 8, s + 8], 1), np.stack([-np.arange(9), np.arange(9)], 1),
                        np.stack([32 - np.arange(9), 32 + np.arange(9)], 1)]) * 0.125 + 10.0
    info, box = ref.one_box(d)
    assert info[2] == 45 and info[3] == len(d)
    assert abs(box[3] - 32 * 0.125 * math.sqrt(2)) < 1e-12 and abs(box[4] - 8 * 0.125 * math.sqrt(2)) < 1e-12


def test_states_and_their_order():
    xy = np.stack([np.arange(7) * 0.1, np.zeros(7)], 1)
    info, box = ref.one_box(xy)
    assert info.tolist() == [ref.TOO_FEW, 7] + [0] * 10 and not box.any()
    wide = np.stack([np.array([0.0, 16384 / 128] + [1.0] * 8), np.zeros(10)], 1)
    assert ref.one_box(wide)[0][:2].tolist() == [ref.TOO_LARGE, 10]
    assert ref.one_box(wide[:7])[0][:2].tolist() == [ref.TOO_FEW, 7]               # TOO_FEW is tested first
    ok = np.stack([np.array([0.0, 16383 / 128] + [1.0] * 8), np.zeros(10)], 1)
    assert ref.one_box(ok)[0][0] == ref.FITTED
    assert ref.one_box(ok, max_points=9)[0][:2].tolist() == [ref.TOO_LARGE, 10]
    # rows that are not usable: no label, not finite, at the bound
    pts = np.zeros((12, 3), np.float32)
    pts[:, 0] = np.arange(12)
    pts[8, 2], pts[9, 1], pts[10, 0], pts[11, 0] = np.nan, np.inf, 4194304 / 128, -4194304 / 128
    labels = np.ones(12, np.int32)
    labels[0] = 0
    info, _ = ref.fit(pts, labels, 1, min_points=1)
    assert info[0, :2].tolist() == [ref.FITTED, 7]
    pts[10, 0] = np.nextafter(np.float32(4194304 / 128), np.float32(0))
    assert ref.fit(pts, labels, 1, min_points=1)[0][0, :2].tolist() == [ref.TOO_LARGE, 8]


# ---- heading: rule H --------------------------------------------------------------------------------------------------------------------
def _one(k, eu, ev, motion):
    info = np.array([[ref.FITTED, 20, k, 20, 0, 0, 0, 0, 0, 0, 20, 0]], np.int32)
    box = np.array([[1.0, 2.0, 0.5, eu, ev, 1.5, motion[0], motion[1], motion[2], 0.0]])
    return info, box


def test_heading_flips_by_motion_and_wraps():
    from himo_amd import box_fit
    th = ref.thetas(90)
    cases = [(10, 4.0, 2.0, (1.0, 0.2, 0.0), True), (10, 4.0, 2.0, (-1.0, -0.2, 0.0), True), (10, 2.0, 4.0, (0.2, -1.0, 0.0), True),
             (10, 4.0, 2.0, (0.03, 0.03, 0.5), True), (10, 4.0, 2.0, (-1.0, -0.2, 0.0), False), (0, 4.0, 2.0, (-1.0, 0.0, 0.0), True),
             (0, 4.0, 2.0, (0.0, 1.0, 0.0), True), (89, 2.0, 4.0, (0.0, -1.0, 0.0), True), (0, 3.0, 3.0, (1.0, 0.0, 0.0), True)]
    for k, eu, ev, m, with_motion in cases:
        info, box = _one(k, eu, ev, m)
        rows, moving = ref.glue(info, box, [77], th, with_motion)
        mine, mine_moving = box_fit.glue(info, box, [77], th, with_motion)
        assert rows.tobytes() == mine.tobytes() and moving.tolist() == mine_moving.tolist(), (k, eu, ev, m)
        assert rows.shape == (1, 12) and rows.dtype == np.float32 and -math.pi < rows[0, 6] <= math.pi
        assert rows[0, 3] == max(eu, ev) and rows[0, 4] == min(eu, ev) and rows[0, 10] == 77 and rows[0, 11] == 20
    yaw = lambda i: float(ref.glue(*_one(*cases[i][:4]), [1], th, cases[i][4])[0][0, 6])      # noqa: E731
    mov = lambda i: bool(ref.glue(*_one(*cases[i][:4]), [1], th, cases[i][4])[1][0])          # noqa: E731
    assert abs(yaw(0) - math.radians(10)) < 1e-6 and mov(0)
    assert abs(yaw(1) - (math.radians(10) - math.pi)) < 1e-6 and mov(1)                      # flipped, and wrapped into (-pi, pi]
    assert abs(yaw(2) - (math.radians(100) - math.pi)) < 1e-6                                # ev > eu: the long side is v; then flipped
    assert abs(yaw(3) - math.radians(10)) < 1e-6 and not mov(3)                              # hypot(mx, my) below motion_min: no flip
    assert abs(yaw(4) - math.radians(10)) < 1e-6 and not mov(4)                              # no motion given: no flip
    assert yaw(5) == np.float32(math.pi)                                                     # 0 + pi stays pi: the interval is (-pi, pi]
    assert yaw(6) == 0.0 and mov(6)                                                          # the two products are equal (0): yaw0
    assert abs(yaw(7) - (math.radians(89) + math.pi / 2 - math.pi)) < 1e-6
    assert yaw(8) == 0.0                                                                     # eu == ev: no quarter turn
    rows, _ = ref.glue(*_one(10, 4.0, 2.0, (1.0, 0.2, -0.1)), [1], th, True)
    assert np.allclose(rows[0, 7:10], [10.0, 2.0, -1.0])                                     # v = mean motion / sensor_dt


# ---- BoxParams and directions ---------------------------------------------------------------------------------------------------------------
def test_box_params_refuse_what_the_rule_does_not_admit():
    from himo_amd.box_fit import BoxParams
    from himo_amd.seflow.ssl_label import MIN_PTS
    p = BoxParams()
    assert {k: getattr(p, k) for k in ref.DEFAULTS} == ref.DEFAULTS and p.min_points == MIN_PTS
    for bad in (dict(scale=0.0), dict(scale=-128.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=1e60), dict(scale=1e-60),
                dict(scale="128"), dict(scale=True), dict(tol_q=-1), dict(tol_q=1025), dict(tol_q=13.0), dict(tol_q=True), dict(min_points=0),
                dict(min_points=8.0), dict(max_points=7), dict(max_points=(1 << 20) + 1), dict(max_points=None), dict(min_points=9, max_points=8)):
        with pytest.raises(ValueError, match="BoxParams"):
            BoxParams(**bad)
    ok = BoxParams(scale=64, tol_q=0, min_points=1, max_points=1 << 20)
    c = ok.c_struct()
    assert (c.scale, c.tol_q, c.min_points, c.max_points) == (64.0, 0, 1, 1 << 20)
    assert BoxParams(tol_q=1024, min_points=8, max_points=8).max_points == 8
    with pytest.raises(Exception):
        ok.tol_q = 3                                               # frozen


def test_direction_table():
    from himo_amd import box_fit
    for K in (1, 2, 89, 90, 128):
        d = box_fit.directions(K)
        assert d.dtype == np.int32 and d.shape == (K, 2) and np.array_equal(d, ref.directions(K))
        assert d[0].tolist() == [4096, 0] and np.abs(d).max() <= 4096 and d.min() >= 0 and ((d.astype(np.int64) ** 2).sum(1) > 0).all()
        assert np.array_equal(box_fit.angles(K), ref.thetas(K)) and box_fit.angles(K)[-1] < math.pi / 2
        assert np.array_equal(box_fit.check_directions(d), d)
        # a_k^2 + b_k^2 is 4096^2 to rounding: the extents divide by its root, never by 4096
        assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(1)) - 4096).max() < 1.0
    assert box_fit.directions(90)[45].tolist() == [2896, 2896] and len(box_fit.directions()) == 90
    for bad in (0, 129, -1, 90.0, True):
        with pytest.raises(ValueError, match="directions"):
            box_fit.directions(bad)
    for bad in (np.zeros((0, 2), np.int32), np.zeros((129, 2), np.int32) + 1, [[0, 0]], [[4097, 0]], [[1, -4097]], [[1.0, 0.0]], [1, 0], [[1, 0, 0]]):
        with pytest.raises(ValueError, match="dirs"):
            box_fit.check_directions(bad)
    assert box_fit.check_directions([[-4096, 4096], [0, -1]]).tolist() == [[-4096, 4096], [0, -1]]


def test_ctypes_mirror_has_the_c_struct_size():
    from himo_amd import _lib
    from himo_amd.box_fit import _CParams
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_boxfit_params") == ctypes.sizeof(_CParams) == 16
    assert lib.himo_boxfit_workspace_bytes(1000, 10, 90) >= 8000
    assert lib.himo_boxfit_workspace_bytes(0, 0, 1) >= 16
    for bad in ((-1, 1, 90), (10, -1, 90), (10, 1, 0), (10, 1, 129), (2 ** 31, 1, 90)):
        assert lib.himo_boxfit_workspace_bytes(*bad) == 0, bad


# ---- binding and program ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_carries_the_entry_points():
    from himo_amd import _lib
    header = (REPO / "include" / "himo_amd.h").read_text()
    for name, args in (("himo_boxfit_workspace_bytes", 3), ("himo_boxfit", 18)):
        m = re.search(r"\b%s\(([^;]*?)\);" % name, header, re.S)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == args, name
    assert "typedef struct himo_boxfit_params" in header
    section = header[header.index("Cluster boxes"):header.index("typedef struct himo_boxfit_params")]
    assert "PARITY UNPINNED" in section and "profiles/box_fit.txt" in section and "field data" in section
    unit = (REPO / "himo_amd" / "csrc" / "boxfit.hip").read_text()
    assert "PARITY UNPINNED" in unit[:400] and '#include "blockops.h"' in unit and "group_sum<" in unit and "wave_max_u64(" in unit
    assert re.search(r"^FLAGS_boxfit := -ffp-contract=off$", (REPO / "himo_amd" / "csrc" / "Makefile").read_text(), re.M)
    for doc, needle in (("README.md", "cluster boxes, v1; parity unpinned"), ("DESIGN.md", "cluster boxes, v1"), ("INTEGRATION.md", "boxes_<name>")):
        assert needle in (REPO / doc).read_text(), doc
    from himo_amd import box_fit
    assert "PARITY UNPINNED" in box_fit.__doc__ and "profiles/box_fit.txt" in box_fit.__doc__ and "field data" in box_fit.__doc__
    assert (REPO / "profiles" / "box_fit.txt").exists() and "box_fit.txt" in (REPO / "profiles" / "README.md").read_text()
    for p in (REPO / "himo_amd").rglob("*.py"):
        assert not re.search(r"^\s*(import|from)\s+\S*boxfit_ref", p.read_text(), re.M), p


def test_entry_point_refusals_come_before_any_launch():
    """every refusal returns before the device is touched, so they can be asked for here: host memory stands in for the buffers"""
    from himo_amd import _lib
    from himo_amd.box_fit import BoxParams, directions
    lib = _lib.load()
    n, C = 16, 2
    pts, labels, rows = np.zeros((n, 3), np.float32), np.ones(n, np.int32), np.arange(n, dtype=np.int64)
    off = np.array([0, 8, 16], np.int64)
    info, box, ws = np.full((C, 12), 7, np.int32), np.full((C, 10), 7.0), np.zeros(4096, np.uint8)
    dirs, prm = directions(90), BoxParams().c_struct()
    P = lambda a: a.ctypes.data                                     # noqa: E731

    def call(**kw):
        a = dict(n=n, pts=P(pts), pitch=3, labels=P(labels), nc=n, rows=P(rows), C=C, h_off=P(off), d_off=P(off), motion=None, dirs=P(dirs),
                 K=90, prm=ctypes.addressof(prm), info=P(info), box=P(box), ws=P(ws), ws_bytes=ws.nbytes)
        a.update(kw)
        return lib.himo_boxfit(a["n"], a["pts"], a["pitch"], a["labels"], a["nc"], a["rows"], a["C"], a["h_off"], a["d_off"], a["motion"],
                               a["dirs"], a["K"], a["prm"], a["info"], a["box"], a["ws"], a["ws_bytes"], None)
    bad_off = [np.array(v, np.int64) for v in ([1, 8, 16], [0, 8, 15], [0, 9, 8], [0, -1, 16])]
    bad_dirs = [np.array(v, np.int32) for v in ([[0, 0]], [[4097, 1]], [[1, -4097]])]
    bad_prm = [BoxParams().c_struct() for _ in range(7)]
    bad_prm[0].scale, bad_prm[1].scale, bad_prm[2].tol_q, bad_prm[3].tol_q = 0.0, float("nan"), -1, 1025
    bad_prm[4].min_points, bad_prm[5].max_points, bad_prm[6].max_points = 0, 7, (1 << 20) + 1
    invalid = [dict(n=-1), dict(nc=-1), dict(nc=n + 1), dict(C=-1), dict(pitch=2), dict(K=0), dict(K=129), dict(dirs=None), dict(prm=None),
               dict(h_off=None), dict(d_off=None), dict(info=None), dict(box=None), dict(pts=None), dict(labels=None), dict(rows=None),
               dict(pts=P(pts) + 2), dict(box=P(box) + 4), dict(rows=P(rows) + 4), dict(motion=P(pts) + 1), dict(C=0)]
    invalid += [dict(h_off=P(o)) for o in bad_off] + [dict(dirs=P(d), K=1) for d in bad_dirs] + [dict(prm=ctypes.addressof(q)) for q in bad_prm]
    for kw in invalid:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(n=2 ** 31, nc=n) == _lib.ERR_UNSUPPORTED
    for kw in (dict(ws=None), dict(ws=P(ws) + 8), dict(ws_bytes=64)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    assert call(n=0, nc=0, C=0, pts=None, labels=None, rows=None, h_off=None, d_off=None, info=None, box=None, ws=None, ws_bytes=0) == _lib.OK
    assert (info == 7).all() and (box == 7.0).all()                # nothing was written


def _npz_dataset(root, extra=()):
    from himo_amd.dataset import NpzDataset
    rng = np.random.default_rng(3)
    frames = []
    for k in range(2):
        n = 50
        f = {"scene_id": "s0", "timestamp": 1000 + k, "pc0": rng.normal(0, 5, (n, 3)).astype(np.float32), "pose0": np.eye(4), "pose1": np.eye(4),
             "lidar_dt": np.zeros(n, np.float32), "flow": np.zeros((n, 3), np.float32), "gm0": np.zeros(n, bool), "ids": np.ones(n, np.int32),
             "real": np.ones(n, np.float32), "short": np.ones(n - k, np.int32)}
        for name in extra:
            f[name] = np.zeros((0, 12), np.float32)
        frames.append(f)
    NpzDataset.write(root, frames)


def test_program_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from himo_amd import _lib, box_fit

    def no_gpu():
        raise AssertionError("the program asked for the GPU before it refused")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    plain = tmp_path / "plain"
    _npz_dataset(plain)
    with pytest.raises(ValueError, match="--against with --label_key cluster"):
        box_fit._cli(["--data_dir", str(plain), "--res_names", "raw,flow", "--label_key", "cluster", "--against", "raw"])
    with pytest.raises(ValueError, match="not one of --res_names"):
        box_fit._cli(["--data_dir", str(plain), "--res_names", "raw,flow", "--label_key", "ids", "--against", "other"])
    with pytest.raises(KeyError, match="seflowpp_best"):
        box_fit._cli(["--data_dir", str(plain), "--res_names", "raw,seflowpp_best", "--label_key", "ids"])
    with pytest.raises(KeyError, match="ray_label"):
        box_fit._cli(["--data_dir", str(plain), "--res_names", "raw,flow", "--label_key", "ray_label"])
    with pytest.raises(ValueError, match="res_names"):
        box_fit.main(str(plain), "raw,raw", "ids")
    with pytest.raises(ValueError, match="real: s0/1000 holds float32"):           # a stored key that is no integer label
        box_fit.main(str(plain), "raw,flow", "real")
    with pytest.raises(ValueError, match="short: s0/1001 holds int32 .49,., not one integer per point of its 50 points"):
        box_fit.main(str(plain), "raw,flow", "short")                              # ... found in the SECOND sweep, before the first is written
    with np.load(plain / "s0" / "1000.npz") as z:
        assert not [k for k in z.files if k.startswith("boxes_")]
    with pytest.raises(ValueError, match="cluster="):
        box_fit.main(str(plain), "raw", "cluster", cluster="kmeans")
    with pytest.raises(ValueError, match="BoxParams.tol_q"):
        box_fit._cli(["--data_dir", str(plain), "--res_names", "raw", "--label_key", "ids", "--tol_q", "2000"])
    with pytest.raises(ValueError, match="directions"):
        box_fit._cli(["--data_dir", str(plain), "--res_names", "raw", "--label_key", "ids", "--directions", "200"])
    done = tmp_path / "done"
    _npz_dataset(done, extra=("boxes_flow",))
    with pytest.raises(FileExistsError, match="boxes_flow.*--overwrite"):
        box_fit.main(str(done), "raw,flow", "ids")
    with np.load(done / "s0" / "1000.npz") as z:                   # nothing was written by a refused run
        assert "boxes_raw" not in z.files and z["boxes_flow"].shape == (0, 12)
    assert "parity unpinned" in box_fit._parser().format_help() and "profiles/box_fit.txt" in box_fit._parser().format_help()


def test_the_against_numbers():
    from himo_amd import box_fit
    a = np.zeros((3, 12), np.float32)
    b = np.zeros((2, 12), np.float32)
    a[:, 3], a[:, 4], a[:, 6], a[:, 0] = [7.0, 5.0, 4.0], [2.0, 2.0, 2.0], [0.1, math.pi / 2, 0.0], [0.0, 3.0, 0.0]
    b[:, 3], b[:, 4], b[:, 6], b[:, 1] = [4.5, 4.0], [1.9, 2.5], [0.1 + math.radians(100), 0.0], [4.0, 0.0]
    acc = box_fit.new_against()
    box_fit.tally_against(acc, a, np.array([True, True, False]), np.array([5, 9, 11]), b, np.array([True, False]), np.array([5, 11]))
    assert acc["all"]["pairs"] == 2 and acc["moving"]["pairs"] == 1
    assert abs(acc["all"]["sum_dl"] - 2.5) < 1e-6 and abs(acc["all"]["sum_dw"] - 0.6) < 1e-6 and abs(acc["all"]["sum_centre"] - 4.0) < 1e-6
    assert abs(acc["all"]["sum_yaw_deg"] - 10.0) < 1e-4 and abs(acc["moving"]["sum_yaw_deg"] - 10.0) < 1e-4    # 100 degrees folds to 10
    totals = {"x": box_fit.new_totals()}
    box_fit.tally(totals["x"], a, np.array([True, True, False]))
    out = box_fit.summary(totals, {"x": acc}, "y")
    assert out["x"]["boxes"] == 3 and out["x"]["moving"] == 2 and out["x"]["mean_l_moving"] == 6.0 and out["x"]["against"]["name"] == "y"
    assert abs(out["x"]["against"]["all"]["mean_dl"] - 1.25) < 1e-6 and out["x"]["against"]["moving"]["pairs"] == 1
    assert box_fit.summary({"x": box_fit.new_totals()}, None, None)["x"]["mean_l_moving"] is None


def test_without_a_gpu_it_raises(monkeypatch):
    import torch
    from himo_amd.box_fit import BoxFitter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        BoxFitter()
