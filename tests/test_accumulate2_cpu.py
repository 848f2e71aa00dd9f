"""Sweep accumulation, v2, without a GPU: the numpy restatement of rules A2, I, H and E2 (tests/accumulate2_ref.py; parity with the
reference is unpinned) against hand-worked cases -- the attribute's quantisation at its edges, the label rule, the motion threshold at
and one ulp below it --, why the feature exists as an exact condition (a translating rigid body lands on the target's own rows bit for
bit), the parser's new defaults, the refusal of ``--advect`` on ``raw``, the new exports against the header, and what v2 says about
itself."""
import ctypes
import re

import numpy as np
import pytest

import accumulate2_ref as ref2
import accumulate_ref as ref
from conftest import REPO
from test_accumulate_cpu import EYE, UNIT, key

f32 = np.float32
FAR_EGO = dict(UNIT, ego_min=(-9.0, -9.0, -9.0), ego_max=(-8.0, -8.0, -8.0))


def call(rows, lag=0, T=EYE, **extras):
    return dict(rows=np.asarray(rows, f32).reshape(-1, 3), T=T, lag=lag, **extras)


def test_the_two_hand_worked_intensities():
    out = ref2.accumulate([call([(1.25, 1.5, 0.5), (1.75, 1.5, 0.5)], attr=[100.4, 201.0])], 1.0, **UNIT)
    assert out[0].tolist() == [key(1, 1, 0)] and out[3].tolist() == [2]
    assert out[4].dtype == np.float32 and out[4].tolist() == [150.5]                  # 100 and 201
    out = ref2.accumulate([call([(0.5, 0.5, 0.5)], attr=[0.5], attr_scale=255.0)], 255.0, **UNIT)
    assert ref2.quantise_attr([0.5], 255.0).tolist() == [128]                         # g = 127.5
    assert out[4].view(np.uint32).tolist() == [int(f32(128.0 / 255.0).view(np.uint32))]
    # the v1 columns are v1's
    assert ref.accumulate([(np.array([[0.5, 0.5, 0.5]], f32), EYE, 0)], **UNIT)[1].tolist() == out[1].tolist() == [[0.501953125] * 3]


def test_quantisation_at_its_edges():
    g = np.array([0.0, -1.0, np.nan, 254.49, 254.5, 255.0, 1e9, np.inf, -np.inf, 0.49, 0.5, 1e-30], f32)
    assert ref2.quantise_attr(g, 1.0).tolist() == [0, 0, 0, 254, 255, 255, 255, 255, 0, 0, 1, 0]
    below = np.nextafter(f32(255.0), f32(0))                                          # g + 0.5f rounds to 255.5f's float32 neighbour: floor 255
    assert ref2.quantise_attr([below], 1.0).tolist() == [255]
    assert ref2.quantise_attr([2.0], 127.5).tolist() == [255] and ref2.quantise_attr([1.0], 127.5).tolist() == [128]
    # rows without an attribute count as intensity 0: they add to the count alone
    p = [(4.5, 4.5, 0.5)]
    out = ref2.accumulate([call(p, attr=[90.0]), call(p), call(p, label=[3])], 1.0, **UNIT)
    assert out[3].tolist() == [3] and out[4].tolist() == [30.0] and out[5].tolist() == [3]


def test_the_label_rule():
    assert ref2.tag_of([-1, -(1 << 31), 0, (1 << 24) - 1, 1 << 24, (1 << 31) - 1, 7], 0).tolist() == \
           [255 << 24, 255 << 24, 255 << 24, (255 << 24) | 0xFFFFFF, 255 << 24, 255 << 24, (255 << 24) | 7]
    assert int(ref2.tag_of([7], 255)[0]) == 7 and int(ref2.tag_of([0], 255)[0]) == 0
    p = [(4.5, 4.5, 0.5)]
    lab = lambda calls: ref2.accumulate(calls, **UNIT)[5].tolist()                   # noqa: E731
    assert lab([call(p, 4, label=[9]), call(p, 1, label=[3])]) == [3]                 # freshest wins over larger
    assert lab([call(p, 1, label=[3]), call(p, 4, label=[9])]) == [3]                 # ... in either order of arrival
    assert lab([call(p, 2, label=[3]), call(p, 2, label=[9]), call(p, 2, label=[5])]) == [9]          # a tie takes the larger label
    assert lab([call(p * 3, 2, label=[3, 9, 5])]) == [9]
    assert lab([call(p, 0, label=[-4])]) == [0] and lab([call(p, 0, label=[1 << 24])]) == [0]
    assert lab([call(p, 0, label=[(1 << 24) - 1])]) == [(1 << 24) - 1]
    assert lab([call(p, 3, label=[6]), call(p, 0, label=[0])]) == [0]                 # a fresher row whose label is GIVEN as 0
    assert lab([call(p, 3, label=[6]), call(p, 0)]) == [6]                            # a fresher row without a label leaves word 7 alone
    assert lab([call(p, 3)]) == [0]
    out = ref2.accumulate([call(p, 4, label=[9]), call(p, 1, label=[3])], **UNIT)
    assert out[5].dtype == np.int32 and out[2].tolist() == [1]


def test_the_motion_threshold_at_and_one_ulp_below():
    m = np.array([[0.03, 0.04, 0.0]], f32)
    s = f32(f32(m[0, 0] * m[0, 0]) + f32(m[0, 1] * m[0, 1])) + f32(0.0)
    p = np.array([[1.5, 1.5, 0.5]], f32)
    at, finite = ref2.advect(p, m, 10, s)                                             # s == motion_min2: the row moves
    assert finite.all() and np.array_equal(at, ref.fma32(f32(10.0), m, p)) and at[0, 0] != p[0, 0]
    stay, finite = ref2.advect(p, m, 10, np.nextafter(s, f32(1)))                     # the threshold one ulp above s: it stays
    assert finite.all() and np.array_equal(stay.view(np.uint32), p.view(np.uint32))
    assert ref2.motion_min2(0.05) == f32(0.05 * 0.05) and ref2.motion_min2(0.0) == 0 and ref2.motion_min2(0.05).dtype == np.float32
    # through the table: 10 sweeps at 0.05 m a sweep are half a voxel
    keys = lambda mm: ref2.accumulate([call(p, 10, motion=[(0.05, 0.0, 0.0)] * 1, motion_min=mm)], **UNIT)[1][0, 0]      # noqa: E731
    assert keys(0.0) == f32(2.001953125) and keys(0.051) == f32(1.501953125)
    # the move is ONE fused multiply-add: 3 * (1 + 2^-23) is 1.5 ulp above 3, a tie that rounds up to 2 ulp before - 2^-24 (a quarter
    # ulp) is added, and 1.25 ulp, which rounds down to 1 ulp, when nothing rounds in between
    m1, p1 = np.array([[f32(1 + 2.0 ** -23), 0, 0]], f32), np.array([[f32(-2.0 ** -24), 1.5, 0.5]], f32)
    fused, _ = ref2.advect(p1, m1, 3, 0.0)
    assert fused[0, 0] == ref.fma32(f32(3), m1[0, 0], p1[0, 0]) and fused[0, 0] != f32(f32(3) * m1[0, 0]) + p1[0, 0]


def test_non_finite_motions_drop_rows_and_lag_0_returns_the_rows_bits():
    rng = np.random.default_rng(2)
    p = rng.uniform(0.1, 7.9, (40, 3)).astype(f32)
    p[:, 2] = rng.uniform(0.1, 3.9, 40)
    m = rng.uniform(-30.0, 30.0, (40, 3)).astype(f32)
    moved, finite = ref2.advect(p, m, 0, 0.0)
    assert finite.all() and np.array_equal(moved.view(np.uint32), p.view(np.uint32))  # lag 0: exactly the rows
    m[3, 0], m[8, 1], m[20, 2] = np.nan, np.inf, -np.inf
    _, finite = ref2.advect(p, m, 2, 0.0)
    assert (~finite).nonzero()[0].tolist() == [3, 8, 20]
    got = ref2.accumulate([call(p, 0, motion=m)], **FAR_EGO)
    want = ref.accumulate([(np.delete(p, [3, 8, 20], axis=0), EYE, 0)], **FAR_EGO)
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want))
    # the ego box stays on the row as given: a row inside it is out wherever its motion would take it, one moved into it stays in
    inside, beside = (2.5, 2.5, 1.5), (0.5, 2.5, 1.5)
    out = ref2.accumulate([call([inside, beside], 1, motion=[(3.0, 0.0, 0.0), (2.0, 0.0, 0.0)])], **UNIT)
    assert out[0].tolist() == [key(2, 2, 1)] and out[3].tolist() == [1]


def test_rule_i_on_a_yawed_pose():
    rng = np.random.default_rng(7)

    def pose(yaw, x, y):
        c, s = np.cos(yaw), np.sin(yaw)
        return np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float64)

    pose0, pose1 = pose(0.30, 4.0, -2.0), pose(0.33, 4.9, -1.7)
    pc0 = rng.uniform(-40.0, 40.0, (200, 4)).astype(f32)
    flow = rng.uniform(-3.0, 3.0, (200, 3)).astype(f32)
    got = ref2.flow_motion(pc0, flow, pose0, pose1)
    E = (np.linalg.inv(pose1) @ pose0).astype(f32)
    x, y, z = pc0[:, 0], pc0[:, 1], pc0[:, 2]
    q0 = (ref.fma32(z, E[0, 2], ref.fma32(y, E[0, 1], (x * E[0, 0]).astype(f32))) + E[0, 3]).astype(f32)      # the written sequence
    q1 = (ref.fma32(z, E[1, 2], ref.fma32(x, E[1, 0], (y * E[1, 1]).astype(f32))) + E[1, 3]).astype(f32)
    q2 = (ref.fma32(z, E[2, 2], ref.fma32(x, E[2, 0], (y * E[2, 1]).astype(f32))) + E[2, 3]).astype(f32)
    want = np.stack([flow[:, 0] - (q0 - x), flow[:, 1] - (q1 - y), flow[:, 2] - (q2 - z)], axis=1).astype(f32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a static world: the flow IS the ego motion, so the motion is 0 to rounding; under identity poses the motion is the flow
    static = (ref.rigid_move(pc0[:, :3], E) - pc0[:, :3]).astype(f32)
    assert not ref2.flow_motion(pc0, static, pose0, pose1).any()
    assert np.array_equal(ref2.flow_motion(pc0, flow, np.eye(4), np.eye(4)), flow)


# ---- why the feature exists --------------------------------------------------------------------------------------------------------
def translating_body(n_sweeps=5, step=2.0):
    """a rigid body of 8 rows, one per voxel, coordinates multiples of 2^-6, translating ``step`` m a sweep along x under identity
    poses; the grid is 12 voxels long"""
    rng = np.random.default_rng(11)
    corners = np.array([(ix, iy, iz) for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)], np.float64)
    body = (corners + rng.integers(1, 64, (8, 3)) / 64.0).astype(f32)
    sweeps = [(body + np.array((step * k, 0.0, 0.0), f32)).astype(f32)[rng.permutation(8)] for k in range(n_sweeps)]
    motions = [np.tile(np.array((step, 0.0, 0.0), f32), (8, 1)) for _ in range(n_sweeps)]
    return sweeps, [np.eye(4)] * n_sweeps, motions, dict(UNIT, nx=12)


def test_a_translating_body_lands_on_the_targets_own_rows():
    sweeps, poses, motions, grid = translating_body()
    alone = ref2.accumulate_target(sweeps, poses, 4, 0, **grid)
    moved = ref2.accumulate_target(sweeps, poses, 4, 4, motions=motions, **grid)
    assert len(alone[0]) == 8 and np.array_equal(moved[0], alone[0]) and moved[3].tolist() == [5] * 8
    assert np.array_equal(moved[1].view(np.uint32), alone[1].view(np.uint32)) and not moved[2].any()
    still = ref2.accumulate_target(sweeps, poses, 4, 4, **grid)
    copies = [ref2.accumulate_target(sweeps, poses, k, 0, **grid)[0] for k in range(5)]
    assert len(still[0]) == 40 and still[0].tolist() == sorted(np.concatenate(copies).tolist()) and len(set(still[0].tolist())) == 40
    assert still[3].tolist() == [1] * 40 and sorted(set(still[2].tolist())) == [0, 1, 2, 3, 4]
    # below the threshold nothing moves
    assert np.array_equal(ref2.accumulate_target(sweeps, poses, 4, 4, motions=motions, motion_min=2.5, **grid)[0], still[0])


# ---- the Python side ---------------------------------------------------------------------------------------------------------------
def test_the_parsers_new_defaults_beside_the_old_ones():
    from himo_amd.accumulate import MOTION_MIN, _parser
    from himo_amd.rigid_refine import RigidParams
    a = _parser().parse_args(["--data_dir", "D", "--out_dir", "O"])
    assert (a.data_dir, a.out_dir, a.res_name, a.window, a.voxel, a.drop_ground, a.drop_label, a.data_name, a.overwrite) == \
           ("D", "O", "seflowpp_best", 10, 0.1, False, None, "av2", False)
    assert (a.advect, a.motion_key, a.motion_min, a.intensity, a.intensity_scale, a.carry_label, a.bin_dir) == (False, None, 0.05, False, 1.0, None, None)
    assert MOTION_MIN == RigidParams().static_disp == 0.05
    a = _parser().parse_args("--data_dir D --out_dir O --advect --motion_key seflowpp_best_rigid --motion_min 0.1 --intensity --intensity_scale 255 "
                             "--carry_label ray_label --bin_dir B".split())
    assert (a.advect, a.motion_key, a.motion_min, a.intensity, a.intensity_scale, a.carry_label, a.bin_dir) == \
           (True, "seflowpp_best_rigid", 0.1, True, 255.0, "ray_label", "B")
    text = " ".join(_parser().format_help().split())
    assert "himo_amd.rigid_refine" in text and "zeros without --intensity" in text and "sweep accumulation, v2 (opt-in; parity unpinned" in text


def test_advect_on_raw_is_refused_before_a_gpu_is_touched(tmp_path):
    from himo_amd import accumulate as acc
    with pytest.raises(ValueError, match="motion_key"):
        acc.main(str(tmp_path), str(tmp_path / "o"), res_name="raw", advect=True)
    with pytest.raises(ValueError, match="motion_min"):
        acc.main(str(tmp_path), str(tmp_path / "o"), advect=True, motion_min=-1.0)
    with pytest.raises(ValueError, match="intensity_scale"):
        acc.main(str(tmp_path), str(tmp_path / "o"), intensity=True, intensity_scale=0.0)
    with pytest.raises(FileNotFoundError):                          # a motion key beside raw is admitted: the next refusal is the empty directory's
        acc.main(str(tmp_path), str(tmp_path / "o"), res_name="raw", advect=True, motion_key="flow")
    assert not (tmp_path / "o").exists()
    assert acc._motion_key("seflowpp_best", True, None) == "seflowpp_best" and acc._motion_key("raw", False, None) is None


def test_the_bin_rows(tmp_path):
    from himo_amd.accumulate import write_bin
    xyz = np.arange(12, dtype=f32).reshape(4, 3)
    lag = np.array([0, 1, 10, 255], np.uint8)
    write_bin(tmp_path / "s" / "1.bin", xyz, np.array([0.5, 1, 2, 3], f32), lag)
    rows = np.fromfile(tmp_path / "s" / "1.bin", dtype="<f4").reshape(-1, 5)
    assert np.array_equal(rows[:, :3], xyz) and rows[:, 3].tolist() == [0.5, 1, 2, 3] and np.array_equal(rows[:, 4], lag.astype(f32) * f32(0.1))
    write_bin(tmp_path / "s" / "2.bin", xyz, None, lag)
    assert not np.fromfile(tmp_path / "s" / "2.bin", dtype="<f4").reshape(-1, 5)[:, 3].any()


def test_the_new_exports_are_declared_in_the_header_and_bound():
    from himo_amd import _lib
    from himo_amd.accumulate import AccumParams
    header = (REPO / "include" / "himo_amd.h").read_text()
    for name, args in (("himo_accum_insert_ex", 16), ("himo_accum_emit_ex", 13), ("himo_accum_motion", 7)):
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"include/himo_amd.h does not declare {name}"
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == args, name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    # the extras are plain arguments: v1's signatures, its struct and the ABI version are what they were
    assert [len(_lib.SIGNATURES[n][1]) for n in ("himo_accum_table_bytes", "himo_accum_clear", "himo_accum_insert", "himo_accum_emit", "himo_accum_status")] == \
           [1, 3, 10, 10, 1]
    lib = _lib.load()
    assert lib.himo_abi_version() == 1 and lib.himo_abi_sizeof(b"himo_accum_params") == ctypes.sizeof(AccumParams) == 56
    assert lib.himo_accum_table_bytes(16) == 32 * 17
    for name in ("himo_accum_insert_ex", "himo_accum_emit_ex", "himo_accum_motion"):
        assert hasattr(lib, name)
    # what needs no device: the refusals come before anything is launched
    bad = _lib.ERR_INVALID_ARGUMENT
    p = AccumParams()
    T = EYE.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.himo_accum_insert_ex(4, 64, 3, None, T, 0, ctypes.addressof(p), 64, 16, None, 0.0, 64, 1, 0.0, None, None) == bad       # scale 0
    assert lib.himo_accum_insert_ex(4, 64, 3, None, T, 0, ctypes.addressof(p), 64, 16, None, 0.0, None, 0, 1.0, None, None) == bad     # stride 0
    assert lib.himo_accum_insert_ex(4, 64, 3, None, T, 0, ctypes.addressof(p), 64, 16, None, -1.0, None, 1, 1.0, None, None) == bad    # motion_min2 < 0
    assert lib.himo_accum_insert_ex(4, 64, 3, None, T, 0, ctypes.addressof(p), 64, 16, 66, 0.0, None, 1, 1.0, None, None) == bad       # misaligned
    assert lib.himo_accum_motion(4, 64, 5, 64, T, 64, None) == bad and lib.himo_accum_motion(-1, 64, 3, 64, T, 64, None) == bad
    assert lib.himo_accum_motion(0, None, 3, None, T, None, None) == 0                                                                 # n == 0: no launch


def test_v2_says_that_its_parity_is_unpinned_everywhere():
    from himo_amd import accumulate
    doc = accumulate.__doc__
    for words in ("sweep accumulation, v2", "PARITY UNPINNED, as v1 is", "tests/accumulate2_ref.py", "Not part of v2", "150.5", "(float)(128.0 / 255.0)",
                  "Nothing of v2 has been tried on field data", "by up to 10", "count as intensity 0", "count as label 0", "sweep accumulation, v1",
                  "Not part of v1", "a world-frame output"):
        assert words in doc, words
    not_v2 = " ".join(doc.split("Not part of v2:")[1].split())
    for words in ("chaining flows sweep to sweep", "rotating a cluster about its centre", "future sweeps as sources", "more than one attribute or label",
                  "a count of moved rows per voxel", "a persistent map", "a world-frame output", "an in-line switch of ``save``"):
        assert words in not_v2, words
    section = (REPO / "include" / "himo_amd.h").read_text().split('"sweep accumulation, v2"')[1][:400]
    assert "PARITY UNPINNED" in section
    head = (REPO / "himo_amd" / "csrc" / "accumulate.hip").read_text()[:600]
    assert "sweep accumulation, v2" in head and "PARITY UNPINNED" in head
    assert "sweep accumulation, v2; parity unpinned" in (REPO / "README.md").read_text()
    design = (REPO / "DESIGN.md").read_text()
    assert "sweep accumulation, v2" in design and "accumulate2_ref.py" in design
    integration = (REPO / "INTEGRATION.md").read_text()
    for name in ("himo_accum_insert_ex", "himo_accum_emit_ex", "himo_accum_motion"):
        assert name in integration, name
    assert "accumulate_v2.txt" in (REPO / "profiles" / "README.md").read_text()
