"""Cross-sensor consistency without a GPU: the rule itself (tests/xsensor_ref.py, the numpy restatement of the rule in
``himo_amd/eval_xsensor.py``) against a double loop written differently and on hand-made edges; the synthetic drive the rule is tried
on; the host glue; and every refusal of the parameters, the entry point and the program, none of which touches a device."""
import ctypes
import re

import numpy as np
import pytest

import xsensor_ref as ref
from conftest import REPO


def two_sensor_cluster(n_a, n_b, seed=0, sep=0.0):
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 1, (n_a + n_b, 3)).astype(np.float32)
    pts[n_a:, 0] += np.float32(sep)
    return pts, np.ones(n_a + n_b, np.int32), np.r_[np.full(n_a, 1), np.full(n_b, 2)].astype(np.uint8)


# ---- the restatement against a double loop ---------------------------------------------------------------------------------------------
def test_restatement_matches_a_brute_force_double_loop():
    rng = np.random.default_rng(5)
    C = 36
    sizes = rng.integers(1, 60, C)
    pts, labels, group = [], [], []
    for k, n in enumerate(sizes):
        pts.append(rng.normal(0, 2, (n, 3)) + rng.uniform(-30, 30, 3))
        labels.append(np.full(n, k + 1))
        group.append(rng.choice([0, 1, 2, 5, 7, 8, 200], n, p=[.3, .3, .2, .08, .08, .02, .02]))
    pts.append(rng.normal(0, 30, (40, 3)))
    labels.append(rng.choice([0, -1, C + 1], 40))
    group.append(rng.integers(0, 3, 40))
    pts, labels, group = np.concatenate(pts).astype(np.float32), np.concatenate(labels).astype(np.int32), np.concatenate(group).astype(np.uint8)
    order = rng.permutation(len(pts))
    pts, labels, group = pts[order], labels[order], group[order]
    pts[rng.choice(len(pts), 12, replace=False), rng.integers(0, 3, 12)] = [np.nan, np.inf, -np.inf] * 4
    dt = rng.uniform(0, 0.1, len(pts)).astype(np.float32)
    dt[rng.choice(len(pts), 8, replace=False)] = np.nan
    for with_dt in (False, True):
        info, rec, mot, m = ref.score(pts, labels, group, C, dt=dt if with_dt else None)
        states, m_rows = ref.brute(pts, labels, group, C, dt=dt if with_dt else None)
        rows, offsets = ref.sort_rows(labels, C)
        assert np.array_equal(info[:, 0], states)
        assert m.tobytes() == m_rows[rows].tobytes()
        assert {ref.SCORED, ref.TOO_FEW, ref.ONE_SENSOR} <= set(states.tolist())
        assert (info[:, 3] == [np.isfinite(m[offsets[k]:offsets[k + 1]]).sum() for k in range(C)]).all()
        assert (rec[:, :, 0].sum(axis=1) == info[:, 1]).all() and (mot == 0).all()
        assert (rec[:, :, 1] != 0).any() == with_dt


# ---- hand-made cases: every state and edge -----------------------------------------------------------------------------------------------
def test_states_in_their_order():
    pts, labels, group = two_sensor_cluster(5, 5)
    assert ref.score(pts, labels, group, 1)[0][0].tolist() == [ref.SCORED, 10, 0b110, 10]
    assert ref.score(pts[:9], labels[:9], group[:9], 1)[0][0].tolist() == [ref.TOO_FEW, 9, 0, 0]
    assert ref.score(pts, labels, group, 1, max_points=9, min_points=9)[0][0].tolist() == [ref.TOO_LARGE, 10, 0, 0]
    # TOO_FEW is tested before TOO_LARGE, TOO_LARGE before ONE_SENSOR
    one = np.ones(10, np.uint8)
    assert ref.score(pts, labels, one, 1, max_points=9, min_points=9)[0][0, 0] == ref.TOO_LARGE
    info, rec, mot, m = ref.score(pts, labels, one, 1, dt=np.full(10, 0.05, np.float32), motion=np.ones((10, 3), np.float32))
    assert info[0].tolist() == [ref.ONE_SENSOR, 10, 0, 0]          # a cluster of one sensor
    assert rec[0, 1].tolist() == [10, 0, 0, 0] and (rec[0, [0, 2, 3, 4, 5, 6, 7]] == 0).all() and (mot == 0).all() and np.isinf(m).all()


def test_a_thin_group_is_neither_query_nor_candidate():
    rng = np.random.default_rng(1)
    pts = rng.normal(0, 1, (24, 3)).astype(np.float32)
    group = np.r_[np.full(10, 0), np.full(10, 3), np.full(4, 6)].astype(np.uint8)        # min_group - 1 = 4 rows of sensor 6
    pts[20:] = pts[:4]                                                                   # ... sitting exactly on rows of sensor 0
    labels = np.ones(24, np.int32)
    info, rec, _, m = ref.score(pts, labels, group, 1, dt=np.full(24, 0.01, np.float32))
    assert info[0].tolist() == [ref.SCORED, 24, 0b1001, 20]
    assert np.isinf(m[20:]).all() and (m[:4] > 0).all()             # not a query; and no candidate: the coincident rows did not win
    assert rec[0, 6].tolist() == [4, 4 * ref.q(np.float32(0.01)), 0, 0]                  # its time is still summed
    with_five = ref.score(np.r_[pts, pts[4:5]], np.ones(25, np.int32), np.r_[group, [6]].astype(np.uint8), 1)
    assert with_five[0][0].tolist() == [ref.SCORED, 25, 0b1001001, 25] and (with_five[3][:5] == 0).all()


def test_unusable_rows():
    pts, labels, group = two_sensor_cluster(6, 6, seed=2)
    base = ref.score(pts, labels, group, 1)[0][0].tolist()
    assert base == [ref.SCORED, 12, 0b110, 12]
    g8 = group.copy()
    g8[0] = 8                                                       # a group id of 8 is unusable
    assert ref.score(pts, labels, g8, 1)[0][0].tolist() == [ref.SCORED, 11, 0b110, 11]
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            p = pts.copy()
            p[7, col] = bad
            info, rec, _, m = ref.score(p, labels, group, 1)
            assert info[0].tolist() == [ref.SCORED, 11, 0b110, 11] and rec[0, 2, 0] == 5 and np.isinf(m[7]) and np.isfinite(np.delete(m, 7)).all()
    dt = np.full(12, 0.02, np.float32)
    dt[3] = np.nan                                                  # a NaN dt is unusable, where dt is given
    assert ref.score(pts, labels, group, 1, dt=dt)[0][0].tolist() == [ref.SCORED, 11, 0b110, 11]
    lab = labels.copy()
    lab[[0, 6]] = [0, 2]                                            # labels outside 1..C
    assert ref.score(pts, lab, group, 1)[0][0].tolist() == [ref.SCORED, 10, 0b110, 10]


def test_coincident_points_near_trunc_and_overflow():
    pts, labels, group = two_sensor_cluster(5, 5, seed=3)
    pts[5:] = pts[:5]                                               # coincident points of two sensors
    info, rec, _, m = ref.score(pts, labels, group, 1)
    assert (m == 0).all() and rec[0, 1].tolist() == [5, 0, 0, 5] and rec[0, 2].tolist() == [5, 0, 0, 5]
    # d exactly at near and exactly at trunc: two sensors on two parallel lines a distance apart that float32 holds exactly
    for gap, near, trunc, want_near, want_c in ((0.25, 0.25, 4.0, 10, 0.25), (0.25, 0.2499, 4.0, 0, 0.25), (4.0, 0.2, 4.0, 0, 4.0),
                                                (5.0, 0.2, 4.0, 0, 4.0), (4.0, 4.0, 4.0, 10, 4.0)):
        p = np.zeros((10, 3), np.float32)
        p[:, 0] = np.r_[np.arange(5), np.arange(5)] * 100.0
        p[5:, 1] = gap
        info, rec, _, m = ref.score(p, labels, group, 1, near=near, trunc=trunc)
        assert (m == np.float32(gap) ** 2).all()
        assert rec[0, :, 3].sum() == want_near and rec[0, :, 2].sum() == 10 * ref.q(want_c), (gap, near, trunc)
    p = np.zeros((10, 3), np.float32)
    p[:5, 0], p[5:, 0] = 3e38, -3e38                                # dx overflows: d2 = +inf, which clips
    info, rec, _, m = ref.score(p, labels, group, 1)
    assert np.isposinf(m).all() and info[0].tolist() == [ref.SCORED, 10, 0b110, 10] and rec[0, :, 2].sum() == 10 * ref.q(4.0) and rec[0, :, 3].sum() == 0


def test_motion_and_time_sums():
    pts, labels, group = two_sensor_cluster(5, 5, seed=4)
    dt = np.r_[np.full(5, 0.0), np.full(5, 0.066)].astype(np.float32)
    dt[0] = 1e30                                                    # clipped to 1024 s
    motion = np.tile(np.array([3.0, 4.0, 0.0], np.float32), (10, 1))
    motion[1, 2] = np.nan                                           # left out of count and sum
    motion[2] = 3e38                                                # clipped at 1024 m
    info, rec, mot, _ = ref.score(pts, labels, group, 1, dt=dt, motion=motion)
    assert rec[0, 1, 1] == ref.q(1024.0) and rec[0, 2, 1] == 5 * ref.q(np.float32(0.066))
    assert mot[0].tolist() == [9, 8 * ref.q(5.0) + ref.q(1024.0)]


# ---- the drive ---------------------------------------------------------------------------------------------------------------------------
def _sum_X(d, which, **kw):
    info, rec, mot, _ = ref.score(d[which], d["labels"], d["group"], int(d["labels"].max()), dt=d["dt"], motion=d["motion"], **kw)
    g = ref.glue(info, rec, mot)
    assert (info[:, 0] == ref.SCORED).all()
    return float(g["X"].sum()), g, (info, rec, mot)


@pytest.mark.parametrize("speed", [20.0, 35.0])
def test_compensation_by_the_true_flow_lowers_the_distance(speed):
    d = ref.drive(seed=int(speed), speeds=[speed] * 4, points=600, noise=0.02)
    raw, g_raw, _ = _sum_X(d, "raw")
    comp, g_comp, _ = _sum_X(d, "comp")
    print(f"{speed} m/s: raw {raw / 4:.3f} m, compensated {comp / 4:.3f} m, ratio {comp / raw:.3f}")
    assert comp <= 0.6 * raw
    assert np.allclose(g_raw["speed"], speed, rtol=1e-5) and np.allclose(g_raw["dt_spread"], 0.066, atol=1e-6)
    assert np.allclose(g_raw["t"][:, 1:4], [[0.0, 0.033, 0.066]] * 4, atol=1e-7) and np.isnan(g_raw["t"][:, 0]).all()


def test_static_vehicles_give_identical_records():
    d = ref.drive(seed=7, speeds=[0.0] * 3, points=600, noise=0.0)
    _, _, a = _sum_X(d, "raw")
    _, _, b = _sum_X(d, "comp")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- parameters, glue --------------------------------------------------------------------------------------------------------------------
def test_parameter_refusals():
    from himo_amd.eval_xsensor import XSensorParams
    p = XSensorParams()
    assert (p.trunc, p.near, p.min_group, p.min_points, p.max_points) == (4.0, 0.2, 5, 10, 8192) == tuple(ref.DEFAULTS.values())
    XSensorParams(trunc=1024, near=0, min_group=1, min_points=2, max_points=2)
    XSensorParams(max_points=1 << 20)
    for bad in (dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("nan")), dict(trunc=float("inf")), dict(trunc=1e-60), dict(trunc=1025.0),
                dict(trunc=True), dict(trunc="4"), dict(near=-0.1), dict(near=float("nan")), dict(near=float("inf")), dict(near=1e39),
                dict(min_group=0), dict(min_group=2.0), dict(min_points=1), dict(min_points=True), dict(max_points=9), dict(max_points=(1 << 20) + 1)):
        with pytest.raises(ValueError, match="XSensorParams"):
            XSensorParams(**bad)


def test_glue_on_hand_made_tables():
    from himo_amd.eval_xsensor import glue
    U = 1 << 24
    info = np.array([[0, 20, 0b0110, 16], [1, 3, 0, 0], [0, 10, 0b10000001, 10]], np.int32)
    rec = np.zeros((3, 8, 4), np.int64)
    rec[0, 1], rec[0, 2], rec[0, 3] = [10, 10 * U // 100, 5 * U, 2], [6, 6 * 4 * U // 100, 3 * U, 6], [4, 4 * U, 0, 0]
    rec[1, 0] = [3, 0, 0, 0]
    rec[2, 0], rec[2, 7] = [5, 0, U, 0], [5, 5 * U // 2, 4 * U, 5]
    mot = np.array([[20, 20 * U * 3], [0, 0], [0, 0]], np.int64)
    g = glue(info, rec, mot, sensor_dt=0.1)
    assert g["X"][0] == 0.5 and g["near"][0] == 0.5 and g["X"][2] == 0.5 and g["near"][2] == 0.5 and np.isnan(g["X"][1]) and np.isnan(g["near"][1])
    assert g["speed"][0] == 3.0 / 0.1 and np.isnan(g["speed"][1:]).all()
    assert g["t"][0, 3] == 1.0 and np.isnan(g["t"][0, 0]) and g["t"][1, 0] == 0.0
    assert abs(g["dt_spread"][0] - 0.03) < 1e-7 and g["dt_spread"][2] == 0.5 and np.isnan(g["dt_spread"][1])      # group 3 of cluster 0 is not live
    assert g["state"].tolist() == [0, 1, 0] and g["queries"].tolist() == [16, 0, 10]
    mine = ref.glue(info, rec, mot, 0.1)
    for k in g:
        assert np.array_equal(g[k], mine[k], equal_nan=True), k
    with pytest.raises(ValueError):
        glue(info, rec[:, :7], mot)
    with pytest.raises(ValueError):
        glue(info, rec, mot, sensor_dt=0.0)


def test_buckets():
    from himo_amd import eval_xsensor as ex
    assert [ex.speed_bucket(v) for v in (0.0, 0.49, 0.5, 9.99, 10.0, 29.9, 30.0, 80.0)] == ["static", "static", "0-10", "0-10", "10-20", "20-30", "30+", "30+"]
    assert [ex.dt_bucket(v) for v in (0.0, 0.0099, 0.01, 0.03, 0.031)] == ["<10ms", "<10ms", "10-30ms", "10-30ms", ">30ms"]
    assert ex.bucket_keys(False) == ["all", "dt:<10ms", "dt:10-30ms", "dt:>30ms"] and len(ex.bucket_keys(True)) == 9


def test_tally_summary_and_the_merge_of_ranks():
    import copy
    from himo_amd import eval_xsensor as ex
    U = ex.UNIT
    info = np.array([[0, 20, 0b0110, 16], [1, 3, 0, 0], [0, 10, 0b0011, 10], [2, 12, 0, 0]], np.int32)
    rec = np.zeros((4, 8, 4), np.int64)
    rec[0, 1], rec[0, 2] = [10, 0, 5 * U, 2], [6, 6 * 4 * U // 100, 3 * U, 6]
    rec[2, 0], rec[2, 1] = [5, 0, U, 0], [5, 5 * U // 200, 4 * U, 5]
    mot = np.array([[20, 20 * U * 3], [0, 0], [10, 0], [0, 0]], np.int64)
    g = ex.glue(info, rec, mot)
    t = ex.new_totals(True)
    ex.tally(t, g, rec, True)
    assert t["states"] == [2, 1, 1, 0]
    assert t["buckets"]["all"] == {"clusters": 2, "queries": 26, "sum_qc": 13 * U, "near": 13, "sum_X": 1.0}
    assert t["buckets"]["speed:30+"]["clusters"] == 1 and t["buckets"]["speed:static"]["queries"] == 10 and t["buckets"]["speed:0-10"]["clusters"] == 0
    assert t["buckets"]["dt:>30ms"]["clusters"] == 1 and t["buckets"]["dt:<10ms"]["clusters"] == 1
    keys = np.array([11, 12, 13, 14], np.int64)
    g_b = dict(g, X=g["X"] * 2, state=np.array([0, 1, 2, 0]))       # under the other name cluster 13 is not scored
    a = ex.new_against(True)
    ex.tally_against(a, g, keys, g_b, keys, True)
    assert a["all"] == {"pairs": 1, "sum_X": 0.5, "sum_X_against": 1.0} and a["speed:30+"]["pairs"] == 1 and a["speed:static"]["pairs"] == 0
    numbers = ex.summary({"x": t}, {"x": a}, "y")
    b = numbers["x"]["buckets"]["all"]
    assert (b["mean_X"], b["mean_X_rows"], b["near_share"]) == (0.5, 0.5, 0.5) and numbers["x"]["buckets"]["speed:0-10"]["mean_X"] is None
    assert numbers["x"]["against"]["buckets"]["all"] == {"pairs": 1, "ratio": 0.5} and numbers["x"]["against"]["buckets"]["dt:10-30ms"]["ratio"] is None
    assert numbers["x"]["states"] == {"scored": 2, "too few": 1, "one sensor": 1, "too large": 0}
    assert "x: clusters scored 2" in ex._table(numbers)
    from himo_amd.distenv import add_sums
    totals, versus = add_sums([{"x": copy.deepcopy(t)}, {"x": copy.deepcopy(a)}], [{"x": copy.deepcopy(t)}, {"x": copy.deepcopy(a)}])
    assert totals["x"]["states"] == [4, 2, 2, 0] and totals["x"]["buckets"]["all"]["sum_qc"] == 26 * U and versus["x"]["all"]["pairs"] == 2
    assert add_sums([{"x": copy.deepcopy(t)}, None], [{"x": copy.deepcopy(t)}, None])[0]["x"]["buckets"]["all"]["clusters"] == 4


# ---- binding -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_carries_the_entry_points():
    from himo_amd import _lib, eval_xsensor
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_xsensor_params") == ctypes.sizeof(eval_xsensor._CParams) == 20
    assert lib.himo_xsensor_workspace_bytes(1000, 10) >= 1000 * 20 + 10 * 32
    assert lib.himo_xsensor_workspace_bytes(0, 0) >= 16
    for bad in ((-1, 1), (10, -1), (2 ** 31, 1)):
        assert lib.himo_xsensor_workspace_bytes(*bad) == 0, bad
    header = (REPO / "include" / "himo_amd.h").read_text()
    for name, args in (("himo_xsensor_workspace_bytes", 2), ("himo_xsensor", 20)):
        m = re.search(r"\b%s\(([^;]*?)\);" % name, header, re.S)
        assert m and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == args, name
    section = header[header.index("Cross-sensor consistency"):header.index("typedef struct himo_xsensor_params")]
    assert "PARITY UNPINNED" in section and "profiles/xsensor.txt" in section and "field data" in section
    unit = (REPO / "himo_amd" / "csrc" / "xsensor.hip").read_text()
    assert "PARITY UNPINNED" in unit[:400] and "HIMO_XSENSOR_CHUNK" in unit
    assert re.search(r"^FLAGS_xsensor := -ffp-contract=off$", (REPO / "himo_amd" / "csrc" / "Makefile").read_text(), re.M)
    for doc, needle in (("README.md", "cross-sensor consistency, v1; parity unpinned"), ("DESIGN.md", "cross-sensor consistency, v1"),
                        ("INTEGRATION.md", "himo_xsensor_workspace_bytes")):
        assert needle in (REPO / doc).read_text(), doc
    assert "PARITY UNPINNED" in eval_xsensor.__doc__ and "profiles/xsensor.txt" in eval_xsensor.__doc__ and "field data" in eval_xsensor.__doc__
    assert (REPO / "profiles" / "xsensor.txt").exists() and "xsensor.txt" in (REPO / "profiles" / "README.md").read_text()
    for p in (REPO / "himo_amd").rglob("*.py"):
        assert not re.search(r"^\s*(import|from)\s+\S*xsensor_ref", p.read_text(), re.M), p
    assert (eval_xsensor.SCORED, eval_xsensor.TOO_FEW, eval_xsensor.ONE_SENSOR, eval_xsensor.TOO_LARGE) == (ref.SCORED, ref.TOO_FEW, ref.ONE_SENSOR, ref.TOO_LARGE)


def test_entry_point_refusals_come_before_any_launch():
    """every refusal returns before the device is touched, so they can be asked for here: host memory stands in for the buffers"""
    from himo_amd import _lib
    from himo_amd.eval_xsensor import XSensorParams
    lib = _lib.load()
    n, C = 16, 2
    pts, labels, rows = np.zeros((n, 3), np.float32), np.ones(n, np.int32), np.arange(n, dtype=np.int64)
    group, dt, motion = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    off = np.array([0, 8, 16], np.int64)
    info, rec, mot, m = np.full((C, 4), 7, np.int32), np.full((C, 8, 4), 7, np.int64), np.full((C, 2), 7, np.int64), np.full(n, 7, np.float32)
    ws = np.zeros(8192, np.uint8)
    ws_at = (ws.ctypes.data + 15) & ~15
    prm = XSensorParams().c_struct()
    P = lambda a: a.ctypes.data                                     # noqa: E731

    def call(**kw):
        a = dict(n=n, pts=P(pts), pitch=3, labels=P(labels), group=P(group), dt=P(dt), motion=P(motion), nc=n, rows=P(rows), C=C, h_off=P(off),
                 d_off=P(off), prm=ctypes.addressof(prm), info=P(info), rec=P(rec), mot=P(mot), m=P(m), ws=ws_at, ws_bytes=4096)
        a.update(kw)
        return lib.himo_xsensor(a["n"], a["pts"], a["pitch"], a["labels"], a["group"], a["dt"], a["motion"], a["nc"], a["rows"], a["C"], a["h_off"],
                                a["d_off"], a["prm"], a["info"], a["rec"], a["mot"], a["m"], a["ws"], a["ws_bytes"], None)
    bad_off = [np.array(v, np.int64) for v in ([1, 8, 16], [0, 8, 15], [0, 9, 8], [0, -1, 16])]
    bad_prm = [XSensorParams().c_struct() for _ in range(11)]
    bad_prm[0].trunc, bad_prm[1].trunc, bad_prm[2].trunc, bad_prm[3].trunc = 0.0, float("nan"), float("inf"), 1025.0
    bad_prm[4].near, bad_prm[5].near, bad_prm[6].near = -1.0, float("nan"), float("inf")
    bad_prm[7].min_group, bad_prm[8].min_points, bad_prm[9].max_points, bad_prm[10].max_points = 0, 1, 9, (1 << 20) + 1
    invalid = [dict(n=-1), dict(nc=-1), dict(nc=n + 1), dict(C=-1), dict(pitch=2), dict(prm=None), dict(h_off=None), dict(d_off=None),
               dict(info=None), dict(rec=None), dict(mot=None), dict(pts=None), dict(labels=None), dict(group=None), dict(rows=None),
               dict(pts=P(pts) + 2), dict(labels=P(labels) + 1), dict(rec=P(rec) + 4), dict(mot=P(mot) + 4), dict(info=P(info) + 2),
               dict(rows=P(rows) + 4), dict(d_off=P(off) + 4), dict(dt=P(dt) + 1), dict(motion=P(motion) + 2), dict(m=P(m) + 2), dict(C=0)]
    invalid += [dict(h_off=P(o)) for o in bad_off] + [dict(prm=ctypes.addressof(q)) for q in bad_prm]
    for kw in invalid:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(n=2 ** 31, nc=n) == _lib.ERR_UNSUPPORTED
    for kw in (dict(ws=None), dict(ws=ws_at + 8), dict(ws_bytes=64)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    assert call(n=0, nc=0, C=0, pts=None, labels=None, group=None, rows=None, h_off=None, d_off=None, info=None, rec=None, mot=None, ws=None,
                ws_bytes=0) == _lib.OK
    assert (info == 7).all() and (rec == 7).all() and (mot == 7).all() and (m == 7).all() and not ws.any()      # nothing was written


# ---- the program's refusals --------------------------------------------------------------------------------------------------------------
def _npz_dataset(root, drop=()):
    from himo_amd.dataset import NpzDataset
    rng = np.random.default_rng(3)
    frames = []
    for k in range(2):
        n = 50
        f = {"scene_id": "s0", "timestamp": 1000 + k, "pc0": rng.normal(0, 5, (n, 3)).astype(np.float32), "pose0": np.eye(4), "pose1": np.eye(4),
             "lidar_dt": np.zeros(n, np.float32), "lidar_id": np.ones(n, np.uint8), "flow": np.zeros((n, 3), np.float32), "gm0": np.zeros(n, bool),
             "ids": np.ones(n, np.int32)}
        if k == 1:
            for name in drop:
                del f[name]
        frames.append(f)
    NpzDataset.write(root, frames)


def test_program_refusals_come_before_the_gpu(tmp_path, monkeypatch, capsys):
    from himo_amd import _lib, eval_xsensor

    def no_gpu():
        raise AssertionError("the program asked for the GPU before it refused")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    plain = tmp_path / "plain"
    _npz_dataset(plain)
    run = lambda d, *rest: eval_xsensor._cli(["--data_dir", str(d)] + list(rest))       # noqa: E731
    with pytest.raises(ValueError, match="not one of --res_names"):
        run(plain, "--res_names", "raw,flow", "--label_key", "ids", "--against", "other")
    with pytest.raises(ValueError, match="res_names"):
        run(plain, "--res_names", "raw,raw", "--label_key", "ids")
    with pytest.raises(ValueError, match="res_names"):
        run(plain, "--res_names", ",", "--label_key", "ids")
    with pytest.raises(ValueError, match="--against with --label_key cluster"):
        run(plain, "--res_names", "raw,flow", "--label_key", "cluster", "--against", "raw")
    with pytest.raises(KeyError, match="seflowpp_best"):                           # a missing result key
        run(plain, "--res_names", "raw,seflowpp_best", "--label_key", "ids")
    with pytest.raises(KeyError, match="ray_label"):                               # a missing label key
        run(plain, "--res_names", "raw,flow", "--label_key", "ray_label")
    with pytest.raises(KeyError, match="other_flow"):                              # a missing motion key
        run(plain, "--res_names", "raw", "--label_key", "ids", "--motion_key", "other_flow")
    with pytest.raises(ValueError, match="XSensorParams.min_group"):
        run(plain, "--res_names", "raw", "--label_key", "ids", "--min_group", "0")
    capsys.readouterr()
    for drop, key in ((("lidar_id",), "lidar_id"), (("gm0",), "gm0")):             # ... found in the SECOND sweep
        d = tmp_path / key
        _npz_dataset(d, drop)
        with pytest.raises(KeyError, match=key):
            run(d, "--res_names", "raw,flow", "--label_key", "cluster" if key == "gm0" else "ids")
        assert f"No {key} in s0/1001" in capsys.readouterr().out
