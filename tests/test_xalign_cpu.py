"""Cross-sensor alignment without a GPU: the rule itself (tests/xalign_ref.py, the numpy restatement of the rule in
``himo_amd/xalign.py``) against the same rule written as plain double loops and on hand-made edges; the synthetic drive the rule is tried
on; and every refusal of the parameters, the entry points and the program, none of which touches a device."""
import ctypes
import functools
import math
import re

import numpy as np
import pytest

import xalign_ref as ref
import xsensor_ref as xs
from conftest import REPO

f32 = np.float32
SMALL = dict(min_points=6, min_group=2, v_max=20.0, bin=1.0)          # a 41 x 41 table: the double loop stays quick


def same(a, b, what=""):
    for name, x, y in zip(("info", "v", "x"), a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        assert x.tobytes() == y.tobytes(), (what, name, x, y)


def moving_cluster(rng, n, v, groups=(1, 2, 3), times=(0.0, 0.033, 0.066), noise=0.01, centre=(0.0, 0.0, 0.0)):
    """n rows of a 3 x 1.5 x 1 m box moving at v, dealt to ``groups`` in turn, group g recorded at times[g]: (pts, group, tau)"""
    p = rng.uniform(-0.5, 0.5, (n, 3)) * [3.0, 1.5, 1.0] + rng.normal(0, noise, (n, 3)) + centre
    g = np.asarray(groups)[np.arange(n) % len(groups)]
    tau = np.asarray(times, f32)[np.arange(n) % len(groups)]
    p[:, :2] += np.asarray(v)[None, :] * tau[:, None].astype(np.float64)
    return p.astype(f32), g.astype(np.uint8), tau


# ---- the restatement against plain double loops --------------------------------------------------------------------------------------------
def test_restatement_matches_plain_double_loops():
    rng = np.random.default_rng(5)
    vs = [(0.0, 0.0), (6.0, -3.0), (-12.0, 4.0), (0.2, 0.1), (15.0, 15.0), (3.0, 0.0), (0.0, -8.0), (30.0, 0.0)]
    sizes = [40, 57, 33, 48, 5, 60, 24, 36]
    pts, labels, group, tau = [], [], [], []
    for k, (n, v) in enumerate(zip(sizes, vs)):
        p, g, t = moving_cluster(rng, n, v, centre=(20.0 * k, -10.0 * k, 0.0), groups=(0, 2, 7) if k % 2 else (1, 2, 3))
        if k == 5:
            g[:] = 4                                                  # one sensor
        if k == 6:
            t[:] = f32(0.02)                                          # equal capture times
        pts.append(p), labels.append(np.full(n, k + 1)), group.append(g), tau.append(t)
    pts.append(rng.normal(0, 30, (30, 3)).astype(f32)), labels.append(rng.choice([0, -1, 9], 30)), group.append(rng.integers(0, 3, 30).astype(np.uint8))
    tau.append(rng.uniform(0, 0.1, 30).astype(f32))
    pts, labels, group, tau = np.concatenate(pts), np.concatenate(labels).astype(np.int32), np.concatenate(group), np.concatenate(tau)
    order = rng.permutation(len(pts))
    pts, labels, group, tau = pts[order], labels[order], group[order], tau[order]
    hurt = rng.choice(len(pts), 16, replace=False)
    pts[hurt[:6], rng.integers(0, 3, 6)] = [np.nan, np.inf, -np.inf] * 2
    tau[hurt[6:10]] = [np.nan, np.inf, -np.inf, np.nan]
    group[hurt[10:]] = [8, 9, 255, 8, 200, 100]
    for kw in (SMALL, dict(SMALL, max_points=50), dict(SMALL, iters=2, min_gain=0.0), dict(SMALL, trunc=0.3, sigma=0.1, static_speed=7.0)):
        got, want = ref.estimate(pts, labels, group, tau, 8, **kw), ref.brute(pts, labels, group, tau, 8, **kw)
        same(got, want, kw)
    info, v, _ = ref.estimate(pts, labels, group, tau, 8, **SMALL)
    print(info, v)
    assert info[4:7, 0].tolist() == [ref.TOO_FEW, ref.ONE_SENSOR, ref.NO_BASELINE] and info[6, 2] != 0 and info[6, 4] == 0
    assert ref.ALIGNED in info[:, 0] and (info[:4, 6] > 0).all()     # the iterations ran where a vote was cast
    assert (v[info[:, 0] != ref.ALIGNED] == 0).all() and (v[:, 2] == 0).all()


def lattice_pair(rng, n, v, step=0.0625):
    """n rows on a 0.25 m lattice seen by sensor 1 at time 0 and again, moved by exactly v * step, by sensor 2 at time ``step``"""
    p = (np.round(rng.uniform(-0.5, 0.5, (n, 3)) * [3.0, 1.5, 1.0] * 4) / 4).astype(f32)
    pts = np.concatenate([p, p + (np.array([v[0], v[1], 0.0]) * step).astype(f32)]).astype(f32)
    return pts, np.repeat([1, 2], n).astype(np.uint8), np.repeat(np.array([0.0, step], f32), n)


# ---- hand-made cases: every state and edge -----------------------------------------------------------------------------------------------
def both(pts, labels, group, tau, C=1, **kw):
    got = ref.estimate(pts, labels, group, tau, C, **kw)
    same(got, ref.brute(pts, labels, group, tau, C, **kw), kw)
    return got


def test_states_in_their_order():
    rng = np.random.default_rng(1)
    pts, group, tau = lattice_pair(rng, 15, (8.0, 0.0))
    labels = np.ones(30, np.int32)
    assert both(pts, labels, group, tau, **SMALL)[0][0, :4].tolist() == [ref.ALIGNED, 30, 0b110, 30]
    assert both(pts[:5], labels[:5], group[:5], tau[:5], **SMALL)[0][0].tolist() == [ref.TOO_FEW, 5, 0, 0, 0, 0, 0, 0]
    assert both(pts, labels, group, tau, **dict(SMALL, max_points=29))[0][0].tolist() == [ref.TOO_LARGE, 30, 0, 0, 0, 0, 0, 0]
    one = np.ones(30, np.uint8)
    assert both(pts, labels, one, tau, **dict(SMALL, max_points=29))[0][0, 0] == ref.TOO_LARGE       # TOO_LARGE is tested before ONE_SENSOR
    assert both(pts, labels, one, tau, **SMALL)[0][0].tolist() == [ref.ONE_SENSOR, 30, 0, 0, 0, 0, 0, 0]
    # NO_BASELINE comes after them: equal capture times, and mean times closer than tau_min
    info, v, x = both(pts, labels, group, np.full(30, 0.05, f32), **SMALL)
    assert info[0].tolist() == [ref.NO_BASELINE, 30, 0b110, 30, 0, 0, 0, 0] and (v == 0).all() and (x == 0).all()
    close = np.where(group == 1, f32(0.0), f32(0.009)).astype(f32)
    assert both(pts, labels, group, close, **SMALL)[0][0].tolist() == [ref.NO_BASELINE, 30, 0b110, 30, 0, 0, 0, 0]
    assert both(pts, labels, one, close, **SMALL)[0][0, 0] == ref.ONE_SENSOR                          # ONE_SENSOR before NO_BASELINE
    # a thin group is neither query nor candidate, and its time does not make a baseline
    thin = group.copy()
    thin[:1] = 5
    info = both(pts, labels, thin, tau, **SMALL)[0]
    assert info[0, 1:4].tolist() == [30, 0b110, 29]
    # STATIC and REJECTED carry v = 0 and their two sums
    exact, g2, t2 = lattice_pair(rng, 24, (4.0, 4.0))
    ones = np.ones(48, np.int32)
    info, v, x = both(exact, ones, g2, t2, **SMALL)
    assert info[0, 0] == ref.ALIGNED and v[0, :3].tolist() == [4.0, 4.0, 0.0] and x[0, 0] > 0 and x[0, 1] == 0
    info, v, x = both(exact, ones, g2, t2, **dict(SMALL, static_speed=6.0))
    assert info[0, 0] == ref.STATIC and (v == 0).all() and x[0, 0] > 0 and x[0, 1] == 0
    info, v, x = both(exact, ones, g2, t2, **dict(SMALL, v_max=5.0))              # both components inside the table, |v| = 5.66 beyond v_max
    assert info[0, 0] == ref.REJECTED and (v == 0).all() and x[0, 0] > 0 and x[0, 1] == 0


def test_vote_ties_go_to_the_smallest_flat_index():
    # one row of sensor 1 between two rows of sensor 2: two votes, (-10, 0) and (10, 0) m/s short of a hair, in bins (50, 60) and (70, 60)
    # of the 121 x 121 table; every bin around either scores 1, and the first of them in flat order is (49, 59)
    pts = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0]], f32)
    group, tau = np.array([1, 2, 2], np.uint8), np.array([0.0, 0.1, 0.1], f32)
    info, v, x = both(pts, np.ones(3, np.int32), group, tau, min_points=2, min_group=1)
    assert info[0, 4] == 2 and info[0, 5] == 49 * 121 + 59
    votes, flat, v0 = ref.vote(pts, tau, group.astype(np.int64), dict(ref.DEFAULTS))
    assert (votes, flat, v0.tolist()) == (2, 49 * 121 + 59, [-11.0, -1.0])
    # velocities exactly on a bin edge fall into the upper bin; at +-v_max they are inside; just beyond, dropped
    tau = np.array([0.0, 0.125, 0.125], f32)
    for dx, bx in ((0.0625, 61), (-0.0625, 60), (7.5, 120), (-7.5, 0), (7.5625, None), (-7.625, None)):
        p = np.array([[0, 0, 0], [dx, 0, 0], [dx, 0, 0]], f32)        # v = (0 - dx) / (0 - 0.125) = 8 dx: +-0.5 (an edge), +-60, beyond
        table_votes, flat, _ = ref.vote(p, tau, group.astype(np.int64), dict(ref.DEFAULTS))
        if bx is None:
            assert table_votes == 0
        else:
            assert table_votes == 2 and flat == max(bx - 1, 0) * 121 + 59       # the first bin whose neighbourhood holds both votes
        both(p, np.ones(3, np.int32), group, tau, min_points=2, min_group=1)


def test_nearest_row_ties_go_to_the_smallest_sorted_row():
    x = np.array([[0, 0, 0], [0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 0]], f32)
    g = np.array([1, 2, 2, 2, 1])
    keys = ref.nearest(x, g, np.arange(10, 15))
    assert (keys & np.uint64(0xFFFFFFFF)).tolist() == [11, 10, 10, 10, 11]       # three rows at distance 1: the first; two queries at 0: the first
    assert ((keys >> np.uint64(32)).astype(np.uint32).view(f32) == 1.0).all()
    # NaN orders after +inf, and every NaN alike: the smallest row among them
    y = np.array([[0, 0, 0], [np.nan, 0, 0], [3e38, 3e38, 0], [np.nan, 0, 0]], f32)
    keys = ref.nearest(y, np.array([1, 2, 2, 2]), np.arange(4))
    assert keys[0] == (np.uint64(0x7F800000) << np.uint64(32)) | np.uint64(2) and keys[1] == (np.uint64(ref.NAN_BITS) << np.uint64(32))
    # a lattice: coincident rows of two sensors and exact ties everywhere
    rng = np.random.default_rng(3)
    pts, group, tau = lattice_pair(rng, 24, (4.0, 0.0))
    info, v, x = both(pts, np.ones(48, np.int32), group, tau, **SMALL)
    assert info[0, 0] == ref.ALIGNED and v[0].tolist() == [4.0, 0.0, 0.0, 4.0] and x[0, 1] == 0 and info[0, 7] == 48


def test_pairs_exactly_at_tau_min_z_gate_and_trunc():
    rng = np.random.default_rng(7)
    n = 12
    base = rng.uniform(-0.05, 0.05, (3 * n, 3)).astype(f32)
    group = np.repeat([1, 2, 3], n).astype(np.uint8)
    labels = np.ones(3 * n, np.int32)
    tm = f32(0.010)
    kw = dict(min_points=6, min_group=2)
    # |tau_i - tau_j| >= tau_min: a pair exactly at tau_min votes, one a float32 below does not
    for t2, votes in ((tm, 3 * n * n), (np.nextafter(tm, f32(0)), 2 * n * n)):
        tau = np.repeat(np.array([0.0, t2, 0.05], f32), n)
        assert both(base, labels, group, tau, z_gate=1.0, **kw)[0][0, 4] == votes
    # |z_i - z_j| < z_gate: a pair exactly at z_gate does not vote, one a float32 below does
    tau = np.repeat(np.array([0.0, 0.03, 0.06], f32), n)
    for dz, votes in ((f32(0.25), 0), (np.nextafter(f32(0.25), f32(0)), 3 * n * n)):
        p = np.zeros((3 * n, 3), f32)
        p[:, 2] = np.repeat(np.array([0.0, dz, 0.0], f32), n)
        p[2 * n:, 2] = np.where(votes, f32(0.0), f32(0.5))            # (group 3 out of reach of both when nothing may vote)
        p[n:2 * n, 2] = dz
        info = both(p, labels, group, tau, z_gate=0.25, **kw)[0]
        assert info[0, 4] == votes and (info[0, 0] == ref.NO_BASELINE) == (votes == 0)
    # sqrt(d2) <= trunc: a pair exactly at trunc is kept, one a float32 above is dropped.  Half the rows are sensor 2's copies of sensor
    # 1's exactly `gap` above them; the other half, 1 km away, moves at (1, 1) m/s, so the votes fill bins (60, 60) and (61, 61), the
    # first bin with the greatest score is (60, 60) and v_0 is exactly zero: the first iteration sees the rows as recorded
    two, tau2 = np.tile(np.repeat([1, 2], n), 2).astype(np.uint8), np.tile(np.repeat(np.array([0.0, 0.0625], f32), n), 2)
    for gap, pairs in ((f32(2.0), 4 * n), (np.nextafter(f32(2.0), f32(3)), 2 * n)):
        p = np.zeros((4 * n, 3), f32)
        p[:, 0] = np.tile(np.arange(n, dtype=f32) * 8, 4)             # rows 8 m apart: the nearest is the row above or below
        p[n:2 * n, 2] = gap
        p[2 * n:, 0] += f32(1000)
        p[3 * n:, :2] += f32(0.0625)
        info, v, x = both(p, np.ones(4 * n, np.int32), two, tau2, z_gate=4.0, iters=1, **kw)
        assert info[0, 4] == 2 * n and info[0, 5] == 60 * 121 + 60 and info[0, 6:].tolist() == [1, pairs]
        assert x[0, 0] == 2 * n * ref.q(2.0, ref.UNIT_X) + 2 * n * ref.q(math.sqrt(float(f32(2 * 0.0625 ** 2))), ref.UNIT_X)


def test_apply_moves_aligned_rows_only():
    rng = np.random.default_rng(9)
    pts = rng.normal(0, 5, (40, 4)).astype(f32)
    labels = rng.integers(0, 5, 40).astype(np.int32)
    labels[:3] = [7, -2, 4]
    pts[5, 1] = np.nan
    info = np.zeros((4, 8), np.int32)
    info[:, 0] = [ref.ALIGNED, ref.STATIC, ref.REJECTED, ref.ALIGNED]
    v = np.array([[3, 4, 0, 5], [0, 0, 0, 0], [0, 0, 0, 0], [-10, 0.5, 0, 10.0125]], f32)
    E = np.array([[0.999, -0.04, 0, 0.8], [0.04, 0.999, 0, -0.02], [0, 0, 1, 0.01]], f32).reshape(12)
    base = rng.normal(0, 1, (40, 3)).astype(f32)
    base[8] = [np.nan, np.inf, -0.0]
    ego = ref.ego_flow(pts, E)
    for b in (None, base):
        out = ref.apply(pts, labels, info, v, E, base=b)
        keep = ego if b is None else base
        hit = np.isin(labels, (1, 4)) & np.isfinite(pts[:, :3]).all(axis=1)
        assert hit.sum() >= 8 and not hit[5]
        assert out[~hit].tobytes() == keep[~hit].tobytes()
        want = (ego[hit] + (v[labels[hit] - 1, :3] * f32(0.1)).astype(f32)).astype(f32)
        assert out[hit].tobytes() == want.tobytes()
    assert ref.apply(pts, labels, info[:0], v[:0], E, base=base).tobytes() == base.tobytes()


# ---- the drive ---------------------------------------------------------------------------------------------------------------------------
SPEEDS = (0.0, 0.0, 2.0, 5.0, 10.0, 20.0, 30.0, 35.0)
# the worst |v - v_true| [m/s] per speed over seeds 0..3 at 600 points, measured with the restatement; the test asserts twice these
WORST = {10.0: 0.801, 20.0: 0.486, 30.0: 0.368, 35.0: 0.324}
# the worst ratio, over the same vehicles, of the cross-sensor distance after compensation by the written flow to that after
# compensation by the true flow (1.0003 measured, at 20 m/s; most are below 1); the test asserts twice the excess over 1
WORST_RATIO = 1.0003


@functools.lru_cache(maxsize=None)
def drive_case(seed):
    d = xs.drive(seed, list(SPEEDS), points=600)
    tau = (d["dt"].max() - d["dt"]).astype(f32)                      # drive's dt is the time remaining: recorded = p - v dt
    return d, tau, ref.estimate(d["raw"], d["labels"], d["group"], tau, len(SPEEDS))


@pytest.mark.parametrize("seed", range(4))
def test_drive_static_vehicles_stay_and_fast_vehicles_are_aligned(seed):
    """Measured (seeds 0..3, 600 points, the defaults, relative acceptance min_gain = 0.1): every vehicle at 5, 10, 20, 30 and 35 m/s
    ALIGNED, none at 0 or 2 m/s; worst |v - v_true| 0.474 m/s at 5, 0.801 at 10, 0.486 at 20, 0.367 at 30, 0.324 at 35; the mean
    cross-sensor distance of the 35 m/s vehicles falls from 0.299 m to 0.111 m (static vehicles: 0.112 m)."""
    d, tau, (info, v, x) = drive_case(seed)
    E = np.eye(4, dtype=f32)[:3].reshape(12)
    flow = ref.apply(d["raw"], d["labels"], info, v, E)
    base = ref.ego_flow(d["raw"], E)
    X0, X1 = ref.glue(info, x)
    for k, speed in enumerate(SPEEDS):
        mine = d["labels"] == k + 1
        true = d["motion"][mine][0].astype(np.float64) / xs.SENSOR_DT
        err = float(np.hypot(v[k, 0] - true[0], v[k, 1] - true[1]))
        print(f"seed {seed} {speed:4.1f} m/s: {ref_state(info[k, 0])}, |v - v_true| {err:.3f} m/s, iterations {info[k, 6]}, X0 {X0[k]:.4f} X1 {X1[k]:.4f}")
        if speed == 0.0:
            assert info[k, 0] != ref.ALIGNED and (v[k] == 0).all()
            assert flow[mine].tobytes() == base[mine].tobytes()     # its rows keep the base's bytes
        if speed >= 10.0:
            assert info[k, 0] == ref.ALIGNED
            assert err < 2 * WORST[speed]
            assert np.allclose(flow[mine], v[k, :3] * f32(0.1), atol=1e-6)


def ref_state(s):
    return ("aligned", "too few", "one sensor", "too large", "no baseline", "rejected", "static")[int(s)]


@pytest.mark.parametrize("seed", range(4))
def test_drive_written_flow_compensates_as_the_true_flow_does(seed):
    d, tau, (info, v, x) = drive_case(seed)
    flow = ref.apply(d["raw"], d["labels"], info, v, np.eye(4, dtype=f32)[:3].reshape(12))
    comp = (d["raw"] + flow * (d["dt"] / f32(xs.SENSOR_DT))[:, None]).astype(f32)        # a point captured dt late moved dt / sensor_dt of the flow
    score = lambda p: xs.glue(*xs.score(p, d["labels"], d["group"], len(SPEEDS), dt=d["dt"])[:3])["X"]       # noqa: E731
    est, true, raw = score(comp), score(d["comp"]), score(d["raw"])
    for k, speed in enumerate(SPEEDS):
        print(f"seed {seed} {speed:4.1f} m/s: raw {raw[k]:.4f} m, by the written flow {est[k]:.4f} m, by the true flow {true[k]:.4f} m, ratio {est[k] / true[k]:.4f}")
        if speed >= 10.0:
            assert est[k] <= (1 + 2 * (WORST_RATIO - 1)) * true[k]
            assert est[k] < 0.8 * raw[k]


# ---- parameters ----------------------------------------------------------------------------------------------------------------------------
def test_parameter_refusals():
    from himo_amd.xalign import XAlignParams, table_side
    p = XAlignParams()
    assert {k: getattr(p, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    assert table_side(60.0, 1.0) == 121 == ref.table_side(60.0, 1.0) and table_side(61.0, 1.0) == 123 and table_side(10.0, 0.3) == 69
    XAlignParams(iters=100)
    XAlignParams(max_points=8192, iters=64)                          # iters * max_points^2 = 2^32: the most one workgroup is asked to walk
    XAlignParams(v_max=61.0, bin=1.0, min_group=1, min_points=2, max_points=2, iters=1, tol=0, min_gain=0, static_speed=0)
    XAlignParams(max_points=16384, iters=16, trunc=1024, sigma=1024, tau_min=1024, v_max=1024, bin=17.0)
    for bad in (dict(v_max=0.0), dict(v_max=-1.0), dict(v_max=float("nan")), dict(v_max=1025.0, bin=100.0), dict(v_max=62.0), dict(bin=0.9),
                dict(bin=0.0), dict(bin=float("inf")), dict(bin=1e-60), dict(bin=True), dict(tau_min=0.0), dict(tau_min=1025.0),
                dict(tau_min="0.01"), dict(z_gate=0.0), dict(z_gate=float("nan")), dict(z_gate=1e39), dict(sigma=0.0), dict(sigma=1025.0),
                dict(trunc=0.0), dict(trunc=-2.0), dict(trunc=1025.0), dict(trunc=float("inf")), dict(tol=-0.1), dict(tol=float("nan")),
                dict(min_gain=-0.1), dict(min_gain=1.0), dict(min_gain=float("nan")), dict(static_speed=-1.0), dict(static_speed=float("inf")),
                dict(min_group=0), dict(min_group=2.0), dict(min_points=1), dict(min_points=True), dict(max_points=599),
                dict(max_points=16385), dict(iters=0), dict(iters=101), dict(iters=3.0), dict(max_points=16384, iters=17),
                dict(max_points=8192, iters=65)):
        with pytest.raises(ValueError, match="XAlignParams"):
            XAlignParams(**bad)


def test_glue_and_totals_on_hand_made_tables():
    import copy
    from himo_amd import xalign as xa
    U = xa.UNIT
    info = np.array([[0, 700, 0b1110, 600, 9, 9, 7, 600], [1, 3, 0, 0, 0, 0, 0, 0], [5, 800, 0b110, 800, 9, 9, 30, 10],
                     [6, 650, 0b11, 640, 9, 9, 2, 640], [4, 900, 0b11, 900, 0, 0, 0, 0], [0, 601, 6, 600, 1, 1, 3, 1]], np.int32)
    x = np.array([[600 * U // 2, 600 * U // 8], [0, 0], [800 * U, 800 * U], [640 * U // 4, 640 * U // 4], [0, 0], [600 * U, 300 * U]], np.int64)
    v = np.zeros((6, 4), f32)
    v[0, 3], v[5, 3] = 34.0, 9.99
    g = xa.glue(info, x)
    assert g["X0"][[0, 2, 3, 5]].tolist() == [0.5, 1.0, 0.25, 1.0] and g["X1"][[0, 2, 3, 5]].tolist() == [0.125, 1.0, 0.25, 0.5]
    assert np.isnan(g["X0"][[1, 4]]).all() and g["state"].tolist() == [0, 1, 5, 6, 4, 0] and g["iters"].tolist() == [7, 0, 30, 2, 0, 3]
    mine = ref.glue(info, x)
    assert np.array_equal(g["X0"], mine[0], equal_nan=True) and np.array_equal(g["X1"], mine[1], equal_nan=True)
    t = xa.new_totals()
    xa.tally(t, info, v, x)
    assert t["states"] == [2, 1, 0, 0, 1, 1, 1] and t["speed"] == {"0-10": 1, "10-20": 0, "20-30": 0, "30+": 1}
    assert (t["decided"], t["sum_iters"], t["sum_X0"], t["sum_X1"]) == (4, 42, 2.75, 1.875)
    n = xa.summary(t)
    assert n["mean_iters"] == 10.5 and n["ratio"] == 1.875 / 2.75 and n["states"]["no baseline"] == 1 and "aligned 2" in xa._table(n)
    assert xa.summary(xa.new_totals())["mean_X0"] is None
    assert [xa.speed_bucket(s) for s in (0.5, 9.99, 10.0, 29.9, 30.0, 80.0)] == ["0-10", "0-10", "10-20", "20-30", "30+", "30+"]
    from himo_amd.distenv import add_sums
    assert add_sums(copy.deepcopy(t), copy.deepcopy(t))["states"] == [4, 2, 0, 0, 2, 2, 2]
    with pytest.raises(ValueError):
        xa.glue(info[:, :4], x)


# ---- binding -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_carries_the_entry_points():
    from himo_amd import _lib, xalign
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_xalign_params") == ctypes.sizeof(xalign._CParams) == 52
    assert lib.himo_xalign_workspace_bytes(1000, 10) >= 1000 * 20 + 10 * 32
    assert lib.himo_xalign_workspace_bytes(0, 0) >= 16
    for bad in ((-1, 1), (10, -1), (2 ** 31, 1)):
        assert lib.himo_xalign_workspace_bytes(*bad) == 0, bad
    header = (REPO / "include" / "himo_amd.h").read_text()
    for name, args in (("himo_xalign_workspace_bytes", 2), ("himo_xalign", 18), ("himo_xalign_apply", 15)):
        m = re.search(r"\b%s\(([^;]*?)\);" % name, header, re.S)
        assert m and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == args, name
    section = header[header.index("Cross-sensor alignment"):header.index("typedef struct himo_xalign_params")]
    assert "PARITY UNPINNED" in section and "profiles/xalign.txt" in section and "field data" in section
    fields = re.search(r"typedef struct himo_xalign_params \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"(?:int32_t|float) (\w+);", fields) == [k for k, _ in xalign._CParams._fields_]
    for name, value in (("ALIGNED", 0), ("TOO_FEW", 1), ("ONE_SENSOR", 2), ("TOO_LARGE", 3), ("NO_BASELINE", 4), ("REJECTED", 5), ("STATIC", 6),
                        ("TABLE_CELLS", xalign.TABLE_CELLS), ("MAX_POINTS", xalign.MAX_POINTS), ("MAX_ITERS", xalign.MAX_ITERS)):
        assert re.search(r"^#define HIMO_XALIGN_%s %d\b" % (name, value), header, re.M), name
        assert getattr(xalign, name) == value and (name in ("TABLE_CELLS", "MAX_POINTS", "MAX_ITERS") or getattr(ref, name) == value)
    assert re.search(r"^#define HIMO_XALIGN_MAX_WORK %dLL\b" % xalign.MAX_WORK, header, re.M) and xalign.MAX_WORK == 1 << 32
    unit = (REPO / "himo_amd" / "csrc" / "xalign.hip").read_text()
    assert "PARITY UNPINNED" in unit[:400] and "HIMO_XALIGN_CHUNK" in unit and '#include "xsensor_rows.h"' in unit
    assert '#include "xsensor_rows.h"' in (REPO / "himo_amd" / "csrc" / "xsensor.hip").read_text()         # rules A and B are stated once
    assert re.search(r"^FLAGS_xalign := -ffp-contract=off$", (REPO / "himo_amd" / "csrc" / "Makefile").read_text(), re.M)
    for doc, needle in (("README.md", "cross-sensor alignment, v1; parity unpinned"), ("DESIGN.md", "cross-sensor alignment, v1"),
                        ("INTEGRATION.md", "himo_xalign_workspace_bytes")):
        assert needle in (REPO / doc).read_text(), doc
    assert "PARITY UNPINNED" in xalign.__doc__ and "profiles/xalign.txt" in xalign.__doc__ and "field data" in xalign.__doc__
    assert (REPO / "profiles" / "xalign.txt").exists() and "xalign.txt" in (REPO / "profiles" / "README.md").read_text()
    assert (REPO / "scripts" / "exp_xalign.py").exists()
    assert "def _ids_host" not in (REPO / "himo_amd" / "xalign.py").read_text()        # shared with eval_xsensor, not copied
    for p in (REPO / "himo_amd").rglob("*.py"):
        assert not re.search(r"^\s*(import|from)\s+\S*xalign_ref", p.read_text(), re.M), p


def test_entry_point_refusals_come_before_any_launch():
    """every refusal returns before the device is touched, so they can be asked for here: host memory stands in for the buffers"""
    from himo_amd import _lib
    from himo_amd.xalign import XAlignParams
    lib = _lib.load()
    n, C = 16, 2
    pts, labels, rows = np.zeros((n, 3), f32), np.ones(n, np.int32), np.arange(n, dtype=np.int64)
    group, tau = np.zeros(n, np.uint8), np.zeros(n, f32)
    off = np.array([0, 8, 16], np.int64)
    info, v, x = np.full((C, 8), 7, np.int32), np.full((C, 4), 7, f32), np.full((C, 2), 7, np.int64)
    ws = np.zeros(8192, np.uint8)
    ws_at = (ws.ctypes.data + 15) & ~15
    prm = XAlignParams().c_struct()
    P = lambda a: a.ctypes.data                                     # noqa: E731

    def call(**kw):
        a = dict(n=n, pts=P(pts), pitch=3, labels=P(labels), group=P(group), tau=P(tau), nc=n, rows=P(rows), C=C, h_off=P(off), d_off=P(off),
                 prm=ctypes.addressof(prm), info=P(info), v=P(v), x=P(x), ws=ws_at, ws_bytes=4096)
        a.update(kw)
        return lib.himo_xalign(a["n"], a["pts"], a["pitch"], a["labels"], a["group"], a["tau"], a["nc"], a["rows"], a["C"], a["h_off"], a["d_off"],
                               a["prm"], a["info"], a["v"], a["x"], a["ws"], a["ws_bytes"], None)
    bad_off = [np.array(o, np.int64) for o in ([1, 8, 16], [0, 8, 15], [0, 9, 8], [0, -1, 16])]
    edits = [("v_max", 0.0), ("v_max", float("nan")), ("v_max", 1025.0), ("v_max", 62.0), ("bin", 0.0), ("bin", 0.9), ("bin", float("inf")),
             ("tau_min", 0.0), ("tau_min", 1025.0), ("z_gate", 0.0), ("z_gate", float("nan")), ("sigma", 0.0), ("sigma", float("inf")),
             ("trunc", 0.0), ("trunc", 1025.0), ("tol", -1.0), ("tol", float("nan")), ("min_gain", -0.5), ("min_gain", 1.0),
             ("static_speed", -1.0), ("static_speed", float("inf")), ("min_group", 0), ("min_points", 1), ("max_points", 599),
             ("max_points", 16385), ("iters", 0), ("iters", 101), ("iters", 36)]
    bad_prm = []
    for name, value in edits:
        q = XAlignParams().c_struct()
        setattr(q, name, value)
        if (name, value) == ("iters", 36):
            q.max_points = 11000                                      # 36 * 11000^2 is above 2^32, 35 * 11000^2 is not
        bad_prm.append(q)
    ok_prm = XAlignParams(max_points=11000, iters=35).c_struct()
    assert call(prm=ctypes.addressof(ok_prm), ws=None) == _lib.ERR_WORKSPACE      # (admitted: the refusal is the next one in line)
    invalid = [dict(n=-1), dict(nc=-1), dict(nc=n + 1), dict(C=-1), dict(pitch=2), dict(prm=None), dict(h_off=None), dict(d_off=None),
               dict(info=None), dict(v=None), dict(x=None), dict(pts=None), dict(labels=None), dict(group=None), dict(rows=None), dict(tau=None),
               dict(pts=P(pts) + 2), dict(labels=P(labels) + 1), dict(x=P(x) + 4), dict(v=P(v) + 2), dict(info=P(info) + 2),
               dict(rows=P(rows) + 4), dict(d_off=P(off) + 4), dict(tau=P(tau) + 1), dict(C=0)]
    invalid += [dict(h_off=P(o)) for o in bad_off] + [dict(prm=ctypes.addressof(q)) for q in bad_prm]
    for kw, what in zip(invalid, invalid[:len(invalid) - len(edits)] + edits):
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, what
    assert call(n=2 ** 31, nc=n) == _lib.ERR_UNSUPPORTED
    for kw in (dict(ws=None), dict(ws=ws_at + 8), dict(ws_bytes=64)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    assert call(n=0, nc=0, C=0, pts=None, labels=None, group=None, tau=None, rows=None, h_off=None, d_off=None, info=None, v=None, x=None,
                ws=None, ws_bytes=0) == _lib.OK
    # the apply entry point
    out, base, E = np.full((n, 3), 7, f32), np.zeros((n, 3), f32), np.zeros((2, 12), f32)

    def apply(**kw):
        a = dict(n=n, pts=P(pts), pitch=3, labels=P(labels), C=C, info=P(info), v=P(v), S=2, h_off=P(off), d_off=P(off), E=P(E), base=P(base),
                 sensor_dt=0.1, out=P(out))
        a.update(kw)
        return lib.himo_xalign_apply(a["n"], a["pts"], a["pitch"], a["labels"], a["C"], a["info"], a["v"], a["S"], a["h_off"], a["d_off"], a["E"],
                                     a["base"], a["sensor_dt"], a["out"], None)
    for kw in [dict(n=-1), dict(pitch=2), dict(C=-1), dict(S=-1), dict(S=0), dict(sensor_dt=0.0), dict(sensor_dt=float("nan")), dict(h_off=None),
               dict(d_off=None), dict(E=None), dict(pts=None), dict(labels=None), dict(out=None), dict(info=None), dict(v=None),
               dict(pts=P(pts) + 2), dict(out=P(out) + 1), dict(base=P(base) + 2), dict(d_off=P(off) + 4), dict(E=P(E) + 2)] + \
              [dict(h_off=P(o)) for o in bad_off]:
        assert apply(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert apply(n=0, pts=None, labels=None, out=None, h_off=None, d_off=None, E=None, S=0) == _lib.OK
    assert (info == 7).all() and (v == 7).all() and (x == 7).all() and (out == 7).all() and not ws.any()      # nothing was written


# ---- the program's refusals --------------------------------------------------------------------------------------------------------------
def _npz_dataset(root, drop=(), extra=()):
    from himo_amd.dataset import NpzDataset
    rng = np.random.default_rng(3)
    frames = []
    for k in range(2):
        n = 50
        f = {"scene_id": "s0", "timestamp": 1000 + k, "pc0": rng.normal(0, 5, (n, 3)).astype(f32), "pose0": np.eye(4), "pose1": np.eye(4),
             "lidar_dt": np.zeros(n, f32), "lidar_id": np.ones(n, np.uint8), "flow": np.zeros((n, 3), f32), "gm0": np.zeros(n, bool),
             "ids": np.ones(n, np.int32)}
        if k == 1:
            for name in drop:
                del f[name]
            for name in extra:
                f[name] = np.zeros((n, 3), f32)
        frames.append(f)
    NpzDataset.write(root, frames)


def test_program_refusals_come_before_the_gpu(tmp_path, monkeypatch, capsys):
    from himo_amd import _lib, xalign

    def no_gpu():
        raise AssertionError("the program asked for the GPU before it refused")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    plain = tmp_path / "plain"
    _npz_dataset(plain)
    run = lambda d, *rest: xalign._cli(["--data_dir", str(d)] + list(rest))       # noqa: E731
    with pytest.raises(ValueError, match="out_name"):
        run(plain, "--label_key", "ids", "--out_name", "raw")
    with pytest.raises(ValueError, match="is the base"):
        run(plain, "--label_key", "ids", "--base", "flow", "--out_name", "flow")
    with pytest.raises(ValueError, match="cluster="):
        run(plain, "--label_key", "cluster", "--cluster", "kmeans")
    with pytest.raises(ValueError, match="batch"):
        run(plain, "--label_key", "ids", "--batch", "0")
    with pytest.raises(ValueError, match="XAlignParams.min_group"):
        run(plain, "--label_key", "ids", "--min_group", "0")
    with pytest.raises(ValueError, match="XAlignParams.bin"):
        run(plain, "--label_key", "ids", "--bin", "0.5")
    with pytest.raises(KeyError, match="seflowpp_best"):                           # a missing base flow
        run(plain, "--label_key", "ids", "--base", "seflowpp_best")
    with pytest.raises(KeyError, match="ray_label"):                               # a missing label key
        run(plain, "--label_key", "ray_label")
    capsys.readouterr()
    for drop, key in ((("lidar_id",), "lidar_id"), (("lidar_dt",), "lidar_dt"), (("gm0",), "gm0")):      # ... found in the SECOND sweep
        d = tmp_path / key
        _npz_dataset(d, drop)
        with pytest.raises(KeyError, match=key):
            run(d, "--label_key", "cluster" if key == "gm0" else "ids")
        assert f"No {key} in s0/1001" in capsys.readouterr().out
    done = tmp_path / "done"
    _npz_dataset(done, extra=("xalign",))
    with pytest.raises(FileExistsError, match="--overwrite"):
        run(done, "--label_key", "ids")
