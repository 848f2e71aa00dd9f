"""Cross-sensor alignment on the GPU: ``himo_xalign`` and ``himo_xalign_apply`` against the numpy restatement of the rule
(tests/xalign_ref.py) at the sizes and inputs where the kernels take another path.  ``info``, ``v``, the two sums and the applied flow
match bit for bit: every sum of the rule is an integer sum, the nearest row is one 64-bit minimum and the float64 chain rounds after
every operation.  Small sweeps: a case is a few thousand rows; the largest cluster has ``max_points + 1`` = 4097 rows."""
import ctypes
import functools
import json

import numpy as np
import pytest

import xalign_ref as ref
import xsensor_ref as xs

pytestmark = pytest.mark.gpu

f32 = np.float32
CHUNK = 1024                                    # HIMO_XALIGN_CHUNK: the moved rows a pass stages in LDS at a time
MAX_POINTS = ref.DEFAULTS["max_points"]
LOW = dict(min_points=10)                       # small clusters take part


def sweep(sizes, seed, groups=(1, 2, 3), times=(0.0, 0.033, 0.066), loose=100, shuffle=True, width=4, speeds=None, jitter=0.002):
    """clusters of the given sizes (label i + 1): boxes about a grid of centres moving at speeds[i] (default: a spread of velocities up
    to 40 m/s), their rows dealt to ``groups`` in turn, ``loose`` rows of label 0 among them, rows in random order
    -> dict(pts float32 [N, width], labels int32, group uint8, tau float32)"""
    rng = np.random.default_rng(seed)
    pts, labels, group, tau = [], [], [], []
    for i, n in enumerate(sizes):
        v = speeds[i] if speeds is not None else (rng.uniform(-1, 1, 2) * [40.0, 15.0] if i % 4 else (0.0, 0.0))
        p, g, t = ref.box_cluster(rng, n, v, groups, times, centre=(-40.0 + 12.0 * (i % 8), -40.0 + 12.0 * (i // 8), 0.0), jitter=jitter)
        pts.append(p), labels.append(np.full(n, i + 1, np.int32)), group.append(g), tau.append(t)
    pts.append(rng.uniform(-50, 50, (loose, 3)).astype(f32)), labels.append(np.zeros(loose, np.int32))
    group.append(rng.integers(0, 8, loose).astype(np.uint8)), tau.append(rng.uniform(0, 0.1, loose).astype(f32))
    pts, labels, group, tau = np.concatenate(pts), np.concatenate(labels), np.concatenate(group), np.concatenate(tau)
    pts = np.concatenate([pts, rng.uniform(0, 1, (len(pts), width - 3)).astype(f32)], axis=1)
    order = rng.permutation(len(pts)) if shuffle else np.arange(len(pts))
    return dict(pts=pts[order], labels=labels[order], group=group[order], tau=tau[order])


def device_estimate(gpu, d, C, pts=None, **params):
    """(info, v, x) host copies of one ``himo_xalign`` call on the current stream"""
    import torch
    from himo_amd import xalign as xa
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)                  # noqa: E731
    p = up(d["pts"]) if pts is None else pts
    info, v, x = xa.xalign_labelled(p, up(d["labels"]), up(d["group"]), up(d["tau"]), C, xa.XAlignParams(**params))
    return info.cpu().numpy(), v.cpu().numpy(), x.cpu().numpy()


def want(d, C, **params):
    return ref.estimate(d["pts"], d["labels"], d["group"], d["tau"], C, **params)


def same(got, expect, what=""):
    for name, a, b in zip(("info", "v", "x"), got, expect):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), bad[:5], a[bad[:3]], b[bad[:3]]))


# ---- cluster sizes: wave, query-tile and chunk edges ---------------------------------------------------------------------------------------
SIZES = (9, 10, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1)


@functools.lru_cache(maxsize=None)
def sizes_case():
    d = sweep(SIZES, seed=11)
    return d, want(d, len(SIZES), **LOW)


def test_cluster_sizes_at_the_wave_tile_and_chunk_edges(gpu):
    d, expect = sizes_case()
    assert expect[0][:2, 0].tolist() == [ref.TOO_FEW, ref.ONE_SENSOR] and (expect[0][2:, 3] == SIZES[2:]).all() and expect[0][:, 1].tolist() == list(SIZES)
    assert {ref.ALIGNED, ref.REJECTED} <= set(expect[0][:, 0].tolist()) and (expect[0][2:, 6] >= 1).all() and (expect[0][2:, 6] > 2).any()
    got = device_estimate(gpu, d, len(SIZES), **LOW)
    same(got, expect)
    again = device_estimate(gpu, d, len(SIZES), **LOW)               # a call repeated gives the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_max_points_and_one_more(gpu):
    d = sweep((MAX_POINTS, MAX_POINTS + 1), seed=12, speeds=[(22.0, -6.0), (5.0, 5.0)], loose=20)
    kw = dict(iters=2)                                              # (two iterations: the restatement walks 4096^2 pairs per pass)
    expect = want(d, 2, **kw)
    assert expect[0][:, :2].tolist() == [[ref.ALIGNED, MAX_POINTS], [ref.TOO_LARGE, MAX_POINTS + 1]] and expect[0][0, 6] == 2
    same(device_estimate(gpu, d, 2, **kw), expect)


# ---- group layouts ---------------------------------------------------------------------------------------------------------------------------
def test_group_layouts(gpu):
    rng = np.random.default_rng(21)
    d = sweep((300, 400, 300, 200, 700), seed=21, shuffle=False, loose=50, groups=(1, 2), times=(0.0, 0.05),
              speeds=[(12.0, 3.0), (-20.0, 8.0), (6.0, 0.0), (9.0, 9.0), (0.0, -30.0)])
    lab, group, tau = d["labels"], d["group"], d["tau"]
    p8, g8, t8 = ref.box_cluster(rng, 400, (-20.0, 8.0), groups=tuple(range(8)), times=tuple(0.012 * k for k in range(8)), centre=(-28.0, -40.0, 0.0))
    d["pts"][lab == 2, :3], group[lab == 2], tau[lab == 2] = p8, g8, t8          # eight groups, 12 ms apart
    group[lab == 3] = np.where(np.arange(300) < 4, 5, np.where(np.arange(300) % 2, 0, 3))       # two live groups and a thin one
    group[lab == 4] = 7                                              # all rows of one sensor
    p5, g5, t5 = ref.box_cluster(rng, 660, (0.0, -30.0), groups=(2, 4), times=(0.0, 0.03), centre=(8.0, -40.0, 0.0))
    p6, g6, t6 = ref.box_cluster(rng, 40, (0.0, -30.0), groups=(6,), times=(0.06,), centre=(8.0, -40.0, 0.0))
    d["pts"][lab == 5, :3], group[lab == 5], tau[lab == 5] = np.concatenate([p5, p6]), np.r_[g5, g6], np.r_[t5, t6]      # three groups, one of 40 rows
    expect = want(d, 5, **LOW)
    assert expect[0][:, 2].tolist() == [0b110, 0xff, 0b1001, 0, 0b1010100] and expect[0][3, 0] == ref.ONE_SENSOR
    assert expect[0][2, 1:4].tolist() == [300, 0b1001, 296] and (expect[0][[0, 1, 2, 4], 4] > 0).all()
    same(device_estimate(gpu, d, 5, **LOW), expect)
    order = rng.permutation(len(lab))                                # rows in random order: the same clusters
    shuffled = {k: a[order] for k, a in d.items()}
    same(device_estimate(gpu, shuffled, 5, **LOW), want(shuffled, 5, **LOW))
    # min_group at its edge: with 41 the group of 40 is not live
    same(device_estimate(gpu, d, 5, min_group=41, **LOW), want(d, 5, min_group=41, **LOW))
    assert want(d, 5, min_group=41, **LOW)[0][4, 2] == 0b10100


# ---- edge inputs -------------------------------------------------------------------------------------------------------------------------------
def tiny_clusters():
    """hand-made clusters of a few rows (min_points 2, min_group 1): (pts, labels, group, tau) and what each one is there for"""
    parts, why = [], []

    def add(p, g, t, what):
        parts.append((np.asarray(p, f32).reshape(-1, 3), np.asarray(g, np.uint8), np.asarray(t, f32)))
        why.append(what)
    add([[0, 0, 0], [1, 0, 0], [-1, 0, 0]], [1, 2, 2], [0.0, 0.1, 0.1], "a symmetric cluster: two votes tie, the smallest flat bin wins")
    for dx in (0.0625, -0.0625, 7.5, -7.5, 7.5625, -7.625):
        add([[0, 0, 0], [dx, 0, 0], [dx, 0, 0]], [1, 2, 2], [0.0, 0.125, 0.125], f"v = {8 * dx}: on a bin edge, at +-v_max, beyond")
    rng = np.random.default_rng(3)
    lattice = (np.round(rng.uniform(-0.5, 0.5, (24, 3)) * [3.0, 1.5, 1.0] * 4) / 4)
    for v in ((4.0, 0.0), (-8.0, 4.0), (0.0, 0.0)):
        add(np.concatenate([lattice, lattice + np.array([v[0], v[1], 0.0]) * 0.0625]), np.repeat([1, 2], 24), np.repeat([0.0, 0.0625], 24),
            f"coincident rows across sensors at v = {v}: exact ties of the nearest row")
    base = rng.uniform(-0.05, 0.05, (36, 3))
    tm = f32(0.010)
    for t2 in (tm, np.nextafter(tm, f32(0)), np.nextafter(tm, f32(1))):
        add(base, np.repeat([1, 2, 3], 12), np.repeat(np.array([0.0, t2, 0.05], f32), 12), f"tau differences of exactly tau_min, and a float32 either side ({t2!r})")
    add(base, np.repeat([1, 2, 3], 12), np.repeat(np.array([0.0, tm, np.nextafter(tm, f32(0))], f32), 12), "mean times not tau_min apart: NO_BASELINE")
    for gap in (f32(2.0), np.nextafter(f32(2.0), f32(3))):
        p = np.zeros((48, 3))
        p[:, 0] = np.tile(np.arange(12) * 8.0, 4)
        p[12:24, 2] = gap
        p[24:, 0] += 1000.0
        p[36:, :2] += 0.0625
        add(p, np.tile(np.repeat([1, 2], 12), 2), np.tile(np.repeat([0.0, 0.0625], 12), 2), f"nearest rows exactly at trunc, and a float32 beyond ({gap!r})")
    add([[0, 0, 0], [3e38, 0, 0], [-3e38, 1, 0], [1, 1, 0.1]], [1, 2, 1, 2], [0.0, 0.05, 0.0, 0.05], "d2 overflows: +inf is never within trunc")
    far = np.array([[0.5, 0.25, 100.0], [0.75, 0.25, 100.0]])          # two rows of two more sensors, out of every vote's z gate, captured "at 3e38 s":
    add(np.concatenate([lattice[:12], lattice[:12] + [0.25, 0.0, 0.0], far]), np.r_[np.repeat([1, 2], 12), 3, 4], np.r_[np.repeat([0.0, 0.0625], 12), 3e38, 3e38],
        "moved rows that overflow: -inf against -inf is a NaN, which orders after the +inf of the other rows")
    pts = np.concatenate([np.asarray(p) + [50.0 * (k % 5), 50.0 * (k // 5), 0.0] for k, (p, _, _) in enumerate(parts)]).astype(f32)
    labels = np.concatenate([np.full(len(p), k + 1, np.int32) for k, (p, _, _) in enumerate(parts)])
    return pts, labels, np.concatenate([g for _, g, _ in parts]), np.concatenate([t for _, _, t in parts]), why


def test_ties_bin_edges_v_max_tau_min_trunc_and_overflow(gpu):
    pts, labels, group, tau, why = tiny_clusters()
    d = dict(pts=pts, labels=labels, group=group, tau=tau)
    kw = dict(min_points=2, min_group=1, z_gate=4.0)
    expect = want(d, len(why), **kw)
    info = expect[0]
    assert info[0, 4:6].tolist() == [2, 49 * 121 + 59]
    assert info[1:7, 4].tolist() == [2, 2, 2, 2, 0, 0] and info[1:5, 5].tolist() == [60 * 121 + 59, 59 * 121 + 59, 119 * 121 + 59, 59]
    assert info[7:10, 0].tolist() == [ref.ALIGNED, ref.ALIGNED, ref.STATIC] and expect[1][7].tolist() == [4.0, 0.0, 0.0, 4.0] and (expect[2][7:10, 1] == 0).all()
    assert info[10:13, 4].tolist() == [3 * 144, 2 * 144, 3 * 144] and info[13, 0] == ref.NO_BASELINE and info[13, 4] == 0
    assert (info[14:16, 5] == 60 * 121 + 60).all() and info[16, 0] == ref.ALIGNED and info[17, 3] == 26 and info[17, 7] == 24 and abs(info[17, 5] // 121 - 60) >= 2
    got = device_estimate(gpu, d, len(why), **kw)
    for k, what in enumerate(why):
        same([a[k:k + 1] for a in got], [a[k:k + 1] for a in expect], what)
    one = dict(kw, iters=1)                                          # the first iteration alone: the pairs at v_0
    first = want(d, len(why), **one)
    assert first[0][14:16, 6:].tolist() == [[1, 48], [1, 24]]          # exactly at trunc: kept; a float32 beyond: dropped
    same(device_estimate(gpu, d, len(why), **one), first, "one iteration")


def test_labels_outside_pitch_and_non_finite_rows(gpu):
    import torch
    rng = np.random.default_rng(31)
    d = sweep((150, 90, 700, 33), seed=31, groups=(0, 4, 7), width=7)
    d["pts"][:, :3] = np.round(d["pts"][:, :3] * 8) / 8               # a 0.125 m lattice: exact ties
    d["labels"][rng.choice(len(d["labels"]), 30, replace=False)] = rng.choice([-3, 5, 1 << 30], 30)       # labels outside 1..C
    bad = rng.choice(len(d["labels"]), 50, replace=False)
    d["pts"][bad[:30], rng.integers(0, 3, 30)] = rng.choice([np.nan, np.inf, -np.inf], 30)
    d["group"][bad[30:40]] = rng.choice([8, 9, 255], 10)
    d["tau"][bad[40:]] = rng.choice([np.nan, np.inf, -np.inf], 10)
    expect = want(d, 4, **LOW)
    assert (expect[0][:, 1] <= [150, 90, 700, 33]).all() and (expect[0][:, 1] < [150, 90, 700, 33]).any() and (expect[0][:, 3] > 0).all()
    wide = torch.from_numpy(d["pts"]).to(gpu)
    same(device_estimate(gpu, d, 4, pts=wide, **LOW), expect, "pitch 7")
    same(device_estimate(gpu, d, 4, pts=wide[:, :4].contiguous(), **LOW), expect, "pitch 4")
    same(device_estimate(gpu, d, 4, pts=wide[:, :5].contiguous(), **LOW), expect, "pitch 5")
    same(device_estimate(gpu, d, 4, pts=wide[:, :3].contiguous(), **LOW), expect, "pitch 3")
    kw = dict(LOW, trunc=0.5, sigma=0.125, z_gate=0.125, bin=2.0, v_max=50.0, tol=0.0, iters=6, min_gain=0.0, static_speed=3.0, max_points=699)
    same(device_estimate(gpu, d, 4, pts=wide, **kw), want(d, 4, **kw), "other parameters on the lattice")


# ---- batching ----------------------------------------------------------------------------------------------------------------------------------
def test_many_small_clusters_in_one_call(gpu):
    d = sweep((24,) * 400, seed=41, loose=300, groups=(1, 2), times=(0.0, 0.05))
    kw = dict(min_points=12, min_group=3, iters=5)
    expect = want(d, 400, **kw)
    assert (expect[0][:, 3] == 24).all() and len(set(expect[0][:, 0].tolist())) >= 2
    same(device_estimate(gpu, d, 400, **kw), expect)
    info = device_estimate(gpu, d, 450, **kw)[0]                      # clusters without rows after the last one that has any
    assert info[:400].tobytes() == expect[0].tobytes() and (info[400:] == [ref.TOO_FEW, 0, 0, 0, 0, 0, 0, 0]).all()


def test_sweeps_laid_end_to_end_equal_the_calls_one_by_one(gpu):
    calls = [sweep((40, 300, 1100), seed=51), sweep((500, 20, 64, 9), seed=52), sweep((257,), seed=53)]
    counts = [int(d["labels"].max()) for d in calls]
    base = np.concatenate([[0], np.cumsum(counts)])
    one = {k: np.concatenate([d[k] for d in calls]) for k in calls[0]}
    one["labels"] = np.concatenate([np.where(d["labels"] > 0, d["labels"] + b, 0) for d, b in zip(calls, base)]).astype(np.int32)
    whole = device_estimate(gpu, one, int(base[-1]), **LOW)
    singles = [device_estimate(gpu, d, c, **LOW) for d, c in zip(calls, counts)]
    for k, name in enumerate(("info", "v", "x")):
        assert whole[k].tobytes() == np.concatenate([s[k] for s in singles]).tobytes(), name
    same(whole, want(one, int(base[-1]), **LOW))


def test_estimator_compacts_arbitrary_ids(gpu):
    from himo_amd.xalign import XAlign, XAlignParams
    d = sweep((40, 300, 25), seed=61)
    ids = np.array([0, 7, 1 << 33, 4_000_000_000], np.int64)[d["labels"]]
    res = XAlign(gpu, XAlignParams(**LOW)).estimate(d["pts"], ids, d["group"], d["tau"])
    assert res.ids.tolist() == [7, 4_000_000_000, 1 << 33]
    relabel = np.array([0, 1, 3, 2], np.int32)[d["labels"]]
    expect = ref.estimate(d["pts"], relabel, d["group"], d["tau"], 3, **LOW)
    same((res.info, res.v, res.x), expect)
    assert res.labels.cpu().numpy().tolist() == relabel.tolist()
    X0, X1 = ref.glue(expect[0], expect[2])
    assert np.array_equal(res.glue["X0"], X0, equal_nan=True) and np.array_equal(res.glue["X1"], X1, equal_nan=True)
    empty = XAlign(gpu).estimate(np.zeros((0, 3), f32), np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, f32))
    assert empty.info.shape == (0, 8) and empty.v.shape == (0, 4)
    with pytest.raises(ValueError, match="tau"):
        XAlign(gpu).estimate(d["pts"], ids, d["group"], None)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_refusals_leave_poisoned_outputs_untouched(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.xalign import XAlignParams
    lib = _lib.load()
    d = sweep((40, 30), seed=71, loose=10)
    n, C = len(d["labels"]), 2
    order, off = xs.sort_rows(d["labels"], C)
    nc = len(order)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)                  # noqa: E731
    pts, labels, group, tau, rows, d_off = (up(d["pts"]), up(d["labels"]), up(d["group"]), up(d["tau"]), up(order), up(off))
    info = torch.full((C, 8), 7, dtype=torch.int32, device=gpu)
    v = torch.full((C, 4), 7.0, dtype=torch.float32, device=gpu)
    x = torch.full((C, 2), 7, dtype=torch.int64, device=gpu)
    ws = torch.zeros(int(lib.himo_xalign_workspace_bytes(nc, C)) + 16, dtype=torch.uint8, device=gpu)
    prm = XAlignParams(**LOW).c_struct()
    P = _lib.ptr

    def call(**kw):
        a = dict(n=n, pts=P(pts), pitch=4, labels=P(labels), group=P(group), tau=P(tau), nc=nc, rows=P(rows), C=C, h_off=off.ctypes.data,
                 d_off=P(d_off), prm=ctypes.addressof(prm), info=P(info), v=P(v), x=P(x), ws=P(ws), ws_bytes=ws.numel() - 16)
        a.update(kw)
        with torch.cuda.device(gpu):
            return lib.himo_xalign(a["n"], a["pts"], a["pitch"], a["labels"], a["group"], a["tau"], a["nc"], a["rows"], a["C"], a["h_off"],
                                   a["d_off"], a["prm"], a["info"], a["v"], a["x"], a["ws"], a["ws_bytes"], _lib.stream_handle())
    bad_off = [np.array(o, np.int64) for o in ([1, 40, nc], [0, 40, nc - 1], [0, 41, 40], [0, -1, nc])]
    bad_prm = []
    for name, value in (("v_max", 0.0), ("v_max", 62.0), ("bin", 0.9), ("bin", float("nan")), ("tau_min", 0.0), ("z_gate", 0.0), ("sigma", 0.0),
                        ("trunc", 1025.0), ("tol", -1.0), ("min_gain", 1.0), ("static_speed", float("inf")), ("min_group", 0), ("min_points", 1),
                        ("max_points", 9), ("max_points", 16385), ("iters", 0)):
        q = XAlignParams(**LOW).c_struct()
        setattr(q, name, value)
        bad_prm.append(q)
    invalid = [dict(n=-1), dict(nc=-1), dict(nc=n + 1), dict(C=-1), dict(pitch=2), dict(prm=None), dict(h_off=None), dict(d_off=None),
               dict(info=None), dict(v=None), dict(x=None), dict(pts=None), dict(labels=None), dict(group=None), dict(rows=None), dict(tau=None),
               dict(pts=P(pts) + 2), dict(x=P(x) + 4), dict(rows=P(rows) + 4), dict(tau=P(tau) + 1), dict(v=P(v) + 2), dict(C=0)]
    invalid += [dict(h_off=o.ctypes.data) for o in bad_off] + [dict(prm=ctypes.addressof(q)) for q in bad_prm]
    for kw in invalid:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(n=2 ** 31) == _lib.ERR_UNSUPPORTED
    for kw in (dict(ws=None), dict(ws=P(ws) + 8), dict(ws_bytes=64)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    assert call(n=0, nc=0, C=0) == _lib.OK
    # the apply entry point
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device=gpu)
    pt_off = np.array([0, n], np.int64)
    d_pt, E = up(pt_off), up(np.eye(4, dtype=f32)[:3].reshape(1, 12))

    def apply(**kw):
        a = dict(n=n, pts=P(pts), pitch=4, labels=P(labels), C=C, info=P(info), v=P(v), S=1, h_off=pt_off.ctypes.data, d_off=P(d_pt), E=P(E),
                 base=None, sensor_dt=0.1, out=P(out))
        a.update(kw)
        with torch.cuda.device(gpu):
            return lib.himo_xalign_apply(a["n"], a["pts"], a["pitch"], a["labels"], a["C"], a["info"], a["v"], a["S"], a["h_off"], a["d_off"],
                                         a["E"], a["base"], a["sensor_dt"], a["out"], _lib.stream_handle())
    for kw in (dict(n=-1), dict(pitch=2), dict(C=-1), dict(S=0), dict(sensor_dt=0.0), dict(sensor_dt=float("inf")), dict(h_off=None), dict(d_off=None),
               dict(E=None), dict(pts=None), dict(labels=None), dict(out=None), dict(info=None), dict(v=None), dict(out=P(out) + 2),
               dict(h_off=np.array([0, n - 1], np.int64).ctypes.data), dict(h_off=np.array([1, n], np.int64).ctypes.data)):
        assert apply(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    torch.cuda.synchronize(gpu)
    assert (info == 7).all() and (v == 7).all() and (x == 7).all() and (out == 7).all() and not ws.any()       # nothing was written
    assert call() == _lib.OK                                         # ... and the same buffers take the calls that are admitted
    assert apply() == _lib.OK
    torch.cuda.synchronize(gpu)
    expect = want(d, C, **LOW)
    same((info.cpu().numpy(), v.cpu().numpy(), x.cpu().numpy()), expect)
    assert out.cpu().numpy().tobytes() == ref.apply(d["pts"], d["labels"], expect[0], expect[1], np.eye(4, dtype=f32)[:3].reshape(12)).tobytes()


# ---- the apply kernel ----------------------------------------------------------------------------------------------------------------------------
def pose(k):
    yaw = 0.02 * k
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0, 0.8 * k], [s, c, 0.0, 0.03 * k], [0.0, 0.0, 1.0, 0.01 * k], [0.0, 0.0, 0.0, 1.0]])


def test_apply_moves_the_rows_of_aligned_clusters_only(gpu):
    import torch
    from himo_amd import xalign as xa
    rng = np.random.default_rng(81)
    sweeps = [sweep((300, 64, 40), seed=82, speeds=[(15.0, -4.0), (0.0, 0.0), (8.0, 8.0)], width=5),
              sweep((20, 500), seed=83, speeds=[(3.0, 3.0), (-25.0, 2.0)], width=5, loose=257)]
    # a cluster the rule decides as STATIC: 24 lattice rows that two sensors recorded at the very same places 62.5 ms apart
    still = (np.round(rng.uniform(-0.5, 0.5, (24, 3)) * [3.0, 1.5, 1.0] * 4) / 4 + [60.0, 60.0, 0.0]).astype(f32)
    extra = dict(pts=np.concatenate([np.tile(still, (2, 1)), rng.uniform(0, 1, (48, 2)).astype(f32)], axis=1), labels=np.full(48, 3, np.int32),
                 group=np.repeat([1, 2], 24).astype(np.uint8), tau=np.repeat(np.array([0.0, 0.0625], f32), 24))
    sweeps[1] = {k: np.concatenate([sweeps[1][k], extra[k]]) for k in extra}
    one = {k: np.concatenate([d[k] for d in sweeps]) for k in sweeps[0]}
    one["labels"] = np.concatenate([sweeps[0]["labels"], np.where(sweeps[1]["labels"] > 0, sweeps[1]["labels"] + 3, 0)]).astype(np.int32)
    unlabelled = one["labels"] == 0
    one["labels"][rng.choice(np.flatnonzero(one["labels"] < 6), 6, replace=False)] = [-1, 7, 9, 1 << 20, -7, 7]      # labels outside 1..C
    hurt = rng.choice(np.flatnonzero(one["labels"] == 1), 3, replace=False)
    one["pts"][hurt, [0, 1, 2]] = [np.nan, np.inf, -np.inf]          # rows of an ALIGNED cluster that are not finite keep the base
    pt_off = np.array([0, len(sweeps[0]["labels"]), len(one["labels"])], np.int64)
    E = np.stack([xa.ego_transform(pose(3), pose(4)), xa.ego_transform(pose(7), pose(9))])
    assert np.array_equal(E[0], ref_E(pose(3), pose(4)))
    expect = want(one, 6, **LOW)
    states = expect[0][:, 0]
    assert states.tolist() == [ref.ALIGNED, ref.REJECTED, ref.ALIGNED, ref.ALIGNED, ref.ALIGNED, ref.STATIC]
    kept = np.isin(one["labels"], (2, 6))                            # the rows of the REJECTED and of the STATIC cluster
    assert (one["labels"] == 2).sum() >= 60 and (one["labels"] == 6).sum() == 48 and unlabelled.sum() >= 357
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)                  # noqa: E731
    info, v, x = xa.xalign_labelled(up(one["pts"]), up(one["labels"]), up(one["group"]), up(one["tau"]), 6, xa.XAlignParams(**LOW))
    same((info.cpu().numpy(), v.cpu().numpy(), x.cpu().numpy()), expect)
    base = rng.normal(0, 1, (len(one["labels"]), 3)).astype(f32)
    base[rng.choice(len(base), 5, replace=False)] = [np.nan, np.inf, -0.0]
    for b in (None, base):
        out = xa.xalign_apply(up(one["pts"]), up(one["labels"]), info, v, pt_off, E, None if b is None else up(b), 0.1).cpu().numpy()
        parts = [ref.apply(one["pts"][pt_off[s]:pt_off[s + 1]], one["labels"][pt_off[s]:pt_off[s + 1]], expect[0], expect[1], E[s],
                           None if b is None else b[pt_off[s]:pt_off[s + 1]]) for s in range(2)]
        assert out.tobytes() == np.concatenate(parts).tobytes(), "raw" if b is None else "stored"
        lab = one["labels"]
        inside = (lab >= 1) & (lab <= 6)
        moved = inside & np.isfinite(one["pts"][:, :3]).all(axis=1) & (states[np.where(inside, lab - 1, 0)] == ref.ALIGNED)
        assert 700 < moved.sum() < inside.sum() and not moved[hurt].any() and not moved[kept].any() and not moved[unlabelled].any()
        # STATIC, REJECTED, unlabelled and out-of-range rows keep the base's bytes: the ego-motion flow (raw) or the stored flow
        keep = np.concatenate([ref.ego_flow(one["pts"][pt_off[s]:pt_off[s + 1]], E[s]) for s in range(2)]) if b is None else base
        for rows, what in ((one["labels"] == 6, "STATIC"), (one["labels"] == 2, "REJECTED"), (unlabelled, "unlabelled"), (~moved, "every other row")):
            assert out[rows].tobytes() == keep[rows].tobytes(), (what, "raw" if b is None else "stored")
        assert not (out[moved] == keep[moved]).all(axis=1).any()
    # other pitches of the point buffer, and no clusters at all
    p3 = up(np.ascontiguousarray(one["pts"][:, :3]))
    assert xa.xalign_apply(p3, up(one["labels"]), info, v, pt_off, E, up(base), 0.1).cpu().numpy().tobytes() == out.tobytes()
    none = xa.xalign_apply(p3, up(np.zeros_like(one["labels"])), info[:0], v[:0], pt_off, E, up(base), 0.1).cpu().numpy()
    assert none.tobytes() == base.tobytes()


def ref_E(pose0, pose1):
    return np.ascontiguousarray((np.linalg.inv(pose1) @ pose0).astype(f32)[:3]).reshape(12)


# ---- the program ---------------------------------------------------------------------------------------------------------------------------------
def test_program_writes_the_restatements_flow(gpu, tmp_path, monkeypatch, capsys):
    from himo_amd import xalign as xa
    from himo_amd.dataset import NpzDataset
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    frames = []
    for s, (scene, stamp, speeds) in enumerate((("a", 10, [0.0, 12.0, 25.0]), ("a", 11, [35.0]), ("b", 10, [0.2, 18.0]))):
        d = xs.drive(seed=80 + s, speeds=speeds, points=660)
        ids = np.array([0, 900, 17, 5_000_000][:len(speeds) + 1], np.uint32)[d["labels"]]
        ids[:7] = 0
        tau = (d["dt"].max() - d["dt"]).astype(f32)
        d["raw"][np.flatnonzero(d["labels"] == len(speeds))[-2:], [0, 2]] = [np.nan, np.inf]      # two rows of the last vehicle are not finite
        frames.append({"scene_id": scene, "timestamp": stamp, "pc0": np.concatenate([d["raw"], np.ones((len(ids), 1), f32)], axis=1),
                       "pose0": pose(s), "pose1": pose(s + 1), "lidar_dt": tau, "lidar_id": d["group"], "est": d["motion"], "ids": ids})
    root = tmp_path / "d"
    NpzDataset.write(root, frames)
    out = tmp_path / "x.json"
    numbers = xa._cli(["--data_dir", str(root), "--label_key", "ids", "--batch", "2", "--json", str(out)])
    assert json.loads(out.read_text()) == json.loads(json.dumps(numbers))
    printed = capsys.readouterr().out
    assert "xalign (cross-sensor alignment, v1; parity unpinned)" in printed and "aligned by speed" in printed and "mean iterations" in printed

    def expect(f, base):
        uniq, compact = np.unique(f["ids"], return_inverse=True)     # 0 first: it is there in every sweep
        res = ref.estimate(f["pc0"], compact.astype(np.int32), f["lidar_id"], f["lidar_dt"], len(uniq) - 1)
        return res, ref.apply(f["pc0"], compact, res[0], res[1], ref_E(f["pose0"], f["pose1"]), base)
    states, by_speed, moved = [0] * 7, {b: 0 for b in xa.SPEED_BUCKETS}, 0
    for f in frames:
        (info, v, _), flow = expect(f, None)
        with np.load(root / f["scene_id"] / f"{f['timestamp']}.npz") as z:
            assert sorted(z.files) == sorted([k for k in f if k not in ("scene_id", "timestamp")] + ["xalign"])
            assert z["xalign"].dtype == f32 and z["xalign"].tobytes() == flow.tobytes()
        for st in info[:, 0]:
            states[st] += 1
        for c in np.flatnonzero(info[:, 0] == ref.ALIGNED):
            by_speed[xa.speed_bucket(float(v[c, 3]))] += 1
            moved += int(((f["ids"] == np.unique(f["ids"])[c + 1]) & np.isfinite(f["pc0"][:, :3]).all(axis=1)).sum())      # rule G: finite rows only
    assert numbers["totals"]["states"] == states and states[ref.ALIGNED] >= 3 and states[ref.ALIGNED] < 6
    assert numbers["speed"] == by_speed and numbers["points_moved"] == moved and moved % 660 and numbers["sweeps"] == 3 and numbers["points"] == 6 * 660
    assert numbers["mean_X1"] < numbers["mean_X0"] and 0 < numbers["ratio"] < 1 and numbers["mean_iters"] >= 1
    # a stored base under another key; a second run is refused without --overwrite and replaces the key with it
    with pytest.raises(FileExistsError, match="--overwrite"):
        xa._cli(["--data_dir", str(root), "--label_key", "ids"])
    xa._cli(["--data_dir", str(root), "--label_key", "ids", "--base", "est", "--out_name", "est_xalign", "--batch", "3"])
    xa._cli(["--data_dir", str(root), "--label_key", "ids", "--base", "est", "--overwrite"])
    for f in frames:
        flow = expect(f, f["est"])[1]
        with np.load(root / f["scene_id"] / f"{f['timestamp']}.npz") as z:
            assert z["est_xalign"].tobytes() == flow.tobytes() and z["xalign"].tobytes() == flow.tobytes() and z["est"].tobytes() == f["est"].tobytes()


def test_program_clusters_for_itself(gpu, tmp_path, monkeypatch):
    """``--label_key cluster``: the labels are a clustering of the sweep's own points, as in ``eval_xsensor``"""
    import torch
    from himo_amd import xalign as xa
    from himo_amd.dataset import NpzDataset
    from himo_amd.seflow.ssl_label import EPS, MIN_PTS, cluster_points
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    d = xs.drive(seed=90, speeds=[0.0, 20.0, 30.0], points=900)
    pc0 = d["raw"] + np.array([45.0, 60.0, 0.0], f32)
    f = {"scene_id": "c", "timestamp": 20, "pc0": pc0, "pose0": np.eye(4), "pose1": np.eye(4), "lidar_dt": (d["dt"].max() - d["dt"]).astype(f32),
         "lidar_id": d["group"], "gm0": np.zeros(len(pc0), bool)}
    NpzDataset.write(tmp_path / "d", [f])
    numbers = xa.main(str(tmp_path / "d"), "cluster")
    labels, count = cluster_points(torch.from_numpy(pc0).to(gpu), torch.zeros(len(pc0), dtype=torch.bool, device=gpu), "dbscan", EPS, MIN_PTS)
    info, v, _ = ref.estimate(pc0, labels.cpu().numpy(), f["lidar_id"], f["lidar_dt"], int(count))
    flow = ref.apply(pc0, labels.cpu().numpy(), info, v, np.eye(4, dtype=f32)[:3].reshape(12))
    with np.load(tmp_path / "d" / "c" / "20.npz") as z:
        assert z["xalign"].tobytes() == flow.tobytes()
    assert numbers["totals"]["states"] == [int((info[:, 0] == s).sum()) for s in range(7)] and numbers["states"]["aligned"] >= 1
