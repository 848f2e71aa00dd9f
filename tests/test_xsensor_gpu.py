"""Cross-sensor consistency on the GPU: ``himo_xsensor`` against the numpy restatement of the rule (tests/xsensor_ref.py) at the sizes
and inputs where the kernels take another path.  ``info``, ``rec``, ``mot`` and the per-row ``m`` match bit for bit: every sum of the
rule is an integer sum and the minimum is order-free.  Small sweeps: every case is a few thousand rows, the one cluster above
``max_points`` apart."""
import ctypes
import functools
import json

import numpy as np
import pytest

import xsensor_ref as ref

pytestmark = pytest.mark.gpu

CHUNK = 1024                                    # HIMO_XSENSOR_CHUNK: the rows the search stages in LDS at a time
MAX_POINTS = ref.DEFAULTS["max_points"]


def sweep(sizes, seed, groups=(1, 2), loose=200, shuffle=True, width=4, spread=2.0):
    """clusters of the given sizes (label i + 1) about a grid of centres, their rows dealt to ``groups`` in turn, ``loose`` rows of label
    0 among them, rows in random order -> dict(pts float32 [N, width], labels int32, group uint8, dt float32, motion float32 [N, 3])"""
    rng = np.random.default_rng(seed)
    pts, labels, group = [], [], []
    for i, n in enumerate(sizes):
        centre = np.array([-40.0 + 12.0 * (i % 8), -40.0 + 12.0 * (i // 8), 0.0])
        pts.append(rng.normal(0, spread, (n, 3)) + centre)
        labels.append(np.full(n, i + 1, np.int32))
        group.append(np.asarray(groups, np.uint8)[np.arange(n) % len(groups)])
    pts.append(rng.uniform(-50, 50, (loose, 3)))
    labels.append(np.zeros(loose, np.int32))
    group.append(rng.integers(0, 8, loose).astype(np.uint8))
    pts, labels, group = np.concatenate(pts), np.concatenate(labels), np.concatenate(group)
    pts = np.concatenate([pts, rng.uniform(0, 1, (len(pts), width - 3))], axis=1).astype(np.float32)
    order = rng.permutation(len(pts)) if shuffle else np.arange(len(pts))
    pts, labels, group = pts[order], labels[order], group[order]
    dt = (np.float32(0.011) * group.astype(np.float32) + rng.uniform(0, 0.002, len(pts)).astype(np.float32)).astype(np.float32)
    motion = (rng.normal(0, 0.3, (len(pts), 3)) + np.array([1.5, -0.7, 0.0])).astype(np.float32)
    return dict(pts=pts, labels=labels, group=group, dt=dt, motion=motion)


def device_score(gpu, d, C, dt=True, motion=True, rows=True, pts=None, **params):
    """(info, rec, mot, m) host copies of one ``himo_xsensor`` call on the current stream (``m`` None without ``rows``)"""
    import torch
    from himo_amd import eval_xsensor as ex
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)                  # noqa: E731
    p = up(d["pts"]) if pts is None else pts
    info, rec, mot, got = ex.xsensor_labelled(p, up(d["labels"]), up(d["group"]), C, ex.XSensorParams(**params), up(d["dt"]) if dt else None,
                                              up(d["motion"]) if motion else None, want_rows=rows)
    return info.cpu().numpy(), rec.cpu().numpy(), mot.cpu().numpy(), (got[0].cpu().numpy() if rows else None)


def want(d, C, dt=True, motion=True, **params):
    return ref.score(d["pts"], d["labels"], d["group"], C, dt=d["dt"] if dt else None, motion=d["motion"] if motion else None, **params)


def same(got, expect, what=""):
    for name, a, b in zip(("info", "rec", "mot", "m"), got, expect):
        if a is None:
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), bad[:5], a[bad[:1]], b[bad[:1]]))


# ---- cluster sizes: wave, query-tile and chunk edges ---------------------------------------------------------------------------------------
SIZES = (1, 9, 10, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, MAX_POINTS + 1)


@functools.lru_cache(maxsize=None)
def sizes_case():
    d = sweep(SIZES, seed=11)
    return d, want(d, len(SIZES))


def test_cluster_sizes_at_the_wave_tile_and_chunk_edges(gpu):
    d, expect = sizes_case()
    assert expect[0][:, 0].tolist() == [ref.TOO_FEW] * 2 + [ref.SCORED] * 11 + [ref.TOO_LARGE] and expect[0][:, 1].tolist() == list(SIZES)
    assert (expect[0][2:13, 3] == SIZES[2:13]).all() and (expect[2][2:13, 0] == SIZES[2:13]).all()
    got = device_score(gpu, d, len(SIZES))
    same(got, expect)
    again = device_score(gpu, d, len(SIZES))                        # a call repeated gives the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("dt,motion,rows", [(False, False, False), (True, False, True), (False, True, False), (False, False, True)])
def test_with_and_without_dt_motion_and_rows(gpu, dt, motion, rows):
    d, _ = sizes_case()
    keep = d["labels"] != len(SIZES)                                 # (without the large cluster: the restatement is made four times)
    d = {k: v[keep] for k, v in d.items()}
    C = len(SIZES) - 1
    expect = want(d, C, dt=dt, motion=motion)
    assert (expect[1][:, :, 1] != 0).any() == dt and (expect[2] != 0).any() == motion
    same(device_score(gpu, d, C, dt=dt, motion=motion, rows=rows), expect)


# ---- group layouts ---------------------------------------------------------------------------------------------------------------------------
def test_group_layouts(gpu):
    rng = np.random.default_rng(21)
    d = sweep((300, 400, 300, 200, 2500), seed=21, shuffle=False, loose=50)
    lab, group = d["labels"], d["group"]
    group[lab == 2] = np.arange(400) % 8                             # eight groups
    group[lab == 3] = np.where(np.arange(300) < 4, 5, 0)             # one live and one thin group
    group[lab == 4] = 7                                              # all rows of one sensor
    last = np.zeros(2500, np.uint8)
    last[-40:] = 3                                                   # a live group whose rows all sit in the last chunk
    group[lab == 5] = last
    expect = want(d, 5)
    assert expect[0][:, 0].tolist() == [ref.SCORED, ref.SCORED, ref.ONE_SENSOR, ref.ONE_SENSOR, ref.SCORED]
    assert expect[0][:, 2].tolist() == [0b110, 0xff, 0, 0, 0b1001] and expect[0][4, 3] == 2500
    same(device_score(gpu, d, 5), expect)
    order = rng.permutation(len(lab))                                # rows in random order: the same clusters, the same integers
    shuffled = {k: v[order] for k, v in d.items()}
    got = device_score(gpu, shuffled, 5)
    same(got[:3], expect[:3])
    same(got, want(shuffled, 5))
    # min_group at its edge: with 41 the group of 40 is not live
    same(device_score(gpu, d, 5, min_group=41), want(d, 5, min_group=41))
    assert want(d, 5, min_group=41)[0][4, 0] == ref.ONE_SENSOR


def test_labels_outside_pitch_ties_and_non_finite_rows(gpu):
    import torch
    rng = np.random.default_rng(31)
    d = sweep((150, 90, 700, 33), seed=31, groups=(0, 4, 7), width=7)
    d["pts"][:, :3] = np.round(d["pts"][:, :3] * 2) / 2               # a 0.5 m lattice: exact ties and coincident points of two sensors
    d["labels"][rng.choice(len(d["labels"]), 30, replace=False)] = rng.choice([-3, 5, 1 << 30], 30)       # labels outside 1..C
    bad = rng.choice(len(d["labels"]), 60, replace=False)
    d["pts"][bad[:30], rng.integers(0, 3, 30)] = rng.choice([np.nan, np.inf, -np.inf], 30)
    d["group"][bad[30:40]] = rng.choice([8, 9, 255], 10)
    d["dt"][bad[40:50]] = rng.choice([np.nan, np.inf], 10)
    d["motion"][bad[50:], rng.integers(0, 3, 10)] = np.nan
    d["pts"][rng.choice(len(d["labels"]), 5, replace=False), 0] = [3e38, -3e38, 3e38, -3e38, 1e30]           # d2 overflows: +inf clips
    expect = want(d, 4)
    assert (expect[3] == 0).any() and (expect[0][:, 0] == ref.SCORED).all() and (expect[0][:, 1] <= [150, 90, 700, 33]).all() and (expect[0][:, 1] < [150, 90, 700, 33]).any()
    assert (expect[2][:, 0] < expect[0][:, 1]).any()
    wide = torch.from_numpy(d["pts"]).to(gpu)
    same(device_score(gpu, d, 4, pts=wide), expect, "pitch 7")
    same(device_score(gpu, d, 4, pts=wide[:, :4].contiguous()), expect, "pitch 4")
    same(device_score(gpu, d, 4, pts=wide[:, 2:]), want(dict(d, pts=d["pts"][:, 2:]), 4), "a view at pitch 7")
    same(device_score(gpu, d, 4, near=0.5, trunc=1.0, min_points=33, max_points=699),
         want(d, 4, near=0.5, trunc=1.0, min_points=33, max_points=699), "near and trunc on the lattice")


def test_many_small_clusters_in_one_call(gpu):
    d = sweep((12,) * 2000, seed=41, loose=500, spread=0.5)
    expect = want(d, 2000, min_group=3)
    assert (expect[0][:, 0] == ref.SCORED).all() and (expect[0][:, 3] == 12).all()
    same(device_score(gpu, d, 2000, min_group=3), expect)
    info = device_score(gpu, d, 2100, min_group=3, rows=False)[0]   # clusters without rows after the last one that has any
    assert info[:2000].tobytes() == expect[0].tobytes() and (info[2000:] == [ref.TOO_FEW, 0, 0, 0]).all()


def test_sweeps_and_names_concatenated_equal_the_calls_one_by_one(gpu):
    parts = [sweep((40, 300, 1100), seed=51), sweep((500, 20, 64, 9), seed=52), sweep((257,), seed=53)]
    moved = []
    for k, d in enumerate(parts):                                    # a second "name": the same rows, points shifted per sensor
        shifted = d["pts"].copy()
        shifted[:, 0] += np.float32(0.05) * d["group"].astype(np.float32)
        moved.append(dict(d, pts=shifted))
    calls = parts + moved
    counts = [int(d["labels"].max()) for d in calls]
    base = np.concatenate([[0], np.cumsum(counts)])
    one = {k: np.concatenate([d[k] for d in calls]) for k in calls[0]}
    one["labels"] = np.concatenate([np.where(d["labels"] > 0, d["labels"] + b, 0) for d, b in zip(calls, base)]).astype(np.int32)
    info, rec, mot, m = device_score(gpu, one, int(base[-1]))
    singles = [device_score(gpu, d, c) for d, c in zip(calls, counts)]
    for name, whole, k in (("info", info, 0), ("rec", rec, 1), ("mot", mot, 2), ("m", m, 3)):
        assert whole.tobytes() == np.concatenate([s[k] for s in singles]).tobytes(), name
    same((info, rec, mot, m), want(one, int(base[-1])))
    assert (info[:counts[0], 0] == ref.SCORED).all() and not np.array_equal(rec[:3, :, 2], rec[base[3]:base[3] + 3, :, 2])


def test_scorer_compacts_arbitrary_ids(gpu):
    from himo_amd.eval_xsensor import XSensor
    d = sweep((40, 300, 25), seed=61)
    ids = np.array([0, 7, 1 << 33, 4_000_000_000], np.int64)[d["labels"]]
    res = XSensor(gpu).score(d["pts"], ids, d["group"], d["dt"], d["motion"], want_rows=True)
    assert res.ids.tolist() == [7, 4_000_000_000, 1 << 33]
    relabel = np.array([0, 1, 3, 2], np.int32)[d["labels"]]
    expect = ref.score(d["pts"], relabel, d["group"], 3, dt=d["dt"], motion=d["motion"])
    same((res.info, res.rec, res.mot, res.device_rows[0].cpu().numpy()), expect)
    mine = ref.glue(*expect[:3])
    for k, v in res.glue.items():
        assert np.array_equal(v, mine[k], equal_nan=True), k
    empty = XSensor(gpu).score(np.zeros((0, 3), np.float32), np.zeros(0, np.int64), np.zeros(0, np.uint8))
    assert empty.info.shape == (0, 4) and empty.rec.shape == (0, 8, 4)
    none = XSensor(gpu).score(d["pts"], np.zeros(len(ids), np.int64), d["group"])
    assert none.info.shape == (0, 4) and none.ids.shape == (0,)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_refusals_leave_poisoned_outputs_untouched(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.eval_xsensor import XSensorParams
    lib = _lib.load()
    d = sweep((40, 30), seed=71, loose=10)
    n, C = len(d["labels"]), 2
    order, off = ref.sort_rows(d["labels"], C)
    nc = len(order)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)                  # noqa: E731
    pts, labels, group, dt, motion, rows, d_off = (up(d["pts"]), up(d["labels"]), up(d["group"]), up(d["dt"]), up(d["motion"]), up(order), up(off))
    info = torch.full((C, 4), 7, dtype=torch.int32, device=gpu)
    rec = torch.full((C, 8, 4), 7, dtype=torch.int64, device=gpu)
    mot = torch.full((C, 2), 7, dtype=torch.int64, device=gpu)
    m = torch.full((nc,), 7.0, dtype=torch.float32, device=gpu)
    ws = torch.zeros(int(lib.himo_xsensor_workspace_bytes(nc, C)) + 16, dtype=torch.uint8, device=gpu)
    prm = XSensorParams().c_struct()
    P = _lib.ptr

    def call(**kw):
        a = dict(n=n, pts=P(pts), pitch=4, labels=P(labels), group=P(group), dt=P(dt), motion=P(motion), nc=nc, rows=P(rows), C=C,
                 h_off=off.ctypes.data, d_off=P(d_off), prm=ctypes.addressof(prm), info=P(info), rec=P(rec), mot=P(mot), m=P(m), ws=P(ws),
                 ws_bytes=ws.numel() - 16)
        a.update(kw)
        with torch.cuda.device(gpu):
            return lib.himo_xsensor(a["n"], a["pts"], a["pitch"], a["labels"], a["group"], a["dt"], a["motion"], a["nc"], a["rows"], a["C"],
                                    a["h_off"], a["d_off"], a["prm"], a["info"], a["rec"], a["mot"], a["m"], a["ws"], a["ws_bytes"],
                                    _lib.stream_handle())
    bad_off = [np.array(v, np.int64) for v in ([1, 40, nc], [0, 40, nc - 1], [0, 41, 40], [0, -1, nc])]
    bad_prm = [XSensorParams().c_struct() for _ in range(8)]
    bad_prm[0].trunc, bad_prm[1].trunc, bad_prm[2].near, bad_prm[3].near = 0.0, float("nan"), -1.0, float("inf")
    bad_prm[4].min_group, bad_prm[5].min_points, bad_prm[6].max_points, bad_prm[7].max_points = 0, 1, 9, (1 << 20) + 1
    invalid = [dict(n=-1), dict(nc=-1), dict(nc=n + 1), dict(C=-1), dict(pitch=2), dict(prm=None), dict(h_off=None), dict(d_off=None),
               dict(info=None), dict(rec=None), dict(mot=None), dict(pts=None), dict(labels=None), dict(group=None), dict(rows=None),
               dict(pts=P(pts) + 2), dict(rec=P(rec) + 4), dict(rows=P(rows) + 4), dict(dt=P(dt) + 1), dict(m=P(m) + 2), dict(C=0)]
    invalid += [dict(h_off=o.ctypes.data) for o in bad_off] + [dict(prm=ctypes.addressof(q)) for q in bad_prm]
    for kw in invalid:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(n=2 ** 31) == _lib.ERR_UNSUPPORTED
    for kw in (dict(ws=None), dict(ws=P(ws) + 8), dict(ws_bytes=64)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    assert call(n=0, nc=0, C=0) == _lib.OK
    torch.cuda.synchronize(gpu)
    assert (info == 7).all() and (rec == 7).all() and (mot == 7).all() and (m == 7).all() and not ws.any()       # nothing was written
    assert call() == _lib.OK                                         # ... and the same buffers take the call that is admitted
    torch.cuda.synchronize(gpu)
    same((info.cpu().numpy(), rec.cpu().numpy(), mot.cpu().numpy(), m.cpu().numpy()), want(d, C))


# ---- the program ---------------------------------------------------------------------------------------------------------------------------------
def test_program_totals_equal_the_restatement(gpu, tmp_path, monkeypatch):
    import torch
    from himo_amd import eval_xsensor as ex
    from himo_amd.accumulate import flow_motion
    from himo_amd.compdis import CompDisEngine
    from himo_amd.dataset import NpzDataset
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    frames = []
    for s, (scene, stamp, speeds) in enumerate((("a", 10, [0.0, 12.0, 25.0]), ("a", 11, [35.0, 4.0]), ("b", 10, [0.2, 18.0]), ("b", 11, [8.0]))):
        d = ref.drive(seed=80 + s, speeds=speeds, points=240)
        ids = np.array([0, 900, 17, 5_000_000][:len(speeds) + 1], np.uint32)[d["labels"]]
        ids[:7] = 0
        frames.append({"scene_id": scene, "timestamp": stamp, "pc0": np.concatenate([d["raw"], np.ones((len(ids), 1), np.float32)], axis=1),
                       "pose0": np.eye(4), "pose1": np.eye(4), "lidar_dt": d["dt"], "lidar_id": d["group"], "est": d["motion"], "ids": ids})
    NpzDataset.write(tmp_path / "d", frames)
    out = tmp_path / "x.json"
    numbers = ex._cli(["--data_dir", str(tmp_path / "d"), "--res_names", "raw,est", "--label_key", "ids", "--against", "raw", "--batch", "3",
                       "--json", str(out)])
    assert json.loads(out.read_text()) == json.loads(json.dumps(numbers))
    for f in frames:
        with np.load(tmp_path / "d" / f["scene_id"] / f"{f['timestamp']}.npz") as z:
            assert sorted(z.files) == sorted(k for k in f if k not in ("scene_id", "timestamp"))       # nothing was written into the scenes

    # the same numbers from the restatement, sweep by sweep
    engine = CompDisEngine()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)                  # noqa: E731
    expect = {name: {"states": [0] * 4, "all": [0, 0, 0, 0, 0.0], "speed": {}} for name in ("raw", "est")}
    pairs, sums = 0, [0.0, 0.0]
    for f in frames:
        uniq, compact = np.unique(f["ids"], return_inverse=True)     # 0 first: it is there in every sweep
        motion = flow_motion(up(f["pc0"]), up(f["est"]), f["pose0"], f["pose1"]).cpu().numpy()
        comp = engine.run_frame(up(f["pc0"]), up(f["est"]), up(f["lidar_dt"]), f["pose0"], f["pose1"], refined=True)[1].cpu().numpy()
        X = {}
        for name, pts in (("raw", f["pc0"][:, :3]), ("est", comp)):
            info, rec, mot, _ = ref.score(pts, compact.astype(np.int32), f["lidar_id"], len(uniq) - 1, dt=f["lidar_dt"], motion=motion)
            g = ref.glue(info, rec, mot)
            e = expect[name]
            for st in info[:, 0]:
                e["states"][st] += 1
            for c in np.flatnonzero(info[:, 0] == ref.SCORED):
                add = [1, int(info[c, 3]), int(rec[c, :, 2].sum()), int(rec[c, :, 3].sum()), float(g["X"][c])]
                e["all"] = [a + b for a, b in zip(e["all"], add)]
                v = g["speed"][c]
                key = "static" if v < 0.5 else "0-10" if v < 10 else "10-20" if v < 20 else "20-30" if v < 30 else "30+"
                e["speed"][key] = e["speed"].get(key, 0) + 1
            X[name] = np.where(info[:, 0] == ref.SCORED, g["X"], np.nan)
        both = ~np.isnan(X["raw"]) & ~np.isnan(X["est"])
        pairs += int(both.sum())
        sums = [sums[0] + float(X["est"][both].sum()), sums[1] + float(X["raw"][both].sum())]
    assert sum(expect["raw"]["states"]) == 8 and expect["raw"]["all"][0] >= 6 and len(expect["raw"]["speed"]) >= 4
    for name in ("raw", "est"):
        t = numbers[name]["totals"]
        assert t["states"] == expect[name]["states"], name
        b = t["buckets"]["all"]
        assert [b["clusters"], b["queries"], b["sum_qc"], b["near"]] == expect[name]["all"][:4], name
        assert abs(b["sum_X"] - expect[name]["all"][4]) <= 1e-12 * expect[name]["all"][4]
        assert {k: t["buckets"][f"speed:{k}"]["clusters"] for k in ex.SPEED_BUCKETS if t["buckets"][f"speed:{k}"]["clusters"]} == expect[name]["speed"]
        assert sum(t["buckets"][f"dt:{k}"]["clusters"] for k in ex.DT_BUCKETS) == b["clusters"]
    a = numbers["est"]["against"]
    assert a["name"] == "raw" and a["buckets"]["all"]["pairs"] == pairs and abs(a["buckets"]["all"]["ratio"] - sums[0] / sums[1]) <= 1e-12
    assert numbers["raw"]["against"]["buckets"]["all"]["ratio"] == 1.0


def test_program_clusters_for_itself(gpu, tmp_path, monkeypatch):
    """``--label_key cluster``: the labels are a clustering of every name's own points (here ``raw`` alone), as in ``box_fit``"""
    import torch
    from himo_amd import eval_xsensor as ex
    from himo_amd.dataset import NpzDataset
    from himo_amd.seflow.ssl_label import EPS, MIN_PTS, cluster_points
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    frames = []
    for s in range(2):
        d = ref.drive(seed=90 + s, speeds=[0.0, 20.0, 30.0], points=900)
        pc0 = d["raw"] + np.array([45.0, 60.0, 0.0], np.float32)
        frames.append({"scene_id": "c", "timestamp": 20 + s, "pc0": pc0, "pose0": np.eye(4), "pose1": np.eye(4), "lidar_dt": d["dt"],
                       "lidar_id": d["group"], "gm0": np.zeros(len(pc0), bool)})
    NpzDataset.write(tmp_path / "d", frames)
    numbers = ex.main(str(tmp_path / "d"), "raw", "cluster")
    states, total = [0] * 4, [0, 0, 0]
    for f in frames:
        labels, count = cluster_points(torch.from_numpy(f["pc0"]).to(gpu), torch.zeros(len(f["pc0"]), dtype=torch.bool, device=gpu), "dbscan", EPS, MIN_PTS)
        info, rec, _, _ = ref.score(f["pc0"], labels.cpu().numpy(), f["lidar_id"], int(count), dt=f["lidar_dt"])
        for st in info[:, 0]:
            states[st] += 1
        sc = info[:, 0] == ref.SCORED
        total = [total[0] + int(info[sc, 3].sum()), total[1] + int(rec[sc][:, :, 2].sum()), total[2] + int(rec[sc][:, :, 3].sum())]
    t = numbers["raw"]["totals"]
    assert states[ref.SCORED] >= 6 and t["states"] == states
    assert [t["buckets"]["all"][k] for k in ("queries", "sum_qc", "near")] == total
    assert list(t["buckets"]) == ex.bucket_keys(False) and "against" not in numbers["raw"]      # no stored name: no motion, no speed buckets
