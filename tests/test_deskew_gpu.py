"""Ego de-skew on the GPU against the restatement of its rule (tests/deskew_ref.py): the two entry points called directly over the
shapes, layouts, modes and twists at which the kernel can go wrong (every coordinate within one float32 ulp, counts and t_ref exact),
run-to-run identity, every refusal, the round trip on the device, the program end to end on scene files, and the chain
``odometry -> deskew`` on a skewed drive."""
import ctypes

import numpy as np
import pytest

import deskew_ref as ref

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
SENTINEL = 0xAB
SINGLE = [(0,), (1,), (63,), (64,), (65,), (257,), (1025,)]
BATCHES = [(0, 65), (257, 63), (0, 257, 1, 65, 1025), (64, 1, 0, 300, 63), (1025, 65, 63, 7, 0)]
LAYOUTS = [(3, 3, False), (3, 4, False), (4, 3, False), (4, 4, False), (3, 3, True), (4, 4, True)]      # in pitch, out pitch, in place
TWISTS = [
    [0, 0, 0, 0, 0, 0],                                          # zero: every row passes through
    [1.0, -0.2, 0.05, 0, 0, 0],                                  # pure translation
    [1.0, 0.2, -0.1, 0.0, 6e-10, 8e-10],                         # theta 1e-9: the first-order form
    [1.0, 0.1, 0.02, 0.0, 0.0, 7e-3],                            # a drive's yaw
    [0.8, -0.3, 0.2, 0.0, 0.0, 0.5],
    [1.1, 0.3, -0.2, 0.12, -0.2, 0.15],                          # an axis off z
]


@pytest.fixture(scope="module")
def eng(gpu):
    from himo_amd.deskew import EgoDeskew
    return EgoDeskew(gpu)


def _sweep(n, pitch, seed):
    """n rows inside +-64 m with lidar_dt in [-0.02, 0.1]: the corners of the range, rows at the reference time, non-finite rows"""
    rng = np.random.default_rng(7919 * n + 13 * pitch + seed)
    p = rng.uniform(-64, 64, (n, pitch)).astype(f32)
    if pitch == 4:
        p[:, 3] = rng.uniform(0, 1, n)
    dt = rng.uniform(-0.02, 0.1, n).astype(f32)
    if n >= 63:
        p[0, :3], p[1, :3] = (64, -64, 64), (-64, 64, -64)
        p[2, 0], p[3, 1], p[4, 2] = np.nan, np.inf, -np.inf
        dt[5], dt[6] = np.nan, -np.inf
        dt[7] = dt[8] = dt[np.isfinite(dt)].max()               # s == 0 under "max", twice
        dt[9] = dt[np.isfinite(dt)].min()                       # and under "min"
        dt[10] = 0.0                                            # and under "zero"
        p[7, 1] = p[10, 0] = f32(-0.0)
    return p, dt


def _twists(B, seed, span=0.1):
    tw = np.zeros((B, 8))
    for b in range(B):
        tw[b, :6] = TWISTS[(b + seed) % len(TWISTS)]
    tw[:, 6] = span
    return tw


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _call(eng, gpu, pts, dts, tw, ref_mode, inverse, out_pitch, in_place):
    """himo_deskew_tref + himo_deskew_rows, called directly: (out [n, out_pitch], counts [B, 2], max_disp [B], t_ref [B])"""
    import torch
    from himo_amd import _lib
    from himo_amd.sweeps import sweep_offsets
    lib, P = eng.lib, _lib.ptr
    B = len(pts)
    pitch = pts[0].shape[1] if B else 3
    h_off = sweep_offsets([len(p) for p in pts])
    n = int(h_off[-1])
    cat = _dev(np.concatenate(pts) if B else np.zeros((0, pitch), f32), gpu)
    dt = _dev(np.concatenate(dts) if B else np.zeros(0, f32), gpu)
    d_off, d_tw = _dev(h_off, gpu), _dev(tw, gpu)
    out = cat if in_place else torch.full((n, out_pitch), -7.0, dtype=torch.float32, device=gpu)
    counts = torch.full((B, 2), -7, dtype=torch.int32, device=gpu)
    disp = torch.full((B,), -7.0, dtype=torch.float32, device=gpu)
    tref = torch.full((B,), -7.0, dtype=torch.float32, device=gpu)
    s = _lib.stream_handle()
    N = lambda t, have: P(t) if have else None                  # noqa: E731
    assert lib.himo_deskew_tref(B, n, h_off.ctypes.data, N(d_off, True), N(dt, n), ref_mode, N(tref, B), s) == 0
    assert lib.himo_deskew_rows(B, n, h_off.ctypes.data, N(d_off, True), N(cat, n), pitch, N(dt, n), tw.ctypes.data if B else None, N(d_tw, B),
                                N(tref, B), int(inverse), N(out, n), out_pitch, N(counts, B), N(disp, B), s) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), counts.cpu().numpy(), disp.cpu().numpy(), tref.cpu().numpy()


def _within_one_ulp(got, want):
    """(all values bit-identical or finite and one float32 step apart at most, how many are not bit-identical)"""
    same = got.view(np.uint32) == want.view(np.uint32)
    g, w = got[~same], want[~same]
    with np.errstate(all="ignore"):
        ok = np.isfinite(g) & np.isfinite(w) & (np.abs(g.astype(f64) - w.astype(f64)) <= np.maximum(np.spacing(np.abs(g)), np.spacing(np.abs(w))))
    return bool(ok.all()), int((~same).sum())


def _check(eng, gpu, sizes, seed, layouts=LAYOUTS, refs=ref.REFS, inverses=(False, True)):
    flipped = values = 0
    for pin, pout, in_place in layouts:
        made = [_sweep(n, pin, seed + b) for b, n in enumerate(sizes)]
        pts, dts = [m[0] for m in made], [m[1] for m in made]
        tw = _twists(len(sizes), seed)
        for ref_name in refs:
            for inverse in inverses:
                out, counts, disp, tref = _call(eng, gpu, pts, dts, tw, ref.REFS.index(ref_name), inverse, pout, in_place)
                at = 0
                for b, (p, d) in enumerate(zip(pts, dts)):
                    want, wc, wd, wt = ref.deskew(p, d, tw[b], ref_name, inverse)
                    got = out[at:at + len(p)]
                    at += len(p)
                    assert tref[b].tobytes() == wt.tobytes(), (sizes, b, ref_name)          # t_ref: exact
                    assert counts[b].tolist() == wc.tolist(), (sizes, b, ref_name, inverse)
                    ok, n_diff = _within_one_ulp(np.ascontiguousarray(got[:, :3]), np.ascontiguousarray(want[:, :3]))
                    assert ok, (sizes, b, pin, pout, ref_name, inverse)
                    flipped, values = flipped + n_diff, values + 3 * len(p)
                    ok, _ = _within_one_ulp(disp[b:b + 1], np.array([wd], f32))
                    assert ok, (disp[b], wd)
                    if pout == 4:                                # column 3: copied, 0 where the input has none
                        assert got[:, 3].tobytes() == (p[:, 3] if pin == 4 else np.zeros(len(p), f32)).tobytes()
                    with np.errstate(all="ignore"):              # rows at the reference time, non-finite rows, a zero twist: their bytes
                        stay = ~(np.isfinite(p[:, :3]).all(axis=1) & np.isfinite(d)) | ((f64(wt) - d.astype(f64)) / tw[b, 6] == 0.0)
                    stay |= not tw[b, :6].any()
                    assert int(stay.sum()) == wc[1] and got[stay, :3].tobytes() == p[stay, :3].tobytes()
                assert at == len(out)
    return flipped, values


@pytest.mark.parametrize("sizes", SINGLE + BATCHES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement(eng, gpu, sizes):
    flipped, values = _check(eng, gpu, sizes, seed=len(sizes))
    print(f"sweeps {sizes}: {flipped} of {values} output values are not bit-identical to the restatement's (all within 1 float32 ulp)")


def test_every_twist_on_one_sweep_size(eng, gpu):
    for seed in range(len(TWISTS)):
        flipped, values = _check(eng, gpu, (257,), seed, layouts=[(4, 4, False), (3, 3, True)])
        print(f"twist {TWISTS[seed]}: {flipped} of {values} values not bit-identical")


def test_no_sweeps(eng, gpu):
    out, counts, disp, tref = _call(eng, gpu, [], [], np.zeros((0, 8)), 0, False, 3, False)
    assert out.shape == (0, 3) and counts.shape == (0, 2) and disp.shape == (0,) and tref.shape == (0,)
    moved, counts, disp = eng.sweeps([], [], np.zeros((0, 8)))
    assert moved == [] and counts.shape == (0, 2) and disp.shape == (0,)


def test_rows_at_the_reference_time_keep_every_byte(eng, gpu):
    """all lidar_dt equal: s == 0 for every row, whatever the twist"""
    p, _ = _sweep(257, 4, 3)
    dt = np.full(257, 0.05, f32)
    for ref_mode, n_kept in ((0, 257), (1, 257)):
        out, counts, disp, tref = _call(eng, gpu, [p], [dt], _twists(1, 4), ref_mode, False, 4, False)
        assert out.tobytes() == p.tobytes() and counts.tolist() == [[0, n_kept]] and disp[0] == 0 and tref[0] == f32(0.05)
    # no finite lidar_dt: t_ref = 0 and every row passes through
    out, counts, disp, tref = _call(eng, gpu, [p], [np.full(257, np.nan, f32)], _twists(1, 4), 0, False, 4, False)
    assert out.tobytes() == p.tobytes() and counts.tolist() == [[0, 257]] and tref[0] == 0


def test_two_runs_give_identical_bytes(eng, gpu):
    sizes = (1025, 0, 257, 65)
    made = [_sweep(n, 4, 40 + b) for b, n in enumerate(sizes)]
    runs = [_call(eng, gpu, [m[0] for m in made], [m[1] for m in made], _twists(4, 3), 0, False, 4, False) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_the_class_equals_the_direct_calls(eng, gpu):
    sizes = (65, 0, 257)
    made = [_sweep(n, 4, 50 + b) for b, n in enumerate(sizes)]
    pts, dts, tw = [m[0] for m in made], [m[1] for m in made], _twists(3, 3)
    out, counts, disp, tref = _call(eng, gpu, pts, dts, tw, 0, False, 4, False)
    moved, c2, d2 = eng.sweeps(pts, dts, tw)
    assert np.concatenate([m.cpu().numpy() for m in moved]).tobytes() == out.tobytes()
    assert c2.tobytes() == counts.tobytes() and d2.tobytes() == disp.tobytes() and eng.t_ref.tobytes() == tref.tobytes()
    assert [tuple(m.shape) for m in moved] == [(n, 4) for n in sizes]
    with pytest.raises(ValueError, match="twists"):
        eng.sweeps(pts, dts, tw[:2])
    with pytest.raises(ValueError, match="span"):
        eng.sweeps(pts, dts, _twists(3, 3, span=0.0))
    with pytest.raises(ValueError, match="pitch"):
        eng.sweeps([pts[0], pts[2][:, :3]], dts[::2], tw[:2])
    with pytest.raises(ValueError, match="lidar_dt"):
        eng.sweeps(pts, [dts[0], dts[1], dts[2][:-1]], tw)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_write_nothing(eng, gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.sweeps import sweep_offsets
    lib, P = eng.lib, _lib.ptr
    INVALID, UNSUPPORTED = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    sizes = (65, 0, 300)
    made = [_sweep(n, 4, 60 + b) for b, n in enumerate(sizes)]
    B, n = len(sizes), sum(sizes)
    good_off, good_tw = sweep_offsets(sizes), _twists(B, 1)
    pts_host = np.concatenate([m[0] for m in made])
    cat, dt = _dev(pts_host, gpu), _dev(np.concatenate([m[1] for m in made]), gpu)
    d_off, d_tw = _dev(good_off, gpu), _dev(good_tw, gpu)
    out = torch.full(((n + 2) * 16,), SENTINEL, dtype=torch.uint8, device=gpu)
    counts = torch.full((B * 8 + 16,), SENTINEL, dtype=torch.uint8, device=gpu)
    disp = torch.full((B * 4 + 16,), SENTINEL, dtype=torch.uint8, device=gpu)
    tref = torch.full((B * 4 + 16,), SENTINEL, dtype=torch.uint8, device=gpu)
    keep = []

    def off(*v):
        keep.append(np.array(v, np.int64))
        return keep[-1].ctypes.data

    def twist(**kw):
        t = good_tw.copy()
        for k, v in kw.items():
            t[1, {"vx": 0, "wz": 5, "span": 6, "spare": 7}[k]] = v
        keep.append(t)
        return t.ctypes.data

    s = _lib.stream_handle()

    def rows(want, B_=B, n_=n, h_off=good_off.ctypes.data, d_off_=P(d_off), pts=P(cat), pin=4, dt_=P(dt), h_tw=good_tw.ctypes.data, d_tw_=P(d_tw),
             tref_=P(tref), inverse=0, out_=P(out), pout=4, counts_=P(counts), disp_=P(disp)):
        assert lib.himo_deskew_rows(B_, n_, h_off, d_off_, pts, pin, dt_, h_tw, d_tw_, tref_, inverse, out_, pout, counts_, disp_, s) == want

    def tr(want, B_=B, n_=n, h_off=good_off.ctypes.data, d_off_=P(d_off), dt_=P(dt), mode=0, tref_=P(tref)):
        assert lib.himo_deskew_tref(B_, n_, h_off, d_off_, dt_, mode, tref_, s) == want

    def both(want, **kw):
        rows(want, **kw)
        tr(want, **{k: v for k, v in kw.items() if k in ("B_", "n_", "h_off", "d_off_", "dt_", "tref_")})

    for pitch in (2, 5, 0, -3):
        rows(INVALID, pin=pitch)
        rows(INVALID, pout=pitch)
    both(INVALID, n_=-1)
    both(INVALID, B_=-1)
    both(INVALID, h_off=None)
    both(INVALID, h_off=off(1, 65, 65, n))                      # does not start at 0
    both(INVALID, h_off=off(0, 65, 64, n))                      # decreases
    both(INVALID, h_off=off(0, 65, 65, n - 1))                  # does not end at the row count
    both(INVALID, h_off=off(0, 65, 65, n + 1))
    both(INVALID, B_=0, h_off=off(0))                           # no sweeps but rows
    both(INVALID, d_off_=None)
    both(INVALID, d_off_=P(d_off) + 4)
    both(INVALID, dt_=None)
    both(INVALID, dt_=P(dt) + 2)
    both(INVALID, tref_=None)
    both(INVALID, tref_=P(tref) + 1)
    rows(INVALID, pts=None)
    rows(INVALID, pts=P(cat) + 2)
    rows(INVALID, out_=None)
    rows(INVALID, out_=P(out) + 3)
    rows(INVALID, h_tw=None)
    rows(INVALID, d_tw_=None)
    rows(INVALID, d_tw_=P(d_tw) + 4)
    rows(INVALID, counts_=None)
    rows(INVALID, counts_=P(counts) + 2)
    rows(INVALID, disp_=None)
    rows(INVALID, disp_=P(disp) + 1)
    for kw in (dict(vx=np.nan), dict(wz=np.inf), dict(span=np.nan), dict(span=np.inf), dict(span=0.0), dict(span=-0.1)):
        rows(INVALID, h_tw=twist(**kw))
    for mode in (-1, 3, 99):
        tr(INVALID, mode=mode)
    for inverse in (-1, 2):
        rows(INVALID, inverse=inverse)
    # overlapping in and out: unequal pitches over one buffer, and equal pitches shifted by a row
    rows(INVALID, out_=P(cat), pout=3)
    rows(INVALID, pts=P(out), pin=3, out_=P(out), pout=4)
    rows(INVALID, out_=P(cat) + 16)
    rows(INVALID, pts=P(out) + 16, out_=P(out))
    both(UNSUPPORTED, B_=1, n_=1 << 31, h_off=off(0, 1 << 31))
    torch.cuda.synchronize()
    for t in (out, counts, disp, tref):
        assert (t.cpu().numpy() == SENTINEL).all()
    assert cat.cpu().numpy().tobytes() == pts_host.tobytes()


# ---- the round trip on the device --------------------------------------------------------------------------------------------------------------
def test_round_trip_on_the_device(eng, gpu):
    """inverse (the skew), then forward: every row within 8e-6 m of where it started (two float32 roundings inside +-64 m)"""
    from himo_amd.deskew import twists_from_poses
    frames, _ = ref.drive("uniform", "random")
    tw = twists_from_poses(np.stack([f["pose0"] for f in frames]), "backward", 0.1)
    pts, dts = [f["pc0"] for f in frames], [f["lidar_dt"] for f in frames]
    skewed, c1, d1 = eng.sweeps(pts, dts, tw, inverse=True)
    back, c2, d2 = eng.sweeps(skewed, dts, tw)
    assert c1.tolist() == c2.tolist() and (c1[:, 0] > 7900).all()
    worst = max(float(ref.row_errors(b.cpu().numpy(), p).max()) for b, p in zip(back, pts))
    moved = np.mean([ref.row_errors(s.cpu().numpy(), p).mean() for s, p in zip(skewed, pts)])
    print(f"round trip: rows displaced {moved:.3f} m on average (max_disp {d1.max():.3f} m), back within {worst:.3g} m")
    assert moved > 0.1 and worst <= 8e-6
    # the device's skew is the restatement's skew
    for s, p, d, t in zip(skewed, pts, dts, tw):
        ok, _ = _within_one_ulp(np.ascontiguousarray(s.cpu().numpy()[:, :3]), np.ascontiguousarray(ref.deskew(p, d, t, "max", True)[0][:, :3]))
        assert ok


# ---- the program -------------------------------------------------------------------------------------------------------------------------------
def _groups(path):
    from himo_amd.dataset import _open_h5
    with _open_h5(path) as h:
        return {ts: {k: np.asarray(h[ts][k][()]) for k in h[ts].keys()} for ts in h.keys()}


def test_program_end_to_end(gpu, tmp_path, capsys):
    import json
    import pickle
    from himo_amd import deskew
    from himo_amd.dataset import NpzDataset
    from himo_amd.synthetic import make_scene, write_h5_scenes
    true = [make_scene(21 + s, 5, n_points=4000, n_instances=8, scene_id=f"drive{s}") for s in range(2)]
    scenes = [ref.skew_scene(fr) for fr in true]
    D, O, O2, BACK = tmp_path / "in", tmp_path / "out", tmp_path / "out2", tmp_path / "back"
    D.mkdir()
    index = write_h5_scenes(D, scenes)
    out = deskew.main(str(D), str(O), pose_key="pose", json_path=str(tmp_path / "deskew.json"), batch=3)
    text = capsys.readouterr().out
    assert "ego de-skew, v1; parity unpinned" in text and "drive0" in text and "drive1" in text and "passed through" in text
    assert json.loads((tmp_path / "deskew.json").read_text()) == out
    a = out["all"]
    print(a)
    assert a["scenes"] == 2 and a["sweeps"] == 10 and a["rows_moved"] + a["rows_passed"] == 10 * 4000 and a["rows_passed"] >= 10
    assert 0.3 < a["mean_max_disp_m"] <= a["max_disp_m"] < 2.0 and 6.0 <= a["mean_speed_mps"] <= 12.0 and a["mean_yaw_rate_dps"] <= 4.01
    assert f"{a['rows_moved']} rows moved" in text and f"{a['max_disp_m']:.4f}" in text
    with open(O / "index_total.pkl", "rb") as fh:
        assert pickle.load(fh) == sorted(index, key=lambda e: (e[0], int(e[1])))
    for fr_true, fr_skew in zip(true, scenes):
        sc = fr_true[0]["scene_id"]
        src, got = _groups(D / f"{sc}.h5"), _groups(O / f"{sc}.h5")
        assert sorted(got) == sorted(src)
        tw = ref.twists_from_poses(np.stack([f["pose0"] for f in fr_true]), "backward", 0.1)
        for k, (ft, fs) in enumerate(zip(fr_true, fr_skew)):
            ts = str(ft["timestamp"])
            assert sorted(got[ts]) == sorted(list(src[ts]) + ["deskew"])
            for name in src[ts]:                                # the carried datasets: byte for byte
                if name != "lidar":
                    assert got[ts][name].dtype == src[ts][name].dtype and got[ts][name].tobytes() == src[ts][name].tobytes(), name
            lidar = got[ts]["lidar"]
            assert lidar.shape == ft["pc0"].shape and lidar.dtype == np.float32 and np.array_equal(lidar[:, 3], ft["pc0"][:, 3])
            assert ref.row_errors(lidar, ft["pc0"]).max() <= 8e-6          # the instantaneous sweep
            key = got[ts]["deskew"]
            assert key.shape == (8,) and key.dtype == np.float64
            assert np.abs(key[:7] - tw[k, :7]).max() <= 1e-15 and key[7] == float(fs["lidar_dt"].max())
    # a rerun is refused, and passes with --overwrite; compensating twice is refused
    with pytest.raises(FileExistsError, match="--overwrite"):
        deskew.main(str(D), str(O))
    before = (O / "drive0.h5").read_bytes()
    again = deskew.main(str(D), str(O), overwrite=True)
    assert again == out and (O / "drive0.h5").read_bytes() == before
    with pytest.raises(ValueError, match="compensating twice"):
        deskew.main(str(O), str(O2))
    assert not O2.exists()
    # --inverse on O: the input's lidar again, the key dropped
    back = deskew.main(str(O), str(BACK), inverse=True)
    assert "inverse" in capsys.readouterr().out and back["all"]["rows_moved"] == a["rows_moved"]
    for fr_skew in scenes:
        sc = fr_skew[0]["scene_id"]
        src, got = _groups(D / f"{sc}.h5"), _groups(BACK / f"{sc}.h5")
        for ts in src:
            assert sorted(got[ts]) == sorted(src[ts])
            assert ref.row_errors(got[ts]["lidar"], src[ts]["lidar"]).max() <= 8e-6
    with pytest.raises(KeyError, match="--inverse re-skews"):
        deskew.main(str(D), str(O2), inverse=True)
    # the containers and directories it refuses
    NpzDataset.write(tmp_path / "npz", scenes[0][:2])
    with pytest.raises(ValueError, match="npz container"):
        deskew.main(str(tmp_path / "npz"), str(O2))
    with pytest.raises(ValueError, match="equals --data_dir"):
        deskew.main(str(D), str(D))


def test_chain_odometry_then_deskew(gpu, tmp_path):
    """A skewed drive through ``odometry`` and then ``deskew --pose_key pose_odom``: the mean row error against the instantaneous sweeps is
    at most 10 % of the skewed sweeps' own (a condition; the float64 prototype of the restatement reached 0.25 to 0.44 % on this cloud)"""
    from himo_amd import deskew, odometry
    from himo_amd.synthetic import write_h5_scenes
    frames, skewed = ref.drive("uniform", "azimuth")
    D, O = tmp_path / "in", tmp_path / "out"
    D.mkdir()
    write_h5_scenes(D, [skewed])
    odo = odometry.main(str(D), gt_key="pose")["all"]
    out = deskew.main(str(D), str(O), pose_key="pose_odom")["all"]
    got = _groups(O / f"{frames[0]['scene_id']}.h5")
    before = np.mean([ref.row_errors(s["pc0"], f["pc0"]).mean() for s, f in zip(skewed, frames)])
    after = np.mean([ref.row_errors(got[str(f["timestamp"])]["lidar"], f["pc0"]).mean() for f in frames])
    print(f"chain: odometry RPE max {odo['rpe_t_max_m']:.4f} m; mean row error skewed {before:.4f} m, de-skewed {after:.5f} m "
          f"({100 * after / before:.2f} %); greatest max_disp {out['max_disp_m']:.3f} m")
    assert out["sweeps"] == len(frames) and "pose_odom" in got[str(frames[0]["timestamp"])]
    assert after <= 0.10 * before
