"""Box evaluation on the GPU: ``himo_boxeval_match`` and ``himo_box_iou_pairs`` against the pure-Python restatement of the rule
(tests/boxeval_ref.py) at the sizes and inputs where the kernels take another path.  ``match_a``, ``match_b``, ``iou_a`` and the listed
pairs' IoUs match bit for bit; no case is left out.  Small sweeps: every case is a few hundred boxes."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest

import boxeval_ref as ref

pytestmark = pytest.mark.gpu

TILE = 128                                      # HIMO_BOXEVAL_TILE: the rects of B a pair-phase block stages in LDS


def device_match(gpu, rows_a, rows_b, min_iou=0.1):
    from himo_amd.eval_box import BoxEvaluator
    return BoxEvaluator(gpu, min_iou).match(rows_a, rows_b)


def same(res, rows_a, rows_b, min_iou=0.1, want=None):
    """every sweep of a ``MatchResult`` against the restatement, bit for bit; returns the restatement's results"""
    want = want if want is not None else [ref.match(a, b, min_iou) for a, b in zip(rows_a, rows_b)]
    assert len(res) == len(rows_a) and res.match_a.dtype == np.int32 and res.match_b.dtype == np.int32 and res.iou_a.dtype == np.float64
    for s, (ma, mb, iou_a) in enumerate(want):
        ga, gb, gi = res.sweep(s)
        assert ga.tobytes() == ma.tobytes(), (s, np.flatnonzero(ga != ma)[:5])
        assert gb.tobytes() == mb.tobytes(), (s, np.flatnonzero(gb != mb)[:5])
        assert gi.tobytes() == iou_a.tobytes(), (s, np.abs(gi - iou_a).max())
    return want


# ---- sizes at the wave, tile and block edges ------------------------------------------------------------------------------------------------
SIZES = ((0, 0), (0, 64), (65, 0), (1, 1), (1, 300), (63, TILE + 1), (64, 64), (65, TILE - 1), (TILE - 1, 65), (TILE, TILE), (TILE + 1, 63), (300, 300),
         (300, 1))


@functools.lru_cache(maxsize=None)
def sizes_case():
    rng = np.random.default_rng(41)
    rows_a, rows_b = [], []
    for fa, fb in SIZES:
        a, b = ref.jittered_sweep(rng, max(fa, fb, 1), extra=0.0)
        rows_a.append(a[:fa].copy())
        rows_b.append(b[:fb].copy())
    return rows_a, rows_b, [ref.match(a, b) for a, b in zip(rows_a, rows_b)]


def test_sizes_at_the_edges_in_one_batched_call_and_one_call_each(gpu):
    rows_a, rows_b, want = sizes_case()
    matched = [int((w[0] >= 0).sum()) for w in want]
    assert matched[0] == matched[1] == matched[2] == 0 and matched[11] >= 250 and sum(matched) >= 600      # the cases do match boxes
    res = device_match(gpu, rows_a, rows_b)
    same(res, rows_a, rows_b, want=want)
    assert res.off_a.tolist() == np.concatenate([[0], np.cumsum([s[0] for s in SIZES])]).tolist()
    for s in range(len(SIZES)):                                     # the same sweeps, one call each: identical
        alone = device_match(gpu, [rows_a[s]], [rows_b[s]])
        for got, batched in zip(alone.sweep(0), res.sweep(s)):
            assert got.tobytes() == batched.tobytes(), s


def test_realistic_sweeps(gpu):
    rng = np.random.default_rng(42)
    rows_a, rows_b = zip(*[ref.jittered_sweep(rng, F) for F in (250, 180, 90)])
    want = same(device_match(gpu, rows_a, rows_b), rows_a, rows_b)
    ma, _, iou_a = want[0]
    assert len(rows_a[0]) == 300 and 200 <= (ma >= 0).sum() <= 250 and 0.3 < iou_a[ma >= 0, 0].mean() < 0.95      # 20 % extra boxes overlap nothing
    same(device_match(gpu, rows_a, rows_b, 0.5), rows_a, rows_b, 0.5)
    same(device_match(gpu, rows_a, rows_b, 1.0), rows_a, rows_b, 1.0)


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------------
def test_ties(gpu):
    eight = ref.box_rows(np.tile([[12.0, -7.0]], (8, 1)), np.tile([[4.5, 1.9]], (8, 1)), np.full(8, 0.7))
    # two boxes of A mirror-symmetric about one box of B: the two IoUs are equal, the lower i wins
    mid = ref.box_rows([[0.0, 0.0]], [[4.0, 2.0]], [0.0])
    two = ref.box_rows([[1.0, 0.0], [-1.0, 0.0]], [[4.0, 2.0], [4.0, 2.0]], [0.0, 0.0])
    iou, _ = ref.iou_matrix(ref.rects(two), ref.rects(mid))
    assert iou[0, 0] == iou[1, 0] == 0.6
    # ... and the same about a turned box, as the restatement rounds it
    turned = ref.box_rows([[8.0, 8.0]], [[4.0, 2.0]], [math.pi / 4])
    d = 0.5
    pair = ref.box_rows([[8.0 + d, 8.0 + d], [8.0 - d, 8.0 - d]], [[4.0, 2.0], [4.0, 2.0]], [math.pi / 4, math.pi / 4])
    iou_t, _ = ref.iou_matrix(ref.rects(pair), ref.rects(turned))
    rows_a, rows_b = [eight, two, mid, pair], [eight, mid, two, turned]
    want = same(device_match(gpu, rows_a, rows_b), rows_a, rows_b)
    assert want[0][0].tolist() == list(range(8)) and want[1][0].tolist() == [0, -1] and want[2][0].tolist() == [0] and want[2][1].tolist() == [0, -1]
    if iou_t[0, 0] == iou_t[1, 0]:
        assert want[3][0].tolist() == [0, -1]


# ---- the chain: one kept pair a round ------------------------------------------------------------------------------------------------------------
def test_the_chain(gpu):
    rows_a, rows_b = ref.chain()
    want = same(device_match(gpu, [rows_a], [rows_b], 0.05), [rows_a], [rows_b], 0.05)
    assert want[0][0].tolist() == list(range(70)) and want[0][1].tolist() == list(range(70))
    # at the default min_iou the end of the chain falls below the threshold
    want = same(device_match(gpu, [rows_a], [rows_b]), [rows_a], [rows_b])
    assert 0 < (want[0][0] >= 0).sum() < 70


# ---- the cap ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_cap(gpu):
    from himo_amd.eval_box import BoxEvaluator
    rng = np.random.default_rng(43)
    a, b = ref.jittered_sweep(rng, 1024, extra=0.0, spacing=7.0)
    few = b[[5, 600, 1023]]
    same(device_match(gpu, [a], [few]), [a], [few])
    same(device_match(gpu, [few], [a]), [few], [a])
    over = np.concatenate([a, a[:1]])
    with pytest.raises(ValueError, match="1025 boxes"):
        BoxEvaluator(gpu).match([few, over], [few, few])
    with pytest.raises(ValueError, match="1025 boxes"):
        BoxEvaluator(gpu).match([few], [over])


# ---- rects ------------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_zero_extent_far_and_z_disjoint_rects(gpu):
    rng = np.random.default_rng(44)
    a, b = ref.jittered_sweep(rng, 80, extra=0.1)
    a[3, 3], a[7, 0], a[11, 6], a[12, 5] = -1.0, np.nan, np.inf, -0.1                   # INVALID: l < 0, x, yaw not finite, h < 0
    b[5, 4], b[9, 1] = -2.0, -np.inf
    a[20, 3:5], a[21, 4], b[22, 3], b[23, 5] = 0.0, 0.0, 0.0, 0.0                      # zero extents are valid
    a[30:40, 2] += 5.0                                             # z ranges that do not overlap: iou3 = 0 while iou > 0
    far_a, far_b = ref.jittered_sweep(rng, 30, extra=0.0)
    far_a[:, 0:2] = far_a[:, 0:2] / 4 + np.float32([51.0, -51.0])   # coordinates at +-51 m
    far_b[:, 0:2] = far_b[:, 0:2] / 4 + np.float32([51.0, -51.0])
    def mirrored(rows):
        out = rows.copy()
        out[:, 0:2] *= np.float32(-1)
        return out
    rows_a, rows_b = [a, far_a, mirrored(far_b)], [b, far_b, mirrored(far_a)]
    want = same(device_match(gpu, rows_a, rows_b), rows_a, rows_b)
    ma, mb, iou_a = want[0]
    assert (ma[[3, 7, 11, 12]] == -1).all() and (mb[[5, 9]] == -1).all()
    lifted = [i for i in range(30, 40) if ma[i] >= 0]
    assert lifted and (iou_a[lifted, 0] > 0).all() and (iou_a[lifted, 1] == 0).all()
    assert (want[1][0] >= 0).sum() >= 5


# ---- listed pairs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_iou_of_listed_pairs(gpu, n):
    from himo_amd.eval_box import BoxEvaluator
    rng = np.random.default_rng(45)
    a, b = ref.jittered_sweep(rng, 40, extra=0.0)
    b = b[:33]
    a[2, 3] = -1.0
    lookup = {int(v): k for k, v in enumerate(b[:, 10])}
    partner = np.array([lookup.get(int(v), 0) for v in a[:, 10]])
    i = rng.integers(0, len(a), n)
    pairs = np.stack([i, np.where(rng.uniform(0, 1, n) < 0.7, partner[i], rng.integers(0, len(b), n))], axis=1).astype(np.int64)
    if n >= 63:                                                     # repeated pairs and indices outside their tables
        pairs[5] = pairs[4]
        pairs[10], pairs[11], pairs[12], pairs[13] = (-1, 0), (0, -1), (len(a), 0), (0, len(b))
        pairs[n - 1] = (2 ** 40, 3)
    got = BoxEvaluator(gpu).iou_pairs(a, b, pairs)
    want = ref.iou_pairs(a, b, pairs)
    assert tuple(got.shape) == (n, 2) and got.cpu().numpy().tobytes() == want.tobytes()
    if n >= 63:
        assert not want[[10, 11, 12, 13, n - 1]].any() and (want[:, 0] > 0.3).sum() > n // 4


# ---- streams and reruns ----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_in_flight_on_two_streams(gpu):
    import torch
    rows_a, rows_b, want = sizes_case()
    rng = np.random.default_rng(46)
    a2, b2 = ref.jittered_sweep(rng, 200)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s1):
        got = device_match(gpu, rows_a, rows_b)
    with torch.cuda.stream(s2):
        got2 = device_match(gpu, [a2], [b2])
    s1.synchronize()
    s2.synchronize()
    same(got, rows_a, rows_b, want=want)
    same(got2, [a2], [b2])


def test_two_runs_give_the_same_bytes(gpu):
    rows_a, rows_b, _ = sizes_case()
    one, two = device_match(gpu, rows_a, rows_b), device_match(gpu, rows_a, rows_b)
    assert one.match_a.tobytes() == two.match_a.tobytes() and one.match_b.tobytes() == two.match_b.tobytes() and one.iou_a.tobytes() == two.iou_a.tobytes()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.eval_box import _CParams
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(47)
    rows_a, rows_b = zip(*[ref.jittered_sweep(rng, F) for F in (40, 25)])
    S = 2
    off_a = np.concatenate([[0], np.cumsum([len(r) for r in rows_a])]).astype(np.int64)
    off_b = np.concatenate([[0], np.cumsum([len(r) for r in rows_b])]).astype(np.int64)
    ra, rb = (torch.from_numpy(np.concatenate([ref.rects(r) for r in rows])).to(gpu) for rows in (rows_a, rows_b))
    d_oa, d_ob = torch.from_numpy(off_a).to(gpu), torch.from_numpy(off_b).to(gpu)
    ma = torch.full((int(off_a[S]),), 7, dtype=torch.int32, device=gpu)
    mb = torch.full((int(off_b[S]),), 7, dtype=torch.int32, device=gpu)
    iou = torch.full((int(off_a[S]), 2), 7.0, dtype=torch.float64, device=gpu)
    need = int(lib.himo_boxeval_workspace_bytes(S, off_a.ctypes.data, off_b.ctypes.data))
    assert need >= int(off_a[S]) * max(len(r) for r in rows_b) * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    prm = _CParams(0.1)

    def call(**kw):
        a = dict(S=S, ra=P(ra), h_oa=off_a.ctypes.data, d_oa=P(d_oa), rb=P(rb), h_ob=off_b.ctypes.data, d_ob=P(d_ob), prm=ctypes.addressof(prm),
                 ma=P(ma), mb=P(mb), iou=P(iou), ws=P(ws), ws_bytes=ws.numel())
        a.update(kw)
        return lib.himo_boxeval_match(a["S"], a["ra"], a["h_oa"], a["d_oa"], a["rb"], a["h_ob"], a["d_ob"], a["prm"], a["ma"], a["mb"], a["iou"],
                                      a["ws"], a["ws_bytes"], _lib.stream_handle())
    negative, decreasing, late, over = off_a.copy(), off_a.copy(), off_a.copy(), off_b.copy()
    negative[0], decreasing[1], late[0] = -1, decreasing[2] + 1, 1
    over[1:] += 1025
    bad = [_CParams(v) for v in (0.0, -0.5, 1.0000001, math.nan, math.inf)]
    refused = [dict(S=-1), dict(prm=None), dict(h_oa=None), dict(h_ob=None), dict(h_oa=negative.ctypes.data), dict(h_oa=decreasing.ctypes.data),
               dict(h_oa=late.ctypes.data), dict(d_oa=None), dict(d_ob=None), dict(d_oa=P(d_oa) + 4), dict(ra=None), dict(rb=None), dict(ra=P(ra) + 4),
               dict(ma=None), dict(mb=None), dict(iou=None), dict(mb=P(mb) + 2), dict(iou=P(iou) + 4)] + [dict(prm=ctypes.addressof(b)) for b in bad]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(h_ob=over.ctypes.data) == _lib.ERR_UNSUPPORTED      # a sweep above the cap
    for kw in (dict(ws=None), dict(ws_bytes=need - 256), dict(ws=P(ws) + 8)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    torch.cuda.synchronize()
    assert (ma == 7).all() and (mb == 7).all() and (iou == 7.0).all() and not ws.any()
    # himo_box_iou_pairs
    pairs = torch.zeros((4, 2), dtype=torch.int64, device=gpu)
    out = torch.full((4, 2), 7.0, dtype=torch.float64, device=gpu)
    lister = lambda n=4, a=P(ra), na=5, b=P(rb), nb=5, pr=P(pairs), o=P(out): lib.himo_box_iou_pairs(n, a, na, b, nb, pr, o, _lib.stream_handle())      # noqa: E731
    for kw in (dict(n=-1), dict(na=-1), dict(nb=-1), dict(a=None), dict(b=None), dict(pr=None), dict(o=None), dict(pr=P(pairs) + 4), dict(o=P(out) + 4),
               dict(a=P(ra) + 4)):
        assert lister(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert lister(n=0, pr=None, o=None) == _lib.OK
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # nothing to do: HIMO_OK, nothing written; then the same call, admitted, writes
    zero = np.zeros(S + 1, np.int64)
    assert call(S=0, h_oa=None, h_ob=None) == _lib.OK and call(h_oa=zero.ctypes.data, h_ob=zero.ctypes.data, ra=None, rb=None) == _lib.OK
    torch.cuda.synchronize()
    assert (ma == 7).all() and (mb == 7).all() and (iou == 7.0).all()
    assert call() == _lib.OK
    torch.cuda.synchronize()
    for s in range(S):
        wa, wb, wi = ref.match(rows_a[s], rows_b[s])
        assert ma[off_a[s]:off_a[s + 1]].cpu().numpy().tobytes() == wa.tobytes() and mb[off_b[s]:off_b[s + 1]].cpu().numpy().tobytes() == wb.tobytes()
        assert iou[off_a[s]:off_a[s + 1]].cpu().numpy().tobytes() == wi.tobytes()


# ---- the program, end to end --------------------------------------------------------------------------------------------------------------------------
def numbers_equal(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (a.keys(), b.keys())
        for k in a:
            numbers_equal(a[k], b[k])
    elif a is None or b is None or isinstance(a, int):
        assert a == b
    else:
        assert a == pytest.approx(b, rel=1e-12, abs=1e-15)


def restated(stored, gt, name, pair_by="iou", min_iou=0.1):
    """the program's numbers for ``name`` from the restatement, over ``stored`` = [{key: box rows}] per sweep"""
    sweeps = []
    for have in stored:
        g, p = have[f"boxes_{gt}"], have[f"boxes_{name}"]
        if pair_by == "iou":
            ma, _, iou_a = ref.match(g, p, min_iou)
        else:
            ids, ig, ip = np.intersect1d(g[:, 10], p[:, 10], return_indices=True)
            ma, iou_a = np.full(len(g), -1, np.int64), np.zeros((len(g), 2))
            ma[ig], iou_a[ig] = ip, ref.iou_pairs(g, p, np.stack([ig, ip], axis=1))
        sweeps.append((g, p, ma, iou_a))
    return ref.score(sweeps, pair_by)


def test_program_on_an_npz_container(gpu, tmp_path, monkeypatch, capsys):
    import test_box_fit_gpu as fit_tests
    from himo_amd import box_fit, eval_box
    from himo_amd.dataset import NpzDataset
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "drive"
    frames = fit_tests._drive(root, sweeps=3)
    for f in frames:
        f["est"] = (0.8 * f["flow"]).astype(np.float32)             # a stored flow that leaves a fifth of the smear
    NpzDataset.write(root, frames)
    box_fit.main(str(root), "flow,raw,est", "ids")
    capsys.readouterr()
    out = tmp_path / "eval.json"
    numbers = eval_box.main(str(root), "flow", "raw,est", json_path=str(out), batch=2)
    assert json.loads(out.read_text()) == numbers and list(numbers) == ["raw", "est"]
    printed = capsys.readouterr().out
    assert "box evaluation, v1; parity unpinned" in printed and "raw against flow" in printed and "est against flow" in printed
    stored = []
    for f in frames:
        with np.load(root / "s0" / f"{f['timestamp']}.npz") as z:
            stored.append({k: z[k] for k in ("boxes_flow", "boxes_raw", "boxes_est")})
    for name in ("raw", "est"):
        numbers_equal(numbers[name], restated(stored, "flow", name))
    # the parked car is the same box under every name; the vehicle at 30 m/s is smeared by 3 m as recorded
    alls = {s: numbers[s]["buckets"]["all"] for s in ("raw", "est")}
    assert alls["raw"]["gt"] == alls["est"]["gt"] == 6 and numbers["raw"]["pred"] == 6
    fast = numbers["raw"]["buckets"]["speed 20-30"]["gt"] + numbers["raw"]["buckets"]["speed 30+"]["gt"]      # 30 m/s, as float32 rounds it
    assert numbers["raw"]["buckets"]["speed static"]["mean_iou"] > 0.99 and numbers["raw"]["buckets"]["speed static"]["gt"] == 3 and fast == 3
    assert alls["est"]["mean_iou"] > alls["raw"]["mean_iou"] and alls["raw"]["at"]["0.7"]["tp"] < 6
    # --pair_by label: the listed pairs of the label intersection
    by_label = eval_box.main(str(root), "flow", "raw,est", pair_by="label")
    ev = eval_box.BoxEvaluator(gpu)
    for name in ("raw", "est"):
        numbers_equal(by_label[name], restated(stored, "flow", name, "label"))
        for have in stored:
            g, p = have["boxes_flow"], have[f"boxes_{name}"]
            ig, ip = eval_box.label_pairs(g, p)
            pairs = np.stack([ig, ip], axis=1)
            assert len(pairs) == 2 and ev.iou_pairs(g, p, pairs).cpu().numpy().tobytes() == ref.iou_pairs(g, p, pairs).tobytes()
    assert "at" not in by_label["raw"]["buckets"]["all"] and by_label["raw"]["buckets"]["all"]["pairs"] == 6
    with pytest.raises(ValueError, match="--gt flow is among"):
        eval_box._cli(["--data_dir", str(root), "--gt", "flow", "--res_names", "flow"])
    eval_box._cli(["--data_dir", str(root), "--gt", "flow", "--res_names", "est", "--min_iou", "0.3", "--batch", "1"])


def test_program_on_h5_scene_files(gpu, tmp_path, monkeypatch):
    import warnings
    from himo_amd import box_fit, eval_box, synthetic
    from himo_amd.dataset import HDF5Dataset, h5_reader
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "scenes"
    root.mkdir()
    synthetic.write_h5_scenes(root, [synthetic.make_scene(s, 3, n_points=3000, n_instances=4, scene_id=f"sc{s}") for s in (1, 2)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # (the last sweep of a scene has no successor)
        box_fit.main(str(root), "flow,raw", "flow_instance_id")
        numbers = eval_box.main(str(root), "flow", "raw")
        by_label = eval_box.main(str(root), "flow", "raw", pair_by="label")
        ds = HDF5Dataset(root, vis_name="", fields=("pose0",))
        with pytest.raises(ValueError, match="--gt flow is among"):
            eval_box.main(str(root), "flow", "flow")
        with pytest.raises(KeyError, match="boxes_nope"):
            eval_box.main(str(root), "flow", "nope")
    stored = []
    for scene_id, ts in ds.index:
        with h5_reader().File(root / f"{scene_id}.h5", "r") as h:
            stored.append({k: np.asarray(h[str(ts)][k][:]) for k in ("boxes_flow", "boxes_raw")})
    ds.close()
    assert len(stored) == 4 and sum(len(s["boxes_flow"]) for s in stored) >= 4
    numbers_equal(numbers["raw"], restated(stored, "flow", "raw"))
    numbers_equal(by_label["raw"], restated(stored, "flow", "raw", "label"))
    assert numbers["raw"]["buckets"]["all"]["gt"] == sum(len(s["boxes_flow"]) for s in stored) and numbers["raw"]["buckets"]["all"]["pairs"] >= 1
