"""Box tracking on the GPU: ``himo_boxtrack`` through ctypes on guarded buffers against the pure-Python restatement of the rule
(tests/boxtrack_ref.py), fed the same tables, at the sizes and inputs where the kernel takes another path.  ``track_id``, ``age``,
``state``, ``iou``, ``live`` and ``scene_info`` match bit for bit; no case is left out.  Then ``BoxTracker`` and the program."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest

import boxeval_ref as be
import boxtrack_ref as ref
from test_box_eval_gpu import numbers_equal

pytestmark = pytest.mark.gpu

GUARD = 64                                      # elements before and after every output, and 256 bytes around the workspace
FILL_I, FILL_D = 0x7A7A7A7A, 7.25
NAMES = ("track_id", "age", "state", "iou", "live", "scene_info")


def host_tables(scenes, dts=None, dt=0.1):
    counts = [len(d) for sc in scenes for d in sc]
    sweep_off = np.concatenate([[0], np.cumsum([len(sc) for sc in scenes])]).astype(np.int64)
    det_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    parts = [np.asarray(d, dtype=np.float64).reshape(-1, 12) for sc in scenes for d in sc]
    det = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 12))
    dts = [[dt] * len(sc) for sc in scenes] if dts is None else dts
    h_dt = np.asarray([v for sc in dts for v in sc], dtype=np.float64)
    return det, sweep_off, det_off, h_dt, dts


class Raw:
    """one call of the entry point on guarded buffers: ``status``, the six outputs as numpy arrays, ``intact`` (no guard was written)"""

    def __init__(self, gpu, scenes, dts=None, slab=None, d_sweep_off=None, d_det_off=None, **params):
        import torch
        from himo_amd import _lib
        from himo_amd.track import TrackParams
        lib, P = _lib.load(), _lib.ptr
        det, sweep_off, det_off, h_dt, self.dts = host_tables(scenes, dts)
        n, sweeps, rows = len(scenes), len(det_off) - 1, len(det)
        prm = TrackParams(**params).c_struct()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)      # noqa: E731
        d_det, d_dt = up(det), up(h_dt)
        d_so = up(sweep_off if d_sweep_off is None else np.asarray(d_sweep_off, dtype=np.int64))
        d_do = up(det_off if d_det_off is None else np.asarray(d_det_off, dtype=np.int64))
        sizes = {"track_id": (rows, torch.int32), "age": (rows, torch.int32), "state": (4 * rows, torch.float64), "iou": (rows, torch.float64),
                 "live": (sweeps, torch.int32), "scene_info": (2 * n, torch.int32)}
        buf = {k: torch.full((m + 2 * GUARD,), FILL_I if t == torch.int32 else FILL_D, dtype=t, device=gpu) for k, (m, t) in sizes.items()}
        at = lambda k: buf[k].data_ptr() + GUARD * buf[k].element_size()      # noqa: E731
        need = int(lib.himo_boxtrack_workspace_bytes(n, sweep_off.ctypes.data, det_off.ctypes.data, ctypes.addressof(prm)))
        ws = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=gpu)
        args = [n, P(d_det), sweep_off.ctypes.data, P(d_so), det_off.ctypes.data, P(d_do), h_dt.ctypes.data, P(d_dt), ctypes.addressof(prm)] + \
            [at(k) for k in NAMES] + [ws.data_ptr() + 256, need]
        with torch.cuda.device(gpu):
            if slab is None:
                self.status = lib.himo_boxtrack(*args, _lib.stream_handle())
            else:
                self.status = lib.himo_boxtrack_slabbed(*args, slab, _lib.stream_handle())
        torch.cuda.synchronize()
        self.need, self.intact = need, bool((ws[:256] == 0x5A).all() and (ws[256 + need:] == 0x5A).all())
        for k, (m, t) in sizes.items():
            fill = FILL_I if t == torch.int32 else FILL_D
            self.intact = self.intact and bool((buf[k][:GUARD] == fill).all() and (buf[k][GUARD + m:] == fill).all())
            setattr(self, k, buf[k][GUARD:GUARD + m].cpu().numpy())
        self.state, self.scene_info = self.state.reshape(-1, 4), self.scene_info.reshape(-1, 2)

    def outputs(self):
        return tuple(getattr(self, k) for k in NAMES)


def same(raw, want):
    assert raw.status == 0 and raw.intact
    for k, got, w in zip(NAMES, raw.outputs(), want):
        assert got.dtype == w.dtype and got.shape == w.shape, k
        assert got.tobytes() == w.tobytes(), (k, np.flatnonzero((got != w).reshape(len(w), -1).any(axis=1))[:8])


# ---- scenes and sweeps of every shape -----------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 0, 127, 128, 129, 65, 0)            # detections per sweep of the long scene: the wave and tile edges, and none


@functools.lru_cache(maxsize=None)
def shapes_case():
    rng = np.random.default_rng(51)
    long = [d[:f].copy() for d, f in zip(ref.moving_scene(rng, 129, len(COUNTS), drop=0.0), COUNTS)]      # (rows in random order: who is seen varies)
    seven = ref.moving_scene(rng, 40, 7, drop=0.15)
    seven[0], seven[3], seven[6] = seven[0][:0], seven[3][:0], seven[6][:0]      # no detection at the start, in the middle, at the end
    scenes = [[], ref.moving_scene(rng, 5, 1), ref.moving_scene(rng, 9, 2, drop=0.2), seven, long, [], ref.moving_scene(rng, 512, 3, spacing=7.0, drop=0.01)]
    return scenes, {(m, a): ref.track(scenes, [[0.1] * len(sc) for sc in scenes], vel_mode=m, max_age=a) for m, a in ((0, 2), (1, 0))}


@pytest.mark.parametrize("mode,max_age", [(0, 2), (1, 0)])
def test_scenes_and_sweeps_of_every_shape_in_one_call(gpu, mode, max_age):
    scenes, wants = shapes_case()
    want = wants[(mode, max_age)]
    assert want[5][:, 0].tolist()[:2] == [0, 5] and want[5][6, 0] >= 512 and (want[0] >= 0).sum() > 1500 and (want[3] > 0.5).sum() > 800      # the cases do track
    assert want[4][3:10].tolist()[0] == 0 and want[5][:, 1].sum() == 0
    same(Raw(gpu, scenes, vel_mode=mode, max_age=max_age), want)


def test_one_scene_a_call_and_slabs_of_three_equal_the_batch(gpu):
    scenes, wants = shapes_case()
    want = wants[(0, 2)]
    same(Raw(gpu, scenes, slab=3), want)                            # three launches: scenes 0-2, 3-5, 6
    same(Raw(gpu, scenes, slab=1), want)
    alone = Raw(gpu, [scenes[3]])
    lo, hi = 3, 10                                                  # the sweeps of scene 3 in the batch
    assert alone.status == 0 and alone.live.tobytes() == want[4][lo:hi].tobytes() and alone.scene_info.tobytes() == want[5][3:4].tobytes()
    assert Raw(gpu, []).status == 0 and Raw(gpu, [[], []]).scene_info.tolist() == [[0, 0], [0, 0]]


# ---- the table fills -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_tracks", [1, 64, 512])
def test_the_table_fills_to_max_tracks_and_one_over(gpu, max_tracks):
    base = ref.moving_scene(np.random.default_rng(53), max_tracks + 1, 1, noise=0.0, spacing=7.0, speed=(0.0,))[0]
    # sweep 0 fills the table exactly; from sweep 1 the first object is gone and one more shows: one over, until the coasting track dies
    scene = [base[:max_tracks]] + [base[1:max_tracks + 1]] * 4
    want = ref.track([scene], [[0.1] * 5], max_tracks=max_tracks)
    assert want[4].tolist() == [max_tracks] * 5 and want[5].tolist() == [[max_tracks + 1, 2]]
    assert want[0][-1] == max_tracks and (want[0][max_tracks:3 * max_tracks] == -1).sum() == 2
    same(Raw(gpu, [scene], max_tracks=max_tracks), want)
    exact = ref.track([[base[:max_tracks]] * 2], [[0.1] * 2], max_tracks=max_tracks)
    assert exact[5].tolist() == [[max_tracks, 0]]
    same(Raw(gpu, [[base[:max_tracks]] * 2], max_tracks=max_tracks), exact)


def test_the_cap(gpu):
    base = ref.moving_scene(np.random.default_rng(54), 513, 1)[0]
    over = Raw(gpu, [[base[:3]], [base[:5], base]])
    assert over.status == 6 and over.need == 0 and over.intact and (over.track_id == FILL_I).all() and (over.scene_info == FILL_I).all()      # HIMO_ERR_UNSUPPORTED


# ---- coasting, ties, invalid rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_age", [0, 2])
def test_coasting_through_the_edge(gpu, max_age):
    def scene(gap):
        rows = [np.array([[5.0 * k * 0.1, 0.0, 0.5, 4.5, 1.9, 1.6, 1.0, 0.0, 5.0, 0.0, 0.0, 0.0], [0.0, 20.0, 0.5, 4.5, 1.9, 1.6, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
                for k in range(4 + gap + 2)]
        for k in range(4, 4 + gap):
            rows[k] = rows[k][1:].copy()
        return rows
    scenes = [scene(max_age), scene(max_age + 1)]
    for mode in (0, 1):
        want = ref.track(scenes, [[0.1] * len(sc) for sc in scenes], max_age=max_age, vel_mode=mode)
        if mode == 0:
            assert want[5].tolist() == [[2, 0], [3, 0]]
        same(Raw(gpu, scenes, max_age=max_age, vel_mode=mode), want)


def test_exact_ties_and_invalid_rows(gpu):
    one = [0.0, 0.0, 0.5, 4.0, 2.0, 1.6, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    T = lambda *rows: np.array(rows, dtype=np.float64).reshape(-1, 12)      # noqa: E731
    right, left = list(one), list(one)
    right[0], left[0] = 1.0, -1.0
    ties = [T(*[one] * 8), T(one), T(*[one] * 8), T(right, left), T(*[one] * 3)]
    rng = np.random.default_rng(55)
    dirty = ref.moving_scene(rng, 70, 4)
    for k, d in enumerate(dirty):
        d[3, 3], d[7, 0], d[11, 6], d[12, 5], d[20, 10], d[21, 11], d[22, 9] = -1.0, np.nan, np.inf, -0.1, np.nan, -np.inf, np.inf
        d[30, 3:5], d[31, 4], d[32, 5] = 0.0, 0.0, 0.0             # zero extents are valid
        d[40, 3] = 1.7e308                                          # a valid row whose area is not finite: a track that nothing ever matches
    scenes = [ties, dirty]
    want = ref.track(scenes, [[0.1] * len(sc) for sc in scenes])
    assert want[0][8:9].tolist() == [0] and want[0][9:17].tolist() == list(range(8)) and want[0][17:19].tolist() == [0, 1]
    assert (want[0][22:][[3, 7, 11, 12, 20, 21, 22]] == -1).all() and want[5][1, 0] >= 70 + 4
    same(Raw(gpu, scenes), want)


def test_time_steps_per_sweep(gpu):
    rng = np.random.default_rng(56)
    scenes = [ref.moving_scene(rng, 30, 5, dt=0.05), ref.moving_scene(rng, 20, 4, dt=0.2)]
    dts = [[math.nan, 0.05, 0.05, 0.05, 0.05], [-1.0, 0.2, 0.2, 0.2]]      # (a scene's first is not read)
    for mode in (0, 1):
        same(Raw(gpu, scenes, dts=dts, vel_mode=mode, alpha=0.3, beta=0.8, min_iou=0.3), ref.track(scenes, dts, vel_mode=mode, alpha=0.3, beta=0.8, min_iou=0.3))


# ---- the device tables, reruns, refusals -----------------------------------------------------------------------------------------------------
def test_device_offsets_that_disagree_write_nothing_outside(gpu):
    scenes, _ = shapes_case()
    scenes = scenes[1:5]
    _, sweep_off, det_off, _, _ = host_tables(scenes)
    wrong_rows = [det_off[::-1].copy(), det_off * 3 + 7, det_off - 50, np.full_like(det_off, 2 ** 40), np.where(np.arange(len(det_off)) % 2, det_off, -5)]
    wrong_sweeps = [sweep_off[::-1].copy(), sweep_off + 5, np.full_like(sweep_off, -3), np.array([0, 2 ** 40, 1, 2 ** 50, 3])]
    for d in wrong_rows:
        r = Raw(gpu, scenes, d_det_off=d)
        assert r.status == 0 and r.intact
    for d in wrong_sweeps:
        r = Raw(gpu, scenes, d_sweep_off=d)
        assert r.status == 0 and r.intact
    r = Raw(gpu, scenes, d_sweep_off=wrong_sweeps[1], d_det_off=wrong_rows[1], max_tracks=7)
    assert r.status == 0 and r.intact


def test_two_runs_give_the_same_bytes(gpu):
    scenes, _ = shapes_case()
    one, two = Raw(gpu, scenes, vel_mode=1), Raw(gpu, scenes, vel_mode=1)
    for a, b in zip(one.outputs(), two.outputs()):
        assert a.tobytes() == b.tobytes()


def test_refusals_leave_the_outputs_untouched(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.track import TrackParams, _CParams
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(57)
    scenes = [ref.moving_scene(rng, 12, 3), ref.moving_scene(rng, 7, 2)]
    det, sweep_off, det_off, h_dt, dts = host_tables(scenes)
    n, sweeps, rows = 2, 5, len(det)
    d_det, d_so, d_do, d_dt = (torch.from_numpy(a).to(gpu) for a in (det, sweep_off, det_off, h_dt))
    tid, age = torch.full((rows,), 7, dtype=torch.int32, device=gpu), torch.full((rows,), 7, dtype=torch.int32, device=gpu)
    state, iou = torch.full((rows, 4), 7.0, dtype=torch.float64, device=gpu), torch.full((rows,), 7.0, dtype=torch.float64, device=gpu)
    live, info = torch.full((sweeps,), 7, dtype=torch.int32, device=gpu), torch.full((n, 2), 7, dtype=torch.int32, device=gpu)
    prm = TrackParams().c_struct()
    need = int(lib.himo_boxtrack_workspace_bytes(n, sweep_off.ctypes.data, det_off.ctypes.data, ctypes.addressof(prm)))
    assert need >= 2 * 512 * 12 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)

    def call(**kw):
        a = dict(n=n, det=P(d_det), h_so=sweep_off.ctypes.data, d_so=P(d_so), h_do=det_off.ctypes.data, d_do=P(d_do), h_dt=h_dt.ctypes.data, d_dt=P(d_dt),
                 prm=ctypes.addressof(prm), tid=P(tid), age=P(age), state=P(state), iou=P(iou), live=P(live), info=P(info), ws=P(ws), ws_bytes=ws.numel())
        a.update(kw)
        return lib.himo_boxtrack(*[a[k] for k in ("n", "det", "h_so", "d_so", "h_do", "d_do", "h_dt", "d_dt", "prm", "tid", "age", "state", "iou", "live",
                                                  "info", "ws", "ws_bytes")], _lib.stream_handle())
    late, falling, rows_late, rows_falling, bad_dt, over = sweep_off.copy(), sweep_off.copy(), det_off.copy(), det_off.copy(), h_dt.copy(), det_off.copy()
    late[0], falling[1], rows_late[0], rows_falling[2], bad_dt[4], over[1:] = 1, 6, 1, 0, 0.0, det_off[1:] + 513
    nan_dt, neg_dt = h_dt.copy(), h_dt.copy()
    nan_dt[1], neg_dt[2] = math.nan, -0.1
    def params(**kw):
        c = TrackParams().c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    bad = [params(min_iou=0.0), params(min_iou=1.5), params(min_iou=math.nan), params(alpha=-0.1), params(alpha=1.5), params(alpha=math.nan),
           params(beta=math.inf), params(beta=-1e-9), params(max_age=-1), params(max_age=256), params(max_tracks=0), params(max_tracks=513),
           params(vel_mode=2), params(vel_mode=-1)]
    refused = [dict(n=-1), dict(prm=None), dict(h_so=None), dict(h_do=None), dict(h_so=late.ctypes.data), dict(h_so=falling.ctypes.data),
               dict(h_do=rows_late.ctypes.data), dict(h_do=rows_falling.ctypes.data), dict(h_dt=None), dict(h_dt=bad_dt.ctypes.data),
               dict(h_dt=nan_dt.ctypes.data), dict(h_dt=neg_dt.ctypes.data), dict(d_so=None), dict(d_do=None), dict(d_so=P(d_so) + 4), dict(d_dt=None),
               dict(det=None), dict(det=P(d_det) + 4), dict(tid=None), dict(age=None), dict(state=None), dict(iou=None), dict(live=None), dict(info=None),
               dict(tid=P(tid) + 2), dict(state=P(state) + 4), dict(iou=P(iou) + 4)] + [dict(prm=ctypes.addressof(b)) for b in bad]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(h_do=over.ctypes.data) == _lib.ERR_UNSUPPORTED      # a sweep above the cap
    for kw in (dict(ws=None), dict(ws_bytes=need - 256), dict(ws=P(ws) + 8)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    assert lib.himo_boxtrack_workspace_bytes(n, late.ctypes.data, det_off.ctypes.data, ctypes.addressof(prm)) == 0
    assert lib.himo_boxtrack_workspace_bytes(n, sweep_off.ctypes.data, over.ctypes.data, ctypes.addressof(prm)) == 0
    assert lib.himo_boxtrack_workspace_bytes(n, sweep_off.ctypes.data, det_off.ctypes.data, ctypes.addressof(bad[0])) == 0
    assert lib.himo_boxtrack_slabbed(n, P(d_det), sweep_off.ctypes.data, P(d_so), det_off.ctypes.data, P(d_do), h_dt.ctypes.data, P(d_dt), ctypes.addressof(prm),
                                     P(tid), P(age), P(state), P(iou), P(live), P(info), P(ws), ws.numel(), 0, _lib.stream_handle()) == _lib.ERR_INVALID_ARGUMENT
    assert ctypes.sizeof(_CParams) == lib.himo_abi_sizeof(b"himo_boxtrack_params")
    torch.cuda.synchronize()
    outs = (tid, age, state, iou, live, info)
    assert all(bool((o == 7).all()) for o in outs) and not ws.any()
    # nothing to do: HIMO_OK, nothing written; then the same call, admitted, writes
    assert call(n=0, h_so=None, h_do=None, h_dt=None) == _lib.OK
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    assert call() == _lib.OK
    torch.cuda.synchronize()
    for got, want in zip(outs, ref.track(scenes, dts)):
        assert got.cpu().numpy().tobytes() == want.tobytes()


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------
def test_the_tracker_equals_the_raw_call(gpu):
    import torch
    from himo_amd.track import BoxTracker
    scenes, wants = shapes_case()
    res = BoxTracker(gpu, vel_mode=1, max_age=0).track(scenes)
    assert len(res) == len(scenes) and res.sweeps(4) == len(COUNTS)
    for got, want in zip((res.track_id, res.age, res.state, res.iou, res.live, res.scene_info), wants[(1, 0)]):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    lo = int(res.det_off[int(res.sweep_off[4]) + 2])
    assert res.sweep(4, 2)[0].tobytes() == wants[(1, 0)][0][lo:lo + 63].tobytes()
    empty = BoxTracker(gpu).track([])
    assert len(empty) == 0 and empty.track_id.shape == (0,) and empty.scene_info.shape == (0, 2)
    s1 = torch.cuda.Stream(device=gpu)                              # on another stream, with time steps of its own
    dts = [[0.2] * len(sc) for sc in scenes[:5]]
    with torch.cuda.stream(s1):
        other = BoxTracker(gpu, sensor_dt=0.3).track(scenes[:5], dts)
    s1.synchronize()
    assert other.track_id.tobytes() == ref.track(scenes[:5], dts)[0].tobytes()


# ---- the program, end to end -------------------------------------------------------------------------------------------------------------------
def restated(scenes, name, gt=None, min_hits=3, **params):
    """(the program's numbers for ``name``, the stored rows per sweep) from the restatement; ``scenes`` = [[{key: array} per sweep] per scene]"""
    from himo_amd import track
    sums, stored = track.new_sums(), []
    for items in scenes:
        first = items[0]["pose0"]
        dets = [ref.detections(f[f"boxes_{name}"], f["pose0"], first) for f in items]
        sweeps, n_ids, over = ref.track_scene(dets, [0.1] * len(items), **params)
        rows = [ref.stored_rows(s[0], s[1], s[2], d, f["pose0"], first) for s, d, f in zip(sweeps, dets, items)]
        stored.append(rows)
        track.tally_scene(sums, [f[f"boxes_{name}"] for f in items], rows, n_ids, over, min_hits)
        if gt:
            mot = []
            for f, r in zip(items, rows):
                ma, _, iou_a = be.match(f[f"boxes_{gt}"], f[f"boxes_{name}"])
                mot.append((f[f"boxes_{gt}"], r[:, 0], ma, iou_a))
            track.tally_mot(sums, mot)
    return track.summary({name: sums}, bool(gt))[name], stored


def test_program_on_an_npz_container(gpu, tmp_path, monkeypatch, capsys):
    import test_box_fit_gpu as fit_tests
    from himo_amd import box_fit, track
    from himo_amd.dataset import NpzDataset
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "drive"
    frames = fit_tests._drive(root, sweeps=4)
    more = [dict(f, scene_id="s1") for f in frames[:2]]            # a second scene of two sweeps, in which the ego drives and turns
    for k, f in enumerate(more):
        c, s = math.cos(0.3 + 0.05 * k), math.sin(0.3 + 0.05 * k)
        f["pose0"] = np.array([[c, -s, 0.0, 5.0 + 0.5 * k], [s, c, 0.0, 0.1 * k], [0.0, 0.0, 1.0, 0.2], [0.0, 0.0, 0.0, 1.0]])
    NpzDataset.write(root, frames + more)
    box_fit.main(str(root), "flow,raw", "ids")
    capsys.readouterr()
    out = tmp_path / "tracks.json"
    numbers = track.main(str(root), "raw", gt="flow", json_path=str(out), point_label_key="ids", batch=1, min_hits=2)
    assert json.loads(out.read_text()) == numbers and list(numbers) == ["raw"]
    printed = capsys.readouterr().out
    assert "box tracking, v1; parity unpinned" in printed and "against flow all" in printed

    def load(keys):
        scenes = []
        for sc, fs in (("s0", frames), ("s1", more)):
            items = []
            for f in fs:
                with np.load(root / sc / f"{f['timestamp']}.npz") as z:
                    items.append({k: z[k] for k in keys if k in z.files})
            scenes.append(items)
        return scenes
    scenes = load(("boxes_raw", "boxes_flow", "pose0", "ids", "tracks_raw", "track_label_raw"))
    want, rows = restated(scenes, "raw", "flow", min_hits=2)
    numbers_equal(numbers["raw"], want)
    for items, rs in zip(scenes, rows):
        for f, r in zip(items, rs):
            assert f["tracks_raw"].dtype == np.float64 and f["tracks_raw"].shape == (2, 6) and f["tracks_raw"].tobytes() == r.tobytes()
            assert f["track_label_raw"].dtype == np.int32 and f["track_label_raw"].tobytes() == track.point_labels(f["ids"], f["boxes_raw"], r[:, 0]).tobytes()
            assert set(f["track_label_raw"][f["ids"] == 17].tolist()) == {int(r[f["boxes_raw"][:, 10] == 17, 0][0])}
    assert numbers["raw"]["ids"] >= 4 and numbers["raw"]["boxes"] == 12 and numbers["raw"]["mot"]["all"]["gt"] == 12
    parked = [int(r[f["boxes_raw"][:, 10] == 17, 0][0]) for f, r in zip(scenes[0], rows[0])]
    assert len(set(parked)) == 1                                    # the parked car of the first scene is one track
    # a second run is refused and leaves the files alone; --overwrite replaces
    with pytest.raises(FileExistsError, match="tracks_raw.*--overwrite"):
        track.main(str(root), "raw")
    track._cli(["--data_dir", str(root), "--res_names", "raw,flow", "--overwrite", "--vel_mode", "track", "--max_age", "0", "--alpha", "0.7"])
    scenes = load(("boxes_raw", "boxes_flow", "pose0", "tracks_raw", "tracks_flow", "track_label_raw"))
    for name in ("raw", "flow"):
        _, rows = restated(scenes, name, vel_mode=1, max_age=0, alpha=0.7)
        for items, rs in zip(scenes, rows):
            for f, r in zip(items, rs):
                assert f[f"tracks_{name}"].tobytes() == r.tobytes() and "track_label_raw" in f


def test_program_on_h5_scene_files(gpu, tmp_path, monkeypatch):
    import warnings
    from himo_amd import box_fit, synthetic, track
    from himo_amd.dataset import HDF5Dataset, h5_reader
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "scenes"
    root.mkdir()
    synthetic.write_h5_scenes(root, [synthetic.make_scene(s, 4, n_points=3000, n_instances=4, scene_id=f"sc{s}") for s in (1, 2)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # (the last sweep of a scene has no successor)
        box_fit.main(str(root), "flow,raw", "flow_instance_id")
        numbers = track.main(str(root), "raw,flow", point_label_key="flow_instance_id")
        with pytest.raises(FileExistsError, match="--overwrite"):
            track.main(str(root), "raw")
        with pytest.raises(KeyError, match="boxes_nope"):
            track.main(str(root), "nope")
        scored = track.main(str(root), "raw", gt="flow", overwrite=True)
        ds = HDF5Dataset(root, vis_name="", fields=("pose0",))
    scenes = {}
    for scene_id, ts in ds.index:
        with h5_reader().File(root / f"{scene_id}.h5", "r") as h:
            g = h[str(ts)]
            scenes.setdefault(scene_id, []).append({k: np.asarray(g[k][:]) for k in ("boxes_flow", "boxes_raw", "tracks_raw", "tracks_flow", "track_label_raw",
                                                                                     "flow_instance_id")} | {"pose0": np.asarray(g["pose"][:])})
    ds.close()
    scenes = list(scenes.values())
    assert [len(s) for s in scenes] == [3, 3] and sum(len(f["boxes_raw"]) for s in scenes for f in s) >= 6
    for name in ("raw", "flow"):
        want, rows = restated(scenes, name)
        numbers_equal(numbers[name], want)
        for items, rs in zip(scenes, rows):
            for f, r in zip(items, rs):
                assert f[f"tracks_{name}"].dtype == np.float64 and f[f"tracks_{name}"].tobytes() == r.tobytes()
                if name == "raw":
                    assert f["track_label_raw"].tobytes() == track.point_labels(f["flow_instance_id"], f["boxes_raw"], r[:, 0]).tobytes()
    numbers_equal(scored["raw"], restated(scenes, "raw", "flow")[0])
    assert scored["raw"]["mot"]["all"]["gt"] == sum(len(f["boxes_flow"]) for s in scenes for f in s) and scored["raw"]["mot"]["all"]["tp"] >= 1
