"""The ICP-Flow baseline on the GPU against the numpy restatement of its written rule (tests/icpflow_ref.py; parity with the
reference's ICP-Flow is unpinned): ``himo_icp_vote`` counter for counter, ``himo_icp_step`` exactly in its decisions and within the
measured bar in its transforms, ``IcpFlow.fit`` end to end, the refusals, and the chain scenes -> ground masks -> save -> zip -> eval.
Every device buffer sits between guard words that are checked afterwards.  tests/test_icpflow_cpu.py shows that the seeded inputs'
discrete decisions have margins."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import icpflow_ref as ref
from conftest import REPO
from test_icpflow_cpu import EGO, HAND, SEED, VOTE_CASES

pytestmark = pytest.mark.gpu

GUARD, FILL = 1024, 0xA5


class Buf:
    """a device array between two guard regions; everything starts as FILL bytes"""

    def __init__(self, dev, data=None, shape=None, dtype=None):
        import torch
        host = None if data is None else np.ascontiguousarray(data)
        self.dtype = np.dtype(dtype if host is None else host.dtype)
        self.shape = tuple(shape if host is None else host.shape)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.t = torch.full((2 * GUARD + self.nbytes + 16,), FILL, dtype=torch.uint8, device=dev)
        if host is not None and self.nbytes:
            self.t[GUARD:GUARD + self.nbytes] = torch.from_numpy(host.reshape(-1).view(np.uint8)).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def get(self):
        return self.t[GUARD:GUARD + self.nbytes].cpu().numpy().view(self.dtype).reshape(self.shape).copy()

    def guards_clean(self):
        h = self.t.cpu().numpy()
        return bool((h[:GUARD] == FILL).all() and (h[GUARD + self.nbytes:] == FILL).all())

    def untouched(self):
        return bool((self.t == FILL).all().item())


def c_params(**kw):
    from himo_amd.icpflow import IcpParams
    rule = {k: v for k, v in kw.items() if k in ref.DEFAULTS}
    return IcpParams(**rule).c_struct(), rule


def offsets_of(labels, C):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(labels, np.int64), minlength=C + 1)[1:C + 1])]).astype(np.int64)


def run_vote(dev, pts, labels, C, tgt, pitch=3, ws_bytes=None, call=None, **kw):
    """raw himo_icp_vote: (status, counts, peak, transform, status words, all guards clean?, outputs untouched?)"""
    import torch
    from himo_amd import _lib
    lib = _lib.load()
    cp, rule = c_params(**kw)
    half = ref.params(**rule)["half"]
    W = 2 * half + 1
    n = len(pts)
    rows = np.concatenate([np.asarray(pts, np.float32).reshape(-1, 3), np.full((n, pitch - 3), 7.0, np.float32)], axis=1)
    h_off = offsets_of(labels, C)
    bufs = dict(pts=Buf(dev, rows), off=Buf(dev, h_off), tgt=Buf(dev, np.asarray(tgt, np.float32).reshape(-1, 3)),
                counts=Buf(dev, shape=(C, W, W), dtype=np.int32), peak=Buf(dev, shape=(C, 2), dtype=np.int32),
                T=Buf(dev, shape=(C, 5), dtype=np.float64), st=Buf(dev, shape=(C, 4), dtype=np.int32))
    need = int(lib.himo_icp_workspace_bytes(len(tgt), C))
    bufs["ws"] = Buf(dev, shape=(max(need, 16),), dtype=np.uint8)
    a = dict(n=n, pts=bufs["pts"].ptr, pitch=pitch, C=C, h_off=h_off.ctypes.data, d_off=bufs["off"].ptr, nt=len(tgt), tgt=bufs["tgt"].ptr,
             params=ctypes.addressof(cp), counts=bufs["counts"].ptr, peak=bufs["peak"].ptr, T=bufs["T"].ptr, st=bufs["st"].ptr,
             ws=bufs["ws"].ptr, ws_bytes=need if ws_bytes is None else ws_bytes)
    a.update(call or {})
    status = lib.himo_icp_vote(a["n"], a["pts"], a["pitch"], a["C"], a["h_off"], a["d_off"], a["nt"], a["tgt"], a["params"], a["counts"],
                               a["peak"], a["T"], a["st"], a["ws"], a["ws_bytes"], _lib.stream_handle())
    torch.cuda.synchronize()
    clean = all(b.guards_clean() for b in bufs.values())
    untouched = all(bufs[k].untouched() for k in ("counts", "peak", "T", "st", "ws"))
    return status, bufs["counts"].get(), bufs["peak"].get(), bufs["T"].get(), bufs["st"].get(), clean, untouched


def assert_vote_equals_the_restatement(dev, pts, labels, C, tgt, **kw):
    st, counts, peak, T, words, clean, _ = run_vote(dev, pts, labels, C, tgt, **kw)
    assert st == 0 and clean
    rule = {k: v for k, v in kw.items() if k in ref.DEFAULTS}
    want_counts, want_peak, _ = ref.vote(pts, labels, C, tgt, **rule)
    assert np.array_equal(counts, want_counts), f"{int((counts != want_counts).sum())} counters differ ({counts.sum()} vs {want_counts.sum()} votes)"
    assert np.array_equal(peak, want_peak)
    b = np.float64(np.float32(ref.params(**rule)["bin"]))
    want_T = np.concatenate([np.ones((C, 1)), np.zeros((C, 1)), want_peak * b, np.zeros((C, 1))], axis=1)
    assert T.tobytes() == want_T.tobytes()
    assert np.array_equal(words, np.concatenate([np.zeros((C, 2), np.int32), want_peak], axis=1))
    return int(want_counts.sum())


# ---- 1. the vote ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, C", VOTE_CASES)
def test_vote_equals_the_restatement(gpu, n, C):
    pts, labels, tgt = ref.vote_case(n, n, C)
    votes = assert_vote_equals_the_restatement(gpu, pts, labels, C, tgt, pitch=3 + n % 2)
    assert votes > 0 or n < 8


def test_vote_one_cluster_over_several_blocks_and_many_small_clusters_in_one_block(gpu):
    pts, labels, tgt = ref.vote_case(41, 300, 1, n_target=900)
    assert assert_vote_equals_the_restatement(gpu, pts, labels, 1, tgt) > 1000
    rng = np.random.default_rng(42)
    centres = rng.uniform(-30, 30, (8, 3)) * [1, 1, 0.02]
    small = (np.repeat(centres, 8, axis=0) + rng.normal(0, 0.2, (64, 3))).astype(np.float32)
    tgt = (small + np.float32([0.6, -0.4, 0.0]) + rng.normal(0, 0.05, (64, 3))).astype(np.float32)
    assert assert_vote_equals_the_restatement(gpu, small, np.repeat(np.arange(1, 9), 8), 8, tgt, pitch=4) >= 64


def test_vote_no_clusters_empty_target_gaps_and_other_halves(gpu):
    pts, labels, tgt = ref.vote_case(43, 200, 6, gaps=True)
    assert set(np.unique(labels)) < set(range(1, 7))               # labels without points
    assert assert_vote_equals_the_restatement(gpu, pts, labels, 6, tgt) > 0
    assert assert_vote_equals_the_restatement(gpu, pts, labels, 6, np.zeros((0, 3), np.float32)) == 0
    for half in (1, 16, 45, 64):                                   # 45 and 64: the counters do not fit the LDS histogram
        assert assert_vote_equals_the_restatement(gpu, pts, labels, 6, tgt, half=half, pitch=4) > 0
    assert assert_vote_equals_the_restatement(gpu, pts, labels, 6, tgt, bin=0.1, z_gate=0.3) > 0
    st, counts, peak, T, words, clean, untouched = run_vote(gpu, np.zeros((0, 3), np.float32), np.zeros(0, np.int32), 0, tgt)
    assert st == 0 and clean and untouched                         # C = 0: nothing to do is not an error


def test_vote_targets_outside_the_grid_and_on_half_bin_boundaries(gpu):
    pts = np.float32([[51.0, 51.0, 0], [51.1, 50.9, 0.2], [-51.2, 0.5, 0], [0, 0, 0], [0.0, 0.0, 0.5]])
    tgt = np.float32([[53.5, 52.5, 0.1], [55.0, 51.0, 1.0], [-54.0, 0.0, 0], [-60.0, 3.0, 0], [0.125, 0.375, 0], [0.625, -0.125, 1.0],
                      [4.125, 0, 0], [4.25, 0, 0], [-4.0, 4.0, -1.0], [200.0, 0, 0]])
    assert assert_vote_equals_the_restatement(gpu, pts, np.int32([1, 1, 2, 3, 3]), 3, tgt) > 6


# ---- 2. one step ----------------------------------------------------------------------------------------------------------------------
def run_step(dev, m, labels, C, tgt, d2, idx, T0, st0, final=False, ws_bytes=None, call=None, **kw):
    import torch
    from himo_amd import _lib
    lib = _lib.load()
    cp, _ = c_params(**kw)
    h_off = offsets_of(labels, C)
    bufs = dict(m=Buf(dev, np.asarray(m, np.float32)), off=Buf(dev, h_off), tgt=Buf(dev, np.asarray(tgt, np.float32)), d2=Buf(dev, np.asarray(d2, np.float32)),
                idx=Buf(dev, np.asarray(idx, np.int32)), T=Buf(dev, np.asarray(T0, np.float64)), st=Buf(dev, np.asarray(st0, np.int32)),
                inl=Buf(dev, shape=(len(m),), dtype=np.uint8))
    need = int(lib.himo_icp_workspace_bytes(len(tgt), C))
    bufs["ws"] = Buf(dev, shape=(max(need, 16),), dtype=np.uint8)
    a = dict(n=len(m), m=bufs["m"].ptr, C=C, h_off=h_off.ctypes.data, d_off=bufs["off"].ptr, nt=len(tgt), tgt=bufs["tgt"].ptr, idx=bufs["idx"].ptr,
             d2=bufs["d2"].ptr, params=ctypes.addressof(cp), final=int(final), T=bufs["T"].ptr, st=bufs["st"].ptr, inl=bufs["inl"].ptr,
             ws=bufs["ws"].ptr, ws_bytes=need if ws_bytes is None else ws_bytes)
    a.update(call or {})
    status = lib.himo_icp_step(a["n"], a["m"], a["C"], a["h_off"], a["d_off"], a["nt"], a["tgt"], a["idx"], a["d2"], a["params"], a["final"],
                               a["T"], a["st"], a["inl"], a["ws"], a["ws_bytes"], _lib.stream_handle())
    torch.cuda.synchronize()
    clean = all(b.guards_clean() for b in bufs.values())
    unchanged = (bufs["T"].get().tobytes() == np.asarray(T0, np.float64).tobytes() and np.array_equal(bufs["st"].get(), st0)
                 and bufs["inl"].untouched() and bufs["ws"].untouched())
    return status, bufs["T"].get(), bufs["st"].get(), bufs["inl"].get(), clean, unchanged


@pytest.mark.parametrize("size", ref.STEP_SIZES)
def test_step_equals_the_restatement(gpu, size):
    """counts, inlier masks and flags exactly; transforms within max(16 s, 1e-12), s = the restatement's own spread over forward,
    reversed and pairwise sums (the table at the top of tests/icpflow_ref.py: the floor for every case); two runs give the same bytes"""
    m, labels, tgt, d2, idx = ref.step_case(size)
    bar = max(16 * ref.step_spread(m, labels, 2, tgt, d2, idx), 1e-12)
    T0 = np.array([[1.0, 0.0, 0.05, -0.02, 0.01]] * 2)
    st0 = np.int32([[0, 0, 3, -1], [0, 0, 0, 0]])
    for kw, final in ((dict(), False), (dict(min_inliers=size + 1), False), (dict(), True), (dict(min_ratio=0.95), True)):
        want_T, want_st = T0.copy(), st0.copy()
        want_in = ref.step(m, labels, 2, tgt, d2, idx, want_T, want_st, final, **kw)
        runs = [run_step(gpu, m, labels, 2, tgt, d2, idx, T0, st0, final, **kw) for _ in range(2)]
        for status, T, st, inl, clean, _ in runs:
            assert status == 0 and clean
            assert np.array_equal(st, want_st), (kw, final, st.tolist(), want_st.tolist())
            assert np.array_equal(inl.astype(bool), want_in)
            err = float(np.abs(T - want_T).max())
            print(f"\nstep size {size} {kw} final={final}: max |T - restatement| = {err:.3e} (bar {bar:.1e})")
            assert err <= bar
        assert runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2].tobytes() == runs[1][2].tobytes()
    # a failed cluster has stopped: the next step leaves it alone
    failed = np.int32([[ref.FAILED, 5, 3, -1], [0, 0, 0, 0]])
    status, T, st, _, clean, _ = run_step(gpu, m, labels, 2, tgt, d2, idx, T0, failed)
    assert status == 0 and clean and T[0].tobytes() == T0[0].tobytes() and st[0].tolist() == [ref.FAILED, 5, 3, -1] and st[1, 1] > 0


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------
def fit_both(dev, pc0, pc1, g0, g1, P0, P1, hand=False, **kw):
    import torch
    from himo_amd.icpflow import IcpFlow, IcpParams
    from himo_amd.seflow.ssl_label import _moved
    icp = IcpFlow(dev, IcpParams(**kw), **(HAND if hand else {}))
    flow = icp.fit(pc0, pc1, g0, g1, P0, P1).cpu().numpy()
    a = None
    if len(pc0):                                                   # rule 0 names the device's call as the definition of `a`
        T = np.linalg.inv(np.asarray(P1, np.float64)) @ np.asarray(P0, np.float64)
        a = _moved(torch.from_numpy(np.ascontiguousarray(pc0, dtype=np.float32)).to(dev), T).cpu().numpy()
    want = ref.fit(pc0, pc1, g0, g1, P0, P1, a=a, **(HAND if hand else {}), **kw)
    assert flow.shape == (len(pc0), 3) and flow.dtype == np.float32
    assert np.array_equal(icp.last_labels, want["labels"])
    assert np.array_equal(icp.last_status, want["status"]), (icp.last_status.tolist(), want["status"].tolist())
    err = float(np.abs(flow - want["flow"]).max(initial=0.0))
    assert err <= 1e-4, err
    ident = np.ones(len(pc0), bool)
    for k in np.flatnonzero(want["status"][:, 0] == ref.ACCEPTED):
        ident &= want["labels"] != k + 1
    assert flow[ident].tobytes() == want["ego_flow"][ident].tobytes()
    return icp, flow, want, err


@pytest.mark.parametrize("yaw, t, peak", [(5.0, (2.0, 0.5, 0.1), [8, 2]), (0.0, (3.5, 0.0, 0.0), [14, 0])])
def test_fit_hand_scenes(gpu, yaw, t, peak):
    pc0, pc1, g0, g1, P0, P1, disp = ref.hand_scene(yaw, t)
    icp, flow, want, _ = fit_both(gpu, pc0, pc1, g0, g1, P0, P1, hand=True)
    assert icp.last_status.tolist() == [[ref.ACCEPTED, 29, *peak], [ref.ACCEPTED, 29, 0, 0]]
    assert np.abs(flow[:29].astype(np.float64) - disp).max() <= 1e-4 and np.abs(flow[29:]).max() <= 1e-4
    assert np.abs(icp.last_transforms[0] - [np.cos(np.deg2rad(yaw)), np.sin(np.deg2rad(yaw)), *t]).max() <= 1e-6


@pytest.mark.parametrize("pose1", [None, EGO], ids=["identity", "ego"])
def test_fit_seeded_pair(gpu, pose1):
    args = ref.seeded_pair(SEED, 3000, 12, pose1)
    icp, flow, want, err = fit_both(gpu, *args)
    st = icp.last_status
    print(f"\nseeded pair: {len(st)} clusters, states {np.bincount(st[:, 0], minlength=3).tolist()}, max |flow - restatement| = {err:.3e} m")
    assert len(st) >= 12 and (np.abs(icp.last_transforms[:, 2:4]).max(1) > 0.5).sum() >= 6
    again = icp.fit(*args).cpu().numpy()
    assert again.tobytes() == flow.tobytes()                       # the same inputs give the same bytes


def test_fit_failure_rejection_and_degenerate_sweeps(gpu):
    pc0, pc1, g0, g1, P0, P1, _ = ref.hand_scene(0.0, (1.0, 0.25, 0.0))
    for kept, kw, state in ((15, {}, ref.ACCEPTED), (14, {}, ref.REJECTED), (8, dict(min_ratio=0.2), ref.ACCEPTED), (7, dict(min_ratio=0.2), ref.FAILED)):
        part = np.concatenate([pc1[29 - kept:29], pc1[29:]])
        icp, flow, want, _ = fit_both(gpu, pc0, part, g0, np.zeros(len(part), bool), P0, P1, hand=True, max_dist=0.25, **kw)
        assert icp.last_status[0].tolist() == [state, kept, 4, 1]
    pose1 = ref.yaw_pose(1.5, (0.8, -0.1, 0.0))
    inv1 = np.linalg.inv(pose1)
    only_static = (pc1[29:].astype(np.float64) @ inv1[:3, :3].T + inv1[:3, 3]).astype(np.float32)
    icp, flow, want, _ = fit_both(gpu, pc0, only_static, g0, np.zeros(29, bool), np.eye(4), pose1, hand=True)
    assert icp.last_status[0].tolist() == [ref.FAILED, 0, 0, 0] and np.abs(flow[:29]).max() > 0.5
    none = np.zeros((0, 3), np.float32)
    icp, flow, _, _ = fit_both(gpu, none, pc1, np.zeros(0, bool), g1, P0, P1, hand=True)             # an empty pc0
    assert flow.shape == (0, 3) and icp.last_status.shape == (0, 4)
    icp, flow, _, _ = fit_both(gpu, pc0, none, g0, np.zeros(0, bool), P0, pose1, hand=True)          # an empty pc1: every cluster fails
    assert (icp.last_status[:, 0] == ref.FAILED).all() and len(icp.last_status) == 2
    icp, flow, want, _ = fit_both(gpu, pc0, pc1, np.ones(58, bool), np.ones(58, bool), P0, pose1, hand=True)     # all ground
    assert icp.last_status.shape == (0, 4) and flow.tobytes() == want["ego_flow"].tobytes()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.icpflow import _CParams
    lib = _lib.load()
    INV, WS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_WORKSPACE
    pts, labels, tgt = ref.vote_case(51, 300, 4)
    need = int(lib.himo_icp_workspace_bytes(len(tgt), 4))
    bad_p = _CParams(0.25, 65, 1.0, 1.0, 8, 0.5, 10)
    nan_p = _CParams(float("nan"), 16, 1.0, 1.0, 8, 0.5, 10)
    beyond = offsets_of(labels, 4)
    beyond[4] -= 3                                                 # three rows past the last cluster: a label >= n_clusters + 1
    down = offsets_of(labels, 4)
    down[2] = down[1] - 1
    cases = [(dict(pitch=2), INV), (dict(pitch=5), INV), (dict(n=-1), INV), (dict(nt=-1), INV), (dict(C=-1), INV), (dict(h_off=beyond.ctypes.data), INV),
             (dict(h_off=down.ctypes.data), INV), (dict(h_off=None), INV), (dict(d_off=None), INV), (dict(pts=None), INV), (dict(tgt=None), INV),
             (dict(counts=None), INV), (dict(peak=None), INV), (dict(T=None), INV), (dict(st=None), INV), (dict(params=None), INV),
             (dict(params=ctypes.addressof(bad_p)), INV), (dict(params=ctypes.addressof(nan_p)), INV), (dict(ws=None), WS), (dict(ws_bytes=need - 1), WS),
             (dict(ws_bytes=0), WS)]
    for call, status in cases:
        st, counts, peak, T, words, clean, untouched = run_vote(gpu, pts, labels, 4, tgt, call=call)
        assert st == status, call
        assert clean and untouched, call
    st, *_, clean, untouched = run_vote(gpu, pts, labels, 4, tgt)
    assert st == 0 and clean and not untouched

    m, lab, tg, d2, idx = ref.step_case(65)
    T0, st0 = np.array([[1.0, 0.0, 0.0, 0.0, 0.0]] * 2), np.zeros((2, 4), np.int32)
    need = int(lib.himo_icp_workspace_bytes(len(tg), 2))
    short = offsets_of(lab, 2)
    short[2] -= 1
    for call, status in [(dict(n=-1), INV), (dict(C=-1), INV), (dict(nt=-1), INV), (dict(h_off=short.ctypes.data), INV), (dict(h_off=None), INV),
                         (dict(d_off=None), INV), (dict(m=None), INV), (dict(tgt=None), INV), (dict(idx=None), INV), (dict(d2=None), INV),
                         (dict(T=None), INV), (dict(st=None), INV), (dict(params=None), INV), (dict(params=ctypes.addressof(bad_p)), INV),
                         (dict(ws=None), WS), (dict(ws_bytes=need - 1), WS)]:
        status_got, T, st, inl, clean, unchanged = run_step(gpu, m, lab, 2, tg, d2, idx, T0, st0, call=call)
        assert status_got == status, call
        assert clean and unchanged, call
    assert run_step(gpu, m[:0], lab[:0], 0, tg, d2[:0], idx[:0], T0[:0], st0[:0])[0] == 0          # C = 0

    a, base, out = Buf(gpu, m), Buf(gpu, m), Buf(gpu, shape=(len(m), 3), dtype=np.float32)
    labs, Tb, sb = Buf(gpu, lab), Buf(gpu, T0), Buf(gpu, st0)
    ok = dict(n=len(m), pts=a.ptr, pitch=3, lab=labs.ptr, C=2, T=Tb.ptr, st=sb.ptr, mode=1, base=base.ptr, bp=3, out=out.ptr)
    for call in (dict(pitch=2), dict(pitch=6), dict(n=-1), dict(C=-1), dict(mode=2), dict(bp=5), dict(pts=None), dict(out=None), dict(base=None),
                 dict(lab=None), dict(T=None), dict(st=None)):
        c = dict(ok, **call)
        got = lib.himo_icp_apply(c["n"], c["pts"], c["pitch"], c["lab"], c["C"], c["T"], c["st"], c["mode"], c["base"], c["bp"], c["out"], _lib.stream_handle())
        torch.cuda.synchronize()
        assert got == INV and out.untouched(), call
    # labels outside 1 .. C are the identity, never an index
    wild = Buf(gpu, np.int32([0, 3, -7, 2 ** 31 - 1] * 5))
    got = lib.himo_icp_apply(20, a.ptr, 3, wild.ptr, 2, Tb.ptr, sb.ptr, 0, None, 0, out.ptr, _lib.stream_handle())
    torch.cuda.synchronize()
    assert got == 0 and out.guards_clean() and out.get()[:20].tobytes() == m[:20].tobytes()


# ---- 5. the chain ---------------------------------------------------------------------------------------------------------------------
def test_scenes_to_ground_masks_to_icpflow_to_zip_to_eval(gpu, tmp_path):
    from himo_amd import ground_seg, h5lite, save
    from test_ground_seg_gpu import H, _scenes_without_masks
    root = tmp_path / "av2_scenes"
    clouds = _scenes_without_masks(root)
    with pytest.raises(KeyError, match="himo_amd.ground_seg"):
        save.main(dataset_path=str(root), model="icpflow")
    ground_seg.main(str(root), sensor_height=H, batch=3)
    done = save.main(dataset_path=str(root), model="icpflow")
    assert done == 4                                               # two scenes of three sweeps: the last of each has no successor
    written = 0
    for sc in ("gs0", "gs1"):
        with h5lite.File(root / f"{sc}.h5") as f:
            for ts in sorted(f.keys()):
                if "icpflow" in f[ts]:
                    flow = f[ts]["icpflow"][:]
                    assert flow.dtype == np.float32 and flow.shape == (len(clouds[(sc, ts)]), 3) and np.isfinite(flow).all()
                    written += 1
    assert written == 4
    env = dict(os.environ, PYTHONPATH=str(REPO))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    tables = {}
    for mod, res in (("himo_amd.save_zip", "icpflow"), ("himo_amd.eval", "icpflow"), ("himo_amd.eval", "raw")):
        cwd = tmp_path / f"{mod.split('.')[-1]}_{res}"
        cwd.mkdir()
        run = subprocess.run([sys.executable, "-m", mod, "--data_dir", str(root), "--res_name", res], env=env, cwd=cwd,
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (mod, res, run.stderr[-3000:])
        if mod.endswith("eval"):
            tables[res] = list(_numbers(json.loads((cwd / "res-av2.json").read_text())))
    assert list(tmp_path.rglob("*.zip")), "save_zip wrote no archive"
    # a finite table: every figure that the data fills at all (finite under the zero-motion key `raw`) is finite under `icpflow`
    assert len(tables["icpflow"]) == len(tables["raw"]) > 0 and np.isfinite(tables["icpflow"]).any()
    assert all(np.isfinite(v) for v, r in zip(tables["icpflow"], tables["raw"]) if np.isfinite(r))


def _numbers(tree):
    if isinstance(tree, dict):
        for v in tree.values():
            yield from _numbers(v)
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            yield from _numbers(v)
    elif isinstance(tree, (int, float)) and not isinstance(tree, bool):
        yield float(tree)
