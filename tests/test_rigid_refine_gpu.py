"""The cluster-rigid refinement on the GPU against the numpy restatement of its written rule (tests/rigidrefine_ref.py; the reference
has no such stage: parity unpinned).  The restatement is fed the DEVICE's labels, so the clustering is not tested again; every case
first asserts the restatement's own margins (tests/test_rigid_refine_cpu.py shows them for the seeded scenes), then
    states, inlier counts, vote peaks and the per-row claim     exactly,
    transforms                                                  to 1e-9 absolute (float64 summation order only: <= n 2^-53 relative at
                                                                n <= 4096, three orders left for the cancellation in q_bar - R a_bar at
                                                                |a| <= 73 m),
    claimed rows                                                to one float32 ulp of the coordinate of R a + t (its last rounding may fall
                                                                either side when the float64 values differ by 1e-9),
    every other row                                             as int32 views equal to the input's bytes.
``himo_rigid_refine`` is also driven directly, with every output buffer between guard words."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rigidrefine_ref as ref
from conftest import REPO
from test_icpflow_gpu import Buf             # a device array between guard words

pytestmark = pytest.mark.gpu


def device_refine(dev, sc, kw, ctor):
    """the library call: dict(flow, status, transforms, claim, labels, a)"""
    import torch
    from himo_amd.rigid_refine import RigidParams, RigidRefine
    from himo_amd.seflow.ssl_label import _moved
    eng = RigidRefine(dev, RigidParams(**kw), **ctor)
    flow = eng.refine(sc["pc0"], sc["flow"], sc["gm0"], sc["pose0"], sc["pose1"])
    a = np.zeros((0, 3), np.float32)
    if len(sc["pc0"]):                                             # step 0 names the device's call as the definition of `a`
        T = np.linalg.inv(np.asarray(sc["pose1"], np.float64)) @ np.asarray(sc["pose0"], np.float64)
        a = _moved(torch.from_numpy(np.ascontiguousarray(sc["pc0"], dtype=np.float32)).to(dev), T).cpu().numpy()
    assert eng.last_clusters == len(eng.last_status)
    return dict(flow=flow.cpu().numpy(), status=eng.last_status, transforms=eng.last_transforms, claim=eng.last_claim, labels=eng.last_labels, a=a)


def raw_refine(dev, sc, a, labels, kw, call=None, ws_bytes=None, c_params=None):
    """himo_rigid_refine itself between guard words: (status code, dict of outputs, guards clean?, outputs untouched?)"""
    import torch
    from himo_amd import _lib
    from himo_amd.rigid_refine import RigidParams
    lib = _lib.load()
    rule = RigidParams(**kw)
    cp = c_params if c_params is not None else rule.c_struct()
    M, half = int(rule.models), int(rule.half)
    pc0, flow = np.ascontiguousarray(sc["pc0"], np.float32), np.ascontiguousarray(sc["flow"], np.float32)
    n, labels = len(pc0), np.asarray(labels, np.int32)
    C = int(labels.max(initial=0))
    order = np.argsort(np.where(labels > 0, labels, np.iinfo(np.int32).max), kind="stable").astype(np.int64)
    h_off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C + 1)[1:C + 1])]).astype(np.int64)
    nc = int(h_off[C])
    need = int(lib.himo_rigid_refine_workspace_bytes(nc, C, half, M))
    bufs = dict(pc0=Buf(dev, pc0), flow=Buf(dev, flow), a=Buf(dev, np.ascontiguousarray(a, np.float32)), labels=Buf(dev, labels),
                rows=Buf(dev, order[:nc]), off=Buf(dev, h_off), st=Buf(dev, shape=(C, M, 4), dtype=np.int32),
                T=Buf(dev, shape=(C, M, 5), dtype=np.float64), claim=Buf(dev, shape=(n,), dtype=np.int8),
                out=Buf(dev, shape=(n, 3), dtype=np.float32), ws=Buf(dev, shape=(max(need, 16),), dtype=np.uint8))
    c = dict(n=n, pc0=bufs["pc0"].ptr, pitch=pc0.shape[1], flow=bufs["flow"].ptr, a=bufs["a"].ptr, labels=bufs["labels"].ptr, nc=nc,
             rows=bufs["rows"].ptr, C=C, h_off=h_off.ctypes.data, d_off=bufs["off"].ptr, params=ctypes.addressof(cp), st=bufs["st"].ptr,
             T=bufs["T"].ptr, claim=bufs["claim"].ptr, out=bufs["out"].ptr, ws=bufs["ws"].ptr, ws_bytes=need if ws_bytes is None else ws_bytes)
    c.update(call or {})
    code = lib.himo_rigid_refine(c["n"], c["pc0"], c["pitch"], c["flow"], c["a"], c["labels"], c["nc"], c["rows"], c["C"], c["h_off"], c["d_off"],
                                 c["params"], c["st"], c["T"], c["claim"], c["out"], c["ws"], c["ws_bytes"], _lib.stream_handle())
    torch.cuda.synchronize()
    clean = all(b.guards_clean() for b in bufs.values())
    untouched = all(bufs[k].untouched() for k in ("st", "T", "claim", "out", "ws"))
    got = dict(flow=bufs["out"].get(), status=bufs["st"].get(), transforms=bufs["T"].get(), claim=bufs["claim"].get())
    return code, got, clean, untouched, need


def assert_margins(want):
    m = want["margins"]
    assert m["e2"] > 1e-6 and m["static"] > 1e-6 and m["ratio"] > 1e-6 and m["count"] >= 1, m


def assert_equals_the_restatement(got, want, sc, labels, what=""):
    assert got["flow"].shape == (len(sc["pc0"]), 3) and got["flow"].dtype == np.float32
    assert np.array_equal(got["status"], want["status"]), (what, got["status"].tolist(), want["status"].tolist())
    assert np.array_equal(got["claim"], want["claim"]), (what, int((got["claim"] != want["claim"]).sum()))
    err_T = float(np.abs(got["transforms"] - want["transforms"]).max(initial=0.0))
    assert err_T <= 1e-9, (what, err_T)
    kept = want["claim"] == 0
    assert got["flow"][kept].view(np.int32).tobytes() == np.asarray(sc["flow"], np.float32)[kept].view(np.int32).tobytes(), what
    off, rows = 0, np.flatnonzero(~kept)
    if len(rows):
        T = want["transforms"][labels[rows] - 1, want["claim"][rows] - 1]
        a = want["a"][rows].astype(np.float64)
        m = np.stack([(T[:, 0] * a[:, 0] - T[:, 1] * a[:, 1]) + T[:, 2], (T[:, 1] * a[:, 0] + T[:, 0] * a[:, 1]) + T[:, 3], a[:, 2] + T[:, 4]],
                     axis=1).astype(np.float32)
        diff = np.abs(got["flow"][rows].astype(np.float64) - want["flow"][rows].astype(np.float64))
        assert (diff <= np.spacing(np.abs(m)).astype(np.float64)).all(), (what, float(diff.max()))
        off = int((diff > 0).sum())
    # a static round's rows: the ego-motion flow, bit for bit
    static = np.zeros(len(kept), bool)
    for k, j in zip(*np.nonzero(want["status"][:, :, 0] == ref.STATIC)):
        static |= (labels == k + 1) & (want["claim"] == j + 1)
    assert got["flow"][static].tobytes() == want["ego_flow"][static].tobytes(), what
    return err_T, off


def check_case(dev, sc, kw=None, ctor=None, expect_labels=True):
    """library call and raw call against the restatement on the device's labels; -> (device result, restatement)"""
    kw, ctor = kw or {}, ctor or {}
    got = device_refine(dev, sc, kw, ctor)
    if expect_labels:
        assert np.array_equal(got["labels"], sc["labels"]), "the device's clusters are not the ones the scene was built from"
    want = ref.refine(sc["pc0"], sc["flow"], sc["gm0"], sc["pose0"], sc["pose1"], got["labels"], a=got["a"], **kw)
    assert_margins(want)
    err_T, off = assert_equals_the_restatement(got, want, sc, got["labels"], "library")
    code, raw, clean, _, _ = raw_refine(dev, sc, got["a"], got["labels"], kw)
    assert code == 0 and clean
    for k in ("flow", "status", "transforms", "claim"):            # the same inputs give the same bytes, through either door
        assert raw[k].tobytes() == got[k].tobytes(), k
    states = np.bincount(want["status"][:, :, 0].ravel(), minlength=5).tolist()
    print(f"\n{len(sc['pc0'])} rows, {len(want['status'])} clusters, rounds by state {states}: max |T - restatement| = {err_T:.3e}, "
          f"{off} claimed coordinates one ulp off")
    return got, want


# ---- 1. degenerate sweeps -----------------------------------------------------------------------------------------------------------------
def test_empty_all_ground_and_clusterless_sweeps(gpu):
    none = dict(pc0=np.zeros((0, 3), np.float32), flow=np.zeros((0, 3), np.float32), gm0=np.zeros(0, bool), pose0=np.eye(4), pose1=ref.EGO,
                labels=np.zeros(0, np.int32))
    got, _ = check_case(gpu, none)
    assert got["flow"].shape == (0, 3) and got["status"].shape == (0, 2, 4) and got["transforms"].shape == (0, 2, 5)
    ground = ref.build_scene([dict(n=5, centre=(3.0, 1.0, -1.7), dims=(0.3, 0.3, 0.05), ground=True, t=(1.0, 0.0, 0.0))], seed=1)
    got, _ = check_case(gpu, ground)
    assert got["status"].shape == (0, 2, 4) and got["flow"].tobytes() == ground["flow"].tobytes() and not got["claim"].any()
    rng = np.random.default_rng(2)
    lone = ref.build_scene([dict(n=1, centre=(x, y, 0.3), t=(1.0, 0.5, 0.0), cluster=None) for x, y in rng.uniform(-40, 40, (40, 2)).round()], seed=3)
    lone["labels"][:] = 0                                          # 40 participating points at least a metre apart: no cluster
    got, _ = check_case(gpu, lone)
    assert got["status"].shape == (0, 2, 4) and got["flow"].tobytes() == lone["flow"].tobytes()


# ---- 2 .. 7. the seeded cases ---------------------------------------------------------------------------------------------------------------
def test_cluster_of_exactly_min_inliers_and_one_below(gpu):
    build, kw, ctor = ref.CASES["eight"]
    got, _ = check_case(gpu, build(), kw, ctor)
    assert got["status"][0, 0].tolist()[:2] == [ref.ACCEPTED, 8] and (got["claim"] == 1).all()
    build, kw, ctor = ref.CASES["seven"]
    sc = build()
    got, _ = check_case(gpu, sc, kw, ctor)
    assert got["status"][0].tolist() == [[ref.FAILED, 7, 2, 1], [ref.NOT_RUN, 0, 0, 0]] and got["flow"].tobytes() == sc["flow"].tobytes()


def test_cluster_sizes_around_the_wave_the_block_and_their_split_and_many_small_clusters(gpu):
    build, kw, ctor = ref.CASES["sizes"]
    sc = build()
    assert sc["pc0"].shape[1] == 4                                 # (a sweep with its intensity column: pitch 4)
    got, want = check_case(gpu, sc, kw, ctor)
    assert np.bincount(got["labels"])[1:8].tolist() == list(ref.SIZES) and len(got["status"]) == len(ref.SIZES) + ref.N_SMALL
    assert (got["status"][:, 0, 0] == ref.ACCEPTED).all() and (got["claim"] == 1).sum() > 4600
    # two runs: identical bytes in every output
    again = device_refine(gpu, sc, kw, ctor)
    for k in ("flow", "status", "transforms", "claim", "labels"):
        assert again[k].tobytes() == got[k].tobytes(), k


def test_merged_clusters_claim_in_the_votes_order_and_a_third_part_stays(gpu):
    build, kw, ctor = ref.CASES["merged"]
    sc = build()
    got, _ = check_case(gpu, sc, kw, ctor)
    assert got["status"][:, :, 0].tolist() == [[ref.STATIC, ref.ACCEPTED], [ref.STATIC, ref.ACCEPTED], [ref.ACCEPTED, ref.ACCEPTED]]
    assert got["status"][:2, :, 1].tolist() == [[120, 180], [180, 120]]
    third = sc["part"] == 6
    assert not got["claim"][third].any() and got["flow"][third].tobytes() == sc["flow"][third].tobytes()


def test_static_cluster_gets_the_ego_motion_flow_bit_for_bit(gpu):
    build, kw, ctor = ref.CASES["static"]
    sc = build()
    got, want = check_case(gpu, sc, kw, ctor)
    assert got["status"][0, 0].tolist() == [ref.STATIC, 120, 0, 0] and got["transforms"][0, 0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert got["flow"].tobytes() == want["ego_flow"].tobytes() and got["flow"].tobytes() != sc["flow"].tobytes()


def test_pass_through_rows_keep_their_bytes(gpu):
    build, kw, ctor = ref.CASES["passthrough"]
    sc = build()
    got, _ = check_case(gpu, sc, kw, ctor)
    assert got["status"][:, 0].tolist() == [[ref.ACCEPTED, 146, 4, 2], [ref.FAILED, 0, 0, 0]]       # 5 m: no votes, start (0, 0), failed
    kept = got["claim"] == 0
    assert kept.sum() == 4 + 60 + 80 + 90 and (got["claim"][:150] == 1).sum() == 146
    assert got["flow"][kept].view(np.int32).tobytes() == sc["flow"][kept].view(np.int32).tobytes()
    assert np.isfinite(got["flow"][~kept]).all()


def test_hdbscan_clusters(gpu):
    build, kw, ctor = ref.CASES["hdbscan"]
    got, _ = check_case(gpu, build(), kw, ctor)
    assert got["status"][:, 0, 0].tolist() == [ref.ACCEPTED, ref.STATIC, ref.ACCEPTED]


def test_other_parameters_and_the_counters_that_do_not_fit_the_lds(gpu):
    sc = ref.merged_scene()
    for kw in (dict(half=22), dict(half=23), dict(half=45), dict(half=64), dict(models=1), dict(models=4, min_ratio=0.2), dict(bin=0.1, half=40),
               dict(tol=0.15, iters=1, min_inliers=30), dict(static_disp=0.001)):
        check_case(gpu, sc, kw)
    # ... and a cluster that a block owns, with its counters in the workspace
    big = ref.build_scene([dict(n=1500, centre=(10.0, 5.0, 0.5), t=(2.1, -1.3, 0.05), yaw=0.04, cluster="b"),
                           dict(n=1100, centre=(10.0, 5.0 + 1.5, 0.5), cluster="b")], seed=91)
    for kw in (dict(), dict(half=50)):
        got, _ = check_case(gpu, big, kw)
        assert sorted(got["status"][0, :, 0].tolist()) == [ref.ACCEPTED, ref.STATIC]


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu):
    from himo_amd import _lib
    from himo_amd.rigid_refine import _CParams
    INV, WS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_WORKSPACE
    sc = ref.merged_scene()
    a, labels = ref.moved(sc["pc0"], sc["pose0"], sc["pose1"]), sc["labels"]
    code, _, clean, untouched, need = raw_refine(gpu, sc, a, labels, {})
    assert code == 0 and clean and not untouched
    half65, models5 = _CParams(0.25, 65, 0.25, 5, 8, 0.25, 0.05, 2), _CParams(0.25, 16, 0.25, 5, 8, 0.25, 0.05, 5)
    nan_tol, no_iters = _CParams(0.25, 16, float("nan"), 5, 8, 0.25, 0.05, 2), _CParams(0.25, 16, 0.25, 0, 8, 0.25, 0.05, 2)
    C = int(labels.max())
    short = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C + 1)[1:])]).astype(np.int64)
    short[C] -= 1
    down = short.copy()
    down[C] += 1
    down[1] = down[2] + 1
    cases = [(dict(c_params=half65), INV), (dict(c_params=models5), INV), (dict(c_params=nan_tol), INV), (dict(c_params=no_iters), INV),
             (dict(ws_bytes=need - 1), WS), (dict(ws_bytes=0), WS), (dict(call=dict(ws=None)), WS), (dict(call=dict(params=None)), INV),
             (dict(call=dict(pitch=2)), INV), (dict(call=dict(pitch=5)), INV), (dict(call=dict(n=-1)), INV), (dict(call=dict(nc=-1)), INV),
             (dict(call=dict(nc=len(a) + 1)), INV), (dict(call=dict(C=-1)), INV), (dict(call=dict(C=0)), INV),
             (dict(call=dict(h_off=short.ctypes.data)), INV), (dict(call=dict(h_off=down.ctypes.data)), INV), (dict(call=dict(h_off=None)), INV),
             (dict(call=dict(d_off=None)), INV), (dict(call=dict(pc0=None)), INV), (dict(call=dict(flow=None)), INV), (dict(call=dict(a=None)), INV),
             (dict(call=dict(labels=None)), INV), (dict(call=dict(rows=None)), INV), (dict(call=dict(st=None)), INV), (dict(call=dict(T=None)), INV),
             (dict(call=dict(claim=None)), INV), (dict(call=dict(out=None)), INV)]
    for how, status in cases:
        code, _, clean, untouched, _ = raw_refine(gpu, sc, a, labels, {}, **how)
        assert code == status, how
        assert clean and untouched, how


# ---- 10. the program, end to end ------------------------------------------------------------------------------------------------------------
def test_program_refines_stored_flows_and_eval_reads_them(gpu, tmp_path, capsys):
    from himo_amd import rigid_refine
    from himo_amd.dataset import open_dataset
    from himo_amd.save import H5ResultSink
    from himo_amd.synthetic import make_scene, write_h5_scenes
    root = tmp_path / "av2_scenes"                              # (eval names the dataset by its path)
    root.mkdir()
    scenes = [make_scene(seed, 3, n_points=4000, n_instances=8, scene_id=f"rr{seed}") for seed in (1, 2)]
    write_h5_scenes(root, scenes)
    sink = H5ResultSink(root, "noisy")
    rng = np.random.default_rng(5)
    for frames in scenes:
        for k, f in enumerate(frames[:2]):                         # the last sweep of a scene has no successor, and no result
            sink(k, f, (f["flow"] + rng.normal(0.0, 0.05, f["flow"].shape)).astype(np.float32))
    sink.close()
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        os.environ.pop(k, None)
    totals = rigid_refine.main(str(root), "noisy")
    line = capsys.readouterr().out.strip().splitlines()[-1]
    print(line)
    assert totals["sweeps"] == 4 and totals["skipped"] == 0 and totals["clusters"] > 8 and totals["rounds"]["accepted"] > 8
    assert "4 sweeps" in line and f"{totals['clusters']} clusters" in line and "accepted" in line
    ds = open_dataset(root, vis_name=["noisy", "noisy_rigid"], fields=("pc0", "flow", "flow_instance_id", "noisy", "noisy_rigid"))
    assert len(ds) == 4
    err = {"noisy": [], "noisy_rigid": []}
    for i in range(len(ds)):
        f = ds[i]
        assert f["noisy_rigid"].shape == f["noisy"].shape == (4000, 3) and f["noisy_rigid"].dtype == np.float32
        inst = np.asarray(f["flow_instance_id"]).astype(np.int64)
        rows = (inst > 0) & (np.bincount(inst)[inst] >= 50)
        for name in err:
            err[name].append(np.linalg.norm(np.asarray(f[name])[rows].astype(np.float64) - np.asarray(f["flow"])[rows], axis=1))
    ds.close()
    before, after = (float(np.concatenate(err[k]).mean()) for k in ("noisy", "noisy_rigid"))
    print(f"instances of >= 50 points: MPE {before:.4f} m under 'noisy', {after:.4f} m under 'noisy_rigid'")
    assert after < before
    with pytest.raises(FileExistsError, match="--overwrite"):      # a second run refuses ...
        rigid_refine.main(str(root), "noisy")
    assert rigid_refine.main(str(root), "noisy", overwrite=True)["sweeps"] == 4          # ... unless told to replace
    env = dict(os.environ, PYTHONPATH=str(REPO))
    run = subprocess.run([sys.executable, "-m", "himo_amd.eval", "--data_dir", str(root), "--res_name", "noisy_rigid"], env=env, cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    table = json.loads(next(tmp_path.glob("res-*.json")).read_text())
    assert table
