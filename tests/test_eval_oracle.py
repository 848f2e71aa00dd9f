"""The checker of the instance evaluator and the exact NN search (oracle/eval_oracle.py), on CPU.  The oracle demands equal bits of
csrc/evalmetrics.hip and csrc/nn.hip, so what has to be shown here is that it says what the reference says and that it would catch a
wrong kernel:

  * its records, run through the package's own host bookkeeping, give the reference's numbers (oracle/himo_oracle.py: eval_frame,
    InstanceMetrics.step_eval, ScoreMetrics.step, nearest_neighbor) within TOL = 1e-9, the bar of tests/test_eval_gpu.py, on the golden
    frames; on the cases of its matrix where the reference's semantics apply, instance by instance;
  * the check functions tests/test_eval_conformance_gpu.py applies pass the restatement's own output;
  * each wrong variant -- the restatement with one line changed -- fails those checks on a named case;
  * every case reaches the paths it names (proved with the kernels' own index arithmetic).
"""
import json

import numpy as np
import pytest

import compdis_oracle as co
import eval_oracle as eo
import himo_oracle as ho
from conftest import RES, golden_frames

F32, F64 = np.float32, np.float64
TOL = 1e-9                                                      # tests/test_eval_gpu.py


SCORE_MPE_TOL = 2e-6                                           # tests/test_score_gpu.py: the reference's cal_mpe is a FLOAT32 mean (score.py:197)


def _approx_tree(got, ref, path="", mpe_tol=TOL):
    if isinstance(ref, dict):
        assert set(got) == set(ref), path
        for k in ref:
            _approx_tree(got[k], ref[k], f"{path}/{k}", mpe_tol)
    elif isinstance(ref, list):
        assert len(got) == len(ref), path
        for i, (g, r) in enumerate(zip(got, ref)):
            _approx_tree(g, r, f"{path}[{i}]", mpe_tol)
    elif isinstance(ref, float):
        tol = mpe_tol if "mpe" in path else TOL
        assert got == pytest.approx(ref, rel=tol, abs=TOL), path
    else:
        assert got == ref, path


def _tree(m):
    return json.loads(json.dumps(m.evaluate_data, default=float))


def _reference_lut():
    lut = np.zeros(256, np.uint8)
    for gid, name in enumerate(("CAR", "OTHER_VEHICLES"), start=1):
        for cat in ho.BUCKETED_METACATAGORIES[name]:
            lut[ho.CATEGORY_TO_INDEX[cat]] = gid
    return lut


def _case(mode, stride, sensor_dt=0.1, **kw):
    c = dict(mode=mode, stride=stride, pose_is_ego=False, est_is_dis=False, has_pc=True, has_dt=True, sensor_dt=sensor_dt)
    c.update(kw)
    return c


def _golden_data(frames, data_name, mode, est_list):
    sizes = [len(f["pc0"]) for f in frames]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    cat = lambda k, t: np.ascontiguousarray(np.concatenate([np.asarray(f[k]) for f in frames]).astype(t))
    pc = cat("pc0", F32)
    est = np.ascontiguousarray(np.concatenate(est_list).astype(F32)) if est_list is not None else np.zeros((len(pc), 3), F32)
    mask = np.concatenate([ho.eval_mask(f, data_name) for f in frames]).astype(np.uint8)
    return eo.make_data(_case(mode, pc.shape[1]), offsets, pc, cat("flow", F32), est, cat("lidar_dt", F32), cat("flow_category_indices", np.uint8),
                        cat("flow_instance_id", np.int64), mask, _reference_lut(), np.stack([f["pose0"] for f in frames]).astype(F64),
                        np.stack([f["pose1"] for f in frames]).astype(F64))


# ---- the reference's numbers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data_name", ["av2", "scania"])
@pytest.mark.parametrize("mode", ["flow", "raw", "zip"])
def test_records_give_eval_frame_of_the_reference(gold, data_name, mode):
    """eval_frame (eval.py:281-310) on the golden frames, all three ways of giving the estimate: the restatement's records through
    the package's host bookkeeping (himo_amd/eval.py _accumulate_frame) against himo_oracle.InstanceMetrics"""
    from himo_amd.eval import InstanceMetrics
    frames = golden_frames(gold, data_name)
    ref = ho.InstanceMetrics(data_name)
    cds = [ho.comp_dis_frame_f32(f, RES) for f in frames] if mode == "zip" else None
    for k, f in enumerate(frames):
        ho.eval_frame(ref, f, res_name="raw" if mode == "raw" else RES, comp_dis=None if cds is None else cds[k])
    d = _golden_data(frames, data_name, {"flow": eo.MODE_FLOW, "raw": eo.MODE_RAW, "zip": eo.MODE_COMPDIS}[mode],
                     cds if mode == "zip" else (None if mode == "raw" else [f[RES] for f in frames]))
    recs = eo.records(d)
    assert len(recs) > 0
    mine = InstanceMetrics(data_name)
    bounds = np.searchsorted(recs["frame"], np.arange(d.F + 1))
    for k in range(d.F):
        mine._accumulate_frame(recs[bounds[k]:bounds[k + 1]], key=k)
    assert mine.frame_cnt == ref.frame_cnt
    _approx_tree(_tree(mine), _tree(ref))
    # POSE_IS_EGO with numpy's own inverse: the same numbers
    d.c["pose_is_ego"] = True
    ego = eo.records(d)
    for k in eo.F64_FIELDS:
        assert np.allclose(ego[k], recs[k], rtol=TOL, atol=TOL, equal_nan=True)


@pytest.mark.parametrize("data_name", ["av2", "scania"])
def test_records_give_step_eval_of_the_reference(gold, data_name):
    """InstanceMetrics.step_eval's own arguments (eval.py:64): masked, ego-motion-free float64 flows, est_flow and est_dis"""
    from himo_amd.eval import InstanceMetrics
    mine, ref = InstanceMetrics(data_name), ho.InstanceMetrics(data_name)
    for f in golden_frames(gold, data_name):
        pf = ho.pose_flow(f["pc0"], f["pose0"], f["pose1"])
        gt_flow, est_flow = f["flow"] - pf, f[RES] - pf
        m = ho.eval_mask(f, data_name)
        dt0 = ho.dt0_from_lidar_dt(f["lidar_dt"])
        args = (f["pc0"][m, :], gt_flow[m, :], dt0[m], f["flow_category_indices"][m], f["flow_instance_id"][m])
        cd = ho.comp_dis_frame_f32(f, RES)
        for kw, est, is_dis in ((dict(est_flow=est_flow[m, :]), est_flow[m, :].astype(F64), False), (dict(est_dis=cd[m, :]), cd[m, :].astype(F32), True)):
            ref.step_eval(*args, **kw)
            n = int(m.sum())
            pc = np.ascontiguousarray(args[0], F32)
            d = eo.make_data(_case(eo.MODE_DIRECT, pc.shape[1], est_is_dis=is_dis), [0, n], pc, np.ascontiguousarray(args[1], F64), np.ascontiguousarray(est),
                             np.ascontiguousarray(args[2], F32), args[3], np.asarray(args[4]).astype(np.int64), np.ones(n, np.uint8), _reference_lut())
            mine._accumulate_frame(eo.records(d), key=mine.frame_cnt)
    assert mine.frame_cnt == ref.frame_cnt
    _approx_tree(_tree(mine), _tree(ref))


@pytest.mark.parametrize("have_norm,have_pc0", [(True, True), (True, False), (False, True), (False, False)])
def test_records_give_score_step_of_the_reference(gold, have_norm, have_pc0):
    """ScoreMetrics.step (tools/test/score.py:223-321) on the ground-truth writer's columns of the golden frames.  The Chamfer
    numbers within TOL; the reference's mpe is a float32 mean of float32 norms where the kernel sums the same float32 norms in float64,
    so against ScoreMetrics.step itself mpe is held to the scorer's existing bar (tests/test_score_gpu.py, 2e-6) and to TOL against
    the float64 mean of the reference's own float32 norms (test_cases_against_the_reference_expressions)"""
    from himo_amd.score import ScoreMetrics
    for data_name in ("av2", "scania"):
        mine, ref = ScoreMetrics(), ho.ScoreMetrics()
        for f in golden_frames(gold, data_name):
            g = ho.gt_frame(f, data_name)
            est = ho.comp_dis_frame_f32(f, RES)
            norm, pc0 = (g["gt_flow_norm"] if have_norm else None), (np.ascontiguousarray(g["pc0"], F32) if have_pc0 else None)
            ref.step(g["comp_dis"], est, g["eval_mask"], f["flow_category_indices"], f["flow_instance_id"], norm, pc0, data_name=data_name)
            n = len(est)
            d = eo.make_data(_case(eo.MODE_SCORE, 3, has_pc=have_pc0, has_dt=have_norm), [0, n], pc0, g["comp_dis"], est, norm,
                             f["flow_category_indices"], np.asarray(f["flow_instance_id"]).astype(np.int64), g["eval_mask"].astype(np.uint8), _reference_lut())
            mine.frame_cnt += 1
            mine._accumulate(eo.records(d), 1.5 if data_name == "scania" else 3.0, have_norm)
        assert mine.frame_cnt == ref.frame_cnt
        _approx_tree(_tree(mine), _tree(ref), mpe_tol=SCORE_MPE_TOL)
        assert sum(len(mine.evaluate_data[c]["mean"]["num_pts"]) for c in mine.evaluate_data) > 0


@pytest.mark.parametrize("nq,nr", [(1, 1), (10, 7), (257, 300), (3000, 1), (2000, 2049)])
def test_nn_search_gives_nearest_neighbor_of_the_reference(nq, nr):
    """float64: sqrt of the restatement's minimum equals cKDTree's distance (both form (dx*dx + dy*dy) + dz*dz); the rows name
    equally distant references"""
    rng = np.random.default_rng(nq * 31 + nr)
    q, r = rng.normal(size=(nq, 3)) * 5, rng.normal(size=(nr, 3)) * 5
    d2, idx = eo.nn_search(q, r, [0, nq], [0, nr], True)
    rd, ri = ho.nearest_neighbor(q, r)
    assert np.allclose(np.sqrt(d2), rd, rtol=TOL, atol=TOL)
    assert np.array_equal(np.linalg.norm(q - r[idx], axis=1), np.linalg.norm(q - r[ri], axis=1))
    # float32: the exact value from the float32 inputs
    q32, r32 = q.astype(F32), r.astype(F32)
    e2, _ = eo.nn_search(q32, r32, [0, nq], [0, nr], False)
    rd32, _ = ho.nearest_neighbor(q32.astype(F64), r32.astype(F64))
    assert np.allclose(np.sqrt(e2), rd32, rtol=TOL, atol=TOL)


def reference_records(d):
    """the per-instance numbers of a case as the reference's own expressions give them (himo_oracle: step_eval's loop body without its
    thresholds, ScoreMetrics.step's for the score mode), keyed (frame, group, id)"""
    c = d.c
    sdt, mode = c["sensor_dt"], c["mode"]
    out = {}
    rows, frame, group, id32 = eo.select(d)
    for f in np.unique(frame):
        a, b = int(d.offsets[f]), int(d.offsets[f + 1])
        pc = d.pc[a:b] if d.pc is not None else None
        if mode == eo.MODE_SCORE:
            gt_ref = (pc[:, :3] + d.gt[a:b]) if c["has_pc"] else d.gt[a:b]
            est_ref = (pc[:, :3] + d.est[a:b]) if c["has_pc"] else d.est[a:b]
        else:
            if mode == eo.MODE_DIRECT:
                gt_flow, dt0 = d.gt[a:b], d.dt[a:b]
                est_flow = None if c["est_is_dis"] else d.est[a:b]
            else:
                ego = d.given[f] if c["pose_is_ego"] else ho.ego_pose(d.pose0[f], d.pose1[f])
                pf = pc[:, :3] @ ego[:3, :3].T + ego[:3, 3] - pc[:, :3]
                gt_flow, dt0 = d.gt[a:b] - pf, ho.dt0_from_lidar_dt(d.dt[a:b])
                est_flow = None if mode == eo.MODE_COMPDIS else (np.zeros_like(pf) if mode == eo.MODE_RAW else d.est[a:b] - pf)
            gt_ref = ho.refine_pts(pc, ho.flow2compDis(gt_flow, dt0, sensor_dt=sdt))
            est_ref = ho.refine_pts(pc, d.est[a:b]) if est_flow is None else ho.refine_pts(pc, ho.flow2compDis(est_flow, dt0, sensor_dt=sdt))
        sel = frame == f
        for g, i in sorted(set(zip(group[sel].tolist(), id32[sel].tolist()))):
            m = rows[sel & (group == g) & (id32 == i)] - a
            if mode == eo.MODE_SCORE:
                vel = (np.mean(d.dt[a:b][m].astype(F64)) / sdt) if c["has_dt"] else 0.0
                dis, mpe = 0.0, np.linalg.norm(d.gt[a:b][m] - d.est[a:b][m], axis=1).astype(F64).mean()   # cal_mpe's float32 norms, a float64 mean
                assert mpe == pytest.approx(float(ho.cal_mpe(d.gt[a:b][m], d.est[a:b][m])), rel=SCORE_MPE_TOL)
            else:
                vel = np.linalg.norm(gt_flow[m], axis=1).mean() / sdt
                # eval.py:94 is a float32 mean of float32 norms (the host casts the record's dis to float32 before it buckets it,
                # himo_amd/eval.py:364); the kernel sums the same float32 norms in float64: TOL against THAT, float32 resolution against eval.py:94
                dis, mpe = np.linalg.norm(pc[m], axis=1).astype(F64).mean(), np.linalg.norm(gt_ref[m] - est_ref[m], axis=1).mean()
                assert dis == pytest.approx(float(np.linalg.norm(pc[m], axis=1).mean()), rel=SCORE_MPE_TOL)
            out[(int(f), g, i)] = (len(m), float(vel), float(dis), float(mpe), ho.cal_chamfer(gt_ref[m], est_ref[m]))
    return out


REFERENCE_CASES = [k for k in eo.CASE_NAMES if eo.CASES[k]["reference"]]


@pytest.mark.parametrize("name", REFERENCE_CASES)
def test_cases_against_the_reference_expressions(name):
    """every case whose operands the reference could be given (two class groups, ids below 2^32): instance by instance within TOL"""
    for ego_mode in ([False, True] if eo.CASES[name]["both_ego_modes"] else [None]):
        d = eo.build(name, ego_mode)
        recs, ref = eo.records(d), reference_records(d)
        assert len(recs) == len(ref) and (len(ref) > 0 or d.T == 0)
        for r in recs:
            n, vel, dis, mpe, cham = ref[(int(r["frame"]), int(r["group"]), int(r["instance"]))]
            assert int(r["num_pts"]) == n
            for k, want in (("vel", vel), ("dis", dis), ("mpe", mpe), ("cham", cham)):
                assert float(r[k]) == pytest.approx(want, rel=TOL, abs=TOL), (name, k, r)


# ---- the checks pass the restatement's own output, and fail every wrong variant ------------------------------------------------------
WRONG_ON = {"no_group": "ids_and_groups", "no_frame": "ids_and_groups", "dis3": "mode_flow_stride6", "one_sided": "mode_flow_stride4",
            "sqrt_after_mean": "mode_compdis_stride3", "vel_no_dt": "mode_direct_stride4"}
NN_WRONG_ON = {"ties_highest": "ties_q17", "range_end_plus_one": "segments_in_a_block"}


def test_the_checks_pass_the_restatement():
    for name in ("ids_and_groups", "mode_flow_stride6", "shared_slot_and_wrap", "empties_0_3_0_1_0"):
        d = eo.build(name)
        want = eo.records(d)
        rng = np.random.default_rng(1)
        assert eo.check_records(want[rng.permutation(len(want))], want, name) == 4 * len(want)
        M, K = len(eo.select(d)[0]), len(want)
        for room in (1, K - 1, K, K + 3):
            slots = want[rng.permutation(K)[:min(room, K)]]
            eo.check_overflow(slots, [M, K], want, M, room, name)
        with pytest.raises(AssertionError):
            eo.check_overflow(want[[0, 0]], [M, K], want, M, 2, name)              # a duplicate
        with pytest.raises(AssertionError):
            eo.check_overflow(want[:1], [M, K + 1], want, M, 1, name)              # a wrong count
        bad = want.copy()
        bad["cham"][0] = np.nextafter(bad["cham"][0], np.inf)
        with pytest.raises(AssertionError):
            eo.check_records(bad, want, name)                                      # one bit
        bad = want.copy()
        bad["num_pts"][-1] += 1
        with pytest.raises(AssertionError):
            eo.check_records(bad, want, name)


def test_the_search_checks_pass_the_restatement():
    for name in ("q17_r1025", "segments_in_a_block", "empty_reference_range", "ties_q17", "nan_query_and_reference", "ranges_far_apart"):
        c = eo.NN_CASES[name]
        q, r = eo.nn_build(name, True)
        d2, idx = eo.nn_search(q, r, c["q_off"], c["r_off"], True)
        assert eo.check_nn_f64(d2, idx, d2, idx, name) == c["nq"]
        if (idx >= 0).any():
            off = idx.copy()
            off[np.nonzero(idx >= 0)[0][0]] += 1
            with pytest.raises(AssertionError):
                eo.check_nn_f64(d2, off, d2, idx, name)
        q, r = eo.nn_build(name, False)
        e2, eidx = eo.nn_search(q, r, c["q_off"], c["r_off"], False)
        got = e2.astype(F32)                                                     # the exact value rounded once: inside the bound
        eo.check_nn_f32(got, eidx, q, r, e2, eidx, c["q_off"], c["r_off"], name)
        ok = np.nonzero((eidx >= 0) & (e2 > 0))[0]
        if len(ok):
            far = got.copy()
            far[ok[0]] *= F32(1 + 8 * eo.U24)
            with pytest.raises(AssertionError):
                eo.check_nn_f32(far, eidx, q, r, e2, eidx, c["q_off"], c["r_off"], name)
    # what the source does with a NaN: a NaN query matches nothing, a NaN reference is never matched
    c = eo.NN_CASES["nan_query_and_reference"]
    q, r = eo.nn_build("nan_query_and_reference", True)
    d2, idx = eo.nn_search(q, r, c["q_off"], c["r_off"], True)
    assert np.isposinf(d2[eo.NAN_QUERY]) and idx[eo.NAN_QUERY] == -1 and not (idx == eo.NAN_REFERENCE).any() and (idx[np.arange(len(idx)) != eo.NAN_QUERY] >= 0).all()
    # the lattice: the lowest of the rows that hold the same point, the same bits in both dtypes
    c = eo.NN_CASES["ties_q17"]
    q, r = eo.nn_build("ties_q17", True)
    d2, idx = eo.nn_search(q, r, c["q_off"], c["r_off"], True)
    q32, r32 = eo.nn_build("ties_q17", False)
    e2, eidx = eo.nn_search(q32, r32, c["q_off"], c["r_off"], False)
    assert np.array_equal(q, q32.astype(F64)) and np.array_equal(d2, e2) and np.array_equal(idx, eidx)
    assert set(idx.tolist()) == {rows[0] for rows in eo.TIE_ROWS}


@pytest.mark.parametrize("wrong", eo.WRONG)
def test_a_wrong_variant_fails(wrong):
    name = WRONG_ON[wrong]
    d = eo.build(name)
    with pytest.raises(AssertionError):
        eo.check_records(eo.records(d, wrong), eo.records(d), f"{name} ({wrong})")


@pytest.mark.parametrize("wrong", eo.NN_WRONG)
def test_a_wrong_search_fails(wrong):
    name = NN_WRONG_ON[wrong]
    c = eo.NN_CASES[name]
    for f64 in (True, False):
        q, r = eo.nn_build(name, f64)
        d2, idx = eo.nn_search(q, r, c["q_off"], c["r_off"], f64)
        w2, widx = eo.nn_search(q, r, c["q_off"], c["r_off"], f64, wrong)
        with pytest.raises(AssertionError):
            if f64:
                eo.check_nn_f64(w2, widx, d2, idx, name)
            else:
                eo.check_nn_f32(w2.astype(F32), widx, q, r, d2, idx, c["q_off"], c["r_off"], name)
                assert np.array_equal(widx, idx)                                     # (on the lattice the rows are pinned in float32 as well)


# ---- the promises ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eo.CASE_NAMES)
def test_a_case_reaches_what_it_names(name):
    d = eo.build(name)
    assert d.T == sum(d.sizes) and len(d.cat) == d.T
    for what in eo.CASES[name]["promises"]:
        assert eo.promise(d, what), f"{name} does not reach {what}"


@pytest.mark.parametrize("name", eo.NN_CASE_NAMES)
def test_a_search_case_reaches_what_it_names(name):
    for what in eo.NN_CASES[name]["promises"]:
        assert eo.nn_promise(name, what), f"{name} does not reach {what}"


def test_the_matrix_covers_the_launch_shapes_and_the_paths():
    shapes = {eo.nn_launch(c["nq"])[0] for c in eo.NN_CASES.values()}
    assert shapes == set(eo.NN_SHAPES)
    assert [eo.nn_launch(n)[0] for n in (16128, 16129, 65280, 65281, 524032, 524033)] == ["SPLIT16", "SPLIT4", "SPLIT4", "QPT1", "QPT1", "QPT2"]
    named = {p for c in eo.CASES.values() for p in c["promises"]}
    assert {"uniform", "straddling", "lane_in_two_frames", "empty_frames", "frame_scan_carry", "block_scan_carry", "table_path", "allpairs_path",
            "labels:1536", "labels:1537", "chain_wraps", "shared_slot:8", "records:1025", "eval_launch:SPLIT4", "eval_launch:QPT1"} <= named
    assert {c["mode"] for c in eo.CASES.values()} == set(range(5)) and {c["stride"] for c in eo.CASES.values()} == {3, 4, 6}
    # the table's hash: eight ids of frame 0, group 1 whose labels start in the last slot
    ids = eo._slot_ids(0, 1, eo.RANK_SLOTS - 1, 8)
    assert all(((((0 << 34) | (1 << 32) | i) * eo.RANK_MULT) % (1 << 64)) >> 53 == eo.RANK_SLOTS - 1 for i in ids)
    assert co.segment_of([0, 0, 3, 3, 4, 4], 3) == 3 and co.segment_of([0, 0, 3, 3, 4, 4], 0) == 1
