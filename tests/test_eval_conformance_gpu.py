"""Conformance of the instance evaluator (csrc/evalmetrics.hip: himo_eval_instances) and of the exact nearest-neighbour search
(csrc/nn.hip: himo_nn_search, himo_sqrt_inplace) through the C ABI, against oracle/eval_oracle.py: an exact restatement of the written
operation order, so the comparison is of BITS.

For every case of the oracle's matrix himo_eval_instances, given a workspace of exactly himo_eval_workspace_bytes, must leave counts
{selected points, records} and records that -- sorted by (frame, group, instance) -- equal the restatement's: frame, group, instance and
num_pts as integers, vel, dis, mpe and cham bit for bit.  himo_nn_search in float64 returns the restatement's squared distances bit for
bit and the lowest row that attains each; in float32 its value lies within 6 * 2^-24 of the exact minimum (2 * 2^-24 for squaring a
rounded difference, one rounding for the product and for each of the two fused multiply-adds, on a sum of non-negative terms) and the
returned row's exact distance within the same factor of it; on the integer lattice of the tie cases every operation is exact and both
dtypes must return the same bits and the lowest row.  himo_sqrt_inplace equals np.sqrt bit for bit.

Every call: operands, outputs and workspace in guarded buffers (oracle/guarded.py), inputs bit-unchanged, no byte outside an output view
or the workspace written, a second run the same records.  Every refusal returns the status written in the source and writes nothing.

The module summary lists, per family, the number of checks, the kernels met (with the launch shapes of nn_kernel) and the wall time.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import eval_oracle as eo
from guarded import BYTE_FILL, NAN_BITS, Guarded, GuardedBytes

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CHECKS = {}                                                     # family -> [values compared, comparisons]
NN_CALLS = {"nn_kernel_f32": {}, "nn_kernel_f64": {}}           # kernel -> launch shape -> launches this module asked for
REFUSED = []
RAN, NN_RAN = set(), set()
MET = {}
EVAL_KERNELS = ("select_count_kernel", "select_scan_kernel", "select_compact_kernel", "rank_frames_kernel", "payload_kernel", "seg_reduce_kernel")
REC = eo.RECORD_DTYPE.itemsize


def _collect():
    from himo_amd import _lib
    if not MET:
        MET.update(_lib.prof_stop())
    return MET


@pytest.fixture(scope="module", autouse=True)
def _summary(gpu):
    from himo_amd import _lib
    t0 = time.perf_counter()
    _lib.prof_start()
    yield
    met = _collect()
    print("\neval conformance: values compared per family (float64 and integer fields bit for bit; float32 NN within 6 * 2^-24)")
    for k, (n, calls) in sorted(CHECKS.items()):
        print(f"  {k:34s} {n:9d} values in {calls} comparisons")
    print("  kernels met: " + ", ".join(f"{k} x{met[k]['count']}" for k in sorted(met)))
    for k, shapes in sorted(NN_CALLS.items()):
        print(f"  {k} launch shapes asked for: " + ", ".join(f"{s} x{shapes.get(s, 0)}" for s in eo.NN_SHAPES))
    print(f"  refusals reached: {len(REFUSED)}")
    print(f"  module wall time: {time.perf_counter() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """a device error ends the module: nothing more is started on a card that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error ({e}); nothing more is started on it", returncode=3)


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def _count(key, n):
    s = CHECKS.setdefault(key, [0, 0])
    s[0] += int(n)
    s[1] += 1


# ---- guarded operands ------------------------------------------------------------------------------------------------------------
def gfloats(gpu, rows, stride, cols, values=None):
    """[rows, cols] float32 at a row stride of ``stride`` floats inside a NaN-filled buffer"""
    idx = torch.arange(rows, dtype=torch.int64)[:, None] * stride + torch.arange(cols, dtype=torch.int64)[None, :]
    g = Guarded(idx, gpu)
    if values is not None and rows:
        g.put(torch.from_numpy(np.ascontiguousarray(values, F32).reshape(rows, cols)))
    return g


def gbytes(gpu, values=None, nbytes=None):
    if values is not None:
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        g = GuardedBytes(raw.size, gpu)
        if raw.size:
            g.put(torch.from_numpy(raw.copy()))
        return g
    return GuardedBytes(nbytes, gpu)


def ptr(g):
    return None if g is None else g.ptr


class Call:
    """inputs bit-unchanged, nothing outside an output view or the workspace written, after one library call"""

    def __init__(self, inputs, outputs=(), byte_outputs=()):
        self.inputs = [g for g in inputs if g is not None]
        self.outputs = [g for g in outputs if g is not None]
        self.byte_outputs = [g for g in byte_outputs if g is not None]
        self.before = [g.buf.clone() for g in self.inputs]

    def check(self, case):
        torch.cuda.synchronize()
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{case}: an input was written"
        for g in self.outputs + self.byte_outputs:
            assert g.untouched_outside(), f"{case}: a write outside an output view or the workspace"

    def refused(self, fn, case, st, status):
        torch.cuda.synchronize()
        assert st == status, f"{fn} {case}: status {st}, the source returns {status}"
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{fn} {case}: refused but wrote an input"
        for g in self.outputs:
            assert g.untouched(), f"{fn} {case}: refused (status {st}) but wrote an output"
        for g in self.byte_outputs:
            assert bool(torch.all(g.buf == BYTE_FILL)), f"{fn} {case}: refused (status {st}) but wrote counts, records, an output or the workspace"
        REFUSED.append((fn, case, st))


# ---- the evaluator -----------------------------------------------------------------------------------------------------------------
EVAL = ("F", "T", "offs", "p0", "p1", "pc", "stride", "gt", "est", "dt", "cat", "inst", "mask", "lut", "sdt", "mode", "flags", "rec", "max",
        "cnt", "ws", "wsb", "stream")


def _lut(values):
    return (ctypes.c_uint8 * 256)(*[int(v) for v in values])


class Operands:
    """the guarded inputs of a case"""

    def __init__(self, gpu, d):
        c = d.c
        mode = c["mode"]
        self.d = d
        self.OFFS = gbytes(gpu, d.offsets)
        self.PC = gfloats(gpu, d.T, c["stride"], c["stride"], d.pc) if c["has_pc"] else None      # (every column is read: the range is over all of them)
        self.GT = gbytes(gpu, np.asarray(d.gt, F64)) if mode == eo.MODE_DIRECT else gfloats(gpu, d.T, 3, 3, d.gt)
        if mode == eo.MODE_RAW:
            self.EST = None
        elif mode == eo.MODE_DIRECT and not c["est_is_dis"]:
            self.EST = gbytes(gpu, np.asarray(d.est, F64))
        else:
            self.EST = gfloats(gpu, d.T, 3, 3, d.est)
        self.DT = gfloats(gpu, d.T, 1, 1, d.dt) if c["has_dt"] else None
        self.CAT, self.INST, self.MASK = gbytes(gpu, d.cat), gbytes(gpu, d.inst), gbytes(gpu, d.mask)
        uses_pose = mode in (eo.MODE_FLOW, eo.MODE_COMPDIS, eo.MODE_RAW)
        self.P0 = gbytes(gpu, d.given if c["pose_is_ego"] else d.pose0) if uses_pose else None
        self.P1 = gbytes(gpu, d.pose1) if uses_pose and not c["pose_is_ego"] else None
        self.inputs = [self.OFFS, self.PC, self.GT, self.EST, self.DT, self.CAT, self.INST, self.MASK, self.P0, self.P1]
        self.flags = (eo.FLAG_POSE_IS_EGO if c["pose_is_ego"] else 0) | (eo.DIRECT_EST_IS_DIS if c["est_is_dis"] else 0)

    def args(self, lut, rec, max_records, cnt, ws, wsb, sensor_dt=None):
        d, c = self.d, self.d.c
        return dict(F=d.F, T=d.T, offs=self.OFFS.ptr, p0=ptr(self.P0), p1=ptr(self.P1), pc=ptr(self.PC), stride=c["stride"] if self.PC else 0,
                    gt=self.GT.ptr, est=ptr(self.EST), dt=ptr(self.DT), cat=self.CAT.ptr, inst=self.INST.ptr, mask=self.MASK.ptr, lut=lut,
                    sdt=c["sensor_dt"] if sensor_dt is None else sensor_dt, mode=c["mode"], flags=self.flags, rec=rec, max=max_records, cnt=cnt, ws=ws,
                    wsb=wsb, stream=_s())


def run_eval(lib, gpu, ops, max_records, case, sensor_dt=None):
    """one call: (counts [2], the slots written, status)"""
    d = ops.d
    need = int(lib.himo_eval_workspace_bytes(d.F, d.T, max_records))
    RECS, CNT, WS = GuardedBytes(max_records * REC, gpu), GuardedBytes(16, gpu), GuardedBytes(need, gpu)
    call = Call(ops.inputs, [], [RECS, CNT, WS])
    a = ops.args(_lut(d.lut), RECS.ptr, max_records, CNT.ptr, WS.ptr, need, sensor_dt)
    st = lib.himo_eval_instances(*[a[k] for k in EVAL])
    assert st == 0, f"{case}: status {st}"
    call.check(case)
    counts = CNT.bytes().numpy().view(np.int64).copy()
    raw = RECS.bytes().numpy()
    n_written = int(min(max(counts[1], 0), max_records))
    assert bool((raw[n_written * REC:] == BYTE_FILL).all()), f"{case}: a record slot past the {n_written} that were due was written"
    if counts[0] > 0:                                            # the two halves of the Chamfer distance: M float64 queries each (:498-500)
        k, s = NN_CALLS["nn_kernel_f64"], eo.nn_launch(int(counts[0]))[0]
        k[s] = k.get(s, 0) + 2
    return counts, raw[:n_written * REC].view(eo.RECORD_DTYPE).copy()


@pytest.mark.parametrize("name", eo.CASE_NAMES)
def test_eval_case(lib, gpu, name):
    modes = [False, True] if eo.CASES[name]["both_ego_modes"] else [None]
    for ego_mode in modes:
        d = eo.build(name, ego_mode)
        c = d.c
        case = (f"{name}: frames={d.F} rows={d.T} mode={eo.MODE_NAMES[c['mode']]} stride={c['stride']} pose={c['pose']} "
                f"pose_is_ego={c['pose_is_ego']} sensor_dt={c['sensor_dt']:g}")
        want = eo.records(d)
        M, K = len(eo.select(d)[0]), len(want)
        print(f"\n  {case}: {M} selected, {K} records")
        ops = Operands(gpu, d)
        counts, got = run_eval(lib, gpu, ops, K + 2, case)
        assert counts.tolist() == [M, K], f"{case}: counts {counts.tolist()} for {[M, K]}"
        _count("counts", 2)
        n = eo.check_records(got, want, case)
        _count("record integers", 4 * K)
        _count(f"record doubles ({eo.MODE_NAMES[c['mode']]})", n)
        counts2, again = run_eval(lib, gpu, ops, K + 2, case + " again")
        assert counts2.tolist() == counts.tolist() and eo.sort_records(again).tobytes() == eo.sort_records(got).tobytes(), f"{case}: a second run differs"
        _count("second run == first", K)
    RAN.add(name)


@pytest.mark.parametrize("name", ["mode_flow_stride4", "ids_and_groups"])
def test_record_overflow(lib, gpu, name):
    """max_records of 1, K - 1 and K: counts are {M, K} in all three, only the first max_records slots are written, and what is written
    is a duplicate-free subset of the expected records with every field complete"""
    d = eo.build(name)
    want = eo.records(d)
    M, K = len(eo.select(d)[0]), len(want)
    assert K >= 3
    ops = Operands(gpu, d)
    for room in (1, K - 1, K):
        case = f"{name}: max_records={room} of {K}"
        counts, slots = run_eval(lib, gpu, ops, room, case)
        _count("record overflow", eo.check_overflow(slots, counts, want, M, room, case))


def test_degenerate_calls(lib, gpu):
    d = eo.build("mode_flow_stride4")
    ops = Operands(gpu, d)
    lut = _lut(d.lut)
    # total_points == 0: OK, the counts zeroed and nothing else written -- whatever the other pointers are
    need = int(lib.himo_eval_workspace_bytes(d.F, 0, 4))
    RECS, CNT, WS = GuardedBytes(4 * REC, gpu), GuardedBytes(16, gpu), GuardedBytes(need, gpu)
    call = Call(ops.inputs, [], [RECS, CNT, WS])
    a = ops.args(lut, RECS.ptr, 4, CNT.ptr, WS.ptr, need)
    a.update(T=0)
    assert lib.himo_eval_instances(*[a[k] for k in EVAL]) == 0
    call.check("total_points == 0")
    assert CNT.bytes().numpy().view(np.int64).tolist() == [0, 0]
    assert bool(torch.all(RECS.buf == BYTE_FILL)) and bool(torch.all(WS.buf == BYTE_FILL)), "total_points == 0 wrote records or workspace"
    a.update(gt=None, est=None, cat=None, inst=None, mask=None, pc=None, dt=None, p0=None, p1=None)
    assert lib.himo_eval_instances(*[a[k] for k in EVAL]) == 0
    call.check("total_points == 0, operands NULL")
    assert bool(torch.all(RECS.buf == BYTE_FILL)) and bool(torch.all(WS.buf == BYTE_FILL))
    _count("degenerate calls", 2)
    # nothing selected (once by the mask, once by the table): OK, counts {0, 0}, the records untouched
    for what, mask, table in (("mask all zero", np.zeros(d.T, np.uint8), d.lut), ("table all zero", d.mask, np.zeros(256, np.uint8)),
                              ("table of 4s: & 3 leaves nothing", d.mask, np.full(256, 4, np.uint8))):
        need = int(lib.himo_eval_workspace_bytes(d.F, d.T, 4))
        RECS, CNT, WS, MASK = GuardedBytes(4 * REC, gpu), GuardedBytes(16, gpu), GuardedBytes(need, gpu), gbytes(gpu, mask)
        call = Call(ops.inputs + [MASK], [], [RECS, CNT, WS])
        a = ops.args(_lut(table), RECS.ptr, 4, CNT.ptr, WS.ptr, need)
        a.update(mask=MASK.ptr)
        assert lib.himo_eval_instances(*[a[k] for k in EVAL]) == 0, what
        call.check(what)
        assert CNT.bytes().numpy().view(np.int64).tolist() == [0, 0], what
        assert bool(torch.all(RECS.buf == BYTE_FILL)), f"{what}: records written"
        _count("degenerate calls", 2)


def test_nan_sensor_dt_is_not_refused(lib, gpu):
    """``!(sensor_dt != 0.0)`` refuses +0.0 and -0.0 only: a NaN passes, and every number that divides by it is a NaN (the Chamfer
    distance of points that are all NaN is +inf: a NaN candidate never wins the search).  Pinned as the source has it."""
    d = eo.build("mode_flow_stride3")
    nan = eo.make_data(dict(d.c, sensor_dt=float("nan")), d.offsets, d.pc, d.gt, d.est, d.dt, d.cat, d.inst, d.mask, d.lut, d.pose0, d.pose1)
    want = eo.records(nan)
    assert np.isnan(want["vel"]).all() and np.isnan(want["mpe"]).all() and np.isposinf(want["cham"]).all() and np.isfinite(want["dis"]).all()
    counts, got = run_eval(lib, gpu, Operands(gpu, d), len(want), "sensor_dt NaN", sensor_dt=float("nan"))
    _count("record doubles (NaN sensor_dt)", eo.check_records(got, want, "sensor_dt NaN"))


def _mutate(base, change):
    a = dict(base)
    for k, v in change.items():
        a[k] = base[k] + int(v[1:]) if isinstance(v, str) and v[0] == "+" else (base[k] - 1 if v == "-1" else v)
    return a


def test_refusals(lib, gpu):
    """every ``return HIMO_ERR_...`` of himo_eval_instances (evalmetrics.hip:436-450) in source order, those of himo_nn_search
    (nn.hip:198-201) and himo_sqrt_inplace (:185-187): the status written there; counts, records, workspace and outputs unwritten"""
    from himo_amd import _lib
    INVALID, WORKSPACE, UNSUPPORTED = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_WORKSPACE, _lib.ERR_UNSUPPORTED
    assert (INVALID, WORKSPACE, UNSUPPORTED) == (1, 3, 6)
    IS_EGO = eo.FLAG_POSE_IS_EGO
    d = eo.build("mode_flow_stride4")
    ops = Operands(gpu, d)
    ds = eo.build("mode_score_stride4")
    sops = Operands(gpu, ds)
    dd = eo.build("mode_direct_stride4")
    dops = Operands(gpu, dd)
    room = 64
    need = max(int(lib.himo_eval_workspace_bytes(x.F, x.T, room)) for x in (d, ds, dd))
    RECS, CNT, WS = GuardedBytes(room * REC, gpu), GuardedBytes(16, gpu), GuardedBytes(need + 16, gpu)
    lut = _lut(d.lut)
    flow = ops.args(lut, RECS.ptr, room, CNT.ptr, WS.ptr, int(lib.himo_eval_workspace_bytes(d.F, d.T, room)))
    score = sops.args(lut, RECS.ptr, room, CNT.ptr, WS.ptr, int(lib.himo_eval_workspace_bytes(ds.F, ds.T, room)))
    direct = dops.args(lut, RECS.ptr, room, CNT.ptr, WS.ptr, int(lib.himo_eval_workspace_bytes(dd.F, dd.T, room)))
    table = [                                                                       # in the order of the source
        ("n_frames < 1", flow, dict(F=0), INVALID), ("total_points < 0", flow, dict(T=-1), INVALID), ("mode < 0", flow, dict(mode=-1), INVALID),
        ("mode > 4", flow, dict(mode=5), INVALID), ("max_records < 1", flow, dict(max=0), INVALID),
        ("total_points > 2^31 - 1", flow, dict(T=1 << 31), UNSUPPORTED), ("n_frames >= 2^29", flow, dict(F=1 << 29), UNSUPPORTED),
        ("offsets NULL", flow, dict(offs=None), INVALID), ("class_lut NULL", flow, dict(lut=None), INVALID), ("records NULL", flow, dict(rec=None), INVALID),
        ("counts NULL", flow, dict(cnt=None), INVALID), ("workspace NULL", flow, dict(ws=None), INVALID),
        ("sensor_dt 0", flow, dict(sdt=0.0), INVALID), ("sensor_dt -0.0", flow, dict(sdt=-0.0), INVALID),
        ("gt NULL", flow, dict(gt=None), INVALID), ("category NULL", flow, dict(cat=None), INVALID), ("instance NULL", flow, dict(inst=None), INVALID),
        ("eval_mask NULL", flow, dict(mask=None), INVALID),
        ("est NULL (flow)", flow, dict(est=None), INVALID), ("est NULL (compdis)", flow, dict(est=None, mode=eo.MODE_COMPDIS), INVALID),
        ("est NULL (score)", score, dict(est=None), INVALID), ("est NULL (direct)", direct, dict(est=None), INVALID),
        ("pc0 NULL (flow)", flow, dict(pc=None), INVALID), ("lidar_dt NULL (flow)", flow, dict(dt=None), INVALID), ("pc_stride < 3 (flow)", flow, dict(stride=2), INVALID),
        ("pc0 NULL (direct)", direct, dict(pc=None), INVALID), ("lidar_dt NULL (direct)", direct, dict(dt=None), INVALID),
        ("pose0 NULL", flow, dict(p0=None), INVALID), ("pose0 NULL with POSE_IS_EGO", flow, dict(p0=None, flags=IS_EGO), INVALID),
        ("pose1 NULL without POSE_IS_EGO", flow, dict(p1=None), INVALID),
        ("pc_stride < 3 with pc0 (score)", score, dict(stride=2), INVALID),
        ("workspace one byte short", flow, dict(wsb="-1"), WORKSPACE), ("workspace one byte short (score)", score, dict(wsb="-1"), WORKSPACE),
        ("workspace 4 bytes off a 16-byte boundary", flow, dict(ws="+4"), WORKSPACE), ("workspace 8 bytes off", flow, dict(ws="+8"), WORKSPACE),
    ]
    call = Call(ops.inputs + sops.inputs + dops.inputs, [], [RECS, CNT, WS])
    for name, base, change, status in table:
        a = _mutate(base, change)
        call.refused("himo_eval_instances", name, lib.himo_eval_instances(*[a[k] for k in EVAL]), status)
    assert lib.himo_eval_workspace_bytes(0, -5, -1) == lib.himo_eval_workspace_bytes(1, 0, 0)      # the query clamps what the call refuses

    # the search
    nq, nr = 20, 30
    rng = np.random.default_rng(3)
    Q, R = gfloats(gpu, nq, 3, 3, rng.normal(size=(nq, 3))), gfloats(gpu, nr, 3, 3, rng.normal(size=(nr, 3)))
    QO, RO = gbytes(gpu, np.array([0, nq], np.int64)), gbytes(gpu, np.array([0, nr], np.int64))
    D2, IDX = gfloats(gpu, nq, 1, 1), gbytes(gpu, nbytes=4 * nq)
    NN = ("S", "qo", "ro", "nq", "nr", "q", "r", "f64", "d2", "idx", "stream")
    base = dict(S=1, qo=QO.ptr, ro=RO.ptr, nq=nq, nr=nr, q=Q.ptr, r=R.ptr, f64=0, d2=D2.ptr, idx=IDX.ptr, stream=_s())
    call = Call([Q, R, QO, RO], [D2], [IDX])
    for name, change, status in (("n_segments < 1", dict(S=0), INVALID), ("nq < 0", dict(nq=-1), INVALID), ("nr < 0", dict(nr=-1), INVALID),
                                 ("q_offsets NULL", dict(qo=None), INVALID), ("r_offsets NULL", dict(ro=None), INVALID),
                                 ("nr > 2^31 - 1", dict(nr=1 << 31), UNSUPPORTED), ("q NULL", dict(q=None), INVALID), ("dist2 NULL", dict(d2=None), INVALID),
                                 ("r NULL with nr > 0", dict(r=None), INVALID)):
        a = _mutate(base, change)
        call.refused("himo_nn_search", name, lib.himo_nn_search(*[a[k] for k in NN]), status)
    a = _mutate(base, dict(nq=0, q=None, d2=None))                                 # nq == 0 is no refusal: status 0, nothing written
    assert lib.himo_nn_search(*[a[k] for k in NN]) == 0
    call.check("nq == 0")
    assert D2.untouched() and bool(torch.all(IDX.buf == BYTE_FILL))

    # the square root
    V = gfloats(gpu, 8, 1, 1)
    call = Call([], [V])
    call.refused("himo_sqrt_inplace", "n < 0", lib.himo_sqrt_inplace(-1, V.ptr, 0, _s()), INVALID)
    call.refused("himo_sqrt_inplace", "values NULL", lib.himo_sqrt_inplace(8, None, 1, _s()), INVALID)
    assert lib.himo_sqrt_inplace(0, None, 0, _s()) == 0 and lib.himo_sqrt_inplace(0, V.ptr, 1, _s()) == 0
    torch.cuda.synchronize()
    assert V.untouched()
    _count("refusals", len(REFUSED))


# ---- the search --------------------------------------------------------------------------------------------------------------------
def run_nn(lib, gpu, name, f64, with_idx=True):
    c = eo.NN_CASES[name]
    q, r = eo.nn_build(name, f64)
    nq, nr = c["nq"], c["nr"]
    if f64:
        Q, R = gbytes(gpu, q), (gbytes(gpu, r) if nr else None)
        D2 = gbytes(gpu, nbytes=8 * nq)
    else:
        Q, R = gfloats(gpu, nq, 3, 3, q), (gfloats(gpu, nr, 3, 3, r) if nr else None)
        D2 = gfloats(gpu, nq, 1, 1)
    IDX = gbytes(gpu, nbytes=4 * nq)
    QO, RO = gbytes(gpu, c["q_off"]), gbytes(gpu, c["r_off"])
    call = Call([Q, R, QO, RO], [] if f64 else [D2], [IDX] + ([D2] if f64 else []))
    case = f"{name} {'f64' if f64 else 'f32'}" + ("" if with_idx else " idx NULL")
    st = lib.himo_nn_search(len(c["q_off"]) - 1, QO.ptr, RO.ptr, nq, nr, Q.ptr, ptr(R), int(f64), D2.ptr, IDX.ptr if with_idx else None, _s())
    assert st == 0, f"{case}: status {st}"
    call.check(case)
    k = NN_CALLS["nn_kernel_f64" if f64 else "nn_kernel_f32"]
    shape = eo.nn_launch(nq)[0]
    k[shape] = k.get(shape, 0) + 1
    if f64:
        d2 = D2.bytes().numpy().view(F64).copy()
    else:
        words = D2.words().numpy().reshape(-1)
        assert not bool((words.view(np.uint32) == np.uint32(NAN_BITS)).any()), f"{case}: a distance was never written"
        d2 = words.view(F32).copy()
    if not with_idx:
        assert bool(torch.all(IDX.buf == BYTE_FILL)), f"{case}: d_idx NULL but the rows were written somewhere"
        return q, r, d2, None
    return q, r, d2, IDX.bytes().numpy().view(np.int32).copy()


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("name", eo.NN_CASE_NAMES)
def test_nn_case(lib, gpu, name, f64):
    c = eo.NN_CASES[name]
    case = f"{name} {'f64' if f64 else 'f32'} ({eo.nn_launch(c['nq'])[0]})"
    q, r, d2, idx = run_nn(lib, gpu, name, f64)
    want_d, want_i = eo.nn_search(q, r, c["q_off"], c["r_off"], f64)
    if f64:
        _count("nn float64 distances and rows", 2 * eo.check_nn_f64(d2, idx, want_d, want_i, case))
    else:
        _count("nn float32 within 6 * 2^-24", eo.check_nn_f32(d2, idx, q, r, want_d, want_i, c["q_off"], c["r_off"], case))
        if c["kind"] == "ties":                                  # the lattice: every operation exact, so the float32 bits and rows are pinned too
            assert np.array_equal(d2.astype(F64), want_d) and np.array_equal(idx, want_i), f"{case}: the lattice's bits or rows differ"
            _count("nn float32 lattice bits and rows", 2 * len(want_d))
    if c["kind"] == "ties":
        assert set(idx.tolist()) == {rows[0] for rows in eo.TIE_ROWS}, f"{case}: a tie did not go to the lowest row"
    if c["kind"] == "nan":                                       # what the source does: a NaN query matches nothing, a NaN reference is never matched
        assert np.isposinf(d2[eo.NAN_QUERY]) and idx[eo.NAN_QUERY] == -1 and not (idx == eo.NAN_REFERENCE).any()
    if c["nq"] <= 40:                                            # d_idx NULL: the same distances, no row written anywhere
        _, _, d2n, _ = run_nn(lib, gpu, name, f64, with_idx=False)
        assert d2n.tobytes() == d2.tobytes(), f"{case}: the distances differ with d_idx NULL"
        _count("nn idx NULL == with idx", len(d2))
    NN_RAN.add((name, f64))


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_sqrt_inplace(lib, gpu, n, f64):
    rng = np.random.default_rng(90 + n)
    T = F64 if f64 else F32
    v = (rng.uniform(0, 1, n) * 10.0 ** rng.integers(-30, 30, n)).astype(T)
    edge = np.array([0.0, np.inf, 2.0, 0.25, np.finfo(T).tiny / 8, np.finfo(T).max, 1.0 + np.finfo(T).eps], T)
    v[:min(n, len(edge))] = edge[:n]
    V = gbytes(gpu, v) if f64 else gfloats(gpu, n, 1, 1, v)
    call = Call([], [] if f64 else [V], [V] if f64 else [])
    case = f"sqrt n={n} {'f64' if f64 else 'f32'}"
    assert lib.himo_sqrt_inplace(n, V.ptr, int(f64), _s()) == 0, case
    call.check(case)
    got = V.bytes().numpy().view(F64) if f64 else V.words().numpy().reshape(-1).view(F32)
    with np.errstate(all="ignore"):
        want = np.sqrt(v)
    assert got.tobytes() == want.tobytes(), f"{case}: {int((got != want).sum())} of {n} differ from np.sqrt"
    _count("sqrt_inplace bits", n)


def test_every_kernel_and_launch_shape_was_met(gpu):
    """after the whole module: the six kernels of the evaluator, both searches with as many launches as the cases asked for, over all
    four launch shapes in both dtypes, and the square root"""
    if RAN != set(eo.CASE_NAMES) or NN_RAN != {(n, f) for n in eo.NN_CASE_NAMES for f in (True, False)}:
        print("\n  only a part of the matrix ran in this session: nothing to conclude")
        return
    met = _collect()
    for k in EVAL_KERNELS + ("nn_kernel_f32", "nn_kernel_f64", "sqrt_kernel"):
        assert k in met and met[k]["count"] > 0, f"{k} was never launched: {sorted(met)}"
    for k, shapes in NN_CALLS.items():
        assert set(shapes) == set(eo.NN_SHAPES), f"{k}: launch shapes {sorted(shapes)}"
        assert met[k]["count"] == sum(shapes.values()), f"{k}: {met[k]['count']} launches, the cases asked for {sum(shapes.values())}"
