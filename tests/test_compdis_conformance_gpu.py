"""Conformance of the motion-compensation kernels (csrc/compdis.hip, csrc/compdis_gt.hip, csrc/compdis_math.h) through the C ABI,
against oracle/compdis_oracle.py: an exact restatement of the documented operation order, so the comparison is of BITS.

For every case of the oracle's matrix himo_compdis_batch must leave, in a workspace of exactly himo_compdis_workspace_bytes,
  * per-frame maxima whose decoded keys equal frame_max bit for bit (NaN elements dropped, NaN where nothing is above -inf),
  * per-frame transforms equal to the given rows bit for bit under HIMO_FLAG_POSE_IS_EGO and otherwise within ego_bound -- the one
    derived bound of the suite -- of the exact rational inv(pose1) @ pose0 and equal in bits to lu_ego, compute_ego's order restated (all NaN for a singular pose1, the neighbours untouched),
and comp_dis, refined and the evaluation mask equal to ``chain`` / ``mask`` run on THOSE transforms and maxima, bit for bit, NaN
positions included: no exact-fraction allowance and no absolute tolerance.  himo_compdis_frame gives the bits of the batch of one;
himo_compdis_gt_batch writes bodies equal to ``gt_body`` byte for byte, pad bytes included, and nothing between or after them; one-row
sweeps follow the single_row order there.  Every call: inputs bit-unchanged, no byte outside an output view or the workspace
written, a second run the same bits, every output element written.  Every refusal of the entry points of both files returns the
status written in the source and writes nothing.  All operands live in guarded buffers (oracle/guarded.py).

The module summary lists the bit-exact checks per output, the worst transform error over its bound per pose, the template
instances and block paths met (mirrored from compdis.hip:373-387 and compdis_gt.hip:281-288) and the refusals reached.
"""
import ctypes

import numpy as np
import pytest
import torch

import compdis_oracle as co
import himo_oracle as ho
from guarded import BYTE_FILL, NAN_BITS, Guarded, GuardedBytes

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CHECKS = {}       # output -> [elements compared bit for bit, calls]
EGO = {}          # pose kind -> [worst err / bound, frames, case of the worst]
INSTANCES = {}    # template instance -> cases that launched it
PATHS = {}        # uniform / straddling / tail -> cases
REFUSED = []      # (entry point, case, status)
RAN = set()

ALL_INSTANCES = {f"compdis_kernel<{s}, {t}>" for s in (4, 3, 0) for t in ("f32", "f64")} | \
                {f"compdis_gt_kernel<{s}, {t}>" for s in (4, 0) for t in ("f32", "f64")}
ALL_PATHS = {"uniform", "straddling", "tail"}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\ncompdis conformance: elements compared bit for bit, per output")
    for k, (n, calls) in sorted(CHECKS.items()):
        print(f"  {k:28s} {n:9d} elements in {calls} comparisons")
    print("  transform |error| / ego_bound, worst element per pose (float64 LU on the device against the exact rational inverse):")
    for k, (w, n, case) in sorted(EGO.items()):
        print(f"    {k:22s} {w:.3g}  ({n} frames; worst in {case})")
    print("  template instances met: " + ", ".join(f"{k} x{v}" for k, v in sorted(INSTANCES.items())))
    print("  block paths met: " + ", ".join(f"{k} x{v}" for k, v in sorted(PATHS.items())))
    print(f"  refusals reached: {len(REFUSED)}")
    for fn, case, st in REFUSED:
        print(f"    {fn}: {case}: status {st}")


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


# ---- guarded operands ------------------------------------------------------------------------------------------------------------
def gfloats(gpu, rows, stride, cols, off_bytes=0, values=None):
    """[rows, cols] float32 at a row stride of ``stride`` floats, ``off_bytes`` past a 16-byte boundary; the rest of each row is fill"""
    assert off_bytes % 4 == 0
    idx = torch.arange(rows, dtype=torch.int64)[:, None] * stride + torch.arange(cols, dtype=torch.int64)[None, :]
    g = Guarded(idx, gpu, off_bytes // 4)
    if values is not None:
        g.put(torch.from_numpy(np.ascontiguousarray(values, F32).reshape(rows, cols)))
    return g


def gbytes(gpu, values=None, nbytes=None, off=0):
    """the bytes of ``values`` (any dtype), or ``nbytes`` of fill"""
    if values is not None:
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        g = GuardedBytes(raw.size, gpu, off)
        g.put(torch.from_numpy(raw.copy()))
        return g
    return GuardedBytes(nbytes, gpu, off)


def bits(g):
    return g.words().numpy().view(np.uint32).reshape(-1)


def _count(key, n):
    s = CHECKS.setdefault(key, [0, 0])
    s[0] += int(n)
    s[1] += 1


def same_bits(key, got_u32, want_f32, case):
    """equal bits; where the oracle itself says NaN any NaN but the buffers' fill pattern will do"""
    want = np.ascontiguousarray(want_f32, F32).reshape(-1)
    got = got_u32.view(F32)
    assert got.shape == want.shape, f"{case} {key}: shape"
    assert not bool((got_u32 == np.uint32(NAN_BITS)).any()), \
        f"{case} {key}: {int((got_u32 == np.uint32(NAN_BITS)).sum())} elements still hold the fill (never written, or computed from a read outside a view)"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{case} {key}: NaN at {int((np.isnan(got) != nan).sum())} other positions than the oracle"
    bad = np.nonzero(got_u32[~nan] != want.view(np.uint32)[~nan])[0]
    if bad.size:
        i = int(np.nonzero(~nan)[0][bad[0]])
        raise AssertionError(f"{case} {key}: {bad.size} of {want.size} elements differ in bits; first at {i}: {got[i]!r} "
                             f"({int(got_u32[i]):#010x}), the oracle {want[i]!r} ({int(want.view(np.uint32)[i]):#010x})")
    _count(key, want.size)


class Call:
    """inputs bit-unchanged, nothing outside an output view or the workspace written, after one library call"""

    def __init__(self, inputs, outputs, ws=None, byte_outputs=()):
        self.inputs = [g for g in inputs if g is not None]
        self.outputs = [g for g in outputs if g is not None]
        self.byte_outputs = [g for g in byte_outputs if g is not None]
        self.ws = ws
        self.before = [g.buf.clone() for g in self.inputs]

    def check(self, case):
        torch.cuda.synchronize()
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{case}: an input was written"
        for g in self.outputs + self.byte_outputs:
            assert g.untouched_outside(), f"{case}: a write outside an output view"
        if self.ws is not None:
            assert self.ws.untouched_outside(), f"{case}: a write outside the workspace size the query returned"

    def refused(self, fn, case, st, status):
        torch.cuda.synchronize()
        assert st == status, f"{fn} {case}: status {st}, the source returns {status}"
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{fn} {case}: refused but wrote an input"
        for g in self.outputs:
            assert g.untouched(), f"{fn} {case}: refused (status {st}) but wrote an output"
        for g in self.byte_outputs + ([self.ws] if self.ws is not None else []):
            assert bool(torch.all(g.buf == BYTE_FILL)), f"{fn} {case}: refused (status {st}) but wrote an output or the workspace"
        REFUSED.append((fn, case, st))


def _bounds(box):
    lo, hi = co.BOX[box]
    return (ctypes.c_float * 6)(*[float(v) for v in list(lo) + list(hi)])


def _flags(c, pose_is_ego):
    from himo_amd import _lib
    return ((_lib.FLAG_F32_CHAIN if c["f32"] else 0) | (_lib.FLAG_RAW if c["raw"] else 0) | (_lib.FLAG_SCANIA if c["scania"] else 0) |
            (_lib.FLAG_POSE_IS_EGO if pose_is_ego else 0))


def keys_bytes(n_frames):
    return (n_frames * 4 + 15) // 16 * 16                       # compdis_math.h:27-29


def read_workspace(ws_bytes, n_frames):
    """compdis_math.h:116-121: keys_bytes(n) bytes of keys, then n x 12 doubles (R[9], t[3]) -> maxima [n] float32, transforms [n, 3, 4]"""
    raw = ws_bytes.numpy()
    keys = raw[:4 * n_frames].view(np.uint32)
    xf = raw[keys_bytes(n_frames):keys_bytes(n_frames) + 96 * n_frames].view(F64).reshape(n_frames, 12)
    ego = np.concatenate([xf[:, :9].reshape(n_frames, 3, 3), xf[:, 9:, None]], axis=2)
    return co.key_to_float(keys), ego


class Operands:
    """the guarded inputs of a case, shared by the batch, frame and ground-truth calls"""

    def __init__(self, gpu, d, pose_is_ego):
        c, off = d.c, d.c["off"]
        self.d, self.pose_is_ego = d, pose_is_ego
        self.PC = gfloats(gpu, d.T, c["stride"], 3, off.get("pc", 0), d.pc[:, :3])
        self.FL = gfloats(gpu, d.T, 3, 3, off.get("flow", 0), d.flow)
        self.DT = gfloats(gpu, d.T, 1, 1, off.get("dt", 0), d.dt)
        self.GM = gbytes(gpu, d.gm, off=off.get("gm", 0))
        self.VALID = gbytes(gpu, d.valid, off=off.get("valid", 0)) if d.valid is not None else None
        self.OFFS = gbytes(gpu, d.offsets)
        self.given = co.numpy_egos(d) if pose_is_ego else None
        self.P0 = gbytes(gpu, self.given if pose_is_ego else d.pose0)
        self.P1 = None if pose_is_ego else gbytes(gpu, d.pose1)
        self.inputs = [self.PC, self.FL, self.DT, self.GM, self.VALID, self.OFFS, self.P0, self.P1]


def run_batch(lib, gpu, ops, case):
    d, c = ops.d, ops.d.c
    off = c["off"]
    need = int(lib.himo_compdis_workspace_bytes(d.F))
    assert need == keys_bytes(d.F) + 96 * d.F + 16 + 256
    CD = gfloats(gpu, d.T, 3, 3, off.get("cd", 0))
    RF = gfloats(gpu, d.T, 3, 3, off.get("rf", 0)) if c["refined"] else None
    MASK = gbytes(gpu, nbytes=d.T, off=off.get("mask", 0)) if c["mask"] else None
    WS = GuardedBytes(need, gpu)
    call = Call(ops.inputs, [CD, RF], WS, [MASK])
    st = lib.himo_compdis_batch(d.F, d.T, ops.OFFS.ptr, ops.P0.ptr, ops.P1.ptr if ops.P1 else None, ops.PC.ptr, c["stride"], ops.FL.ptr,
                                ops.DT.ptr, c["sensor_dt"], _flags(c, ops.pose_is_ego), CD.ptr, RF.ptr if RF else None,
                                MASK.ptr if MASK else None, ops.GM.ptr, ops.VALID.ptr if ops.VALID else None, _bounds(c["box"]),
                                co.CLOSE, WS.ptr, need, _s())
    assert st == 0, f"{case}: status {st}"
    call.check(case)
    if d.T:                                                     # the launch conditions of compdis.hip:373-387, from the pointers themselves
        looked = [ops.PC.ptr, ops.DT.ptr, CD.ptr] + ([] if c["raw"] else [ops.FL.ptr]) + ([RF.ptr] if RF else [])
        al4 = [MASK.ptr, ops.GM.ptr] + ([ops.VALID.ptr] if c["scania"] else []) if MASK else []
        inst, vec = co.compdis_instance(c["stride"], c["f32"], all(p % 16 == 0 for p in looked), all(p % 4 == 0 for p in al4))
        assert vec == co.is_vec(c), f"{case}: the case's layout does not select what it says"
        INSTANCES[inst] = INSTANCES.get(inst, 0) + 1
        for p in co.block_paths(d.offsets, vec):
            PATHS[p] = PATHS.get(p, 0) + 1
    return dict(cd=bits(CD), rf=bits(RF) if RF else None, mask=MASK.bytes().numpy() if MASK else None, ws=WS.bytes())


def check_batch(out, ops, case):
    """keys, transforms, then the points from the device's own transforms and maxima"""
    d, c = ops.d, ops.d.c
    fmax, ego = read_workspace(out["ws"], d.F)
    want_max = co.maxima(d)
    assert np.array_equal(fmax.view(np.uint32), want_max.view(np.uint32)), \
        f"{case}: per-frame maxima differ from frame_max in frames {np.nonzero(fmax.view(np.uint32) != want_max.view(np.uint32))[0][:8]}"
    _count("max(lidar_dt) keys", d.F)
    if ops.pose_is_ego:
        assert np.array_equal(ego.view(np.uint64), np.ascontiguousarray(ops.given[:, :3, :]).view(np.uint64)), f"{case}: POSE_IS_EGO transforms are not the given rows"
        _count("transforms (POSE_IS_EGO)", ego.size)
    else:
        first = {}
        for f in range(d.F):
            k = d.pose_kinds[f]
            if k in first:                                      # the same pose pair again: the same bits, whichever thread and block made them
                assert np.array_equal(ego[f].view(np.uint64), ego[first[k]].view(np.uint64)), f"{case}: frame {f} ({k}) differs from frame {first[k]}"
                continue
            first[k] = f
            if k == "singular":
                assert np.isnan(ego[f]).all(), f"{case}: a singular pose1 must give an all-NaN transform, got {ego[f]}"
                continue
            r = co.ego_ratio(ego[f], d.pose0[f], d.pose1[f])
            label = f"{k} {'f32' if c['f32'] else 'f64'} poses"
            s = EGO.setdefault(label, [0.0, 0, case.split(":")[0]])
            if r >= s[0]:
                s[0], s[2] = r, case.split(":")[0]
            assert r <= 1.0, f"{case}: frame {f} ({k}): transform error {r:g} of ego_bound"
            lu = co.lu_ego(d.pose0[f], d.pose1[f])                # compute_ego's own order, restated: first maximal pivot, swaps, k-ordered product
            assert np.array_equal(ego[f].view(np.uint64), lu.view(np.uint64)), \
                f"{case}: frame {f} ({k}): {int((ego[f].view(np.uint64) != lu.view(np.uint64)).sum())} of 12 elements differ in bits from the restated LU"
            _count("transforms (== lu_ego)", 12)
        for k in first:
            if k != "singular":
                EGO[f"{k} {'f32' if c['f32'] else 'f64'} poses"][1] += sum(1 for x in d.pose_kinds if x == k)
        _count("transforms (within ego_bound)", 12 * d.F)
    cd, rf, nrm, m = co.points(d, ego, fmax)
    same_bits("comp_dis", out["cd"], cd, case)
    if out["rf"] is not None:
        same_bits("refined", out["rf"], rf, case)
    if out["mask"] is not None:
        assert np.array_equal(out["mask"], m), f"{case}: eval_mask differs at rows {np.nonzero(out['mask'] != m)[0][:8]}"
        _count("eval_mask", m.size)
    return fmax, ego


def same_run(a, b, case):
    for k in ("cd", "rf", "mask"):
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), f"{case}: {k} of a second run differs"
    assert torch.equal(a["ws"], b["ws"]), f"{case}: the workspace of a second run differs"


def run_frame(lib, gpu, ops, batch_out, case):
    """himo_compdis_frame: host poses, the single-frame wrapper's own offsets and poses in the workspace tail"""
    d, c = ops.d, ops.d.c
    need = int(lib.himo_compdis_workspace_bytes(1))
    CD = gfloats(gpu, d.T, 3, 3, c["off"].get("cd", 0))
    RF = gfloats(gpu, d.T, 3, 3, c["off"].get("rf", 0)) if c["refined"] else None
    WS = GuardedBytes(need, gpu)
    dbl = ctypes.c_double * 16
    h0 = dbl(*(ops.given[0] if ops.pose_is_ego else d.pose0[0]).reshape(-1).tolist())
    h1 = None if ops.pose_is_ego else dbl(*d.pose1[0].reshape(-1).tolist())
    call = Call([ops.PC, ops.FL, ops.DT], [CD, RF], WS)
    from himo_amd import _lib
    flags = _flags(c, ops.pose_is_ego) & ~_lib.FLAG_SCANIA
    st = lib.himo_compdis_frame(d.T, h0, h1, ops.PC.ptr, c["stride"], ops.FL.ptr, ops.DT.ptr, c["sensor_dt"], flags, CD.ptr,
                                RF.ptr if RF else None, WS.ptr, need, _s())
    assert st == 0, f"{case}: himo_compdis_frame status {st}"
    call.check(case + " (frame)")
    assert np.array_equal(bits(CD), batch_out["cd"]), f"{case}: himo_compdis_frame's comp_dis differs from the batch of one"
    _count("comp_dis (frame == batch)", 3 * d.T)
    if RF is not None:
        assert np.array_equal(bits(RF), batch_out["rf"]), f"{case}: himo_compdis_frame's refined differs from the batch of one"
        _count("refined (frame == batch)", 3 * d.T)


def run_gt(lib, gpu, ops, fmax, ego, batch_out, case):
    """himo_compdis_gt_batch on the same operands: bodies 16 bytes apart in a buffer of fill"""
    from himo_amd import _lib
    d, c = ops.d, ops.d.c
    columns = c["columns"]
    starts, sizes = [], []
    for n in d.sizes:
        h = (ctypes.c_int64 * _lib.GT_MAX_COLUMNS)()
        nb = int(lib.himo_gt_column_starts(n, columns, h))
        assert nb == int(lib.himo_gt_body_bytes(n, columns)) and nb % 8 == 0
        starts.append(list(h))
        sizes.append(nb)
    gap = 16
    body_off = np.concatenate([[0], np.cumsum([s + gap for s in sizes])]).astype(np.int64)
    total = int(body_off[-1])
    BODY = GuardedBytes(total, gpu)
    BO = gbytes(gpu, body_off)
    CAT = gbytes(gpu, d.cat) if columns & 1 else None
    INST = gbytes(gpu, d.inst) if columns & 2 else None
    need = int(lib.himo_compdis_workspace_bytes(d.F))
    WS = GuardedBytes(need, gpu)
    call = Call(ops.inputs + [BO, CAT, INST], [], WS, [BODY])
    flags = _flags(c, ops.pose_is_ego)
    st = lib.himo_compdis_gt_batch(d.F, d.T, ops.OFFS.ptr, ops.P0.ptr, ops.P1.ptr if ops.P1 else None, ops.PC.ptr, c["stride"], ops.FL.ptr,
                                   ops.DT.ptr, c["sensor_dt"], flags, ops.GM.ptr, ops.VALID.ptr if ops.VALID else None,
                                   CAT.ptr if CAT else None, INST.ptr if INST else None, columns, _bounds(c["box"]), co.CLOSE,
                                   BO.ptr, BODY.ptr, WS.ptr, need, _s())
    assert st == 0, f"{case}: himo_compdis_gt_batch status {st}"
    call.check(case + " (gt)")
    used = keys_bytes(d.F) + 96 * d.F
    assert torch.equal(WS.bytes()[:used], batch_out["ws"][:used]), f"{case}: the ground-truth writer's keys or transforms differ from the batch's"
    if d.T:
        inst = co.gt_instance(c["stride"], c["f32"], ops.PC.ptr % 16 == 0)
        INSTANCES[inst] = INSTANCES.get(inst, 0) + 1
    cd, _, nrm, m = co.points(d, ego, fmax, gt=True)
    want = np.full(total, BYTE_FILL, np.uint8)
    o = d.offsets
    for f, n in enumerate(d.sizes):
        r = slice(int(o[f]), int(o[f + 1]))
        want[body_off[f]:body_off[f] + sizes[f]] = co.gt_body(starts[f], sizes[f], cd[r], m[r], d.cat[r], d.inst[r], nrm[r], d.pc[r, :3]) if n else 0
    got = BODY.bytes().numpy().copy()
    for f, n in enumerate(d.sizes):                             # where the oracle itself says NaN, any NaN will do (the bytes of a NaN are not pinned)
        for k in (co.GT_CD, co.GT_CD + 1, co.GT_CD + 2, co.GT_NORM):
            a = int(body_off[f]) + starts[f][k]
            g, w = got[a:a + 4 * n].view(F32), want[a:a + 4 * n].view(F32)
            both = np.isnan(g) & np.isnan(w) & (g.view(np.uint32) != np.uint32(NAN_BITS))
            g.view(np.uint32)[both] = w.view(np.uint32)[both]
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        f = int(np.searchsorted(body_off, i, side="right") - 1)
        col = max((k for k in range(10) if 0 <= starts[f][k] <= i - body_off[f]), default=-1) if i - body_off[f] < sizes[f] else "the gap after it"
        raise AssertionError(f"{case}: {int((got != want).sum())} body bytes differ; first at byte {i}: sweep {f} ({d.sizes[f]} rows), "
                             f"column {col}, byte {i - body_off[f]} of the body: {got[i]} for {want[i]}")
    _count("gt body bytes", total)
    # the comp_dis columns against himo_compdis_batch's own bits, sweep by sweep (one-row float64 sweeps follow the single_row order)
    bcd = batch_out["cd"].reshape(-1, 3)
    n_cmp = 0
    for f, n in enumerate(d.sizes):
        if n >= 2 or (n == 1 and c["f32"]):
            for k in range(3):
                a = int(body_off[f]) + starts[f][co.GT_CD + k]
                g, b = got[a:a + 4 * n].view(F32), bcd[int(o[f]):int(o[f + 1]), k].view(F32)
                assert np.array_equal(np.isnan(g), np.isnan(b)) and np.array_equal(g.view(np.uint32)[~np.isnan(g)], b.view(np.uint32)[~np.isnan(b)]), f"{case}: sweep {f} comp_dis column {k} differs from the batch's"
            n_cmp += 3 * n
    _count("gt comp_dis == batch", n_cmp)


# ---- the matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", co.CASE_NAMES)
def test_compdis_case(lib, gpu, name):
    d = co.build(name)
    c = d.c
    case = (f"{name}: frames={d.F} rows={d.T} stride={c['stride']} off={c['off']} pose={c['pose']} {'f32' if c['f32'] else 'f64'} chain "
            f"raw={c['raw']} box={c['box']} refined={c['refined']} mask={c['mask']} dt={c['dt']} sensor_dt={c['sensor_dt']:g}")
    print(f"\n  {case}")
    modes = [bool(c.get("pose_is_ego", False))] + ([True] if c.get("both_ego_modes") else [])
    for i, ego_mode in enumerate(modes):
        label = case + (" POSE_IS_EGO" if ego_mode else "")
        ops = Operands(gpu, d, ego_mode)
        out = run_batch(lib, gpu, ops, label)
        fmax, ego = check_batch(out, ops, label)
        same_run(out, run_batch(lib, gpu, ops, label + " again"), label)
        if d.F == 1 and d.T > 0:
            run_frame(lib, gpu, ops, out, label)
        if i == 0 and not c["raw"]:
            run_gt(lib, gpu, ops, fmax, ego, out, label)
    RAN.add(name)


def test_every_instance_and_path_was_met(gpu):
    """after the whole matrix: every template instance of both kernels and every block path appeared at least once"""
    if RAN != set(co.CASE_NAMES):
        print(f"\n  only {len(RAN)} of {len(co.CASE_NAMES)} cases ran in this session: nothing to conclude")
        return
    assert set(INSTANCES) == ALL_INSTANCES, sorted(ALL_INSTANCES - set(INSTANCES))
    assert set(PATHS) == ALL_PATHS, sorted(ALL_PATHS - set(PATHS))
    assert {f"{k} {t} poses" for k in co.POSE_KINDS for t in ("f32", "f64")} <= set(EGO), sorted(EGO)


# ---- the element-wise utilities ---------------------------------------------------------------------------------------------------
def _f64(g, shape):
    return g.bytes().numpy().view(F64).reshape(shape)


@pytest.mark.parametrize("n", [1, 85, 86, 256, 257])
def test_flow2compdis(lib, gpu, n):
    """3 n = 255, 258, 768, 771 around the 256-element blocks; float32 x float32, float64 x float32, float64 x float64; divide THEN multiply"""
    rng = np.random.default_rng(50 + n)
    flow = rng.uniform(-200, 200, (n, 3))
    dt0 = rng.uniform(0, 0.1, n).astype(F32)
    dt0[::7] = 0
    for flags, tf, td, sdt in ((0, F32, F32, 0.1), (1, F64, F32, 0.1), (3, F64, F64, 10.0), (0, F32, F32, 10.0)):
        fl, d0 = flow.astype(tf), (dt0.astype(F64) * (1 + 2.0 ** -40)).astype(td) if td is F64 else dt0
        A = gfloats(gpu, n, 3, 3, 0, fl) if tf is F32 else gbytes(gpu, fl)
        B = gfloats(gpu, n, 1, 1, 0, d0) if td is F32 else gbytes(gpu, d0)
        O = gfloats(gpu, n, 3, 3) if tf is F32 else gbytes(gpu, nbytes=24 * n)
        call = Call([A, B], [O] if tf is F32 else [], None, [] if tf is F32 else [O])
        case = f"flow2compdis n={n} dtype_flags={flags} sensor_dt={sdt:g}"
        assert lib.himo_flow2compdis(n, A.ptr, B.ptr, sdt, flags, O.ptr, _s()) == 0, case
        call.check(case)
        want = ho.flow2compDis(fl, d0, sensor_dt=sdt)
        assert want.dtype == tf
        if tf is F32:
            same_bits("flow2compdis f32", bits(O), want, case)
        else:
            assert np.array_equal(_f64(O, (n, 3)).view(np.uint64), want.view(np.uint64)), case
            _count("flow2compdis f64", want.size)


@pytest.mark.parametrize("stride", [3, 4, 7])
@pytest.mark.parametrize("n", [85, 86, 257])
def test_refine_pts(lib, gpu, n, stride):
    rng = np.random.default_rng(60 + n + stride)
    pc = rng.uniform(-200, 200, (n, 3)).astype(F32)
    ds = rng.uniform(-3, 3, (n, 3))
    PC = gfloats(gpu, n, stride, 3, 0, pc)
    for is64, t in ((0, F32), (1, F64)):
        DS = gfloats(gpu, n, 3, 3, 0, ds.astype(t)) if t is F32 else gbytes(gpu, ds)
        O = gfloats(gpu, n, 3, 3) if t is F32 else gbytes(gpu, nbytes=24 * n)
        call = Call([PC, DS], [O] if t is F32 else [], None, [] if t is F32 else [O])
        case = f"refine_pts n={n} stride={stride} f64={is64}"
        assert lib.himo_refine_pts(n, PC.ptr, stride, DS.ptr, is64, O.ptr, _s()) == 0, case
        call.check(case)
        want = ho.refine_pts(pc, ds.astype(t))
        assert want.dtype == t
        if t is F32:
            same_bits("refine_pts f32", bits(O), want, case)
        else:
            assert np.array_equal(_f64(O, (n, 3)).view(np.uint64), want.view(np.uint64)), case
            _count("refine_pts f64", want.size)


@pytest.mark.parametrize("stride", [3, 4, 7])
@pytest.mark.parametrize("box", ["av2", "scania"])
def test_ego_pts_mask_on_its_faces(lib, gpu, box, stride):
    """on every face, one float32 step inside and outside it (strict compares: a point ON a face is outside the box), and 300 more
    rows so that a second block runs"""
    pts, what = co.threshold_points(box)
    rng = np.random.default_rng(70 + stride)
    pts = np.concatenate([pts, rng.uniform(-10, 10, (300, 3)).astype(F32)])
    n = len(pts)
    P = gfloats(gpu, n, stride, 3, 0, pts)
    O = gbytes(gpu, nbytes=n)
    call = Call([P], [], None, [O])
    case = f"ego_pts_mask {box} stride={stride}"
    assert lib.himo_ego_pts_mask(n, P.ptr, stride, _bounds(box), O.ptr, _s()) == 0, case
    call.check(case)
    lo, hi = np.asarray(co.BOX[box][0], F32), np.asarray(co.BOX[box][1], F32)
    want = ho.ego_pts_mask(pts, lo, hi)
    got = O.bytes().numpy()
    assert np.array_equal(got, want.astype(np.uint8)), f"{case}: rows {np.nonzero(got != want)[0][:8]}"
    for i, w in enumerate(what[3:], 3):
        assert got[i] == (0 if w.startswith("inside") else 1), (case, w)
    _count("ego_pts_mask", n)


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_dt0(lib, gpu, n, off):
    """max(lidar_dt) - lidar_dt in float32 around the 4096-element chunk of the max pre-pass, the input 16-byte aligned (vector loads)
    and 4 bytes past that (scalar loads)"""
    rng = np.random.default_rng(80 + n)
    dt = rng.uniform(0, 0.1, n).astype(F32)
    dt[n - 1] = F32(0.2)                                          # the maximum in the last element: the second chunk's only one for n = 4097
    D = gfloats(gpu, n, 1, 1, off, dt)
    O = gfloats(gpu, n, 1, 1)
    WS = GuardedBytes(int(lib.himo_compdis_workspace_bytes(1)), gpu)
    call = Call([D], [O], WS)
    case = f"dt0 n={n} off={off}"
    assert lib.himo_dt0(n, D.ptr, O.ptr, WS.ptr, _s()) == 0, case
    call.check(case)
    same_bits("dt0", bits(O), dt.max() - dt, case)
    assert np.array_equal(dt.max() - dt, ho.dt0_from_lidar_dt(dt))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
BATCH = ("F", "T", "offs", "p0", "p1", "pc", "stride", "flow", "dt", "sdt", "flags", "cd", "rf", "mask", "gm", "valid", "bounds", "close", "ws",
         "wsb", "stream")
GT = ("F", "T", "offs", "p0", "p1", "pc", "stride", "flow", "dt", "sdt", "flags", "gm", "valid", "cat", "inst", "columns", "bounds", "close",
      "bo", "body", "ws", "wsb", "stream")
FRAME = ("T", "h0", "h1", "pc", "stride", "flow", "dt", "sdt", "flags", "cd", "rf", "ws", "wsb", "stream")


def _mutate(base, change):
    a = dict(base)
    for k, v in change.items():
        a[k] = base[k] + int(v[1:]) if isinstance(v, str) and v[0] == "+" else (base[k] - 1 if v == "-1" else v)
    return a


def test_refusals(lib, gpu):
    """every ``return HIMO_ERR_...`` of the entry points of compdis.hip (:400-408, :419-436, :453-456, :473-475, :489-491, :499-501)
    and compdis_gt.hip (:248-261): the status written there, and not a byte written -- outputs and workspace alike"""
    from himo_amd import _lib
    INVALID, EMPTY, WORKSPACE, SINGULAR = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_EMPTY_FRAME, _lib.ERR_WORKSPACE, _lib.ERR_SINGULAR_POSE
    assert (INVALID, EMPTY, WORKSPACE, SINGULAR) == (1, 2, 3, 4)
    RAW, SCANIA, IS_EGO = _lib.FLAG_RAW, _lib.FLAG_SCANIA, _lib.FLAG_POSE_IS_EGO
    d = co.build("n4")
    ops = Operands(gpu, d, False)
    valid = gbytes(gpu, np.ones(d.T, np.uint8))
    need = int(lib.himo_compdis_workspace_bytes(d.F))
    CD, RF, MASK = gfloats(gpu, d.T, 3, 3), gfloats(gpu, d.T, 3, 3), gbytes(gpu, nbytes=d.T)
    WS = GuardedBytes(need + 16, gpu)                           # room for the misaligned pointer; the size passed stays ``need``
    bounds = _bounds("av2")
    base = dict(F=d.F, T=d.T, offs=ops.OFFS.ptr, p0=ops.P0.ptr, p1=ops.P1.ptr, pc=ops.PC.ptr, stride=4, flow=ops.FL.ptr, dt=ops.DT.ptr, sdt=0.1,
                flags=0, cd=CD.ptr, rf=RF.ptr, mask=MASK.ptr, gm=ops.GM.ptr, valid=valid.ptr, bounds=bounds, close=co.CLOSE, ws=WS.ptr,
                wsb=need, stream=_s())
    common = {
        "n_frames < 1": (dict(F=0), INVALID), "total_points < 0": (dict(T=-1), INVALID), "pc_stride < 3": (dict(stride=2), INVALID),
        "offsets NULL": (dict(offs=None), INVALID), "pose0 NULL": (dict(p0=None), INVALID), "workspace NULL": (dict(ws=None), INVALID),
        "pose1 NULL without POSE_IS_EGO": (dict(p1=None), INVALID),
        "pc0 NULL": (dict(pc=None), INVALID), "lidar_dt NULL": (dict(dt=None), INVALID),
        "flow NULL": (dict(flow=None), INVALID),
        "SCANIA without flow_is_valid": (dict(flags=SCANIA, valid=None), INVALID),
        "sensor_dt 0": (dict(sdt=0.0), INVALID), "sensor_dt -0.0": (dict(sdt=-0.0), INVALID),
        "workspace one byte short": (dict(wsb="-1"), WORKSPACE), "workspace 4 bytes off a 16-byte boundary": (dict(ws="+4"), WORKSPACE),
    }
    table = dict(common)
    table.update({"comp_dis NULL": (dict(cd=None), INVALID), "eval_mask without gm0": (dict(gm=None), INVALID),
                  "eval_mask without bounds": (dict(bounds=None), INVALID)})
    call = Call(ops.inputs + [valid], [CD, RF], WS, [MASK])
    for name, (change, status) in table.items():
        a = _mutate(base, change)
        call.refused("himo_compdis_batch", name, lib.himo_compdis_batch(*[a[k] for k in BATCH]), status)

    # the ground-truth writer
    h = (ctypes.c_int64 * _lib.GT_MAX_COLUMNS)()
    nb = int(lib.himo_gt_column_starts(d.T, 3, h))
    BODY, BO = GuardedBytes(nb + 16, gpu), gbytes(gpu, np.array([0, nb], np.int64))
    CAT, INST = gbytes(gpu, d.cat), gbytes(gpu, d.inst)
    gbase = dict(base, cat=CAT.ptr, inst=INST.ptr, columns=3, bo=BO.ptr, body=BODY.ptr)
    table = dict(common)
    table.update({"bounds NULL": (dict(bounds=None), INVALID), "body_offsets NULL": (dict(bo=None), INVALID), "RAW": (dict(flags=RAW), INVALID),
                  "an unknown column bit": (dict(columns=4), INVALID), "gm0 NULL": (dict(gm=None), INVALID), "body NULL": (dict(body=None), INVALID),
                  "HAS_CATEGORY without the column": (dict(cat=None), INVALID), "HAS_INSTANCE without the column": (dict(inst=None), INVALID),
                  "body 4 bytes off an 8-byte boundary": (dict(body="+4"), INVALID), "pc0 1 byte off a 4-byte boundary": (dict(pc="+1"), INVALID),
                  "flow 2 bytes off": (dict(flow="+2"), INVALID), "lidar_dt 1 byte off": (dict(dt="+1"), INVALID),
                  "instance 2 bytes off": (dict(inst="+2"), INVALID)})
    call = Call(ops.inputs + [valid, BO, CAT, INST], [], WS, [BODY])
    for name, (change, status) in table.items():
        a = _mutate(gbase, change)
        call.refused("himo_compdis_gt_batch", name, lib.himo_compdis_gt_batch(*[a[k] for k in GT]), status)
    assert lib.himo_gt_body_bytes(0, 3) == 0 and lib.himo_gt_body_bytes(-5, 3) == 0

    # the single-frame wrapper
    dbl = ctypes.c_double * 16
    h0, h1 = dbl(*d.pose0[0].reshape(-1).tolist()), dbl(*d.pose1[0].reshape(-1).tolist())
    sing = dbl(*co.pose_pair("singular")[1].reshape(-1).tolist())
    need1 = int(lib.himo_compdis_workspace_bytes(1))
    fbase = dict(T=d.T, h0=h0, h1=h1, pc=ops.PC.ptr, stride=4, flow=ops.FL.ptr, dt=ops.DT.ptr, sdt=0.1, flags=0, cd=CD.ptr, rf=RF.ptr, ws=WS.ptr,
                 wsb=need1, stream=_s())
    table = {
        "n_points < 0": (dict(T=-1), INVALID), "pc_stride < 3": (dict(stride=1), INVALID), "pose0 NULL": (dict(h0=None), INVALID),
        "workspace NULL": (dict(ws=None), INVALID), "pose1 NULL without POSE_IS_EGO": (dict(h1=None), INVALID),
        "n_points == 0 (max() of an empty sequence)": (dict(T=0), EMPTY),
        "pc0 NULL": (dict(pc=None), INVALID), "lidar_dt NULL": (dict(dt=None), INVALID), "comp_dis NULL": (dict(cd=None), INVALID),
        "flow NULL": (dict(flow=None), INVALID), "sensor_dt 0": (dict(sdt=0.0), INVALID), "sensor_dt -0.0": (dict(sdt=-0.0), INVALID),
        "workspace one byte short": (dict(wsb="-1"), WORKSPACE), "workspace 4 bytes off a 16-byte boundary": (dict(ws="+4"), WORKSPACE),
        "singular pose1": (dict(h1=sing), SINGULAR), "all-zero pose1": (dict(h1=dbl()), SINGULAR),
    }
    call = Call([ops.PC, ops.FL, ops.DT], [CD, RF], WS)
    for name, (change, status) in table.items():
        a = _mutate(fbase, change)
        call.refused("himo_compdis_frame", name, lib.himo_compdis_frame(*[a[k] for k in FRAME]), status)
    # with POSE_IS_EGO the same singular matrix is a transform like any other: not refused
    a = _mutate(fbase, dict(h0=sing, h1=None, flags=IS_EGO))
    assert lib.himo_compdis_frame(*[a[k] for k in FRAME]) == 0
    torch.cuda.synchronize()

    # the utilities
    n = 8
    A, B, O = gfloats(gpu, n, 3, 3, 0, d.flow[:n] if d.T >= n else np.ones((n, 3))), gfloats(gpu, n, 1, 1, 0, np.ones(n)), gfloats(gpu, n, 3, 3)
    OB = gbytes(gpu, nbytes=n)
    WS2 = GuardedBytes(need1, gpu)
    call = Call([A, B], [O], WS2, [OB])
    s = _s()
    for name, args, status in (("n < 0", (-1, A.ptr, B.ptr, 0.1, 0, O.ptr, s), INVALID), ("flow NULL", (n, None, B.ptr, 0.1, 0, O.ptr, s), INVALID),
                               ("dt0 NULL", (n, A.ptr, None, 0.1, 0, O.ptr, s), INVALID), ("out NULL", (n, A.ptr, B.ptr, 0.1, 0, None, s), INVALID),
                               ("float32 flow with float64 dt0 (the result would be promoted)", (n, A.ptr, B.ptr, 0.1, 2, O.ptr, s), INVALID)):
        call.refused("himo_flow2compdis", name, lib.himo_flow2compdis(*args), status)
    for name, args, status in (("n < 0", (-1, A.ptr, 3, A.ptr, 0, O.ptr, s), INVALID), ("pc_stride < 3", (n, A.ptr, 2, A.ptr, 0, O.ptr, s), INVALID),
                               ("pc NULL", (n, None, 3, A.ptr, 0, O.ptr, s), INVALID), ("ds NULL", (n, A.ptr, 3, None, 0, O.ptr, s), INVALID),
                               ("out NULL", (n, A.ptr, 3, A.ptr, 0, None, s), INVALID)):
        call.refused("himo_refine_pts", name, lib.himo_refine_pts(*args), status)
    for name, args, status in (("n < 0", (-1, A.ptr, 3, bounds, OB.ptr, s), INVALID), ("pc_stride < 3", (n, A.ptr, 0, bounds, OB.ptr, s), INVALID),
                               ("bounds NULL", (n, A.ptr, 3, None, OB.ptr, s), INVALID), ("pts NULL", (n, None, 3, bounds, OB.ptr, s), INVALID),
                               ("out NULL", (n, A.ptr, 3, bounds, None, s), INVALID)):
        call.refused("himo_ego_pts_mask", name, lib.himo_ego_pts_mask(*args), status)
    for name, args, status in (("n < 0", (-1, B.ptr, O.ptr, WS2.ptr, s), INVALID), ("workspace NULL", (n, B.ptr, O.ptr, None, s), INVALID),
                               ("n == 0 (max() of an empty sequence)", (0, B.ptr, O.ptr, WS2.ptr, s), EMPTY),
                               ("lidar_dt NULL", (n, None, O.ptr, WS2.ptr, s), INVALID), ("dt0 NULL", (n, B.ptr, None, WS2.ptr, s), INVALID)):
        call.refused("himo_dt0", name, lib.himo_dt0(*args), status)
    # n == 0 is not a refusal of the three element-wise operators: status 0, nothing written
    assert lib.himo_flow2compdis(0, None, None, 0.1, 0, None, s) == 0 and lib.himo_refine_pts(0, None, 3, None, 0, None, s) == 0
    assert lib.himo_ego_pts_mask(0, None, 3, bounds, None, s) == 0
    call.check("n == 0")
    assert O.untouched() and bool(torch.all(OB.buf == BYTE_FILL))
