"""Conformance of the training-mode BatchNorm kernels (csrc/batchnorm.hip) over what their entry points admit, not only the
layouts the trainer feeds them: himo_bn_train_fwd, himo_bn_train_bwd, himo_bn_train_bwd_x, himo_bn_fold, with workspaces of
exactly himo_bn_workspace_bytes.

For every case of oracle/bn_oracle.py's matrix the library must return every output within the worst-case bound of the oracle
against float64 and within its aggregate ratio R_ELEM of the float32 twin, with the inputs bit-unchanged (except where an output
aliases one on purpose), no byte outside an output view or the workspace written, the same bits from a second run (the file
claims fixed reduction trees), and the same bits from himo_bn_train_bwd_x (x + mean) as from himo_bn_train_bwd (the forward
pass's xhat).  Every refusal must return the status the entry point returns in the source and write nothing.  Operands, outputs
and workspaces all live in NaN- or byte-filled guarded buffers (oracle/guarded.py): a read outside an input view poisons the
result.

The case strings name the kernels the host code launches (mirrored from csrc/batchnorm.hip:274-373 by bn_oracle.dispatch); the
module summary lists which were met, and at which block counts.
"""
import pytest
import torch

import bn_oracle as bo
from guarded import BYTE_FILL, Guarded, GuardedBytes, layout

pytestmark = pytest.mark.gpu

STATS = {}        # output -> [worst err / bound, worst rms ratio, checks, case of the first, case of the second]
KERNELS = {}      # kernel name -> cases that met it
BLOCKS = {}       # block count of the partial kernels -> cases
REFUSED = []      # (entry point, case, status)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nbn conformance: per output, the largest err/bound and rms ratio over the matrix")
    for fam, (w, r, n, wc, rc) in sorted(STATS.items()):
        print(f"  {fam:14s} err/bound {w:.3g}  rms ratio {r:.3g} (R {bo.R_ELEM:g})  {n} checks\n    worst err/bound: {wc}\n    worst rms: {rc}")
    print("  kernels met: " + ", ".join(f"{k} x{v}" for k, v in sorted(KERNELS.items())))
    print("  block counts met: " + ", ".join(f"{k} x{v}" for k, v in sorted(BLOCKS.items())))
    print(f"  refused: {len(REFUSED)}")
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
    from himo_amd.seflow import train                         # noqa: F401  (registers the signatures)
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def _met(kernel):
    KERNELS[kernel] = KERNELS.get(kernel, 0) + 1


def _ok(key, got, ref, bnd, twin, case):
    assert not bool(torch.isnan(got).any()), f"{case} {key}: NaN in the result (a read outside an input view, or an output element never written)"
    worst, rr, report = bo.check_map(got, ref, bnd, twin, f"{case} {key}")
    print(f"    {report}")
    s = STATS.setdefault(key, [0.0, 0.0, 0, "", ""])
    if worst >= s[0]:
        s[0], s[3] = worst, case
    if rr >= s[1]:
        s[1], s[4] = rr, case
    s[2] += 1
    assert worst <= 1.0, report
    assert rr <= bo.R_ELEM, report


# ---- guarded operands in the layouts of the matrix -----------------------------------------------------------------------------
def strides(c, which):
    """(img_stride, pitch) of operand ``which`` (x, xhat, y, dy, dx) in the case's layout (bn_oracle.MATRIX)"""
    n_img, rows, ch, lay = c["n_img"], c["rows"], c["ch"], c["layout"]
    dense = (rows * ch, ch)
    if lay in ("pitch4", "pitch32"):                          # different operands of one call at different pitches
        a, b = (4, 32) if lay == "pitch4" else (32, 4)
        p = ch + (a if which in ("x", "y", "dx") else b)
        return rows * p, p
    if lay == "gap":
        return (rows * ch + 8, ch) if which in ("x", "y", "dy") else dense
    if lay == "concat":                                       # the trainer's last encoder layer: images as channel groups of one buffer
        return (ch, n_img * ch) if which in ("y", "dy") else dense
    if lay == "alias_xhat":
        return (rows * (ch + 4), ch + 4) if which in ("x", "xhat") else dense
    if lay == "alias_dx":
        return (rows * (ch + 4) + 4, ch + 4) if which in ("dy", "dx") else dense
    assert lay == "dense", lay
    return dense


def gmap(gpu, c, which, values=None):
    bs, pitch = strides(c, which)
    assert bs % 4 == 0 and pitch % 4 == 0 and pitch >= c["ch"]
    g = Guarded(layout(c["n_img"], c["n_img"], bs, 0, c["rows"], pitch, c["ch"]), gpu)
    if values is not None:
        g.put(values.float())
    return g


def gflat(gpu, numel, values=None):
    g = Guarded(layout(1, 1, 0, 0, 1, max(numel, 1), numel), gpu)
    if values is not None:
        g.put(values.float())
    return g


def vec(g):
    return g.get().reshape(-1)


def flat(g, c):
    return g.get().reshape(c["n_img"] * c["rows"], c["ch"])


class Call:
    """inputs bit-unchanged, nothing outside an output view or the workspace written, after one library call"""

    def __init__(self, inputs, outputs, ws=None):
        self.inputs, self.outputs, self.ws = inputs, outputs, ws
        self.before = [g.buf.clone() for g in inputs]

    def check(self, case):
        torch.cuda.synchronize()
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{case}: an input was written"
        for g in self.outputs:
            assert g.untouched_outside(), f"{case}: a write outside an output view (pitch gap, image gap, another image's channels or guard)"
        if self.ws is not None:
            assert self.ws.untouched_outside(), f"{case}: a write outside the workspace size the query returned"

    def refused(self, fn, case, st, status):
        torch.cuda.synchronize()
        assert st == status, f"{fn} {case}: status {st}, the source returns {status}"
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{fn} {case}: refused but wrote an input"
        for g in self.outputs:
            assert g.untouched(), f"{fn} {case}: refused (status {st}) but wrote"
        if self.ws is not None:
            assert bool(torch.all(self.ws.buf == BYTE_FILL)), f"{fn} {case}: refused (status {st}) but wrote the workspace"
        REFUSED.append((fn, case, st))


# ---- the matrix -----------------------------------------------------------------------------------------------------------------
def _forward(lib, gpu, c, need, with_xhat, with_running, case):
    ch = c["ch"]
    alias = c["layout"] == "alias_xhat" and with_xhat
    X, Y = gmap(gpu, c, "x", c["x"]), gmap(gpu, c, "y")
    XH = X if alias else (gmap(gpu, c, "xhat") if with_xhat else None)
    GA, BE, M, IS = gflat(gpu, ch, c["gamma"]), gflat(gpu, ch, c["beta"]), gflat(gpu, ch), gflat(gpu, ch)
    RM, RV = (gflat(gpu, ch, c["rm"]), gflat(gpu, ch, c["rv"])) if with_running else (None, None)
    WS = GuardedBytes(need, gpu)
    hs, hp = strides(c, "xhat") if with_xhat else (0, 0)
    call = Call([GA, BE] + ([] if alias else [X]), [g for g in (Y, XH, M, IS, RM, RV) if g is not None], WS)
    st = lib.himo_bn_train_fwd(c["n_img"], c["rows"], ch, X.ptr, *strides(c, "x"), GA.ptr, BE.ptr, c["eps"], c["momentum"],
                               RM.ptr if RM else None, RV.ptr if RV else None, M.ptr, IS.ptr, XH.ptr if XH else None, hs, hp,
                               Y.ptr, *strides(c, "y"), WS.ptr, need, _s())
    assert st == 0, f"{case}: status {st}"
    call.check(case)
    return dict(X=X, Y=Y, XH=XH, GA=GA, BE=BE, M=M, IS=IS, RM=RM, RV=RV)


def _backward(lib, gpu, c, need, f, src, from_x, case):
    """src: the guarded xhat (the forward pass's output) or, from_x, the guarded x"""
    ch = c["ch"]
    alias = c["layout"] == "alias_dx"
    acc = bool(c["flags"] & 1)
    DY = gmap(gpu, c, "dy", c["dy"])
    DX = DY if alias else gmap(gpu, c, "dx")
    DG, DB = gflat(gpu, ch, c["old_dgamma"] if acc else None), gflat(gpu, ch, c["old_dbeta"] if acc else None)
    WS = GuardedBytes(need, gpu)
    call = Call([src, f["GA"], f["BE"], f["M"], f["IS"]] + ([] if alias else [DY]), [DX, DG, DB], WS)
    head = (c["n_img"], c["rows"], ch, DY.ptr, *strides(c, "dy"), src.ptr, *strides(c, "x" if from_x else "xhat"), f["GA"].ptr, f["BE"].ptr)
    tail = (f["IS"].ptr, DX.ptr, *strides(c, "dx"), DG.ptr, DB.ptr, c["flags"], WS.ptr, need, _s())
    st = lib.himo_bn_train_bwd_x(*head, f["M"].ptr, *tail) if from_x else lib.himo_bn_train_bwd(*head, *tail)
    assert st == 0, f"{case}: status {st}"
    call.check(case)
    return dict(DX=DX, DG=DG, DB=DB)


def _same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is not None:
            assert torch.equal(a[k].words(), b[k].words()), f"{what}: {k} differs"


@pytest.mark.parametrize("name", bo.CASE_NAMES)
def test_bn_train_case(lib, gpu, name):
    c = bo.case(name)
    ref, bnd, twin = bo.refs(name)
    N, ch = c["x"].shape
    d = bo.dispatch(N, ch)
    running = c["rm"] is not None
    need = int(lib.himo_bn_workspace_bytes(N, ch))
    assert need > 0
    case = (f"{name}: n_img={c['n_img']} rows={c['rows']} ch={ch} layout={c['layout']} eps={c['eps']:g} momentum={c['momentum']:g} "
            f"flags={c['flags']} running={running} qs={d['qs']} rows_pb={d['rows_pb']} blocks={d['nb']}x{d['tiles']}")
    print(f"\n  {case}")
    BLOCKS[d["nb"]] = BLOCKS.get(d["nb"], 0) + 1
    # forward
    f1 = _forward(lib, gpu, c, need, True, running, case + " fwd")
    for k in (f"bn_stats_partial_kernel qs={d['qs']}", "bn_stats_finalize_kernel", "bn_normalize_gelu_kernel (xhat)"):
        _met(k)
    _ok("mean", vec(f1["M"]), ref["mean"], bnd["mean"], twin["mean"], case)
    _ok("invstd", vec(f1["IS"]), ref["invstd"], bnd["invstd"], twin["invstd"], case)
    if running:
        _ok("running_mean", vec(f1["RM"]), ref["running_mean"], bnd["running_mean"], twin["running_mean"], case)
        _ok("running_var", vec(f1["RV"]), ref["running_var"], bnd["running_var"], twin["running_var"], case)
    _ok("xhat", flat(f1["XH"], c), ref["xhat"], bnd["xhat"], twin["xhat"], case)
    _ok("y", flat(f1["Y"], c), ref["y"], bnd["y"], twin["y"], case)
    f2 = _forward(lib, gpu, c, need, True, running, case + " fwd again")
    _same_bits(f1, f2, ("Y", "XH", "M", "IS", "RM", "RV"), case + ": a second forward run")
    f3 = _forward(lib, gpu, c, need, False, False, case + " fwd, xhat and running statistics NULL")
    _met("bn_normalize_gelu_kernel (no xhat)")
    _same_bits(f1, f3, ("Y", "M", "IS"), case + ": forward without xhat")
    del f2
    # backward from the forward pass's xhat, again, and from x + mean
    b1 = _backward(lib, gpu, c, need, f1, f1["XH"], False, case + " bwd")
    for k in (f"bn_bwd_partial_kernel<false> qs={d['qs']}", f"bn_bwd_finalize_kernel accumulate={c['flags'] & 1}", "bn_bwd_apply_kernel<false>"):
        _met(k)
    _ok("dbeta", vec(b1["DB"]), ref["dbeta"], bnd["dbeta"], twin["dbeta"], case)
    _ok("dgamma", vec(b1["DG"]), ref["dgamma"], bnd["dgamma"], twin["dgamma"], case)
    _ok("dx", flat(b1["DX"], c), ref["dx"], bnd["dx"], twin["dx"], case)
    b2 = _backward(lib, gpu, c, need, f1, f1["XH"], False, case + " bwd again")
    _same_bits(b1, b2, ("DX", "DG", "DB"), case + ": a second backward run")
    del b2
    b3 = _backward(lib, gpu, c, need, f3, f3["X"], True, case + " bwd_x")
    for k in (f"bn_bwd_partial_kernel<true> qs={d['qs']}", "bn_bwd_apply_kernel<true>"):
        _met(k)
    _same_bits(b1, b3, ("DX", "DG", "DB"), case + ": himo_bn_train_bwd_x against himo_bn_train_bwd")


# ---- himo_bn_fold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 4, 255, 256, 257])
def test_bn_fold(lib, gpu, ch):
    """any ch >= 1 (one block and the second block's first lane), var including 0, both eps of the specification"""
    g = torch.Generator().manual_seed(900 + ch)
    gamma, beta, mean = torch.randn(ch, generator=g), torch.randn(ch, generator=g), torch.randn(ch, generator=g) * 3
    var = torch.rand(ch, generator=g) * 10.0 ** (-6 * torch.rand(ch, generator=g))
    var[::3] = 0.0
    for eps in (bo.BN_EPS, bo.BN_EPS_PFN):
        ins = [gflat(gpu, ch, v) for v in (gamma, beta, mean, var)]
        SC, SH = gflat(gpu, ch), gflat(gpu, ch)
        call = Call(ins, [SC, SH])
        case = f"bn_fold ch={ch} eps={eps:g}"
        assert lib.himo_bn_fold(ch, *[t.ptr for t in ins], eps, SC.ptr, SH.ptr, _s()) == 0, case
        call.check(case)
        _met("bn_fold_kernel")
        s, h = bo.fold(gamma, beta, mean, var, eps)
        s32, h32 = bo.fold(gamma, beta, mean, var, eps, torch.float32)
        bs, bh = bo.fold_bound(gamma, beta, mean, var, eps)
        _ok("fold scale", vec(SC), s, bs, s32, case)
        _ok("fold shift", vec(SH), h, bh, h32, case)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
INVALID, WORKSPACE, UNSUPPORTED = 1, 3, 6                     # _lib.ERR_* (asserted below), as read from csrc/batchnorm.hip:278-286, :337-343, :368
FWD = ("n_img", "rows", "ch", "x", "xs", "xp", "gamma", "beta", "eps", "momentum", "rm", "rv", "mean", "invstd", "xhat", "hs", "hp",
       "y", "ys", "yp", "ws", "wsb", "stream")
BWD = ("n_img", "rows", "ch", "dy", "dys", "dyp", "xhat", "hs", "hp", "gamma", "beta", "invstd", "dx", "dxs", "dxp", "dgamma", "dbeta",
       "flags", "ws", "wsb", "stream")
BWD_X = BWD[:11] + ("mean",) + BWD[11:]
SHAPE = {"n_img < 1": dict(n_img=0), "rows < 1": dict(rows=0), "ch < 4 (0)": dict(ch=0), "ch < 4 (2)": dict(ch=2), "ch % 4": dict(ch=10)}
BIG = {"total ch / 4 >= 2^31": dict(n_img=1, rows=1 << 30)}   # with ch = 8: 2^30 rows x 2 quads


def _refusal_table(maps, nulls, extra_invalid=()):
    t = {k: (v, INVALID) for k, v in SHAPE.items()}
    for k in nulls:
        t[f"{k} NULL"] = ({k: None}, INVALID)
    t["workspace NULL"] = (dict(ws=None), INVALID)
    for k, v in extra_invalid:
        t[k] = (v, INVALID)
    for p, s_, q in maps:                                       # (pointer, image stride, pitch) argument names of every map
        t[f"{p} 4 bytes off a 16-byte boundary"] = ({p: "+4"}, UNSUPPORTED)
        t[f"{s_} % 4"] = ({s_: 42}, UNSUPPORTED)
        t[f"{q} % 4"] = ({q: 10}, UNSUPPORTED)
        t[f"{q} < ch"] = ({q: 4}, UNSUPPORTED)
    t.update({k: (v, UNSUPPORTED) for k, v in BIG.items()})
    t["workspace one byte short"] = (dict(wsb="-1"), WORKSPACE)
    t["workspace 4 bytes off a 16-byte boundary"] = (dict(ws="+4"), WORKSPACE)
    return t


def _mutate(base, change):
    a = dict(base)
    for k, v in change.items():
        a[k] = base[k] + 4 if v == "+4" else (base[k] - 1 if v == "-1" else v)
    return a


def test_refusals(lib, gpu):
    """every refusal of the three training entry points: the status the source returns, and not a byte written -- outputs,
    in/out running statistics and workspace alike"""
    from himo_amd import _lib
    assert (_lib.ERR_INVALID_ARGUMENT, _lib.ERR_WORKSPACE, _lib.ERR_UNSUPPORTED) == (INVALID, WORKSPACE, UNSUPPORTED)
    n_img, rows, ch = 2, 5, 8
    c = dict(n_img=n_img, rows=rows, ch=ch, layout="dense")
    g = torch.Generator().manual_seed(77)
    need = int(lib.himo_bn_workspace_bytes(n_img * rows, ch))
    X, DY, XH_in = (gmap(gpu, c, w, torch.randn(n_img * rows, ch, generator=g)) for w in ("x", "dy", "xhat"))
    GA, BE, M_in, IS_in = (gflat(gpu, ch, torch.rand(ch, generator=g) + 0.5) for _ in range(4))
    Y, XH, DX = gmap(gpu, c, "y"), gmap(gpu, c, "xhat"), gmap(gpu, c, "dx")
    M, IS, RM, RV, DG, DB = (gflat(gpu, ch) for _ in range(6))
    WS = GuardedBytes(need + 16, gpu)                          # room for the misaligned pointer; the size passed stays ``need``
    bs = rows * ch
    fwd = dict(n_img=n_img, rows=rows, ch=ch, x=X.ptr, xs=bs, xp=ch, gamma=GA.ptr, beta=BE.ptr, eps=bo.BN_EPS, momentum=0.1, rm=RM.ptr, rv=RV.ptr,
               mean=M.ptr, invstd=IS.ptr, xhat=XH.ptr, hs=bs, hp=ch, y=Y.ptr, ys=bs, yp=ch, ws=WS.ptr, wsb=need, stream=_s())
    table = _refusal_table((("x", "xs", "xp"), ("xhat", "hs", "hp"), ("y", "ys", "yp")), ("gamma", "beta", "mean", "invstd"),
                           (("running_mean without running_var", dict(rv=None)), ("running_var without running_mean", dict(rm=None))))
    call = Call([X, GA, BE], [Y, XH, M, IS, RM, RV], WS)
    for name, (change, status) in table.items():
        a = _mutate(fwd, change)
        call.refused("himo_bn_train_fwd", name, lib.himo_bn_train_fwd(*[a[k] for k in FWD]), status)
    bwd = dict(n_img=n_img, rows=rows, ch=ch, dy=DY.ptr, dys=bs, dyp=ch, xhat=XH_in.ptr, hs=bs, hp=ch, gamma=GA.ptr, beta=BE.ptr, mean=M_in.ptr,
               invstd=IS_in.ptr, dx=DX.ptr, dxs=bs, dxp=ch, dgamma=DG.ptr, dbeta=DB.ptr, flags=0, ws=WS.ptr, wsb=need, stream=_s())
    maps = (("dy", "dys", "dyp"), ("xhat", "hs", "hp"), ("dx", "dxs", "dxp"))
    nulls = ("gamma", "beta", "invstd", "dgamma", "dbeta")
    call = Call([DY, XH_in, GA, BE, M_in, IS_in], [DX, DG, DB], WS)
    for name, (change, status) in _refusal_table(maps, nulls).items():
        a = _mutate(bwd, change)
        call.refused("himo_bn_train_bwd", name, lib.himo_bn_train_bwd(*[a[k] for k in BWD]), status)
    for name, (change, status) in _refusal_table(maps, nulls + ("mean",)).items():
        a = _mutate(bwd, change)
        call.refused("himo_bn_train_bwd_x", name, lib.himo_bn_train_bwd_x(*[a[k] for k in BWD_X]), status)
    assert lib.himo_bn_workspace_bytes(0, ch) == 0 and lib.himo_bn_workspace_bytes(n_img * rows, 0) == 0
    # himo_bn_fold: ch < 1 and each NULL
    ins = [gflat(gpu, ch, torch.rand(ch, generator=g)) for _ in range(4)]
    SC, SH = gflat(gpu, ch), gflat(gpu, ch)
    call = Call(ins, [SC, SH])
    ptrs = [t.ptr for t in ins]
    call.refused("himo_bn_fold", "ch < 1", lib.himo_bn_fold(0, *ptrs, bo.BN_EPS, SC.ptr, SH.ptr, _s()), INVALID)
    for i, k in enumerate(("gamma", "beta", "mean", "var", "scale", "shift")):
        p = ptrs + [SC.ptr, SH.ptr]
        p[i] = None
        call.refused("himo_bn_fold", f"{k} NULL", lib.himo_bn_fold(ch, *p[:4], bo.BN_EPS, *p[4:], _s()), INVALID)
