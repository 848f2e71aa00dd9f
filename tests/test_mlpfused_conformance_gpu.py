"""Conformance of the LAYER-KERNEL path of the per-pair fit -- what FastNSF(objective="nn") takes and three_launch=False falls back
to -- over what its entry points admit: himo_mlp_forward_fused, himo_mlp_backward_fused, himo_mlp_backward_fused_bias,
himo_mlp_bias_workspace_bytes (csrc/mlpfused.hip), himo_chamfer_trunc and its size query (csrc/fastnsf.hip), himo_nsfp_prepare,
himo_nsfp_objective, himo_nsfp_keep_best and their size queries (csrc/nsfp.hip).  The entry points are called through ctypes, not
through the engines (tests/test_fastnsf_gpu.py, tests/test_nsfp_gpu.py do that).

For every call the library must either refuse it (the documented status, no byte written) or return results within the bounds of
oracle/mlpfused_oracle.py against float64 and within the project's aggregate limit of the float32 twin, with the inputs
bit-unchanged and no byte outside an output view or a workspace written.  Operands, outputs and workspaces live in guarded buffers
(oracle/guarded.py) of EXACTLY the size the library's query or contract gives: every [n][.] buffer of csrc/mlpfused.hip holds
ceil(n / 64) * 64 rows, and its padding rows are compared like the others.  Every H_k and dZ_k is compared element by element.
tests/test_mlpfused_oracle.py shows on the CPU that these checks pass the float32 twin and fail eight wrong ones.

The fully dead row of the ``dead`` cases: every FIRST-layer unit is off, so H_0 and dZ_0 of that row are exactly zero; H_k of the
deeper layers is relu(b_k + 0), which the reference demands like any other element (exactly 0 where z_k <= 0).

Pinned where include/himo_amd.h was silent (the sentences are there now): himo_chamfer_trunc squares trunc_dist, so a negative
one acts as its magnitude and a NaN one drops every term; with n0 == 0 or n1 == 0 it returns loss 0 and a zero gradient and reads
no correspondence; himo_mlp_backward_fused_bias answers a short or missing workspace with HIMO_ERR_INVALID_ARGUMENT.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_oracle as co
import grad_oracle as go
import mlpfused_oracle as mo
import nsf_oracle as no
from guarded import BYTE_FILL, NAN_BITS, Guarded, GuardedBytes

pytestmark = pytest.mark.gpu

STATS = {}        # (family, arith) -> [worst err / bound, worst rms ratio, checks, case of the first, case of the second]
REFUSED = []      # (family, case, status)
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 3, 6
PK_BYTES = 8 * 2 * 128 * 16 * 2          # the two planes himo_mlp_repack writes for a 128 x 128 layer
N_BLOCKS = (1, 7, 8, 9, 24, 25, 31, 32, 33, 57, 64, 65)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    from himo_amd import _lib
    _lib.prof_start()
    yield
    met = _lib.prof_stop()
    print("\nmlpfused conformance: per family and arithmetic, the largest err/bound and rms ratio over the matrix")
    for (fam, a), (w, r, n, wc, rc) in sorted(STATS.items()):
        lim = "-" if a == "exact" else f"{go.R_ELEM if fam in ('chamfer', 'nsfp_objective') else co.R[a]:g}"
        print(f"  {fam:15s} {a:7s} err/bound {w:.3g}  rms ratio {r:.3g} (R {lim})  {n} checks\n    worst err/bound: {wc}\n    worst rms: {rc}")
    print("  kernels met: " + ", ".join(f"{k} x{v['count']}" for k, v in sorted(met.items())))
    print(f"  refused: {len(REFUSED)}")
    for fam, case, st in REFUSED:
        print(f"    {fam}: {case}: status {st}")


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
    from himo_amd import fastnsf                              # noqa: F401  (registers the signatures)
    from himo_amd import nsfp                                 # noqa: F401
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def _run(checks, case):
    for fam, name, arith, got, ref, bnd, r32, cols in checks:
        got = torch.as_tensor(got)
        assert not bool(torch.isnan(got).any()), f"{case} {fam}/{name}: NaN in the result (a read of a guard or of a word never written)"
        good, worst, rr, report = mo.verdict(fam, arith, got, ref, bnd, r32, f"{case} {fam}/{name}", cols=cols)
        print(report)
        assert good, report
        s = STATS.setdefault((fam, arith), [0.0, 0.0, 0, "", ""])
        if worst >= s[0]:
            s[0], s[3] = worst, f"{case} {name}"
        if rr >= s[1]:
            s[1], s[4] = rr, f"{case} {name}"
        s[2] += 1


def _exact(fam, n=1):
    s = STATS.setdefault((fam, "exact"), [0.0, 0.0, 0, "bit-equal", "-"])
    s[2] += n


# ---- guarded buffers -----------------------------------------------------------------------------------------------------
def gwords(gpu, words, off=0):
    """``words`` 32-bit words, ``off`` words past the aligned base"""
    return Guarded(torch.arange(int(words), dtype=torch.int64), gpu, off=off)


def gvals(gpu, values, off=0):
    values = torch.as_tensor(values)
    g = gwords(gpu, values.numel(), off)
    g.put(values.reshape(-1) if values.dtype == torch.int32 else values.reshape(-1).float())
    return g


def gf64(gpu, values):
    return gvals(gpu, torch.as_tensor(values, dtype=torch.float64).reshape(-1).view(torch.int32))


def f64_of(g):
    return g.words().reshape(-1).view(torch.float64)


def gbytes(gpu, nbytes):
    return GuardedBytes(nbytes, gpu)


def _untouched(g):
    """no byte of the whole buffer, view included, was written"""
    if isinstance(g, GuardedBytes):
        return bool(torch.all(g.buf == BYTE_FILL))
    return g.untouched()


class Call:
    """inputs bit-unchanged and nothing outside an output view (or workspace) written, after one library call"""

    def __init__(self, inputs, outputs):
        self.inputs, self.outputs = inputs, outputs
        self.before = [g.buf.clone() for g in inputs]

    def check(self, case):
        torch.cuda.synchronize()
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{case}: an input was written"
        for g in self.outputs:
            assert g.untouched_outside(), f"{case}: a write outside an output view or workspace"

    def refused(self, fam, case, st, allowed):
        torch.cuda.synchronize()
        assert st in allowed, f"{case}: status {st}, expected one of {allowed}"
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{case}: refused but an input was written"
        for g in self.outputs:
            assert _untouched(g), f"{case}: refused (status {st}) but wrote"
        REFUSED.append((fam, case, st))


# ---- the network on the device ------------------------------------------------------------------------------------------
PTRS = ctypes.c_void_p * (no.MAX_HIDDEN + 4)


class Net:
    """a case's operands in guarded buffers of exactly block_rows(n) rows: the flat parameter vector (layer i's W at off_w[i], b at
    off_b[i]), the packed copies of the hidden layers (himo_mlp_repack), x, out, H_k, dout, dZ_k, db_k, the bias workspace"""

    def __init__(self, lib, gpu, case, x_off=0, dout_off=0):
        self.lib, self.gpu, self.case = lib, gpu, case
        L, n = case.n_hidden, case.n
        self.L, self.n, self.R = L, n, mo.block_rows(n)
        flat, self.off_w, self.off_b = no.flat(case.params)
        self.P = gvals(gpu, flat)
        self.pk_size = int(lib.himo_conv_packed_weight_bytes(1, 128, 128))
        assert self.pk_size >= PK_BYTES and self.pk_size % 4 == 0
        self.pk_f = [None] + [gwords(gpu, self.pk_size // 4) for _ in range(1, L)]
        self.pk_b = [None] + [gwords(gpu, self.pk_size // 4) for _ in range(1, L)]
        if L > 1:
            A, I = ctypes.c_void_p * (L - 1), ctypes.c_int * (L - 1)
            st = lib.himo_mlp_repack(L - 1, A(*[self.wptr(i) for i in range(1, L)]), I(*[128] * (L - 1)), I(*[128] * (L - 1)),
                                     A(*[self.pk_f[i].ptr for i in range(1, L)]), A(*[self.pk_b[i].ptr for i in range(1, L)]), _s())
            assert st == 0, st
            torch.cuda.synchronize()
        self.x = gvals(gpu, case.x[:self.R], off=x_off)
        self.out = gwords(gpu, self.R * 4)
        self.dout = gwords(gpu, self.R * 4, off=dout_off)
        self.H = [gwords(gpu, self.R * 128) for _ in range(L)]
        self.new_backward_outputs()

    def new_backward_outputs(self):
        self.dZ = [gwords(self.gpu, self.R * 128) for _ in range(self.L)]
        self.db = [gwords(self.gpu, 128) for _ in range(self.L)]
        self.ws_bytes = int(self.lib.himo_mlp_bias_workspace_bytes(self.n, self.L))
        assert self.ws_bytes == self.L * (self.R // 64) * 512 + 64
        self.ws = gbytes(self.gpu, self.ws_bytes)

    def wptr(self, i):
        return self.P.ptr + 4 * self.off_w[i]

    def bptr(self, i):
        return self.P.ptr + 4 * self.off_b[i]

    def packed(self, bufs):
        return PTRS(*([None] + [bufs[k].ptr for k in range(1, self.L)]))

    def biases(self):
        return PTRS(*([None] + [self.bptr(k) for k in range(1, self.L)]))

    def table(self, bufs):
        return PTRS(*[b.ptr for b in bufs])

    def params(self):
        return [self.P] + self.pk_f[1:] + self.pk_b[1:]

    def forward(self, **over):
        a = dict(n=self.n, x=self.x.ptr, L=self.L, w0=self.wptr(0), b0=self.bptr(0), wf=self.packed(self.pk_f), bias=self.biases(),
                 wl=self.wptr(self.L), bl=self.bptr(self.L), H=self.table(self.H), out=self.out.ptr)
        a.update(over)
        return self.lib.himo_mlp_forward_fused(*a.values(), _s())

    def backward(self, bias=False, **over):
        a = dict(n=self.n, dout=self.dout.ptr, L=self.L, wb=self.packed(self.pk_b), wl=self.wptr(self.L), H=self.table(self.H), dZ=self.table(self.dZ))
        b = dict(db=self.table(self.db), ws=self.ws.ptr, ws_bytes=self.ws_bytes)
        a.update({k: v for k, v in over.items() if k in a})
        b.update({k: v for k, v in over.items() if k in b})
        if bias:
            return self.lib.himo_mlp_backward_fused_bias(*a.values(), *b.values(), _s())
        return self.lib.himo_mlp_backward_fused(*a.values(), _s())

    def got_forward(self):
        return dict(H=[h.get().reshape(self.R, 128) for h in self.H], out=self.out.get().reshape(self.R, 4))


def _name(what, n, n_hidden, dead):
    return f"{what} n {n} hidden {n_hidden}{' dead' if dead else ''}"


def _forward(lib, gpu, case, name):
    net = Net(lib, gpu, case)
    call = Call(net.params() + [net.x], net.H + [net.out])
    st = net.forward()
    assert st == 0, f"{name}: status {st}"
    call.check(name)
    for g in net.H + [net.out]:
        assert not bool((g.words() == NAN_BITS).any()), f"{name}: an output row was not written (the padding rows are stored too)"
    assert _untouched(net.dout) and all(_untouched(g) for g in net.dZ + net.db + [net.ws])
    return net


def _dead_row(case):
    return int(torch.nonzero((case.x[:case.n, :3] == torch.tensor(no.SPECIAL_DEAD)).all(1))[0])


@pytest.mark.parametrize("n,n_hidden,dead", no.FWD_CASES)
def test_forward(lib, gpu, n, n_hidden, dead):
    case, name = no.mlp_case(n, n_hidden, dead), _name("forward", n, n_hidden, dead)
    net = _forward(lib, gpu, case, name)
    got = net.got_forward()
    _run(mo.mlpfused_checks(case, got), name)
    if dead and n >= 63:
        assert not got["H"][0][_dead_row(case)].any(), f"{name}: the dead row's H_0 is not zero"


def _backward(lib, gpu, case, name):
    """both backward entry points on the kernel's OWN H_k and case.dout -> (net, dZ of the bias entry point, db)"""
    net = _forward(lib, gpu, case, name)
    net.dout.put(case.dout[:net.R])
    inputs = net.params() + net.H + [net.dout]
    call = Call(inputs, net.dZ)
    st = net.backward()
    assert st == 0, f"{name}: backward status {st}"
    call.check(name)
    assert all(_untouched(g) for g in net.db + [net.ws]), f"{name}: himo_mlp_backward_fused wrote a bias gradient or the workspace"
    plain = [z.words() for z in net.dZ]
    net.new_backward_outputs()
    call = Call(inputs, net.dZ + net.db + [net.ws])
    st = net.backward(bias=True)
    assert st == 0, f"{name}: backward_bias status {st}"
    call.check(name)
    for k in range(net.L):
        assert torch.equal(net.dZ[k].words(), plain[k]), f"{name}: dZ{k} of himo_mlp_backward_fused_bias differs from himo_mlp_backward_fused's"
        assert not bool((plain[k] == NAN_BITS).any()), f"{name}: a row of dZ{k} was not written"
    _exact("mlp_backward", net.L)
    return net, [z.get().reshape(net.R, 128) for z in net.dZ], [b.get() for b in net.db]


@pytest.mark.parametrize("n,n_hidden,dead", no.BWD_CASES)
def test_backward_and_bias(lib, gpu, n, n_hidden, dead):
    case, name = mo.mlp_case(n, n_hidden, dead), _name("backward", n, n_hidden, dead)
    net, dZ, db = _backward(lib, gpu, case, name)
    got = net.got_forward()
    got.update(dZ=dZ, db=db)
    _run(mo.mlpfused_checks(case, got), name)
    if dead and n >= 63:
        row = _dead_row(case)
        assert not got["H"][0][row].any() and not dZ[0][row].any(), f"{name}: the dead row's H_0 / dZ_0 is not zero"
    for k in range(n_hidden):
        assert not dZ[k][n:].any(), f"{name}: dZ{k} of a padding row is not zero"


def test_relu_at_exactly_zero(lib, gpu):
    """a point at the origin and first-layer biases of exactly 0: z = 0 -> H = 0 and no gradient passes (the z > 0 convention)"""
    case = mo.mask_case()
    net, dZ, db = _backward(lib, gpu, case, "mask threshold")
    got = net.got_forward()
    got.update(dZ=dZ, db=db)
    _run(mo.mlpfused_checks(case, got), "mask threshold")
    for j in no.MASK_ZERO_BIAS:
        assert float(got["H"][0][0, j]) == 0.0 and float(dZ[0][0, j]) == 0.0 and float(case.ref["gs"][0][0, j]) != 0.0


@pytest.mark.parametrize("n_blocks", N_BLOCKS)
def test_bias_reduce_alone(lib, gpu, n_blocks):
    """the boundaries of the reduce's stride-32 loop (b + 24 < n_blocks) and of its stride-8 tail, on the kernel's own dZ"""
    case = mo.reduce_case(n_blocks)
    name = f"bias reduce, {n_blocks} blocks"
    net, dZ, db = _backward(lib, gpu, case, name)
    _run(mo.bias_reduce_checks(dZ, db, n_blocks), name)


# ---- Chamfer on hand-made correspondences -----------------------------------------------------------------------------------------
class Chamfer:
    def __init__(self, lib, gpu, c):
        self.lib, self.c = lib, c
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32))
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
        self.moved, self.pc1 = gvals(gpu, f32(c.moved)), gvals(gpu, f32(c.pc1))
        self.d_a, self.i_a, self.d_b, self.i_b = gvals(gpu, f32(c.d_a)), gvals(gpu, i32(c.i_a)), gvals(gpu, f32(c.d_b)), gvals(gpu, i32(c.i_b))
        self.loss, self.grad = gwords(gpu, 2), gwords(gpu, 3 * c.n0)
        self.ws_bytes = int(lib.himo_chamfer_trunc_workspace_bytes(c.n0, c.n1))
        self.ws = gbytes(gpu, self.ws_bytes)
        self.inputs = [self.moved, self.pc1, self.d_a, self.i_a, self.d_b, self.i_b]

    def __call__(self, **over):
        c = self.c
        both = c.n0 > 0 and c.n1 > 0                             # otherwise no correspondence is read: none is passed
        p = lambda g, on: g.ptr if on else None
        a = dict(n0=c.n0, n1=c.n1, moved=p(self.moved, c.n0), pc1=p(self.pc1, both), d_a=p(self.d_a, both), i_a=p(self.i_a, both), d_b=p(self.d_b, both),
                 i_b=p(self.i_b, both), trunc=c.trunc, loss=self.loss.ptr, grad=p(self.grad, c.n0), ws=self.ws.ptr, ws_bytes=self.ws_bytes)
        a.update(over)
        return self.lib.himo_chamfer_trunc(*a.values(), _s())

    def got(self):
        return dict(loss=float(f64_of(self.loss)[0]), grad=self.grad.get().reshape(self.c.n0, 3))


@pytest.mark.parametrize("n0,n1", mo.CHAMFER_CASES)
def test_chamfer_with_hand_made_correspondences(lib, gpu, n0, n1):
    c, name = mo.chamfer_case(n0, n1), f"chamfer {n0} x {n1}"
    ch = Chamfer(lib, gpu, c)
    call = Call(ch.inputs, [ch.loss, ch.grad, ch.ws])
    runs = []
    for i in range(2):                                           # the second call on the same workspace: the same bits
        st = ch()
        assert st == 0, f"{name}: status {st}"
        call.check(name)
        runs.append((ch.loss.words().clone(), ch.grad.words().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{name}: a second call gives other bits"
    got = ch.got()
    _run(mo.chamfer_checks(c, got), name)
    if n0 == 0 or n1 == 0:
        assert got["loss"] == 0.0 and not got["grad"].any()
    if n1 > mo.FAN_IN:
        g = got["grad"][mo.FAN_ROW]
        assert g[0] < 0 and g[1] == 0.0 and g[2] > 0, f"{name}: the fan-in row's sums {g.tolist()}"


def test_chamfer_squares_its_trunc(lib, gpu):
    """pinned: t2 = trunc_dist * trunc_dist, so -0.5 is 0.5 (the same bits), and a NaN drops every term"""
    c = mo.chamfer_case(257, 255)
    ch = Chamfer(lib, gpu, c)
    assert ch() == 0
    torch.cuda.synchronize()
    want = (ch.loss.words().clone(), ch.grad.words().clone())
    neg = Chamfer(lib, gpu, c)
    call = Call(neg.inputs, [neg.loss, neg.grad, neg.ws])
    assert neg(trunc=-0.5) == 0
    call.check("chamfer trunc -0.5")
    assert torch.equal(neg.loss.words(), want[0]) and torch.equal(neg.grad.words(), want[1])
    nan = Chamfer(lib, gpu, c)
    call = Call(nan.inputs, [nan.loss, nan.grad, nan.ws])
    assert nan(trunc=float("nan")) == 0
    call.check("chamfer trunc NaN")
    got = nan.got()
    assert got["loss"] == 0.0 and not got["grad"].any() and not bool((nan.grad.words() == NAN_BITS).any())
    _exact("chamfer", 2)


# ---- the NSFP objective ---------------------------------------------------------------------------------------------------------------
def _grid():
    from himo_amd.ssl_loss import GRID_CELL, GRID_H, GRID_W, GRID_X0, GRID_Y0
    return GRID_X0, GRID_Y0, GRID_CELL, GRID_W, GRID_H


class Objective:
    def __init__(self, lib, gpu, c):
        self.lib, self.c = lib, c
        n0, n1 = c.n0, c.n1
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
        self.n_pad, self.parts = int(lib.himo_nsf_padded_rows(n0)), int(lib.himo_nsfp_partials(n0, n1))
        assert self.n_pad == len(c.x0) and self.parts == self.n_pad // 64 + (n1 + 255) // 256
        self.x0, self.out, self.pc1 = gvals(gpu, f32(c.x0)), gvals(gpu, f32(c.out)), gvals(gpu, f32(c.pc1))
        self.moved, self.d_a, self.i_a = gwords(gpu, 3 * n0), gwords(gpu, n0), gwords(gpu, n0)
        self.d_b, self.i_b = gwords(gpu, n1), gwords(gpu, n1)
        self.dout, self.lp, self.cp = gwords(gpu, 4 * self.n_pad), gwords(gpu, 2 * self.parts), gwords(gpu, self.parts)
        self.ws_bytes = int(lib.himo_nsfp_workspace_bytes(n0, n1, *_grid()[3:]))
        self.ws = gbytes(gpu, self.ws_bytes)
        self.inputs = [self.x0, self.out, self.pc1]
        self.outputs = [self.moved, self.d_a, self.i_a, self.d_b, self.i_b, self.dout, self.lp, self.cp]

    def prepare(self, **over):
        a = dict(n0=self.c.n0, n1=self.c.n1, pc1=self.pc1.ptr if self.c.n1 else None, grid=_grid(), ws=self.ws.ptr, ws_bytes=self.ws_bytes)
        a.update(over)
        return self.lib.himo_nsfp_prepare(a["n0"], a["n1"], a["pc1"], *a["grid"], a["ws"], a["ws_bytes"], _s())

    def __call__(self, **over):
        c, on = self.c, self.c.n1 > 0
        a = dict(n0=c.n0, n1=c.n1, x0=self.x0.ptr, out=self.out.ptr, pc1=self.pc1.ptr if on else None, grid=_grid(), trunc=c.trunc, moved=self.moved.ptr,
                 d_a=self.d_a.ptr, i_a=self.i_a.ptr, d_b=self.d_b.ptr if on else None, i_b=self.i_b.ptr if on else None, dout=self.dout.ptr,
                 lp=self.lp.ptr, cp=self.cp.ptr, ws=self.ws.ptr, ws_bytes=self.ws_bytes)
        a.update(over)
        return self.lib.himo_nsfp_objective(a["n0"], a["n1"], a["x0"], a["out"], a["pc1"], *a["grid"], a["trunc"], a["moved"], a["d_a"], a["i_a"],
                                            a["d_b"], a["i_b"], a["dout"], a["lp"], a["cp"], a["ws"], a["ws_bytes"], _s())


@pytest.mark.parametrize("n0,n1", mo.NSFP_CASES)
def test_nsfp_objective_on_a_lattice_with_out_not_zero(lib, gpu, n0, n1):
    c, name = mo.nsfp_case(n0, n1), f"nsfp objective {n0} x {n1}"
    ob = Objective(lib, gpu, c)
    call = Call(ob.inputs, ob.outputs + [ob.ws])
    assert ob.prepare() == 0
    call.check(name + " prepare")
    assert all(_untouched(g) for g in ob.outputs)
    runs = []
    for i in range(2):                                           # the workspace is left so that a second identical call gives the same bytes
        st = ob()
        assert st == 0, f"{name}: status {st}"
        call.check(name)
        runs.append([g.words().clone() for g in ob.outputs])
    for a, b, what in zip(runs[0], runs[1], ("moved", "d_a", "i_a", "d_b", "i_b", "dout", "lp", "cp")):
        assert torch.equal(a, b), f"{name}: {what} differs in a second call"
    ref = mo.nsfp_objective(c)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32).reshape(-1)
    assert np.array_equal(ob.moved.words().numpy(), bits(ref["moved"])), f"{name}: moved is not float32(x0 + out)"
    assert np.array_equal(ob.d_a.words().numpy(), bits(ref["d_a"])) and np.array_equal(ob.i_a.words().numpy(), ref["i_a"]), f"{name}: moved -> pc1"
    assert np.array_equal(ob.d_b.words().numpy(), bits(ref["d_b"])) and np.array_equal(ob.i_b.words().numpy(), ref["i_b"]), f"{name}: pc1 -> moved"
    assert np.array_equal(ob.cp.words().numpy(), ref["cp"]), f"{name}: count_partial {ob.cp.words().tolist()}"
    if n0 == 1:
        assert ob.cp.words()[:4].tolist() == [1, 0, 0, 0]
    _exact("nsfp_objective", 6)
    dout = ob.dout.get().reshape(-1, 4)
    assert not dout[n0:].any() and not dout[:, 3].any(), f"{name}: a padding row or column 3 of dout is not zero"
    _run(mo.nsfp_checks(c, dict(dout=dout.numpy(), lp=f64_of(ob.lp).numpy())), name)


# ---- keep-best ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 257))
def test_keep_best_follows_the_restatement(lib, gpu, n):
    n_pad = int(lib.himo_nsf_padded_rows(n))
    for si, (losses, patience, min_delta) in enumerate(mo.KEEP_SCRIPTS):
        name = f"keep_best n {n} script {si}"
        state = gf64(gpu, list(mo.KEEP_INIT) + [-1.0, -2.0, -3.0, -4.0])
        best_out, out, loss = gwords(gpu, 4 * n_pad), gwords(gpu, 4 * n_pad), gf64(gpu, [0.0])
        want_best, st_ref = None, mo.KEEP_INIT
        for t, L in enumerate(losses, 1):
            values = torch.arange(4 * n_pad, dtype=torch.float32) * 0.5 + 1000.0 * t
            out.put(values)
            loss.put(torch.tensor([L], dtype=torch.float64).view(torch.int32))
            before, held = f64_of(state).clone(), best_out.buf.clone()
            call = Call([out, loss], [best_out, state])
            st = lib.himo_nsfp_keep_best(n, out.ptr, best_out.ptr, loss.ptr, state.ptr, t, patience, float(min_delta), _s())
            assert st == 0, f"{name} step {t}: status {st}"
            call.check(f"{name} step {t}")
            st_ref, improved = mo.keep_best_step(st_ref, float(L), t, patience, min_delta)
            after = f64_of(state)
            slot, other = (t & 1) * 4, ((t - 1) & 1) * 4
            assert after[slot:slot + 4].tolist() == list(st_ref), f"{name} step {t}: state {after[slot:slot + 4].tolist()}, restatement {st_ref}"
            assert torch.equal(after[other:other + 4], before[other:other + 4]), f"{name} step {t}: the slot that was read was written"
            if improved:
                want_best = values
                assert torch.equal(best_out.get(), want_best), f"{name} step {t}: best_out is not the improving step's out over all {n_pad} rows"
            else:
                assert torch.equal(best_out.buf, held), f"{name} step {t}: best_out was written without an improvement"
        assert want_best is not None
        _exact("keep_best", len(losses))


# ---- refusals and size queries -----------------------------------------------------------------------------------------------------
def test_mlp_refusals(lib, gpu):
    case = mo.mlp_case(63, 2, True)
    net = Net(lib, gpu, case)
    net.dout.put(case.dout[:net.R])
    outs = net.H + [net.out] + net.dZ + net.db + [net.ws]
    call = Call(net.params() + [net.x, net.dout], outs)
    for L in (0, 13):
        call.refused("forward", f"n_hidden {L}", net.forward(L=L), (INVALID,))
        call.refused("backward", f"n_hidden {L}", net.backward(L=L), (INVALID,))
        call.refused("backward_bias", f"n_hidden {L}", net.backward(bias=True, L=L), (INVALID,))
    hole = lambda bufs: PTRS(*[bufs[0].ptr, None])
    call.refused("forward", "a null H[1]", net.forward(H=hole(net.H)), (INVALID,))
    call.refused("backward", "a null H[1]", net.backward(H=hole(net.H)), (INVALID,))
    call.refused("backward", "a null dZ[1]", net.backward(dZ=hole(net.dZ)), (INVALID,))
    call.refused("backward_bias", "a null dZ[1]", net.backward(bias=True, dZ=hole(net.dZ)), (INVALID,))
    call.refused("backward_bias", "a null db[1]", net.backward(bias=True, db=hole(net.db)), (INVALID,))
    call.refused("backward_bias", "a null db table", net.backward(bias=True, db=None), (INVALID,))
    call.refused("forward", "a packed weight 8 bytes off", net.forward(wf=PTRS(None, net.pk_f[1].ptr + 8)), (INVALID,))
    call.refused("backward", "a packed weight 8 bytes off", net.backward(wb=PTRS(None, net.pk_b[1].ptr + 8)), (INVALID,))
    call.refused("forward", "a null packed weight", net.forward(wf=PTRS()), (INVALID,))
    call.refused("backward", "d_w_last 4 bytes off", net.backward(wl=net.wptr(net.L) + 4), (INVALID,))
    call.refused("backward_bias", "d_w_last 4 bytes off", net.backward(bias=True, wl=net.wptr(net.L) + 4), (INVALID,))
    call.refused("backward_bias", "the workspace one byte short", net.backward(bias=True, ws_bytes=net.ws_bytes - 1), (INVALID,))
    call.refused("backward_bias", "a null workspace", net.backward(bias=True, ws=None), (INVALID,))
    call.refused("forward", "n = 0 writes nothing", net.forward(n=0), (OK,))
    call.refused("backward", "n = 0 writes nothing", net.backward(n=0), (OK,))
    call.refused("backward_bias", "n = 0 writes nothing", net.backward(bias=True, n=0), (OK,))
    REFUSED[-3:] = []                                            # (admitted, not refused: kept out of the list)
    for what in ("x", "dout"):                                   # each 4 bytes off its 16-byte alignment
        m = Net(lib, gpu, case, **{what + "_off": 1})
        m.dout.put(case.dout[:m.R])
        c = Call(m.params() + [m.x, m.dout], m.H + [m.out] + m.dZ + m.db + [m.ws])
        if what == "x":
            c.refused("forward", "d_x0 misaligned", m.forward(), (INVALID,))
        else:
            c.refused("backward", "d_dout misaligned", m.backward(), (INVALID,))
            c.refused("backward_bias", "d_dout misaligned", m.backward(bias=True), (INVALID,))


def test_chamfer_and_nsfp_refusals(lib, gpu):
    c = mo.chamfer_case(257, 255)
    ch = Chamfer(lib, gpu, c)
    call = Call(ch.inputs, [ch.loss, ch.grad, ch.ws])
    call.refused("chamfer", "the workspace one byte short", ch(ws_bytes=ch.ws_bytes - 1), (WORKSPACE,))
    call.refused("chamfer", "a null d_loss", ch(loss=None), (INVALID,))
    call.refused("chamfer", "a null workspace", ch(ws=None), (INVALID,))
    call.refused("chamfer", "n0 < 0", ch(n0=-1), (INVALID,))
    call.refused("chamfer", "a null d_idx_b", ch(i_b=None), (INVALID,))
    n = mo.nsfp_case(65, 256)
    ob = Objective(lib, gpu, n)
    call = Call(ob.inputs, ob.outputs + [ob.ws])
    gx0, gy0, cell, gw, gh = _grid()
    call.refused("nsfp_prepare", "a short workspace", ob.prepare(ws_bytes=ob.ws_bytes - 1), (WORKSPACE,))
    call.refused("nsfp_prepare", "a grid above 2^20 cells", ob.prepare(grid=(gx0, gy0, cell, 1025, 1024)), (UNSUPPORTED,))
    call.refused("nsfp_prepare", "cell 0", ob.prepare(grid=(gx0, gy0, 0.0, gw, gh)), (INVALID,))
    call.refused("nsfp_objective", "a short workspace", ob(ws_bytes=ob.ws_bytes - 1), (WORKSPACE,))
    call.refused("nsfp_objective", "trunc < 0", ob(trunc=-0.5), (INVALID,))
    call.refused("nsfp_objective", "trunc NaN", ob(trunc=float("nan")), (INVALID,))
    call.refused("nsfp_objective", "a grid above 2^20 cells", ob(grid=(gx0, gy0, cell, 1025, 1024)), (UNSUPPORTED,))
    call.refused("nsfp_objective", "a null d_dout", ob(dout=None), (INVALID,))
    call.refused("nsfp_objective", "d_x0 4 bytes off", ob(x0=ob.x0.ptr + 4), (INVALID,))
    call.refused("nsfp_objective", "n0 = 0 writes nothing", ob(n0=0), (OK,))
    REFUSED.pop()
    n_pad = int(lib.himo_nsf_padded_rows(65))
    out, best, loss, state = gvals(gpu, torch.ones(4 * n_pad)), gwords(gpu, 4 * n_pad), gf64(gpu, [1.0]), gwords(gpu, 16)
    call = Call([out, loss], [best, state])
    kb = lambda **kw: lib.himo_nsfp_keep_best(kw.get("n", 65), kw.get("out", out.ptr), best.ptr, kw.get("loss", loss.ptr), state.ptr, kw.get("step", 1), 3, 0.0, _s())
    call.refused("keep_best", "step 0", kb(step=0), (INVALID,))
    call.refused("keep_best", "n < 0", kb(n=-1), (INVALID,))
    call.refused("keep_best", "a null d_loss", kb(loss=None), (INVALID,))
    call.refused("keep_best", "d_out 4 bytes off", kb(out=out.ptr + 4), (INVALID,))


def test_size_queries(lib, gpu):
    for n in (0, 1, 63, 64, 65, 4160, 120_000):
        for L in (-1, 0, 1, 8, 12):
            assert int(lib.himo_mlp_bias_workspace_bytes(n, L)) == max(L, 1) * ((n + 63) // 64) * 512 + 64
    up16 = lambda v: (v + 15) // 16 * 16
    for n0, n1 in ((0, 0), (1, 1), (255, 257), (256, 256), (257, 255), (300, 0), (0, 300), (120_000, 119_000)):
        assert int(lib.himo_chamfer_trunc_workspace_bytes(n0, n1)) == up16(((n0 + 255) // 256 + (n1 + 255) // 256 + 2) * 8) + max(n0, 1) * 24 + 64
        assert int(lib.himo_nsfp_partials(n0, n1)) == no.padded_rows(n0) // 64 + (n1 + 255) // 256
    gw, gh = _grid()[3:]
    for args in ((-1, 5, gw, gh), (5, -1, gw, gh), (5, 5, 0, gh), (5, 5, gw, -3)):
        assert int(lib.himo_nsfp_workspace_bytes(*args)) == 0
    assert int(lib.himo_nsfp_partials(-1, 5)) == 0 and int(lib.himo_nsfp_partials(5, -1)) == 0
    small, big = int(lib.himo_nsfp_workspace_bytes(1, 1, gw, gh)), int(lib.himo_nsfp_workspace_bytes(257, 1, gw, gh))
    assert small > 0 and big - small >= 256 * 24                 # (the fixed-point sums: 24 bytes per moved row, after the search's share)
    _exact("size queries", 4)
