"""Conformance of the per-pair fit kernels over what their entry points admit: himo_nsf_forward, himo_nsf_forward_keep,
himo_nsf_last_grad, himo_nsf_backward, himo_nsf_update and their size queries (csrc/nsffused.hip), himo_dt_build, himo_dt_loss
and their size queries (csrc/dtloss.hip, csrc/dtlookup.h), himo_adam_step (whose arithmetic himo_nsf_update restates) and
himo_mlp_repack as the packer that feeds the others.  The entry points are called through ctypes, not through the FastNSF / NSFP
engines (tests/test_fastnsf_gpu.py, tests/test_nsfp_gpu.py do that).

For every call the library must either refuse it (the documented status, no output byte written) or return results within the
bounds of oracle/nsf_oracle.py against float64 and within conv_oracle.R of the float32 twin -- the uint16 distance-transform
volume EQUAL to the brute-force one -- with the inputs bit-unchanged and no word outside an output view or a workspace written.
Operands, outputs and workspaces live in NaN-filled guarded buffers (oracle/guarded.py) sized by the library's own queries.
tests/test_nsf_oracle.py shows on the CPU that these checks pass the float32 twin and fail the wrong ones, and that every point
of every case keeps each discrete decision (ReLU mask, base cell, in-volume, D <= trunc) at least twice its asserted bound from
its threshold, so that a float64 comparison means something.  The spill's fragment layout is not decoded: it is checked through
the backward pass.

himo_nsf_update alone: the issue's "random partials and m = 0" is read as Adam moments m = v = 0 with a NON-zero point count (a
zero count makes every gradient exactly zero and would hide the four-run split); the zero count is one more case.

The layer-kernel path -- csrc/mlpfused.hip, himo_chamfer_trunc and csrc/nsfp.hip's objective and keep-best rule -- is pinned in
tests/test_mlpfused_conformance_gpu.py (oracle/mlpfused_oracle.py); himo_nn_grid in tests/test_sslloss_conformance_gpu.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_oracle as co
import grad_oracle as go
import nsf_oracle as no
from guarded import NAN_BITS, Guarded, layout

pytestmark = pytest.mark.gpu

STATS = {}        # (family, arith) -> [worst err / bound, worst rms ratio, checks, case of the first, case of the second]
REFUSED = []      # (family, case, status)
INVALID, WORKSPACE = 1, 3
PK_BYTES = 8 * 2 * 128 * 16 * 2          # the two planes himo_mlp_repack writes for a 128 x 128 layer


@pytest.fixture(scope="module", autouse=True)
def _summary():
    from himo_amd import _lib
    _lib.prof_start()
    yield
    met = _lib.prof_stop()
    print("\nnsf conformance: per family and arithmetic, the largest err/bound and rms ratio over the matrix")
    for (fam, a), (w, r, n, wc, rc) in sorted(STATS.items()):
        lim = "-" if a == "exact" else f"{go.R_ELEM if fam in ('adam', 'dt_loss') else co.R[a]:g}"
        print(f"  {fam:12s} {a:7s} err/bound {w:.3g}  rms ratio {r:.3g} (R {lim})  {n} checks\n    worst err/bound: {wc}\n    worst rms: {rc}")
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
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def _run(checks, case):
    for fam, name, arith, got, ref, bnd, r32, cols in checks:
        got = torch.as_tensor(got)
        assert not bool(torch.isnan(got).any()), f"{case} {fam}/{name}: NaN in the result (a read of a guard or of a word never written)"
        limit = go.R_ELEM if fam in ("adam", "dt_loss") else None
        good, worst, rr, report = no.verdict(arith, got, ref, bnd, r32, f"{case} {fam}/{name}", limit=limit, cols=cols)
        print(report)
        assert good, report
        s = STATS.setdefault((fam, arith), [0.0, 0.0, 0, "", ""])
        if worst >= s[0]:
            s[0], s[3] = worst, f"{case} {name}"
        if rr >= s[1]:
            s[1], s[4] = rr, f"{case} {name}"
        s[2] += 1


# ---- guarded buffers -----------------------------------------------------------------------------------------------------
def gwords(gpu, words, off=0):
    """``words`` 32-bit words, ``off`` words past the aligned base"""
    return Guarded(torch.arange(int(words), dtype=torch.int64), gpu, off=off)


def gbytes(gpu, nbytes, off=0):
    assert nbytes % 4 == 0
    return gwords(gpu, nbytes // 4, off)


def gvals(gpu, values, off=0):
    g = gwords(gpu, values.numel(), off)
    g.put(values.reshape(-1) if values.dtype == torch.int32 else values.reshape(-1).float())
    return g


def gf64(gpu, values):
    return gvals(gpu, torch.as_tensor(values, dtype=torch.float64).reshape(-1).view(torch.int32))


def f64_of(g):
    return g.words().reshape(-1).view(torch.float64)


def bytes_of(g):
    return g.words().reshape(-1).view(torch.uint8)


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
            assert g.untouched(), f"{case}: refused (status {st}) but wrote"
        REFUSED.append((fam, case, st))


# ---- the distance transform ---------------------------------------------------------------------------------------------
def _grid_args(gr):
    return (ctypes.c_float * 3)(*gr.origin.tolist()), (ctypes.c_int * 3)(*gr.dims)


class Volume:
    def __init__(self, lib, gpu, gr, fill=False):
        self.gr = gr
        self.o_c, self.d_c = _grid_args(gr)
        self.bytes = int(lib.himo_dt_volume_bytes(self.d_c))
        cells = gr.dims[0] * gr.dims[1] * gr.dims[2]
        assert self.bytes == 2 * (-(-cells * 2 // 256) * 256)
        self.g = gbytes(gpu, self.bytes)
        self.cells = cells
        if fill:                                             # the brute-force volume itself, for the kernels that only read one
            w = np.zeros(-(-cells // 2) * 2, np.uint16)
            w[:cells] = gr.G.reshape(-1)
            self.g.buf[self.g.base: self.g.base + len(w) // 2] = torch.from_numpy(w.view(np.int32)).to(gpu)

    def G(self):
        return bytes_of(self.g).numpy().view(np.uint16)[: self.cells].reshape(self.gr.dims[::-1])


def _build(lib, gpu, gr, case):
    vol = Volume(lib, gpu, gr)
    t = gvals(gpu, torch.from_numpy(gr.targets)) if len(gr.targets) else None
    call = Call([t] if t is not None else [], [vol.g])
    st = lib.himo_dt_build(len(gr.targets), t.ptr if t is not None else None, vol.o_c, float(gr.cell), vol.d_c, gr.window, vol.g.ptr, vol.bytes, _s())
    assert st == 0, f"{case}: status {st}"
    call.check(case)
    return vol


@pytest.mark.parametrize("i", range(len(no.DT_CASES)))
def test_dt_build_equals_the_brute_force_volume(lib, gpu, i):
    gr = no.dt_case(i)
    case = f"dt_build {gr.dims} window {gr.window} cell {float(gr.cell):g} {gr.kind}"
    got = _build(lib, gpu, gr, case).G()
    bad = got != gr.G
    assert not bad.any(), f"{case}: {int(bad.sum())} cells differ, first at (z, y, x) {tuple(np.argwhere(bad)[0])}: got {got[bad][0]} ref {gr.G[bad][0]}"
    s = STATS.setdefault(("dt_build", "exact"), [0.0, 0.0, 0, "bit-equal", "-"])
    s[2] += 1


def _dt_loss(lib, gpu, vol, pts, case, exact_u=False):
    gr, n = vol.gr, len(pts)
    moved = gvals(gpu, pts) if n else gwords(gpu, 0)
    grad, loss = gwords(gpu, 3 * n), gwords(gpu, 2)
    ws_bytes = int(lib.himo_dt_loss_workspace_bytes(n))
    ws = gbytes(gpu, ws_bytes)
    call = Call([moved, vol.g], [grad, loss, ws])
    st = lib.himo_dt_loss(n, moved.ptr if n else None, vol.o_c, float(gr.cell), vol.d_c, gr.window, vol.g.ptr, float(gr.trunc), loss.ptr,
                          grad.ptr if n else None, ws.ptr, ws_bytes, _s())
    assert st == 0, f"{case}: status {st}"
    call.check(case)
    got = dict(loss=float(f64_of(loss)[0]), grad=grad.get().reshape(n, 3))
    _run(no.dt_loss_checks(gr, pts, got, exact_u), case)
    return got


@pytest.mark.parametrize("i,n,nan", no.DT_LOSS_CASES)
def test_dt_loss(lib, gpu, i, n, nan):
    gr = no.dt_case(i)
    case = f"dt_loss {gr.dims} n {n}{' with NaN' if nan else ''}"
    vol = _build(lib, gpu, gr, case)
    pts, _ = no.dt_points(gr, n, nan=nan)
    got = _dt_loss(lib, gpu, vol, pts, case)
    if gr.dims[2] == 1 or n == 0:                             # nobody in the volume: m = 0, loss 0, every gradient exactly 0
        assert got["loss"] == 0.0 and not got["grad"].any()


def test_dt_loss_decides_at_the_thresholds(lib, gpu):
    """u exactly 0 and n - 1 are outside; an integer u inside has f = 0; D == trunc is counted and has a gradient"""
    gr = no.threshold_grid()
    vol = _build(lib, gpu, gr, "dt thresholds")
    assert np.array_equal(vol.G(), gr.G)
    pts = torch.tensor(list(no.threshold_points().values()))
    got = _dt_loss(lib, gpu, vol, pts, "dt thresholds", exact_u=True)
    ref = no.dt_objective(pts, gr)
    assert ref["m"] == 3 and got["loss"] * 3 == pytest.approx(ref["dsum"], rel=1e-6)
    names = list(no.threshold_points())
    assert not got["grad"][names.index("u_zero")].any() and not got["grad"][names.index("u_last")].any()
    assert got["grad"][names.index("d_is_trunc")].any()


def test_dt_refusals(lib, gpu):
    gr = no.dt_case(4)
    vol = Volume(lib, gpu, gr)
    t = gvals(gpu, torch.from_numpy(gr.targets))
    n1 = len(gr.targets)
    call = Call([t], [vol.g])

    def build(case, allowed, window=gr.window, cell=float(gr.cell), dims=gr.dims, ptr=vol.g.ptr, nbytes=vol.bytes):
        st = lib.himo_dt_build(n1, t.ptr, vol.o_c, cell, (ctypes.c_int * 3)(*dims), window, ptr, nbytes, _s())
        call.refused("dt_build", case, st, allowed)
    build("window 0", (INVALID,), window=0)
    build("window 41", (INVALID,), window=41)
    build("cell 0", (INVALID,), cell=0.0)
    build("cell < 0", (INVALID,), cell=-0.1)
    build("a zero dimension", (INVALID,), dims=(257, 0, 2))
    build("more than 2^31 cells", (INVALID,), dims=(2048, 2048, 513))
    build("a short volume", (WORKSPACE,), nbytes=vol.bytes - 1)
    build("a misaligned volume", (WORKSPACE,), ptr=vol.g.ptr + 4)
    pts, _ = no.dt_points(gr, 257)
    moved, grad, loss = gvals(gpu, pts), gwords(gpu, 3 * 257), gwords(gpu, 2)
    need = int(lib.himo_dt_loss_workspace_bytes(257))
    ws = gbytes(gpu, need)
    call = Call([moved], [grad, loss, ws, vol.g])
    for case, allowed, kw in (("a short workspace", (WORKSPACE,), dict(nbytes=need - 1)), ("window 0", (INVALID,), dict(window=0)),
                              ("window 41", (INVALID,), dict(window=41)), ("cell 0", (INVALID,), dict(cell=0.0))):
        st = lib.himo_dt_loss(257, moved.ptr, vol.o_c, kw.get("cell", float(gr.cell)), vol.d_c, kw.get("window", gr.window), vol.g.ptr,
                              float(gr.trunc), loss.ptr, grad.ptr, ws.ptr, kw.get("nbytes", need), _s())
        call.refused("dt_loss", case, st, allowed)


# ---- the network on the device ------------------------------------------------------------------------------------------
PTRS = ctypes.c_void_p * (no.MAX_HIDDEN + 2)


class Net:
    """a case's operands in guarded buffers sized by the library's queries: the flat parameter vector (layer i's W at off_w[i], b
    at off_b[i]), the packed copies of the hidden layers (himo_mlp_repack), x, out, dout, the spill, the partials"""

    def __init__(self, lib, gpu, case, x_off=0, out_off=0, dout_off=0, spill_off=0):
        self.lib, self.gpu, self.case = lib, gpu, case
        L, n = case.n_hidden, case.n
        self.L, self.n = L, n
        flat, self.off_w, self.off_b = no.flat(case.params)
        self.total = flat.numel()
        self.stride = (self.total + 63) // 64 * 64
        self.P = gvals(gpu, flat)
        self.pk_size = int(lib.himo_conv_packed_weight_bytes(1, 128, 128))
        assert self.pk_size >= PK_BYTES
        self.pk_f = [None] + [gbytes(gpu, self.pk_size) for _ in range(1, L)]
        self.pk_b = [None] + [gbytes(gpu, self.pk_size) for _ in range(1, L)]
        self.repack(self.P, self.pk_f, self.pk_b)
        self.n_pad = int(lib.himo_nsf_padded_rows(n))
        assert self.n_pad == no.padded_rows(n) == len(case.x)
        self.tiles, self.blocks = self.n_pad // 64, int(lib.himo_nsf_backward_blocks(n))
        assert self.blocks == self.tiles // 4
        self.x = gvals(gpu, case.x, off=x_off)
        self.out, self.dout = gwords(gpu, self.n_pad * 4, off=out_off), gwords(gpu, self.n_pad * 4, off=dout_off)
        self.spill_bytes = int(lib.himo_nsf_spill_bytes(n, L))
        assert self.spill_bytes == L * self.tiles * (32768 + 1024) + self.tiles * no.LAST_STRIDE * 4 + 256
        self.spill = gbytes(gpu, self.spill_bytes, off=spill_off)
        self.lp, self.cp = gwords(gpu, 2 * self.tiles), gwords(gpu, self.tiles)
        self.partial = Guarded(layout(1, 1, 0, 0, self.blocks, self.stride, self.total), gpu)
        self.vol = Volume(lib, gpu, case.grid, fill=True) if case.grid is not None else None
        self.I = (ctypes.c_int * (L + 1))

    def wptr(self, i):
        return self.P.ptr + 4 * self.off_w[i]

    def bptr(self, i):
        return self.P.ptr + 4 * self.off_b[i]

    def table(self, bufs):
        return PTRS(*([None] + [bufs[k].ptr for k in range(1, self.L)]))

    def biases(self):
        return PTRS(*([None] + [self.bptr(k) for k in range(1, self.L)]))

    def repack(self, P, pk_f, pk_b):
        """himo_mlp_repack of the hidden layers of the flat vector P into pk_f / pk_b"""
        k = self.L - 1
        if k == 0:
            return
        A, I = ctypes.c_void_p * k, ctypes.c_int * k
        st = self.lib.himo_mlp_repack(k, A(*[P.ptr + 4 * self.off_w[i] for i in range(1, self.L)]), I(*[128] * k), I(*[128] * k),
                                      A(*[pk_f[i].ptr for i in range(1, self.L)]), A(*[pk_b[i].ptr for i in range(1, self.L)]), _s())
        assert st == 0, st
        torch.cuda.synchronize()

    def inputs(self):
        return [self.P, self.x] + self.pk_f[1:] + self.pk_b[1:] + ([self.vol.g] if self.vol else [])

    def forward(self, objective=True, keep=False, **over):
        a = dict(n=self.n, x=self.x.ptr, L=self.L, w0=self.wptr(0), b0=self.bptr(0), wf=self.table(self.pk_f), bias=self.biases(),
                 wl=self.wptr(self.L), bl=self.bptr(self.L), spill=self.spill.ptr, out=self.out.ptr)
        a.update({k: v for k, v in over.items() if k in a})
        if keep:
            return self.lib.himo_nsf_forward_keep(*a.values(), _s())
        v = self.vol
        b = dict(o=v.o_c, cell=float(v.gr.cell), d=v.d_c, window=v.gr.window, vol=v.g.ptr, trunc=float(v.gr.trunc),
                 dout=self.dout.ptr if objective else None, lp=self.lp.ptr, cp=self.cp.ptr)
        b.update({k: v_ for k, v_ in over.items() if k in b})
        return self.lib.himo_nsf_forward(*a.values(), *b.values(), _s())

    def backward(self, **over):
        a = dict(n=self.n, x=self.x.ptr, dout=self.dout.ptr, L=self.L, wb=self.table(self.pk_b), wl=self.wptr(self.L), spill=self.spill.ptr,
                 off_w=self.I(*self.off_w), off_b=self.I(*self.off_b), stride=self.stride, partial=self.partial.ptr)
        a.update(over)
        return self.lib.himo_nsf_backward(*a.values(), _s())

    def last_offset(self):
        return self.L * self.tiles * (32768 + 1024)

    def last_partials(self):
        """the forward's per-tile last-layer gradients, summed over the tiles in float64 -> dW_last [128, 4], db_last [4]"""
        b = bytes_of(self.spill)[self.last_offset(): self.last_offset() + self.tiles * no.LAST_STRIDE * 4].view(torch.float32)
        t = b.reshape(self.tiles, no.LAST_STRIDE).double().sum(0)
        return t[:512].reshape(128, 4), t[512:516]

    def h_last(self):
        """himo_nsf_forward_keep's H_{L-1}: float32 [64][128] per tile in layer L - 1's slot of the spill"""
        o = (self.L - 1) * self.tiles * 32768
        return bytes_of(self.spill)[o: o + self.tiles * 32768].view(torch.float32).reshape(self.n_pad, 128)

    def grads(self):
        """the block partials summed in float64 -> [(dW, db)] in the parameter shapes"""
        t = self.partial.get().reshape(self.blocks, self.total).double().sum(0)
        return [(t[self.off_w[i]: self.off_b[i]].reshape(w.shape), t[self.off_b[i]: self.off_b[i] + b.numel()])
                for i, (w, b) in enumerate(self.case.params)]


def _objective_results(net):
    out = net.out.get().reshape(-1, 4)
    pad = out[net.n:]
    assert bool(torch.isfinite(out).all()) and (len(pad) == 0 or bool((pad == pad[0]).all())), "padding rows of out differ from each other"
    return dict(out=out, dout=net.dout.get().reshape(-1, 4), dsum=float(f64_of(net.lp).sum()), m=int(net.cp.words().sum()))


def _forward_objective(lib, gpu, case, name):
    net = Net(lib, gpu, case)
    call = Call(net.inputs(), [net.out, net.dout, net.spill, net.lp, net.cp])
    st = net.forward()
    assert st == 0, f"{name}: status {st}"
    call.check(name)
    got = _objective_results(net)
    got["grads"] = [(None, None)] * case.n_hidden + [net.last_partials()]
    _run(no.iteration_checks(case, got), name)
    return net


@pytest.mark.parametrize("n,n_hidden,dead", no.FWD_CASES)
def test_forward_with_the_objective(lib, gpu, n, n_hidden, dead):
    _forward_objective(lib, gpu, no.mlp_case(n, n_hidden, dead), f"forward n {n} hidden {n_hidden}{' dead' if dead else ''}")


def test_forward_decides_the_lookup_at_the_thresholds(lib, gpu):
    """the fused forward's own in-volume / D <= trunc / count lines: a zero last layer makes moved = x exactly"""
    case = no.threshold_network_case()
    net = _forward_objective(lib, gpu, case, "forward thresholds")
    got, names = _objective_results(net), list(no.threshold_points())
    assert got["m"] == 3 and not got["out"].any()
    d = got["dout"]
    assert not d[names.index("u_zero")].any() and not d[names.index("u_last")].any() and d[names.index("d_is_trunc")].any()


def _external_dout(case, seed=0):
    g = torch.Generator().manual_seed(seed + case.n)
    d = torch.randn(len(case.x), 4, generator=g) * 10.0 ** (-3 * torch.rand(4, generator=g))
    d[case.n:] = 0.0
    return d


@pytest.mark.parametrize("n,n_hidden,dead", no.FWD_CASES)
def test_forward_keep_and_last_grad(lib, gpu, n, n_hidden, dead):
    case = no.mlp_case(n, n_hidden, dead)
    name = f"forward_keep n {n} hidden {n_hidden}{' dead' if dead else ''}"
    net = Net(lib, gpu, case)
    call = Call(net.inputs(), [net.out, net.spill])
    st = net.forward(keep=True)
    assert st == 0, f"{name}: status {st}"
    call.check(name)
    assert net.dout.untouched() and net.lp.untouched() and net.cp.untouched()
    _run(no.iteration_checks(case, dict(out=net.out.get().reshape(-1, 4), h_last=net.h_last())), name)
    dout = _external_dout(case)
    net.dout.put(dout)
    call = Call(net.inputs() + [net.dout], [net.spill])
    st = lib.himo_nsf_last_grad(n, n_hidden, net.dout.ptr, net.spill.ptr, _s())
    assert st == 0, f"{name}: last_grad status {st}"
    call.check(name)
    _run(no.last_grad_checks(case, dout, *net.last_partials()), name.replace("forward_keep", "last_grad"))


# ---- the full iteration -----------------------------------------------------------------------------------------------------
def _update(lib, gpu, net, step, state, name, n_partials=None, partial=None, lp=None, cp=None, tiles=None):
    """himo_nsf_update on net's partials (or the given ones) -> dict g, p, m, v, loss, count and the packed copies it wrote"""
    L = net.L
    p0, m0, v0 = state
    P, M, V, Gd = gvals(gpu, p0), gvals(gpu, m0), gvals(gpu, v0), gwords(gpu, net.total)
    pk_f = [None] + [gbytes(gpu, net.pk_size) for _ in range(1, L)]
    pk_b = [None] + [gbytes(gpu, net.pk_size) for _ in range(1, L)]
    loss, count = gwords(gpu, 2), gwords(gpu, 1)
    partial = net.partial if partial is None else partial
    lp, cp = (net.lp if lp is None else lp), (net.cp if cp is None else cp)
    call = Call([partial, lp, cp], [P, M, V, Gd, loss, count] + pk_f[1:] + pk_b[1:])
    A = no.ADAM
    st = lib.himo_nsf_update(net.total, net.blocks if n_partials is None else n_partials, net.stride, partial.ptr, net.tiles if tiles is None else tiles,
                             lp.ptr, cp.ptr, P.ptr, Gd.ptr, M.ptr, V.ptr, float(A["lr"]), float(A["b1"]), float(A["b2"]), float(A["eps"]), step, L,
                             net.I(*net.off_w), PTRS(*([None] + [b.ptr for b in pk_f[1:]])), PTRS(*([None] + [b.ptr for b in pk_b[1:]])),
                             loss.ptr, count.ptr, _s())
    assert st == 0, f"{name}: update status {st}"
    call.check(name)
    got = dict(g=Gd.get(), p=P.get(), m=M.get(), v=V.get(), loss=float(f64_of(loss)[0]), count=int(count.words()[0]))
    # Adam against float64 on the kernel's OWN gradient, and himo_adam_step on the same data: the same bits
    ref, bnd = no.adam(p0, got["g"], m0, v0, step), no.adam_bound(p0, got["g"], m0, v0, step)
    r32 = no.adam(p0, got["g"], m0, v0, step, torch.float32)
    _run([("adam", k, "f32", got[k], r, bnd[k], t, False) for k, r, t in zip(("p", "m", "v"), ref, r32)], name)
    P2, M2, V2 = gvals(gpu, p0), gvals(gpu, m0), gvals(gpu, v0)
    call = Call([Gd], [P2, M2, V2])
    st = lib.himo_adam_step(net.total, P2.ptr, Gd.ptr, M2.ptr, V2.ptr, float(A["lr"]), float(A["b1"]), float(A["b2"]), float(A["eps"]), step, _s())
    assert st == 0, st
    call.check(name + " adam_step")
    for a, b, k in ((P, P2, "p"), (M, M2, "m"), (V, V2, "v")):
        assert torch.equal(a.words(), b.words()), f"{name}: himo_adam_step's {k} differs from the update kernel's"
    # the packed copies: byte-identical to himo_mlp_repack of the updated parameters into fresh buffers
    fr_f = [None] + [gbytes(gpu, net.pk_size) for _ in range(1, L)]
    fr_b = [None] + [gbytes(gpu, net.pk_size) for _ in range(1, L)]
    net.repack(P, fr_f, fr_b)
    for k in range(1, L):
        for mine, fresh, what in ((pk_f[k], fr_f[k], "forward"), (pk_b[k], fr_b[k], "backward")):
            assert fresh.untouched_outside()
            a, b = bytes_of(mine), bytes_of(fresh)
            assert torch.equal(a, b), f"{name}: the {what} copy of layer {k} differs from himo_mlp_repack's at byte {int(torch.nonzero(a != b)[0])}"
            assert not bool((a[:PK_BYTES].view(torch.int32) == NAN_BITS).any()), f"{name}: the {what} copy of layer {k} was not written whole"
    return got


def _state(total, step, seed=0):
    g = torch.Generator().manual_seed(seed)
    if step == 1:
        return torch.zeros(total), torch.zeros(total)
    return torch.randn(total, generator=g) * 1e-3, torch.rand(total, generator=g) * 1e-5


def _iteration(lib, gpu, case, name, step):
    net = _forward_objective(lib, gpu, case, name)
    call = Call(net.inputs() + [net.dout, net.spill], [net.partial])
    st = net.backward()
    assert st == 0, f"{name}: backward status {st}"
    call.check(name)
    grads = net.grads()
    _run(no.iteration_checks(case, dict(grads=grads)), name)
    m0, v0 = _state(net.total, step, case.n)
    p0 = no.flat(case.params)[0]
    got = _update(lib, gpu, net, step, (p0, m0, v0), name)
    ref = case.ref
    m = ref["m"]
    assert got["count"] == m, f"{name}: count {got['count']}, reference {m}"
    inv = 1.0 / m if m else 0.0
    _run([("objective", "loss", "f16x2", torch.tensor([got["loss"]]), torch.tensor([ref["dsum"] * inv]), torch.tensor([case.e_dsum * inv + no.TINY]), None, False)], name)
    # g = (the float32 sum of the block partials) x float32(1 / m): blocks + 1 roundings on the partials' magnitudes, two on 1 / m and
    # the product
    mag = net.partial.get().reshape(net.blocks, net.total).double().abs().sum(0) * inv
    e_sum = no.gamma(net.blocks + 3) * mag
    for i, ((rw, rb), (ew, eb), (tw, tb)) in enumerate(zip(ref["grads"], case.e_grads, case.ref32["grads"])):
        w = slice(net.off_w[i], net.off_b[i])
        b = slice(net.off_b[i], net.off_b[i] + rb.numel())
        arith = "f16x2" if i == net.L else "bf16x2"
        _run([("update", f"g W{i}", arith, got["g"][w].reshape(rw.shape), rw * inv, ew * inv + e_sum[w].reshape(rw.shape), tw.double() * inv, True),
              ("update", f"g b{i}", arith, got["g"][b], rb * inv, eb * inv + e_sum[b], tb.double() * inv, False)], name)


@pytest.mark.parametrize("n,n_hidden,dead", no.BWD_CASES)
def test_full_iteration(lib, gpu, n, n_hidden, dead):
    step = 1 if (n % 2) else 1000
    _iteration(lib, gpu, no.mlp_case(n, n_hidden, dead), f"iteration n {n} hidden {n_hidden}{' dead' if dead else ''} step {step}", step)


def test_iteration_with_a_pre_activation_of_exactly_zero(lib, gpu):
    """a point at the origin and first-layer biases of exactly 0: z = 0, the mask bit is clear, no gradient passes"""
    case = no.mask_threshold_case()
    _iteration(lib, gpu, case, "iteration mask threshold step 1", 1)


_EXT = {}


@pytest.mark.parametrize("n,n_hidden,dead", no.BWD_CASES)
def test_backward_of_an_external_dout(lib, gpu, n, n_hidden, dead):
    """himo_nsf_forward_keep + himo_nsf_last_grad + himo_nsf_backward (the NSFP path) with a random dout whose padding rows are zero"""
    import copy
    base = no.mlp_case(n, n_hidden, dead)
    case = copy.copy(base)
    dout = _external_dout(base, seed=7)
    no.finish_case(case, dout)
    name = f"external dout n {n} hidden {n_hidden}{' dead' if dead else ''}"
    net = Net(lib, gpu, case)
    assert net.forward(keep=True) == 0
    net.dout.put(dout)
    assert lib.himo_nsf_last_grad(n, n_hidden, net.dout.ptr, net.spill.ptr, _s()) == 0
    call = Call(net.inputs() + [net.dout, net.spill], [net.partial])
    st = net.backward()
    assert st == 0, f"{name}: backward status {st}"
    call.check(name)
    _run(no.iteration_checks(case, dict(out=net.out.get().reshape(-1, 4), grads=net.grads())), name)


@pytest.mark.parametrize("n_partials", (1, 2, 3, 4, 5, 9, 33))
def test_update_alone(lib, gpu, n_partials):
    """the four-run split of the partial list and its eight-chain tail: random partials, Adam moments zero, seven points counted"""
    case = no.mlp_case(1, 2)
    net = Net(lib, gpu, case)
    g = torch.Generator().manual_seed(n_partials)
    part = torch.randn(n_partials, net.total, generator=g) * 10.0 ** (-4 * torch.rand(net.total, generator=g))
    partial = Guarded(layout(1, 1, 0, 0, n_partials, net.stride, net.total), gpu)
    partial.put(part)
    tiles = 5
    counts = torch.tensor([3, 0, 4, 0, 0], dtype=torch.int32)
    lp, cp = gf64(gpu, [0.5, 0.0, 1.25, 0.0, 0.0]), gvals(gpu, counts)
    p0 = no.flat(case.params)[0]
    name = f"update alone, {n_partials} partials"
    got = _update(lib, gpu, net, 1, (p0, torch.zeros(net.total), torch.zeros(net.total)), name, n_partials, partial, lp, cp, tiles)
    assert got["count"] == 7 and got["loss"] == 1.75 / 7
    ref = part.double().sum(0) / 7
    bnd = no.gamma(n_partials + 3) * part.double().abs().sum(0) / 7 + no.TINY
    r32 = torch.from_numpy(np.add.accumulate(part.numpy(), axis=0)[-1].copy()) * (torch.tensor(1.0) / torch.tensor(7.0))
    _run([("update", "g", "f32", got["g"], ref, bnd, r32, False)], name)
    if n_partials == 5:                                       # nobody counted: every gradient exactly zero, loss 0
        cp0 = gvals(gpu, torch.zeros(5, dtype=torch.int32))
        got = _update(lib, gpu, net, 1, (p0, torch.zeros(net.total), torch.zeros(net.total)), name + ", count 0", n_partials, partial, lp, cp0, tiles)
        assert got["count"] == 0 and got["loss"] == 0.0 and not got["g"].any() and torch.equal(got["p"], p0)


# ---- refusals and size queries -----------------------------------------------------------------------------------------------
def test_size_queries(lib, gpu):
    for n in (-1, 0, 1, 64, 65, 256, 257, 1024, 1025, 120_000):
        assert int(lib.himo_nsf_padded_rows(n)) == no.padded_rows(n)
        assert int(lib.himo_nsf_backward_blocks(n)) == no.padded_rows(n) // 256
        for L in (1, 8, 12):
            t = no.padded_rows(max(n, 0)) // 64
            assert int(lib.himo_nsf_spill_bytes(n, L)) == (0 if n < 0 else L * t * (32768 + 1024) + t * no.LAST_STRIDE * 4 + 256)
    assert int(lib.himo_nsf_spill_bytes(64, 0)) == 0
    for n in (0, 1, 256, 257):
        assert int(lib.himo_dt_loss_workspace_bytes(n)) == ((n + 255) // 256 + 2) * 12 + 64


def test_nsf_refusals(lib, gpu):
    case = no.mlp_case(63, 2, True)
    outs = lambda net: [net.out, net.dout, net.spill, net.lp, net.cp, net.partial]
    net = Net(lib, gpu, case)
    call = Call(net.inputs(), outs(net))
    for L in (0, 13):
        call.refused("forward", f"n_hidden {L}", net.forward(L=L), (INVALID,))
        call.refused("forward_keep", f"n_hidden {L}", net.forward(keep=True, L=L), (INVALID,))
        call.refused("last_grad", f"n_hidden {L}", lib.himo_nsf_last_grad(case.n, L, net.dout.ptr, net.spill.ptr, _s()), (INVALID,))
    for L in (0, 1, 13):
        call.refused("backward", f"n_hidden {L}", net.backward(L=L), (INVALID,))
    call.refused("forward", "a missing hidden weight pointer", net.forward(wf=PTRS()), (INVALID,))
    call.refused("backward", "a missing hidden weight pointer", net.backward(wb=PTRS()), (INVALID,))
    bad = list(net.off_w)
    bad[net.L] = net.stride - 100
    call.refused("backward", "an offset table that overruns partial_stride", net.backward(off_w=net.I(*bad)), (INVALID,))
    call.refused("backward", "partial_stride below the last layer's end", net.backward(stride=net.off_w[net.L] + 100), (INVALID,))
    call.refused("forward", "n = 0 writes nothing", net.forward(n=0), (0,))
    call.refused("forward_keep", "n = 0 writes nothing", net.forward(keep=True, n=0), (0,))
    call.refused("backward", "n = 0 writes nothing", net.backward(n=0), (0,))
    call.refused("last_grad", "n = 0 writes nothing", lib.himo_nsf_last_grad(0, net.L, net.dout.ptr, net.spill.ptr, _s()), (0,))
    for what in ("x", "out", "dout", "spill"):               # each operand 4 bytes off its 16-byte alignment
        m = Net(lib, gpu, case, **{what + "_off": 1})
        c = Call(m.inputs(), outs(m))
        c.refused("forward", f"{what} misaligned", m.forward(), (INVALID,))
        if what != "dout":
            c.refused("forward_keep", f"{what} misaligned", m.forward(keep=True), (INVALID,))
        if what in ("dout", "spill"):
            c.refused("last_grad", f"{what} misaligned", lib.himo_nsf_last_grad(case.n, m.L, m.dout.ptr, m.spill.ptr, _s()), (INVALID,))
        if what != "out":
            c.refused("backward", f"{what} misaligned", m.backward(), (INVALID,))
    # himo_nsf_update
    p0 = no.flat(case.params)[0]
    P, M, V, Gd, loss, count = gvals(gpu, p0), gwords(gpu, net.total), gwords(gpu, net.total), gwords(gpu, net.total), gwords(gpu, 2), gwords(gpu, 1)
    before = [g.buf.clone() for g in (P, net.pk_f[1], net.pk_b[1])]
    A = no.ADAM

    def update(step=1, stride=net.stride, L=net.L):
        return lib.himo_nsf_update(net.total, net.blocks, stride, net.partial.ptr, net.tiles, net.lp.ptr, net.cp.ptr, P.ptr, Gd.ptr, M.ptr, V.ptr,
                                   float(A["lr"]), float(A["b1"]), float(A["b2"]), float(A["eps"]), step, L, net.I(*net.off_w),
                                   net.table(net.pk_f), net.table(net.pk_b), loss.ptr, count.ptr, _s())
    for case_name, st in (("step 0", update(step=0)), ("partial_stride < total", update(stride=net.total - 1)), ("n_hidden 0", update(L=0)),
                          ("n_hidden 13", update(L=13))):
        torch.cuda.synchronize()
        assert st == INVALID, f"update {case_name}: status {st}"
        assert all(torch.equal(g.buf, b) for g, b in zip((P, net.pk_f[1], net.pk_b[1]), before)), f"update {case_name}: refused but wrote"
        assert all(g.untouched() for g in (M, V, Gd, loss, count))
        REFUSED.append(("update", case_name, st))
