"""Conformance of the gradient kernels over the descriptors their entry points admit, not only the shapes the trainer feeds
them: himo_conv3x3_wgrad_batch(_bias), himo_conv3x3_wgrad, himo_linear_wgrad(_ex), himo_colsum, himo_zero_stuff2x,
himo_upsample2x_bwd, himo_weight_flip, himo_transpose and the element-wise kernels of the training step.  (The data-gradient
forms of himo_conv2d sit in tests/test_conv_conformance_gpu.py, through its own conv_case.)

For every descriptor the library must either refuse it (a documented status, no output byte written) or return a result
within the worst-case bound of oracle/grad_oracle.py against float64 and within its aggregate ratio R of the float32 twin,
with the inputs bit-unchanged and no byte outside the output view written.  Operands, outputs and workspaces all live in
NaN-filled guarded buffers (oracle/guarded.py): a read outside an input view poisons the result.  Workspaces have exactly
the size the library's own query returns.

The case strings name the kernel the host code dispatches to (mirrored from csrc/fastnsf.hip:757-823 and
csrc/train.hip:948-976); the module summary lists which were met.
"""
import pytest
import torch

import conv_oracle as co
import grad_oracle as go
from guarded import Guarded, layout

pytestmark = pytest.mark.gpu

STATS = {}        # (family, arith) -> [worst err / bound, worst rms ratio, checks, case of the first, case of the second]
KERNELS = {}      # kernel name -> cases that met it
REFUSED = []      # (family, case, status)
SKIPPED = []      # cases left out to keep a float64 reference small
_REFS = {}        # references shared by the flag parametrisations of one shape


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\ntrain conformance: per family and arithmetic, the largest err/bound and rms ratio over the matrix")
    for (fam, a), (w, r, n, wc, rc) in sorted(STATS.items()):
        lim = go.R_ELEM if a == "elem" else go.R.get(a, 0)
        print(f"  {fam:24s} {a:7s} err/bound {w:.3g}  rms ratio {r:.3g} (R {lim:g})  {n} checks\n    worst err/bound: {wc}\n    worst rms: {rc}")
    print("  kernels met: " + ", ".join(f"{k} x{v}" for k, v in sorted(KERNELS.items())))
    print(f"  refused: {len(REFUSED)}")
    for fam, case, st in REFUSED:
        print(f"    {fam}: {case}: status {st}")
    print(f"  skipped to keep a float64 reference small: {len(SKIPPED)}" + "".join(f"\n    {c}" for c in SKIPPED))


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib, fastnsf                       # noqa: F401  (registers the signatures)
    from himo_amd.seflow import model, train                 # noqa: F401
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def _note(fam, arith, worst, rr, case, kernel=None):
    s = STATS.setdefault((fam, arith), [0.0, 0.0, 0, "", ""])
    if worst >= s[0]:
        s[0], s[3] = worst, case
    if rr >= s[1]:
        s[1], s[4] = rr, case
    s[2] += 1
    if kernel:
        KERNELS[kernel] = KERNELS.get(kernel, 0) + 1


def g2(gpu, values, pitch=None, off=0):
    """a [rows, cols] matrix at ``pitch`` (>= cols) floats per row, ``off`` floats past the 16-byte aligned base"""
    rows, cols = values.shape
    g = Guarded(layout(1, 1, 0, 0, rows, pitch or cols, cols), gpu, off=off)
    g.put(values.float())
    return g


def g4(gpu, values, pitch=None, gap=0):
    """[N, H, W, C] images, ``pitch`` floats per pixel, ``gap`` floats between images -> (Guarded, batch stride)"""
    n, h, w, c = values.shape
    pitch = pitch or c
    bs = h * w * pitch + gap
    g = Guarded(layout(n, n, bs, 0, h * w, pitch, c), gpu)
    g.put(values.float())
    return g, bs


def gflat(gpu, numel, values=None):
    g = Guarded(layout(1, 1, 0, 0, 1, max(numel, 1), numel), gpu)
    if values is not None:
        g.put(values.float())
    return g


def gws(gpu, nbytes, short=0):
    """a workspace of exactly ``nbytes`` (the library's own query), guarded"""
    return gflat(gpu, (int(nbytes) - short + 3) // 4)


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
            assert g.untouched_outside(), f"{case}: a write outside an output view (pitch gap, image gap or guard)"
        if self.ws is not None:
            assert self.ws.untouched_outside(), f"{case}: a write past the workspace size the query returned"

    def refused(self, fam, case, st, allowed):
        torch.cuda.synchronize()
        assert st in allowed, f"{case}: status {st}, expected one of {allowed}"
        for g in self.outputs:
            assert g.untouched(), f"{case}: refused (status {st}) but wrote"
        REFUSED.append((fam, case, st))


def _ok(fam, arith, got, ref, bnd, ref32, case, kernel=None, cols=True):
    """cols: the last axis is dY's output channel, whose scales span decades (grad_oracle.check_cols)"""
    assert not bool(torch.isnan(got).any()), f"{case}: NaN in the result (a read outside an input view, or an output element never written)"
    if arith == "elem":
        worst, rr = go.ok_elem(got, ref, bnd, ref32, case)
    else:
        worst, rr = go.ok_cols(got, ref, bnd, ref32, arith, case) if cols else co.ok(got, ref, bnd, ref32, arith, case)
    _note(fam, arith, worst, rr, case, kernel)


# ---- himo_conv3x3_wgrad_batch / _batch_bias ------------------------------------------------------------------------
def _batch_shapes():
    out = []
    i = 0
    for h in (2, 4, 24):
        for w in (32, 64, 96):
            for cin in (64, 192):
                for cout in (64, 192):
                    out.append((1, (1, 2, 5)[i % 3], h, w, cin, cout, (0, 4, 12)[(i // 2) % 3], (0, 8)[i % 2], 8 * (i % 2)))
                    i += 1
    for h in (2, 16):
        for w in (64, 128):
            for cin in (32, 64, 128):
                out.append((2, (1, 2, 5)[i % 3], h, w, cin, (64, 192)[i % 2], (0, 4, 12)[(i // 2) % 3], (0, 8)[i % 2], 8 * (i % 2)))
                i += 1
    return out


BATCH_SHAPES = _batch_shapes()      # (stride, n_img, h, w, cin, cout, x pitch pad, dy pitch pad, image gap)


def _batch_kernel(stride, flags):
    if flags & 2:
        return "conv_wgrad_split_kernel" if stride == 1 else "conv_wgrad_split2_kernel"
    return f"conv_wgrad_tiled_kernel<{stride}>"


def _batch_refs(key, shape):
    if key not in _REFS:
        stride, n, h, w, cin, cout = shape[:6]
        x, dy = go.operands(1000 + key, (n, h, w, cin), (n, h // stride, w // stride, cout))
        old = torch.randn(3, 3, cin, cout, generator=torch.Generator().manual_seed(key)) * 0.5
        _REFS[key] = dict(x=x, dy=dy, old=old, ref=go.conv3x3_dw(x, dy, stride), ref32=go.conv3x3_dw(x, dy, stride, torch.float32))
    return _REFS[key]


def _batch_case(lib, gpu, key, shape, flags, bias=False):
    stride, n, h, w, cin, cout, xpad, ypad, gap = shape
    r = _batch_refs(key, shape)
    arith = "bf16x2" if flags & 2 else "f32"
    acc = bool(flags & 1)
    kernel = _batch_kernel(stride, flags)
    case = f"wgrad_batch{'_bias' if bias else ''} {kernel} flags={flags} s={stride} n={n} h={h} w={w} cin={cin} cout={cout} " \
           f"xp={cin + xpad} dyp={cout + ypad} gap={gap}"
    xg, x_bs = g4(gpu, r["x"], cin + xpad, gap)
    dg, d_bs = g4(gpu, r["dy"], cout + ypad, 2 * gap)
    dw = gflat(gpu, 9 * cin * cout, r["old"] if acc else None)
    old_b = torch.randn(cout, generator=torch.Generator().manual_seed(key + 7))
    db = gflat(gpu, cout, old_b if acc else None)
    need = int(lib.himo_conv_wgrad_batch_workspace_bytes(n, h, w, cin, cout, stride))
    assert need > 0, case
    ws = gws(gpu, need)
    c = Call([xg, dg], [dw, db] if bias else [dw], ws)
    if bias:
        st = lib.himo_conv3x3_wgrad_batch_bias(n, xg.ptr, x_bs, cin + xpad, h, w, cin, dg.ptr, d_bs, cout + ypad, cout, stride, dw.ptr, db.ptr,
                                               flags, ws.ptr, need, _s())
    else:
        st = lib.himo_conv3x3_wgrad_batch(n, xg.ptr, x_bs, cin + xpad, h, w, cin, dg.ptr, d_bs, cout + ypad, cout, stride, dw.ptr,
                                          flags, ws.ptr, need, _s())
    assert st == 0, f"{case}: status {st}"
    c.check(case)
    key_b = (key, arith, acc)
    if key_b not in _REFS:
        _REFS[key_b] = go.conv3x3_dw_bound(arith, r["x"], r["dy"], stride, r["old"] if acc else None)
    add = r["old"] if acc else 0
    _ok("conv3x3_wgrad_batch", arith, dw.get().reshape(3, 3, cin, cout), r["ref"] + (r["old"].double() if acc else 0),
        _REFS[key_b], r["ref32"] + add, case, kernel)
    if bias:
        ob = old_b if acc else None
        _ok("wgrad_batch_bias db", "f32", db.get().reshape(cout), go.colsum(r["dy"]) + (old_b.double() if acc else 0),
            go.colsum_bound(r["dy"], ob), go.colsum(r["dy"], torch.float32) + (old_b if acc else 0), case + " db")


@pytest.mark.parametrize("flags", [0, 1, 2, 3, 6])
def test_conv3x3_wgrad_batch(lib, gpu, flags):
    """The four tiled kernels at the limits of wgrad_tiled_ok: h = 2, w = 32 / 64, cin = 32 at stride 2, cout = 64 and 192;
    n_img 1, 2, 5 (the n_tiles / 4 clamp, one chunk, ragged last chunks); pitches wider than the channels, image gaps;
    accumulate onto a non-zero dW; flag 4 (one block per CU: another split of the pixel chunks)."""
    for key, shape in enumerate(BATCH_SHAPES):
        _batch_case(lib, gpu, key, shape, flags)


@pytest.mark.parametrize("flags", [2, 3, 6])
def test_conv3x3_wgrad_batch_bias(lib, gpu, flags):
    """the same stride-1 split cases with the bias gradient from the same pass over dY; stride 2 / flag 0: UNSUPPORTED"""
    from himo_amd import _lib
    for key, shape in enumerate(BATCH_SHAPES):
        if shape[0] == 1:
            _batch_case(lib, gpu, key, shape, flags, bias=True)
    for stride, fl in ((2, 2), (1, 0), (1, 1)):
        n, h, w, cin, cout = 1, 4, 64, 64, 64
        x, dy = go.operands(5, (n, h, w, cin), (n, h // stride, w // stride, cout))
        xg, x_bs = g4(gpu, x)
        dg, d_bs = g4(gpu, dy)
        dw, db = gflat(gpu, 9 * cin * cout), gflat(gpu, cout)
        need = int(lib.himo_conv_wgrad_batch_workspace_bytes(n, h, w, cin, cout, stride))
        ws = gws(gpu, need)
        c = Call([xg, dg], [dw, db, ws])
        st = lib.himo_conv3x3_wgrad_batch_bias(n, xg.ptr, x_bs, cin, h, w, cin, dg.ptr, d_bs, cout, cout, stride, dw.ptr, db.ptr, fl,
                                               ws.ptr, need, _s())
        c.refused("wgrad_batch_bias", f"stride {stride} flags {fl}", st, (_lib.ERR_UNSUPPORTED,))


def test_conv3x3_wgrad_batch_refusals(lib, gpu):
    """what wgrad_tiled_ok and the pitch / workspace tests rule out: the documented status, dW and db untouched, and the
    workspace query returns 0 exactly where the SHAPE is unsupported (it does not see pitches)"""
    from himo_amd import _lib
    base = dict(stride=1, n=2, h=4, w=32, cin=64, cout=64, xp=64, dyp=64, xbs_add=0, dbs_add=0, short=0, ws_off=0)
    table = {"odd h": (dict(h=5), _lib.ERR_UNSUPPORTED, True), "w % 32": (dict(w=40), _lib.ERR_UNSUPPORTED, True),
             "cin = 32 at stride 1": (dict(cin=32, xp=32), _lib.ERR_UNSUPPORTED, True),
             "cin % 64": (dict(cin=96, xp=96), _lib.ERR_UNSUPPORTED, True), "cout % 64": (dict(cout=96, dyp=96), _lib.ERR_UNSUPPORTED, True),
             "stride 2, w % 64": (dict(stride=2, w=32), _lib.ERR_UNSUPPORTED, True),
             "stride 2, odd h": (dict(stride=2, h=3, w=64), _lib.ERR_UNSUPPORTED, True),
             "stride 3": (dict(stride=3), _lib.ERR_UNSUPPORTED, True),
             "x_pitch % 4": (dict(xp=66), _lib.ERR_UNSUPPORTED, False), "dy_pitch % 4": (dict(dyp=67), _lib.ERR_UNSUPPORTED, False),
             "x_batch_stride % 4": (dict(xbs_add=2), _lib.ERR_UNSUPPORTED, False),
             "dy_batch_stride % 4": (dict(dbs_add=1), _lib.ERR_UNSUPPORTED, False),
             "workspace one byte short": (dict(short=1), _lib.ERR_WORKSPACE, False),
             "workspace misaligned": (dict(ws_off=1), _lib.ERR_WORKSPACE, False)}
    for name, (change, status, zero_query) in table.items():
        p = dict(base, **change)
        s_ = p["stride"] if p["stride"] in (1, 2) else 1
        ho, wo = (p["h"] + s_ - 1) // s_, (p["w"] + s_ - 1) // s_
        x, dy = go.operands(9, (p["n"], p["h"], p["w"], p["cin"]), (p["n"], ho, wo, p["cout"]))
        xg, x_bs = g4(gpu, x, p["xp"], p["xbs_add"])
        dg, d_bs = g4(gpu, dy, p["dyp"], p["dbs_add"])
        dw, db = gflat(gpu, 9 * p["cin"] * p["cout"]), gflat(gpu, p["cout"])
        need = int(lib.himo_conv_wgrad_batch_workspace_bytes(p["n"], p["h"], p["w"], p["cin"], p["cout"], p["stride"]))
        assert (need == 0) == zero_query, (name, need)
        size = need or (1 << 20)
        ws = gflat(gpu, size // 4 + 4)
        for flags, with_db in ((0, False), (2, False), (2, True)):
            c = Call([xg, dg], [dw, db, ws])
            args = (p["n"], xg.ptr, x_bs, p["xp"], p["h"], p["w"], p["cin"], dg.ptr, d_bs, p["dyp"], p["cout"], p["stride"], dw.ptr)
            tail = (flags, ws.ptr + 4 * p["ws_off"], size - p["short"], _s())
            st = lib.himo_conv3x3_wgrad_batch_bias(*args, db.ptr, *tail) if with_db else lib.himo_conv3x3_wgrad_batch(*args, *tail)
            allowed = (status,) if not (with_db and p["stride"] != 1) else (status, _lib.ERR_UNSUPPORTED)
            c.refused("wgrad_batch refusals", f"{name} flags={flags} db={with_db}", st, allowed)


# ---- himo_conv3x3_wgrad (the fallback) ----------------------------------------------------------------------------------
FALLBACK_HW = [(1, 1), (1, 37), (33, 1), (7, 9), (19, 37), (65, 31), (130, 100)]
FALLBACK_CIN, FALLBACK_COUT = (1, 3, 4, 20, 132), (4, 36, 132)


def _fallback_case(lib, gpu, seed, n, h, w, cin, cout, stride, xpad, ypad, start_acc):
    """n images through n calls (the first with flag ``start_acc`` onto a non-zero dW, the others accumulating)"""
    ho, wo = go.out_size(h, stride), go.out_size(w, stride)
    chunk = max(256, (ho * wo + 47) // 48)
    chunk += chunk & 1
    case = f"wgrad conv_wgrad_partial_kernel s={stride} n={n} h={h} w={w} cin={cin} cout={cout} xp={cin + xpad} dyp={cout + ypad} " \
           f"first_flag={start_acc} chunks={(ho * wo + chunk - 1) // chunk}x{chunk}"
    x, dy = go.operands(seed, (n, h, w, cin), (n, ho, wo, cout))
    old = torch.randn(3, 3, cin, cout, generator=torch.Generator().manual_seed(seed)) * 0.5
    xg, x_bs = g4(gpu, x, cin + xpad, 5)
    dg, d_bs = g4(gpu, dy, cout + ypad, 3)
    dw = gflat(gpu, 9 * cin * cout, old if start_acc else None)
    need = int(lib.himo_conv_wgrad_workspace_bytes(ho, wo, cin, cout))
    ws = gws(gpu, need)
    c = Call([xg, dg], [dw], ws)
    for i in range(n):
        st = lib.himo_conv3x3_wgrad(xg.ptr + 4 * i * x_bs, cin + xpad, h, w, cin, dg.ptr + 4 * i * d_bs, cout + ypad, cout, stride, dw.ptr,
                                    1 if (i or start_acc) else 0, ws.ptr, need, _s())
        assert st == 0, f"{case}: status {st} at image {i}"
    c.check(case)
    n_acc = n - 1 + start_acc
    o = old if start_acc else torch.zeros_like(old)
    bnd = go.conv3x3_dw_bound("f32", x, dy, stride, o if n_acc else None, max(n_acc, 1))
    add = o if start_acc else 0
    _ok("conv3x3_wgrad", "f32", dw.get().reshape(3, 3, cin, cout), go.conv3x3_dw(x, dy, stride) + (o.double() if start_acc else 0), bnd,
        go.conv3x3_dw(x, dy, stride, torch.float32) + add, case, "conv_wgrad_partial_kernel")


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_wgrad_fallback(lib, gpu, stride):
    """any h, w >= 1 (odd sizes at stride 2: ho = (h + 1) / 2), ragged channel counts on both sides of the 128 tiles, pitches
    wider than the channels and no multiples of 4, several pixel chunks, the accumulate flag alone and over several images"""
    i = 0
    for (h, w) in FALLBACK_HW:
        for k in range(3):                                    # every size meets three (cin, cout) pairs; all values occur
            cin, cout = FALLBACK_CIN[(i + k) % 5], FALLBACK_COUT[(i + 2 * k) % 3]
            n = (1, 3, 2)[k]
            _fallback_case(lib, gpu, 2000 + 10 * i + k, n, h, w, cin, cout, stride, (0, 3, 6)[(i + k) % 3], (0, 5, 2)[(i + k) % 3], int(k == 0))
        i += 1
    for j, cin in enumerate(FALLBACK_CIN):                    # every cin against every cout once more, small
        for cout in FALLBACK_COUT:
            _fallback_case(lib, gpu, 2500 + j, 1, 7, 9, cin, cout, stride, 1, 2, 0)


def test_conv3x3_wgrad_fallback_refusals(lib, gpu):
    from himo_amd import _lib
    x, dy = go.operands(3, (1, 7, 9, 20), (1, 7, 9, 36))
    xg, _ = g4(gpu, x)
    dg, _ = g4(gpu, dy)
    dw = gflat(gpu, 9 * 20 * 36)
    need = int(lib.himo_conv_wgrad_workspace_bytes(7, 9, 20, 36))
    ws = gflat(gpu, need // 4 + 4)
    for name, (stride, size, off, status) in {"stride 3": (3, need, 0, _lib.ERR_INVALID_ARGUMENT), "workspace one byte short": (1, need - 1, 0, _lib.ERR_WORKSPACE),
                                              "workspace misaligned": (1, need, 1, _lib.ERR_WORKSPACE)}.items():
        c = Call([xg, dg], [dw, ws])
        st = lib.himo_conv3x3_wgrad(xg.ptr, 20, 7, 9, 20, dg.ptr, 36, 36, stride, dw.ptr, 0, ws.ptr + 4 * off, size, _s())
        c.refused("conv3x3_wgrad refusals", name, st, (status,))


# ---- himo_linear_wgrad_ex -------------------------------------------------------------------------------------------------
LINEAR_N = (1, 7, 9, 31, 33, 255, 257, 4097, 16383, 16384, 70_001)
LINEAR_CH = ((3, 64), (4, 128), (5, 20), (20, 132), (128, 128), (132, 36), (192, 128), (192, 256), (160, 256), (384, 64))
# operand layouts: (x pitch pad, dz pitch pad, offset in floats from a 16-byte boundary)
LINEAR_LAYOUTS = ((0, 0, 0), (4, 8, 0), (1, 3, 0), (0, 0, 1))


def _linear_kernel(n, cin, cout, flags, vec):
    if cin <= 4:
        return "wgrad_thin_partial_kernel"
    if flags & 2:
        return "wgrad_full_split_kernel" if (128 < cin <= 192 and cout in (128, 256) and n >= 16384) else "wgrad_partial_split_kernel"
    return "wgrad_partial_lds_kernel" if vec else "wgrad_partial_kernel"


def _linear_case(lib, gpu, seed, n, cin, cout, flags, with_db, lay):
    xpad, zpad, off = lay
    vec = not ((cin + xpad) & 3 or (cout + zpad) & 3 or cin & 3 or cout & 3 or off & 3)
    kernel = _linear_kernel(n, cin, cout, flags, vec)
    arith = "bf16x2" if "split" in kernel else "f32"
    acc = bool(flags & 1)
    case = f"linear_wgrad_ex {kernel} flags={flags} n={n} cin={cin} cout={cout} xp={cin + xpad} zp={cout + zpad} off={off} db={with_db}"
    x, dz = go.operands(seed, (n, cin), (n, cout))
    gen = torch.Generator().manual_seed(seed + 1)
    old, old_b = torch.randn(cin, cout, generator=gen), torch.randn(cout, generator=gen)
    xg, zg = g2(gpu, x, cin + xpad, off), g2(gpu, dz, cout + zpad, off)
    dw, db = gflat(gpu, cin * cout, old if acc else None), gflat(gpu, cout, old_b if acc else None)
    need = int(lib.himo_wgrad_workspace_bytes_ex(n, cin, cout))
    ws = gws(gpu, need)
    c = Call([xg, zg], [dw, db], ws)
    st = lib.himo_linear_wgrad_ex(n, xg.ptr, cin + xpad, cin, zg.ptr, cout + zpad, cout, dw.ptr, db.ptr if with_db else None, flags,
                                  ws.ptr, need, _s())
    assert st == 0, f"{case}: status {st}"
    c.check(case)
    if not with_db:
        assert db.untouched() or acc, f"{case}: d_db was NULL, something wrote a bias gradient"
    _ok("linear_wgrad_ex", arith, dw.get().reshape(cin, cout), go.linear_dw(x, dz) + (old.double() if acc else 0),
        go.linear_dw_bound(arith, x, dz, old if acc else None), go.linear_dw(x, dz, torch.float32) + (old if acc else 0), case, kernel)
    if with_db:
        _ok("linear_wgrad_ex db", "f32", db.get().reshape(cout), go.colsum(dz) + (old_b.double() if acc else 0),
            go.colsum_bound(dz, old_b if acc else None), go.colsum(dz, torch.float32) + (old_b if acc else 0), case + " db")


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_linear_wgrad_ex(lib, gpu, flags):
    """the thin, full-split, partial-split, LDS-vector and scalar kernels on both sides of their conditions: row counts at
    the 8 / 32 / 256-row and the 16384-row boundaries, ragged channel counts, pitches wider than the matrix, a pitch that is
    no multiple of 4, operands 4 bytes off a 16-byte boundary, with and without d_db.
    (The thin path's fall-through for a workspace too small for it cannot be reached: the entry point first requires
    himo_wgrad_workspace_bytes_ex(n, cin, cout) >= 65536 (ceil(n / 256) + 1) bytes, and the thin path needs at most
    20 cout min(512, ceil(n / 64)) -- fewer for every n and cout.  That branch is dead.)"""
    i = 0
    for n in LINEAR_N:
        for cin, cout in LINEAR_CH:
            i += 1
            if n == 70_001 and cin * cout > 20_000:
                SKIPPED.append(f"linear_wgrad_ex flags={flags} n={n} cin={cin} cout={cout}")
                continue
            _linear_case(lib, gpu, 3000 + i, n, cin, cout, flags, bool(i % 2), LINEAR_LAYOUTS[(i // 2) % 4])
    # the full-split kernel and its neighbours with every layout, with and without d_db
    if flags & 2:
        for j, lay in enumerate(LINEAR_LAYOUTS):
            for n in (16383, 16384):
                _linear_case(lib, gpu, 3500 + j, n, (192, 160)[j % 2], (256, 128)[j // 2], flags, bool((j + n) % 2), lay)


def test_linear_wgrad_and_colsum(lib, gpu):
    """himo_linear_wgrad (cin, cout <= 128, refused beyond) and both column-sum kernels (16-byte rows and not), n = 1 and
    ragged, accumulate; z_pitch < cout refused"""
    from himo_amd import _lib
    for i, (n, cin, cout, lay) in enumerate([(1, 20, 36, 0), (33, 128, 128, 1), (257, 4, 128, 2), (4097, 36, 20, 3)]):
        xpad, zpad, off = LINEAR_LAYOUTS[lay]
        x, dz = go.operands(4000 + i, (n, cin), (n, cout))
        xg, zg = g2(gpu, x, cin + xpad, off), g2(gpu, dz, cout + zpad, off)
        dw, db = gflat(gpu, cin * cout), gflat(gpu, cout)
        need = int(lib.himo_wgrad_workspace_bytes(n))
        ws = gws(gpu, need)
        c = Call([xg, zg], [dw, db], ws)
        case = f"linear_wgrad n={n} cin={cin} cout={cout} layout={LINEAR_LAYOUTS[lay]}"
        assert lib.himo_linear_wgrad(n, xg.ptr, cin + xpad, cin, zg.ptr, cout + zpad, cout, dw.ptr, db.ptr, ws.ptr, need, _s()) == 0, case
        c.check(case)
        _ok("linear_wgrad", "f32", dw.get().reshape(cin, cout), go.linear_dw(x, dz), go.linear_dw_bound("f32", x, dz),
            go.linear_dw(x, dz, torch.float32), case)
        _ok("linear_wgrad db", "f32", db.get().reshape(cout), go.colsum(dz), go.colsum_bound(dz), go.colsum(dz, torch.float32), case + " db")
    for cin, cout in ((132, 64), (64, 132)):
        x, dz = go.operands(1, (9, cin), (9, cout))
        xg, zg = g2(gpu, x), g2(gpu, dz)
        dw, db = gflat(gpu, cin * cout), gflat(gpu, cout)
        ws = gflat(gpu, int(lib.himo_wgrad_workspace_bytes_ex(9, cin, cout)) // 4)
        c = Call([xg, zg], [dw, db, ws])
        st = lib.himo_linear_wgrad(9, xg.ptr, cin, cin, zg.ptr, cout, cout, dw.ptr, db.ptr, ws.ptr, 4 * ws.shape[-1], _s())
        c.refused("linear_wgrad", f"cin={cin} cout={cout}", st, (_lib.ERR_INVALID_ARGUMENT,))
    i = 0
    for n in (1, 7, 255, 257, 4097, 70_001):
        for cout in (4, 20, 130, 256):
            for zpad, off in ((0, 0), (4, 0), (3, 0), (0, 1)):
                i += 1
                if (i % 3) and n > 300:
                    continue
                acc = i % 2
                _, z = go.operands(4100 + i, (1, 1), (n, cout))
                old = torch.randn(cout, generator=torch.Generator().manual_seed(i))
                zg = g2(gpu, z, cout + zpad, off)
                out = gflat(gpu, cout, old if acc else None)
                need = ((cout + 127) // 128) * ((n + 255) // 256) * 512                  # the header's formula
                ws = gws(gpu, need)
                vec = not ((cout + zpad) & 3 or cout & 3 or off)
                kernel = "colsum_partial_v4_kernel" if vec else "colsum_partial_kernel"
                case = f"colsum {kernel} n={n} cout={cout} zp={cout + zpad} off={off} acc={acc}"
                c = Call([zg], [out], ws)
                assert lib.himo_colsum(n, zg.ptr, cout + zpad, cout, out.ptr, acc, ws.ptr, need, _s()) == 0, case
                c.check(case)
                _ok("colsum", "f32", out.get().reshape(cout), go.colsum(z) + (old.double() if acc else 0), go.colsum_bound(z, old if acc else None),
                    go.colsum(z, torch.float32) + (old if acc else 0), case, kernel)
    _, z = go.operands(1, (1, 1), (9, 20))
    zg, out, ws = g2(gpu, z), gflat(gpu, 20), gflat(gpu, 128)
    c = Call([zg], [out, ws])
    c.refused("colsum", "z_pitch < cout", lib.himo_colsum(9, zg.ptr, 16, 20, out.ptr, 0, ws.ptr, 512, _s()), (_lib.ERR_INVALID_ARGUMENT,))
    c.refused("colsum", "workspace short", lib.himo_colsum(9, zg.ptr, 20, 20, out.ptr, 0, ws.ptr, 511, _s()), (_lib.ERR_WORKSPACE,))


# ---- exact kernels: stuffing, flips, transposes; the upsampling adjoint ----------------------------------------------
def test_zero_stuff_flip_transpose_are_exact(lib, gpu):
    from himo_amd import _lib
    g = torch.Generator().manual_seed(50)
    i = 0
    for (h, w) in ((1, 1), (1, 9), (7, 1), (5, 7), (16, 24)):
        for c_ in (4, 20, 64):
            n, pad = (1, 2, 3)[i % 3], 4 * (i % 3)
            dy = torch.randn(n, h, w, c_, generator=g)
            dg, d_bs = g4(gpu, dy, c_ + pad, 4 * (i % 2))
            zg, z_bs = g4(gpu, torch.zeros(n, 2 * h, 2 * w, c_), c_ + 2 * pad, 8 * (i % 2))
            zg.reset()
            c = Call([dg], [zg])
            case = f"zero_stuff2x n={n} h={h} w={w} c={c_} pad={pad}"
            assert lib.himo_zero_stuff2x(n, h, w, c_, dg.ptr, d_bs, c_ + pad, zg.ptr, z_bs, c_ + 2 * pad, _s()) == 0, case
            c.check(case)
            assert torch.equal(zg.words().view(torch.float32).reshape(n, 2 * h, 2 * w, c_), go.zero_stuff2x(dy)), case
            _note("zero_stuff2x", "exact", 0.0, 0.0, case, "zero_stuff_kernel")
            i += 1
    for name, (c_, dp, zp) in {"c % 4": (6, 8, 8), "dy_pitch % 4": (4, 6, 8), "z_pitch % 4": (4, 8, 6)}.items():
        dg, d_bs = g4(gpu, torch.randn(1, 3, 3, c_, generator=g), dp)
        zg, z_bs = g4(gpu, torch.zeros(1, 6, 6, c_), zp)
        zg.reset()
        c = Call([dg], [zg])
        c.refused("zero_stuff2x", name, lib.himo_zero_stuff2x(1, 3, 3, c_, dg.ptr, d_bs, dp, zg.ptr, z_bs, zp, _s()), (_lib.ERR_INVALID_ARGUMENT,))
    for (k, cin, cout) in ((3, 1, 1), (3, 3, 20), (3, 20, 132), (1, 36, 4), (3, 64, 64)):
        w_ = torch.randn(k, k, cin, cout, generator=g)
        wg, fg = gflat(gpu, w_.numel(), w_), gflat(gpu, w_.numel())
        c = Call([wg], [fg])
        case = f"weight_flip k={k} cin={cin} cout={cout}"
        assert lib.himo_weight_flip(wg.ptr, k, cin, cout, fg.ptr, _s()) == 0, case
        c.check(case)
        assert torch.equal(fg.get().reshape(k, k, cout, cin), go.weight_flip(w_)), case
        _note("weight_flip", "exact", 0.0, 0.0, case, "weight_flip_kernel")
    for (rows, cols) in ((1, 1), (1, 37), (33, 1), (20, 132), (192, 256), (3, 64)):
        w_ = torch.randn(rows, cols, generator=g)
        wg, tg = gflat(gpu, w_.numel(), w_), gflat(gpu, w_.numel())
        c = Call([wg], [tg])
        case = f"transpose {rows}x{cols}"
        assert lib.himo_transpose(wg.ptr, rows, cols, tg.ptr, _s()) == 0, case
        c.check(case)
        assert torch.equal(tg.get().reshape(cols, rows), w_.T.contiguous()), case
        _note("transpose", "exact", 0.0, 0.0, case, "transpose_kernel")


def test_upsample2x_bwd(lib, gpu):
    """the adjoint of the bilinear x2 upsampling against float64: h or w = 1, odd sizes, pitches; c % 4 and pitches % 4 refused"""
    from himo_amd import _lib
    g = torch.Generator().manual_seed(60)
    i = 0
    for (h, w) in ((1, 1), (1, 9), (7, 1), (5, 7), (17, 23), (2, 33), (32, 48)):
        for c_ in (4, 20, 64):
            pad = 4 * (i % 3)
            dy = torch.randn(2 * h, 2 * w, c_, generator=g)
            dg, _ = g4(gpu, dy[None], c_ + pad)
            xg, _ = g4(gpu, torch.zeros(1, h, w, c_), c_ + 2 * pad)
            xg.reset()
            c = Call([dg], [xg])
            case = f"upsample2x_bwd h={h} w={w} c={c_} pad={pad}"
            assert lib.himo_upsample2x_bwd(dg.ptr, c_ + pad, h, w, c_, xg.ptr, c_ + 2 * pad, _s()) == 0, case
            c.check(case)
            _ok("upsample2x_bwd", "f32", xg.get().reshape(h, w, c_), go.upsample2x_adjoint(dy), go.upsample2x_adjoint_bound(dy),
                go.upsample2x_adjoint(dy, torch.float32), case, "upsample2x_bwd_kernel", cols=False)
            i += 1
    for name, (c_, dp, xp) in {"c % 4": (6, 8, 8), "dy_pitch % 4": (4, 6, 8), "dx_pitch % 4": (4, 8, 6)}.items():
        dg, _ = g4(gpu, torch.randn(1, 6, 6, c_, generator=g), dp)
        xg, _ = g4(gpu, torch.zeros(1, 3, 3, c_), xp)
        xg.reset()
        c = Call([dg], [xg])
        c.refused("upsample2x_bwd", name, lib.himo_upsample2x_bwd(dg.ptr, dp, 3, 3, c_, xg.ptr, xp, _s()), (_lib.ERR_INVALID_ARGUMENT,))


# ---- element-wise kernels -----------------------------------------------------------------------------------------------
ROWS = (0, 1, 63, 65, 4097)


def _sat(t, a, g):
    """a tenth of the entries pushed to +-a: the saturated ends of sigmoid / tanh / GELU"""
    return torch.where(torch.rand(t.shape, generator=g) < 0.1, torch.where(t < 0, -a, a).to(t.dtype), t)


def _elem_check(name, args, outs, case, kernel):
    ref, ref32, bnd = go.elementwise(name, **args), go.elementwise(name, torch.float32, **args), go.elementwise_bound(name, **args)
    for key, got in outs.items():
        if got.numel() == 0:
            continue
        _ok(name, "elem", got, ref[key], bnd[key], ref32[key], f"{case} {key}", kernel)


@pytest.mark.parametrize("n", ROWS)
def test_gru_elementwise(lib, gpu, n):
    g = torch.Generator().manual_seed(70 + n)
    rn = lambda *s: torch.randn(*s, generator=g)
    hx, z, r = rn(n, 192), torch.rand(n, 128, generator=g), torch.rand(n, 128, generator=g)
    q = torch.tanh(_sat(rn(n, 128), 12.0, g))
    G = lambda t: g2(gpu, t) if t.shape[0] else gflat(gpu, 0)
    E = lambda cols: g2(gpu, torch.zeros(max(n, 1), cols)) if n else gflat(gpu, 0)

    def fresh(cols):
        e = E(cols)
        e.reset()
        return e
    V = lambda e, cols: e.get().reshape(n, cols)
    # forward, gate 1
    a = dict(pre=_sat(rn(n, 256) * 3, 30.0, g), hx=hx)
    ins, (zo, ro, oo) = [G(a["pre"]), G(hx)], (fresh(128), fresh(128), fresh(192))
    c = Call(ins, [zo, ro, oo])
    assert lib.himo_gru_gates_fwd(n, 1, ins[0].ptr, None, ins[1].ptr, zo.ptr, ro.ptr, None, oo.ptr, _s()) == 0
    c.check(f"gru_gates_fwd 1 n={n}")
    _elem_check("gru_gates1", a, dict(z=V(zo, 128), r=V(ro, 128), out=V(oo, 192)), f"gru_gates_fwd which=1 n={n}", "gru_gate1_kernel")
    # forward, gate 2
    a = dict(pre=_sat(rn(n, 128) * 3, 20.0, g), z=z, hx=hx)
    ins, (qo, oo) = [G(a["pre"]), G(z), G(hx)], (fresh(128), fresh(192))
    c = Call(ins, [qo, oo])
    assert lib.himo_gru_gates_fwd(n, 2, ins[0].ptr, ins[1].ptr, ins[2].ptr, None, None, qo.ptr, oo.ptr, _s()) == 0
    c.check(f"gru_gates_fwd 2 n={n}")
    _elem_check("gru_gates2", a, dict(q=V(qo, 128), out=V(oo, 192)), f"gru_gates_fwd which=2 n={n}", "gru_gate2_kernel")
    # backward 1
    a = dict(dh_next=rn(n, 128), z=z, q=q, hx=hx)
    ins, outs = [G(a["dh_next"]), G(z), G(q), G(hx)], (fresh(128), fresh(128), fresh(128))
    c = Call(ins, list(outs))
    assert lib.himo_gru_bwd1(n, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, _s()) == 0
    c.check(f"gru_bwd1 n={n}")
    _elem_check("gru_bwd1", a, dict(daq=V(outs[0], 128), dz=V(outs[1], 128), dhp=V(outs[2], 128)), f"gru_bwd1 n={n}", "gru_bwd1_kernel")
    # backward 2 (dhp and dx are read and written)
    a = dict(d_rhx=rn(n, 192), hx=hx, z=z, r=r, dz=rn(n, 128), dhp=rn(n, 128), dx=rn(n, 64))
    ins = [G(a[k]) for k in ("d_rhx", "hx", "z", "r", "dz")]
    dhp, dx, dazr = G(a["dhp"]), G(a["dx"]), fresh(256)
    c = Call(ins, [dhp, dazr, dx])
    assert lib.himo_gru_bwd2(n, *[t.ptr for t in ins], dhp.ptr, dazr.ptr, dx.ptr, _s()) == 0
    c.check(f"gru_bwd2 n={n}")
    _elem_check("gru_bwd2", a, dict(dhp=V(dhp, 128), dazr=V(dazr, 256), dx=V(dx, 64)), f"gru_bwd2 n={n}", "gru_bwd2_kernel")
    # backward 3
    a = dict(d_hx=rn(n, 192), dhp=rn(n, 128), dx=rn(n, 64))
    ins, dh, dx = [G(a["d_hx"]), G(a["dhp"])], fresh(128), G(a["dx"])
    c = Call(ins, [dh, dx])
    assert lib.himo_gru_bwd3(n, ins[0].ptr, ins[1].ptr, dh.ptr, dx.ptr, _s()) == 0
    c.check(f"gru_bwd3 n={n}")
    _elem_check("gru_bwd3", a, dict(dh=V(dh, 128), dx=V(dx, 64)), f"gru_bwd3 n={n}", "gru_bwd3_kernel")


@pytest.mark.parametrize("rows", ROWS)
def test_pitched_elementwise(lib, gpu, rows):
    """affine-GELU forward / backward (with and without scale / shift), add2d, mask_rows, rows_add (with / without d_b,
    zero_tail), pitches wider than the columns"""
    g = torch.Generator().manual_seed(80 + rows)
    rn = lambda *s: torch.randn(*s, generator=g)
    P = lambda t, pitch: g2(gpu, t, pitch) if t.shape[0] else gflat(gpu, 0)

    def fresh(cols, pitch, full=False):
        e = g2(gpu, torch.zeros(max(rows, 1), pitch if full else cols), pitch)
        e.reset()
        return e
    V = lambda e, cols: e.get().reshape(-1, e.shape[-1])[:rows, :cols]
    for ch, pads in ((20, (0, 0, 0)), (20, (4, 8, 12)), (64, (3, 1, 2)), (1, (0, 2, 5))):
        for affine in (True, False):
            sc, sh = (torch.rand(ch, generator=g) + 0.5, rn(ch) * 0.1) if affine else (None, None)
            scg, shg = (gflat(gpu, ch, sc), gflat(gpu, ch, sh)) if affine else (None, None)
            a = dict(x=_sat(rn(rows, ch) * 2, 10.0, g), scale=sc, shift=sh)
            xg, pre, y = P(a["x"], ch + pads[0]), fresh(ch, ch + pads[1]), fresh(ch, ch + pads[2])
            c = Call([xg] + ([scg, shg] if affine else []), [pre, y])
            case = f"affine_gelu_fwd rows={rows} ch={ch} pads={pads} affine={affine}"
            assert lib.himo_affine_gelu_fwd(rows, ch, xg.ptr, ch + pads[0], scg.ptr if affine else None, shg.ptr if affine else None,
                                            pre.ptr, ch + pads[1], y.ptr, ch + pads[2], _s()) == 0, case
            c.check(case)
            _elem_check("affine_gelu_fwd", a, dict(pre=V(pre, ch), y=V(y, ch)), case, "affine_gelu_fwd_kernel")
            a = dict(dy=rn(rows, ch), pre=_sat(rn(rows, ch) * 2, 10.0, g), scale=sc)
            dyg, pg, dx = P(a["dy"], ch + pads[2]), P(a["pre"], ch + pads[0]), fresh(ch, ch + pads[1])
            c = Call([dyg, pg] + ([scg] if affine else []), [dx])
            case = f"affine_gelu_bwd rows={rows} ch={ch} pads={pads} affine={affine}"
            assert lib.himo_affine_gelu_bwd(rows, ch, dyg.ptr, ch + pads[2], pg.ptr, ch + pads[0], scg.ptr if affine else None, dx.ptr,
                                            ch + pads[1], _s()) == 0, case
            c.check(case)
            _elem_check("affine_gelu_bwd", a, dict(dx=V(dx, ch)), case, "affine_gelu_bwd_kernel")
        # add2d: y += b
        a = dict(y=rn(rows, ch), b=rn(rows, ch))
        bg, yg = P(a["b"], ch + pads[0]), P(a["y"], ch + pads[1])
        c = Call([bg], [yg])
        case = f"add2d rows={rows} cols={ch} pads={pads}"
        assert lib.himo_add2d(rows, ch, bg.ptr, ch + pads[0], yg.ptr, ch + pads[1], _s()) == 0, case
        c.check(case)
        _elem_check("add2d", a, dict(y=V(yg, ch) if rows else torch.zeros(0, ch)), case, "add2d_kernel")
        # mask_rows: rows with a negative cell id are zeroed, the others bit-unchanged
        v = rn(rows, ch)
        pid = torch.randint(-2, 3, (rows,), generator=g, dtype=torch.int32)
        vg = P(v, ch + pads[2])
        pg = gflat(gpu, rows, None)
        if rows:
            pg.put(pid)
        c = Call([pg], [vg])
        case = f"mask_rows rows={rows} cols={ch} pitch={ch + pads[2]}"
        assert lib.himo_mask_rows(rows, ch, pg.ptr, vg.ptr, ch + pads[2], _s()) == 0, case
        c.check(case)
        if rows:
            assert torch.equal(V(vg, ch), torch.where(pid[:, None] < 0, torch.zeros_like(v), v)), case
        _note("mask_rows", "exact", 0.0, 0.0, case, "mask_rows_kernel")
        # rows_add: y = a + s b; zero_tail clears the columns cols .. y_pitch - 1
        for with_b in (True, False):
            for zero_tail in (0, 1):
                a = dict(a=rn(rows, ch), b=rn(rows, ch) if with_b else None, b_scale=-1.5)
                ag, bg = P(a["a"], ch + pads[0]), (P(a["b"], ch + pads[1]) if with_b else None)
                yp = ch + pads[2]
                yg = fresh(ch, yp, full=bool(zero_tail))
                c = Call([ag] + ([bg] if with_b else []), [yg])
                case = f"rows_add rows={rows} cols={ch} pads={pads} b={with_b} zero_tail={zero_tail}"
                assert lib.himo_rows_add(rows, ch, ag.ptr, ch + pads[0], bg.ptr if with_b else None, ch + pads[1], -1.5, yg.ptr, yp,
                                         zero_tail, _s()) == 0, case
                c.check(case)
                if rows:
                    got = yg.get().reshape(-1, yg.shape[-1])[:rows]
                    if zero_tail:
                        assert bool(torch.all(got[:, ch:] == 0)), f"{case}: the tail was not cleared"
                    _elem_check("rows_add", a, dict(y=got[:, :ch]), case, "rows_add_kernel")


def test_elementwise_refusals(lib, gpu):
    from himo_amd import _lib
    t = torch.randn(9, 20, generator=torch.Generator().manual_seed(1))
    bg, yg = g2(gpu, t), g2(gpu, t)
    yg.reset()
    c = Call([bg], [yg])
    c.refused("add2d", "y_pitch < cols", lib.himo_add2d(9, 20, bg.ptr, 20, yg.ptr, 16, _s()), (_lib.ERR_INVALID_ARGUMENT,))
    c.refused("add2d", "b_pitch < cols", lib.himo_add2d(9, 20, bg.ptr, 16, yg.ptr, 20, _s()), (_lib.ERR_INVALID_ARGUMENT,))
    c.refused("rows_add", "y_pitch < cols", lib.himo_rows_add(9, 20, bg.ptr, 20, None, 0, 0.0, yg.ptr, 16, 0, _s()), (_lib.ERR_INVALID_ARGUMENT,))
    c.refused("rows_add", "b_pitch < cols", lib.himo_rows_add(9, 20, bg.ptr, 20, bg.ptr, 16, 1.0, yg.ptr, 20, 0, _s()), (_lib.ERR_INVALID_ARGUMENT,))
    c.refused("mask_rows", "pitch < cols", lib.himo_mask_rows(9, 20, bg.ptr, yg.ptr, 16, _s()), (_lib.ERR_INVALID_ARGUMENT,))
    c.refused("gru_gates_fwd", "which = 3", lib.himo_gru_gates_fwd(9, 3, bg.ptr, bg.ptr, bg.ptr, yg.ptr, yg.ptr, yg.ptr, yg.ptr, _s()),
              (_lib.ERR_INVALID_ARGUMENT,))
    c.refused("affine_gelu_fwd", "scale without shift", lib.himo_affine_gelu_fwd(9, 20, bg.ptr, 20, bg.ptr, None, yg.ptr, 20, yg.ptr, 20, _s()),
              (_lib.ERR_INVALID_ARGUMENT,))
