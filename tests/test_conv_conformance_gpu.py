"""Conformance of himo_conv2d (and himo_upsample2x_batch_ex) over the descriptors the ABI admits, not only the shapes the
network happens to use: ragged channel counts, H or W of 1, odd stride-2 sizes, pitches, offsets, n_outer, every tile
variant, every arithmetic.  For every descriptor the library must either refuse it (a non-OK status, output bytes
untouched) or return a result within the worst-case bound of oracle/conv_oracle.py against float64, with no byte outside
the output view changed.

Every operand lives inside a larger buffer with guard regions before and after it.  Everything that is not an operand --
pitch padding, gaps between images, the guards -- holds a fixed NaN bit pattern: a read of it poisons a result, and a
write into it shows up in the bitwise comparison after the call.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_oracle as co
import grad_oracle as go
from guarded import GUARD, NAN_BITS, Guarded, layout

pytestmark = pytest.mark.gpu

HINTS = (0, 0x41, 0x42, 0x81, 0x82, 0x1001, 0x1002, 0x1004, 0x1005, 0x1006, 0x1008, 0x1009, 0x100A, 0x100C)
PACK = {"bf16x3": 0, "f16x2": 1, "bf16x2": 2}

STATS = {}        # arith -> [worst err / bound, worst rms ratio, checks, case of the first, case of the second]
FALLBACKS = []    # (case, hint, status) of a pinned variant the shape does not admit


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nconv conformance: per arithmetic, the largest err/bound and rms ratio over the matrix")
    for a, (w, r, n, wc, rc) in sorted(STATS.items()):
        print(f"  {a:7s} err/bound {w:.3g}  rms ratio {r:.3g} (R {co.R[a]:g})  {n} checks\n    worst err/bound: {wc}\n    worst rms: {rc}")
    counts = {}
    for c, h, st in FALLBACKS:
        key = (c.split()[0], h, st) if h else (c, h, st)
        counts[key] = counts.get(key, 0) + 1
    print(f"  refused (a pinned variant the shape does not admit, or a documented limit): {len(FALLBACKS)}")
    for (c, h, st), k in sorted(counts.items()):
        print(f"    {c} hint {h:#x} status {st}: {k} cases")


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import model  # noqa: F401  (registers the convolution entry points)
    return _lib.load()


def _stream():
    from himo_amd import _lib
    return _lib.stream_handle()


def _note(arith, worst, rr, case=""):
    s = STATS.setdefault(arith, [0.0, 0.0, 0, "", ""])
    if worst > s[0]:
        s[0], s[3] = worst, case
    if rr > s[1]:
        s[1], s[4] = rr, case
    s[2] += 1


def split_encode(x):
    """float32 [..., C] (C % 16 == 0) -> (int32 words of the split activation format, float64 value h + l)"""
    h = x.half()
    l = (x - h.float()).half()
    g = x.shape[-1] // 16
    rec = torch.stack([h.reshape(*x.shape[:-1], g, 16), l.reshape(*x.shape[:-1], g, 16)], -2).reshape(*x.shape[:-1], 2 * x.shape[-1])
    return rec.view(torch.int32), h.double() + l.double()


def split_decode(words):
    t = words.view(torch.float16).reshape(*words.shape[:-1], words.shape[-1] // 16, 2, 16).double()
    return t.sum(-2).reshape(words.shape)


def conv_case(lib, gpu, arith, n, H, W, cin, cout, k=3, stride=1, epi=0, *, x_pitch=None, y_pitch=None, x_gap=0, y_gap=0,
              y_off=0, n_outer=1, outer_gap=0, groups=False, hints=(0,), act=0, aux_pad=4, seed=0, x_scale=1.0, bias=True,
              expect_ok=True):
    """One descriptor (k = 1: a row GEMM of H * W rows), run for every hint in ``hints``, checked against float64.

    groups: the "frames as channel groups" layout -- image i of a sample at channel offset i * cin of an (n * cin)-wide
    pixel, samples one map apart (n_outer of them).  Otherwise images are x_gap / y_gap floats apart beyond their map, and
    samples (n_outer > 1) outer_gap floats beyond n images.
    act & 8 (HIMO_ACT_ACCUMULATE): y holds a non-zero map before the call and must hold map + result after it.
    act & 16 (HIMO_ACT_STUFFED_2X): the operand is a compact [H / 2][W / 2] map (pitches, gaps and strides describe it) and the
    result is checked against the float64 adjoint of the stride-2 convolution (grad_oracle.conv3x3_dx)."""
    case = f"{arith} n={n} H={H} W={W} cin={cin} cout={cout} k={k} s={stride} epi={epi} xp={x_pitch} yp={y_pitch} " \
           f"gap={x_gap},{y_gap} off={y_off} outer={n_outer},{outer_gap} groups={groups} act={act}"
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    N = n * n_outer
    if groups:
        x_pitch, y_pitch = n * cin, n * cout
        x_bs, y_bs = cin, cout
        x_os, y_os = H * W * x_pitch + outer_gap, Ho * Wo * y_pitch + outer_gap
    else:
        x_pitch, y_pitch = x_pitch or cin, y_pitch or cout
        x_bs, y_bs = H * W * x_pitch + x_gap, Ho * Wo * y_pitch + y_gap
        x_os, y_os = n * x_bs + outer_gap, n * y_bs + outer_gap
    y_cols = cout // 2 if epi == 3 else cout
    x = torch.randn(N, H, W, cin, generator=g) * x_scale
    accumulate, stuffed = bool(act & 8), bool(act & 16)
    x_pixels = H * W
    if stuffed:
        xc = torch.randn(N, H // 2, W // 2, cin, generator=g) * x_scale
        x = go.zero_stuff2x(xc)
        x_pixels = (H // 2) * (W // 2)
        if not groups:
            x_bs = x_pixels * x_pitch + x_gap
            x_os = n * x_bs + outer_gap
    w = torch.randn(k, k, cin, cout, generator=g) / np.sqrt(k * k * cin)
    b = torch.randn(cout, generator=g) * 0.1 if (bias and epi != 6) else None
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    xg = Guarded(layout(N, n, x_bs, x_os, x_pixels, x_pitch, cin), gpu)
    if stuffed:
        xg.put(xc)
    elif act & 1:
        words, x64 = split_encode(x)
        xg.put(words)
        x = x64.float()              # exact: the value the kernel reads
    else:
        xg.put(x)
    yg = Guarded(layout(N, n, y_bs, y_os, Ho * Wo, y_pitch, y_cols if epi != 4 else 0), gpu, off=y_off)
    aux_in = aux_out = None
    ag_in = ag_out = None
    if epi in (3, 4, 6):
        assert N == 1, "the GRU / ReLU-mask epilogues address aux by output row"
        rows, C = Ho * Wo, (cout // 2 if epi == 3 else cout)
        aux_in = torch.rand(1, Ho, Wo, C, generator=g) if epi == 4 else torch.randn(1, Ho, Wo, C, generator=g)
        ag_in = Guarded(layout(1, 1, 0, 0, rows, C + aux_pad, C), gpu)
        ag_in.put(aux_in)
        if epi in (3, 4):
            aux_out = torch.randn(1, Ho, Wo, C, generator=g)
            ag_out = Guarded(layout(1, 1, 0, 0, rows, C + 2 * aux_pad, C), gpu)
    dev = lambda t: None if t is None else t.contiguous().to(gpu)
    wd, bd, scd, shd = dev(w), dev(b), dev(sc), dev(sh)
    from himo_amd.seflow.model import ConvDesc
    d = ConvDesc()
    d.x, d.x_batch_stride, d.x_pitch = xg.ptr, x_bs, x_pitch
    d.w, d.bias = wd.data_ptr(), (bd.data_ptr() if bd is not None else None)
    d.scale, d.shift = scd.data_ptr(), shd.data_ptr()
    d.y, d.y_batch_stride, d.y_pitch = yg.ptr, y_bs, y_pitch
    d.n, d.h, d.w_in, d.cin, d.cout, d.ksize, d.stride, d.epilogue = n, H, W, cin, cout, k, stride, epi
    d.n_outer, d.x_outer_stride, d.y_outer_stride = n_outer, x_os, y_os
    d.act_layout = act
    if ag_in is not None:
        d.aux_in, d.aux_in_pitch = ag_in.ptr, C + aux_pad
    if ag_out is not None:
        d.aux_out, d.aux_out_pitch = ag_out.ptr, C + 2 * aux_pad
    pk = None
    if arith != "f32":
        pk = torch.empty(int(lib.himo_conv_packed_weight_bytes(k, cin, cout)), dtype=torch.uint8, device=gpu)
        assert lib.himo_conv_pack_weights_ex(wd.data_ptr(), k, cin, cout, PACK[arith], pk.data_ptr(), _stream()) == 0
        d.w_packed, d.packed_format = pk.data_ptr(), PACK[arith]

    ref = co.conv_ref(x, w, b, stride, epi, sc, sh, aux_in, aux_out)
    ref32 = co.conv_ref(x, w, b, stride, epi, sc, sh, aux_in, aux_out, dtype=torch.float32)
    bnd = co.bound(arith, x, w, b, stride, epi, sc, sh, aux_in, aux_out, ref=ref, split_out=bool(act & 2))
    if stuffed and k == 3 and stride == 1 and epi == 0 and not (H & 1 or W & 1):
        # the same thing said independently: dX of a stride-2 convolution whose weights are these with taps and channels swapped back
        adj = go.conv3x3_dx(xc, w.flip(0, 1).permute(0, 1, 3, 2), 2, H, W) + (0 if b is None else b.double())
        assert torch.allclose(adj, ref["y"], rtol=1e-12, atol=1e-12), f"{case}: the two float64 references disagree"
    y0 = None
    if accumulate and ref["y"] is not None:
        y0 = torch.randn(N, Ho, Wo, y_cols, generator=g)
        ref["y"] = ref["y"] + y0.double()
        ref32["y"] = ref32["y"] + y0
        bnd["y"] = bnd["y"] + co.U * (y0.double().abs() + ref["y"].abs())       # one more rounding, of old + new
    x_before = xg.buf.clone()
    results = []
    for hint in hints:
        yg.reset()
        if y0 is not None:
            yg.put(y0)
        y_before = yg.buf.clone()
        if ag_out is not None:
            ag_out.reset()
            if epi == 4:
                ag_out.put(aux_out)
        d.tile_hint = hint
        st = lib.himo_conv2d(ctypes.byref(d), _stream())
        torch.cuda.synchronize()
        if st != 0:
            assert not expect_ok or hint != 0, f"{case}: refused (status {st})"
            FALLBACKS.append((case, hint, st))
            assert yg.untouched_outside() and torch.equal(yg.buf, y_before), f"{case} hint {hint:#x}: refused but wrote"
            continue
        assert expect_ok, f"{case}: accepted a descriptor it should refuse"
        tag = f"{case} hint={hint:#x}"
        assert torch.equal(xg.buf, x_before), f"{tag}: the input was written"
        assert yg.untouched_outside(), f"{tag}: a write outside the output view (pitch gap, image gap or guard)"
        checks = []
        if epi != 4:
            got = yg.words()
            got = split_decode(got) if act & 2 else got.view(torch.float32)
            checks.append(("y", got.reshape(N, Ho, Wo, y_cols)))
        if ag_out is not None:
            assert ag_out.untouched_outside(), f"{tag}: a write outside aux_out's view"
            checks.append(("aux_out", ag_out.get().reshape(1, Ho, Wo, -1)))
        if ag_in is not None:
            assert ag_in.untouched_outside()
        for key, got in checks:
            worst, rr = co.ok(got, ref[key], bnd[key], ref32[key], arith, f"{tag} {key}")
            _note(arith, worst, rr, f"{tag} {key}")
        results.append(hint)
    return results


ARITHS = ["f32", "bf16x3", "f16x2", "bf16x2"]
S1_SHAPES = [(1, 1, 1, 16, 32), (2, 1, 37, 32, 64), (1, 33, 1, 16, 32), (2, 2, 2, 4, 4), (1, 7, 45, 12, 20),
             (3, 19, 37, 20, 68), (1, 31, 33, 36, 132), (2, 17, 65, 64, 100), (1, 9, 70, 132, 36),
             # H against the 1 / 2 / 4 / 8 / 12-row wave tiles, W against the 32-pixel segments
             (1, 3, 31, 16, 32), (1, 5, 32, 16, 68), (2, 9, 33, 32, 64), (1, 13, 63, 16, 48), (1, 12, 65, 64, 64)]
S2_SHAPES = [(1, 1, 1, 16, 32), (2, 3, 5, 16, 32), (1, 33, 17, 32, 64), (2, 65, 31, 64, 132), (1, 2, 2, 4, 4), (1, 7, 9, 20, 36)]


@pytest.mark.parametrize("arith", ARITHS)
def test_3x3_stride1(lib, gpu, arith):
    for i, (n, H, W, ci, co_) in enumerate(S1_SHAPES):
        epi = 0 if arith == "bf16x2" else i % 3
        conv_case(lib, gpu, arith, n, H, W, ci, co_, epi=epi, seed=i)


@pytest.mark.parametrize("arith", ARITHS)
def test_3x3_stride2(lib, gpu, arith):
    for i, (n, H, W, ci, co_) in enumerate(S2_SHAPES):
        epi = 0 if arith == "bf16x2" else i % 3
        conv_case(lib, gpu, arith, n, H, W, ci, co_, stride=2, epi=epi, seed=50 + i)


GEMM_CH = [(4, 4), (4, 128), (12, 36), (132, 20), (192, 256), (256, 192)]


@pytest.mark.parametrize("arith", ARITHS)
def test_row_gemm(lib, gpu, arith):
    """1x1: both sides of the Cout % 32 vector-store condition, partial 32-row blocks."""
    i = 0
    for rows in (1, 31, 33, 4097, 70_001):
        for ci, co_ in GEMM_CH:
            if rows == 70_001 and ci * co_ > 20_000:
                continue                                        # keeps the float64 reference small
            epi = 0 if arith == "bf16x2" else i % 3
            conv_case(lib, gpu, arith, 1, 1, rows, ci, co_, k=1, epi=epi, seed=100 + i)
            i += 1


@pytest.mark.parametrize("arith", ["f32", "bf16x3", "f16x2"])
def test_gru_epilogues(lib, gpu, arith):
    """z|r and q on the head's row GEMMs (192 -> 256 | 128) and ragged ones, aux pitches wider than their columns."""
    for i, (rows, ci, co_) in enumerate([(4097, 192, 256), (333, 192, 128), (65, 36, 72), (31, 20, 40)]):
        for epi in (3, 4):
            conv_case(lib, gpu, arith, 1, 1, rows, ci, co_ if epi == 3 else co_ // 2, k=1, epi=epi, aux_pad=4 + 4 * i,
                      seed=200 + i)


@pytest.mark.parametrize("arith", ARITHS)
def test_relu_epilogues(lib, gpu, arith):
    """Bias + ReLU and the ReLU mask on the FastNSF row GEMMs (4 and 128 channels), plus a ragged one."""
    for i, (rows, ci, co_) in enumerate([(4097, 4, 128), (4097, 128, 128), (1000, 128, 4), (333, 36, 20)]):
        for epi in (5, 6):
            if arith == "bf16x2" and epi == 5:
                continue
            for pad in (0, 6):      # an aux_in pitch that is no multiple of 4 leaves the 16-byte mask loads
                conv_case(lib, gpu, arith, 1, 1, rows, ci, co_, k=1, epi=epi, aux_pad=pad, seed=300 + i)


@pytest.mark.parametrize("arith", ARITHS)
def test_addressing(lib, gpu, arith):
    """Pitches, misaligned / offset outputs, image and sample gaps, n_outer in both layouts; 3x3 and 1x1."""
    epi = 0 if arith == "bf16x2" else 1
    for k, (n, H, W, ci, co_) in ((3, (2, 9, 35, 20, 36)), (1, (2, 1, 333, 36, 64))):
        kw = dict(k=k, epi=epi)
        conv_case(lib, gpu, arith, n, H, W, ci, co_, x_pitch=ci + 12, y_pitch=co_ + 8, x_gap=20, y_gap=12, seed=1, **kw)
        conv_case(lib, gpu, arith, n, H, W, ci, co_, y_pitch=co_ + 2, seed=2, **kw)        # y_pitch % 4 != 0: scalar stores
        conv_case(lib, gpu, arith, n, H, W, ci, co_, y_off=4, seed=3, **kw)                # 16 bytes off a 64-byte boundary
        conv_case(lib, gpu, arith, n, H, W, ci, co_, y_off=1, y_pitch=co_ + 1, y_gap=3, seed=4, **kw)   # y not 16-byte aligned
        conv_case(lib, gpu, arith, 3, H, W, ci, co_, n_outer=2, groups=True, seed=5, **kw)  # frames as channel groups
        conv_case(lib, gpu, arith, n, H, W, ci, co_, n_outer=3, outer_gap=28, x_gap=8, y_gap=4, seed=6, **kw)


TILE_SHAPES = [(1, 5, 33, 16, 32), (2, 13, 37, 36, 68), (1, 9, 65, 64, 128), (1, 7, 31, 132, 100)]


@pytest.mark.parametrize("arith", ["f32", "bf16x3", "f16x2", "bf16x2"])
def test_every_tile_hint(lib, gpu, arith):
    """Every hint of SeFlowTrainer.TILE_HINTS and SeFlowNet._tune: within the bound, or refused / the heuristic."""
    for i, shape in enumerate(TILE_SHAPES):
        epi = 0 if arith == "bf16x2" else 1
        assert conv_case(lib, gpu, arith, *shape, epi=epi, hints=HINTS, seed=400 + i)
        if arith != "bf16x2":
            conv_case(lib, gpu, arith, *shape, stride=2, epi=2, hints=HINTS, seed=410 + i)
    for i, (rows, ci, co_) in enumerate([(333, 36, 68), (4097, 64, 128)]):
        conv_case(lib, gpu, arith, 1, 1, rows, ci, co_, k=1, hints=HINTS, seed=420 + i)


@pytest.mark.parametrize("arith", ARITHS)
def test_conv2d_nhwc_caller(gpu, arith):
    """The stand-alone operator the other suites use, at ragged shapes, against the same bound."""
    from himo_amd.seflow.model import conv2d_nhwc
    g = torch.Generator().manual_seed(600)
    for (n, H, W, ci, co_, k, s) in [(2, 7, 45, 12, 20, 3, 1), (1, 33, 17, 36, 68, 3, 2), (3, 1, 37, 20, 36, 1, 1)]:
        if arith == "bf16x2" and s == 2:
            continue
        x = torch.randn(n, H, W, ci, generator=g)
        w = torch.randn(k, k, ci, co_, generator=g) / np.sqrt(k * k * ci)
        b = torch.randn(co_, generator=g) * 0.1
        got = conv2d_nhwc(x.to(gpu), w.to(gpu), b.to(gpu), stride=s, precision=arith).cpu()
        ref = co.conv_ref(x, w, b, s)
        bnd = co.bound(arith, x, w, b, s, ref=ref)
        worst, rr = co.ok(got, ref["y"], bnd["y"], co.conv_ref(x, w, b, s, dtype=torch.float32)["y"], arith,
                          f"conv2d_nhwc {arith} {(n, H, W, ci, co_, k, s)}")
        _note(arith, worst, rr, f"conv2d_nhwc {(n, H, W, ci, co_, k, s)}")


def test_data_gradient_forms(lib, gpu):
    """HIMO_ACT_ACCUMULATE (3x3 stride 1 in the two-term bf16 split; row GEMMs of either bf16 split) onto a non-zero map, and
    HIMO_ACT_STUFFED_2X alone and with accumulate against the float64 adjoint of the stride-2 convolution: ragged shapes,
    compact maps with h or w = 1, pitches and gaps, every hint; the combinations the header rules out are refused."""
    for i, (n, H, W, ci, co_) in enumerate(S1_SHAPES):
        kw = dict(x_pitch=ci + 12, y_pitch=co_ + 8, x_gap=20, y_gap=12) if i % 2 else {}
        conv_case(lib, gpu, "bf16x2", n, H, W, ci, co_, act=8, seed=700 + i, **kw)
    i = 0
    for arith in ("bf16x3", "bf16x2"):
        for rows in (1, 33, 4097):
            for ci, co_ in GEMM_CH:
                kw = dict(x_pitch=ci + 4, y_pitch=co_ + 12) if i % 2 else {}
                conv_case(lib, gpu, arith, 1, 1, rows, ci, co_, k=1, act=8, seed=720 + i, **kw)
                i += 1
    for i, (n, hc, wc, ci, co_) in enumerate([(1, 1, 1, 16, 32), (2, 1, 19, 32, 64), (1, 17, 1, 16, 32), (2, 5, 7, 20, 36),
                                              (1, 9, 33, 64, 100), (1, 16, 16, 132, 36)]):
        for act in (16, 24):
            kw = dict(x_pitch=ci + 8, y_pitch=co_ + 4, x_gap=12, y_gap=20) if i % 2 else {}
            assert conv_case(lib, gpu, "bf16x2", n, 2 * hc, 2 * wc, ci, co_, act=act, hints=HINTS, seed=760 + 2 * i + act // 16, **kw)
    for act in (8, 16, 24):                                   # what the header rules out
        conv_case(lib, gpu, "f16x2", 1, 6, 8, 16, 32, act=act, expect_ok=False)
        conv_case(lib, gpu, "f32", 1, 6, 8, 16, 32, act=act, expect_ok=False)
        conv_case(lib, gpu, "bf16x2", 1, 6, 8, 16, 32, act=act, stride=2, expect_ok=False)
        conv_case(lib, gpu, "bf16x2", 1, 6, 8, 16, 32, act=act, epi=5, expect_ok=False)
    conv_case(lib, gpu, "bf16x3", 1, 6, 8, 16, 32, act=8, expect_ok=False)              # 3x3 accumulate: the two-term split only
    conv_case(lib, gpu, "bf16x3", 1, 6, 8, 16, 32, act=16, expect_ok=False)
    conv_case(lib, gpu, "f16x2", 1, 1, 33, 16, 32, k=1, act=8, expect_ok=False)         # row GEMM accumulate: the bf16 splits only
    conv_case(lib, gpu, "bf16x2", 1, 1, 33, 16, 32, k=1, act=8, epi=5, expect_ok=False)
    conv_case(lib, gpu, "bf16x2", 1, 2, 34, 16, 32, k=1, act=16, expect_ok=False)       # stuffed: 3x3 only


def test_split_activation_format(lib, gpu):
    """f16x2 with ACT_SPLIT_IN / ACT_SPLIT_OUT on ragged images, Cout in {16, 48, 80}: the decoded split output against
    float64 (not only against its float32 twin), with pitches and the rows-per-wave variants."""
    from himo_amd.seflow.model import ACT_SPLIT_IN, ACT_SPLIT_OUT
    hints = (0, 0x1001, 0x1002, 0x1004, 0x1008, 0x100C)
    for i, (n, H, W, ci, co_) in enumerate([(2, 13, 37, 32, 16), (1, 5, 67, 16, 48), (1, 1, 33, 48, 80)]):
        for act in (ACT_SPLIT_IN, ACT_SPLIT_OUT, ACT_SPLIT_IN | ACT_SPLIT_OUT):
            conv_case(lib, gpu, "f16x2", n, H, W, ci, co_, epi=1, act=act, hints=hints, seed=500 + i)
        conv_case(lib, gpu, "f16x2", n, H, W, ci, co_, epi=0, act=3, x_pitch=ci + 16, y_pitch=co_ + 32, x_gap=64, y_gap=32,
                  seed=510 + i)
        conv_case(lib, gpu, "f16x2", n, H, W, ci, co_, stride=2, epi=1, act=ACT_SPLIT_IN | ACT_SPLIT_OUT, seed=520 + i)
        conv_case(lib, gpu, "f16x2", 1, 1, H * W, ci, co_, k=1, act=ACT_SPLIT_IN | ACT_SPLIT_OUT, hints=(0, 0x1001, 0x1002, 0x1004),
                  seed=530 + i)


def test_range_seen_word(lib, gpu):
    """d_range_seen: a split-output layer whose outputs all sit below 2^-7 leaves the word 0; one whose outputs all sit at
    2^-5 or above sets it to 1."""
    from himo_amd.seflow.model import ConvDesc, ACT_SPLIT_OUT
    n, H, W, ci, co_ = 1, 9, 35, 16, 32
    g = torch.Generator().manual_seed(7)
    x = torch.rand(n, H, W, ci, generator=g).to(gpu)
    w = (torch.rand(3, 3, ci, co_, generator=g) * 1e-5).to(gpu)            # |conv| <= 144 * 1e-5 = 1.4e-3
    pk = torch.empty(int(lib.himo_conv_packed_weight_bytes(3, ci, co_)), dtype=torch.uint8, device=gpu)
    assert lib.himo_conv_pack_weights_ex(w.data_ptr(), 3, ci, co_, 1, pk.data_ptr(), _stream()) == 0
    for bias_value, expect in ((2.0 ** -8, 0), (-2.0 ** -8, 0), (2.0 ** -5, 1), (-1.0, 1)):
        b = torch.full((co_,), bias_value, device=gpu)
        y = torch.empty(n, H, W, co_, device=gpu)
        word = torch.zeros(1, dtype=torch.int32, device=gpu)
        d = ConvDesc()
        d.x, d.x_batch_stride, d.x_pitch = x.data_ptr(), H * W * ci, ci
        d.w, d.bias, d.y, d.y_batch_stride, d.y_pitch = w.data_ptr(), b.data_ptr(), y.data_ptr(), H * W * co_, co_
        d.n, d.h, d.w_in, d.cin, d.cout, d.ksize, d.stride, d.epilogue = n, H, W, ci, co_, 3, 1, 0
        d.w_packed, d.packed_format, d.act_layout, d.range_seen = pk.data_ptr(), 1, ACT_SPLIT_OUT, word.data_ptr()
        assert lib.himo_conv2d(ctypes.byref(d), _stream()) == 0
        torch.cuda.synchronize()
        vals = split_decode(y.cpu().view(torch.int32)).abs()
        assert (vals.max() < 2 ** -7) if expect == 0 else (vals.min() >= 2 ** -5)
        assert int(word.item()) == expect, (bias_value, int(word.item()))


def test_large_output_offsets(lib, gpu):
    """A row GEMM whose output passes 2^29 floats (2 GiB): the 32-bit-offset epilogues must step aside.  Sampled rows
    (first / last 4096, 64k seeded random ones) against float64; the packed path may refuse instead."""
    from himo_amd.seflow.model import ConvDesc
    rows, ci, co_ = (1 << 22) + 37, 64, 128
    assert rows * co_ >= 1 << 29
    g = torch.Generator().manual_seed(11)
    w = torch.randn(1, 1, ci, co_, generator=g) / 8
    b = torch.randn(co_, generator=g) * 0.1
    sample = torch.cat([torch.arange(4096), torch.arange(rows - 4096, rows), torch.randint(0, rows, (65536,), generator=g)])
    x = torch.randn(rows, ci, device=gpu)
    wd, bd = w.to(gpu), b.to(gpu)
    xs = x[sample.to(gpu)].cpu()
    for arith in ("f32", "f16x2"):
        y = torch.full((rows * co_ + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=gpu)
        d = ConvDesc()
        d.x, d.x_batch_stride, d.x_pitch = x.data_ptr(), rows * ci, ci
        d.w, d.bias = wd.data_ptr(), bd.data_ptr()
        d.y, d.y_batch_stride, d.y_pitch = y.data_ptr() + 4 * GUARD, rows * co_, co_
        d.n, d.h, d.w_in, d.cin, d.cout, d.ksize, d.stride, d.epilogue = 1, 1, rows, ci, co_, 1, 1, 0
        pk = None
        if arith != "f32":
            pk = torch.empty(int(lib.himo_conv_packed_weight_bytes(1, ci, co_)), dtype=torch.uint8, device=gpu)
            assert lib.himo_conv_pack_weights_ex(wd.data_ptr(), 1, ci, co_, PACK[arith], pk.data_ptr(), _stream()) == 0
            d.w_packed, d.packed_format = pk.data_ptr(), PACK[arith]
        st = lib.himo_conv2d(ctypes.byref(d), _stream())
        torch.cuda.synchronize()
        if st != 0:
            assert arith != "f32", st
            FALLBACKS.append((f"large offsets {arith}", 0, st))      # convbf.hip: 32-bit image offsets
            assert bool(torch.all(y == NAN_BITS))
        else:
            assert bool(torch.all(y[:GUARD] == NAN_BITS)) and bool(torch.all(y[-GUARD:] == NAN_BITS))
            yv = y[GUARD:GUARD + rows * co_].view(torch.float32).view(rows, co_)
            got = yv[sample.to(gpu)].cpu()[None, None]
            xr = xs[None, None]
            ref = co.conv_ref(xr, w, b)
            bnd = co.bound(arith, xr, w, b, ref=ref)
            ref32 = co.conv_ref(xr, w, b, dtype=torch.float32)
            worst, rr = co.ok(got, ref["y"], bnd["y"], ref32["y"], arith, f"large offsets {arith}")
            _note(arith, worst, rr, f"large offsets {arith}")
            assert not bool(torch.isnan(yv).any()), "an output row was not written"
            del yv
        del y, pk
        torch.cuda.empty_cache()


def test_refusals_leave_the_output_untouched(lib, gpu):
    """conv.hip's admissibility rules and the header: each descriptor must be refused (HIMO_ERR_INVALID_ARGUMENT or
    HIMO_ERR_UNSUPPORTED) and the output bytes must stay as they were."""
    from himo_amd import _lib
    from himo_amd.seflow.model import ConvDesc, ACT_SPLIT_IN, ACT_SPLIT_OUT, ACT_STUFFED_2X
    H, W = 7, 9
    xb = torch.randn(4096 * 4, device=gpu)
    wb = torch.randn(9 * 64 * 64 + 64, device=gpu)
    bias = torch.zeros(64, device=gpu)
    y = torch.full((4096 * 8,), NAN_BITS, dtype=torch.int32, device=gpu)
    packs = {}

    def packed(fmt, k, ci, co_):
        if (fmt, k, ci, co_) not in packs:
            kk = min(k, 3)
            p = torch.empty(int(lib.himo_conv_packed_weight_bytes(kk, ci, co_)), dtype=torch.uint8, device=gpu)
            assert lib.himo_conv_pack_weights_ex(wb.data_ptr(), kk, ci, co_, fmt, p.data_ptr(), _stream()) == 0
            packs[(fmt, k, ci, co_)] = p
        return packs[(fmt, k, ci, co_)].data_ptr()

    def desc(ci=16, co_=32, k=3, stride=1, epi=0, x_pitch=None, x_off=0, w_off=0, fmt=None, act=0, h=H, aux=False, scale=True):
        d = ConvDesc()
        d.x, d.x_batch_stride, d.x_pitch = xb.data_ptr() + 4 * x_off, h * W * (x_pitch or ci), x_pitch or ci
        d.w, d.bias = wb.data_ptr() + 4 * w_off, bias.data_ptr()
        d.scale = d.shift = bias.data_ptr() if scale else None
        d.y, d.y_batch_stride, d.y_pitch = y.data_ptr(), h * W * co_, co_
        d.n, d.h, d.w_in, d.cin, d.cout, d.ksize, d.stride, d.epilogue = 1, h, W, ci, co_, k, stride, epi
        if aux:
            d.aux_in = d.aux_out = xb.data_ptr()
            d.aux_in_pitch = d.aux_out_pitch = co_
        if fmt is not None:
            d.w_packed, d.packed_format = packed(fmt, k, ci, co_), fmt
        d.act_layout = act
        return d

    table = {
        "cin % 4": desc(ci=18, x_pitch=20),
        "cout % 4": desc(co_=30),
        "x_pitch % 4": desc(x_pitch=18),
        "x misaligned": desc(x_off=1),
        "w misaligned": desc(w_off=2),
        "ksize 1, stride 2": desc(k=1, stride=2),
        "ksize 5": desc(k=5),
        "stride 3": desc(stride=3),
        "split in, cin % 16": desc(ci=20, fmt=1, act=ACT_SPLIT_IN),
        "split in, x_pitch % 16": desc(ci=16, x_pitch=20, fmt=1, act=ACT_SPLIT_IN),
        "split out, cout % 16": desc(co_=36, fmt=1, act=ACT_SPLIT_OUT),
        "split out, GELU epilogue": desc(fmt=1, act=ACT_SPLIT_OUT, epi=2),
        "split on bf16x3": desc(fmt=0, act=ACT_SPLIT_IN),
        "split on bf16x2": desc(fmt=2, act=ACT_SPLIT_OUT),
        "split without packed weights": desc(act=ACT_SPLIT_IN),
        "split 1x1 output only": desc(k=1, fmt=1, act=ACT_SPLIT_OUT),
        "stuffed, odd H": desc(fmt=2, act=ACT_STUFFED_2X, h=7),
        "GRU z|r without aux": desc(k=1, epi=3),
        "GRU q without aux": desc(k=1, epi=4),
        "ReLU mask without aux": desc(k=1, epi=6),
        "BN without scale": desc(epi=1, scale=False),
        "epilogue 7": desc(epi=7),
        "bf16x2, BN + GELU": desc(fmt=2, epi=1),
        "bf16x2 row GEMM, GELU": desc(k=1, fmt=2, epi=2),
    }
    for name, d in table.items():
        st = lib.himo_conv2d(ctypes.byref(d), _stream())
        torch.cuda.synchronize()
        assert st in (_lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED), (name, st)
        assert bool(torch.all(y == NAN_BITS)), f"{name}: refused but wrote"


def _up_case(lib, gpu, n, h, w, c, x_pitch, y_pitch, out_split, seed, x_gap=0, y_gap=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    x_bs, y_bs = h * w * x_pitch + x_gap, 4 * h * w * y_pitch + y_gap
    xg = Guarded(layout(n, n, x_bs, 0, h * w, x_pitch, c), gpu)
    xg.put(x)
    yg = Guarded(layout(n, n, y_bs, 0, 4 * h * w, y_pitch, c), gpu)
    st = lib.himo_upsample2x_batch_ex(n, xg.ptr, x_bs, x_pitch, h, w, c, yg.ptr, y_bs, y_pitch, out_split, _stream())
    torch.cuda.synchronize()
    assert st == 0, (n, h, w, c, st)
    assert yg.untouched_outside(), ("upsample wrote outside its view", n, h, w, c, x_pitch, y_pitch, out_split)
    got = split_decode(yg.words()) if out_split else yg.get().double()
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    # a convex combination of four inputs in float32: a few roundings of max |x|; the float32 source coordinate
    # s = o * (h - 1) / (2 h - 1) is off by up to 2 u s, times a slope of at most 2 max |x| per pixel (both axes); plus
    # the split's representation
    amax = x.abs().amax().item()
    bound = co.U * amax * (8 + 4 * (h - 1) + 4 * (w - 1)) + (torch.clamp(2.0 ** -22 * ref.abs(), min=2.0 ** -25) if out_split else 0)
    err = (got.reshape(ref.shape) - ref).abs()
    assert not bool(torch.isnan(err).any()), ("NaN: a read outside the input view", n, h, w, c)
    assert bool(torch.all(err <= bound)), ((n, h, w, c, x_pitch, y_pitch, out_split), float(err.max()))


def test_upsample_paths(lib, gpu):
    """The three paths of himo_upsample2x_batch_ex -- split-LDS (c in 64 / 128 / 256), split-row (other multiples of 16),
    plain float32 -- at h or w = 1, odd sizes, pitches wider than c, against float64 bilinear (align_corners)."""
    i = 0
    for (h, w) in ((1, 1), (1, 9), (7, 1), (5, 7), (17, 23), (2, 33)):
        for c, split in ((4, 0), (20, 0), (64, 0), (48, 1), (64, 1), (128, 1), (256, 1), (16, 1)):
            pad = 16 if split else 4 * (i % 3)
            _up_case(lib, gpu, 2, h, w, c, c + pad, c + 2 * pad, split, seed=i, x_gap=4 * (i % 2), y_gap=16 * (i % 2))
            i += 1
