"""The gradient checker itself (oracle/grad_oracle.py), on CPU: emulations of the kernels' arithmetic (float32 products and
sums, the bf16 terms of the split, partial sums merged in chunks) must pass its two-level check on the inputs of
tests/test_train_conformance_gpu.py, and each emulated WRONG kernel must fail it, at a small and at a large reduction
length.  This is what keeps the tolerances of the GPU matrix honest for whoever edits them."""
import numpy as np
import pytest
import torch

import conv_oracle as co
import grad_oracle as go

ARITHS = ["f32", "bf16x2"]
# (n_img, h, w, cin, cout, stride): reduction lengths N * Ho * Wo = 259, 252 (odd sizes, stride 2), 19 200, 18 560
CONV_SHAPES = {"small s1": (1, 7, 37, 12, 20, 1), "small s2 odd": (2, 17, 27, 12, 20, 2), "large s1": (5, 24, 160, 4, 12, 1),
               "large s2 odd": (4, 129, 143, 4, 12, 2)}
# (n, cin, cout): both sides of the 8-row and 256-row chunking
LINEAR_SHAPES = {"n=33": (33, 20, 36), "n=70001": (70_001, 12, 20)}


def _conv_data(shape, seed=0):
    n, h, w, cin, cout, s = shape
    return go.operands(seed + h + w, (n, h, w, cin), (n, go.out_size(h, s), go.out_size(w, s), cout))


def _emulate_dw(arith, x, dy, stride, chunk=256, kept=None):
    return go._fold_dw(go.emulate_product(arith, go.patches(x, stride).numpy(), dy.reshape(-1, dy.shape[-1]).numpy(), chunk, kept),
                       x.shape[-1])


def _verdict(arith, got, ref, bnd, ref32):
    worst, rr, report = go.check_cols(got, ref, bnd, ref32, arith)
    return worst <= 1.0 and rr <= go.R[arith], report


def _conv_verdict(arith, got, x, dy, stride, old=None):
    ref = go.conv3x3_dw(x, dy, stride)
    ref32 = go.conv3x3_dw(x, dy, stride, torch.float32)
    if old is not None:
        ref, ref32 = ref + old.double(), ref32 + old
    return _verdict(arith, got, ref, go.conv3x3_dw_bound(arith, x, dy, stride, old), ref32)


def _linear_verdict(arith, got, x, dz, old=None):
    ref, ref32 = go.linear_dw(x, dz), go.linear_dw(x, dz, torch.float32)
    if old is not None:
        ref, ref32 = ref + old.double(), ref32 + old
    return _verdict(arith, got, ref, go.linear_dw_bound(arith, x, dz, old), ref32)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", sorted(CONV_SHAPES))
def test_correct_conv_weight_gradient_passes(arith, name):
    shape = CONV_SHAPES[name]
    x, dy = _conv_data(shape)
    for chunk in (64, 256, 4096):                  # tile runs of the tiled kernels, the fallback's pixel chunks
        good, report = _conv_verdict(arith, _emulate_dw(arith, x, dy, shape[5], chunk), x, dy, shape[5])
        assert good, (chunk, report)
    old = torch.randn(3, 3, shape[3], shape[4], generator=torch.Generator().manual_seed(1))
    good, report = _conv_verdict(arith, old + _emulate_dw(arith, x, dy, shape[5]), x, dy, shape[5], old)
    assert good, report


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", sorted(LINEAR_SHAPES))
def test_correct_linear_weight_gradient_passes(arith, name):
    n, cin, cout = LINEAR_SHAPES[name]
    x, dz = go.operands(n, (n, cin), (n, cout))
    for chunk in (256, 2048):                       # wgrad_rows_per_block: 256 rows or more per block
        good, report = _linear_verdict(arith, go.emulate_product(arith, x.numpy(), dz.numpy(), chunk), x, dz)
        assert good, (chunk, report)
    old = torch.randn(cin, cout, generator=torch.Generator().manual_seed(2))
    good, report = _linear_verdict(arith, old + go.emulate_product(arith, x.numpy(), dz.numpy()), x, dz, old)
    assert good, report


@pytest.mark.parametrize("groups", [2, 8])
def test_correct_column_sums_pass(groups):
    """the bias gradients and himo_colsum: both kernels' summation order at every (n, cout) of the GPU matrix, alone and
    accumulated onto an old value, against the sequential float32 twin"""
    for n in (1, 7, 33, 255, 257, 4097, 16384, 70_001):
        for cout in (4, 20, 36, 64, 130, 256):
            _, z = go.operands(n + cout, (1, 1), (n, cout))
            old = torch.randn(cout, generator=torch.Generator().manual_seed(n))
            got = go.emulate_colsum(z.numpy(), groups)
            good, report = _verdict("f32", got, go.colsum(z), go.colsum_bound(z), go.colsum(z, torch.float32))
            assert good, (n, cout, report)
            good, report = _verdict("f32", old + got, go.colsum(z) + old.double(), go.colsum_bound(z, old), go.colsum(z, torch.float32) + old)
            assert good, (n, cout, report)


def test_the_aggregate_level_needs_a_sample():
    """four outputs are no statistic: the same correct column sums, ratio taken over 4 columns of which one dominates, pass
    or miss R by chance -- check_cols asserts the aggregate level from 32 outputs on and scales every column alike"""
    ratios = []
    for seed in range(40):
        _, z = go.operands(seed, (1, 1), (255, 4))
        ratios.append(co.check(go.emulate_colsum(z.numpy(), 8), go.colsum(z), go.colsum_bound(z), go.colsum(z, torch.float32), "f32")[1])
        assert go.check_cols(go.emulate_colsum(z.numpy(), 8), go.colsum(z), go.colsum_bound(z), go.colsum(z, torch.float32), "f32")[1] == 0.0
    assert max(ratios) > go.R["f32"] > min(ratios)


def test_dx_is_the_convolution_of_the_stuffed_gradient_with_the_flipped_kernel():
    """conv3x3_dx (a transposed convolution) against its definition, stride 1 and 2, odd sizes -- and against autograd."""
    g = torch.Generator().manual_seed(3)
    for (h, w, s) in ((6, 8, 2), (7, 9, 2), (1, 5, 2), (5, 4, 1)):
        ho, wo = go.out_size(h, s), go.out_size(w, s)
        dy = torch.randn(2, ho, wo, 5, generator=g).double()
        wt = torch.randn(3, 3, 3, 5, generator=g).double()
        dx = go.conv3x3_dx(dy, wt, s, h, w)
        z = go.zero_stuff2x(dy)[:, :h, :w] if s == 2 else dy
        if s == 2 and (z.shape[1] < h or z.shape[2] < w):
            continue
        assert torch.allclose(dx, co.conv(z, go.weight_flip(wt)), atol=1e-12)
        x = torch.randn(2, h, w, 3, generator=g).double().requires_grad_(True)
        (co.conv(x, wt, s) * dy).sum().backward()
        assert torch.allclose(dx, x.grad, atol=1e-12)
        assert torch.allclose(go.conv3x3_dw(x.detach(), dy, s), torch.autograd.grad((co.conv(x.detach(), wt.requires_grad_(True), s) * dy).sum(), wt)[0],
                              atol=1e-12)


def test_upsample_adjoint_is_the_transpose_of_the_interpolation():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    for (h, w) in ((1, 1), (1, 7), (5, 1), (5, 7), (8, 3)):
        x = torch.randn(h, w, 4, generator=g).double().requires_grad_(True)
        dy = torch.randn(2 * h, 2 * w, 4, generator=g).double()
        up = F.interpolate(x.permute(2, 0, 1)[None], scale_factor=2, mode="bilinear", align_corners=True)[0].permute(1, 2, 0)
        (up * dy).sum().backward()
        assert torch.allclose(go.upsample2x_adjoint(dy), x.grad, atol=1e-12)
        # the float32 twin sits inside the bound
        got = go.upsample2x_adjoint(dy.float(), torch.float32)
        assert bool(torch.all((got.double() - go.upsample2x_adjoint(dy.float())).abs() <= go.upsample2x_adjoint_bound(dy.float())))


def _wrong_conv():
    """name -> (arith, stride class, builder(x, dy, stride) -> wrong dW)"""
    def halo_row(x, dy, s):                                 # the ky = 2 taps of output row 0 (input row 1) are missing
        p = go.patches(x, s).reshape(x.shape[0], dy.shape[1], dy.shape[2], x.shape[-1], 3, 3).clone()
        p[:, 0, :, :, 2, :] = 0
        return go._fold_dw(go.emulate_product("f32", p.reshape(-1, x.shape[-1] * 9).numpy(), dy.reshape(-1, dy.shape[-1]).numpy()), x.shape[-1])

    def halo_col(x, dy, s):                                 # the kx = 2 taps of output column 0 (input column 1) are missing
        p = go.patches(x, s).reshape(x.shape[0], dy.shape[1], dy.shape[2], x.shape[-1], 3, 3).clone()
        p[:, :, 0, :, :, 2] = 0
        return go._fold_dw(go.emulate_product("f32", p.reshape(-1, x.shape[-1] * 9).numpy(), dy.reshape(-1, dy.shape[-1]).numpy()), x.shape[-1])

    def last_chunk(x, dy, s):                               # the last (ragged) pixel chunk is never summed
        a, b = go.patches(x, s).numpy(), dy.reshape(-1, dy.shape[-1]).numpy()
        keep = (a.shape[0] - 1) // 256 * 256
        return go._fold_dw(go.emulate_product("f32", a[:keep], b[:keep]), x.shape[-1])

    def cin_tail(x, dy, s):
        dw = _emulate_dw("f32", x, dy, s)
        dw[:, :, x.shape[-1] // 8 * 8:, :] = 0              # the ragged input-channel tail (cin % 8 here, cin % 128 on the device)
        return dw

    def cout_tail(x, dy, s):
        dw = _emulate_dw("bf16x2", x, dy, s)
        dw[..., dy.shape[-1] // 8 * 8:] = 0
        return dw

    def cross(x, dy, s):
        return _emulate_dw("bf16x2", x, dy, s, kept=[(0, 0), (1, 0)])

    def odd_sampling(x, dy, s):
        n, ho, wo = dy.shape[:3]
        p = go.patches(x, 1).reshape(n, x.shape[1], x.shape[2], -1)[:, 1::2, 1::2]
        pp = torch.zeros(n, ho, wo, p.shape[-1])
        pp[:, :p.shape[1], :p.shape[2]] = p
        return go._fold_dw(go.emulate_product("f32", pp.reshape(-1, p.shape[-1]).numpy(), dy.reshape(-1, dy.shape[-1]).numpy()), x.shape[-1])

    def last_row(x, dy, s):
        d = dy.clone()
        d[:, -1] = 0
        return _emulate_dw("f32", x, d, s)

    def last_col(x, dy, s):
        d = dy.clone()
        d[:, :, -1] = 0
        return _emulate_dw("f32", x, d, s)

    return {"halo row missing": ("f32", 1, halo_row), "halo column missing": ("f32", 1, halo_col),
            "last pixel chunk dropped": ("f32", 1, last_chunk), "cin tail zeroed": ("f32", 1, cin_tail),
            "cout tail zeroed": ("bf16x2", 1, cout_tail), "h * m dropped": ("bf16x2", 1, cross),
            "stride 2 at odd pixels": ("f32", 2, odd_sampling), "odd H: last output row ignored": ("f32", 2, last_row),
            "odd W: last output column ignored": ("f32", 2, last_col)}


WRONG_CONV = _wrong_conv()


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("name", sorted(WRONG_CONV))
def test_wrong_conv_weight_gradient_is_rejected(name, size):
    arith, stride, make = WRONG_CONV[name]
    shape = CONV_SHAPES[f"{size} s1" if stride == 1 else f"{size} s2 odd"]
    x, dy = _conv_data(shape, seed=5)
    good, report = _conv_verdict(arith, make(x, dy, stride), x, dy, stride)
    assert not good, f"{name} passed the check: {report}"


@pytest.mark.parametrize("name", sorted(LINEAR_SHAPES))
def test_wrong_linear_weight_gradient_is_rejected(name):
    n, cin, cout = LINEAR_SHAPES[name]
    x, dz = go.operands(n + 1, (n, cin), (n, cout))
    xa, za = x.numpy(), dz.numpy()
    keep = n - n % 8
    wrong = {"last n % 8 rows dropped": ("f32", go.emulate_product("f32", xa[:keep], za[:keep])),
             "m * h dropped": ("bf16x2", go.emulate_product("bf16x2", xa, za, kept=[(0, 0), (0, 1)]))}
    t = go.emulate_product("f32", xa, za)
    t[cin // 8 * 8:] = 0
    wrong["cin tail zeroed"] = ("f32", t)
    t = go.emulate_product("bf16x2", xa, za)
    t[:, cout // 8 * 8:] = 0
    wrong["cout tail zeroed"] = ("bf16x2", t)
    for key, (arith, got) in wrong.items():
        good, report = _linear_verdict(arith, got, x, dz)
        assert not good, f"{key} passed the check: {report}"
    old = torch.randn(cin, cout, generator=torch.Generator().manual_seed(6))
    good, report = _linear_verdict("f32", go.emulate_product("f32", xa, za), x, dz, old)       # overwrote instead of adding
    assert not good, f"accumulate that overwrites passed the check: {report}"


def test_wrong_bias_gradient_and_wrong_upsample_adjoint_are_rejected():
    _, dy = _conv_data(CONV_SHAPES["small s2 odd"], seed=7)
    ref, bnd = go.colsum(dy), go.colsum_bound(dy)
    worst, _, report = go.check_cols(go.colsum(dy[:1], torch.float32), ref, bnd, go.colsum(dy, torch.float32), "f32")
    assert worst > 1.0, f"the bias gradient of the first image only passed: {report}"
    g = torch.Generator().manual_seed(8)
    for (h, w) in ((5, 9), (16, 24)):
        d = torch.randn(2 * h, 2 * w, 4, generator=g)
        wrong = go.upsample2x_adjoint(d, torch.float32, ratio_from=(w, h))
        err = (wrong.double() - go.upsample2x_adjoint(d)).abs()
        assert not bool(torch.all(err <= go.upsample2x_adjoint_bound(d))), (h, w)


def test_elementwise_float32_twins_pass_and_wrong_formulas_fail():
    """every element-wise kernel: the float32 twin inside the bound and inside R_ELEM, on inputs that reach the saturated ends
    of sigmoid / tanh / GELU; a formula with one factor missing outside it"""
    g = torch.Generator().manual_seed(9)
    n = 65
    rn = lambda *s: torch.randn(*s, generator=g)
    sat = lambda t, a: torch.where(torch.rand(t.shape, generator=g) < 0.1, t.sign() * a, t)
    hx = rn(n, 192)
    z, r, q = torch.rand(n, 128, generator=g), torch.rand(n, 128, generator=g), torch.tanh(rn(n, 128))
    cases = {
        "gru_gates1": dict(pre=sat(rn(n, 256) * 3, 30.0), hx=hx),
        "gru_gates2": dict(pre=sat(rn(n, 128) * 3, 20.0), z=z, hx=hx),
        "gru_bwd1": dict(dh_next=rn(n, 128), z=z, q=q, hx=hx),
        "gru_bwd2": dict(d_rhx=rn(n, 192), hx=hx, z=z, r=r, dz=rn(n, 128), dhp=rn(n, 128), dx=rn(n, 64)),
        "gru_bwd3": dict(d_hx=rn(n, 192), dhp=rn(n, 128), dx=rn(n, 64)),
        "affine_gelu_fwd": dict(x=sat(rn(n, 20) * 2, 10.0), scale=torch.rand(20, generator=g) + 0.5, shift=rn(20) * 0.1),
        "affine_gelu_bwd": dict(dy=rn(n, 20), pre=sat(rn(n, 20) * 2, 10.0), scale=torch.rand(20, generator=g) + 0.5),
        "add2d": dict(y=rn(n, 20), b=rn(n, 20)),
        "rows_add": dict(a=rn(n, 3), b=rn(n, 3), b_scale=-1.5),
    }
    for name, args in cases.items():
        ref, ref32, bnd = go.elementwise(name, **args), go.elementwise(name, torch.float32, **args), go.elementwise_bound(name, **args)
        for key in ref:
            worst, rr, report = co.check(ref32[key], ref[key], bnd[key], ref32[key], "f32", f"{name} {key}", limit=go.R_ELEM)
            assert worst <= 1.0 and rr <= go.R_ELEM, report
    a = cases["gru_bwd1"]
    wrong = a["dh_next"] * a["z"] * (1 - a["q"])                                  # 1 - q instead of 1 - q^2
    assert co.check(wrong, go.elementwise("gru_bwd1", **a)["daq"], go.elementwise_bound("gru_bwd1", **a)["daq"])[0] > 1
    a = cases["affine_gelu_bwd"]
    wrong = a["dy"] * go._gelu_grad(a["pre"])                                     # the scale factor forgotten
    assert co.check(wrong, go.elementwise("affine_gelu_bwd", **a)["dx"], go.elementwise_bound("affine_gelu_bwd", **a)["dx"])[0] > 1
