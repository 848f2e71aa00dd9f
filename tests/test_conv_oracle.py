"""The convolution checker itself (oracle/conv_oracle.py), on CPU: the split arithmetics of csrc/bf16x3.h emulated in
float32 must pass its two-level check, and each emulated WRONG kernel must fail it, at a small and at a large K.  This is
what keeps the tolerances of tests/test_conv_conformance_gpu.py honest for whoever edits them."""
import numpy as np
import pytest
import torch

import conv_oracle as co


def _data(n, h, w, cin, cout, seed, k=3, wscale=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g)
    K = k * k * cin
    w_ = torch.randn(k, k, cin, cout, generator=g) * (wscale if wscale is not None else 1.0 / np.sqrt(K))
    b = torch.randn(cout, generator=g) * 0.1
    return x, w_, b


def emulate(arith, x, w, stride=1, kept=None, weight_scale=None):
    """The accumulator of ``arith``: every kept product of split terms convolved in float32 (exact products, float32
    sums), the partial results added in float32."""
    kept = co.KEPT[arith] if kept is None else kept
    xs = co.split_terms(arith, x.numpy())
    if weight_scale is None:
        ws = co.split_terms(arith, w.numpy(), weights=True)
    else:                                       # a wrong packing scale (f16x2)
        s = np.float32(weight_scale)
        ww = w.numpy() * s
        hh = ww.astype(np.float16).astype(np.float32)
        ws = [hh / s, (ww - hh).astype(np.float16).astype(np.float32) / s]
    acc = None
    for i, j in kept:
        t = co.conv(torch.from_numpy(xs[i]), torch.from_numpy(ws[j]), stride)
        acc = t if acc is None else acc + t
    return acc


def _verdict(arith, x, w, b, acc, stride=1):
    ref = co.conv_ref(x, w, b, stride)
    bnd = co.bound(arith, x, w, b, stride, ref=ref)
    ref32 = co.conv_ref(x, w, b, stride, dtype=torch.float32)["y"]
    worst, rr, report = co.check(acc + b, ref["y"], bnd["y"], ref32, arith)
    return worst <= 1.0 and rr <= co.R[arith], report


SHAPES = [(2, 5, 7, 20, 12), (1, 6, 6, 768, 8), (1, 5, 4, 772, 12)]      # K = 180, 9 * 768, 9 * 772 (ragged Cin)


@pytest.mark.parametrize("arith", ["f32", "bf16x3", "f16x2", "bf16x2"])
@pytest.mark.parametrize("shape", SHAPES)
def test_correct_arithmetic_passes(arith, shape):
    x, w, b = _data(*shape, seed=sum(shape))
    good, report = _verdict(arith, x, w, b, emulate(arith, x, w))
    assert good, report


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("epilogue", [1, 2, 3, 4, 5, 6])
def test_correct_epilogues_pass(epilogue, stride):
    """The epilogue budget: the float32 epilogue (torch's own erf / sigmoid / tanh) on the emulated accumulators."""
    x, w, b = _data(2, 9, 11, 36, 20, seed=epilogue)
    g = torch.Generator().manual_seed(100 + epilogue)
    scale, shift = torch.rand(20, generator=g) + 0.5, torch.randn(20, generator=g) * 0.1
    ho, wo = (5, 6) if stride == 2 else (9, 11)
    aux_c = 10 if epilogue == 3 else 20
    aux_in = torch.randn(2, ho, wo, aux_c, generator=g)
    if epilogue == 4:
        aux_in = torch.rand(2, ho, wo, aux_c, generator=g)
    aux_out = torch.randn(2, ho, wo, aux_c, generator=g)
    for arith in ("f32", "bf16x3", "f16x2"):
        acc = emulate(arith, x, w, stride)
        bb = None if epilogue == 6 else b
        got = co.epilogue_ref(acc, bb, epilogue, scale, shift, aux_in, aux_out, dtype=torch.float32)
        ref = co.conv_ref(x, w, bb, stride, epilogue, scale, shift, aux_in, aux_out)
        bnd = co.bound(arith, x, w, bb, stride, epilogue, scale, shift, aux_in, aux_out, ref=ref)
        ref32 = co.conv_ref(x, w, bb, stride, epilogue, scale, shift, aux_in, aux_out, dtype=torch.float32)
        for key in ("y", "aux_out"):
            if ref[key] is not None:
                worst, rr, report = co.check(got[key], ref[key], bnd[key], ref32[key], arith, f"epilogue {epilogue} {key}")
                assert worst <= 1.0 and rr <= co.R[arith], report


def _wrong_answers():
    """name -> (arith, shape-independent builder(x, w, stride) -> wrong accumulator, stride)"""
    def drop_ha_lb(x, w, s):
        return emulate("f16x2", x, w, s, kept=[(0, 0), (1, 0)])

    def unscaled_weights(x, w, s):
        return emulate("f16x2", x, w, s, weight_scale=1.0)

    def tail_zero(x, w, s):
        acc = emulate("bf16x3", x, w, s)
        acc[..., -4:] = 0
        return acc

    def first_row_no_halo(x, w, s):
        acc = emulate("bf16x3", x, w, s)
        xx = x.clone()
        xx[:, 1] = 0
        acc[:, 0] = emulate("bf16x3", xx, w, s)[:, 0]
        return acc

    def last_row_no_halo(x, w, s):
        acc = emulate("bf16x3", x, w, s)
        xx = x.clone()
        xx[:, -2] = 0
        acc[:, -1] = emulate("bf16x3", xx, w, s)[:, -1]
        return acc

    def ragged_tail_ignored(x, w, s):
        xx = x.clone()
        xx[..., x.shape[-1] // 16 * 16:] = 0
        return emulate("f32", xx, w, s)

    def odd_sampling(x, w, s):
        return emulate("f32", x, w, 1)[:, 1::2, 1::2]

    return {"ha*lb dropped": ("f16x2", drop_ha_lb, 1), "weights packed without 2^6": ("f16x2", unscaled_weights, 1),
            "last 4 channels zero": ("bf16x3", tail_zero, 1), "first row without halo": ("bf16x3", first_row_no_halo, 1),
            "last row without halo": ("bf16x3", last_row_no_halo, 1), "ragged Cin slab ignored": ("f32", ragged_tail_ignored, 1),
            "stride 2 at odd pixels": ("f32", odd_sampling, 2)}


WRONG = _wrong_answers()


@pytest.mark.parametrize("shape", [(2, 6, 8, 20, 12), (1, 6, 6, 772, 8)])      # K = 180 and 9 * 772, ragged Cin, even H / W
@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_arithmetic_is_rejected(name, shape):
    arith, make, stride = WRONG[name]
    # weights of the network's magnitude (~0.03); the missing 2^6 weight scale costs precision only where the weights' low
    # fp16 halves fall on the subnormal floor (2^-25 absolute), and is visible above the float32 accumulation error of
    # K = 9 * 772 only for small weights: 1e-3 (a layer behind a small BatchNorm gain, test_parity_hardening_gpu.py)
    x, w, b = _data(*shape, seed=7, wscale=1e-3 if "2^6" in name else 0.03)
    good, report = _verdict(arith, x, w, b, make(x, w, stride), stride)
    assert not good, f"{name} passed the check: {report}"


def test_report_names_the_worst_element():
    x, w, b = _data(1, 6, 8, 20, 12, seed=3)
    acc = emulate("f32", x, w)
    acc[0, 5, 3, 10] += 1.0
    ref = co.conv_ref(x, w, b)
    bnd = co.bound("f32", x, w, b, ref=ref)
    worst, rr, report = co.check(acc + b, ref["y"], bnd["y"], None, "f32", "probe")
    assert worst > 1 and "(0, 5, 3, 10)" in report and "border row" in report and "tail channel" in report
    # a NaN is never within a bound
    acc = emulate("f32", x, w)
    acc[0, 2, 2, 2] = float("nan")
    assert co.check(acc + b, ref["y"], bnd["y"], None, "f32")[0] > 1


def test_splits_match_their_definitions():
    """bf16 round-to-nearest-even by bit masking, the three-term residual, the f16x2 floors (bf16x3.h)."""
    a = np.array([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -3.14159265, 1e-30, 0.1], np.float32)
    h = co.bf16_rne(a)
    assert h[1] == 1.0 and h[2] == 1.0 + 2 ** -6           # ties to even
    x = np.random.default_rng(0).standard_normal(10000).astype(np.float32)
    t3 = co.split_terms("bf16x3", x)
    assert np.all(np.abs(x.astype(np.float64) - sum(t.astype(np.float64) for t in t3)) <= 2.0 ** -24 * np.abs(x))
    t2 = co.split_terms("f16x2", x)
    res = np.abs(x.astype(np.float64) - sum(t.astype(np.float64) for t in t2))
    assert np.all(res <= np.maximum(2.0 ** -25, 2.0 ** -22 * np.abs(x)))
    w2 = co.split_terms("f16x2", x * 0.01, weights=True)
    resw = np.abs((x * 0.01).astype(np.float64) - sum(t.astype(np.float64) for t in w2))
    assert np.all(resw <= np.maximum(2.0 ** -31, 2.0 ** -22 * np.abs(x * 0.01)))
