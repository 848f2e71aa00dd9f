"""Float64 reference and worst-case error model of ``himo_conv2d`` (include/himo_amd.h; csrc/conv*.hip).  CPU only.

Every map here is NHWC: x [N, H, W, Cin], w [k, k, Cin, Cout] (the library's weight layout), outputs [N, Ho, Wo, Cout];
3x3 layers pad 1, stride 1 | 2 (Ho = ceil(H / stride)); 1x1 layers are row GEMMs.

The error model (``bound``) is a per-output WORST case: it never flakes, but at K = 9 * 256 its accumulation term is
hundreds of times the typical error, so a systematic loss (a dropped cross term, an unscaled weight split) can hide under
it.  ``check`` therefore asserts a second, aggregate level: the RMS error against the float64 reference must stay
within ``R[arith]`` times the RMS error of the same operation done in float32 (CPU torch), plus a small floor.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                    # float32 unit roundoff (round to nearest even)
ARITHS = ("f32", "bf16x3", "f16x2", "bf16x2")
F16_WEIGHT_SCALE = 64.0           # bf16x3.h kF16WeightScale: f16x2 weights are packed x 2^6

# Aggregate level: rms(got - ref) <= R * rms(ref32 - ref) + floor.  Largest ratios met by the conformance matrix on an
# MI355X (tests/test_conv_conformance_gpu.py, single-row GEMMs, where the float32 reference's own error is smallest):
# f32 1.57, bf16x3 1.03, f16x2 1.26, bf16x2 54.7.
# f32: the float32 MFMA rounds every product and every partial sum once -- the arithmetic of the float32 CPU
#   reference, summed in another order: the ratio sits near 1, 2 leaves room for an unlucky order on a small case.
# bf16x3: three-term operands (2^-24 relative residual) and six kept products (dropped terms <= 2^-24 relative) add
#   at most about one float32 rounding per product to the float32 accumulation: ratio near 1, R = 2.
# f16x2: below |x| = 1/4 the low fp16 half is subnormal, an activation keeps 2^-25 ABSOLUTE, which for the N(0, 1)
#   activations used here is up to a few float32 roundings of the product; la * lb (2^-22) is dropped.  Started at 8,
#   tightened to 4 after the first run (observed 1.26); weights packed without their 2^6 scale give 11-24 on 1e-3
#   weights (tests/test_conv_oracle.py).
# bf16x2: 16 significant bits per operand, 2^-17 relative against float32's 2^-24: at most 2^7 = 128 times the float32
#   error per product, less once the float32 accumulation error grows with K.  R = 128.
R = {"f32": 2.0, "bf16x3": 2.0, "f16x2": 4.0, "bf16x2": 128.0}


# ---- reference ------------------------------------------------------------------------------------------------------
def conv(x, w, stride=1):
    """Plain convolution of NHWC ``x`` with [k][k][Cin][Cout] ``w`` in the dtype of the inputs (pad k // 2)."""
    k = w.shape[0]
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=stride, padding=k // 2)
    return y.permute(0, 2, 3, 1)


def _gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def conv_ref(x, w, b=None, stride=1, epilogue=0, scale=None, shift=None, aux_in=None, aux_out=None, dtype=torch.float64):
    """The header's epilogues (include/himo_amd.h HIMO_EPI_*) on conv(x, w) in ``dtype``.

    Returns dict(v=pre-activation acc + bias, y=output or None, aux_out=updated aux_out or None).  aux_in / aux_out are
    [N, Ho, Wo, C] (GRU z|r: C = Cout / 2, GRU q / ReLU-mask: C = Cout).  GRU z|r writes y only in columns [0, Cout / 2);
    GRU q writes only aux_out."""
    x, w = torch.as_tensor(x).to(dtype), torch.as_tensor(w).to(dtype)
    return epilogue_ref(conv(x, w, stride), b, epilogue, scale, shift, aux_in, aux_out, dtype)


def epilogue_ref(acc, b=None, epilogue=0, scale=None, shift=None, aux_in=None, aux_out=None, dtype=torch.float64):
    """The epilogue alone on an accumulator ``acc`` (see conv_ref)."""
    t = lambda a: None if a is None else torch.as_tensor(a).to(dtype)
    acc, b, scale, shift, aux_in, aux_out = map(t, (acc, b, scale, shift, aux_in, aux_out))
    v = acc if (b is None or epilogue == 6) else acc + b
    y, ao = None, None
    if epilogue == 0:
        y = v
    elif epilogue == 1:
        y = _gelu(v * scale + shift)
    elif epilogue == 2:
        y = _gelu(v)
    elif epilogue == 3:
        half = v.shape[-1] // 2
        g = torch.sigmoid(v)
        y = g[..., :half]
        ao = g[..., half:] * aux_in
    elif epilogue == 4:
        ao = (1 - aux_in) * aux_out + aux_in * torch.tanh(v)
    elif epilogue == 5:
        y = torch.clamp(v, min=0)
    elif epilogue == 6:
        y = torch.where(aux_in > 0, v, torch.zeros_like(v))
    else:
        raise ValueError(epilogue)
    return dict(v=v, y=y, aux_out=ao)


def mag(x, w, stride=1):
    """conv(|x|, |w|) in float64: the scale the rounding errors of one output are relative to."""
    return conv(torch.as_tensor(x).double().abs(), torch.as_tensor(w).double().abs(), stride)


# ---- operand splits (CPU emulations of csrc/bf16x3.h) -------------------------------------------------------------
def bf16_rne(a):
    """float32 -> nearest bf16 (ties to even), returned as float32 (bf16x3.h bf16_rne_bits)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def split_terms(arith, a, weights=False):
    """The float32 terms a kernel holds for operand ``a`` (each exactly representable; their sum approximates a).
    f16x2 weights are returned UNscaled (packed x 2^6 by the kernel, product rescaled exactly)."""
    a = np.asarray(a, dtype=np.float32)
    if arith == "f32":
        return [a]
    if arith in ("bf16x3", "bf16x2"):
        h = bf16_rne(a)
        m = bf16_rne(a - h)
        if arith == "bf16x2":
            return [h, m]
        return [h, m, bf16_rne((a - h) - m)]
    if arith == "f16x2":
        s = np.float32(F16_WEIGHT_SCALE if weights else 1.0)
        aa = a * s
        h = aa.astype(np.float16).astype(np.float32)
        l = (aa - h).astype(np.float16).astype(np.float32)
        return [h / s, l / s]
    raise ValueError(arith)


# kept cross products (i, j) = term i of the activation x term j of the weight
KEPT = {"f32": [(0, 0)],
        "bf16x3": [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)],
        "f16x2": [(0, 0), (0, 1), (1, 0)],
        "bf16x2": [(0, 0), (0, 1), (1, 0)]}


def operand_bound(arith, x, w, stride=1):
    """Per-output worst case of |acc - conv(x, w)| for the accumulator of ``arith`` (float64, no bias).

    f32 (v_mfma_f32_32x32x2_f32): each product rounds once, each of the K additions once:
        (K + 2) u mag.
    split formats (bf16x3 split3, f16x2 split2, bf16x2 HIMO_PACK_BF16X2): every kept product of two terms is exact in
    float32 (8 x 8, 11 x 11 or 8 x 8 significant bits), so the error is
      * operand residuals, elementwise and exact:  conv(dx, |w|) + conv(|x|, dw) + conv(dx, dw),  d = |a - sum(terms)|
        (f16x2: dx is the 2^-25 absolute / 2^-23 relative of the split, dw that of the 2^6-scaled weight split);
      * the dropped products, exactly:  sum over dropped (i, j) of conv(|x_i|, |w_j|);
      * float32 accumulation of P * K terms (P kept products):  (P K + 2) u conv(sum|x_i|, sum|w_j|).
    """
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    K = w.shape[0] * w.shape[1] * w.shape[2]
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    if arith == "f32":
        return (K + 2) * U * mag(x, w, stride)
    xs, ws = split_terms(arith, x), split_terms(arith, w, weights=True)
    dx = np.abs(x.astype(np.float64) - sum(t.astype(np.float64) for t in xs))
    dw = np.abs(w.astype(np.float64) - sum(t.astype(np.float64) for t in ws))
    ax, aw = np.abs(x).astype(np.float64), np.abs(w).astype(np.float64)
    b = conv(d(dx), d(aw), stride) + conv(d(ax), d(dw), stride) + conv(d(dx), d(dw), stride)
    kept = KEPT[arith]
    for i in range(len(xs)):
        for j in range(len(ws)):
            if (i, j) not in kept:
                b = b + conv(d(np.abs(xs[i])), d(np.abs(ws[j])), stride)
    sx = sum(np.abs(t).astype(np.float64) for t in xs)
    sw = sum(np.abs(t).astype(np.float64) for t in ws)
    return b + (len(kept) * K + 2) * U * conv(d(sx), d(sw), stride)


GELU_SLOPE = 1.129                 # max over t of |d gelu / dt| = Phi(t) + t phi(t)
ERF_AS = 1.5e-7                    # Abramowitz & Stegun 7.1.26 (conv_common.h gelu_exact)


def bound(arith, x, w, b=None, stride=1, epilogue=0, scale=None, shift=None, aux_in=None, aux_out=None, ref=None,
          split_out=False):
    """Per-output worst-case error of y (and of aux_out for the GRU epilogues) -> dict(y=..., aux_out=...).

    dv = operand_bound + u |v| (the bias add).  Epilogue budget on top:
      BN + GELU: t = fma(acc, k sc, fma(b, sc, sh)) -> dt = |sc| dv + u (|b sc + sh| + |t|);
      GELU: slope <= 1.129 times dt, plus the A&S erf (1.5e-7) and the hardware exp2 / rcp (~16 u on erf) scaled by |t| / 2,
            plus 4 u |y| of float32 arithmetic;
      sigmoid (GRU z|r): slope 1/4; hardware exp of -v is good to u (6 + |v|) relative (argument rounding grows with |v|);
      tanh (GRU q): slope 1; 2 e u (4 + 2 |v|) + 4 u |tanh|, e = exp(-2 |v|); the blend (1 - z) h + z q adds
            3 u (|(1 - z) h| + |z q|);
      ReLU, ReLU-mask: slope 1, no evaluation error.
    split_out: y is decoded from the split activation format (fp16 h + l): + max(2^-25, 2^-22 |y|)."""
    if ref is None:
        ref = conv_ref(x, w, b, stride, epilogue, scale, shift, aux_in, aux_out)
    v = ref["v"]
    dv = operand_bound(arith, x, w, stride) + U * v.abs()
    out = dict(y=None, aux_out=None)
    if epilogue in (0, 5, 6):
        by = dv
    elif epilogue in (1, 2):
        if epilogue == 1:
            sc, sh = torch.as_tensor(scale).double(), torch.as_tensor(shift).double()
            bb = torch.zeros_like(sc) if b is None else torch.as_tensor(b).double()
            t = v * sc + sh
            dt = sc.abs() * dv + U * ((bb * sc + sh).abs() + t.abs())
        else:
            t, dt = v, dv
        by = GELU_SLOPE * dt + 0.5 * (t.abs() + dt) * (ERF_AS + 16 * U) + 4 * U * ref["y"].abs() + 1e-37
    elif epilogue == 3:
        half = v.shape[-1] // 2
        g = torch.sigmoid(v)
        bg = 0.25 * dv + g * U * (6 + v.abs())
        by = bg[..., :half]
        h = torch.as_tensor(aux_in).double()
        out["aux_out"] = h.abs() * bg[..., half:] + U * ref["aux_out"].abs()
    elif epilogue == 4:
        z, h = torch.as_tensor(aux_in).double(), torch.as_tensor(aux_out).double()
        q = torch.tanh(v)
        e = torch.exp(-2 * v.abs())
        bq = dv + 2 * e * U * (4 + 2 * v.abs()) + 4 * U * q.abs()
        out["aux_out"] = z.abs() * bq + 3 * U * (((1 - z) * h).abs() + (z * q).abs())
        return out
    else:
        raise ValueError(epilogue)
    if split_out:
        by = by + torch.clamp(2.0 ** -22 * ref["y"].abs(), min=2.0 ** -25)
    out["y"] = by
    return out


# ---- the two-level check ---------------------------------------------------------------------------------------------
def rms(a):
    a = torch.as_tensor(a).double()
    return float(a.pow(2).mean().sqrt()) if a.numel() else 0.0


def check(got, ref, bnd, ref32=None, arith="f32", case="", floor=None, limit=None):
    """Worst err / bound and a readable report.

    got, ref, bnd: [..., H, W, C] (NHWC; ref float64).  ref32: the same operation in float32 (CPU torch) or None.
    Returns (worst, rms_ratio, report); the caller asserts worst <= 1 and rms_ratio <= R[arith]
    (``ok(...)`` does both).  rms_ratio = rms(got - ref) / (rms(ref32 - ref) + floor), floor = 2^-24 rms(ref) unless
    given (a case whose float32 reference happens to be exact must not divide by zero).  ``limit``: the aggregate limit of
    an arithmetic R does not list (oracle/grad_oracle.py)."""
    got = torch.as_tensor(got).double()
    ref = torch.as_tensor(ref).double()
    bnd = torch.as_tensor(bnd).double()
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    ratio = err / bnd.clamp(min=1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    rr = 0.0
    if ref32 is not None:
        fl = U * rms(ref) if floor is None else floor
        denom = rms(torch.as_tensor(ref32).double() - ref) + fl
        rr = rms(torch.where(torch.isinf(err), torch.full_like(err, 1e30), err)) / denom if denom > 0 else 0.0
    report = f"{case} [{arith}]: worst err/bound {worst:.3g}, rms ratio {rr:.3g} (R {R[arith] if limit is None else limit:g})"
    if ratio.numel() and worst > 0:
        idx = np.unravel_index(int(torch.argmax(ratio)), tuple(ratio.shape))
        where = []
        if ref.dim() >= 3:
            H, W, C = ref.shape[-3:]
            yy, xx, cc = idx[-3], idx[-2], idx[-1]
            if yy in (0, H - 1):
                where.append("border row")
            if xx in (0, W - 1):
                where.append("border column")
            if cc >= C - C % 32 or cc >= C - 4:
                where.append("tail channel")
        report += (f"; worst at {tuple(int(i) for i in idx)} {'/'.join(where) or 'interior'}: got {float(got[idx]):.9g} "
                   f"ref {float(ref[idx]):.9g} bound {float(bnd[idx]):.3g}")
    return worst, rr, report


def ok(got, ref, bnd, ref32=None, arith="f32", case="", floor=None, limit=None):
    """check(...) and assert both levels; returns (worst, rms_ratio) for the caller's record."""
    worst, rr, report = check(got, ref, bnd, ref32, arith, case, floor, limit)
    assert worst <= 1.0, report
    assert rr <= (R[arith] if limit is None else limit), report
    return worst, rr
