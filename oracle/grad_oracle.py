"""Float64 references and a worst-case error model of the gradient kernels (include/himo_amd.h: himo_conv3x3_wgrad*,
himo_linear_wgrad*, himo_colsum, himo_upsample2x_bwd, the data-gradient forms of himo_conv2d and the element-wise kernels of
the training step; csrc/train.hip, csrc/fastnsf.hip).  CPU only.  Conventions of oracle/conv_oracle.py: NHWC maps,
[k][k][Cin][Cout] weights, a per-output WORST-case bound plus an aggregate rms ratio against the same operation in float32.

Every weight gradient here is one matrix product dW = A^T B over a reduction index (pixels or rows): A = the unfolded 3x3
patches of x (or x itself for a Linear layer), B = dY.  The float32 twin is that product as a float32 matrix product, not
whatever autograd dispatches to.

Arithmetics (names of conv_oracle.R, whose values and arguments are taken over unchanged):
  f32     v_mfma_f32_32x32x2_f32 on float32 operands -- conv_wgrad_partial_kernel (train.hip:256-274),
          conv_wgrad_tiled_kernel (train.hip:358-367), wgrad_partial_kernel (fastnsf.hip:54-68), wgrad_partial_lds_kernel
          (fastnsf.hip:136-149) -- and the float32 FMA chains of wgrad_thin_partial_kernel (fastnsf.hip:712-717) and the
          column-sum kernels (fastnsf.hip:507, 525-528).  Every product rounds once, every addition once, in the order of
          the kernel: conv_oracle.R["f32"] = 2.
  bf16x2  flag 2: x = h + m per operand (split2_bf16_pair train.hip:391-400, wg_split_pair fastnsf.hip:176-185: h = RNE
          bf16 of x, m = RNE bf16 of x - h, i.e. conv_oracle.split_terms("bf16x2")), three v_mfma_f32_32x32x16_bf16 per
          fragment pair.  The kept products, as (term of A, term of B):
              conv_wgrad_split_kernel    train.hip:525-527     (1, 0) (0, 1) (0, 0)
              conv_wgrad_split2_kernel   train.hip:665-667     (1, 0) (0, 1) (0, 0)
              wgrad_partial_split_kernel fastnsf.hip:288-290   (1, 0) (0, 1) (0, 0)
              wgrad_full_split_kernel    fastnsf.hip:434-436   (1, 0) (0, 1) (0, 0)
          m * m (2^-18 relative) is dropped: conv_oracle.KEPT["bf16x2"] and conv_oracle.R["bf16x2"] = 128.
  elem    the element-wise kernels; R_ELEM below.

Partial-sum merges (conv_wgrad_reduce_kernel train.hip:745, conv_wgrad_tiled_reduce_kernel train.hip:716-729,
wgrad_reduce_kernel fastnsf.hip:481-494, colsum_reduce_kernel fastnsf.hip:550-564, wgrad_thin_reduce_kernel
fastnsf.hip:734-748): a product passes through the additions of its own block (at most the block's share K_b of the K
products), then through at most ceil(blocks / 16) + 4 additions of the reduce kernel.  A second block exists only when the
first owns at least 256 products (conv_wgrad_chunk, wgrad_rows_per_block, four 64-pixel tiles per chunk), so
K_b + ceil(blocks / 16) + 4 <= K + 4 for any admitted size; with the rounding of the product itself and two spare
roundings the accumulation term is (K + MERGE_C) u mag, MERGE_C = 8 (P K + MERGE_C for P kept products).
The accumulate flag adds one rounding of old + new: u (|old| + mag).

Aggregate level (check_cols below): every column of dY's output channel is scaled alike before the rms is taken, the
float32 twin of a column sum is the sequential float32 sum, and the level is asserted from 32 outputs on -- an rms ratio
over the four outputs of a 4-column sum is no statistic, and correct column sums (emulate_colsum) miss R = 2 there by chance.

Observed on an MI355X: see the table at the end of this comment block (information only -- no constant here was chosen
from it).

    (no MI355X run of tests/test_train_conformance_gpu.py has been recorded for this revision yet)
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_oracle as co
from conv_oracle import U, bf16_rne, split_terms, check, ok, rms  # noqa: F401  (re-exported for the tests)

MERGE_C = 8
SPLIT_KEPT = co.KEPT["bf16x2"]           # (term of A, term of B); see the list above
R = {"f32": co.R["f32"], "bf16x2": co.R["bf16x2"]}
# Element-wise kernels: the float32 twin makes one rounding per operation and evaluates its transcendental to about half
# a rounding, an rms error of at least u / 2 relative per output that carries a rounding at all.  The budgets below allow
# the device functions (6 + |v|) u on a sigmoid and 4 u + 2 e u (4 + 2 |v|) on a tanh (conv_oracle.bound), i.e. at most 16
# roundings at the |v| <= 10 where those functions are not yet saturated to a constant: 16 / (1 / 2) = 32.
R_ELEM = 32.0
TINY = 2.0 ** -125                       # float32 results below the smallest normal (2^-126) may be flushed to zero


def _d(a):
    return torch.as_tensor(np.asarray(a, np.float64)) if not torch.is_tensor(a) else a.double()


# ---- references ------------------------------------------------------------------------------------------------------
def patches(x, stride=1):
    """The unfolded 3x3 (pad 1) patches of NHWC ``x``: [N * Ho * Wo, Cin * 9], column = (ci, ky, kx); Ho = ceil(H / stride)."""
    n, h, w, c = x.shape
    p = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1, stride=stride)            # [N, Cin * 9, Ho * Wo]
    return p.permute(0, 2, 1).reshape(-1, c * 9)


def _fold_dw(m, cin):
    """[Cin * 9, Cout] (rows (ci, ky, kx)) -> [3][3][Cin][Cout]"""
    return m.reshape(cin, 3, 3, -1).permute(1, 2, 0, 3).contiguous()


def out_size(h, stride):
    return (h + stride - 1) // stride


def conv3x3_dw(x, dy, stride=1, dtype=torch.float64):
    """dW [3][3][Cin][Cout] of y = conv3x3(x, W, pad 1, stride) summed over the batch: patches(x)^T dY as a matrix product
    in ``dtype`` (float64: the reference; float32: the defined float32 twin)."""
    x, dy = torch.as_tensor(x).to(dtype), torch.as_tensor(dy).to(dtype)
    assert dy.shape[1:3] == (out_size(x.shape[1], stride), out_size(x.shape[2], stride)), (x.shape, dy.shape, stride)
    return _fold_dw(patches(x, stride).T @ dy.reshape(-1, dy.shape[-1]), x.shape[-1])


def conv3x3_dx(dy, w, stride, h, w_in, dtype=torch.float64):
    """dX [N][h][w_in][Cin] of the same convolution: the adjoint, i.e. the convolution of the zero-stuffed dY with the flipped
    kernel, cropped to [h][w_in] (as a transposed convolution)."""
    dy, w = torch.as_tensor(dy).to(dtype), torch.as_tensor(w).to(dtype)
    ho, wo = dy.shape[1:3]
    op = (h + 2 - 3 - (ho - 1) * stride, w_in + 2 - 3 - (wo - 1) * stride)
    dx = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=stride, padding=1, output_padding=op)
    return dx.permute(0, 2, 3, 1)


def zero_stuff2x(dy):
    """z [N][2 Ho][2 Wo][C], z[2 i][2 j] = dy[i][j], zeros elsewhere (himo_zero_stuff2x)"""
    n, h, w, c = dy.shape
    z = torch.zeros(n, 2 * h, 2 * w, c, dtype=dy.dtype)
    z[:, ::2, ::2] = dy
    return z


def weight_flip(w):
    """wf [k][k][Cout][Cin] = w [k][k][Cin][Cout] with mirrored taps (himo_weight_flip)"""
    return torch.as_tensor(w).flip(0, 1).permute(0, 1, 3, 2).contiguous()


def linear_dw(x, dz, dtype=torch.float64):
    return torch.as_tensor(x).to(dtype).T @ torch.as_tensor(dz).to(dtype)


def colsum(z, dtype=torch.float64):
    """column sums of [..., C] over every other axis.  float32: the DEFINED twin -- one float32 accumulator per column, rows added
    in order (numpy's accumulate along axis 0), not a library's blocked or pairwise sum."""
    z = torch.as_tensor(z).to(dtype)
    z = z.reshape(-1, z.shape[-1])
    if dtype == torch.float32:
        return torch.from_numpy(np.add.accumulate(z.numpy(), axis=0)[-1].copy())
    return z.sum(0)


def _axis_weights(n_in, n_ratio=None):
    """[n_in, 2 n_in] bilinear x2 weights with align_corners: output o reads source o (n - 1) / (2 n - 1).  ``n_ratio``:
    the axis length the ratio is taken from (a wrong kernel uses the other axis')."""
    nr = n_in if n_ratio is None else n_ratio
    a = torch.zeros(n_in, 2 * n_in, dtype=torch.float64)
    for o in range(2 * n_in):
        s = o * (nr - 1) / (2 * nr - 1) if nr > 1 else 0.0
        i0 = min(int(math.floor(s)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        f = min(max(s - i0, 0.0), 1.0)
        a[i0, o] += 1.0 - f
        a[i1, o] += f
    return a


def _axis_weights32(n_in):
    """the same weights computed in float32 the way the kernels do (train.hip:200-205): r = (n - 1) / (2 n - 1), s = r o,
    i0 = int(s), f = s - i0, every step rounded to float32"""
    a = torch.zeros(n_in, 2 * n_in, dtype=torch.float32)
    r = np.float32(n_in - 1) / np.float32(2 * n_in - 1) if n_in > 1 else np.float32(0)
    for o in range(2 * n_in):
        s = np.float32(r * np.float32(o))
        i0 = int(s)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        f = np.float32(s - np.float32(i0))
        a[i0, o] += float(np.float32(1) - f)
        a[i1, o] += float(f)
    return a


def upsample2x_adjoint(dy, dtype=torch.float64, ratio_from=None):
    """dx [H][W][C] = the adjoint of the bilinear x2 (align_corners) upsampling applied to dy [2 H][2 W][C]
    (himo_upsample2x_bwd).  ratio_from = (h, w): axis lengths the weights are computed from (emulating a wrong kernel)."""
    dy = torch.as_tensor(dy).to(dtype)
    h, w = dy.shape[0] // 2, dy.shape[1] // 2
    rh, rw = (h, w) if ratio_from is None else ratio_from
    if dtype == torch.float32 and ratio_from is None:      # the float32 twin: float32 source coordinates, weights and sums
        return torch.einsum("yo,xp,opc->yxc", _axis_weights32(h), _axis_weights32(w), dy)
    return torch.einsum("yo,xp,opc->yxc", _axis_weights(h, rh).to(dtype), _axis_weights(w, rw).to(dtype), dy)


def upsample2x_adjoint_bound(dy):
    """upsample2x_bwd_kernel (train.hip:183-221): the float32 source coordinate s = r o carries the rounding of r and of
    the product, d = 2 u s + u <= u (2 (n - 1) + 2) on either weight of that axis, and an output pixel within d of an
    integer source coordinate may gain or lose a weight of at most d (candidate range train.hip:195-198); the weight
    product and the at most 16 accumulated terms round (16 + 2) u.  E = d on every (pixel, output) pair whose exact source
    coordinate lies within one pixel."""
    dy = _d(dy).abs()
    h, w = dy.shape[0] // 2, dy.shape[1] // 2

    def axis(n):
        a = _axis_weights(n)
        e = torch.zeros_like(a)
        dlt = U * (2 * (n - 1) + 2)
        for o in range(2 * n):
            s = o * (n - 1) / (2 * n - 1) if n > 1 else 0.0
            for i in range(max(0, int(math.floor(s)) - 1), min(n - 1, int(math.floor(s)) + 2) + 1):
                if abs(s - i) <= 1.0 + 1e-3:
                    e[i, o] = dlt
        return a, e
    ay, ey = axis(h)
    ax, ex = axis(w)
    exact = torch.einsum("yo,xp,opc->yxc", ay, ax, dy)
    wide = torch.einsum("yo,xp,opc->yxc", ay + ey, ax + ex, dy)
    return (wide - exact) + 18 * U * exact + TINY


# ---- bounds of the matrix products --------------------------------------------------------------------------------
def product_bound(arith, a, b, old=None, n_acc=1):
    """Per-output worst case of |got - A^T B| for float32 matrices A [K, M], B [K, N] -> float64 [M, N].

    f32:    (K + MERGE_C) u |A|^T |B|.
    bf16x2: operand residuals, exact:  dA^T |B| + |A|^T dB + dA^T dB,  d = |a - (h + m)|;
            the dropped product, exact:  |m_A|^T |m_B|;
            float32 accumulation of the three kept products (each exact: 8 x 8 significant bits):
            (3 K + MERGE_C) u (|h_A| + |m_A|)^T (|h_B| + |m_B|).
    old (the accumulate flag): + u (|old| + |A|^T |B|), n_acc times when the sum is built by n_acc accumulating calls."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    K = a.shape[0]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    aa, ab = t(np.abs(a)), t(np.abs(b))
    mag = aa.T @ ab
    if arith == "f32":
        bnd = (K + MERGE_C) * U * mag
    elif arith == "bf16x2":
        ta, tb = split_terms("bf16x2", a), split_terms("bf16x2", b)
        da = t(np.abs(a.astype(np.float64) - ta[0].astype(np.float64) - ta[1].astype(np.float64)))
        db = t(np.abs(b.astype(np.float64) - tb[0].astype(np.float64) - tb[1].astype(np.float64)))
        bnd = da.T @ ab + aa.T @ db + da.T @ db
        for i in range(2):
            for j in range(2):
                if (i, j) not in SPLIT_KEPT:
                    bnd = bnd + t(np.abs(ta[i])).T @ t(np.abs(tb[j]))
        sa, sb = t(np.abs(ta[0])) + t(np.abs(ta[1])), t(np.abs(tb[0])) + t(np.abs(tb[1]))
        bnd = bnd + (len(SPLIT_KEPT) * K + MERGE_C) * U * (sa.T @ sb)
    else:
        raise ValueError(arith)
    if old is not None:
        bnd = bnd + n_acc * U * (_d(old).abs().reshape(bnd.shape) + mag)
    return bnd + TINY


def conv3x3_dw_bound(arith, x, dy, stride=1, old=None, n_acc=1):
    x, dy = torch.as_tensor(x).float(), torch.as_tensor(dy).float()
    cin, cout = x.shape[-1], dy.shape[-1]
    o = None if old is None else _d(old).permute(2, 0, 1, 3).reshape(cin * 9, cout)
    return _fold_dw(product_bound(arith, patches(x, stride).numpy(), dy.reshape(-1, cout).numpy(), o, n_acc), cin)


def linear_dw_bound(arith, x, dz, old=None):
    return product_bound(arith, torch.as_tensor(x).float().numpy(), torch.as_tensor(dz).float().numpy(), old)


def colsum_bound(z, old=None):
    """float32 column sums (colsum_partial*_kernel, the bias partials of the split kernels, train.hip:475 / fastnsf.hip:256):
    (K + MERGE_C) u sum |z|, K = rows."""
    z = _d(z).abs()
    z = z.reshape(-1, z.shape[-1])
    bnd = (z.shape[0] + MERGE_C) * U * z.sum(0)
    if old is not None:
        bnd = bnd + U * (_d(old).abs() + z.sum(0))
    return bnd + TINY


# ---- emulations of the kernels' arithmetic (tests/test_grad_oracle.py) ---------------------------------------------
def emulate_product(arith, a, b, chunk=256, kept=None):
    """A^T B the way the kernels compute it: float32 products and sums per chunk of ``chunk`` reduction steps (for bf16x2
    every kept product of the split terms, exact, summed in float32), the chunk partials merged in float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    kept = (SPLIT_KEPT if arith == "bf16x2" else [(0, 0)]) if kept is None else kept
    ta, tb = split_terms(arith, a), split_terms(arith, b)
    acc = None
    for k0 in range(0, a.shape[0], chunk):
        part = None
        for i, j in kept:
            p = torch.from_numpy(ta[i][k0:k0 + chunk]).T @ torch.from_numpy(tb[j][k0:k0 + chunk])
            part = p if part is None else part + p
        acc = part if acc is None else acc + part
    return acc


# ---- element-wise kernels (include/himo_amd.h, "a11, training side") ------------------------------------------------
def _gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def _gelu_grad(t):
    return 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)


def elementwise(name, dtype=torch.float64, **a):
    """The documented formula of kernel ``name`` in ``dtype`` -> dict of outputs.  In/out tensors (dhp, dx of the GRU
    backward stages, y of add2d) are passed with their old value and returned with the new one."""
    a = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in a.items()}
    if name == "gru_gates1":                               # pre [n, 256], hx [n, 192]
        z, r = torch.sigmoid(a["pre"][:, :128]), torch.sigmoid(a["pre"][:, 128:])
        return dict(z=z, r=r, out=torch.cat([r * a["hx"][:, :128], a["hx"][:, 128:]], 1))
    if name == "gru_gates2":                               # pre [n, 128], z [n, 128], hx [n, 192]
        q = torch.tanh(a["pre"])
        return dict(q=q, out=torch.cat([(1 - a["z"]) * a["hx"][:, :128] + a["z"] * q, a["hx"][:, 128:]], 1))
    if name == "gru_bwd1":
        g, z, q, h = a["dh_next"], a["z"], a["q"], a["hx"][:, :128]
        return dict(dz=g * (q - h), daq=g * z * (1 - q * q), dhp=g * (1 - z))
    if name == "gru_bwd2":
        drh, h, z, r = a["d_rhx"][:, :128], a["hx"][:, :128], a["z"], a["r"]
        return dict(dhp=a["dhp"] + drh * r, dazr=torch.cat([a["dz"] * z * (1 - z), (drh * h) * r * (1 - r)], 1),
                    dx=a["dx"] + a["d_rhx"][:, 128:])
    if name == "gru_bwd3":
        return dict(dh=a["dhp"] + a["d_hx"][:, :128], dx=a["dx"] + a["d_hx"][:, 128:])
    if name == "affine_gelu_fwd":
        pre = a["x"] if a.get("scale") is None else a["x"] * a["scale"] + a["shift"]
        return dict(pre=pre, y=_gelu(pre))
    if name == "affine_gelu_bwd":
        g = a["dy"] * _gelu_grad(a["pre"])
        return dict(dx=g if a.get("scale") is None else g * a["scale"])
    if name == "add2d":
        return dict(y=a["y"] + a["b"])
    if name == "rows_add":
        return dict(y=a["a"] if a.get("b") is None else a["a"] + a["b_scale"] * a["b"])
    raise ValueError(name)


def elementwise_bound(name, **a):
    """Per-output worst case of the float32 kernels (train.hip:17-144, fastnsf.hip:646-654), float64 inputs as given:
    conv_oracle.bound's budgets for the transcendental functions (sigmoid: g u (6 + |v|); tanh: 2 e u (4 + 2 |v|) + 4 u |q|,
    e = exp(-2 |v|); GELU: (|t| / 2) (1.5e-7 + 16 u) + 4 u |y|) plus c u |value| for the c roundings of the products and sums
    of each formula (counted below), plus the float32 underflow floor."""
    a = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in a.items()}
    r = elementwise(name, **a)
    ab = torch.abs
    if name == "gru_gates1":
        v = a["pre"]
        g = torch.sigmoid(v)
        bg = g * U * (6 + ab(v))
        h = a["hx"][:, :128]
        out = torch.cat([ab(h) * bg[:, 128:] + U * ab(r["out"][:, :128]), torch.zeros_like(a["hx"][:, 128:])], 1)
        b = dict(z=bg[:, :128], r=bg[:, 128:], out=out)
    elif name == "gru_gates2":
        v, z, h = a["pre"], a["z"], a["hx"][:, :128]
        q = r["q"]
        bq = 2 * torch.exp(-2 * ab(v)) * U * (4 + 2 * ab(v)) + 4 * U * ab(q)
        # 1 - z, two products, one sum: 3 u on either term (conv_oracle.bound, GRU q)
        out = torch.cat([ab(z) * bq + 3 * U * (ab((1 - z) * h) + ab(z * q)), torch.zeros_like(a["hx"][:, 128:])], 1)
        b = dict(q=bq, out=out)
    elif name == "gru_bwd1":
        g, z, q = a["dh_next"], a["z"], a["q"]
        # dz, dhp: a difference and a product, 2 roundings (3 u); daq: q q and 1 - q q round absolutely, then two products
        b = dict(dz=3 * U * ab(r["dz"]), dhp=3 * U * ab(r["dhp"]),
                 daq=U * (ab(g * z) * (q * q + ab(1 - q * q)) + 3 * ab(r["daq"])))
    elif name == "gru_bwd2":
        drh, rr = a["d_rhx"][:, :128], a["r"]
        b = dict(dhp=2 * U * (ab(a["dhp"]) + ab(drh * rr)),                    # product, sum
                 dazr=5 * U * ab(r["dazr"]),                                   # 1 - g and up to three products (4 roundings)
                 dx=2 * U * (ab(a["dx"]) + ab(a["d_rhx"][:, 128:])))
    elif name == "gru_bwd3":
        b = dict(dh=2 * U * (ab(a["dhp"]) + ab(a["d_hx"][:, :128])), dx=2 * U * (ab(a["dx"]) + ab(a["d_hx"][:, 128:])))
    elif name == "affine_gelu_fwd":
        t = r["pre"]
        dt = torch.zeros_like(t) if a.get("scale") is None else 2 * U * (ab(a["x"] * a["scale"]) + ab(a["shift"]))
        by = co.GELU_SLOPE * dt + 0.5 * (ab(t) + dt) * (co.ERF_AS + 16 * U) + 4 * U * ab(r["y"])
        b = dict(pre=dt, y=by)
    elif name == "affine_gelu_bwd":
        t = a["pre"]
        phi = torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
        # Phi from erf as in the GELU budget; t phi(t): the exponent -t^2 / 2 rounds twice (u t^2 on exp) + exp and two products
        dg = 0.5 * (co.ERF_AS + 16 * U) + ab(t) * phi * U * (t * t + 8) + 2 * U * ab(_gelu_grad(t))
        sc = 1.0 if a.get("scale") is None else ab(a["scale"])
        b = dict(dx=ab(a["dy"]) * sc * dg + 3 * U * ab(r["dx"]))
    elif name == "add2d":
        b = dict(y=2 * U * (ab(a["y"]) + ab(a["b"])))
    elif name == "rows_add":
        b = dict(y=torch.zeros_like(r["y"]) if a.get("b") is None else 2 * U * (ab(a["a"]) + ab(a["b_scale"] * a["b"])))
    else:
        raise ValueError(name)
    return {k: v + TINY for k, v in b.items()}


# ---- the two-level check for gradients whose columns span decades ------------------------------------------------------
MIN_AGGREGATE = 32


def check_cols(got, ref, bnd, ref32, arith, case=""):
    """conv_oracle.check on a gradient whose LAST axis is the output channel of dY.

    The columns of dY span six decades (``operands``), and an rms over the whole tensor would be the rms of its one or two
    largest columns.  Every column is therefore divided by its own scale first (the rms of its worst-case bound, which is
    proportional to sum |a| |b| and, unlike the reference itself, does not vanish where a sum happens to cancel) -- the
    per-element bound level is unchanged by that, the aggregate level now weighs every column alike.  The aggregate level
    is a statistic: the ratio of two rms errors over k independent outputs is F-distributed, and for k = 4 a correct
    kernel exceeds any fixed R of a few units in one case of ten (tests/test_grad_oracle.py shows it for the column sums).
    It is asserted where the result has at least MIN_AGGREGATE = 32 elements (P(F(32, 32) > 4) < 1e-4); below that only
    the bound level holds, which is per element and needs no sample."""
    got, ref, bnd = torch.as_tensor(got).double(), torch.as_tensor(ref).double(), torch.as_tensor(bnd).double()
    c = ref.shape[-1]
    s = bnd.reshape(-1, c).pow(2).mean(0).sqrt().clamp(min=1e-290)
    r32 = None if (ref32 is None or ref.numel() < MIN_AGGREGATE) else torch.as_tensor(ref32).double() / s
    return check(got / s, ref / s, bnd / s, r32, arith, case)


def ok_cols(got, ref, bnd, ref32, arith, case=""):
    worst, rr, report = check_cols(got, ref, bnd, ref32, arith, case)
    assert worst <= 1.0, report
    assert rr <= R[arith], report
    return worst, rr


def emulate_colsum(z, groups=8):
    """the column-sum kernels' order (fastnsf.hip:499-566): blocks of wgrad_rows_per_block rows, ``groups`` interleaved
    sequential chains per block (2: colsum_partial_kernel, 8: colsum_partial_v4_kernel), the block partials reduced by 8
    groups of 4 chains, every step in float32"""
    z = np.asarray(z, np.float32)
    n, c = z.shape
    rows_pb = (max(256, -(-n // 512)) + 31) // 32 * 32
    nb = -(-n // rows_pb)
    parts = np.zeros((nb, c), np.float32)
    for b in range(nb):
        blk = z[b * rows_pb:(b + 1) * rows_pb]
        gs = [np.add.accumulate(blk[g::groups], axis=0)[-1] if blk[g::groups].shape[0] else np.zeros(c, np.float32) for g in range(groups)]
        t = gs[0]
        for g in gs[1:]:
            t = t + g
        parts[b] = t
    sh = []
    for g in range(8):
        ch = [np.zeros(c, np.float32) for _ in range(4)]
        b = g
        while b + 24 < nb:
            for k in range(4):
                ch[k] = ch[k] + parts[b + 8 * k]
            b += 32
        while b < nb:
            ch[0] = ch[0] + parts[b]
            b += 8
        sh.append((ch[0] + ch[1]) + (ch[2] + ch[3]))
    t = sh[0]
    for g in sh[1:]:
        t = t + g
    return torch.from_numpy(t)


def ok_elem(got, ref, bnd, ref32, case):
    """both levels for an element-wise output (2-D): within the bound, and rms error within R_ELEM of the float32 twin's"""
    return ok(got, ref, bnd, ref32, "f32", case, limit=R_ELEM)


# ---- the inputs of the conformance matrix (shared by tests/test_grad_oracle.py and tests/test_train_conformance_gpu.py) ----
def operands(seed, a_shape, b_shape):
    """A = N(0, 1) x a per-channel scale in [0.1, 3]; B = N(0, 1) x a per-column scale spanning six decades
    (10^U(-6, 0)), the gradients of tests/test_train_gpu.py::test_split_bf16_weight_gradient_matches_autograd."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(*a_shape, generator=g) * (0.1 + 2.9 * torch.rand(a_shape[-1], generator=g))
    b = torch.randn(*b_shape, generator=g) * 10.0 ** (-6.0 * torch.rand(b_shape[-1], generator=g))
    return a, b
