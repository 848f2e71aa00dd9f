"""Float64 reference and worst-case error model of the per-pair fit kernels (include/himo_amd.h: himo_nsf_forward,
himo_nsf_forward_keep, himo_nsf_last_grad, himo_nsf_backward, himo_nsf_update, himo_dt_build, himo_dt_loss, himo_adam_step;
csrc/nsffused.hip, csrc/dtloss.hip, csrc/dtlookup.h, csrc/adam.h).  CPU only.  Conventions of oracle/conv_oracle.py, oracle/grad_oracle.py
and oracle/head_oracle.py: a per-output WORST-case bound plus an aggregate rms ratio against the same operation in float32.

Shapes are the interface's: x [n_pad][4] (column 3 and the padding rows zero), a parameter set is a list of (W [cin][cout],
b [cout]) float32 -- first (W [4][128]), n_hidden - 1 hidden (W [128][128]), last (W [128][4]).  ``iteration`` is the whole
operation in ``dtype``: float64 is the reference, float32 the defined float32 twin; ``variant`` names a deliberately WRONG twin
(tests/test_nsf_oracle.py shows that each misses the bounds below).

The distance transform is a brute-force integer computation (``dt_brute``): G[c] = min over occupied cells within the window
on every axis of dx^2 + dy^2 + dz^2, 0xFFFF when there is none -- the function the three separable passes of csrc/dtloss.hip
compute, so the device's uint16 volume must EQUAL it.  Occupancy is dt_mark_kernel's rule in float32 (``occupancy``).

Bounds (u = 2^-24, gamma(k) = k u / (1 - k u); every constant is counted from the code, none was chosen from a GPU run):
  lookup   (dtlookup.h) u_c = (p_c - o_c) / cell - 1/2: a difference, a quotient and a difference, each rounding relative to a
           value of at most |p - o| / cell + 1/2: e_u = gamma(3) (|p - o| / cell + 1/2) (+ e_p / cell when p = x + out carries the
           network's error e_p).  f = u - floor(u) is exact.  The interpolant is affine in each coordinate, so a coordinate error
           moves D by at most e_u times the largest of the four edge differences along that axis (S_c), and a gradient component
           by e_u times the largest mixed second difference (M_ca).  The arithmetic: sqrtf and the product with cell (2
           roundings per corner value), 1 - f (1), three levels of two products and a sum (3 each, with 1 - f: 4): 14 roundings
           of values <= Dmax = the largest corner value; the gradient forms differences of such values and scales them by
           1 / cell (4 more): gamma(16) Dmax on D, gamma(24) Dmax / cell on a gradient component.
  first    layer: z = fma(x3, w3, fma(x2, w2, fma(x1, w1, x0 w0))) + b: 5 roundings: gamma(5) (|x| |W| + |b|).
  hidden   layers (nsf_fwd_gemm): the fp16 split of the activations against the 2^6-scaled fp16 split of the weights, kept
           products conv_oracle.KEPT["f16x2"], one float32 accumulator: head_oracle.gemm_mag_bound("f16x2") (= conv_oracle.
           operand_bound with the operand's split at its worst case) with its accumulation term counted in the kernel's order
           and over the units that are on (``gemm_bound``), + u |z| for z = fma(acc, 2^-6, b).
  last     layer: s = b; 128 x s = fma(y_k, w_k, s): gamma(129) (|h| |W| + |b|).
  g_{L-1}  = fma chain over the 4 outputs: gamma(4) |dout| |W_last^T|.
  g_{k-1}  = dZ_k W_k^T (two-term bf16 on either side, kept conv_oracle.KEPT["bf16x2"]): ``gemm_bound("bf16x2")`` likewise.
  dW_k     = H_{k-1}^T dZ_k, hidden k: grad_oracle.product_bound("bf16x2") with both operands' splits at their worst case
           (``wgrad_coeff``; K = the 256 rows of a backward block, the blocks' partials are summed in float64 by the test);
           hidden db_k, db_0, dW_0: float32 sums of 128 + 1 terms per block: gamma(130); dW_last: 32-term fma chains merged in
           pairs, then four tiles: gamma(40); db_last: 64 + 3 + 1: gamma(70).
  Adam     grad_oracle.elementwise_bound's style: roundings counted per formula (``adam_bound``), aggregate limit R_ELEM.

Propagation.  ReLU makes the network piecewise LINEAR: while the kernel's masks equal the reference's, the kernel's error at
layer j is exactly sum over k <= j of delta_k J_{k -> j} with delta_k the local error of layer k's product (bounded as above, for
an operand of magnitude |h| + E) and J_{k -> j} = D_k W_{k+1} D_{k+1} ... W_j the network's own Jacobian for that point.  The
bound is therefore E_j = sum_k b_k |J_{k -> j}| with the absolute value taken AFTER the matrix products -- head_oracle.
propagate_forward's scheme with the ReLU masks (1-Lipschitz, and 0 where the unit is off) inside the product.  Taking |W| layer by
layer instead grows about threefold per layer with init_mlp's weights and leaves no usable margin at eight layers.  The
backward pass is linear in dout given the masks and is propagated the same way through the transposed Jacobians.

Decision margins.  That argument needs the masks -- and the lookup's base cell, in-volume and D <= trunc decisions -- to agree.
``mlp_case`` admits a candidate point only if, in the float64 reference, |z_k| >= 2 E_k for every unit of every layer, every
lookup coordinate is at least 2 e_u from the nearest integer (0 and n - 1 among them; for a point outside the volume: one
violated axis by that margin) and |D - trunc| >= 2 e_D, with e_u including the bound on out.  By induction over the layers the
kernel then takes the reference's decisions as long as it is within the asserted bounds.  Decisions AT a threshold are tested
with exactly representable inputs instead (``threshold_points``, ``mask_threshold_case``).

Observed on an MI355X (information only -- no constant here was chosen from it): worst err/bound and worst rms ratio per family
from the module summary of tests/test_nsf_conformance_gpu.py:
    dt_build   bit-equal (10 volumes)           dt_loss    0.239, 0.97 (R_ELEM 32)      forward    f16x2 0.505, 1.79 (R 4)
    objective  f16x2 0.105, 0.917               last_grad  f16x2 0.0558, 1.58           backward   bf16x2 0.35, 36.8 (R 128)
    update     bf16x2 0.173, 20.8; f16x2 0.0141, 1.66; f32 (alone) 0.5, 0.528           adam       0.986 (the final rounding of p), 0.454
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import conv_oracle as co
import grad_oracle as go
import head_oracle as ho
from conv_oracle import U

HID, ROWS, BLOCK_TILES, LAST_STRIDE, MAX_HIDDEN, INF, MAX_WINDOW = 128, 64, 4, 4 * 128 + 8, 12, 0xFFFF, 40
TINY = go.TINY
gamma = ho.gamma
F64 = torch.float64


def padded_rows(n):
    """himo_nsf_padded_rows: whole 64-row tiles, rounded up to whole backward blocks of four tiles"""
    return 0 if n <= 0 else -(-(-(-n // ROWS)) // BLOCK_TILES) * BLOCK_TILES * ROWS


# ---- the distance-transform volume ---------------------------------------------------------------------------------------
def grid(origin, cell, dims, window, trunc, G=None):
    return SimpleNamespace(origin=np.asarray(origin, np.float32), cell=np.float32(cell), dims=tuple(int(d) for d in dims),
                           window=int(window), trunc=np.float32(trunc), G=G)


def occupancy(pts, gr):
    """(nz, ny, nx) bool: dt_mark_kernel's rule in float32 -- floorf((p - o) / cell) per axis, inside iff 0 <= f < n, NaN dropped"""
    nx, ny, nz = gr.dims
    occ = np.zeros((nz, ny, nx), bool)
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    if len(p):
        with np.errstate(invalid="ignore"):
            f = np.floor((p - gr.origin) / gr.cell)
            ok = ((f >= 0) & (f < np.asarray(gr.dims, np.float32))).all(1)
        c = f[ok].astype(np.int64)
        occ[c[:, 2], c[:, 1], c[:, 0]] = True
    return occ


def mark_margin_ok(pts, gr):
    """dt_mark's decision margin: (p - o) / cell (two roundings, relative) at least 2 gamma(2) |q| from an integer"""
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    q = (p - gr.origin.astype(np.float64)) / float(gr.cell)
    return (np.abs(q - np.round(q)) >= 2 * gamma(2) * np.abs(q)).all(1) | np.isnan(q).any(1)


def dt_brute(occ, window):
    """uint16 (nz, ny, nx): min over occupied cells with |dx|, |dy|, |dz| <= window of dx^2 + dy^2 + dz^2, else 0xFFFF"""
    oc = np.argwhere(occ).astype(np.int32)
    G = np.full(occ.size, INF, np.uint16)
    if len(oc):
        cells = np.indices(occ.shape, dtype=np.int32).reshape(3, -1).T
        chunk = max(1, (1 << 21) // len(oc))
        for s in range(0, len(cells), chunk):
            d = np.abs(cells[s:s + chunk, None, :] - oc[None, :, :])
            d2 = np.where((d <= window).all(2), (d * d).sum(2), INF)
            G[s:s + chunk] = d2.min(1)
    return G.reshape(occ.shape)


def _dvol(gr, dtype):
    """dt_value: min(sqrt(G), W) cell, W where G is 0xFFFF"""
    g = torch.from_numpy(gr.G.astype(np.int64))
    d = torch.where(g == INF, torch.full(g.shape, float(gr.window), dtype=dtype), g.to(dtype).sqrt())
    return torch.clamp(d, max=float(gr.window)) * torch.tensor(float(gr.cell), dtype=dtype)


def lookup(p, gr, dtype=F64, variant=None):
    """dtlookup.h in ``dtype`` on the float32 points p [n, 3] -> inside, D, keep = inside and D <= trunc, gr = dD/dp where keep
    (per metre, unnormalised), u, and the eight corner values d [n, 2, 2, 2] (x, y, z)"""
    p = torch.as_tensor(p).to(dtype).reshape(-1, 3)
    o = torch.from_numpy(gr.origin).to(dtype)
    cell = torch.tensor(float(gr.cell), dtype=dtype)
    dims = torch.tensor(gr.dims, dtype=dtype)
    u = (p - o) / cell
    if variant != "corner":
        u = u - 0.5
    hi = dims - 1
    inside = ((u >= 0) & (u <= hi)).all(1) if variant == "inside_ge" else ((u > 0) & (u < hi)).all(1)
    b = torch.nan_to_num(u.floor(), nan=0.0, posinf=0.0, neginf=0.0)
    b = torch.minimum(b, dims - 2).clamp(min=0)
    f = torch.nan_to_num(u - b, nan=0.0, posinf=0.0, neginf=0.0)
    bi = b.long()
    V = _dvol(gr, dtype)
    nx, ny, nz = gr.dims
    at = lambda dx, dy, dz: V[(bi[:, 2] + dz).clamp(max=nz - 1), (bi[:, 1] + dy).clamp(max=ny - 1), (bi[:, 0] + dx).clamp(max=nx - 1)]
    d = torch.stack([torch.stack([torch.stack([at(i, j, k) for k in (0, 1)], 1) for j in (0, 1)], 1) for i in (0, 1)], 1)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    gx, gy, gz = 1 - fx, 1 - fy, 1 - fz
    c00, c10 = d[:, 0, 0, 0] * gx + d[:, 1, 0, 0] * fx, d[:, 0, 1, 0] * gx + d[:, 1, 1, 0] * fx
    c01, c11 = d[:, 0, 0, 1] * gx + d[:, 1, 0, 1] * fx, d[:, 0, 1, 1] * gx + d[:, 1, 1, 1] * fx
    c0, c1 = c00 * gy + c10 * fy, c01 * gy + c11 * fy
    D = c0 * gz + c1 * fz
    trunc = float(gr.trunc)
    keep = inside & ((D < trunc) if variant == "trunc_lt" else (D <= trunc))
    s = torch.tensor(1.0, dtype=dtype) if variant == "no_scale" else 1.0 / cell
    g0 = (((d[:, 1, 0, 0] - d[:, 0, 0, 0]) * gy + (d[:, 1, 1, 0] - d[:, 0, 1, 0]) * fy) * gz
          + ((d[:, 1, 0, 1] - d[:, 0, 0, 1]) * gy + (d[:, 1, 1, 1] - d[:, 0, 1, 1]) * fy) * fz) * s
    g1 = ((c10 - c00) * gz + (c11 - c01) * fz) * s
    g2 = (c1 - c0) * s
    z = torch.zeros_like(D)
    grd = torch.where(keep[:, None], torch.stack([g0, g1, g2], 1), torch.zeros(len(p), 3, dtype=dtype))
    return dict(inside=inside, D=torch.where(inside, D, z), keep=keep, gr=grd, u=u, d=d)


def lookup_bound(res, gr, ep=None, exact_u=False):
    """(e_u [n, 3], e_D [n], e_g [n, 3]) of a float64 ``lookup`` result (module docstring); ep [n, 3]: the error p arrives with;
    exact_u: the coordinates are exactly representable all the way (threshold cases: cell a power of two, integer origin)"""
    u = torch.nan_to_num(res["u"].double(), nan=0.0, posinf=0.0, neginf=0.0)
    cell = float(gr.cell)
    eu = torch.zeros_like(u) if exact_u else gamma(3) * ((u + 0.5).abs() + 0.5)
    if ep is not None:
        eu = eu + ep.double() / cell * (1 + 4 * U)
    d = res["d"].double()
    dmax = d.amax((1, 2, 3))
    dx, dy, dz = d[:, 1] - d[:, 0], d[:, :, 1] - d[:, :, 0], d[:, :, :, 1] - d[:, :, :, 0]
    S = torch.stack([dx.abs().amax((1, 2)), dy.abs().amax((1, 2)), dz.abs().amax((1, 2))], 1)
    eD = (S * eu).sum(1) + gamma(16) * dmax
    mxy = (dx[:, 1] - dx[:, 0]).abs().amax(1)
    mxz = (dx[:, :, 1] - dx[:, :, 0]).abs().amax(1)
    myz = (dy[:, :, 1] - dy[:, :, 0]).abs().amax(1)
    eg = torch.stack([mxy * eu[:, 1] + mxz * eu[:, 2], mxy * eu[:, 0] + myz * eu[:, 2], mxz * eu[:, 0] + myz * eu[:, 1]], 1)
    eg = (eg + gamma(24) * dmax[:, None]) / cell
    live = res["inside"][:, None]
    return eu, torch.where(res["inside"], eD, torch.zeros_like(eD)), torch.where(res["keep"][:, None] & live, eg, torch.zeros_like(eg))


def lookup_margin_ok(res, gr, eu, eD):
    """every decision of the lookup at least twice its bound from its threshold (NaN points are outside for everybody)"""
    u = res["u"].double()
    nan = torch.isnan(u).any(1)
    u = torch.nan_to_num(u, nan=0.0)
    hi = torch.tensor(gr.dims, dtype=F64) - 1
    in_ok = ((u - u.round()).abs() >= 2 * eu).all(1) & ((res["D"].double() - float(gr.trunc)).abs() >= 2 * eD)
    out_ok = ((u <= -2 * eu) | (u >= hi + 2 * eu)).any(1)
    return torch.where(res["inside"], in_ok, out_ok) | nan


def dt_objective(p, gr, dtype=F64, variant=None):
    """himo_dt_loss: loss = (1 / m) sum_keep D, grad [n, 3] = gr / m, m = points in the volume (0 -> loss 0, grad 0)"""
    r = lookup(p, gr, dtype, variant)
    m = int(r["inside"].sum())
    dsum = float(torch.where(r["keep"], r["D"], torch.zeros_like(r["D"])).double().sum())
    inv = (torch.tensor(1.0, dtype=dtype) / torch.tensor(float(m), dtype=dtype)) if m else torch.tensor(0.0, dtype=dtype)
    return dict(loss=dsum / m if m else 0.0, dsum=dsum, m=m, grad=r["gr"] * inv, look=r)


def dt_objective_bound(ref, gr, exact_u=False):
    """bounds of himo_dt_loss's outputs: grad = gr (1 / m): the quotient and the product round once each on top of e_g / m;
    loss: a float64 sum of float32 D's: sum e_D / m"""
    eu, eD, eg = lookup_bound(ref["look"], gr, exact_u=exact_u)
    m = max(ref["m"], 1)
    keep = ref["look"]["keep"]
    e_sum = float(torch.where(keep, eD, torch.zeros_like(eD)).sum()) + 1e-15 * abs(ref["dsum"])
    return dict(grad=eg / m + gamma(2) * ref["grad"].double().abs() + TINY, dsum=e_sum + TINY, loss=e_sum / m + TINY, eu=eu, eD=eD)


# ---- the network -----------------------------------------------------------------------------------------------------------
DEAD_FIRST, DEAD_HIDDEN = (5, 64, 127), (0, 31, 96)


def mlp_params(seed, n_hidden, dead=False):
    """init_mlp-scaled parameters (U(-1 / sqrt(fan_in), ..), fan_in 3 for the first layer) in the interface's padded shapes; the
    padding row of the first W and the padding column of the last are drawn too (x's column 3 is zero; column 3 of out is
    an ordinary output that the objective ignores).  dead: units DEAD_FIRST of the first layer (W = 0, b = -1) and DEAD_HIDDEN
    of every hidden layer (W = -|W|, b = -1/2) are off for every point, and the first layer's x weights are |w| + 0.3, so that
    EVERY unit of the first layer is off for a point at x = -8 m: a fully dead row."""
    g = torch.Generator().manual_seed(1000 + seed)
    shapes = [(4, HID, 3)] + [(HID, HID, HID)] * (n_hidden - 1) + [(HID, 4, HID)]
    ps = []
    for ci, co_, fan in shapes:
        bd = 1.0 / math.sqrt(fan)
        ps.append([((torch.rand(ci, co_, generator=g) * 2 - 1) * bd).float(), ((torch.rand(co_, generator=g) * 2 - 1) * bd).float()])
    if dead:
        ps[0][0][0] = ps[0][0][0].abs() + 0.3
        for j in DEAD_FIRST:
            ps[0][0][:, j] = 0.0
            ps[0][1][j] = -1.0
        for k in range(1, n_hidden):
            for j in DEAD_HIDDEN:
                ps[k][0][:, j] = -ps[k][0][:, j].abs()
                ps[k][1][j] = -0.5
    return [(w.contiguous(), b.contiguous()) for w, b in ps]


def forward(params, x, dtype=F64):
    """-> zs (pre-activations of the n_hidden ReLU layers), out [n, 4]"""
    h = torch.as_tensor(x).to(dtype)
    zs = []
    for w, b in params[:-1]:
        z = h @ w.to(dtype) + b.to(dtype)
        zs.append(z)
        h = z.clamp(min=0)
    return zs, h @ params[-1][0].to(dtype) + params[-1][1].to(dtype)


def masks(zs, variant=None):
    """ReLU' as z > 0"""
    if variant == "mask_ge":
        return [z >= 0 for z in zs]
    if variant == "mask_prev":
        return [zs[0] > 0] + [zs[k - 1] > 0 for k in range(1, len(zs))]
    return [z > 0 for z in zs]


def backward(params, x, zs, dout, dtype=F64, variant=None, swap=(1, 2)):
    """every parameter's UNSCALED gradient [(dW, db)] of sum(out * dout), closed form; the hidden activations' gradients g_k"""
    L = len(zs)
    D = masks(zs, variant)
    x, dout = torch.as_tensor(x).to(dtype), torch.as_tensor(dout).to(dtype)
    hs = [z.clamp(min=0) for z in zs]
    grads = [None] * (L + 1)
    grads[L] = (hs[L - 1].T @ dout, dout.sum(0))
    g = dout @ params[L][0].to(dtype).T
    gs = [None] * L
    for k in range(L - 1, -1, -1):
        gs[k] = g
        dz = g * D[k]
        hin = x if k == 0 else hs[k - 1]
        if variant == "swap_rows" and k == 1:                # two rows of one 32-row half swapped in H_{k-1} but not in dZ_k
            hin = hin.clone()
            hin[[swap[0], swap[1]]] = hin[[swap[1], swap[0]]]
        grads[k] = (hin.T @ dz, dz.sum(0))
        if k:
            g = dz @ params[k][0].to(dtype).T
    return grads, gs


def iteration(params, x, n, gr=None, dtype=F64, variant=None, dout=None):
    """One evaluation on x [n_pad, 4] of which rows [0, n) are points: forward pass, then either the distance-transform
    objective of moved = x + out (``gr`` given) or an external dout; the unscaled gradients of every parameter.
    -> dict zs, out, dout [n_pad, 4], dsum = sum of the counted D, m = points in the volume, look, grads, gs"""
    x = torch.as_tensor(x).float()
    zs, out = forward(params, x, dtype)
    r = dict(zs=zs, out=out, dsum=0.0, m=0, look=None)
    real = torch.arange(len(x)) < n
    if dout is None:
        lk = lookup(x[:, :3].to(dtype) + out[:, :3], gr, dtype, variant)
        r["look"] = lk
        counted = lk["inside"] if variant == "pad_in_m" else lk["inside"] & real
        r["m"] = int(counted.sum())
        r["dsum"] = float(torch.where(lk["keep"] & real, lk["D"], torch.zeros_like(lk["D"])).double().sum())
        full = torch.cat([lk["gr"], torch.zeros(len(x), 1, dtype=dtype)], 1)
        dout = torch.where(real[:, None], full, torch.zeros_like(full))
    else:
        full = dout = torch.as_tensor(dout).to(dtype)
    r["dout"] = dout
    r["grads"], r["gs"] = backward(params, x, zs, dout, dtype, variant)
    if variant == "bias_pad":                                # hidden bias gradients summed over padding rows whose dout was not zeroed
        wrong, _ = backward(params, x, zs, full, dtype)
        r["grads"] = [(gw, wrong[k][1] if 1 <= k < len(zs) else gb) for k, (gw, gb) in enumerate(r["grads"])]
    return r


# ---- propagated bounds -------------------------------------------------------------------------------------------------
def _through(vec, M, Dk, Wnext):
    """a source's matrix one layer on: (M masked by the units that are on) W"""
    return (M * Dk[:, None, :].to(M.dtype)) @ Wnext


def gemm_bound(arith, amag, active, w):
    """head_oracle.gemm_mag_bound for an operand that is exactly ZERO outside ``active`` (the units a ReLU mask switched off),
    with the accumulation term counted in the kernels' order.  gemm_mag_bound charges every one of the P K product-adds (P kept
    products) a rounding at the FULL magnitude sum |a| |w|.  Two facts of nsf_fwd_gemm / nsf_bwd_layer allow less, in the same
    model (one rounding per product added to the accumulator): the product of a zero is zero and adding it rounds nothing, so
    a slab of 16 reduction steps costs 3 nnz roundings, not 48; and the slabs are added one after the other (the accumulator
    is a loop-carried dependency), so a rounding in slab s is relative to at most the magnitude accumulated up to and including
    slab s.  Residual and dropped-product terms are gemm_mag_bound's, unchanged."""
    amag = amag.double()
    base = ho.gemm_mag_bound(arith, amag, w) - ho.TINY
    w32 = np.asarray(w.float().numpy(), np.float32)
    K = w32.shape[0]
    terms, _ = ho._act_terms(arith, amag)
    st = sum(terms)
    sw = torch.from_numpy(sum(np.abs(t).astype(np.float64) for t in co.split_terms(arith, w32, weights=True)))
    P = len(co.KEPT[arith])
    full = (P * K + 2) * U * (st @ sw)
    cum, acc = torch.zeros_like(full), torch.zeros_like(full)
    for s0 in range(0, K, 16):
        cum = cum + st[:, s0:s0 + 16] @ sw[s0:s0 + 16]
        acc = acc + P * active[:, s0:s0 + 16].sum(1, keepdim=True).double() * U * cum
    return (base - full).clamp(min=0) + acc + 2 * U * cum


def forward_bounds(params, x, zs):
    """E_z [k] [n, 128] on every pre-activation and E_out [n, 4] (module docstring: local bounds through the point's own Jacobian).
    No floor is added: a unit whose pre-activation is exact (x = 0 and b = 0) has bound 0."""
    L = len(zs)
    W = [w.double() for w, _ in params]
    x64 = torch.as_tensor(x).double()
    E, E_out = [], []
    for r0 in range(0, len(x64), ROWS):                      # rows are independent: 64 at a time keeps the matrices small
        sl = slice(r0, r0 + ROWS)
        z = [t[sl] for t in zs]
        Dm = [(t > 0) for t in z]
        e = [torch.zeros_like(z[0]) for _ in range(L)]
        eo = torch.zeros(len(z[0]), 4, dtype=F64)
        for k in range(L):
            if k == 0:
                b = gamma(5) * (x64[sl].abs() @ W[0].abs() + params[0][1].double().abs())
            else:
                amag = z[k - 1].clamp(min=0) + e[k - 1] * Dm[k - 1]
                gm = gemm_bound("f16x2", amag, Dm[k - 1], params[k][0])
                b = gm + U * (z[k].abs() + e[k] + gm)
            e[k] = e[k] + b
            M = None
            for j in range(k + 1, L + 1):                    # source k through layers k + 1 .. L - 1 and the last layer
                M = Dm[k][:, :, None].double() * W[k + 1][None] if M is None else _through(None, M, Dm[j - 1], W[j])
                add = torch.einsum("ri,rio->ro", b, M.abs())
                if j < L:
                    e[j] = e[j] + add
                else:
                    eo = eo + add
        hmag = z[L - 1].clamp(min=0) + e[L - 1] * Dm[L - 1]
        eo = eo + gamma(129) * (hmag @ W[L].abs() + params[L][1].double().abs())
        E.append(e)
        E_out.append(eo)
    return [torch.cat([e[k] for e in E]) for k in range(L)], torch.cat(E_out)


def relu_margin_ok(zs, E):
    ok = torch.ones(len(zs[0]), dtype=torch.bool)
    for z, e in zip(zs, E):
        ok &= (z.abs() >= 2 * e).all(1)
    return ok


def wgrad_coeff(K=ROWS * BLOCK_TILES):
    """grad_oracle.product_bound("bf16x2") per unit of |A|^T |B| with both splits at their worst case (head_oracle._act_terms):
    residuals u_b^2 per operand (dA |B| + |A| dB + dA dB), the dropped product m_A m_B <= ((1 + u_b) u_b)^2, and the float32
    accumulation (3 K + MERGE_C) u of terms summing to at most (1 + u_b)^2 |a| per operand"""
    ub, c = ho.UB, 1.0 + ho.UB
    return 2 * ub ** 2 + ub ** 4 + (c * ub) ** 2 + (3 * K + go.MERGE_C) * U * c ** 4


def backward_bounds(params, x, ref, E, e_dout=None):
    """bounds on the UNSCALED gradients [(e_dW, e_db)] (block partials summed in float64) and on g_k, given the forward bounds E
    and the bound e_dout [n, 4] on dout (None: dout is an input)"""
    zs, dout = ref["zs"], ref["dout"].double()
    L = len(zs)
    W = [w.double() for w, _ in params]
    x64 = torch.as_tensor(x).double()
    n = len(x64)
    ed = torch.zeros_like(dout) if e_dout is None else e_dout.double()
    Dm = [(z > 0) for z in zs]
    eg = [torch.zeros(n, HID, dtype=F64) for _ in range(L)]
    dmag = dout.abs() + ed
    for r0 in range(0, n, ROWS):
        sl = slice(r0, r0 + ROWS)
        if not bool((dmag[sl] > 0).any()):
            continue                                         # rows without a gradient (padding, outside the volume): all zero
        rows = len(x64[sl])

        def run(vec, M, j):                                  # a source sitting at g_j: into g_j, g_{j-1}, ... g_0
            for i in range(j, -1, -1):
                eg[i][sl] += torch.einsum("ri,rio->ro", vec, M.abs())
                if i:
                    M = _through(None, M, Dm[i][sl], W[i].T)
        run(ed[sl], W[L].T[None].expand(rows, 4, HID), L - 1)
        eye = torch.eye(HID, dtype=F64)[None].expand(rows, HID, HID)
        run(gamma(4) * (dmag[sl] @ W[L].T.abs()), eye, L - 1)
        for j in range(L - 1, 0, -1):                        # the product g_{j-1} = dZ_j W_j^T (eg[j] is complete by now)
            bmag = (ref["gs"][j][sl].abs() + eg[j][sl]) * Dm[j][sl]
            run(gemm_bound("bf16x2", bmag, Dm[j][sl], params[j][0].T.contiguous()), eye, j - 1)
    kap = wgrad_coeff()
    out = []
    for k in range(L + 1):
        if k == L:
            hm, eh = zs[L - 1].clamp(min=0), E[L - 1] * Dm[L - 1]
            e_w = eh.T @ dmag + hm.T @ ed + gamma(40) * ((hm + eh).T @ dmag)
            e_b = ed.sum(0) + gamma(70) * dmag.sum(0)
        else:
            dz, edz = (ref["gs"][k] * Dm[k]).abs(), eg[k] * Dm[k]
            e_b = edz.sum(0) + gamma(130) * (dz + edz).sum(0)
            if k == 0:
                e_w = x64.abs().T @ edz + gamma(130) * (x64.abs().T @ (dz + edz))
            else:
                hm, eh = zs[k - 1].clamp(min=0), E[k - 1] * Dm[k - 1]
                e_w = eh.T @ (dz + edz) + hm.T @ edz + kap * ((hm + eh).T @ (dz + edz))
        out.append((e_w + TINY, e_b + TINY))
    return out, eg


# ---- Adam -------------------------------------------------------------------------------------------------------------
ADAM = dict(lr=np.float32(1e-3), b1=np.float32(0.9), b2=np.float32(0.999), eps=np.float32(1e-8))


def adam(p, g, m, v, step, dtype=F64, variant=None, lr=ADAM["lr"], b1=ADAM["b1"], b2=ADAM["b2"], eps=ADAM["eps"]):
    """torch.optim.Adam's order on the float32 inputs: m' = b1 m + (1 - b1) g, v' = b2 v + (1 - b2) g g,
    p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)"""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype) if not torch.is_tensor(a) else a.to(dtype)
    p, g, m, v, lr, b1, b2, eps = (t(a) for a in (p, g, m, v, lr, b1, b2, eps))
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if variant == "adam_nobc":
        bc1, bc2 = torch.ones_like(bc1), torch.ones_like(bc2)
    mn = b1 * m + (1 - b1) * g
    vn = b2 * v + (1 - b2) * g * g
    return p - (lr / bc1) * (mn / (vn.sqrt() / bc2.sqrt() + eps)), mn, vn


def adam_bound(p, g, m, v, step, lr=ADAM["lr"], b1=ADAM["b1"], b2=ADAM["b2"], eps=ADAM["eps"]):
    """Roundings counted from adam_update (csrc/adam.h; nsf_update_kernel and adam_kernel both call it), fused steps counted as if
    they rounded twice: m': 1 - b1, two products, a sum: 3 u on either term; v': 1 - b2, three products, a sum: 4 u relative (all
    terms >= 0);
    bc = 1 - powf(b, step) on the host: powf within one ulp (2 u b^step), the difference u: relative e_bc = 2 u b^step / bc + u;
    denom = sqrtf(v') / sqrtf(bc2) + eps: (e_v / 2 + u) + (e_bc2 / 2 + u) + u for the quotient, u for the sum;
    step = (lr / bc1) (m' / denom): e_bc1 + u, the quotient u, the product u, plus e_m' over denom; p' = p - step: u |p'|."""
    d = lambda a: torch.as_tensor(np.asarray(a, np.float64)) if not torch.is_tensor(a) else a.double()
    p, g, m, v = d(p), d(g), d(m), d(v)
    lr, b1, b2, eps = float(lr), float(b1), float(b2), float(eps)
    pn, mn, vn = adam(p, g, m, v, step)
    e_m = gamma(3) * ((b1 * m).abs() + ((1 - b1) * g).abs())
    e_v = gamma(4) * vn
    ebc = lambda b: 2 * U * b ** step / (1 - b ** step) + U
    denom = vn.sqrt() / math.sqrt(1 - b2 ** step) + eps
    e_den = vn.sqrt() / math.sqrt(1 - b2 ** step) * (gamma(4) / 2 + 3 * U + ebc(b2) / 2) + U * denom
    scale = lr / (1 - b1 ** step)
    stp = scale * (mn / denom)
    e_stp = stp.abs() * (ebc(b1) + 3 * U + e_den / denom) * (1 + 1e-3) + scale * e_m / denom
    return dict(p=e_stp + U * (pn.abs() + e_stp) + TINY, m=e_m + TINY, v=e_v + TINY)


# ---- the cases -----------------------------------------------------------------------------------------------------------
_CACHE = {}


def mlp_grid():
    """the volume of the network cases: 72 x 72 x 24 cells of 0.25 m from (-9, -9, -3), window 9, trunc 2 m; 150 target points in
    x < 3 m, so that points beyond x = 5.5 m are further than trunc from all of them"""
    if "grid" not in _CACHE:
        g = torch.Generator().manual_seed(77)
        gr = grid((-9.0, -9.0, -3.0), 0.25, (72, 72, 24), 9, 2.0)
        t = (torch.rand(150, 3, generator=g) * torch.tensor([12.0, 18.0, 6.0]) + torch.tensor([-9.0, -9.0, -3.0])).float().numpy()
        t = t[mark_margin_ok(t, gr)]
        gr.targets = t
        gr.G = dt_brute(occupancy(t, gr), gr.window)
        _CACHE["grid"] = gr
    return _CACHE["grid"]


SPECIAL_DEAD = (-8.0, 0.25, 0.125)          # the fully dead row of a ``dead`` parameter set
CAP = 4                                     # candidates drawn per point kept, at most


def _admit(params, x, gr):
    """which rows of x [c, 4] keep every discrete decision at least twice its bound from its threshold, in float64 alone"""
    zs, out = forward(params, x)
    E, e_out = forward_bounds(params, x, zs)
    ok = relu_margin_ok(zs, E)
    if gr is not None:
        x64 = x.double()
        ep = e_out[:, :3] + U * (x64[:, :3].abs() + out[:, :3].abs() + e_out[:, :3])
        lk = lookup(x64[:, :3] + out[:, :3], gr)
        eu, eD, _ = lookup_bound(lk, gr, ep=ep)
        ok &= lookup_margin_ok(lk, gr, eu, eD)
    return ok


def mlp_case(n, n_hidden, dead=False, seed=0, objective=True, extra=None):
    """n admitted points (module docstring), uniform in x, y within +-10 m (a fifth outside the volume) and z within +-2.5 m, with
    ``extra`` [k, 3] constructed points first (kept unconditionally: threshold cases) and, for a dead set, SPECIAL_DEAD next (it
    must pass like any other); the reference iteration and every bound.  Cached."""
    key = (n, n_hidden, dead, seed, objective, None if extra is None else tuple(map(tuple, np.asarray(extra).tolist())))
    if key in _CACHE:
        return _CACHE[key]
    params = mlp_params(seed, n_hidden, dead)
    gr = mlp_grid() if objective else None
    g = torch.Generator().manual_seed(7919 * seed + 31 * n + n_hidden)
    rows = [] if extra is None else [torch.as_tensor(np.asarray(extra, np.float32)).reshape(-1, 3)]
    have, drawn, first = sum(len(r) for r in rows), 0, True
    while have < n and drawn < CAP * n:
        c = min(max(2 * (n - have), 4), CAP * n - drawn)
        cand = ((torch.rand(c, 3, generator=g) * 2 - 1) * torch.tensor([10.0, 10.0, 2.5])).float()
        if dead and first and c > 1:
            cand[0] = torch.tensor(SPECIAL_DEAD)
        first = False
        drawn += c
        ok = _admit(params, torch.cat([cand, torch.zeros(c, 1)], 1), gr)
        rows.append(cand[ok][: n - have])
        have += len(rows[-1])
    pts = torch.cat(rows)[:n] if rows else torch.zeros(0, 3)
    assert len(pts) == n, f"only {len(pts)} of {n} points admitted from {drawn} candidates: a derived margin is too loose"
    x = torch.zeros(padded_rows(n), 4)
    x[:n, :3] = pts
    case = SimpleNamespace(n=n, n_hidden=n_hidden, params=params, grid=gr, x=x, drawn=drawn, dead=dead, seed=seed)
    if objective:
        finish_case(case)
    _CACHE[key] = case
    return case


def finish_case(case, dout=None):
    """reference, float32 twin and bounds of ``case`` (with an external dout [n_pad, 4] when given)"""
    p, x, n, gr = case.params, case.x, case.n, case.grid
    case.ref = ref = iteration(p, x, n, gr, dout=dout)
    case.ref32 = iteration(p, x, n, gr, torch.float32, dout=dout)
    case.E, case.e_out = forward_bounds(p, x, ref["zs"])
    e_dout = None
    if dout is None:
        x64 = x.double()
        ep = case.e_out[:, :3] + U * (x64[:, :3].abs() + ref["out"][:, :3].abs() + case.e_out[:, :3])
        eu, eD, eg = lookup_bound(ref["look"], gr, ep=ep)
        real = (torch.arange(len(x)) < n)
        case.e_dsum = float(torch.where(ref["look"]["keep"] & real, eD, torch.zeros_like(eD)).sum()) + 1e-15 * abs(ref["dsum"]) + TINY
        e_dout = torch.cat([torch.where(real[:, None], eg, torch.zeros_like(eg)), torch.zeros(len(x), 1, dtype=F64)], 1)
        case.lookup_ok = lookup_margin_ok(ref["look"], gr, eu, eD)
    case.e_dout = e_dout
    case.e_grads, case.e_g = backward_bounds(p, x, ref, case.E, e_dout)
    return case


def flat(params_or_grads):
    """the flat parameter vector's layout (himo_amd/fastnsf.py _load): per layer W then b -> (vector, off_w, off_b)"""
    parts, off_w, off_b, o = [], [], [], 0
    for w, b in params_or_grads:
        off_w.append(o)
        o += w.numel()
        off_b.append(o)
        o += b.numel()
        parts += [w.reshape(-1), b.reshape(-1)]
    return torch.cat(parts), off_w, off_b


# ---- decisions AT a threshold: exactly representable inputs (cell 1/4, integer origin, trunc 1/2) ------------------------
def threshold_grid():
    """8 x 8 x 8 cells of 0.25 m from (-1, -1, -1), window 3, trunc 0.5; one target in cell (3, 3, 3): G = 4 at cell (5, 3, 3)"""
    gr = grid((-1.0, -1.0, -1.0), 0.25, (8, 8, 8), 3, 0.5)
    gr.targets = np.asarray([[-0.125, -0.125, -0.125]], np.float32)          # the centre of cell (3, 3, 3)
    gr.G = dt_brute(occupancy(gr.targets, gr), gr.window)
    return gr


def threshold_points():
    """name -> point.  u = (p + 1) / 0.25 - 0.5, so p = -1 + 0.25 (u + 0.5):
    u_x exactly 0 and exactly n - 1 = 7 (outside), u an exact integer strictly inside (base cell = that integer, f = 0; D = the
    cell's own value), the centre of cell (5, 3, 3) where G = 4: D = 2 cells = 0.5 = trunc exactly (counted, with a gradient)"""
    c = lambda ux, uy, uz: [-1 + 0.25 * (ux + 0.5), -1 + 0.25 * (uy + 0.5), -1 + 0.25 * (uz + 0.5)]
    return dict(u_zero=c(0, 3, 3), u_last=c(7, 3, 3), u_integer=c(4, 3, 3), d_is_trunc=c(5, 3, 3), ordinary=c(3.5, 3.25, 2.75))


MASK_ZERO_BIAS = (1, 2, 40, 100)


def mask_threshold_case(n_hidden=2, seed=3):
    """a real point at the origin, in the volume and within trunc of a target, with first-layer biases MASK_ZERO_BIAS exactly 0:
    z = fma(0, w, ... 0 * w) + 0 = 0 exactly in either precision, the mask bit is clear, the unit passes no gradient.  Three
    admitted points follow it."""
    key = ("mask", n_hidden, seed)
    if key in _CACHE:
        return _CACHE[key]
    params = mlp_params(seed, n_hidden)
    for j in MASK_ZERO_BIAS:
        params[0][1][j] = 0.0
    gr = mlp_grid()
    g = torch.Generator().manual_seed(seed)
    pts = [torch.zeros(1, 3)]
    drawn = 0
    while sum(len(p) for p in pts) < 4 and drawn < 64:
        cand = ((torch.rand(8, 3, generator=g) * 2 - 1) * torch.tensor([6.0, 6.0, 2.0])).float()
        drawn += 8
        pts.append(cand[_admit(params, torch.cat([cand, torch.zeros(8, 1)], 1), gr)])
    pts = torch.cat(pts)[:4]
    x = torch.zeros(padded_rows(4), 4)
    x[:4, :3] = pts
    case = finish_case(SimpleNamespace(n=4, n_hidden=n_hidden, params=params, grid=gr, x=x, drawn=drawn, dead=False, seed=seed))
    _CACHE[key] = case
    return case


# ---- the case tables (shared by tests/test_nsf_oracle.py and tests/test_nsf_conformance_gpu.py) ---------------------------------
# (n, n_hidden, dead set): every n of {1, 63, 64, 65, 255, 256, 257, 321} and every n_hidden of {1, 2, 8, 12}; the twelve-layer
# network at the tile tail, the eight-layer one at a full tile and at two backward blocks
FWD_CASES = ((1, 1, False), (63, 2, True), (64, 8, True), (65, 12, False), (255, 2, False), (256, 1, False), (257, 8, False), (321, 2, True))
BWD_CASES = ((1, 2, False), (63, 2, True), (64, 8, True), (65, 12, False), (255, 2, False), (256, 2, True), (257, 8, False), (321, 2, True))

# dims, window, cell, targets: every nx of {1, 2, 255, 256, 257, 300}, every ny and nz of {1, 2, 63, 64, 65}, every window of
# {1, 3, 21, 40}, windows larger than a dimension, both cells, every kind of target
DT_CASES = (((1, 1, 1), 1, 0.25, "one"), ((2, 2, 2), 3, 0.1, "full"), ((255, 63, 1), 21, 0.1, "sparse"), ((256, 1, 64), 40, 0.25, "faces"),
            ((257, 65, 2), 3, 0.1, "sparse"), ((300, 2, 65), 21, 0.25, "nan_neg"), ((2, 64, 63), 40, 0.1, "one"),
            ((1, 65, 64), 1, 0.25, "sparse"), ((256, 2, 1), 1, 0.25, "empty"), ((255, 1, 2), 3, 0.25, "full"))
DT_ORIGIN = (-3.0, 2.0, -1.0)
# (index into DT_CASES, n, with NaN points): every n of {0, 1, 255, 256, 257, 1000}; case 2 has nz = 1: no point is in the volume
DT_LOSS_CASES = ((4, 0, False), (4, 1, False), (2, 255, False), (5, 256, False), (6, 257, False), (4, 1000, True))


def dt_case(i):
    """DT_CASES[i] -> grid with .targets (float32 [k, 3], every dt_mark decision clear of its threshold) and .G (brute force);
    trunc = 0.6 window cells"""
    key = ("dt", i)
    if key in _CACHE:
        return _CACHE[key]
    dims, window, cell, kind = DT_CASES[i]
    gr = grid(DT_ORIGIN, cell, dims, window, 0.6 * window * cell)
    g = torch.Generator().manual_seed(500 + i)
    o, c = gr.origin.astype(np.float64), float(gr.cell)
    ext = np.asarray(dims, np.float64) * c
    mid = o + (np.asarray(dims) // 2 + 0.5) * c
    rnd = lambda k: (o + torch.rand(k, 3, generator=g).numpy().astype(np.float64) * ext).astype(np.float32)
    if kind == "empty":
        t = np.zeros((0, 3), np.float32)
    elif kind == "one":
        t = mid[None].astype(np.float32)
    elif kind == "full":
        idx = np.indices(dims).reshape(3, -1).T
        t = (o + (idx + 0.5) * c).astype(np.float32)
    elif kind == "faces":                                    # on the near faces (cell 0: kept) and on the far faces (cell n: dropped)
        t = []
        for a in range(3):
            for far in (0, 1):
                p = mid.copy()
                p[a] = o[a] + far * ext[a]
                t.append(p)
        t = np.asarray(t + [o, o + ext], np.float32)
    else:
        t = np.concatenate([rnd(40), (o - torch.rand(6, 3, generator=g).numpy() * ext).astype(np.float32)])      # (the last six: negative side)
        if kind == "nan_neg":
            nan = rnd(4)
            nan[0, :] = np.nan
            nan[1, 0] = np.nan
            nan[2, 1] = np.nan
            nan[3, 2] = np.nan
            t = np.concatenate([nan[:2], t, nan[2:]])
    if kind != "faces":                                      # (the faces are AT the threshold on purpose: cell 1/4 and an integer
        t = t[mark_margin_ok(t, gr)]                         # origin make their quotient exact in float32)
    gr.targets, gr.kind = t, kind
    gr.G = dt_brute(occupancy(t, gr), window)
    _CACHE[key] = gr
    return gr


def dt_points(gr, n, seed=0, nan=False):
    """n float32 points for himo_dt_loss: half uniform over the box grown by a tenth (some outside), half near a target, every lookup decision clear of
    its threshold (from at most CAP n candidates); nan: every 97th point has a NaN coordinate"""
    g = torch.Generator().manual_seed(900 + seed + n)
    o, ext = gr.origin.astype(np.float64), np.asarray(gr.dims, np.float64) * float(gr.cell)
    rows, have, drawn = [], 0, 0
    while have < n and drawn < CAP * n:
        c = min(max(2 * (n - have), 4), CAP * n - drawn)
        cand = torch.from_numpy((o - 0.1 * ext + torch.rand(c, 3, generator=g).numpy() * 1.2 * ext).astype(np.float32))
        tg = gr.targets[~np.isnan(gr.targets).any(1)]
        if len(tg):                                          # every other candidate within about a window of a target: D below trunc
            pick = torch.randint(len(tg), (c,), generator=g).numpy()
            near = tg[pick] + torch.randn(c, 3, generator=g).numpy() * 0.4 * gr.window * float(gr.cell)
            cand[::2] = torch.from_numpy(near.astype(np.float32))[::2]
        drawn += c
        lk = lookup(cand, gr)
        eu, eD, _ = lookup_bound(lk, gr)
        rows.append(cand[lookup_margin_ok(lk, gr, eu, eD)][: n - have])
        have += len(rows[-1])
    pts = torch.cat(rows) if rows else torch.zeros(0, 3)
    assert len(pts) == n, f"only {len(pts)} of {n} lookup points admitted from {drawn} candidates"
    if nan:
        pts[::97, 1] = float("nan")
    return pts, drawn


def verdict(arith, got, ref, bnd, ref32, case, limit=None, cols=False):
    """both levels -> (passed, worst err / bound, rms ratio, report).  cols: a gradient whose last axis is an output channel
    (grad_oracle.check_cols' per-column scaling); otherwise head_oracle.verdict (bit equality where the bound is zero, the
    aggregate level from 128 outputs on)"""
    if cols:
        worst, rr, report = go.check_cols(got, ref, bnd, ref32, arith, case)
        return worst <= 1.0 and rr <= co.R[arith], worst, rr, report
    return ho.verdict(arith, got, ref, bnd, ref32, case, limit=limit)


def iteration_checks(case, got, scale=1.0):
    """every comparison of one iteration's results ``got`` (dict out [n_pad, 4], dout [n_pad, 4], dsum, m, grads [(dW, db)]
    unscaled; missing keys are skipped) with ``case``: (family, name, arith, got, ref, bound, float32 twin, cols)"""
    n, ref, r32 = case.n, case.ref, case.ref32
    out = []
    if "out" in got:
        out.append(("forward", "out", "f16x2", got["out"][:n], ref["out"][:n], case.e_out[:n] + TINY, r32["out"][:n], False))
    if "h_last" in got:
        out.append(("forward", "h_last", "f16x2", got["h_last"][:n], ref["zs"][-1][:n].clamp(min=0),
                    (case.E[-1] * (ref["zs"][-1] > 0))[:n] + TINY, r32["zs"][-1][:n].clamp(min=0), False))
    if "dout" in got:
        z = torch.zeros_like(ref["dout"])
        out.append(("objective", "dout", "f16x2", got["dout"], ref["dout"], case.e_dout + TINY * (case.e_dout > 0), r32["dout"], False))
        out.append(("objective", "dsum", "f16x2", torch.tensor([got["dsum"]]), torch.tensor([ref["dsum"]]), torch.tensor([case.e_dsum]), None, False))
        out.append(("objective", "count", "f16x2", torch.tensor([float(got["m"])]), torch.tensor([float(ref["m"])]), torch.zeros(1), None, False))
    for k, (gw, gb) in enumerate(got.get("grads", ())):
        if gw is None:
            continue
        last = k == len(ref["grads"]) - 1
        arith = "f16x2" if last else "bf16x2"
        fam = "last_grad" if last else "backward"
        (rw, rb), (ew, eb), (tw, tb) = ref["grads"][k], case.e_grads[k], r32["grads"][k]
        out.append((fam, f"dW{k}", arith, gw, rw * scale, ew * scale, tw.double() * scale, True))
        out.append((fam, f"db{k}", arith, gb, rb * scale, eb * scale, tb.double() * scale, False))
    return out


def dt_loss_checks(gr, pts, got, exact_u=False):
    """himo_dt_loss's results ``got`` (loss, grad [n, 3]) on pts: the gradient per point, the loss, and the count through loss x m"""
    ref, r32 = dt_objective(pts, gr), dt_objective(pts, gr, torch.float32)
    b = dt_objective_bound(ref, gr, exact_u)
    return [("dt_loss", "grad", "f32", got["grad"], ref["grad"], b["grad"] * (ref["look"]["keep"][:, None]), r32["grad"], False),
            ("dt_loss", "loss", "f32", torch.tensor([got["loss"]]), torch.tensor([ref["loss"]]), torch.tensor([b["loss"]]), None, False),
            ("dt_loss", "loss x m", "f32", torch.tensor([got["loss"] * ref["m"]]), torch.tensor([ref["dsum"]]), torch.tensor([b["dsum"]]), None, False)]


def last_grad_checks(case, dout, got_w, got_b):
    """himo_nsf_last_grad on an external dout [n_pad, 4] (an input: no error of its own): the tiles' dW_last [128, 4] and db_last
    [4], summed in float64 by the caller, against H_{L-1}^T dout with H_{L-1} within its forward bound"""
    z = case.ref["zs"][-1]
    h, eh, d = z.clamp(min=0), case.E[-1] * (z > 0), torch.as_tensor(dout).double()
    ew = eh.T @ d.abs() + gamma(40) * ((h + eh).T @ d.abs()) + TINY
    tw = case.ref32["zs"][-1].clamp(min=0).T @ torch.as_tensor(dout).float()
    return [("last_grad", "dW_last", "f16x2", got_w, h.T @ d, ew, tw.double(), True),
            ("last_grad", "db_last", "f16x2", got_b, d.sum(0), gamma(70) * d.abs().sum(0) + TINY, None, False)]


def threshold_network_case():
    """the lookup's threshold decisions THROUGH the fused forward kernel: one hidden layer and a last layer of zeros, so that
    out = 0 and moved = x + 0 = x exactly; x = threshold_points() on threshold_grid().  Only the forward pass and the objective are
    checked with it (no mask decides anything there: H and H^T dout are continuous in z)."""
    if "thr_net" not in _CACHE:
        params = mlp_params(5, 1)
        params[-1] = (torch.zeros_like(params[-1][0]), torch.zeros_like(params[-1][1]))
        pts = torch.tensor(list(threshold_points().values()))
        x = torch.zeros(padded_rows(len(pts)), 4)
        x[:len(pts), :3] = pts
        _CACHE["thr_net"] = finish_case(SimpleNamespace(n=len(pts), n_hidden=1, params=params, grid=threshold_grid(), x=x, drawn=0,
                                                        dead=False, seed=5))
    return _CACHE["thr_net"]
