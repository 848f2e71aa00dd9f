"""Float64 reference, float32 twin and a worst-case error model of the training-mode BatchNorm kernels (include/himo_amd.h:
himo_bn_train_fwd, himo_bn_train_bwd, himo_bn_train_bwd_x, himo_bn_fold; csrc/batchnorm.hip).  CPU only.  Conventions of
oracle/conv_oracle.py and oracle/grad_oracle.py: a per-output WORST-case bound against float64 plus an aggregate rms ratio
against the same operation in float32, here per channel scale (check_map: grad_oracle.check_cols with the limit R_ELEM).

The operation, over an [n_img][rows][ch] map of N = n_img rows rows (torch.nn.BatchNorm semantics followed by the exact-erf GELU):
    mean = sum x / N,  var = sum (x - mean)^2 / N  (biased),  invstd = 1 / sqrt(var + eps)
    running_mean <- (1 - m) running_mean + m mean,  running_var <- (1 - m) running_var + m var N / (N - 1)
    xhat = (x - mean) invstd,  y = gelu(gamma xhat + beta)
    g = dy gelu'(gamma xhat + beta),  dbeta = sum g,  dgamma = sum g xhat  (flags bit 0: added to the old values)
    dx = gamma invstd (g - mean(g) - xhat mean(g xhat))
    fold: scale = gamma / sqrt(var + eps),  shift = beta - mean scale
N = 1: torch refuses; the rule is the kernel's (batchnorm.hip:123-128): var = 0 and the running variance takes var unchanged.

The kernels' arrangement (what twin32 mirrors; u = 2^-24, D = 2^-53):
  statistics  bn_stats_partial_kernel (batchnorm.hip:66-83): float64 sums of x and of x x (the square is exact in float64);
              bn_stats_finalize_kernel (:115-133): var = ss / N - mean^2 in float64, clamped at 0; mean, invstd and the running
              pair each rounded ONCE to float32.
  forward     bn_normalize_gelu_kernel (:136-154): xhat = fl(fl(x - m) is) from the float32 m, is; t = gamma xhat + beta (one
              or two roundings: the file is compiled with the default contraction); y = gelu_exact(t) (conv_common.h:70-80).
  sums        bn_bwd_partial_kernel (:160-191): a thread's own rows, ceil(rows_pb / G) of them, in float32 (g added, g xhat by
              fmaf); everything across threads and blocks in float64 (bn_block_partials :50-63, bn_sum_partials :88-111).
  backward    bn_bwd_finalize_kernel (:194-207): k1 = fl(gamma is), k2 = fl(sum g / N), k3 = fl(sum g xhat / N);
              bn_bwd_apply_kernel (:212-241): dx = k1 ((g - k2) - xhat k3), g evaluated again.
  FROM_X      himo_bn_train_bwd_x re-forms xhat from x, m, is with the forward pass's expression: the same bits.
The twin's GELU and GELU' are torch's float32 erf and exp (about half a rounding), not the kernels' polynomial: the twin says
what float32 can do, the bound what the kernels may do.

Bound (per output, derived below in ``bound``; no constant is taken from a device run):
  float64 sums: a term passes through at most L64 = T + G + ceil(nb / 256) + 69 additions, T = ceil(rows_pb / G) its thread's own
      chain, G - 1 the groups of its block, ceil(nb / 256) + 3 its chain over the block partials, 2 + 64 the combine
      (``dispatch`` mirrors rows_pb, G and nb; never more than N - 1, adding a zero being exact).  With the division,
      d mean = (L64 + 2) D mean|x|; ss / N, mean^2 (twice the error of the mean, |mean| mean|x| <= mean(x^2)) and their
      difference give d var = (3 L64 + 9) D mean(x^2): the cancellation in ss / N - mean^2 is against mean(x^2).  N = 1:
      every step is exact.
  invstd: d is / is = d(var + eps) / (2 (var + eps - d)) + 4 D + u.
  xhat: the saved float32 mean is off by dm = u |mean| + d mean:  is (dm + u |x - mean|) + |xhat| (d is / is + u).
  t = gamma xhat + beta:  dt = |gamma| d xhat + 2 u (|gamma xhat| + |beta|).
  y: grad_oracle.elementwise_bound("affine_gelu_fwd") at t, plus conv_oracle.GELU_SLOPE dt + dt (ERF_AS + 16 u) / 2.
  g: grad_oracle.elementwise_bound("affine_gelu_bwd") at (dy, t), plus |dy| GELU2_MAX dt, GELU2_MAX = max |gelu''| =
      |phi(t) (2 - t^2)| at t = 0 = 2 / sqrt(2 pi).
  sums: the element errors add up; the thread's float32 chain rounds T - 1 times on g (T times on the fmaf chain of g xhat),
      u each, on at most the sum of the magnitudes; L64 D of that for the float64 part; u |sum| for the float32 result;
      the accumulate flag adds u (|old| + |new|).
  dx: the three coefficients carry the errors of the sums (/ N) and one rounding each; the expression rounds four times.
Thresholds the matrix keeps away from (``facts``): var + eps - d(var + eps) > 0, and |t| + dt < T_EXP = 13: from |t| = 13.2 on
exp(-t^2 / 2) leaves float32's normal range, and the relative exponential term of the GELU' budget assumes a normal number.
GELU itself has no threshold: both device forms are continuous at 0 and saturate smoothly.

Observed on an MI355X (information only -- no constant here was chosen from it): worst err/bound and worst rms ratio (R_ELEM 32)
per output from the module summary of tests/test_bn_conformance_gpu.py, 25 cases (running statistics: 21), bn_fold 10:
    mean          0.999, 0.312  (the final rounding of the float64 mean: at most u |mean| by construction)
    invstd        0.968, 0.412         running_mean  0.974, 0.312         running_var   0.975, 0.326
    xhat          0.914, 0.996         y             0.501, 1.3           dbeta         0.908, 1.15
    dgamma        0.631, 1             dx            0.393, 0.995         fold scale    0.753, 0.421
    fold shift    0.541, 0.44
    Every kernel of batchnorm.hip met: the partial kernels at qs = 3, 4, 5 (statistics and both FROM_X instantiations), both
    apply kernels, the normalise kernel with and without xhat, the finalize kernels with accumulate 0 and 1, bn_fold; block
    counts 1, 2, 5, 16, 64, 65, 129, 193, 257, 683; 87 refusals, each with the status read from the source.  No case outside
    its bound, every rerun and every himo_bn_train_bwd_x result bit-identical.  (total = 1: dx comes out a few 1e-3 of its bound
    instead of exactly 0 -- the g the apply kernel evaluates again and the g the partial kernel summed do not agree to the last
    bit there; the file is compiled with contraction, so the product dy gelu' may enter the sum unrounded.)
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import grad_oracle as go
from conv_oracle import U, GELU_SLOPE, ERF_AS, check  # noqa: F401  (re-exported for the tests)
from grad_oracle import R_ELEM, MIN_AGGREGATE, TINY   # noqa: F401

D = 2.0 ** -53                                        # float64 unit roundoff
GELU2_MAX = 2.0 / math.sqrt(2.0 * math.pi)            # max |gelu''(t)| = |phi(t) (2 - t^2)|, at t = 0
T_EXP = 13.0                                          # exp(-t^2 / 2) >= 2^-126 up to |t| = sqrt(252 ln 2) = 13.2
BN_EPS, BN_EPS_PFN = 1e-5, 1e-3                       # himo_amd/seflow/spec.py (the tests assert they still agree)
OUTPUTS_FWD = ("mean", "invstd", "running_mean", "running_var", "xhat", "y")
OUTPUTS_BWD = ("dbeta", "dgamma", "dx")


def _f32(v):
    return float(np.float32(v))


def dispatch(total, ch):
    """What the host code launches for ``total`` rows of ``ch`` channels."""
    qs = 5 if ch > 64 else (4 if ch > 32 else 3)              # bn_quad_shift, batchnorm.hip:47
    G = 256 >> qs                                             # row groups of a block, batchnorm.hip:68, :165
    r = (total + 1023) // 1024                                # bn_rows_per_block, batchnorm.hip:254-258
    r = (r + 31) // 32 * 32
    rows_pb = max(64, r)
    nb = (total + rows_pb - 1) // rows_pb                     # batchnorm.hip:289, :346
    T = (rows_pb + G - 1) // G                                # a thread's own rows, batchnorm.hip:76, :177
    return dict(qs=qs, G=G, rows_pb=rows_pb, nb=nb, tiles=(ch + 127) // 128, T=T,
                L64=T + G + (nb + 255) // 256 + 69,           # batchnorm.hip:60, :97-108
                four_chain_trips=(nb - 192 + 255) // 256 if nb > 192 else 0)      # of group 0, batchnorm.hip:97


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def _gelu(t):
    return go._gelu(t)


def _gelu_grad(t):
    return go._gelu_grad(t)


def fold(gamma, beta, mean, var, eps, dtype=torch.float64):
    """himo_bn_fold in ``dtype`` (float32: every operation rounded once, the twin)"""
    gamma, beta, mean, var = (torch.as_tensor(v).to(dtype) for v in (gamma, beta, mean, var))
    e = torch.tensor(_f32(eps), dtype=dtype)
    scale = gamma / torch.sqrt(var + e)
    return scale, beta - mean * scale


def reference(c):
    """every output of the three entry points in float64 -> dict"""
    x, dy = c["x"].double(), c["dy"].double()
    gamma, beta = c["gamma"].double(), c["beta"].double()
    N = x.shape[0]
    eps, m = _f32(c["eps"]), _f32(c["momentum"])
    mean = x.mean(0)
    var = (x - mean).pow(2).mean(0) if N > 1 else torch.zeros_like(mean)
    invstd = 1.0 / torch.sqrt(var + eps)
    unbiased = var * N / (N - 1) if N > 1 else var
    out = dict(mean=mean, var=var, invstd=invstd)
    if c["rm"] is not None:
        out["running_mean"] = (1.0 - m) * c["rm"].double() + m * mean
        out["running_var"] = (1.0 - m) * c["rv"].double() + m * unbiased
    xhat = (x - mean) * invstd
    t = gamma * xhat + beta
    g = dy * _gelu_grad(t)
    sg, sgx = g.sum(0), (g * xhat).sum(0)
    acc = bool(c["flags"] & 1)
    out.update(xhat=xhat, t=t, y=_gelu(t), g=g, sg=sg, sgx=sgx,
               dbeta=sg + (c["old_dbeta"].double() if acc else 0), dgamma=sgx + (c["old_dgamma"].double() if acc else 0),
               dx=gamma * invstd * (g - sg / N - xhat * (sgx / N)))
    fm, fv = (out["running_mean"], out["running_var"]) if c["rm"] is not None else (mean, var)
    out["scale"], out["shift"] = fold(gamma, beta, fm, fv, eps)
    return out


# ---- float32 twin (and its wrong variants) ----------------------------------------------------------------------------------
def _r32(v):
    return v.to(torch.float32)


def _fma32(a, b, c):
    """fl32(a b + c): the product of two float32 is exact in float64, the sum then rounds to 53 bits and to 24"""
    return _r32(a.double() * b.double() + c.double())


def _gelu_grad_tanh(t):
    """d/dt of the tanh approximation of GELU (a wrong kernel's)"""
    k = math.sqrt(2.0 / math.pi)
    inner = k * (t + 0.044715 * t ** 3)
    th = torch.tanh(inner)
    return 0.5 * (1 + th) + 0.5 * t * (1 - th * th) * k * (1 + 3 * 0.044715 * t * t)


def _thread_sums(g, h, d, drop_last):
    """sum g and sum g h the kernels' way: thread (block b, group j) owns rows b rows_pb + j + k G, summed in float32 (g h by
    fmaf); threads and blocks in float64"""
    N, ch = g.shape
    rows_pb, G, nb = d["rows_pb"], d["G"], d["nb"]
    pad = nb * rows_pb - N
    z = torch.zeros(pad, ch, dtype=torch.float32)
    gp = torch.cat([g, z]).reshape(nb, rows_pb // G, G, ch)
    hp = torch.cat([h, z]).reshape(nb, rows_pb // G, G, ch)
    if drop_last and nb > 1:
        gp, hp = gp[:-1], hp[:-1]
    fs = torch.zeros(gp.shape[0], G, ch, dtype=torch.float32)
    fx = torch.zeros_like(fs)
    for k in range(rows_pb // G):
        fs = fs + gp[:, k]
        fx = _fma32(gp[:, k], hp[:, k], fx)
    return fs.double().sum((0, 1)), fx.double().sum((0, 1))


def _stats64(x, N):
    """float64 sums of the float32 values: mean and the clamped single-pass variance"""
    xd = x.double()
    mean = xd.sum(0) / N
    var = ((xd * xd).sum(0) / N - mean * mean).clamp(min=0.0)
    return mean, var


def twin32(c, wrong=None):
    """The same outputs computed in the kernels' arrangement with float32 where they use float32 (module docstring).
    ``wrong``: a key of WRONG -- the twin with one plausible kernel bug."""
    assert wrong is None or wrong in WRONG, wrong
    x, dy = c["x"], c["dy"]
    gamma, beta = c["gamma"], c["beta"]
    N, ch = x.shape
    n_img, rows = c["n_img"], c["rows"]
    d = dispatch(N, ch)
    eps, m = _f32(c["eps"]), _f32(c["momentum"])
    drop = wrong == "last partial row block dropped"
    xs = x[:(N - 1) // d["rows_pb"] * d["rows_pb"]] if (drop and d["nb"] > 1) else x
    if wrong == "single-pass variance in float32":
        s = torch.from_numpy(np.add.accumulate(xs.numpy(), axis=0)[-1].copy())
        ss = torch.from_numpy(np.add.accumulate((xs * xs).numpy(), axis=0)[-1].copy())
        mean = s / np.float32(N)
        var = (ss / np.float32(N) - mean * mean).clamp(min=0.0).double()
        mean = mean.double()
    elif wrong == "statistics per image":
        mean, var = _stats64(x[:rows], rows)
    else:
        mean, var = _stats64(xs, N)
    nvar = var * N / (N - 1) if (wrong == "unbiased variance normalises" and N > 1) else var
    invstd = 1.0 / (torch.sqrt(nvar) + eps) if wrong == "eps outside the square root" else 1.0 / torch.sqrt(nvar + eps)
    m32, is32 = _r32(mean), _r32(invstd)
    out = dict(mean=m32, invstd=is32)
    if c["rm"] is not None:
        unbiased = var * N / (N - 1) if (N > 1 and wrong != "biased variance feeds the running estimate") else var
        a, b = (m, 1.0 - m) if wrong == "momentum on the wrong term" else (1.0 - m, m)
        out["running_mean"] = _r32(a * c["rm"].double() + b * mean)
        out["running_var"] = _r32(a * c["rv"].double() + b * unbiased)
    cm, ci, cg, cb = m32.clone(), is32.clone(), gamma.clone(), beta.clone()
    if wrong == "one quad of channels shifted by four":       # the last quad reads its constants one quad off
        q = ch // 4 - 1
        src = q - 1 if q > 0 else q
        lo, so = 4 * q, 4 * src
        if q == 0:                                            # a single quad: rotate within it
            for v in (cm, ci, cg, cb):
                v[:] = torch.roll(v, 1)
        else:
            for v in (cm, ci, cg, cb):
                v[lo:lo + 4] = v[so:so + 4].clone()
    if wrong == "statistics per image":                       # every image normalised by its own statistics
        parts = [_stats64(x[i * rows:(i + 1) * rows], rows) for i in range(n_img)]
        mm = torch.stack([_r32(p[0]) for p in parts]).repeat_interleave(rows, 0)
        ii = torch.stack([_r32(1.0 / torch.sqrt(p[1] + eps)) for p in parts]).repeat_interleave(rows, 0)
        h = (x - mm) * ii
    else:
        h = (x - cm) * ci
    t = _fma32(cg, h, cb)
    y = _r32(0.5 * t * (1.0 + torch.erf(t * np.float32(1.0 / math.sqrt(2.0)))))
    gp = _r32(_gelu_grad_tanh(t.double())) if wrong == "tanh-GELU derivative" else _gelu_grad(t)
    g = dy * gp
    sg, sgx = _thread_sums(g, x if wrong == "dgamma from x" else h, d, drop)
    acc = bool(c["flags"] & 1) and wrong != "accumulate overwrites"
    out.update(xhat=h, y=y, dbeta=_r32(sg) + (c["old_dbeta"] if acc else 0), dgamma=_r32(sgx) + (c["old_dgamma"] if acc else 0))
    k1, k2, k3 = cg * ci, _r32(sg / N), _r32(sgx / N)
    if wrong == "dx without mean(g)":
        k2 = torch.zeros_like(k2)
    if wrong == "dx without xhat mean(g xhat)":
        k3 = torch.zeros_like(k3)
    out["dx"] = k1 * _fma32(-h, k3.expand_as(h), g - k2)
    fm, fv = (out["running_mean"], out["running_var"]) if c["rm"] is not None else (m32, _r32(var))
    out["scale"], out["shift"] = fold(gamma, beta, fm, fv, eps, torch.float32)
    return out


WRONG = ("unbiased variance normalises", "biased variance feeds the running estimate", "momentum on the wrong term",
         "eps outside the square root", "statistics per image", "last partial row block dropped", "single-pass variance in float32",
         "dx without mean(g)", "dx without xhat mean(g xhat)", "dgamma from x", "tanh-GELU derivative", "accumulate overwrites",
         "one quad of channels shifted by four")


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def _model(c, ref=None):
    """the intermediate error terms of the module docstring, all [ch] or [N, ch] float64"""
    ref = reference(c) if ref is None else ref
    x = c["x"].double()
    N, ch = x.shape
    d = dispatch(N, ch)
    L = min(d["L64"], N - 1)                                  # adding the zeros of idle lanes and chains is exact
    eps = _f32(c["eps"])
    ab = torch.abs
    mean, var, invstd, xhat, t = ref["mean"], ref["var"], ref["invstd"], ref["xhat"], ref["t"]
    one = 0 if N == 1 else 1                                  # N = 1: s / 1, x x, mean mean and their difference are all exact
    dmean = (L + 2 * one) * D * ab(x).mean(0)
    dvar = (3 * L + 9 * one) * D * (x * x).mean(0)
    v = var + eps
    dv = dvar + D * v
    rel_is = 0.5 * dv / (v - dv).clamp(min=1e-300) + 4 * D + U
    dm = U * ab(mean) + dmean
    dh = (invstd * (dm + U * ab(x - mean)) + ab(xhat) * (rel_is + U)) * (1 + 8 * U) + TINY
    dt = ab(c["gamma"].double()) * dh + 2 * U * (ab(c["gamma"].double() * xhat) + ab(c["beta"].double()))
    return dict(ref=ref, d=d, dmean=dmean, dvar=dvar, v=v, dv=dv, rel_is=rel_is, dh=dh, dt=dt)


def bound(c, ref=None):
    """per-output worst case of |kernel - reference(c)| for every output of the forward and backward entry points"""
    mo = _model(c, ref)
    ref, d = mo["ref"], mo["d"]
    x, dy = c["x"].double(), c["dy"].double()
    gamma = c["gamma"].double()
    N = x.shape[0]
    L, T = min(d["L64"], N - 1), min(d["T"], N)
    m = _f32(c["momentum"])
    ab = torch.abs
    mean, var, invstd, xhat, t, g = ref["mean"], ref["var"], ref["invstd"], ref["xhat"], ref["t"], ref["g"]
    dh, dt = mo["dh"], mo["dt"]
    dis = invstd * mo["rel_is"]
    out = dict(mean=U * ab(mean) + mo["dmean"] + TINY, invstd=dis + TINY, xhat=dh)
    if c["rm"] is not None:
        rm, rv = c["rm"].double(), c["rv"].double()
        unb_f = N / (N - 1) if N > 1 else 1.0
        out["running_mean"] = U * ab(ref["running_mean"]) + m * mo["dmean"] + 4 * D * (ab((1 - m) * rm) + ab(m * mean)) + TINY
        out["running_var"] = U * ab(ref["running_var"]) + m * unb_f * mo["dvar"] + 4 * D * (ab((1 - m) * rv) + ab(m * unb_f * var)) + TINY
    # y and g: the budgets of the affine-GELU kernels at the exact t, plus the slope times the error of t
    out["y"] = go.elementwise_bound("affine_gelu_fwd", x=t)["y"] + GELU_SLOPE * dt + 0.5 * dt * (ERF_AS + 16 * U)
    bg = (go.elementwise_bound("affine_gelu_bwd", dy=dy, pre=t)["dx"] + ab(dy) * GELU2_MAX * dt) * (1 + 8 * U)
    # the sums, before their float32 result is rounded
    Sg, Sbg = ab(g).sum(0), bg.sum(0)
    e_sg = Sbg + (T - 1) * U * (1 + T * U) * (Sg + Sbg) + L * D * (Sg + Sbg)
    egh = ab(xhat) * bg + ab(g) * dh + bg * dh
    Sgh, Segh = ab(g * xhat).sum(0), egh.sum(0)
    e_sgx = Segh + T * U * (1 + T * U) * (Sgh + Segh) + L * D * (Sgh + Segh)
    sg, sgx = ref["sg"], ref["sgx"]
    out["dbeta"] = e_sg + U * (ab(sg) + e_sg) + TINY
    out["dgamma"] = e_sgx + U * (ab(sgx) + e_sgx) + TINY
    if c["flags"] & 1:                                          # one rounding of old + new
        out["dbeta"] = out["dbeta"] + U * (ab(c["old_dbeta"].double()) + ab(sg) + e_sg)
        out["dgamma"] = out["dgamma"] + U * (ab(c["old_dgamma"].double()) + ab(sgx) + e_sgx)
    # dx = k1 ((g - k2) - xhat k3)
    k1, k2, k3 = gamma * invstd, sg / N, sgx / N
    dk1 = ab(gamma) * dis + U * ab(k1)
    dk2 = e_sg / N + (U + 2 * D) * ab(k2)
    dk3 = e_sgx / N + (U + 2 * D) * ab(k3)
    inner = g - k2 - xhat * k3
    e_in = bg + dk2 + U * ab(g - k2) + ab(xhat) * dk3 + ab(k3) * dh + dh * dk3 + U * ab(xhat * k3) + U * ab(inner)
    out["dx"] = (ab(k1) * e_in + ab(inner) * dk1 + dk1 * e_in + U * ab(ref["dx"])) * (1 + 8 * U) + TINY
    return out


def fold_bound(gamma, beta, mean, var, eps):
    """scale = gamma / sqrtf(var + eps) rounds three times, the sum entering the root at half weight: 2.5 u, held to 3 u
    relative.  shift = beta - mean scale is two more float32 operations on that scale: it carries the scale's 3 u through
    |mean| and rounds the product and the difference, 3 u |mean scale| + u |mean scale| + u |shift|.  (3 u of its own
    magnitude |beta| + |mean scale| is not derivable: the correctly rounded float32 formula itself reaches 3.2 u of it,
    tests/test_bn_oracle.py.)"""
    s, h = fold(gamma, beta, mean, var, eps)
    ms = (torch.as_tensor(mean).double() * s).abs()
    return 3 * U * s.abs() + TINY, 4 * U * ms + U * h.abs() + TINY


def facts(c, ref=None):
    """the thresholds a case must stay away from -> (min over channels of var + eps - d(var + eps), max of |t| + dt)"""
    mo = _model(c, ref)
    return float((mo["v"] - mo["dv"]).min()), float((mo["ref"]["t"].abs() + mo["dt"]).max())


# ---- the two-level check, per channel scale --------------------------------------------------------------------------------------
def check_map(got, ref, bnd, ref32, case=""):
    """conv_oracle.check on an output whose LAST axis is the channel (a [ch] vector is a one-row map): every channel divided
    by the rms of its own bound first, as grad_oracle.check_cols does -- the channels of one map span eight decades here
    (``cases``) -- and the aggregate level, R_ELEM against the twin, taken from MIN_AGGREGATE outputs on."""
    got, ref, bnd = torch.as_tensor(got).double(), torch.as_tensor(ref).double(), torch.as_tensor(bnd).double()
    ch = ref.shape[-1]
    got, ref, bnd = got.reshape(-1, ch), ref.reshape(-1, ch), bnd.reshape(-1, ch)
    s = bnd.pow(2).mean(0).sqrt().clamp(min=1e-290)
    r32 = None if (ref32 is None or ref.numel() < MIN_AGGREGATE) else torch.as_tensor(ref32).double().reshape(-1, ch) / s
    return check(got / s, ref / s, bnd / s, r32, "f32", case, limit=R_ELEM)


def ok_map(got, ref, bnd, ref32, case=""):
    worst, rr, report = check_map(got, ref, bnd, ref32, case)
    assert worst <= 1.0, report
    assert rr <= R_ELEM, report
    return worst, rr


# ---- the conformance matrix (shared by tests/test_bn_oracle.py and tests/test_bn_conformance_gpu.py) --------------------------
# name -> (n_img, rows, ch, layout, statistics, eps, momentum, flags, running statistics given)
# layouts (tests/test_bn_conformance_gpu.py builds them): dense; pitch4 / pitch32: x, y, dx at ch + 4 (ch + 32), xhat, dy at
# ch + 32 (ch + 4); gap: 8 floats between the images of x, y, dy; concat: y (forward) and dy (backward) as channel groups of
# one buffer (img_stride = ch, pitch = n_img ch), the rest dense; alias_xhat: xhat written over x; alias_dx: dx over dy.
MATRIX = {
    "t1 c4":          (1, 1, 4, "dense", "unit", BN_EPS, 0.1, 0, True),          # total = 1: var = 0, running var takes it
    "t1 c132":        (1, 1, 132, "pitch4", "edge", BN_EPS, 0.1, 1, True),
    "t2 c8":          (2, 1, 8, "dense", "edge", BN_EPS, 0.1, 0, True),
    "t63 c32":        (1, 63, 32, "pitch4", "edge", BN_EPS, 0.1, 0, True),
    "t64 c36":        (1, 64, 36, "pitch32", "unit", BN_EPS_PFN, 0.1, 0, True),
    "t65 c64":        (5, 13, 64, "gap", "edge", BN_EPS, 0.1, 0, True),          # 2 blocks, the second one row; rows < G = 16
    "t65 c68":        (1, 65, 68, "dense", "edge", BN_EPS, 1.0, 1, True),
    "b193 c36":       (2, 6176, 36, "concat", "edge", BN_EPS, 0.1, 0, True),     # 193 blocks: the four-chain loop's first trip
    "b257 c8":        (5, 3277, 8, "dense", "unit", BN_EPS, 0.1, 1, False),      # 257 blocks: tail and second trip meet
    "b257 c4":        (1, 16385, 4, "pitch32", "edge", BN_EPS_PFN, 1.0, 0, True),
    "b683 c36":       (1, 65537, 36, "dense", "unit", BN_EPS, 0.1, 0, True),     # rows_pb = 96, 683 blocks
    "b683 c32":       (1, 65537, 32, "alias_dx", "edge", BN_EPS, 0.1, 1, False),
    "s50x1 c128":     (50, 1, 128, "concat", "edge", BN_EPS, 0.1, 0, True),      # rows < G = 8
    "s40x3 c64":      (40, 3, 64, "gap", "edge", BN_EPS, 1.0, 0, True),          # rows < G = 16
    "s40x3 c4":       (40, 3, 4, "concat", "edge", BN_EPS_PFN, 0.1, 1, True),    # rows < G = 32
    "s7x9 c32":       (7, 9, 32, "concat", "unit", BN_EPS, 0.1, 0, False),       # rows < G = 32
    "s7x9 c132":      (7, 9, 132, "pitch4", "edge", BN_EPS, 0.1, 0, True),       # a second tile holding a single quad
    "s3x32 c8":       (3, 32, 8, "gap", "unit", BN_EPS, 0.1, 1, True),           # rows == G
    "s2x4099 c36":    (2, 4099, 36, "pitch32", "edge", BN_EPS, 0.1, 0, False),   # rows prime
    "w4097 c256":     (1, 4097, 256, "dense", "edge", BN_EPS, 0.1, 0, True),
    "w1023 c128":     (3, 341, 128, "alias_xhat", "edge", BN_EPS, 0.1, 0, True),
    "w300 c68":       (3, 100, 68, "alias_dx", "edge", BN_EPS_PFN, 0.1, 1, True),
    "w66 c256":       (2, 33, 256, "pitch32", "edge", BN_EPS_PFN, 1.0, 0, True),
    "shifted mean":   (2, 2048, 32, "dense", "shifted", BN_EPS, 0.1, 0, True),   # every channel: mean / deviation = 1e3
    "b193 c132":      (2, 6176, 132, "gap", "edge", BN_EPS, 0.1, 1, True),       # the four-chain loop in the second tile's partials
}
CASE_NAMES = tuple(MATRIX)
# per-channel statistics of an "edge" map, channel c takes kind (c + case index) % 9:
KINDS = ("unit", "mean / deviation 1e3", "scale 1e4", "scale 1e-4", "constant", "gamma 0", "gamma negative", "beta +6", "beta -6")


@functools.lru_cache(maxsize=None)
def case(name):
    """One case of the matrix, seeded by its position, built once.  x, dy: [n_img rows, ch] float32."""
    n_img, rows, ch, lay, stats, eps, mom, flags, running = MATRIX[name]
    k = CASE_NAMES.index(name)
    gen = torch.Generator().manual_seed(4100 + k)
    N = n_img * rows
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = rn(N, ch) * 1.7 + 0.4
    gamma, beta = torch.rand(ch, generator=gen) + 0.5, rn(ch) * 0.2
    dy = rn(N, ch) * (0.1 + 2.9 * torch.rand(ch, generator=gen))
    kinds = ["unit"] * ch
    if stats == "shifted":
        kinds = ["mean / deviation 1e3"] * ch
    elif stats == "edge":
        kinds = [KINDS[(c_ + k) % len(KINDS)] for c_ in range(ch)]
        dy = torch.where(torch.rand(N, ch, generator=gen) < 0.1, torch.zeros(()), dy)      # exact zeros
    z = rn(N, ch)
    for c_, kind in enumerate(kinds):
        if kind == "mean / deviation 1e3":
            x[:, c_] = 1000.0 + z[:, c_]
        elif kind == "scale 1e4":
            x[:, c_] = 3e3 + 1e4 * z[:, c_]
        elif kind == "scale 1e-4":
            x[:, c_] = 1e-4 * z[:, c_]
        elif kind == "constant":
            x[:, c_] = 2.5
        elif kind == "gamma 0":
            gamma[c_] = 0.0
        elif kind == "gamma negative":
            gamma[c_] = -gamma[c_]
        elif kind in ("beta +6", "beta -6"):
            gamma[c_], beta[c_] = 0.5, (6.0 if kind == "beta +6" else -6.0)
    c = dict(name=name, n_img=n_img, rows=rows, ch=ch, layout=lay, kinds=tuple(kinds), eps=eps, momentum=mom, flags=flags,
             x=x.contiguous(), dy=dy.contiguous(), gamma=gamma, beta=beta,
             rm=rn(ch) * 0.1 if running else None, rv=torch.rand(ch, generator=gen) + 0.5 if running else None,
             old_dgamma=rn(ch) * 1e3, old_dbeta=rn(ch) * 1e3)     # another magnitude than the sums (flags bit 0)
    return c


def cases():
    return {name: case(name) for name in CASE_NAMES}


@functools.lru_cache(maxsize=None)
def refs(name):
    """(reference, bound, twin) of a case, computed once and shared by the tests that need them; callers leave them unchanged"""
    c = case(name)
    ref = reference(c)
    return ref, bound(c, ref), twin32(c)
