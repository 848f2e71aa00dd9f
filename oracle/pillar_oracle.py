"""Exact emulation, float64 references and a worst-case error model of the pillar stage (include/himo_amd.h: himo_pillarize*,
himo_pillar_features_multi, himo_pfn_bn_stats*, himo_pfn_backward, himo_pfn_backward_bn*, himo_head_scatter; csrc/pillar.hip).
CPU only.  A restatement from himo_amd/seflow/spec.py steps 0-2 and the operation order the kernels document; it shares no code
with oracle/seflow_oracle.py::pillar_image, which stays the network's oracle.

EXACT parts (float32 operation by operation, no fused multiply-add: pillar.hip is built with -ffp-contract=off) -- compared bit
for bit:
  transform     ((x R0 + y R1) + z R2) + t                                       (``transform``)
  cell rule     floorf((t - min) / v), 0 <= f < W | H | 1, cell = iy W + ix       (``cells_of``)
  offsets       t - ((float)ix v + c0), zeros for dropped points                  (``cells_of``)
  point order   every cell's points in ascending point index                      (``cell_lists``)
  scatter       himo_head_scatter: the ordered float32 sum of a cell's rows      (``scatter_ref``)
  split image   h = fp16(x), l = fp16(x - h), [h0..h15 | l0..l15] per 16 channels (``split_words``; conv_oracle.split_terms)

FLOAT64 parts, each with a per-output WORST-case bound; u = 2^-24, the "f32" arithmetic class of conv_oracle: every product and
every addition rounds once, the fma chain once per step.  All bounds carry the factor SLACK = 1 + 2^-10 for second-order terms.
  image   per cell of cnt points (ascending order): m = (sum x) / cnt [e_m = (cnt - 1) u sum|x| / cnt + u |m|; 0 for cnt = 1, where
          the kernel takes the point itself]; f = [x, x - m, offset] [e_f = e_m + u (|x - m| + e_m) on the middle three; the offsets
          are the exact float32 values]; v = the 9-step fma chain [e_v = 9 u sum|f_q w_q| + sum |w_q| e_f,q]; y = v scale + shift
          [e_y = |scale| e_v + u |v scale| + u |y|]; ReLU is 1-Lipschitz, so e_y passes through it; feature = (sum relu y) / cnt
          [(sum e_y + (cnt - 1) u sum relu y) / cnt + u |feature|].
  stats   himo_pfn_bn_stats*: float64 sums of the float32 v over a GROUP's in-range points (torch.nn.BatchNorm1d: biased variance
          normalises, the unbiased one updates the running variance, a count of 1 leaves the variance uncorrected).  The kernel's
          sums are float64 (block partials of pfn_walk_kernel, then the four-chain, 16-group fixed-order combine of
          pfn_bn_finalize_kernel): their own error, at most (points + 22) 2^-53 relative, is covered by D = 2^-40.
          e_mean = avg e_v; e_var = (2 / N) sum |v - mean| e_v + avg e_v^2 + D E[v^2];
          invstd = (float)(1 / sqrt(var + eps)) [e = e_var / (2 (var - e_var + eps)^1.5) + u invstd]; scale = gamma invstd, shift =
          beta - (float)mean scale, the running statistics: first order, one u per float32 rounding.
  dW, dgamma, dbeta   himo_pfn_backward (frozen statistics: dW = sum f g scale, g = d_image / cnt where y > 0) and
          himo_pfn_backward_bn* (dbeta = sum g, dgamma = sum g xhat, dy = scale (g - mean g - xhat mean(g xhat)), dW = sum f dy, the
          two means over the GROUP): first-order propagation of e_f, e_v and one u per float32 rounding.  Partial-sum merges, in the
          manner of grad_oracle: a product f_k dy passes through the additions of its own half-wave (at most the N in-range points
          of its sweep), 8 (the half-waves of a block), then ceil(1024 / 128) = 8 + 2 + 32 additions of pfn_backward_reduce_kernel
          (four chains per group, 32 groups), 3 roundings of its own factors and one per sweep summed into d_dweight: the
          accumulation term is (N + PFN_MERGE_C + n_sweeps) u sum|f_k dy|, PFN_MERGE_C = 56.  The accumulate flag adds u (|old| + |new|).
  ReLU mask   a decision, not a rounding: a (point, channel) pair is UNDECIDED when |y| <= e_y; its whole term is added to the
          tolerance of every output it feeds, and those outputs are left out of both rms sums of the aggregate level.  ``UNDECIDED_CAP``: at most
          0.1 % of a case's in-range pairs -- a condition on the case (tests/test_pillar_oracle.py), not a measurement.

Aggregate level: conv_oracle.check / ok with R["f32"] = 2 against the float32 twin (the same steps in float32 numpy: sequential
means, a BLAS float32 product for the chain, float32 sums), from MIN_AGGREGATE = 32 outputs on (grad_oracle), for the image, dW,
dgamma and dbeta.  The emulated correct kernel of tests/test_pillar_oracle.py (fma chain, reversed summation order, per-32 partial
sums of dW) stays under 2 for the image, the frozen dW, dgamma and dbeta on every case of the CPU matrix (largest: 1.29, 0.73,
1.84, 0.27), so R["f32"] holds for them as it stands.  It does NOT for the dW of himo_pfn_backward_bn*: the two group means
(mean g, mean g xhat) are rounded to float32 ONCE and enter the dy of every point, and sum dy = 0, so dW = sum f dy is a sum of
cancelling terms whose error is led by those two shared roundings (and the shared float32 mean / invstd products) rather than by N
independent ones -- the rms ratio is then the ratio of a handful of roundings of the kernel to a handful of the twin, no
statistic.  The emulated correct kernel reaches 3.6 there (scenes 1x1 .. 41x25, four gradient draws each: 64x1, draw 2; asserted by
tests/test_pillar_oracle.py::test_bn_dw_limit_rests_on_the_correct_twin);
times 2 for the freedom of summation order: R_BN_DW = 7.2.  The wrong kernels of the CPU suite miss it by orders of magnitude.

Observed on an MI355X: see the table at the end of this comment block (information only -- no constant here was chosen
from it).

    (no MI355X run of tests/test_pillar_conformance_gpu.py has been recorded for this revision yet)
"""
from __future__ import annotations

import math

import numpy as np

import conv_oracle as co
from conv_oracle import U, check, ok, rms  # noqa: F401  (re-exported for the tests)

F32, F64 = np.float32, np.float64
SLACK = 1.0 + 2.0 ** -10
D = 2.0 ** -40
PFN_MERGE_C = 56
UNDECIDED_CAP = 1e-3
MIN_AGGREGATE = 32
R = {"f32": co.R["f32"]}
R_BN_DW = 7.2                           # dW of himo_pfn_backward_bn*: derivation in the comment block above


class Grid:
    """W x H x 1 pillars: cell (ix, iy) = [min + i v, min + (i + 1) v); what the host passes is float32."""

    def __init__(self, W, H, vmin, voxel):
        self.W, self.H, self.cells = int(W), int(H), int(W) * int(H)
        self.vmin = np.asarray(vmin, F32)
        self.voxel = np.asarray(voxel, F32)
        self.centre = (self.voxel.astype(F64) / 2 + self.vmin.astype(F64)).astype(F32)      # voxel / 2 + min, rounded to float32
        self.vmax = (self.vmin.astype(F64) + np.array([W, H, 1], F64) * self.voxel.astype(F64)).astype(F32)

    def __repr__(self):
        return f"{self.W}x{self.H} v={tuple(float(v) for v in self.voxel)} min={tuple(float(v) for v in self.vmin)}"


# ---- exact parts ------------------------------------------------------------------------------------------------------------------
def transform(pts, T):
    """p' = ((x R0 + y R1) + z R2) + t, every product and sum rounded to float32.  pts [n, >= 3], T row-major 4x4 float32."""
    p = np.asarray(pts, F32)
    T = np.asarray(T, F32).reshape(4, 4)
    out = np.empty((p.shape[0], 3), F32)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((p[:, 0] * T[r, 0] + p[:, 1] * T[r, 1]) + p[:, 2] * T[r, 2]) + T[r, 3]
    return out


def cell_centres(grid, ix, iy):
    """(float)ix vx + cx0, (float)iy vy + cy0, 0 vz + cz0 -- two float32 roundings each"""
    cx = ix.astype(F32) * grid.voxel[0] + grid.centre[0]
    cy = iy.astype(F32) * grid.voxel[1] + grid.centre[1]
    cz = np.full(ix.shape, F32(0) * grid.voxel[2] + grid.centre[2], F32)
    return np.stack([cx, cy, cz], 1).astype(F32)


def cells_of(xyz_t, grid):
    """-> pid int32 [n] (iy W + ix, -1 = dropped), offsets float32 [n, 3] (zeros for dropped points)"""
    t = np.asarray(xyz_t, F32)
    with np.errstate(all="ignore"):
        f = np.floor((t - grid.vmin[None, :]) / grid.voxel[None, :]).astype(F32)
        lim = np.array([grid.W, grid.H, 1], F32)
        okk = np.all((f >= 0) & (f < lim[None, :]), axis=1)
    ix = np.where(okk, f[:, 0], 0).astype(np.int64)
    iy = np.where(okk, f[:, 1], 0).astype(np.int64)
    pid = np.where(okk, iy * grid.W + ix, -1).astype(np.int32)
    with np.errstate(all="ignore"):
        off = np.where(okk[:, None], t - cell_centres(grid, ix, iy), F32(0)).astype(F32)
    return pid, off


def cell_lists(pid, cells):
    """-> start int64 [cells + 1], order int64 [P]: the in-range points grouped by cell, ascending point index inside a cell"""
    pid = np.asarray(pid)
    idx = np.nonzero((pid >= 0) & (pid < cells))[0]
    order = idx[np.argsort(pid[idx], kind="stable")]
    start = np.zeros(cells + 1, np.int64)
    np.cumsum(np.bincount(pid[idx], minlength=cells), out=start[1:])
    return start, order


def ordered_sum32(rows, start, order):
    """per cell, the float32 sum of rows[order[start[c] : start[c + 1]]] taken one after another from 0 -> [cells, cols]"""
    cnt = np.diff(start)
    out = np.zeros((cnt.size, rows.shape[1]), F32)
    for r in range(int(cnt.max()) if cnt.size else 0):
        sel = np.nonzero(cnt > r)[0]
        out[sel] = out[sel] + rows[order[start[sel] + r]].astype(F32)
    return out


def scatter_ref(start, order, dhx, group0, group1, n_groups):
    """himo_head_scatter -> d_b0 [cells, n_groups, 32], d_dec [cells, 64]; bit-exact"""
    s = ordered_sum32(np.asarray(dhx, F32)[:, :128], start, order)
    b0 = np.zeros((s.shape[0], n_groups, 32), F32)
    b0[:, group0] = s[:, :32]
    b0[:, group1] = s[:, 32:64]
    return b0, s[:, 64:128].copy()


def split_words(img):
    """[cells, 32] float32 -> [cells, 32] int32 words of the split activation format"""
    h, l = co.split_terms("f16x2", np.asarray(img, F32))
    hb = h.astype(np.float16).view(np.uint16).reshape(-1, 2, 1, 16)
    lb = l.astype(np.float16).view(np.uint16).reshape(-1, 2, 1, 16)
    return np.ascontiguousarray(np.concatenate([hb, lb], 2)).view(np.int32).reshape(-1, 32)


# ---- float64 references ------------------------------------------------------------------------------------------------------------
class Terms:
    """per in-range point, in cell-major ascending order: features, the chain's value and their error bounds"""

    def __init__(self, xyz_t, pid, grid, w, dtype=F64):
        self.start, self.order = cell_lists(pid, grid.cells)
        o = self.order
        self.cnt = np.diff(self.start)
        self.ne = np.nonzero(self.cnt)[0]                      # non-empty cells
        self.first = self.start[self.ne]
        self.cell = np.asarray(pid)[o].astype(np.int64)
        self.P = o.size
        cp = self.cnt[self.cell].astype(F64)[:, None] if self.P else np.zeros((0, 1))
        x32 = np.asarray(xyz_t, F32)[o]
        iy, ix = self.cell // grid.W, self.cell % grid.W
        off = (x32 - cell_centres(grid, ix, iy)).astype(F32)    # the exact float32 offsets
        self.cp = cp
        w = np.asarray(w, F32)
        if dtype == F32:
            # the twin: sequential float32 mean, float32 features, a float32 matrix product
            m = (ordered_sum32(x32, self.start, np.arange(self.P))[self.cell] / cp.astype(F32)).astype(F32) if self.P else x32
            m = np.where(cp == 1, x32, m)
            self.f = np.concatenate([x32, (x32 - m).astype(F32), off], 1).astype(F32)
            self.v = (self.f @ w).astype(F32)
            return
        x = x32.astype(F64)
        if self.P:
            sx = np.add.reduceat(x, self.first, axis=0)
            sa = np.add.reduceat(np.abs(x), self.first, axis=0)
            c = self.cnt[self.ne].astype(F64)[:, None]
            m_c = sx / c
            em_c = np.where(c > 1, (c - 1) * U * sa / c + U * np.abs(m_c), 0.0)
            rank = np.searchsorted(self.ne, self.cell)
            m, em = m_c[rank], em_c[rank]
        else:
            m = em = np.zeros((0, 3))
        dm = x - m
        self.f = np.concatenate([x, dm, off.astype(F64)], 1)
        z = np.zeros_like(x)
        self.ef = np.concatenate([z, np.where(cp > 1, em + U * (np.abs(dm) + em), 0.0), z], 1)
        w64 = w.astype(F64)
        self.v = self.f @ w64
        self.mag = np.abs(self.f) @ np.abs(w64)
        self.ev = SLACK * (9 * U * self.mag + self.ef @ np.abs(w64))

    def y(self, scale, shift):
        """v scale + shift and its bound (float64 terms only)"""
        s, b = np.asarray(scale, F64)[None, :], np.asarray(shift, F64)[None, :]
        y = self.v * s + b
        return y, SLACK * (np.abs(s) * self.ev + U * np.abs(self.v * s) + U * np.abs(y))

    def per_cell(self, a, cells):
        out = np.zeros((cells, a.shape[1]), a.dtype)
        if self.P:
            out[self.ne] = np.add.reduceat(a, self.first, axis=0)
        return out


def image_ref(xyz_t, pid, grid, w, scale, shift):
    """-> ref [cells, 32] float64, bound, ref32 (the float32 twin), mask of the non-empty cells"""
    t = Terms(xyz_t, pid, grid, w)
    y, ey = t.y(scale, shift)
    r = np.maximum(y, 0.0)
    c = np.maximum(t.cnt, 1).astype(F64)[:, None]
    ref = t.per_cell(r, grid.cells) / c
    bnd = SLACK * ((t.per_cell(ey, grid.cells) + (c - 1) * U * t.per_cell(r, grid.cells)) / c + U * np.abs(ref))
    t32 = Terms(xyz_t, pid, grid, w, F32)
    y32 = (t32.v * np.asarray(scale, F32)[None, :] + np.asarray(shift, F32)[None, :]).astype(F32)
    ref32 = (t32.per_cell(np.maximum(y32, F32(0)), grid.cells) / c.astype(F32)).astype(F32)
    return ref, bnd, ref32, t.cnt > 0


def bn_stats_ref(members, grid, w, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """One GROUP (members: [(xyz_t, pid), ...]) -> dict name -> (ref float64 [32], bound [32]); names scale, shift, mean,
    invstd and, when tracked, running_mean / running_var (the values AFTER the update)."""
    ts = [Terms(x, p, grid, w) for x, p in members]
    v = np.concatenate([t.v for t in ts]) if ts else np.zeros((0, 32))
    ev = np.concatenate([t.ev for t in ts]) if ts else np.zeros((0, 32))
    n = v.shape[0]
    g, b = np.asarray(gamma, F64), np.asarray(beta, F64)
    eps = float(F32(eps))
    out = {}
    if n == 0:
        rv = np.asarray(running_var, F64) if running_var is not None else np.ones(32)
        rm = np.asarray(running_mean, F64) if running_mean is not None else np.zeros(32)
        sc = g / np.sqrt(rv + eps)
        sh = b - rm * sc
        e_sc = 4 * U * np.abs(sc)
        out["scale"] = (sc, SLACK * e_sc)
        out["shift"] = (sh, SLACK * (np.abs(rm) * e_sc + U * np.abs(rm * sc) + U * np.abs(sh)))
        out["mean"] = out["invstd"] = (np.zeros(32), np.zeros(32))
        if running_mean is not None:
            out["running_mean"], out["running_var"] = (rm, np.zeros(32)), (rv, np.zeros(32))
        return out
    mean = v.mean(0)
    var = ((v - mean[None]) ** 2).mean(0) if n > 1 else np.zeros(32)       # E[v^2] - mean^2 in its better-conditioned form
    e_mean = ev.mean(0) + D * np.abs(v).mean(0)
    e_var = 2 * (np.abs(v - mean[None]) * ev).mean(0) + (ev * ev).mean(0) + D * (v * v).mean(0)
    invstd = 1.0 / np.sqrt(var + eps)
    e_inv = 0.5 * e_var / (np.maximum(var - e_var, 0.0) + eps) ** 1.5 + U * invstd
    sc = g * invstd
    e_sc = np.abs(g) * e_inv + U * np.abs(sc)
    sh = b - mean * sc
    e_sh = np.abs(sc) * (e_mean + U * np.abs(mean)) + np.abs(mean) * e_sc + U * np.abs(mean * sc) + U * np.abs(sh)
    out["scale"], out["shift"] = (sc, SLACK * e_sc), (sh, SLACK * e_sh)
    out["mean"], out["invstd"] = (mean, SLACK * (e_mean + U * np.abs(mean))), (invstd, SLACK * e_inv)
    if running_mean is not None:
        mo = float(F32(momentum))
        unb = var * n / (n - 1) if n > 1 else var
        rm = (1 - mo) * np.asarray(running_mean, F64) + mo * mean
        rv = (1 - mo) * np.asarray(running_var, F64) + mo * unb
        out["running_mean"] = (rm, SLACK * (mo * e_mean + U * np.abs(rm)))
        out["running_var"] = (rv, SLACK * (mo * e_var * (n / (n - 1) if n > 1 else 1.0) + U * np.abs(rv)))
    return out


def backward_ref(sweeps, grid, w, scale, shift, mean=None, invstd=None, n_groups=None, old=None):
    """sweeps: [(xyz_t, pid, d_image [cells, 32]), ...].  mean is None: himo_pfn_backward (frozen statistics, ONE sweep, scale /
    shift [32]); otherwise himo_pfn_backward_bn_groups (sweep i in group i % n_groups; scale / shift / mean / invstd [n_groups, 32]).
    old: None or (dW, dgamma, dbeta) float32 that the call accumulates into.
    -> dict name -> (ref, bound, ref32, undecided tolerance) for dW [9, 32] (and dgamma, dbeta [32]), plus "pairs" and "undecided"."""
    frozen = mean is None
    n_groups = 1 if frozen else (n_groups or len(sweeps))
    sc = np.asarray(scale, F64).reshape(n_groups, 32)
    sh = np.asarray(shift, F64).reshape(n_groups, 32)
    pts = []
    pairs = und_n = 0
    for i, (x, p, dimg) in enumerate(sweeps):
        g_ = i % n_groups
        t, t32 = Terms(x, p, grid, w), Terms(x, p, grid, w, F32)
        y, ey = t.y(sc[g_], sh[g_])
        on, und = y > 0, np.abs(y) <= ey
        gi = np.asarray(dimg, F64)[t.cell] / t.cp
        gi32 = (np.asarray(dimg, F32)[t.cell] / t.cp.astype(F32)).astype(F32)
        y32 = (t32.v * sc[g_].astype(F32)[None] + sh[g_].astype(F32)[None]).astype(F32)
        pairs += y.size
        und_n += int(und.sum())
        pts.append(dict(t=t, t32=t32, on=on, und=und, gi=gi, g=np.where(on, gi, 0.0), ug=np.where(und, np.abs(gi), 0.0),
                        g32=np.where(y32 > 0, gi32, F32(0)).astype(F32), grp=g_))
    res = {"pairs": pairs, "undecided": und_n}
    dW, eW, uW, dW32 = np.zeros((9, 32)), np.zeros((9, 32)), np.zeros((9, 32)), np.zeros((9, 32), F32)
    n_sw = len(sweeps)

    def fold(q, dy, e_dy, u_dy, dy32):
        t = q["t"]
        af = np.abs(t.f)
        nonlocal dW, eW, uW, dW32
        dW += t.f.T @ dy
        mg = af.T @ np.abs(dy)
        eW += t.ef.T @ (np.abs(dy) + e_dy) + af.T @ e_dy + U * mg + (t.P + PFN_MERGE_C + n_sw) * U * mg
        uW += (af + t.ef).T @ u_dy
        dW32 = (dW32 + (q["t32"].f.T @ dy32).astype(F32)).astype(F32)

    if frozen:
        q = pts[0]
        s = sc[0][None]
        fold(q, q["g"] * s, 2 * U * np.abs(q["g"] * s), q["ug"] * np.abs(s), (q["g32"] * s.astype(F32)).astype(F32))
    else:
        mu = np.asarray(mean, F64).reshape(n_groups, 32)
        iv = np.asarray(invstd, F64).reshape(n_groups, 32)
        dg, eg_, ug_, dg32 = (np.zeros(32) for _ in range(4))
        db, eb_, ub_, db32 = (np.zeros(32) for _ in range(4))
        for g_ in range(n_groups):
            mem = [q for q in pts if q["grp"] == g_]
            n = sum(q["t"].P for q in mem)
            a0 = a1 = e0 = e1 = u0 = u1 = np.zeros(32)
            a0_32 = a1_32 = np.zeros(32, F32)
            for q in mem:
                t = q["t"]
                q["xh"] = (t.v - mu[g_][None]) * iv[g_][None]
                q["exh"] = np.abs(iv[g_])[None] * (t.ev + U * np.abs(t.v - mu[g_][None])) + U * np.abs(q["xh"])
                q["xh32"] = ((q["t32"].v - mu[g_].astype(F32)[None]) * iv[g_].astype(F32)[None]).astype(F32)
                g, xh, exh, ug = q["g"], q["xh"], q["exh"], q["ug"]
                a0 = a0 + g.sum(0)
                a1 = a1 + (g * xh).sum(0)
                e0 = e0 + (U * np.abs(g)).sum(0) + D * np.abs(g).sum(0)
                e1 = e1 + (U * np.abs(g * xh) + np.abs(g) * exh).sum(0) + D * np.abs(g * xh).sum(0)
                u0 = u0 + ug.sum(0)
                u1 = u1 + (ug * (np.abs(xh) + exh)).sum(0)
                a0_32 = a0_32 + q["g32"].sum(0, dtype=F32)
                a1_32 = a1_32 + (q["g32"] * q["xh32"]).sum(0, dtype=F32)
            db, dg = db + a0, dg + a1
            eb_, eg_ = eb_ + e0 + 2 * U * np.abs(a0), eg_ + e1 + 2 * U * np.abs(a1)
            ub_, ug_ = ub_ + u0, ug_ + u1
            db32, dg32 = db32 + a0_32, dg32 + a1_32
            if n == 0:
                continue
            k2, k3 = a0 / n, a1 / n
            ek2, ek3 = (e0 + u0) / n + U * np.abs(k2), (e1 + u1) / n + U * np.abs(k3)
            k2_32, k3_32 = (a0_32 / F32(n)).astype(F32), (a1_32 / F32(n)).astype(F32)
            s = sc[g_][None]
            for q in mem:
                g, xh, exh = q["g"], q["xh"], q["exh"]
                inner = g - k2[None] - xh * k3[None]
                e_in = (U * np.abs(g) + ek2[None] + exh * (np.abs(k3) + ek3)[None] + np.abs(xh) * ek3[None]
                        + U * (np.abs(xh * k3[None]) + np.abs(g - k2[None]) + np.abs(inner)))
                dy = s * inner
                dy32 = (s.astype(F32) * ((q["g32"] - k2_32[None]) - q["xh32"] * k3_32[None])).astype(F32)
                fold(q, dy, np.abs(s) * e_in + U * np.abs(dy), q["ug"] * np.abs(s), dy32)
        for name, a, e, u_, a32, o in (("dgamma", dg, eg_, ug_, dg32, 1), ("dbeta", db, eb_, ub_, db32, 2)):
            if old is not None:
                oo = np.asarray(old[o], F64)
                a, a32, e = a + oo, (a32 + np.asarray(old[o], F32)).astype(F32), e + U * (np.abs(oo) + np.abs(a))
            res[name] = (a, SLACK * (e + u_) + 1e-300, a32.astype(F32), u_)
    if old is not None:
        oo = np.asarray(old[0], F64).reshape(9, 32)
        eW = eW + U * (np.abs(oo) + np.abs(dW))
        dW, dW32 = dW + oo, (dW32 + np.asarray(old[0], F32).reshape(9, 32)).astype(F32)
    res["dW"] = (dW, SLACK * (eW + uW) + 1e-300, dW32, uW)
    return res


def verify(name, got, ref, bnd, ref32=None, und=None, case="", limit=None):
    """Both levels (conv_oracle.check).  The worst-case level covers every output; the aggregate level leaves the outputs fed by an
    undecided pair (und > 0) out of BOTH rms sums and is asserted from MIN_AGGREGATE remaining outputs on."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64)))
    got = np.asarray(got, F64).reshape(np.shape(ref))
    assert not np.isnan(got).any(), f"{case} {name}: NaN in the result"
    w, _, report = check(t(got), t(ref), t(bnd), None, "f32", f"{case} {name}")
    assert w <= 1.0, report
    if ref32 is None:
        return w, 0.0
    keep = np.ones(np.shape(ref), bool) if und is None else np.asarray(und) == 0
    if int(keep.sum()) < MIN_AGGREGATE:
        return w, 0.0
    _, rr, report = check(t(got[keep]), t(np.asarray(ref)[keep]), t(np.asarray(bnd)[keep]), t(np.asarray(ref32)[keep]), "f32",
                          f"{case} {name}", limit=limit)
    assert rr <= (R["f32"] if limit is None else limit), report
    return w, rr


def exact(name, got, want, case=""):
    """bit for bit; float arrays compare their words, NaN against NaN by isnan"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{case} {name}: shape {got.shape} != {want.shape}"
    if want.dtype == F32:
        both = np.isnan(got) & np.isnan(want)
        bad = (got.view(np.int32) != want.view(np.int32)) & ~both
    else:
        bad = got != want
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{case} {name}: {int(bad.sum())} of {bad.size} differ, first at {i}: got {got[i]!r} want {want[i]!r}")


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def rigid(kind):
    """'general': a rotation about z with a small tilt and a translation; 'quarter': an exact quarter turn with a dyadic translation,
    under which the float32 transform of dyadic coordinates is exact (the boundary rows)"""
    T = np.eye(4)
    if kind == "quarter":
        T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
        T[:3, 3] = [0.5, -0.25, 0.125]
    else:
        a, b = 0.3, 0.01
        rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        T[:3, :3] = rz @ rx
        T[:3, 3] = [0.37, -0.21, 0.05]
    return T.astype(F32)


def source_of(target, T):
    """float32 source rows whose transform is (near) ``target``"""
    T = np.asarray(T, F64)
    return ((np.asarray(target, F64) - T[:3, 3][None]) @ T[:3, :3]).astype(F32)


def scene(grid, placed, filler, seed, T, n_out=0):
    """Points (source frame, float32 [n, 3]) that put exactly ``count`` points into ``cell`` for every (cell, count) of ``placed``
    and, with probability ``filler``, one to three into each other cell; ``n_out`` more land outside the range.  Coordinates keep
    a fifth of a cell away from the faces; the rows are shuffled, so a cell's members are spread over the whole sweep in
    non-monotonic order.  The builder asserts its own populations through the exact emulation."""
    rng = np.random.default_rng(seed)
    want = np.zeros(grid.cells, np.int64)
    fill = rng.random(grid.cells) < filler
    want[fill] = rng.integers(1, 4, int(fill.sum()))
    for cell, count in placed:
        want[cell % grid.cells] = count
    cell = np.repeat(np.arange(grid.cells), want)
    frac = rng.uniform(0.2, 0.8, (cell.size, 3))
    ij = np.stack([cell % grid.W, cell // grid.W, np.zeros_like(cell)], 1)
    tgt = grid.vmin.astype(F64)[None] + (ij + frac) * grid.voxel.astype(F64)[None]
    if n_out:
        o = grid.vmax.astype(F64)[None] + rng.uniform(0.5, 3.0, (n_out, 3)) * grid.voxel.astype(F64)[None]
        tgt, cell = np.concatenate([tgt, o]), np.concatenate([cell, np.full(n_out, -1)])
    perm = rng.permutation(cell.size)
    pts, cell = source_of(tgt[perm], T), cell[perm]
    pid, _ = cells_of(transform(pts, T), grid)
    assert np.array_equal(pid, cell), "scene: a point left its cell"
    return pts


def boundary_rows(grid, T):
    """-> source rows [k, 3], kept [k] (the intent), hit [k] (False where the float32 transform misses the face by a rounding and
    only the emulation decides): a minimum, a maximum and nextafter below it on every axis, the corner, NaN and +-inf rows"""
    lo, hi, v = grid.vmin.astype(F64), grid.vmax.astype(F64), grid.voxel.astype(F64)
    mid = lo + np.array([grid.W // 2 + 0.5, grid.H // 2 + 0.5, 0.5]) * v
    below = np.nextafter(grid.vmax, np.float32(-np.inf)).astype(F64)
    rows, kept = [], []
    for ax in range(3):
        for val, k in ((lo[ax], True), (hi[ax], False), (below[ax], True)):
            p = mid.copy()
            p[ax] = val
            rows.append(p)
            kept.append(k)
    rows.append(lo.copy()); kept.append(True)
    src = source_of(np.array(rows), T)
    hit = np.all(transform(src, T) == np.array(rows).astype(F32), axis=1)      # the float32 transform lands ON the face
    for ax in range(3):     # nextafter below a maximum stays inside only where t - min is exact in float32; elsewhere the emulation decides
        hit[3 * ax + 2] &= float(F32(below[ax] - lo[ax])) == below[ax] - lo[ax]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.inf, -np.inf, np.nan]], F32)
    return np.concatenate([src, bad]), np.array(kept + [False] * 4), np.concatenate([hit, np.ones(4, bool)])


# ---- the cases both suites run -----------------------------------------------------------------------------------------------------
def _g(W, H, kind):
    if kind == "dyadic":           # non-square voxels, off-centre range, every face a dyadic number
        return Grid(W, H, (-1.75, 3.0, -1.0), (0.25, 0.5, 4.0))
    if kind == "fifth":            # the in-tree voxel (0.2, 0.2, 6): faces that are no float32 numbers
        return Grid(W, H, (-0.2 * W / 2, -0.2 * H / 2, -3.0), (0.2, 0.2, 6.0))
    return Grid(W, H, (-0.5 * W / 2, -0.5 * H / 2 + 8.0, -3.0), (0.5, 0.5, 6.0))


POPS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 97)


def _spread(cells, pops=POPS):
    """the populations at cell 0, the last cell and either side of every 64 / 256 / 1024 boundary the grid has"""
    marks = [0, cells - 1]
    for b in (64, 256, 1024):
        if cells > b:
            marks += [b - 1, b]
    marks = sorted(set(m for m in marks if 0 <= m < cells))
    return [(m, pops[(3 + 2 * i) % len(pops)]) for i, m in enumerate(marks)]


# name -> (grid, placed, filler, transform kind, points outside, boundary rows?)
SCENES = {
    "1x1": (_g(1, 1, "dyadic"), [(0, 33)], 0.0, "quarter", 3, True),
    "7x5": (_g(7, 5, "fifth"), [(0, 33), (34, 97), (17, 32), (5, 1), (6, 2), (20, 31), (21, 0)], 0.5, "general", 5, False),
    "64x1": (_g(64, 1, "dyadic"), [(0, 65), (63, 64), (31, 63)], 0.4, "quarter", 2, True),
    "1x64": (_g(1, 64, "square"), [(0, 2), (63, 33), (32, 1000)], 0.4, "general", 2, False),
    "65x1": (_g(65, 1, "dyadic"), [(63, 33), (64, 65), (0, 1)], 0.3, "quarter", 0, True),
    "32x32": (_g(32, 32, "square"), _spread(1024) + [(500, 1000)], 0.2, "general", 7, False),
    "41x25": (_g(41, 25, "dyadic"), _spread(1025), 0.2, "general", 4, False),
    "128x96": (_g(128, 96, "fifth"), _spread(128 * 96) + [(1023 + 1024, 33), (2048, 97), (255 + 256, 64), (512, 65)], 0.1, "general", 9, False),
}


def build_scene(name, seed=0):
    """-> grid, T, pts [n, 3] float32 (boundary rows, where the scene has them, at the front, the middle and the end)"""
    grid, placed, filler, kind, n_out, faces = SCENES[name]
    T = rigid(kind)
    pts = scene(grid, placed, filler, 100 + seed, T, n_out)
    if faces:
        b = boundary_rows(grid, T)[0]
        h = pts.shape[0] // 2
        pts = np.concatenate([b[:4], pts[:h], b[4:9], pts[h:], b[9:]])
    return grid, T, pts


def params(seed):
    """pfn weight [9, 32], BatchNorm gamma / beta and constants scale / shift [32] with shifts well away from zero"""
    rng = np.random.default_rng(7000 + seed)
    w = rng.uniform(-0.5, 0.5, (9, 32)).astype(F32)
    gamma = rng.uniform(0.6, 1.4, 32).astype(F32) * np.where(rng.random(32) < 0.25, -1, 1).astype(F32)
    beta = rng.uniform(-0.5, 0.5, 32).astype(F32)
    scale = rng.uniform(0.3, 1.2, 32).astype(F32) * np.where(rng.random(32) < 0.25, -1, 1).astype(F32)
    shift = rng.uniform(-1.0, 1.0, 32).astype(F32)
    return dict(w=w, gamma=gamma, beta=beta, scale=scale, shift=shift)


def check_forward(got, pts, T, grid, p, case=""):
    """got: xyz_t, pid, offsets, start, order (the workspace's lists), image [cells, 32] -> (worst err / bound, rms ratio)"""
    xyz = transform(pts, T)
    exact("xyz_t", got["xyz_t"], xyz, case)
    pid, off = cells_of(xyz, grid)
    exact("pid", got["pid"], pid, case)
    exact("offsets", got["offsets"], off, case)
    start, order = cell_lists(pid, grid.cells)
    exact("cell offsets", np.asarray(got["start"], np.int64), start, case)
    exact("ascending point order", np.asarray(got["order"], np.int64), order, case)
    ref, bnd, ref32, ne = image_ref(xyz, pid, grid, p["w"], p["scale"], p["shift"])
    img = np.asarray(got["image"], F32)
    assert not img[~ne].view(np.int32).any(), f"{case}: an empty cell is not +0"
    if not ne.any():
        return 0.0, 0.0
    return verify("image", img[ne], ref[ne], bnd[ne], ref32[ne], None, case)
