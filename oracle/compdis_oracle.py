"""An exact restatement of the motion-compensation kernels (csrc/compdis.hip, csrc/compdis_gt.hip, csrc/compdis_math.h).  CPU only.

The kernels claim a FIXED operation order with every fused multiply-add explicit (the files are compiled with -ffp-contract=off),
so this oracle restates that order and the conformance suite (tests/test_compdis_conformance_gpu.py) demands equal bits: there is
no tolerance anywhere but in ``ego_bound``, which is derived, not measured.

  chain        point_math of compdis_math.h:66-100, operation by operation, in the float64 and the float32 chain: the k-order of
               pose_flow_f64 (and its ``single_row`` variant), (dot + t) - p, divide THEN multiply, dt0 in float32, the casts.
  frame_max    the per-frame maximum as frame_prep_kernel forms it (order-preserving integer keys, NaN elements dropped).
  python_max   the reference's ``max(lidar_dt)``: kept apart so that the divergence is visible.
  mask         eval_mask_point with its float32 norm.
  gt_body      the ten-column body of one sweep of compdis_gt_kernel, pad bytes zero.
  lu_ego       compute_ego of compdis.hip:35-88 in the kernel's order (the wrong variants of the pivoting are variants of this).
  exact_ego    inv(pose1) @ pose0 in rational arithmetic;  ego_bound: the forward-error bound the device transforms are held to.
  CASES        the matrix; every case names the paths it promises to reach and ``promise`` proves each with integer arithmetic.

A fused multiply-add is ONE rounding of the exact a b + c.  Python before 3.13 has no math.fma, so the float64 one is formed in
integer arithmetic (fma64; fma_fraction is the same thing said with ``Fraction`` and tests/test_compdis_oracle.py ties the two);
the float32 one rounds the exact sum to odd in float64 and then once to float32 (fma32; fma32_fraction says it with ``Fraction``).
Every other operation is numpy's, one ufunc per rounding: numpy does not contract.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
BLOCK_PTS = 1024                       # compdis_math.h:20  kBlockPts
LANE_PTS = 4                           # compdis_math.h:19  kPtsPerThread
PREP_CHUNK = 4096                      # compdis_math.h:17  kPrepChunk
PREP_THREADS = 256                     # compdis_math.h:16  kPrepThreads
CLOSE = 35.0                           # himo_amd/compdis.py CLOSE_DISTANCE_DEFAULT
BOX = {"av2": ([-1.5, -1.5, -2.0], [1.5, 1.5, 2.0]), "scania": ([-9.5, -3 / 2, 0], [5, 2.760004 / 2, 5])}   # compdis.py EGO_BOX
NAN_KEY0 = 0xFFFFFFFF                  # key_to_float(0): what a frame with no element above -inf decodes to


# ---- fused multiply-adds -------------------------------------------------------------------------------------------------------
def fma_fraction(a, b, c):
    """the definition: the exact rational a b + c, rounded once (``float`` of a Fraction is correctly rounded)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _split(x):
    m, e = math.frexp(x)
    return int(m * 9007199254740992.0), e - 53


def fma64(a, b, c):
    """fma_fraction in integer arithmetic (a fifth of the time): the exact sum as an integer times a power of two, rounded by
    ``float(int)`` (half to even).  Non-finite operands, zero products and results near the subnormal range take the plain way."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    ma, ea = _split(a)
    mb, eb = _split(b)
    n = ma * mb
    if n == 0:
        return a * b + c                                       # the product is an exact zero: one rounding already
    mc, ec = _split(c)
    e = ea + eb
    if mc == 0:
        tot, ex = n, e
    elif e >= ec:
        tot, ex = (n << (e - ec)) + mc, ec
    else:
        tot, ex = n + (mc << (ec - e)), e
    if tot == 0:
        return 0.0
    if tot.bit_length() + ex > 1000 or tot.bit_length() + ex < -960 or tot.bit_length() > 1000:
        return fma_fraction(a, b, c)
    return math.ldexp(float(tot), ex)


def fma64v(a, b, c):
    """elementwise fma64 of float64 arrays (b may be a scalar)"""
    a, c = np.asarray(a, F64), np.asarray(c, F64)
    b = np.broadcast_to(np.asarray(b, F64), a.shape)
    return np.array([fma64(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=F64).reshape(a.shape)


def fma32(a, b, c):
    """float32 fused multiply-add of arrays: the product of two float32 is exact in float64; the sum is rounded to ODD in float64
    (two_sum says which way the exact value lies), and a value rounded to odd at 53 bits rounds to 24 bits as the exact one does"""
    with np.errstate(all="ignore"):
        p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
        c = np.broadcast_to(np.asarray(c, F32).astype(F64), p.shape)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        need = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(need, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def round_f32(x: Fraction):
    """a rational rounded ONCE to float32, half to even (finite, normal range or not)"""
    f = F32(float(x))
    cands = {float(f), float(np.nextafter(f, F32(-np.inf))), float(np.nextafter(f, F32(np.inf)))}
    best = min((c for c in cands if math.isfinite(c)),
               key=lambda c: (abs(Fraction(c) - x), int(np.array(c, F32).view(np.uint32)) & 1))
    return F32(best)


def fma32_fraction(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ---- the per-point chain -------------------------------------------------------------------------------------------------------
WRONG_CHAIN = ("mul_then_div", "k_reversed", "dt0_f64", "p_plus_t_first")


def pose_flow(ego, pc_xyz, f32, single_row=False, wrong=None):
    """R p + t - p in the chain's dtype, [n, 3]: pose_flow_f64 (compdis_math.h:51-61) or the float32 line :78"""
    ego = np.asarray(ego, F64)
    T = F32 if f32 else F64
    R, t = ego[:3, :3].astype(T), ego[:3, 3].astype(T)                            # :71-72 (float) casts of the float64 transform
    p = np.ascontiguousarray(pc_xyz, F32).reshape(-1, 3).astype(T)
    fma = fma32 if f32 else fma64v
    out = np.empty(p.shape, T)
    with np.errstate(all="ignore"):
        for c in range(3):
            order = (1, 0, 2) if (single_row and not f32) else (0, 1, 2)            # :58-59
            if wrong == "k_reversed":
                order = order[::-1]
            k0, k1, k2 = order
            dot = fma(p[:, k2], R[c, k2], fma(p[:, k1], R[c, k1], p[:, k0] * R[c, k0]))
            out[:, c] = dot + (t[c] - p[:, c]) if wrong == "p_plus_t_first" else (dot + t[c]) - p[:, c]   # :60, :78
    return out


def chain(ego, pc_xyz, flow, lidar_dt, fmax, sensor_dt, f32, raw, single_row=False, wrong=None):
    """compdis_math.h:66-100.  ego: [>=3, 4] float64 (rows R | t);  pc_xyz, flow: [n, 3] float32;  lidar_dt: [n] float32;  fmax: the
    frame's float32 maximum.  Returns comp_dis [n, 3] float32, refined [n, 3] float32 and the norm column [n] float32.
    ``single_row``: the dgemv order of compdis_math.h:58 (float64 chain only, as in the kernel).  ``wrong``: one line changed."""
    ego = np.asarray(ego, F64)
    pc = np.ascontiguousarray(pc_xyz, F32).reshape(-1, 3)
    n = pc.shape[0]
    dt = np.asarray(lidar_dt, F32).reshape(n)
    with np.errstate(all="ignore"):
        if wrong == "dt0_f64":
            dt0 = F64(fmax) - dt.astype(F64)
        else:
            dt0 = F32(fmax) - dt                                                  # :69, float32
        T = F32 if f32 else F64
        sdt = T(sensor_dt)
        p = pc.astype(T)
        fl = np.zeros((n, 3), T) if raw else np.ascontiguousarray(flow, F32).reshape(n, 3).astype(T)
        pfs = pose_flow(ego, pc, f32, single_row, wrong)
        cd, rf, est = np.empty((n, 3), F32), np.empty((n, 3), F32), np.empty((n, 3), T)
        for c in range(3):
            pf = pfs[:, c]
            e = np.zeros(n, T) if raw else fl[:, c] - pf                          # :79, :92
            d0 = dt0.astype(T)
            v = e * d0 / sdt if wrong == "mul_then_div" else e / sdt * d0          # :80, :93
            cd[:, c] = v.astype(F32)                                              # :81, :94
            rf[:, c] = (p[:, c] + v).astype(F32)                                  # :82, :95
            est[:, c] = e
        nrm = np.sqrt((est[:, 0] * est[:, 0] + est[:, 1] * est[:, 1]) + est[:, 2] * est[:, 2]).astype(F32)   # :85, :98
    return cd, rf, nrm


# ---- the per-frame maximum -----------------------------------------------------------------------------------------------------
def float_to_key(v):
    b = np.asarray(v, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def frame_max(lidar_dt, wrong=None):
    """the kernel's rule (compdis.hip:108-172): NaN elements are dropped (fmaxf), a frame with no element above -inf -- empty, all NaN,
    all -inf -- leaves key 0, which decodes to a NaN; otherwise the float32 maximum in the order of the keys (+0 above -0)"""
    dt = np.asarray(lidar_dt, F32).reshape(-1)
    if wrong == "nan_propagating":
        return F32(np.max(dt)) if dt.size else key_to_float(np.uint32(0))[()]
    keep = dt[~np.isnan(dt)]
    keep = keep[keep > -np.inf]
    if keep.size == 0:
        return key_to_float(np.uint32(0))[()]
    return key_to_float(float_to_key(keep).max())[()]


def python_max(lidar_dt):
    """save_zip.py:120, eval.py:299: Python's max() over the array: a NaN is kept only if it comes FIRST (every later comparison
    with it is False), and of -0.0 and +0.0 the first one met stays.  Raises ValueError on an empty sweep, as the reference does."""
    return max(np.asarray(lidar_dt, F32).reshape(-1))


# ---- the evaluation mask -------------------------------------------------------------------------------------------------------
WRONG_MASK = ("dist_lt", "face_ge", "gm_eq_1")


def mask(pc_xyz, gm, valid, bmin, bmax, close, wrong=None):
    """compdis_math.h:103-109.  bmin, bmax, close are rounded to float32 as the entry points receive them; valid None = all ones."""
    p = np.asarray(pc_xyz, F32).reshape(-1, 3)
    lo, hi, close = np.asarray(bmin, F32), np.asarray(bmax, F32), F32(close)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        d = np.sqrt(px * px + py * py)                                            # three float32 roundings
    near = d < close if wrong == "dist_lt" else d <= close
    x_lo = px >= lo[0] if wrong == "face_ge" else px > lo[0]
    inside = x_lo & (px < hi[0]) & (py > lo[1]) & (py < hi[1]) & (pz > lo[2]) & (pz < hi[2])
    gm = np.asarray(gm, np.uint8)
    ground = gm == 1 if wrong == "gm_eq_1" else gm != 0
    ok = np.ones(len(p), bool) if valid is None else np.asarray(valid, np.uint8) != 0
    return (near & ~ground & ~inside & ok).astype(np.uint8)


# ---- the ground-truth writer's body --------------------------------------------------------------------------------------------
GT_CD, GT_MASK, GT_CAT, GT_INST, GT_NORM, GT_PC = 0, 3, 4, 5, 6, 7                 # compdis_gt.hip:22


def gt_body(starts, nbytes, cd, m, cat, inst, nrm, pc_xyz):
    """one sweep's body: ``starts`` (ten byte offsets, -1 = absent) and ``nbytes`` as himo_gt_column_starts returns them"""
    out = np.zeros(int(nbytes), np.uint8)

    def put(col, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        out[int(starts[col]):int(starts[col]) + b.size] = b
    for c in range(3):
        put(GT_CD + c, np.ascontiguousarray(cd[:, c], F32))
        put(GT_PC + c, np.ascontiguousarray(np.asarray(pc_xyz, F32)[:, c]))
    put(GT_MASK, np.asarray(m, np.uint8))
    if starts[GT_CAT] >= 0:
        put(GT_CAT, np.asarray(cat, np.uint8))
    if starts[GT_INST] >= 0:
        put(GT_INST, np.asarray(inst, np.uint32))
    put(GT_NORM, np.asarray(nrm, F32))
    return out


# ---- the ego transform ---------------------------------------------------------------------------------------------------------
WRONG_LU = ("no_swap", "last_maximal")


def lu_ego(pose0, pose1, wrong=None, trace=None):
    """compute_ego of compdis.hip:35-88 in its order: LU with partial pivoting (first maximal pivot), the inverse by substitution on
    the identity, a k-ordered product whose additions are fused.  [3, 4] float64, all NaN for a singular pose1.  ``trace``: a list
    that receives (k, pivot row, tie) for every column."""
    a = [[float(v) for v in row] for row in np.asarray(pose1, F64).reshape(4, 4)]
    p0 = [[float(v) for v in row] for row in np.asarray(pose0, F64).reshape(4, 4)]
    b = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    singular = False
    for k in range(4):
        p, best = k, abs(a[k][k])
        for r in range(k + 1, 4):
            v = abs(a[r][k])
            if v > best or (wrong == "last_maximal" and v == best):
                best, p = v, r
        tie = best > 0.0 and sum(1 for r in range(k, 4) if abs(a[r][k]) == best) > 1
        if wrong == "no_swap":
            p, best = k, abs(a[k][k])
        if trace is not None:
            trace.append((k, p, tie))
        singular = singular or not best > 0.0
        if p != k:
            a[k], a[p] = a[p], a[k]
            b[k], b[p] = b[p], b[k]
        with np.errstate(all="ignore"):
            rp = float(F64(1.0) / F64(a[k][k]))
            for r in range(k + 1, 4):
                a[r][k] = float(F64(a[r][k]) * F64(rp))
                for c in range(k + 1, 4):
                    a[r][c] = float(F64(a[r][c]) - F64(a[r][k]) * F64(a[k][c]))
    with np.errstate(all="ignore"):
        for col in range(4):
            for r in range(1, 4):
                for c in range(r):
                    b[r][col] = float(F64(b[r][col]) - F64(a[r][c]) * F64(b[c][col]))
            for r in range(3, -1, -1):
                for c in range(r + 1, 4):
                    b[r][col] = float(F64(b[r][col]) - F64(a[r][c]) * F64(b[c][col]))
                b[r][col] = float(F64(b[r][col]) / F64(a[r][r]))
        out = np.empty((3, 4), F64)
        for r in range(3):
            for c in range(4):
                s = float(F64(b[r][0]) * F64(p0[0][c]))
                for k in range(1, 4):
                    s = fma64(b[r][k], p0[k][c], s)
                out[r, c] = math.nan if singular else s
    return out


def pivots(pose1):
    """(number of row swaps, whether a column had a tie between maximal candidates) of lu_ego on pose1"""
    tr = []
    lu_ego(np.eye(4), pose1, trace=tr)
    return sum(1 for k, p, _ in tr if p != k), any(t for _, _, t in tr)


def _frac_inv(A):
    n = 4
    M = [[Fraction(float(A[r][c])) for c in range(n)] + [Fraction(int(r == c)) for c in range(n)] for r in range(n)]
    for k in range(n):
        piv = next((r for r in range(k, n) if M[r][k] != 0), None)
        if piv is None:
            return None
        M[k], M[piv] = M[piv], M[k]
        d = M[k][k]
        M[k] = [v / d for v in M[k]]
        for r in range(n):
            if r != k and M[r][k] != 0:
                f = M[r][k]
                M[r] = [x - f * y for x, y in zip(M[r], M[k])]
    return [row[n:] for row in M]


def exact_ego(pose0, pose1):
    """inv(pose1) @ pose0 in rational arithmetic: a 4x4 list of Fractions, None for a singular pose1"""
    X = _frac_inv(np.asarray(pose1, F64).reshape(4, 4))
    if X is None:
        return None
    P = [[Fraction(float(v)) for v in row] for row in np.asarray(pose0, F64).reshape(4, 4)]
    return [[sum(X[r][k] * P[k][c] for k in range(4)) for c in range(4)] for r in range(4)]


def ego_bound(pose0, pose1):
    """The forward error of LU with partial pivoting followed by the 4x4 product, elementwise [4, 4]:

        16 u cond_inf(pose1) (|inv(pose1)| |pose0|),   u = 2^-53.

    Factor and solve of an n x n system in floating point leave |X^ - X| <= 3 n u |X| |L^| |U^| |X^| (Higham, Accuracy and Stability,
    9.3 and 14.1 with gamma_3n ~ 3 n u); with partial pivoting on these well-scaled 4x4 poses | |L^| |U^| | is of the size of |A|, so the
    relative error of the inverse is 3 n u cond = 12 u cond; the k-ordered product of four terms adds gamma_4 = 4 u of |X| |pose0|,
    which cond >= 1 covers.  Together 16 u cond (|X| |pose0|).  None for a singular pose1."""
    A = np.asarray(pose1, F64).reshape(4, 4)
    X = _frac_inv(A)
    if X is None:
        return None
    Xa = np.array([[float(abs(v)) for v in row] for row in X])
    cond = float(np.abs(A).sum(1).max() * Xa.sum(1).max())
    return 16.0 * 2.0 ** -53 * cond * (Xa @ np.abs(np.asarray(pose0, F64).reshape(4, 4)))


def ego_ratio(got, pose0, pose1):
    """the largest |got - exact| / bound over the [3, 4] transform (0 / 0 counts as 0; anything over a zero bound as inf)"""
    ex, bd = exact_ego(pose0, pose1), ego_bound(pose0, pose1)
    worst = 0.0
    for r in range(3):
        for c in range(4):
            g = float(got[r][c])
            if not math.isfinite(g):
                return math.inf
            err = float(abs(Fraction(g) - ex[r][c]))
            if err > 0.0:
                worst = max(worst, err / bd[r, c] if bd[r, c] > 0.0 else math.inf)
    return worst


# ---- the launch conditions, mirrored ---------------------------------------------------------------------------------------------
def segment_of(offsets, i):
    """blockops.h:17-24: the largest k in [0, n) with offsets[k] <= i"""
    lo, hi = 0, len(offsets) - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if offsets[mid] <= i:
            lo = mid
        else:
            hi = mid
    return lo


def frame_ids(offsets, wrong=None):
    """the frame of every packed row; ``block_first_frame``: the frame of the row's 1024-point block start instead"""
    o = np.asarray(offsets, np.int64)
    ids = np.repeat(np.arange(len(o) - 1), np.diff(o))
    if wrong == "block_first_frame":
        ids = np.array([segment_of(o, (i // BLOCK_PTS) * BLOCK_PTS) for i in range(int(o[-1]))], dtype=np.int64)
    return ids


def block_paths(offsets, vec):
    """which branches of compdis_kernel (compdis.hip:215-232) the blocks of a batch take: 'uniform' (a block inside one frame whose
    lanes take the vector path; needs ``vec``), 'straddling' (a frame boundary inside the block), 'tail' (a lane whose four points
    the block's end cuts, in a uniform block)"""
    o = [int(v) for v in offsets]
    total, met = o[-1], set()
    for bstart in range(0, total, BLOCK_PTS):
        bend = min(bstart + BLOCK_PTS, total)
        f0 = segment_of(o, bstart)
        if o[f0 + 1] >= bend:
            if vec and bend - bstart >= LANE_PTS:
                met.add("uniform")
            if (bend - bstart) % LANE_PTS:
                met.add("tail")
        else:
            met.add("straddling")
    return met


def is_vec(c):
    """compdis.hip:373-378 on a case of the matrix: the offsets (bytes) of the operands the launch looks at"""
    off = c["off"]
    looked = ["pc", "dt", "cd"] + ([] if c["raw"] else ["flow"]) + (["rf"] if c["refined"] else [])
    if c["mask"]:
        looked += ["mask", "gm"] + (["valid"] if c["scania"] else [])
    return c["stride"] in (3, 4) and not any(off.get(k) for k in looked)


def compdis_instance(stride, f32, aligned16, mask_aligned4):
    """compdis.hip:373-387"""
    vec = stride in (3, 4) and aligned16 and mask_aligned4
    return f"compdis_kernel<{stride if vec else 0}, {'f32' if f32 else 'f64'}>", vec


def gt_instance(stride, f32, pc_aligned16):
    """compdis_gt.hip:281-288"""
    return f"compdis_gt_kernel<{4 if stride == 4 and pc_aligned16 else 0}, {'f32' if f32 else 'f64'}>"


# ---- poses ---------------------------------------------------------------------------------------------------------------------
def _rot(yaw, pitch=0.0, roll=0.0):
    cz, sz, cy, sy, cx, sx = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


def _pose(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


def pose_pair(kind, f32=False):
    """(pose0, pose1) float64 [4, 4]; ``f32``: every element a float32 value (the float32 chain's poses)"""
    p0 = _pose(_rot(0.011, 0.002, -0.003), [1.25, -0.4, 0.03])
    if kind == "identity":
        p0, p1 = np.eye(4), np.eye(4)
    elif kind == "shift":                                      # a float32-exact translation: the pose flow is exact, flow can cancel it
        p0, p1 = _pose(np.eye(3), [0.5, -0.25, 0.125]), np.eye(4)
    elif kind == "small":
        p1 = _pose(_rot(0.02), [0.3, 0.1, 0.0])
    elif kind == "yaw90":                                      # |cos| ~ 6e-17 on the diagonal: one swap in the first column
        p1 = _pose(_rot(math.pi / 2), [2.0, -1.0, 0.1])
    elif kind == "yaw135roll":                                 # (a hundredth of a radian short of 135 degrees: no tie once rounded to float32)
        p1 = _pose(_rot(3 * math.pi / 4 - 0.01, 0.3, 1.9), [-3.0, 2.0, 0.5])
    elif kind == "tie45":                                      # |a00| == |a10| in bits: "first maximal" keeps row 0
        v = 0.7071067811865476
        p1 = _pose(np.array([[v, -v, 0], [v, v, 0], [0, 0, 1.0]]) @ _rot(0.0, 0.0, 0.3), [1.0, 2.0, -0.5])
    elif kind == "far":                                        # a map frame a thousand kilometres from its origin
        p0 = _pose(_rot(0.4, 0.01, 0.0), [1.0e6 + 3.0, -2.0e6, 50.0])
        p1 = _pose(_rot(0.41, 0.01, 0.0), [1.0e6, -2.0e6 + 1.0, 50.0])
    elif kind == "cond1e8":                                    # rotation scaled by 1e-4 beside a translation of 60 m
        p1 = _pose(_rot(0.7, 0.1, 0.2) * 1.0e-4, [60.0, 30.0, 2.0])
    elif kind == "singular":
        p1 = _pose(_rot(0.02), [0.3, 0.1, 0.0])
        p1[2, :] = p1[0, :] * 2.0                              # exactly dependent rows
    else:
        raise KeyError(kind)
    if f32:
        p0, p1 = p0.astype(F32).astype(F64), p1.astype(F32).astype(F64)
    return p0, p1


POSE_KINDS = ("identity", "small", "yaw90", "yaw135roll", "tie45", "far", "cond1e8")


# ---- the matrix ----------------------------------------------------------------------------------------------------------------
def _case(sizes, promises=(), **kw):
    c = dict(sizes=list(sizes), promises=tuple(promises), stride=4, off={}, pose="small", f32=False, raw=False, box="av2", scania=False,
             valid=False, refined=True, mask=True, dt="uniform", sensor_dt=0.1, thresholds=False, columns=3, cancel=False, seed=0)
    c.update(kw)
    return c


_rng0 = np.random.default_rng(20260130)
_S300 = [int(v) for v in _rng0.integers(1, 8, 300)]
_S513 = [0 if i % 3 == 2 else int(v) for i, v in enumerate(_rng0.integers(1, 6, 513))]
_L = [1022, 5, 1021, 1027]            # blocks: straddling, straddling, uniform and full, uniform with a tail of 3
_D = [4100, 9]                        # a chunk boundary inside the first frame, a frame boundary inside the second chunk

CASES = {
    # frame sizes
    "n1": _case([1], ("one_row_sweep", "tail")),
    "n2": _case([2], ("tail",), sensor_dt=0.2),
    "n4": _case([4], ("uniform",), sensor_dt=10.0),
    "n1023": _case([1023], ("uniform", "tail"), thresholds=True),
    "n1024": _case([1024], ("uniform",), f32=True),
    "n1025": _case([1025], ("uniform", "tail")),
    "edge_1024_1024": _case([1024, 1024], ("block_edge_boundary", "uniform"), pose="mixed"),
    "lane_1022_5_1021": _case([1022, 5, 1021], ("lane_group_boundary", "straddling"), pose="mixed"),
    "tail3_1027": _case([1027], ("tail3_after_full_block",), columns=0),
    "chunks_4095_2_4097": _case([4095, 2, 4097], ("multi_round_chunk", "straddling", "uniform"), pose="mixed", thresholds=True),
    "empties_0_7_0_4096_0": _case([0, 7, 0, 4096, 0], ("empty_frames", "straddling"), pose="mixed"),
    "total0": _case([0, 0, 0], ("total_zero",)),
    "frames300": _case(_S300, ("gt256_frames", "many_in_block", "multi_round_chunk", "one_row_sweep"), pose="mixed"),
    "frames513_ego": _case(_S513, ("gt256_frames", "gt512_frames", "empty_frames", "one_row_sweep"), pose="mixed", pose_is_ego=True),
    "frames513_f32": _case(_S513, ("gt256_frames", "empty_frames"), pose="mixed", f32=True, sensor_dt=0.2),
    "off3_2048": _case([3, 2048], ("gt_257th_group",), thresholds=True),
    "off1_1025": _case([1, 1025], ("one_row_sweep", "straddling"), f32=True),   # (its second block is cut short: no 257th group here)
    "off1_2048": _case([1, 2048], ("gt_257th_group", "one_row_sweep"), f32=True),
    "mod8": _case([8, 9, 10, 11, 12, 13, 14, 15, 1, 2, 3, 4, 5, 6, 7], ("every_n_mod_8", "one_row_sweep"), pose="mixed"),
    "mod8_nolabels": _case([15, 14, 13, 12, 11, 10, 9, 8], ("every_n_mod_8",), columns=0, f32=True),
    # layouts
    "stride3": _case(_L, ("uniform", "straddling", "tail"), stride=3, thresholds=True),
    "stride3_f32": _case(_L, ("uniform",), stride=3, f32=True),
    "stride5": _case(_L, ("straddling",), stride=5, thresholds=True),
    "stride5_f32": _case(_L, ("straddling",), stride=5, f32=True, pose="mixed"),
    "off_pc0": _case(_L, (), off={"pc": 4}),
    "off_flow": _case(_L, (), off={"flow": 4}),
    "off_lidar_dt": _case(_L + [3100], ("multi_round_chunk",), off={"dt": 4}),
    "off_comp_dis": _case(_L, (), off={"cd": 4}),
    "off_refined": _case(_L, (), off={"rf": 4}),
    "off_mask": _case(_L, (), off={"mask": 1}, thresholds=True),
    "off_gm0": _case(_L, (), off={"gm": 1}, thresholds=True),
    "off_valid": _case(_L, (), off={"valid": 1}, scania=True, valid=True, box="scania", thresholds=True),
    "no_refined": _case(_L, ("uniform",), refined=False),
    "no_mask": _case(_L, ("uniform",), mask=False),
    "scania": _case(_L, ("uniform", "thresholds"), scania=True, valid=True, box="scania", thresholds=True),
    "av2_thresholds": _case(_L, ("uniform", "thresholds"), thresholds=True, valid=True),
    "raw_mask": _case(_L, ("uniform",), raw=True, thresholds=True),
    "raw_f32": _case(_L, ("uniform",), raw=True, f32=True, off={"flow": 4}, thresholds=True),   # (RAW never looks at flow)
    # lidar_dt
    "dt_all_equal": _case(_D, (), dt="all_equal"),
    "dt_all_negative": _case(_D, (), dt="all_negative"),
    "dt_one_inf": _case(_D, (), dt="one_inf"),
    "dt_all_ninf__the_maximum_is_nan": _case(_D, (), dt="all_ninf"),
    "dt_nan_first__dropped_where_python_max_keeps_it": _case(_D, ("python_max_differs",), dt="nan_first"),
    "dt_nan_last__dropped_as_python_max_drops_it": _case(_D, (), dt="nan_last"),
    "dt_all_nan__the_maximum_is_nan": _case(_D, (), dt="all_nan"),
    "dt_max_last_of_chunk": _case(_D, ("max_last_of_chunk",), dt="max_last_of_chunk"),
    "dt_max_first_of_next_chunk": _case(_D, ("max_first_of_next_chunk",), dt="max_first_of_next_chunk"),
    "dt_zeros_mixed__plus_zero_wins": _case(_D, (), dt="zeros_mixed"),
    "dt_denormal_dt0": _case(_D, ("denormal_dt0",), dt="denormal"),
    "dt_denormal_dt0_f32": _case(_D, ("denormal_dt0",), dt="denormal", f32=True),
    "singular_middle": _case([5, 1030, 7], ("singular_batch", "straddling"), pose=("small", "singular", "yaw90")),
    # numbers
    "cancel_to_zero": _case([5, 1030], ("cancel_zero",), pose="shift", cancel=True),
    "cancel_to_zero_f32": _case([5, 1030], ("cancel_zero",), pose="shift", cancel=True, f32=True),
}
for _k in POSE_KINDS:                                            # poses, each in both chains and (in the GPU test) as POSE_IS_EGO too
    for _f in (False, True):
        _p = {"yaw90": ("swap1",), "yaw135roll": ("swap2",), "tie45": ("tie",)}.get(_k, ())
        CASES[f"pose_{_k}_{'f32' if _f else 'f64'}"] = _case([2, 1029], _p, pose=_k, f32=_f, both_ego_modes=True,
                                                             sensor_dt=(0.2 if _k == "far" else 0.1))
for _i, _k in enumerate(CASES):
    CASES[_k]["seed"] = 1000 + _i
CASE_NAMES = tuple(CASES)


def threshold_points(box, close=CLOSE):
    """points ON every threshold of eval_mask_point and one float32 step to either side: [k, 3] float32 and what each row is"""
    lo, hi = np.asarray(BOX[box][0], F32), np.asarray(BOX[box][1], F32)
    close = F32(close)
    rows, what = [], []

    def norm(x, y):
        return np.sqrt(x * x + y * y)
    x0, y0 = F32(30.0) * close / F32(50.0), F32(40.0) * close / F32(50.0)         # 21, 28: the float32 norm is exactly 35
    assert norm(x0, y0) == close
    rows.append((x0, y0, F32(0.5))); what.append("norm == close")
    for side, lab in ((np.inf, "norm one step above close"), (-np.inf, "norm one step below close")):
        x = x0
        while norm(x, y0) == close:
            x = np.nextafter(x, F32(side))
        assert norm(x, y0) == np.nextafter(close, F32(side))
        rows.append((x, y0, F32(0.5))); what.append(lab)
    mid = ((lo.astype(F64) + hi.astype(F64)) / 2).astype(F32)
    for a in range(3):
        for bound, out_dir, lab in ((lo[a], -np.inf, "min"), (hi[a], np.inf, "max")):
            for v, w in ((bound, "on"), (np.nextafter(bound, F32(-out_dir)), "inside"), (np.nextafter(bound, F32(out_dir)), "outside")):
                p = mid.copy()
                p[a] = v
                rows.append(tuple(p)); what.append(f"{w} the {lab} face of axis {a}")
    return np.array(rows, F32), what


class Data:
    pass


_BUILT = {}


def build(name):
    """the operands of a case, from its seed: offsets, pc [T, stride], flow, lidar_dt, gm, valid, category, instance, pose0 / pose1 [F, 4, 4]"""
    if name in _BUILT:
        return _BUILT[name]
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    d = Data()
    d.name, d.c = name, c
    d.sizes = list(c["sizes"])
    d.offsets = np.concatenate([[0], np.cumsum(d.sizes)]).astype(np.int64)
    F, T = len(d.sizes), int(d.offsets[-1])
    d.F, d.T = F, T
    xyz = rng.uniform(-200.0, 200.0, (T, 3))
    near = rng.uniform(size=T) < 0.5
    xyz[near] *= 0.15                                            # half the rows within 30 m of the sensor in each axis
    inside = rng.uniform(size=T) < 0.1
    xyz[inside] = rng.uniform(-2.5, 2.5, (int(inside.sum()), 3))
    xyz[:, 2] = np.where(inside, xyz[:, 2], xyz[:, 2] * 0.05)
    d.pc = np.zeros((T, c["stride"]), F32)
    d.pc[:, :3] = xyz
    if c["stride"] > 3:
        d.pc[:, 3:] = rng.uniform(0, 1, (T, c["stride"] - 3))
    d.flow = rng.uniform(-200.0, 200.0, (T, 3)).astype(F32)
    small = rng.uniform(size=T) < 0.7
    d.flow[small] = (d.flow[small] * F32(0.01))
    d.gm = rng.choice(np.array([0, 0, 0, 1, 2, 255], np.uint8), T)
    d.valid = rng.choice(np.array([1, 1, 1, 0, 2, 255], np.uint8), T) if c["valid"] else None
    d.cat = rng.integers(0, 31, T).astype(np.uint8)
    d.inst = rng.integers(0, 2 ** 32, T, dtype=np.uint64).astype(np.uint32)
    d.th_rows, d.th_what = np.zeros(0, np.int64), []
    if c["thresholds"]:
        pts, what = threshold_points(c["box"])
        f = int(np.argmax(d.sizes))
        assert d.sizes[f] >= 2 * len(pts)
        at = int(d.offsets[f]) + 3                               # not on a lane's group boundary
        d.th_rows, d.th_what = np.arange(at, at + len(pts)), what
        d.pc[d.th_rows, :3] = pts
        d.gm[d.th_rows] = 0
        if d.valid is not None:
            d.valid[d.th_rows] = 1
    # lidar_dt
    dt = rng.uniform(0.0, 0.1, T).astype(F32)
    kind = c["dt"]
    f0 = slice(0, d.sizes[0])                                    # the first frame carries the edge; the others stay ordinary
    if kind == "all_equal":
        dt[f0] = F32(0.05)
    elif kind == "all_negative":
        dt[f0] = -dt[f0] - F32(0.001)
    elif kind == "one_inf":
        dt[d.sizes[0] // 2] = np.inf
    elif kind == "all_ninf":
        dt[f0] = -np.inf
    elif kind == "nan_first":
        dt[0] = np.nan
    elif kind == "nan_last":
        dt[d.sizes[0] - 1] = np.nan
    elif kind == "all_nan":
        dt[f0] = np.nan
    elif kind == "max_last_of_chunk":
        dt[PREP_CHUNK - 1] = F32(0.25)
    elif kind == "max_first_of_next_chunk":
        dt[PREP_CHUNK] = F32(0.25)
    elif kind == "zeros_mixed":
        dt[f0] = np.where(rng.uniform(size=d.sizes[0]) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
        dt[0] = F32(-0.0)                                        # Python's max() would keep this first -0.0; the keys put +0 above it
    elif kind == "denormal":
        base = F32(1.5e-38)                                      # a normal float32 just above the smallest; differences are subnormal
        dt[f0] = (np.full(d.sizes[0], base, F32).view(np.uint32) + rng.integers(0, 4000, d.sizes[0]).astype(np.uint32)).view(F32)
    else:
        assert kind == "uniform", kind
    d.dt = dt
    # poses
    kinds = POSE_KINDS if c["pose"] == "mixed" else (c["pose"] if isinstance(c["pose"], tuple) else (c["pose"],))
    d.pose_kinds = [kinds[f % len(kinds)] for f in range(F)]
    pairs = {k: pose_pair(k, c["f32"]) for k in kinds}
    d.pose0 = np.stack([pairs[k][0] for k in d.pose_kinds]) if F else np.zeros((0, 4, 4))
    d.pose1 = np.stack([pairs[k][1] for k in d.pose_kinds]) if F else np.zeros((0, 4, 4))
    # static rows: the flow IS the ego motion, rounded to float32 -- est_flow is then the rounding residue, where the last bits of the
    # pose flow (the k-order, the place of t, the single_row order) decide bits of the result even after the cast to float32
    static = rng.uniform(size=T) < 0.3
    ids = frame_ids(d.offsets)
    egos = numpy_egos(d)
    for f in range(F):
        rows = np.nonzero(static & (ids == f))[0]
        if len(rows):
            with np.errstate(all="ignore"):
                d.flow[rows] = pose_flow(egos[f], d.pc[rows, :3], c["f32"]).astype(F32)
    if c["cancel"]:                                              # rows whose flow IS the pose flow, to the last bit: est_flow is an exact 0
        ego = np.linalg.inv(d.pose1[0]) @ d.pose0[0]
        rows = np.arange(0, T, 3)
        pf = pose_flow(ego, d.pc[rows, :3], c["f32"]).astype(F64)
        assert np.array_equal(pf.astype(F32).astype(F64), pf)
        d.flow[rows] = pf.astype(F32)
        d.cancel_rows = rows
    _BUILT[name] = d
    return d


def numpy_egos(d):
    """save_zip.py:115 for every frame (float64): what POSE_IS_EGO batches are given"""
    def one(p0, p1):
        try:
            return np.linalg.inv(p1) @ p0
        except np.linalg.LinAlgError:                              # (batch mode has no error to raise: the kernel's transform is NaN)
            return np.full((4, 4), np.nan)
    return np.stack([one(d.pose0[f], d.pose1[f]) for f in range(d.F)]) if d.F else np.zeros((0, 4, 4))


def maxima(d, wrong=None):
    return np.array([frame_max(d.dt[d.offsets[f]:d.offsets[f + 1]], wrong) for f in range(d.F)], F32)


def points(d, egos, fmaxs, wrong=None, gt=False):
    """the whole batch through ``chain`` and ``mask``: comp_dis, refined, norm, mask.  ``egos`` [F, >=3, 4] and ``fmaxs`` [F] are the
    device's own (read back from the workspace) in the GPU test.  ``gt``: one-row sweeps take the single_row order (compdis_gt.hip:118).
    ``wrong``: a variant of chain / mask, 'block_first_frame' or 'single_row_for_two'."""
    c = d.c
    ids = frame_ids(d.offsets, wrong if wrong == "block_first_frame" else None)
    cd, rf, nrm = np.zeros((d.T, 3), F32), np.zeros((d.T, 3), F32), np.zeros(d.T, F32)
    cw = wrong if wrong in WRONG_CHAIN else None
    for f in np.unique(ids):
        rows = np.nonzero(ids == f)[0]
        n_sweep = d.sizes[f]
        single = (gt and n_sweep == 1) or (wrong == "single_row_for_two" and n_sweep == 2)
        a, b, e = chain(egos[f], d.pc[rows, :3], d.flow[rows], d.dt[rows], fmaxs[f], c["sensor_dt"], c["f32"], c["raw"], single, cw)
        cd[rows], rf[rows], nrm[rows] = a, b, e
    lo, hi = BOX[c["box"]]
    m = mask(d.pc[:, :3], d.gm, d.valid if c["scania"] else None, lo, hi, CLOSE, wrong if wrong in WRONG_MASK else None)
    return cd, rf, nrm, m


# ---- the promises of the cases, proved with integer arithmetic -------------------------------------------------------------------
def promise(d, what):
    o = [int(v) for v in d.offsets]
    sizes, T = d.sizes, d.T
    inner = [v for v in o[1:-1] if 0 < v < T]                    # frame boundaries with rows on both sides
    vec = is_vec(d.c)
    if what in ("uniform", "straddling", "tail"):
        return what in block_paths(o, vec)
    if what == "block_edge_boundary":
        return any(v % BLOCK_PTS == 0 for v in inner)
    if what == "lane_group_boundary":
        return any(v % LANE_PTS for v in inner)
    if what == "tail3_after_full_block":
        return T > BLOCK_PTS and T % BLOCK_PTS == 3 and len(block_paths(o, vec) & {"uniform", "tail"}) == 2
    if what == "one_row_sweep":
        return 1 in sizes
    if what == "gt256_frames":
        return len(sizes) > PREP_THREADS
    if what == "gt512_frames":
        return len(sizes) > 2 * PREP_THREADS
    if what == "empty_frames":
        return 0 in sizes and T > 0
    if what == "total_zero":
        return T == 0 and len(sizes) > 1
    if what == "many_in_block":
        return max(len({segment_of(o, i) for i in range(b, min(b + BLOCK_PTS, T))}) for b in range(0, T, BLOCK_PTS)) >= 100
    if what == "multi_round_chunk":                              # a chunk of the max pre-pass that holds rows of several frames
        return any(segment_of(o, b) != segment_of(o, min(b + PREP_CHUNK, T) - 1) for b in range(0, T, PREP_CHUNK))
    if what == "gt_257th_group":                                 # a full block inside one sweep that starts off the sweep's groups of four
        return any(o[segment_of(o, b)] <= b and o[segment_of(o, b) + 1] >= b + BLOCK_PTS and (b - o[segment_of(o, b)]) % LANE_PTS
                   for b in range(0, T - BLOCK_PTS + 1, BLOCK_PTS))
    if what == "every_n_mod_8":
        return {s % 8 for s in sizes} == set(range(8))
    if what == "thresholds":
        lo, hi = np.asarray(BOX[d.c["box"]][0], F32), np.asarray(BOX[d.c["box"]][1], F32)
        p = d.pc[d.th_rows, :3]
        nr = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
        ok = {F32(CLOSE), np.nextafter(F32(CLOSE), F32(np.inf)), np.nextafter(F32(CLOSE), F32(-np.inf))} <= set(nr.tolist())
        for a in range(3):
            for bnd in (lo[a], hi[a]):
                want = {float(bnd), float(np.nextafter(bnd, F32(np.inf))), float(np.nextafter(bnd, F32(-np.inf)))}
                ok = ok and want <= set(p[:, a].astype(F64).tolist())
        return bool(ok) and len(d.th_rows) == 21
    if what in ("swap1", "swap2", "tie"):
        sw, tie = pivots(d.pose1[0])
        return {"swap1": sw == 1 and not tie, "swap2": sw >= 2, "tie": tie}[what]
    if what == "singular_batch":
        f = d.pose_kinds.index("singular")
        return 0 < f < d.F - 1 and exact_ego(d.pose0[f], d.pose1[f]) is None and all(k != "singular" for k in d.pose_kinds[:f] + d.pose_kinds[f + 1:])
    if what == "cancel_zero":
        cd, _, nrm, _ = points(d, numpy_egos(d), maxima(d))
        return bool((nrm[d.cancel_rows] == 0).all()) and bool((cd[d.cancel_rows] == 0).all()) and bool((nrm != 0).any())
    if what == "denormal_dt0":
        dt0 = maxima(d)[0] - d.dt[:sizes[0]]
        tiny = np.finfo(F32).tiny
        return bool(((dt0 > 0) & (dt0 < tiny)).sum() > sizes[0] // 2)
    if what == "max_last_of_chunk":
        return int(np.argmax(d.dt[:sizes[0]])) == PREP_CHUNK - 1 and sizes[0] > PREP_CHUNK
    if what == "max_first_of_next_chunk":
        return int(np.argmax(d.dt[:sizes[0]])) == PREP_CHUNK and sizes[0] > PREP_CHUNK
    if what == "python_max_differs":
        a, b = frame_max(d.dt[:sizes[0]]), python_max(d.dt[:sizes[0]])
        return bool(np.isnan(b)) and not bool(np.isnan(a))
    raise KeyError(what)
