"""EXACT brute-force restatement of the rule in csrc/dbscan.hip's header, and the inputs at which a cell-grid DBSCAN goes wrong --
test infrastructure, NOT product code.  It shares no code with oracle/dbscan_oracle.dbscan (cKDTree + sklearn): plain numpy, an
all-pairs neighbour matrix in float32.  tests/test_dbscan_oracle.py holds the two against each other on the CPU;
tests/test_dbscan_conformance_gpu.py holds the library against this one.

The rule: a row with a NaN, an infinite coordinate or a non-zero skip byte takes no part (label 0).  q is a neighbour of p when
(dx*dx + dy*dy) + dz*dz <= eps*eps in float32, every operation rounded on its own.  A point with at least min_pts neighbours,
itself included, is core; clusters are the connected components of the core points; a non-core point with core neighbours takes
the lowest root (= lowest core index of a cluster) among them; labels are 1 .. K in the order of the clusters' lowest core index.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

F = np.float32


def dbscan_exact(points, eps, min_pts, skip=None, chunk=512):
    """int32 labels of ``points[:, :3]`` under the rule above.  The neighbour matrix is built ``chunk`` rows at a time (the float32
    temporaries stay small); about a second for 8k participating points."""
    pts = np.ascontiguousarray(np.asarray(points)[:, :3], dtype=F)
    n = len(pts)
    labels = np.zeros(n, np.int32)
    take = np.isfinite(pts).all(1)
    if skip is not None:
        take &= np.asarray(skip).reshape(n) == 0
    idx = np.flatnonzero(take)
    m = len(idx)
    if m == 0:
        return labels
    x, y, z = (np.ascontiguousarray(pts[idx, k]) for k in range(3))
    e2 = F(eps) * F(eps)
    near = np.empty((m, m), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, m, chunk):
            b = min(a + chunk, m)
            d = x[None, :] - x[a:b, None]
            d2 = d * d
            d = y[None, :] - y[a:b, None]
            d2 += d * d                                         # (dx*dx + dy*dy), rounded
            d = z[None, :] - z[a:b, None]
            d2 += d * d                                         # ... + dz*dz, rounded
            near[a:b] = d2 <= e2
    core = near.sum(1) >= int(min_pts)
    root = np.full(m, -1, np.int64)                             # original index of the cluster's lowest core point
    ci = np.flatnonzero(core)
    c = len(ci)
    if c:
        cc = near[np.ix_(ci, ci)]
        seen = np.zeros(c, bool)
        for s in range(c):                                      # ascending: the first unseen core point is its component's lowest
            if seen[s]:
                continue
            comp = np.zeros(c, bool)
            comp[s] = True
            front = np.array([s])
            while len(front):
                reach = cc[front].any(0) & ~comp
                comp |= reach
                front = np.flatnonzero(reach)
            seen |= comp
            root[ci[comp]] = idx[ci[s]]
        big = np.iinfo(np.int64).max
        rest = np.flatnonzero(~core)
        for a in range(0, len(rest), chunk):
            rows = rest[a:a + chunk]
            low = np.where(near[np.ix_(rows, ci)], root[ci][None, :], big).min(1)
            root[rows] = np.where(low == big, -1, low)
        roots = np.unique(root[ci])
        has = root >= 0
        labels[idx[has]] = np.searchsorted(roots, root[has]) + 1
    return labels


# ---- floats in order -----------------------------------------------------------------------------------------------------------
def _key(x):
    """float32 -> int64 that orders like the floats (-0 and +0 share 0)"""
    i = np.asarray(x, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _unkey(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32).view(F)


def naive_cell(v, origin, cell):
    """the cell index a grid takes from floor((v - origin) * (1 / cell)) in float32 -- the expression whose hazard the pairs below sit on"""
    return np.floor((np.asarray(v, F) - F(origin)) * (F(1) / F(cell)))


def cell_hazard_pairs(eps, origin=-52.0, cell=None, n_cells=None, reach=8):
    """(k, 2) float32 coordinates (p, q), p < q, along one axis: fl(q - p)^2 <= fl(eps * eps), so p and q are neighbours when their
    other two coordinates agree, yet naive_cell puts them TWO cells apart (both inside the grid of ``n_cells`` cells).  Exhaustive and
    deterministic: every cell's first float is found by bisection over the ordered floats, then the ``reach`` floats below the first
    float of cell k are paired with the ``reach`` first floats of cell k + 1."""
    cell = eps if cell is None else cell
    n_cells = int(np.ceil(2 * abs(origin) / cell)) if n_cells is None else n_cells
    ks = np.arange(1, n_cells + 1, dtype=np.int64)              # first float of cells 1 .. n_cells
    lo = np.full(len(ks), _key(F(origin) - F(4 * cell)))        # cell < k here
    hi = np.full(len(ks), _key(F(origin) + F((n_cells + 4) * cell)))   # cell >= k here
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        up = naive_cell(_unkey(mid), origin, cell) >= ks
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    first = hi                                                  # first[k - 1] = key of the first float of cell k
    j = np.arange(reach, dtype=np.int64)
    k = np.arange(1, n_cells - 1)                               # p in cell k - 1 >= 0, q in cell k + 1 <= n_cells - 1
    p = _unkey(first[k - 1][:, None, None] - 1 - j[None, :, None])
    q = _unkey(first[k][:, None, None] + j[None, None, :])
    p, q = np.broadcast_arrays(p, q)
    d = q - p
    ok = (d * d <= F(eps) * F(eps)) & (naive_cell(q, origin, cell) - naive_cell(p, origin, cell) == 2)
    return np.stack([p[ok], q[ok]], 1).astype(F)


# ---- pairs whose distance test depends on whether a*b + c is contracted ---------------------------------------------------------
def _r32(v: Fraction) -> Fraction:
    """a non-negative rational rounded to float32 (nearest, ties to even; the normal range only)"""
    if v == 0:
        return v
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if v < Fraction(2) ** e:
        e -= 1
    unit = Fraction(2) ** (e - 23)
    return round(v / unit) * unit


def _sums(a, b, c, r):
    """the unfused sum and the five ways a compiler may contract it; a, b, c the exact squares, r rounds to float32"""
    A, B, C = r(a), r(b), r(c)
    return (r(r(A + B) + C),                                    # (dx*dx + dy*dy) + dz*dz
            r(r(b + A) + C),                                    # fma(dy,dy,dx*dx) + dz*dz
            r(c + r(b + A)),                                    # fma(dz,dz,fma(dy,dy,dx*dx))
            r(c + r(A + B)),                                    # fma(dz,dz,dx*dx + dy*dy)
            r(r(a + B) + C),                                    # fma(dx,dx,dy*dy) + dz*dz
            r(c + r(a + B)))                                    # fma(dz,dz,fma(dx,dx,dy*dy))


@functools.lru_cache(maxsize=None)
def contraction_pairs(eps, direction, seed=0, draws=4_000_000, span=40.0):
    """(p, q): float32 (k, 3) each, pairs at distance ~ eps with coordinates in +-span on which the float32 test
    (dx*dx + dy*dy) + dz*dz <= eps*eps gives one answer unfused and the OTHER answer under all five contractions of ``_sums``.
    direction "in_out": neighbours unfused, not neighbours fused; "out_in" the reverse.  Screened in float64 (float32 products are
    exact there), every kept pair confirmed in exact rational arithmetic; pairs nearer than 4 m to a kept pair are dropped, so each
    is isolated from the others for any eps <= 1."""
    assert direction in ("in_out", "out_in")
    rng = np.random.default_rng(seed)
    p = rng.uniform(-span, span, (draws, 3)).astype(F)
    u = rng.normal(size=(draws, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = (p.astype(np.float64) + u * (eps * (1.0 + rng.uniform(-2e-6, 2e-6, draws)))[:, None]).astype(F)
    d = (q - p).astype(np.float64)
    r = lambda v: v.astype(F).astype(np.float64)
    e2 = float(F(eps) * F(eps))
    s = _sums(d[:, 0] ** 2, d[:, 1] ** 2, d[:, 2] ** 2, r)
    inside = [v <= e2 for v in s]
    fused_in, fused_out = np.logical_and.reduce(inside[1:]), ~np.logical_or.reduce(inside[1:])
    cand = np.flatnonzero(inside[0] & fused_out if direction == "in_out" else ~inside[0] & fused_in)
    keep = []
    for i in cand:
        dx, dy, dz = (Fraction(float(v)) for v in d[i])
        exact = [v <= Fraction(e2) for v in _sums(dx * dx, dy * dy, dz * dz, _r32)]
        if exact[0] == (direction == "in_out") and all(v != exact[0] for v in exact[1:]) \
                and all(np.abs(p[i] - p[k]).max() > 4.0 for k in keep):
            keep.append(i)
    keep = np.asarray(keep, np.int64)
    p, q = p[keep], q[keep]
    p.flags.writeable = q.flags.writeable = False               # the cache hands the same arrays to every caller
    return p, q


# ---- clouds -------------------------------------------------------------------------------------------------------------------
def blobs(seed, n, n_blobs=6, lo=-48.0, hi=48.0, sigma=0.25, noise=0.3):
    """Gaussian blobs plus uniform noise, float32 (n, 3), rows shuffled"""
    rng = np.random.default_rng(seed)
    n_noise = int(n * noise)
    centres = np.concatenate([rng.uniform(lo, hi, (n_blobs, 2)), rng.uniform(-1, 2, (n_blobs, 1))], 1)
    which = rng.integers(0, n_blobs, n - n_noise)
    pts = np.concatenate([centres[which] + rng.normal(0, sigma, (n - n_noise, 3)),
                          np.concatenate([rng.uniform(lo, hi, (n_noise, 2)), rng.uniform(-1, 2, (n_noise, 1))], 1)])
    return pts[rng.permutation(n)].astype(F)


def isolated_pairs(seed, n, eps=0.5, origin=-50.0, per_row=48):
    """n rows: pairs eps/2 apart on sites 4 eps apart (z layers 4 eps apart), a few singletons (one when n is odd, plus 2 * min(3,
    n // 16)), in a seeded permutation -- about n / 2 clusters whose lowest indices are spread over all rows"""
    rng = np.random.default_rng(seed)
    n_single = n % 2 + 2 * min(3, n // 16)
    n_pairs = (n - n_single) // 2
    site = np.arange(n_pairs + n_single)
    base = np.stack([origin + 4 * eps * (site % per_row), origin + 4 * eps * ((site // per_row) % per_row),
                     4 * eps * (site // (per_row * per_row))], 1)
    second = base[:n_pairs] + np.where((np.arange(n_pairs) % 2)[:, None] == 1, [eps / 2, 0, 0], [0, eps / 2, 0])
    pts = np.concatenate([base, second])
    return pts[rng.permutation(len(pts))].astype(F)


def hazard_cloud(eps, origin=-52.0, min_pts=2):
    """EVERY pair of ``cell_hazard_pairs`` placed along x and along y, each far from the others (sites 3 eps apart in the other
    axis, 16 to a z layer, layers 3 eps apart).  min_pts = 2: every pair is one cluster, 4 rows per generated pair.  min_pts = 3:
    for every pair two triples p, q, r (6 rows) with q = (b1, a2) the only core point, p = (a1, a2) across an x boundary and
    r = (b1, b2) across a y boundary, (a1, b1) the pair and (a2, b2) the pair at the mirrored place of the list: p and r are border
    points of q's cluster; then the same with x and y exchanged.  -> float32 (n, 3), rows shuffled by a seed"""
    pairs = cell_hazard_pairs(eps, origin)
    k = len(pairs)
    i = np.arange(k)
    out = []
    if min_pts == 2:
        other = origin + 1.0 + 3 * eps * (i % 16)
        zz = 3 * eps * (i // 16)
        for axis in (0, 1):
            for col in (0, 1):
                pt = np.zeros((k, 3))
                pt[:, axis], pt[:, 1 - axis], pt[:, 2] = pairs[:, col], other, zz + (3 * eps * (k // 16 + 2) if axis else 0)
                out.append(pt)
    else:
        a1, b1 = pairs[:, 0], pairs[:, 1]
        a2, b2 = pairs[::-1, 0], pairs[::-1, 1]                 # another boundary for the y side
        zz = 3 * eps * i                                        # triples may share boundaries: one z layer each
        for xs, ys in ((a1, a2), (b1, a2), (b1, b2)):
            out.append(np.stack([xs, ys, zz], 1))
        for xs, ys in ((a2, a1), (a2, b1), (b2, b1)):           # mirrored: the lone neighbour in y first
            out.append(np.stack([xs, ys, zz + 3 * eps * (k + 2)], 1))
    pts = np.concatenate(out).astype(F)
    return pts[np.random.default_rng(k).permutation(len(pts))]


def tie_cloud(origin=-52.0):
    """eps = 0.625, every coordinate a multiple of 1/8: products and sums are exact, contraction cannot matter.  Offsets (3,4,0)/8,
    (0,3,4)/8 and (5,0,0)/8 are neighbours (d2 = eps2 exactly), (5,1,0)/8 is not; each offset from base points on a cell boundary
    of the 0.625 grid from ``origin`` (a multiple of 1/8), just below one and inside a cell, and in both directions.  Pairs 5 m apart."""
    offs = [(3, 4, 0), (0, 3, 4), (5, 0, 0), (5, 1, 0)]
    bx, by = origin + 0.625 * 8, origin + 0.625 * 16          # a corner of the grid's cells; sites 5 m = 8 cells apart keep that alignment
    bases = [(bx, by), (bx - 0.125, by - 0.125), (bx + 0.25, by + 0.25), (bx, by - 0.25)]
    pts = []
    site = 0
    for o in offs:
        for bx, by in bases:
            for sign in (1, -1):
                b = np.array([bx + 5.0 * (site % 12), by + 5.0 * (site // 12), 0.25])
                pts += [b, b + sign * np.array(o) / 8.0]
                site += 1
    pts = np.asarray(pts)
    assert np.all(pts * 8 == np.round(pts * 8))
    return pts.astype(F)


def hand_built():
    """[(name, points float32 (n, >= 3), eps, min_pts, skip or None, expected labels or None)]: the hand-built inputs of the
    conformance suite.  ``expected`` is given where the labels were worked out by hand; both references must give it."""
    out = []
    A = lambda *rows: np.asarray(rows, F)
    line = lambda xs, y=0.0, z=0.0: [(x, y, z) for x in xs]
    # exact ties
    t = tie_cloud()
    want = np.zeros(len(t), np.int32)
    want[:2 * 24] = np.repeat(np.arange(1, 25), 2)              # the first three offsets: 24 neighbour pairs; the fourth: noise
    out.append(("exact ties, eps 0.625", t, 0.625, 2, None, want))
    # a neighbourhood count equal to min_pts, and one short of it
    clump = A(*line([0.0, 0.1, 0.2, 0.3, 0.4]), (30.0, 30.0, 0.0))
    out.append(("count == min_pts", clump, 0.5, 5, None, np.array([1, 1, 1, 1, 1, 0], np.int32)))
    out.append(("count == min_pts - 1", clump, 0.5, 6, None, np.zeros(6, np.int32)))
    # only the point at 0.6 reaches min_pts = 5: it is the one core point (row 0), the others are its border; min_pts = 6: no core point
    five = A(*line([0.6, 0.0, 0.3, 0.9, 1.2]))
    out.append(("one core point, four border points", five, 0.65, 5, None, np.ones(5, np.int32)))
    out.append(("no core point", five, 0.65, 6, None, np.zeros(5, np.int32)))
    # duplicates
    same = np.tile(A((1.25, -3.5, 0.75)), (300, 1))
    out.append(("300 identical points, min_pts 300", same, 0.5, 300, None, np.ones(300, np.int32)))
    out.append(("300 identical points, min_pts 301", same, 0.5, 301, None, np.zeros(300, np.int32)))
    # min_pts = 1: every finite participating point is a cluster; inf, NaN and skipped rows are not
    inf, nan = np.inf, np.nan
    p1 = A((0, 0, 0), (inf, 0, 0), (10, 10, 0), (0, -inf, 1), (10.2, 10, 0), (3, 3, nan), (-20, 5, 1), (0, 0, inf), (-20, 5, 1), (7, 7, 7), (-inf, inf, 0))
    sk = np.zeros(len(p1), np.uint8)
    sk[9] = 1
    out.append(("min_pts 1 with inf, NaN and skipped rows", p1, 0.5, 1, sk, np.array([1, 0, 2, 0, 2, 0, 3, 0, 3, 0, 0], np.int32)))
    # border rule, min_pts = 4: clusters A (x -0.3 .. 0) and B (x 0.9 .. 1.2), a border point at 0.45 within eps of one core of each
    ax, bx = [-0.3, -0.2, -0.1, 0.0], [0.9, 1.0, 1.1, 1.2]
    # rows: 0 = A's far core (A's root), 1 = B's far core (B's root), 2 = B's core next to the border point, 3 = the border point,
    # 4.. = the rest, 7 = A's core next to the border point: the border point's lower-index (2) core neighbour is B's, A's root wins
    rows = [(ax[0], 0, 0), (bx[3], 0, 0), (bx[0], 0, 0), (0.45, 0, 0), (ax[1], 0, 0), (bx[1], 0, 0), (ax[2], 0, 0), (ax[3], 0, 0), (bx[2], 0, 0)]
    out.append(("border point between two clusters takes the lower root", A(*rows), 0.5, 4, None, np.array([1, 2, 2, 1, 1, 2, 1, 1, 2], np.int32)))
    # the same with the border point nearer to B's core (0.5 from A's: an exact tie would not do, 0.49 and 0.41)
    rows2 = list(rows)
    rows2[3] = (0.49, 0, 0)
    out.append(("border point nearer to the other cluster takes the lower root", A(*rows2), 0.5, 4, None, np.array([1, 2, 2, 1, 1, 2, 1, 1, 2], np.int32)))
    # a border point of index 0 in B, whose cores all have higher indices than A's: A is label 1, B label 2
    rows3 = [(1.65, 0, 0)] + line(ax) + line(bx)
    out.append(("border point of index 0 does not number its cluster", A(*rows3), 0.5, 4, None, np.array([2, 1, 1, 1, 1, 2, 2, 2, 2], np.int32)))
    # NaN in z only; +-inf rows beside a cluster; points 1e6 m outside the grid on every side
    c5 = line([0.0, 0.1, 0.2, 0.3, 0.4], 2.0, 1.0)
    out.append(("NaN in z only", A(*c5[:2], (0.2, 2.0, nan), *c5[3:], (0.25, 2.0, 1.0)), 0.5, 5, None, np.array([1, 1, 0, 1, 1, 1], np.int32)))
    out.append(("inf rows beside a cluster", A((inf, 2.0, 1.0), *c5, (0.2, -inf, 1.0), (0.2, 2.0, inf)), 0.5, 5, None,
                np.array([0, 1, 1, 1, 1, 1, 0, 0], np.int32)))
    far = []
    for cx, cy in ((1e6, 0), (-1e6, 0), (0, 1e6), (0, -1e6), (1e6, 1e6), (-1e6, -1e6), (1e6, -1e6), (-1e6, 1e6)):
        far += [(cx, cy, 0.0), (cx + 0.25, cy, 0.0), (cx, cy + 0.25, 0.0)]
    far += [(1e6, 30.0, 0.0), (0.0, 0.0, 0.0)]
    out.append(("points 1e6 m outside the grid on every side", A(*far), 0.5, 3, None, np.concatenate([np.repeat(np.arange(1, 9), 3), [0, 0]]).astype(np.int32)))
    return out
