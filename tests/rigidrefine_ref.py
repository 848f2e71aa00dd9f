"""The checker of the cluster-rigid refinement: a numpy restatement of "cluster-rigid refinement, v1" (the module docstring of
``himo_amd/rigid_refine.py`` is the text).  The votes are integers, the sums are float64 in ROW order, the labels are an ARGUMENT
(the clustering is checked elsewhere).  Nothing under ``himo_amd/`` imports it; it imports nothing from there either.

Beside the result it returns ``margins``: how far the run's float decisions were from their thresholds, so that a test can show that
a case tests the kernel and not a coin toss --
    "e2"      the smallest |e2 - tol^2| / tol^2 over every row of every pass p >= 1 (pass 0's inliers only seed the first refit),
    "static"  the smallest |max |m - a|^2 - static_disp^2| / static_disp^2 over the accepted rounds,
    "ratio"   the smallest |n / size - min_ratio| over the rounds that reached the acceptance test,
    "count"   over every pass that compared n with min_inliers, the fewest rows whose inlier test would have to flip for the comparison
              to come out the other way (n = min_inliers gives 1, n = min_inliers - 1 gives 1): an integer, read beside "e2".
A margin that was never taken is ``inf``.
"""
import numpy as np

DEFAULTS = dict(bin=0.25, half=16, tol=0.25, iters=5, min_inliers=8, min_ratio=0.25, static_disp=0.05, models=2)
ACCEPTED, FAILED, REJECTED, STATIC, NOT_RUN = 0, 1, 2, 3, 4
RANGE_NET = 51.2

f32, f64 = np.float32, np.float64


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown parameters {sorted(unknown)}")
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- step 0 -------------------------------------------------------------------------------------------------------------------------
def moved(pc0, pose0, pose1):
    """pc0 in pc1's frame: inv(pose1) @ pose0 rounded to float32, then ((x T0 + y T1) + z T2) + T3 in float32"""
    T = (np.linalg.inv(np.asarray(pose1, f64)) @ np.asarray(pose0, f64)).astype(f32)
    p = np.asarray(pc0, f32)[:, :3]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((x * T[r, 0] + y * T[r, 1]) + z * T[r, 2]) + T[r, 3] for r in range(3)], axis=1).astype(f32)


def participates(a, flow, ground):
    with np.errstate(all="ignore"):
        return ~np.asarray(ground, bool) & ~(np.abs(a[:, :2]).max(axis=1, initial=0.0) > f32(RANGE_NET)) & np.isfinite(flow).all(axis=1)


# ---- step 2a ------------------------------------------------------------------------------------------------------------------------
def vote(a, q, **kw):
    """(kx, ky) of the peak over the rows given, and the counters int64 [W, W] indexed [ky + half, kx + half]"""
    p = params(**kw)
    half = int(p["half"])
    W = 2 * half + 1
    counts = np.zeros((W, W), np.int64)
    with np.errstate(all="ignore"):
        r = (np.asarray(q, f32) - np.asarray(a, f32)).astype(f32)
        kx = np.rint((r[:, 0] / f32(p["bin"])).astype(f32))
        ky = np.rint((r[:, 1] / f32(p["bin"])).astype(f32))
        ok = (np.abs(kx) <= half) & (np.abs(ky) <= half)
    np.add.at(counts, (ky[ok].astype(np.int64) + half, kx[ok].astype(np.int64) + half), 1)
    ky_g, kx_g = np.meshgrid(np.arange(-half, half + 1), np.arange(-half, half + 1), indexing="ij")
    order = np.lexsort((kx_g.ravel(), ky_g.ravel(), (kx_g ** 2 + ky_g ** 2).ravel(), -counts.ravel()))
    best = order[0]
    return int(kx_g.ravel()[best]), int(ky_g.ravel()[best]), counts


# ---- step 2b ------------------------------------------------------------------------------------------------------------------------
def model_points(a, T):
    """m = ((c x - s y) + tx, (s x + c y) + ty, z + tz) in float64 from the float32 rows"""
    c, s, tx, ty, tz = (f64(v) for v in T)
    x, y, z = (np.asarray(a, f32)[:, k].astype(f64) for k in range(3))
    return np.stack([(c * x - s * y) + tx, (s * x + c * y) + ty, z + tz], axis=1)


def errors(a, q, T, with_z=True):
    m, q = model_points(a, T), np.asarray(q, f32).astype(f64)
    e2 = (q[:, 0] - m[:, 0]) ** 2 + (q[:, 1] - m[:, 1]) ** 2
    return e2 + (q[:, 2] - m[:, 2]) ** 2 if with_z else e2


def _rowsum(v):
    s = f64(0.0)
    for x in v:
        s = s + x
    return s


def refit(a, q):
    """the closed form over the rows given (float64, row order)"""
    a, q = np.asarray(a, f32).astype(f64), np.asarray(q, f32).astype(f64)
    n = f64(len(a))
    ab = np.array([_rowsum(a[:, k]) / n for k in range(3)])
    qb = np.array([_rowsum(q[:, k]) / n for k in range(3)])
    ax, ay, qx, qy = a[:, 0] - ab[0], a[:, 1] - ab[1], q[:, 0] - qb[0], q[:, 1] - qb[1]
    A, B = _rowsum(ax * qx + ay * qy), _rowsum(ax * qy - ay * qx)
    h = np.sqrt(A * A + B * B)
    c, s = (f64(1.0), f64(0.0)) if h == 0.0 else (A / h, B / h)
    return np.array([c, s, qb[0] - (c * ab[0] - s * ab[1]), qb[1] - (s * ab[0] + c * ab[1]), qb[2] - ab[2]])


def _closer(margins, key, value):
    margins[key] = min(margins[key], float(value))


def fit_round(a, q, size, margins, **kw):
    """one round over the unclaimed rows given: (state, n of the last pass, kx, ky, transform, claim mask)"""
    p = params(**kw)
    tol2 = f64(f32(p["tol"])) * f64(f32(p["tol"]))
    iters, min_in = int(p["iters"]), int(p["min_inliers"])
    kx, ky, _ = vote(a, q, **kw)
    T = np.array([1.0, 0.0, f64(kx) * f64(f32(p["bin"])), f64(ky) * f64(f32(p["bin"])), 0.0])
    none = np.zeros(len(a), bool)
    n = 0
    for it in range(iters + 1):
        e2 = errors(a, q, T, with_z=it > 0)
        if it > 0 and len(e2):
            _closer(margins, "e2", np.abs(e2 - tol2).min() / tol2)
        inl = e2 <= tol2
        n = int(inl.sum())
        _closer(margins, "count", abs(n - (min_in - 0.5)) + 0.5)
        if it == iters:
            break
        if n < min_in:
            return FAILED, n, kx, ky, T, none
        T = refit(a[inl], q[inl])
    if n < min_in:
        return REJECTED, n, kx, ky, T, none
    _closer(margins, "ratio", abs(f64(n) / f64(size) - f64(f32(p["min_ratio"]))))
    if not f64(n) / f64(size) >= f64(f32(p["min_ratio"])):
        return REJECTED, n, kx, ky, T, none
    sd2 = f64(f32(p["static_disp"])) * f64(f32(p["static_disp"]))
    d = model_points(a[inl], T) - np.asarray(a[inl], f32).astype(f64)
    far = ((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2).max()
    _closer(margins, "static", abs(far - sd2) / sd2)
    if far < sd2:
        return STATIC, n, kx, ky, np.array([1.0, 0.0, 0.0, 0.0, 0.0]), inl
    return ACCEPTED, n, kx, ky, T, inl


def apply_flow(a, base, T):
    """float32(R a + t) - pc0, subtracted in float32"""
    return (model_points(a, T).astype(f32) - np.asarray(base, f32)[:, :3]).astype(f32)


def refine(pc0, flow, gm0, pose0, pose1, labels, a=None, **kw):
    """the whole rule given the labels (int (N,), 0 = no cluster; rows that take no part must carry 0).  ``a``: the moved points when
    they come from somewhere else (the device's ``himo_rigid_transform``: step 0 names that call as the definition).
    -> dict(flow, status int32 [C, models, 4], transforms float64 [C, models, 5], claim int8 [N], ego_flow, a, margins)"""
    p = params(**kw)
    models = int(p["models"])
    pc0, flow = np.asarray(pc0, f32), np.asarray(flow, f32)
    n = len(pc0)
    a = moved(pc0, pose0, pose1) if a is None else np.asarray(a, f32)
    labels = np.asarray(labels, np.int64)
    part = participates(a, flow, gm0) if n else np.zeros(0, bool)
    assert not (labels[~part] > 0).any(), "a row that takes no part carries a label"
    C = int(labels.max(initial=0))
    with np.errstate(all="ignore"):
        q = (pc0[:, :3] + flow).astype(f32)
    out = flow.copy()
    claim = np.zeros(n, np.int8)
    status = np.zeros((C, models, 4), np.int32)
    status[:, :, 0] = NOT_RUN
    T_all = np.zeros((C, models, 5), f64)
    T_all[:, :, 0] = 1.0
    margins = dict(e2=np.inf, static=np.inf, ratio=np.inf, count=np.inf)
    for k in range(C):
        rows = np.flatnonzero(labels == k + 1)
        free = np.ones(len(rows), bool)
        for j in range(models):
            r = rows[free]
            state, cnt, kx, ky, T, got = fit_round(a[r], q[r], len(rows), margins, **kw)
            status[k, j] = (state, cnt, kx, ky)
            T_all[k, j] = T
            if state in (FAILED, REJECTED):
                break
            out[r[got]] = apply_flow(a[r[got]], pc0[r[got]], T)
            claim[r[got]] = j + 1
            free[np.flatnonzero(free)[got]] = False
    ego = (a - pc0[:, :3]).astype(f32) if n else np.zeros((0, 3), f32)
    return dict(flow=out, status=status, transforms=T_all, claim=claim, ego_flow=ego, a=a, margins=margins)


def kabsch_2d(a, q):
    """an independent 2-D Kabsch through numpy.linalg.svd: (c, s, tx, ty, tz) of the least-squares yaw + translation a -> q"""
    a, q = np.asarray(a, f64), np.asarray(q, f64)
    ab, qb = a.mean(0), q.mean(0)
    H = (a[:, :2] - ab[:2]).T @ (q[:, :2] - qb[:2])
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    t = qb[:2] - R @ ab[:2]
    return np.array([R[0, 0], R[1, 0], t[0], t[1], qb[2] - ab[2]])


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def yaw_pose(deg, t):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    P = np.eye(4)
    P[:2, :2] = [[c, -s], [s, c]]
    P[:3, 3] = t
    return P


def rigid_motion(pts, yaw, t, pivot):
    """the points turned by ``yaw`` (rad) about the vertical through ``pivot`` and moved by ``t`` (float64)"""
    c, s = np.cos(yaw), np.sin(yaw)
    d = np.asarray(pts, f64) - pivot
    return np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1], d[:, 2]], axis=1) + pivot + np.asarray(t, f64)


def box(rng, n, centre, dims=(8.0, 2.5, 2.5)):
    return rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(dims) + np.asarray(centre, f64)


def flow_from(pc0, target_in_pc1, rng, sigma):
    """the stored-flow contract: where the point goes in pc1's frame minus where it is in pc0's, plus noise"""
    return (np.asarray(target_in_pc1, f64) - np.asarray(pc0, f64)[:, :3] + rng.normal(0.0, sigma, (len(pc0), 3))).astype(f32)


EGO = yaw_pose(2.0, (3.0, 0.4, 0.0))          # pose1 of the scenes below (pose0 = identity): yaw 2 degrees, 3 m, so that a != pc0


def blob_dims(n, density=80.0):
    """a 2 : 1 : 1 box that holds n uniform points at ``density`` per m^3: DBSCAN(0.5, 8) keeps it one cluster"""
    u = (n / density / 2.0) ** (1.0 / 3.0)
    return (2.0 * u, u, u)


def build_scene(parts, seed, sigma=0.03, pose1=EGO, pitch=3):
    """A sweep from ``parts``: dicts with ``n``, ``centre`` (pc0's frame), optionally ``dims``, ``yaw`` (rad), ``t``, ``pivot`` (offset of
    the turning point from the part's centre), ``cluster`` (parts that share a value are one cluster; None = the part's own),
    ``ground`` (bool), ``sigma``.  Clusters are numbered in the order their first part appears, as DBSCAN numbers them by their lowest
    row.  -> dict(pc0, flow, gm0, pose0, pose1, labels (as constructed), true_flow, part (index of every row's part))"""
    rng = np.random.default_rng(seed)
    pcs, grounds, part_of, ids, keys = [], [], [], [], {}
    for k, p in enumerate(parts):
        n = int(p["n"])
        pcs.append(box(rng, n, p["centre"], p.get("dims", blob_dims(max(n, 8)))))
        grounds.append(np.full(n, bool(p.get("ground", False))))
        part_of.append(np.full(n, k))
        key = p.get("cluster", ("own", k))
        ids.append(np.full(n, keys.setdefault(key, len(keys) + 1)))
    pc0 = np.concatenate(pcs).astype(f32) if pcs else np.zeros((0, 3), f32)
    gm0, part_of, labels = np.concatenate(grounds), np.concatenate(part_of), np.concatenate(ids).astype(np.int32)
    pose0 = np.eye(4)
    a = moved(pc0, pose0, pose1)
    target = a.astype(f64).copy()
    noise = np.zeros((len(pc0), 3))
    for k, p in enumerate(parts):
        rows = part_of == k
        centre = a[rows].astype(f64).mean(0) if rows.any() else np.zeros(3)
        target[rows] = rigid_motion(a[rows], p.get("yaw", 0.0), p.get("t", (0.0, 0.0, 0.0)), centre + np.asarray(p.get("pivot", (0.0, 0.0, 0.0))))
        noise[rows] = rng.normal(0.0, p.get("sigma", sigma), (int(rows.sum()), 3))
    true_flow = (target - pc0.astype(f64)).astype(f32)
    flow = (target - pc0.astype(f64) + noise).astype(f32)
    labels = np.where(participates(a, flow, gm0), labels, 0).astype(np.int32)
    live = np.unique(labels[labels > 0])                        # a cluster all of whose rows dropped out leaves no gap
    remap = np.zeros(int(labels.max(initial=0)) + 1, np.int32)
    remap[live] = np.arange(1, len(live) + 1)
    labels = remap[labels]
    if pitch == 4:
        pc0 = np.concatenate([pc0, rng.uniform(0.0, 1.0, (len(pc0), 1)).astype(f32)], axis=1)
    return dict(pc0=pc0, flow=flow, gm0=gm0, pose0=pose0, pose1=np.asarray(pose1, f64), labels=labels, true_flow=true_flow, part=part_of)


def spoil(scene, rows, values):
    """rows of a scene whose flow becomes non-finite: they take no part and lose their label (their cluster keeps its number)"""
    scene["flow"][rows] = values
    scene["labels"][rows] = 0
    return scene


def vehicle_scene(n_static, seed=5, sigma=0.05):
    """the scene the rule was tried on: one 300-point box of 8 x 2.5 x 2.5 m moving (1.5, 0.2, 0) with yaw 0.03 about a point 4 m
    behind its centre, alone or in ONE cluster with ``n_static`` static points 2.5 m beside it"""
    parts = [dict(n=300, centre=(12.0, 3.0, 0.5), dims=(8.0, 2.5, 2.5), yaw=0.03, t=(1.5, 0.2, 0.0), pivot=(-4.0, 0.0, 0.0), cluster="c")]
    if n_static:
        parts.append(dict(n=n_static, centre=(12.0, 5.5, 0.5), dims=(8.0, 1.0, 2.5), cluster="c"))
    return build_scene(parts, seed, sigma)


def three_part_scene(seed=11, sigma=0.03, n=200):
    """one cluster of three rigid parts, 40 / 35 / 25 % of its rows, each with its own motion"""
    shares, motions = (0.40, 0.35, 0.25), (((1.5, 0.0, 0.0), 0.02), ((-1.0, 0.5, 0.0), -0.03), ((0.0, -1.5, 0.0), 0.0))
    parts = [dict(n=int(round(n * sh)), centre=(-10.0, -6.0 + 1.2 * k, 0.4), dims=(3.0, 1.0, 1.0), t=t, yaw=yaw, cluster="three")
             for k, (sh, (t, yaw)) in enumerate(zip(shares, motions))]
    return build_scene(parts, seed, sigma)


# ---- the cases of tests/test_rigid_refine_gpu.py (tests/test_rigid_refine_cpu.py shows that their decisions have margins) ----------------
SIZES = (63, 64, 65, 255, 256, 257, 1025)      # around the wave's 64 lanes, a 256-thread block and the wave / block split at 1024 rows
N_SMALL = 300                                   # 9-point clusters: more clusters than one round of blocks on 256 CUs


def sizes_scene(seed=21):
    rng = np.random.default_rng(1000 + seed)
    spots = [(8, -20), (16, -20), (24, -20), (8, -10), (20, -10), (8, 10), (25, 10)]
    parts = [dict(n=n, centre=(x, y, 0.5), t=(*rng.uniform(-3.4, 3.4, 2), rng.uniform(-0.1, 0.1)), yaw=rng.uniform(-0.05, 0.05))
             for n, (x, y) in zip(SIZES, spots)]
    for k in range(N_SMALL):
        parts.append(dict(n=9, centre=(-44.0 + 2.0 * (k % 20), -14.0 + 2.0 * (k // 20), 0.3), dims=(0.3, 0.3, 0.3),
                          t=(*rng.uniform(-3.4, 3.4, 2), rng.uniform(-0.05, 0.05)), sigma=0.01))
    return build_scene(parts, seed, sigma=0.03, pitch=4)


def merged_scene(seed=31):
    parts = []
    for c, (moving, static, x) in enumerate(((180, 120, 10.0), (120, 180, -15.0))):
        parts.append(dict(n=moving, centre=(x, 8.0, 0.5), dims=(3.0, 1.2, 1.0), yaw=0.06, t=(1.2, -0.6, 0.0), cluster=c))
        parts.append(dict(n=static, centre=(x, 9.1, 0.5), dims=(3.0, 0.8, 1.0), cluster=c))
    shares, motions = (80, 70, 50), (((1.5, 0.0, 0.0), 0.02), ((-1.0, 0.5, 0.0), -0.03), ((0.0, -1.5, 0.0), 0.0))
    for k, (n, (t, yaw)) in enumerate(zip(shares, motions)):
        parts.append(dict(n=n, centre=(-10.0, -6.0 + 0.9 * k, 0.4), dims=(1.6, 0.7, 0.7), t=t, yaw=yaw, cluster="three"))
    return build_scene(parts, seed, sigma=0.03)


def static_scene(seed=41):
    return build_scene([dict(n=120, centre=(6.0, -4.0, 0.2))], seed, sigma=0.03)


def passthrough_scene(seed=51):
    parts = [dict(n=150, centre=(10.0, 5.0, 0.5), t=(1.0, 0.5, 0.0), yaw=0.02),             # rows with a non-finite flow inside it
             dict(n=60, centre=(58.0, 0.0, 0.5), t=(1.0, 0.0, 0.0)),                        # beyond 51.2 m
             dict(n=80, centre=(-8.0, 3.0, -1.7), dims=(4.0, 4.0, 0.1), ground=True),       # ground rows
             dict(n=90, centre=(-12.0, -9.0, 0.5), t=(5.0, 0.0, 0.0))]                      # residual outside the +-4 m window
    sc = build_scene(parts, seed, sigma=0.03)
    bad = np.array([[np.nan, 0.1, 0.0], [0.2, np.inf, 0.0], [0.1, 0.0, -np.inf], [np.nan, np.nan, np.nan]], f32)
    return spoil(sc, np.array([3, 40, 77, 149]), bad)


def eight_scene(seed=61):
    return build_scene([dict(n=8, centre=(5.0, 2.0, 0.3), dims=(0.3, 0.3, 0.3), t=(0.5, 0.25, 0.0), sigma=0.01)], seed)


def seven_scene(seed=62):
    return build_scene([dict(n=7, centre=(5.0, 2.0, 0.3), dims=(0.3, 0.3, 0.3), t=(0.5, 0.25, 0.0), sigma=0.01)], seed)


def hdbscan_scene(seed=71):
    parts = [dict(n=150, centre=(9.0, 4.0, 0.5), t=(1.3, 0.2, 0.0), yaw=0.03), dict(n=150, centre=(-7.0, -6.0, 0.5)),
             dict(n=100, centre=(3.0, -12.0, 0.5), t=(-0.8, 0.9, 0.05))]
    return build_scene(parts, seed, sigma=0.03)


# name -> (scene builder, rule parameters, constructor options)
CASES = {
    "eight": (eight_scene, {}, {}),
    "seven": (seven_scene, {}, dict(min_pts=4)),
    "sizes": (sizes_scene, {}, {}),
    "merged": (merged_scene, {}, {}),
    "static": (static_scene, {}, {}),
    "passthrough": (passthrough_scene, {}, {}),
    "hdbscan": (hdbscan_scene, {}, dict(cluster="hdbscan")),
}
