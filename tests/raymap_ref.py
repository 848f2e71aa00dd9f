"""The checker of the free-space labeller: a numpy restatement of rules A-G of "free-space ray map, v1" (the module docstring of
``himo_amd/raymap.py`` is the text).  Rule A is float32 operation by operation; the walk of rule C exists twice -- ``walk_one`` in
Python integers, one ray at a time, and ``carve`` in int64 arrays over all rays at once (tests/test_raymap_cpu.py holds one against
the other).  Nothing under ``himo_amd/`` imports it; it imports nothing from there either (parameters come as keywords)."""
import numpy as np

DEFAULTS = dict(x0=-51.2, y0=-51.2, z0=-3.0, voxel=0.2, nx=512, ny=512, nz=30, guard=2, min_votes=2)
LIMIT = np.float32(4194304.0)                                   # 2^22 sub-voxel units
EPS, MIN_PTS, RANGE_NET = 0.5, 8, 51.2                          # rule F: the values of himo_amd/seflow/ssl_label.py, restated
MIN_DYNAMIC, SHARE = 3, (1, 4)

f32 = np.float32


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def scale_of(voxel):
    """(float)(256.0 / voxel), the division in double on the float32 voxel size"""
    return f32(256.0 / float(f32(voxel)))


def new_map(**kw):
    p = params(**kw)
    return np.zeros((int(p["nz"]), int(p["ny"]), int(p["nx"])), dtype=np.uint32)


def quantise(xyz, **kw):
    """rule A: (u int64 [N, 3] in 1/256 voxel -- 0 where unusable --, usable bool [N])"""
    p = params(**kw)
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    m = np.array([p["x0"], p["y0"], p["z0"]], dtype=np.float32)
    with np.errstate(all="ignore"):
        diff = (xyz - m).astype(np.float32)
        f = (diff * scale_of(p["voxel"])).astype(np.float32)
        usable = (np.isfinite(f) & (np.abs(f) < LIMIT)).all(axis=1)
        u = np.floor(np.where(usable[:, None], f, f32(0))).astype(np.int64)
    return u, usable


def in_grid(v, **kw):
    p = params(**kw)
    n = np.array([p["nx"], p["ny"], p["nz"]], dtype=np.int64)
    return ((v >= 0) & (v < n)).all(axis=-1)


def walk_one(A, B):
    """rules B and C for one ray in Python integers: (visited voxels in order, end voxel).  ``A``, ``B``: quantised origin and end."""
    A, B = [int(a) for a in A], [int(b) for b in B]
    v, e = [a >> 8 for a in A], [b >> 8 for b in B]
    d = [b - a for a, b in zip(A, B)]
    step = [(x > 0) - (x < 0) for x in d]
    den = [abs(x) for x in d]
    r = [abs(ek - vk) for ek, vk in zip(e, v)]
    num = [abs((v[k] + (1 if step[k] > 0 else 0)) * 256 - A[k]) for k in range(3)]
    seen = []
    while any(x > 0 for x in r):
        seen.append(tuple(v))
        a = None
        for k in range(3):
            if r[k] > 0 and (a is None or num[k] * den[a] < num[a] * den[k]):
                a = k
        v[a] += step[a]
        num[a] += 256
        r[a] -= 1
    assert v == e
    return seen, tuple(e)


def marks_one(A, B, **kw):
    """rule D for one ray: (FREE voxels, the HIT voxel or None), each in grid"""
    p = params(**kw)
    seen, e = walk_one(A, B)
    inside = lambda v: bool(in_grid(np.array(v, dtype=np.int64), **kw))
    free = [v for v in seen if inside(v) and max(abs(v[k] - e[k]) for k in range(3)) > int(p["guard"])]
    return free, (e if inside(e) else None)


def carve(grid, pts, slot, origins, **kw):
    """rules B-D over all rays at once: OR the marks into ``grid`` (uint32 [nz, ny, nx]) in place.  ``slot``: uint8 [N] (255 = the ray
    takes no part; 16..254 is a refused call: ValueError, nothing written), ``origins``: float32 [16, 3].  Walks every ray to its end
    (no early stop).  Returns the number of voxel visits."""
    p = params(**kw)
    guard = int(p["guard"])
    slot = np.asarray(slot, dtype=np.uint8).reshape(-1)
    if ((slot > 15) & (slot != 255)).any():
        raise ValueError("a slot byte in 16..254")
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    origins = np.asarray(origins, dtype=np.float32).reshape(16, 3)
    B, ok_b = quantise(pts, **kw)
    A16, ok_o = quantise(origins, **kw)
    s = np.where(slot == 255, 0, slot).astype(np.int64)
    take = np.nonzero(ok_b & ok_o[s] & (slot != 255))[0]
    A, B, s = A16[s[take]], B[take], s[take]
    v, e = A >> 8, B >> 8
    d = B - A
    step, den, r = np.sign(d), np.abs(d), np.abs(e - v)
    num = np.abs((v + (step > 0)) * 256 - A)
    flat = grid.reshape(-1)
    nx, ny = int(p["nx"]), int(p["ny"])
    index = lambda vox: (vox[:, 2] * ny + vox[:, 1]) * nx + vox[:, 0]
    free_bit, hit_bit = (np.uint32(1) << s.astype(np.uint32)), (np.uint32(1) << (s + 16).astype(np.uint32))
    rows = np.nonzero((r > 0).any(axis=1))[0]
    visits = 0
    while len(rows):
        vv, rr = v[rows], r[rows]
        visits += len(rows)
        mark = in_grid(vv, **kw) & (rr.max(axis=1) > guard)
        np.bitwise_or.at(flat, index(vv[mark]), free_bit[rows[mark]])
        nn, dd = num[rows], den[rows]
        a = np.full(len(rows), -1, dtype=np.int64)
        for k in range(3):
            cur = np.maximum(a, 0)
            na, da = nn[np.arange(len(rows)), cur], dd[np.arange(len(rows)), cur]
            better = (rr[:, k] > 0) & ((a < 0) | (nn[:, k] * da < na * dd[:, k]))
            a = np.where(better, k, a)
        v[rows, a] += step[rows, a]
        num[rows, a] += 256
        r[rows, a] -= 1
        rows = rows[(r[rows] > 0).any(axis=1)]
    assert np.array_equal(v, e)
    hit = in_grid(e, **kw)
    np.bitwise_or.at(flat, index(e[hit]), hit_bit[hit])
    return visits


def votes(w):
    """rule E on map words: (fv, hv)"""
    w = np.asarray(w, dtype=np.uint32)
    pop = lambda x: np.array([bin(int(t)).count("1") for t in x.reshape(-1)], dtype=np.uint8).reshape(x.shape)
    return pop((w & np.uint32(0xFFFF)) & ~(w >> np.uint32(16))), pop(w >> np.uint32(16))


_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.uint8)


def query(grid, pts, skip=None, **kw):
    """rule E: (dynamic bool [N], fv uint8 [N], hv uint8 [N])"""
    p = params(**kw)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    u, usable = quantise(pts, **kw)
    v = u >> 8
    live = usable & in_grid(v, **kw)
    if skip is not None:
        live &= np.asarray(skip).reshape(-1) == 0
    w = np.zeros(len(pts), dtype=np.uint32)
    w[live] = grid[v[live, 2], v[live, 1], v[live, 0]]
    fv = _POP16[(w & np.uint32(0xFFFF)) & ~(w >> np.uint32(16)) & np.uint32(0xFFFF)]
    hv = _POP16[w >> np.uint32(16)]
    fv, hv = np.where(live, fv, 0).astype(np.uint8), np.where(live, hv, 0).astype(np.uint8)
    return live & (fv >= int(p["min_votes"])) & (fv > hv), fv, hv


def cluster_labels(ids, dynamic, min_dynamic=MIN_DYNAMIC, share=SHARE):
    """rule F on DBSCAN ids (0 = noise / no part): int32 labels, the dynamic clusters renumbered 1..K in ascending id order"""
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    dynamic = np.asarray(dynamic).astype(bool).reshape(-1)
    out = np.zeros(len(ids), dtype=np.int32)
    nxt = 1
    for c in sorted(set(ids[ids > 0].tolist())):
        member = ids == c
        n, k = int(member.sum()), int((member & dynamic).sum())
        if k >= min_dynamic and share[1] * k >= share[0] * n:
            out[member] = nxt
            nxt += 1
    return out


def dbscan(xyz, eps=EPS, min_pts=MIN_PTS, skip=None):
    """plain DBSCAN (a point's neighbourhood includes itself) for the CPU tests of rule F: clusters numbered 1.. by their lowest point
    index, a border point joins the neighbouring cluster of lowest such index; 0 = noise or skipped.  O(n^2): small inputs only."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    use = np.ones(n, bool) if skip is None else ~np.asarray(skip).astype(bool)
    idx = np.nonzero(use)[0]
    q = xyz[idx]
    near = np.zeros((len(idx), len(idx)), dtype=bool)
    for lo in range(0, len(idx), 256):                          # (row blocks: the differences of all pairs at once would not fit)
        near[lo:lo + 256] = ((q[lo:lo + 256, None, :] - q[None, :, :]) ** 2).sum(-1) <= eps * eps
    core = near.sum(1) >= min_pts
    lab = np.zeros(len(idx), dtype=np.int64)
    c = 0
    for i in range(len(idx)):
        if core[i] and lab[i] == 0:
            c += 1
            lab[i] = c
            stack = [i]
            while stack:
                j = stack.pop()
                for k in np.nonzero(near[j] & core & (lab == 0))[0]:
                    lab[k] = c
                    stack.append(k)
    for i in np.nonzero(~core)[0]:
        cand = lab[near[i] & core]
        if len(cand):
            lab[i] = cand.min()
    out = np.zeros(n, dtype=np.int64)
    out[idx] = lab
    return out


def cluster_skip(xyz, ground):
    """rule F: the target points that take no part in DBSCAN -- ground, non-finite, or outside RANGE_NET in x or y"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.asarray(ground).astype(bool) | ~np.isfinite(xyz).all(axis=1) | ~(np.abs(xyz[:, :2]).max(axis=1) <= f32(RANGE_NET))


def neighbours(t, n_sweeps, window=5):
    """rule G: the neighbour sweeps of target ``t``, in slot order"""
    return [k for k in range(max(0, t - window), min(n_sweeps, t + window + 1)) if k != t]


def relative_pose(pose_t, pose_k):
    """rule G: T = inv(pose_t) @ pose_k in float64, rounded to float32"""
    return (np.linalg.inv(np.asarray(pose_t, np.float64)) @ np.asarray(pose_k, np.float64)).astype(np.float32)


def move(xyz, T):
    """a float32 rigid transform for the CPU tests (the GPU tests feed the restatement the device's own moved points)"""
    T = np.asarray(T, dtype=np.float32)
    xyz = np.asarray(xyz, dtype=np.float32)[:, :3]
    return ((xyz[:, 0:1] * T[:3, 0] + xyz[:, 1:2] * T[:3, 1]).astype(np.float32) + xyz[:, 2:3] * T[:3, 2] + T[:3, 3]).astype(np.float32)


def dynamic_flags(target_xyz, target_ground, moved, origins16, **kw):
    """rule G given the neighbours ALREADY moved into the target's frame (``moved``: list of float32 [n_k, 3] in slot order) and
    their origins: (dynamic, fv, hv) of the target's points"""
    grid = new_map(**kw)
    if moved:
        pts = np.concatenate([np.asarray(m, np.float32).reshape(-1, 3) for m in moved])
        slot = np.concatenate([np.full(len(m), k, np.uint8) for k, m in enumerate(moved)])
        carve(grid, pts, slot, origins16, **kw)
    return query(grid, target_xyz, np.asarray(target_ground).astype(np.uint8), **kw)
