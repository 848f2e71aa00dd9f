"""The free-space labeller without a GPU: the numpy restatement of "free-space ray map, v1" (tests/raymap_ref.py; the rule is the
module docstring of himo_amd/raymap.py) against hand-worked cases, against an independent property check of its walk, and on a
ray-cast toy scene; and the loader's ``<name>_next`` fields, which make labels stored in the scene files trainable."""
import warnings

import numpy as np
import pytest

import raymap_ref as ref

UNIT = dict(x0=0.0, y0=0.0, z0=0.0, voxel=1.0, nx=8, ny=8, nz=4)          # scale 256: a coordinate IS its voxel index
ORIGINS = np.zeros((16, 3), np.float32)


def one_ray(o, p, slot=0, **kw):
    """the map after the single ray o -> p: ({voxel (x, y, z): word}, the restatement's Python-integer marks)"""
    rule = {**UNIT, **kw}
    origins = ORIGINS.copy()
    origins[slot] = o
    grid = ref.new_map(**rule)
    ref.carve(grid, np.array([p], np.float32), np.array([slot], np.uint8), origins, **rule)
    A, ok_a = ref.quantise(np.array([o], np.float32), **rule)
    B, ok_b = ref.quantise(np.array([p], np.float32), **rule)
    assert ok_a[0] and ok_b[0]
    z, y, x = np.nonzero(grid)
    return {(int(a), int(b), int(c)): int(grid[c, b, a]) for a, b, c in zip(x, y, z)}, ref.marks_one(A[0], B[0], **rule)


def test_scale_and_quantisation():
    assert ref.scale_of(0.2) == np.float32(256.0 / float(np.float32(0.2))) and ref.scale_of(1.0) == 256.0
    u, ok = ref.quantise(np.array([[0.5, 1.25, 3.999], [-0.001, 0.0, 7.0]], np.float32), **UNIT)
    assert ok.all() and u.tolist() == [[128, 320, 1023], [-1, 0, 1792]]
    assert (u >> 8).tolist() == [[0, 1, 3], [-1, 0, 7]]                     # the arithmetic shift floors
    # default grid: f = (c - m) * scale, each operation rounded to float32
    c, m = np.float32(8.07), np.float32(-51.2)
    want = int(np.floor(np.float32(np.float32(c - m) * ref.scale_of(0.2))))
    assert ref.quantise(np.array([[8.07, 8.07, 8.07]], np.float32))[0][0, 0] == want


def test_nan_inf_and_the_2_22_limit_are_unusable():
    big = np.float32(16384.0)                                               # * 256 = 2^22
    below = np.nextafter(big, np.float32(0))
    pts = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [big, 1, 1], [1, -big, 1], [below, 1, 1], [1, 1, -below], [3e38, 1, 1]], np.float32)
    _, ok = ref.quantise(pts, **UNIT)
    assert ok.tolist() == [False, False, False, False, False, True, True, False]
    grid = ref.new_map(**UNIT)
    origins = ORIGINS.copy()
    origins[0], origins[1] = (0.5, 0.5, 0.5), (np.nan, 0.5, 0.5)
    # unusable ends, an unusable origin (slot 1), and slot 255: nothing is marked
    ends = np.concatenate([pts[:5], [[5.5, 0.5, 0.5]], [[5.5, 0.5, 0.5]]]).astype(np.float32)
    assert ref.carve(grid, ends, np.array([0, 0, 0, 0, 0, 1, 255], np.uint8), origins, **UNIT) == 0 and not grid.any()
    dyn, fv, hv = ref.query(np.full_like(grid, 0x7), pts, **UNIT)
    assert not dyn.any() and not fv.any() and not hv.any()
    with pytest.raises(ValueError):
        ref.carve(grid, ends[5:6], np.array([16], np.uint8), origins, **UNIT)


@pytest.mark.parametrize("guard, free_x", [(0, [0, 1, 2, 3, 4]), (1, [0, 1, 2, 3]), (2, [0, 1, 2])])
def test_axis_aligned_ray_and_the_guard(guard, free_x):
    words, (free, hit) = one_ray((0.5, 0.5, 0.5), (5.5, 0.5, 0.5), slot=3, guard=guard)
    assert words == {**{(x, 0, 0): 1 << 3 for x in free_x}, (5, 0, 0): 1 << 19}
    assert free == [(x, 0, 0) for x in free_x] and hit == (5, 0, 0)


def test_exact_diagonal_steps_x_then_y_then_z():
    A, B = (128, 128, 128), (640, 640, 640)
    seen, e = ref.walk_one(A, B)
    assert seen == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1)] and e == (2, 2, 2)
    words, _ = one_ray((0.5, 0.5, 0.5), (2.5, 2.5, 2.5), guard=0)
    assert words == {**{v: 1 for v in seen}, (2, 2, 2): 1 << 16}
    words, _ = one_ray((0.5, 0.5, 0.5), (2.5, 2.5, 2.5), guard=1)
    assert words == {(0, 0, 0): 1, (1, 0, 0): 1, (1, 1, 0): 1, (2, 2, 2): 1 << 16}      # from (1, 1, 1) on the end is one voxel away (Chebyshev)


def test_origin_on_a_boundary_moving_in_the_negative_direction():
    seen, e = ref.walk_one((768, 128, 128), (128, 128, 128))
    assert seen == [(3, 0, 0), (2, 0, 0), (1, 0, 0)] and e == (0, 0, 0)     # num = 0 on x: the first step is immediate, voxel 3 still counts
    words, _ = one_ray((3.0, 0.5, 0.5), (0.5, 0.5, 0.5), guard=0)
    assert words == {(3, 0, 0): 1, (2, 0, 0): 1, (1, 0, 0): 1, (0, 0, 0): 1 << 16}
    # ... and in two axes at once, both on a boundary: x first
    seen, e = ref.walk_one((512, 512, 10), (256, 256, 10))
    assert seen == [(2, 2, 0), (1, 2, 0)] and e == (1, 1, 0)


def test_origin_outside_and_end_outside_the_grid():
    words, (free, hit) = one_ray((-2.5, 0.5, 0.5), (2.5, 0.5, 0.5), guard=0)
    assert words == {(0, 0, 0): 1, (1, 0, 0): 1, (2, 0, 0): 1 << 16}
    assert ref.walk_one((-640, 128, 128), (640, 128, 128))[0][:3] == [(-3, 0, 0), (-2, 0, 0), (-1, 0, 0)]
    words, (free, hit) = one_ray((5.5, 0.5, 0.5), (10.5, 0.5, 0.5), guard=2)
    assert words == {(5, 0, 0): 1, (6, 0, 0): 1, (7, 0, 0): 1} and hit is None      # voxels 8 and 9 are walked but outside; no HIT
    words, _ = one_ray((5.5, 0.5, 0.5), (10.5, 0.5, 0.5), guard=0, nz=1, z0=1.0)   # the whole ray below the grid
    assert words == {}


def test_vote_table():
    F = lambda *s: sum(1 << k for k in s)
    H = lambda *s: sum(1 << (16 + k) for k in s)
    #        word                               fv hv  dynamic at min_votes 2 / 1
    table = [(0,                                0, 0, False, False),
             (F(0),                             1, 0, False, True),
             (F(0, 5),                          2, 0, True, True),
             (F(0, 5) | H(9),                   2, 1, True, True),
             (F(0, 5) | H(9, 10),               2, 2, False, False),           # fv == hv
             (F(0, 5, 7) | H(9, 10),            3, 2, True, True),
             (F(0, 5) | H(5),                   1, 1, False, False),           # sweep 5 also returned from the voxel: its free vote is void
             (F(0, 5, 6) | H(5),                2, 1, True, True),
             (H(1, 2, 3),                       0, 3, False, False),
             (0xFFFFFFFF,                       0, 16, False, False),
             (0x0000FFFF,                       16, 0, True, True)]
    words = np.array([t[0] for t in table], np.uint32)
    fv, hv = ref.votes(words)
    assert fv.tolist() == [t[1] for t in table] and hv.tolist() == [t[2] for t in table]
    rule = {**UNIT, "nx": len(table), "ny": 1, "nz": 1}
    grid = words.reshape(1, 1, -1).copy()
    pts = np.array([[k + 0.5, 0.5, 0.5] for k in range(len(table))], np.float32)
    for mv, col in ((2, 3), (1, 4)):
        dyn, qf, qh = ref.query(grid, pts, min_votes=mv, **rule)
        assert qf.tolist() == fv.tolist() and qh.tolist() == hv.tolist() and dyn.tolist() == [t[col] for t in table]
    skip = np.zeros(len(table), np.uint8)
    skip[2] = 1
    dyn, qf, qh = ref.query(grid, pts, skip, **rule)
    assert not dyn[2] and qf[2] == 0 and qh[2] == 0 and dyn[3]
    outside = np.array([[len(table) + 0.5, 0.5, 0.5], [0.5, 0.5, 1.5], [-0.5, 0.5, 0.5]], np.float32)
    dyn, qf, qh = ref.query(np.full_like(grid, 0xFFFF), outside, **rule)
    assert not dyn.any() and not qf.any() and not qh.any()


def test_rule_f_thresholds():
    def labels(sizes_and_hits):
        ids, dyn = [], []
        for c, (n, k) in enumerate(sizes_and_hits, start=1):
            ids += [c] * n
            dyn += [1] * k + [0] * (n - k)
        ids += [0, 0]
        dyn += [1, 1]                                                        # DYNAMIC points DBSCAN left as noise stay 0
        return ref.cluster_labels(np.array(ids), np.array(dyn)), np.array(ids)
    out, ids = labels([(8, 2), (8, 3), (13, 3), (12, 3), (9, 9), (40, 9), (40, 10)])
    got = [int(out[ids == c][0]) for c in range(1, 8)]
    # k = 2 fails; k = 3 with n = 8, 12 pass (4k >= n), n = 13 fails (4k = n - 1); 9 of 40 fails (36 = n - 4), 10 of 40 passes (4k = n)
    assert got == [0, 1, 0, 2, 3, 0, 4]
    assert all(len(set(out[ids == c].tolist())) == 1 for c in range(1, 8)) and (out[ids == 0] == 0).all() and out.dtype == np.int32
    out, ids = labels([(11, 3), (12, 3)])
    assert [int(out[ids == c][0]) for c in (1, 2)] == [1, 2]                # 4k = n + 1 and 4k = n both pass


def test_array_walk_equals_the_python_walk():
    rng = np.random.default_rng(5)
    rule = dict(UNIT, guard=1)
    n = 600
    origins = rng.uniform(-2.0, 10.0, (16, 3)).astype(np.float32)
    origins[:, 2] = rng.uniform(-1.0, 5.0, 16)
    origins[3] = (4.0, 2.0, 1.0)                                             # on voxel boundaries
    pts = rng.uniform(-3.0, 11.0, (n, 3)).astype(np.float32)
    pts[:, 2] = rng.uniform(-1.5, 5.5, n)
    pts[::7] = np.floor(pts[::7])                                            # ends on boundaries: ties
    slot = rng.integers(0, 16, n).astype(np.uint8)
    grid = ref.new_map(**rule)
    ref.carve(grid, pts, slot, origins, **rule)
    want = ref.new_map(**rule)
    A16, _ = ref.quantise(origins, **rule)
    B, _ = ref.quantise(pts, **rule)
    for i in range(n):
        free, hit = ref.marks_one(A16[slot[i]], B[i], **rule)
        for x, y, z in free:
            want[z, y, x] |= np.uint32(1 << int(slot[i]))
        if hit is not None:
            want[hit[2], hit[1], hit[0]] |= np.uint32(1 << (16 + int(slot[i])))
    assert np.array_equal(grid, want) and (grid & 0xFFFF).any() and (grid >> 16).any()
    # marks accumulate and do not depend on the order or the split of the calls
    again = ref.new_map(**rule)
    order = rng.permutation(n)
    ref.carve(again, pts[order][:250], slot[order][:250], origins, **rule)
    ref.carve(again, pts[order][250:], slot[order][250:], origins, **rule)
    assert np.array_equal(again, grid)


def test_walk_is_a_monotone_6_connected_path_through_every_sample():
    """Independent of the rule's arithmetic: the float64 points A + t (B - A) of a segment must all lie in voxels of the path."""
    rng = np.random.default_rng(20)
    n_seg, n_samples = 300, 4096
    t = np.linspace(0.0, 1.0, n_samples)
    exempt = total = 0
    for i in range(n_seg):
        span = (2000, 40000, 600000)[i % 3]
        A = rng.integers(-span, span, 3)
        B = A + rng.integers(-span, span, 3) * np.array(((1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 1, 1))[i % 4])
        seen, e = ref.walk_one(A, B)
        path = seen + [e]
        v, owed = A >> 8, np.abs((B >> 8) - (A >> 8))
        assert path[0] == tuple(v) and len(path) == int(owed.sum()) + 1
        steps = np.diff(np.array(path, dtype=np.int64), axis=0)
        assert (np.abs(steps).sum(axis=1) == 1).all()                        # 6-connected: one axis, one voxel at a time
        assert ((steps * np.sign(B - A)) >= 0).all()                         # monotone on every axis
        pos = A[None, :].astype(np.float64) + t[:, None] * (B - A).astype(np.float64)[None, :]
        vox = pos / 256.0
        near_edge = (np.abs(vox - np.round(vox)) <= 1e-6).any(axis=1)        # the ONLY exclusion: within 1e-6 voxel of a boundary
        cells = set(path)
        inside = np.array([tuple(c) in cells for c in np.floor(vox).astype(np.int64).tolist()])
        assert inside[~near_edge].all(), f"segment {i}: {A} -> {B}"
        exempt, total = exempt + int(near_edge.sum()), total + n_samples
    assert exempt < 0.01 * total, (exempt, total)


def test_params_mirror_and_what_is_admitted():
    """host side of the ABI: the ctypes mirror has the compiled layout, ``scale`` follows from ``voxel``, and the admitted ranges"""
    import ctypes
    from himo_amd import _lib
    from himo_amd.raymap import RaymapParams, map_bytes, neighbours
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_raymap_params") == ctypes.sizeof(RaymapParams) == 40
    p = RaymapParams()
    assert (p.nx, p.ny, p.nz, p.guard, p.min_votes) == (512, 512, 30, 2, 2) and np.float32(p.scale) == ref.scale_of(0.2)
    assert map_bytes(p) == 4 * 512 * 512 * 30 and map_bytes(RaymapParams(**UNIT)) == 4 * 256
    assert map_bytes(RaymapParams(nx=1024, ny=1024, nz=16)) == 4 << 24 and map_bytes(RaymapParams(nx=1024, ny=1024, nz=17)) == 0
    for kw in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(y0=float("inf")), dict(nx=0), dict(nx=1025), dict(nz=65),
               dict(guard=-1), dict(guard=9), dict(min_votes=0), dict(min_votes=17)):
        assert map_bytes(RaymapParams(**kw)) == 0, kw
    assert all(map_bytes(RaymapParams(guard=g, min_votes=m)) > 0 for g, m in ((0, 1), (8, 16)))
    for t, n, w in ((0, 1, 5), (0, 12, 5), (5, 11, 5), (11, 12, 5), (8, 20, 8), (3, 9, 0)):
        assert neighbours(t, n, w) == ref.neighbours(t, n, w)
    assert len(neighbours(8, 20, 8)) == 16
    with pytest.raises(ValueError):
        neighbours(0, 4, 9)


# ---- the toy scene ---------------------------------------------------------------------------------------------------------------
SENSOR_H, WALL_Y, DT = 1.73, 8.07, 0.1
BOX_DIMS, BOX_SPEED, EGO_SPEED = np.array([4.0, 2.0, 1.6]), 10.0, 5.0
GROUND, WALL, BOX = 0, 1, 2


def ray_cast_sweep(k, n_beams=24, n_az=600):
    """Sweep k of the toy drive: (points float32 [n, 3] in the sensor frame, kind uint8 [n], pose float64 4x4).  World: the ground
    plane z = -SENSOR_H, a wall in the plane y = WALL_Y (fixed in the world), one box on the ground driving along +x at BOX_SPEED; the sensor drives
    along +x at EGO_SPEED, no rotation.  One return per ray: the nearest surface within 45 m."""
    ego = np.array([EGO_SPEED * DT * k, 0.0, 0.0])
    centre = np.array([3.0 + BOX_SPEED * DT * k, -5.0, -SENSOR_H + BOX_DIMS[2] / 2])
    el = np.deg2rad(np.linspace(-24.0, 4.0, n_beams))
    az = np.deg2rad(np.arange(n_az) * (360.0 / n_az) + 0.05)
    el, az = np.meshgrid(el, az, indexing="ij")
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)
    with np.errstate(all="ignore"):
        tg = np.where(d[:, 2] < 0, -SENSOR_H / d[:, 2], np.inf)
        tw = np.where(d[:, 1] > 0, WALL_Y / d[:, 1], np.inf)
        hw = ego + tw[:, None] * d
        tw = np.where((hw[:, 2] <= 2.5) & (np.abs(hw[:, 0] - 2.5) <= 30.0), tw, np.inf)
        lo, hi = (centre - BOX_DIMS / 2 - ego) / d, (centre + BOX_DIMS / 2 - ego) / d
        t_in, t_out = np.minimum(lo, hi).max(axis=1), np.maximum(lo, hi).min(axis=1)
        tb = np.where((t_in <= t_out) & (t_in > 0), t_in, np.inf)
    tt = np.stack([tg, tw, tb], axis=1)
    kind, t_hit = tt.argmin(axis=1), tt.min(axis=1)
    keep = t_hit <= 45.0
    pose = np.eye(4)
    pose[:3, 3] = ego
    return (t_hit[keep, None] * d[keep]).astype(np.float32), kind[keep].astype(np.uint8), pose


@pytest.fixture(scope="module")
def toy_scene():
    sweeps = [ray_cast_sweep(k) for k in range(11)]
    return [s[0] for s in sweeps], [s[1] for s in sweeps], [s[2] for s in sweeps]


TARGET = 5


def toy_flags(clouds, kinds, poses, moved=None):
    """the restatement on the toy scene's target sweep; ``moved``: the neighbours' points already in the target's frame"""
    nb = ref.neighbours(TARGET, len(clouds))
    assert nb == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]
    origins = np.zeros((16, 3), np.float32)
    own = []
    for s, k in enumerate(nb):
        T = ref.relative_pose(poses[TARGET], poses[k])
        origins[s] = T[:3, 3]
        own.append(ref.move(clouds[k], T))
    return ref.dynamic_flags(clouds[TARGET], kinds[TARGET] == GROUND, own if moved is None else moved, origins)


def test_toy_scene_box_is_dynamic_and_wall_is_not(toy_scene):
    clouds, kinds, poses = toy_scene
    assert all(len(c) <= 32 * 900 for c in clouds)
    kind = kinds[TARGET]
    n_box, n_wall = int((kind == BOX).sum()), int((kind == WALL).sum())
    assert n_box >= 200 and n_wall >= 1000
    dyn, fv, hv = toy_flags(clouds, kinds, poses)
    box_share, wall_share = dyn[kind == BOX].mean(), dyn[kind == WALL].mean()
    print(f"\ntoy scene, guard 2: {100 * box_share:.1f} % of {n_box} box points and {100 * wall_share:.1f} % of {n_wall} wall points DYNAMIC")
    assert not dyn[kind == GROUND].any()                                     # the target's ground is passed as skip
    assert box_share >= 0.80
    assert wall_share <= 0.10
    ids = ref.dbscan(clouds[TARGET], skip=ref.cluster_skip(clouds[TARGET], kind == GROUND))
    labels = ref.cluster_labels(ids, dyn)
    assert (labels[kind == WALL] == 0).all()
    assert set(labels[kind == BOX].tolist()) == {1} and int(labels.max()) == 1 and (labels[kind != BOX] == 0).all()


# ---- the loader --------------------------------------------------------------------------------------------------------------------
def test_loader_serves_any_field_of_the_next_sweep(tmp_path):
    from himo_amd import h5lite
    from himo_amd.dataset import HDF5Dataset
    from himo_amd.seflow.fit import train_fields
    from himo_amd.synthetic import make_scene, write_h5_scenes
    import pickle
    scenes = [make_scene(70 + s, 3, n_points=500, scene_id=f"rm{s}") for s in range(2)]
    write_h5_scenes(tmp_path, scenes)
    # the same scenes with one more dataset per sweep, as the labeller leaves them
    index, labels = [], {}
    for frames in scenes:
        tree = {}
        for j, f in enumerate(frames):
            ts = str(f["timestamp"])
            with h5lite.File(tmp_path / f"{f['scene_id']}.h5") as old:
                tree[ts] = {k: np.asarray(old[ts][k][:]) for k in old[ts].keys()}
            labels[(f["scene_id"], ts)] = tree[ts]["ray_label"] = (np.arange(len(f["pc0"])) % (j + 2)).astype(np.int32)
            index.append([f["scene_id"], ts])
        h5lite.write_file(tmp_path / f"{frames[0]['scene_id']}.h5", tree)
    with open(tmp_path / "index_total.pkl", "wb") as fh:
        pickle.dump(index, fh)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                      # (the last sweep of a scene has no successor)
        ds = HDF5Dataset(tmp_path, fields=train_fields("ray_label"))
    try:
        assert len(ds) == 4
        for i in range(len(ds)):
            f = ds[i]
            scene, ts = f["scene_id"], str(f["timestamp"])
            nxt = ds._next[(scene, ts)]
            assert f["ray_label"].dtype == np.int32 and np.array_equal(f["ray_label"], labels[(scene, ts)])
            assert np.array_equal(f["ray_label_next"], labels[(scene, nxt)]) and len(f["ray_label_next"]) == len(f["pc1"])
            assert "flow" not in f and "gm1" in f
        only = ds.read(0, ("ray_label_next",))                               # the successor is opened for such a field alone
        assert set(only) == {"scene_id", "timestamp", "ray_label_next"}
        assert "no_such_next" not in ds.read(0, ("pc0", "no_such_next"))     # a name the successor does not hold is left out
    finally:
        ds.close()
