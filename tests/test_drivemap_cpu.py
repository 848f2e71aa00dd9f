"""The whole-drive free-space map without a GPU: the numpy restatement of "free-space drive map, v1" (tests/drivemap_ref.py; the rule
is the module docstring of himo_amd/drivemap.py) tied to the already pinned restatement of "free-space ray map, v1", against
hand-worked cases and on the ray-cast toy drive of tests/test_raymap_cpu.py; and the host side of the rule: the extent of a scene, the
admitted parameters, the struct mirror and the per-sensor ray origins."""
import ctypes

import numpy as np
import pytest

import drivemap_ref as ref
import raymap_ref as rr
import test_raymap_cpu as toy
from test_raymap_cpu import BOX, GROUND, UNIT, WALL, ray_cast_sweep

SMALL = dict(UNIT, guard=0, min_votes=2, min_hits=2)              # the 8 x 8 x 4 grid, a coordinate IS its voxel index


def table(*rows):
    o = np.zeros((16, 3), np.float32)
    for k, r in enumerate(rows):
        o[k] = r
    return o


def carve_rays(dm, sweep, ends, origin=(0.5, 0.5, 0.5)):
    ends = np.asarray(ends, np.float32).reshape(-1, 3)
    dm.carve(ends, np.zeros(len(ends), np.uint8), table(origin), sweep)


# ---- (a) the tie to v1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sweeps, guard", [(1, 0), (7, 1), (16, 2)])
def test_counts_equal_the_votes_of_one_v1_map_with_a_slot_per_sweep(n_sweeps, guard):
    rng = np.random.default_rng(100 + n_sweeps)
    rule = dict(SMALL, guard=guard)
    dm = ref.DriveMap(**rule)
    one = rr.new_map(**ref.v1_rule(**rule))
    origins16 = np.zeros((16, 3), np.float32)
    for s in range(n_sweeps):
        origin = rng.uniform((-1.0, -1.0, 0.0), (9.0, 9.0, 4.0)).astype(np.float32)
        ends = rng.uniform((-2.0, -2.0, -1.0), (10.0, 10.0, 5.0), (120, 3)).astype(np.float32)
        ends[::5] = np.floor(ends[::5])
        dm.carve(ends, np.zeros(len(ends), np.uint8), table(origin), s)
        origins16[s] = origin
        rr.carve(one, ends, np.full(len(ends), s, np.uint8), origins16, **ref.v1_rule(**rule))
    free_n, hit_n = dm.counts()
    fv, hv = rr.votes(one)
    assert np.array_equal(free_n, fv) and np.array_equal(hit_n, hv) and hit_n.any() and (n_sweeps == 1 or free_n.max() > 1)


# ---- (b) hand-worked cases ---------------------------------------------------------------------------------------------------------
def test_free_in_sweeps_0_1_and_hit_in_1_2_counts_one_free_and_two_hits():
    dm = ref.DriveMap(**SMALL)
    carve_rays(dm, 0, [(5.5, 0.5, 0.5)])                                   # FREE x = 0..4, HIT 5
    carve_rays(dm, 1, [(5.5, 0.5, 0.5), (3.5, 0.5, 0.5)])                  # voxel 3: FREE and HIT in one sweep -> HIT only
    carve_rays(dm, 2, [(3.5, 0.5, 0.5)])
    free_n, hit_n = dm.counts()
    assert free_n[0, 0, :6].tolist() == [3, 3, 3, 1, 2, 0] and hit_n[0, 0, :6].tolist() == [0, 0, 0, 2, 0, 2]
    assert free_n.sum() == 12 and hit_n.sum() == 4
    # the split over calls, the order of the rays and carving them twice change nothing
    again = ref.DriveMap(**SMALL)
    carve_rays(again, 0, [(5.5, 0.5, 0.5)])
    carve_rays(again, 1, [(3.5, 0.5, 0.5)])
    carve_rays(again, 1, [(5.5, 0.5, 0.5)])
    carve_rays(again, 1, [(3.5, 0.5, 0.5), (5.5, 0.5, 0.5)])
    carve_rays(again, 2, [(3.5, 0.5, 0.5)])
    assert all(np.array_equal(a, b) for a, b in zip(again.counts(), (free_n, hit_n)))
    with pytest.raises(ValueError):
        carve_rays(again, 1, [(3.5, 0.5, 0.5)])                            # sweep numbers do not decrease
    with pytest.raises(ValueError):
        carve_rays(again, ref.MAX_SWEEP + 1, [(3.5, 0.5, 0.5)])
    with pytest.raises(ValueError):
        again.carve(np.array([[3.5, 0.5, 0.5]], np.float32), np.array([16], np.uint8), table((0.5, 0.5, 0.5)), 2)
    assert all(np.array_equal(a, b) for a, b in zip(again.counts(), (free_n, hit_n)))


@pytest.mark.parametrize("guard, free_x", [(0, [0, 1, 2, 3, 4]), (1, [0, 1, 2, 3]), (2, [0, 1, 2])])
def test_the_guard(guard, free_x):
    dm = ref.DriveMap(**dict(SMALL, guard=guard))
    carve_rays(dm, 4, [(5.5, 0.5, 0.5)])
    free_n, hit_n = dm.counts()
    assert np.nonzero(free_n[0, 0])[0].tolist() == free_x and free_n.sum() == len(free_x)
    assert np.nonzero(hit_n.reshape(-1))[0].tolist() == [5] and hit_n[0, 0, 5] == 1


def test_an_end_outside_the_grid_hits_nothing():
    dm = ref.DriveMap(**dict(SMALL, guard=2))
    carve_rays(dm, 0, [(10.5, 0.5, 0.5)], origin=(5.5, 0.5, 0.5))
    free_n, hit_n = dm.counts()
    assert np.nonzero(free_n[0, 0])[0].tolist() == [5, 6, 7] and free_n.sum() == 3 and not hit_n.any()
    dyn, fv, hv = dm.query(np.array([[10.5, 0.5, 0.5], [6.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [6.5, 0.5, 0.5]], np.float32), [0, 0, 0, 1])
    assert fv.tolist() == [0, 1, 0, 0] and hv.tolist() == [0, 0, 0, 0] and not dyn.any()


def test_min_votes_and_min_hits_at_their_thresholds():
    def drive(**kw):
        dm = ref.DriveMap(**dict(SMALL, **kw))
        carve_rays(dm, 0, [(3.5, 0.5, 0.5), (1.5, 2.5, 0.5)])              # voxel (3,0,0): HIT once ...
        carve_rays(dm, 1, [(6.5, 0.5, 0.5), (1.5, 2.5, 0.5)])              # ... and seen through by sweeps 1, 2 (and 3)
        carve_rays(dm, 2, [(6.5, 0.5, 0.5), (1.5, 2.5, 0.5)])
        return dm
    q = np.array([[3.5, 0.5, 0.5], [6.5, 0.5, 0.5], [1.5, 2.5, 0.5]], np.float32)
    dm = drive()
    dyn, fv, hv = dm.query(q)
    assert fv.tolist() == [2, 0, 0] and hv.tolist() == [1, 2, 3] and dyn.tolist() == [True, False, False]      # fv = min_votes
    assert drive(min_votes=3).query(q)[0].tolist() == [False, False, False]
    assert dm.query(q, skip=[1, 0, 0])[0].tolist() == [False, False, False]
    # fv == hv is not DYNAMIC, whatever min_votes
    dm1 = drive(min_votes=1)
    carve_rays(dm1, 3, [(3.5, 0.5, 0.5)])
    assert [int(x[0]) for x in dm1.query(q[:1])] == [0, 2, 2]
    # STATIC: hit_n >= min_hits and not DYNAMIC-by-count
    static = lambda d: {tuple(int(c) for c in np.array(v)[::-1]) for v in zip(*np.nonzero(d.static()))}
    assert static(dm) == {(6, 0, 0), (1, 2, 0)}                            # hit_n 2 and 3; voxel (3,0,0) has hit_n 1
    assert static(drive(min_hits=3)) == {(1, 2, 0)} and static(drive(min_hits=4)) == set()
    assert static(drive(min_hits=1)) == {(6, 0, 0), (1, 2, 0)}             # (3,0,0): hit_n 1 but free_n 2 > 1: carved away
    assert static(drive(min_hits=1, min_votes=3)) == {(3, 0, 0), (6, 0, 0), (1, 2, 0)}


def test_emit_order_and_centres():
    dm = ref.DriveMap(**dict(SMALL, min_hits=1))
    ends = [(6.5, 7.5, 3.5), (0.5, 0.5, 0.5), (7.5, 0.5, 0.5), (2.5, 1.5, 0.5), (1.5, 0.5, 2.5)]
    carve_rays(dm, 0, ends, origin=(4.5, 4.5, 1.5))
    carve_rays(dm, 1, ends[:2], origin=(4.5, 4.5, 1.5))
    rows, hits, free = dm.emit()
    assert rows.dtype == np.float32 and hits.dtype == np.int32 and free.dtype == np.int32
    assert rows.tolist() == [[0.5, 0.5, 0.5, 0.0], [7.5, 0.5, 0.5, 0.0], [2.5, 1.5, 0.5, 0.0], [1.5, 0.5, 2.5, 0.0], [6.5, 7.5, 3.5, 0.0]]
    assert hits.tolist() == [2, 1, 1, 1, 2] and free.tolist() == [0, 0, 0, 0, 0]
    # the centre is ((float)v + 0.5f) * voxel + minimum, every operation rounded to float32
    rule = dict(x0=-12.3, y0=4.56, z0=-3.0, voxel=0.2, nx=40, ny=30, nz=12, guard=1, min_votes=2, min_hits=1)
    dm = ref.DriveMap(**rule)
    rng = np.random.default_rng(8)
    ends = (rng.uniform(0.0, 1.0, (200, 3)) * (8.0, 6.0, 2.4) + (-12.3, 4.56, -3.0)).astype(np.float32)
    dm.carve(ends, np.zeros(200, np.uint8), table((-8.0, 7.0, -2.0)), 0)
    rows, hits, free = dm.emit()
    u, ok = rr.quantise(rows[:, :3], **ref.v1_rule(**rule))
    v = u >> 8
    lin = (v[:, 2] * 30 + v[:, 1]) * 40 + v[:, 0]
    assert ok.all() and (np.diff(lin) > 0).all() and len(rows) == int(dm.static().sum()) > 50
    f = np.float32
    for col, m in enumerate((-12.3, 4.56, -3.0)):
        want = [f(f(f(f(int(c)) + f(0.5)) * f(0.2)) + f(m)) for c in v[:, col]]
        assert rows[:, col].tolist() == [float(x) for x in want]
    assert np.array_equal(hits, dm.counts()[1].reshape(-1)[lin]) and (rows[:, 3] == 0).all()


# ---- (c) the extent of a scene -------------------------------------------------------------------------------------------------------
def pose_at(x, y=0.0, z=0.0, yaw=0.0):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = (x, y, z)
    return T


def test_scene_extent():
    from himo_amd.drivemap import scene_extent
    p = scene_extent([np.eye(4)])
    assert (p.nx, p.ny, p.nz, p.guard, p.min_votes, p.min_hits) == (512, 512, 30, 2, 2, 2) and np.float32(p.voxel) == np.float32(0.2)
    assert np.float32(p.scale) == rr.scale_of(0.2) and p.admitted()
    # the frame is the first sweep's: a scene that starts far from the world origin, heading elsewhere, has the same grid
    world = pose_at(5000.0, -300.0, 12.0, yaw=0.7)
    local = [pose_at(3.33 * k, -0.777 * k, 0.05 * k) for k in range(20)]
    p = scene_extent(local, voxel=0.25, z_lo=-3.1, z_hi=3.1)
    q = scene_extent([world @ T for T in local], voxel=0.25, z_lo=-3.1, z_hi=3.1)
    assert (p.nx, p.ny, p.nz) == (q.nx, q.ny, q.nz) and abs(p.x0 - q.x0) < 1e-3 and abs(p.y0 - q.y0) < 1e-3
    for m, n, lo, hi in ((p.x0, p.nx, -51.2, 3.33 * 19 + 51.2), (p.y0, p.ny, -0.777 * 19 - 51.2, 51.2), (p.z0, p.nz, -3.1, 0.95 + 3.1)):
        assert abs(m / 0.25 - round(m / 0.25)) < 1e-4, m                  # a multiple of the voxel
        assert lo - 0.25 < m <= lo + 1e-4 and hi - 1e-4 <= m + 0.25 * n < hi + 0.5
    # a 40 km drive does not fit 16384 voxels of 0.2 m; a coarser voxel or half the drive does not help here either -- refused by name
    with pytest.raises(ValueError, match=r"long_drive.*not admitted.*raise --voxel or split the scene"):
        scene_extent([pose_at(0.0), pose_at(40_000.0)], where="long_drive")
    # 1 km of 0.2 m voxels: 5512 x 512 x 30 words = 0.63 GiB
    km = [pose_at(0.0), pose_at(1000.0)]
    assert scene_extent(km).nx == 5512
    with pytest.raises(ValueError, match=r"0\.63 GiB.*--max_map_gib 0\.5.*raise --voxel or split the scene"):
        scene_extent(km, max_map_gib=0.5)
    assert scene_extent(km, max_map_gib=0.5, voxel=0.4).nx == 2756
    for kw in (dict(voxel=0.0), dict(voxel=float("nan")), dict(guard=9), dict(min_votes=0), dict(min_hits=65536), dict(z_lo=1.0, z_hi=0.0)):
        with pytest.raises(ValueError):
            scene_extent([np.eye(4)], **kw)
    with pytest.raises(ValueError):
        scene_extent([])


# ---- (d) parameters and the struct mirror --------------------------------------------------------------------------------------------
def test_params_mirror_and_what_is_admitted():
    from himo_amd import _lib
    from himo_amd.drivemap import DriveMapParams, map_bytes
    names = [n for n, _ in DriveMapParams._fields_]
    assert names == ["x0", "y0", "z0", "voxel", "scale", "nx", "ny", "nz", "guard", "min_votes", "min_hits"]
    assert all(t is ctypes.c_float for _, t in DriveMapParams._fields_[:5]) and all(t is ctypes.c_int32 for _, t in DriveMapParams._fields_[5:])
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_drivemap_params") == ctypes.sizeof(DriveMapParams) == 44
    p = DriveMapParams()
    assert (np.float32(p.voxel), p.guard, p.min_votes, p.min_hits) == (np.float32(0.2), 2, 2, 2) and np.float32(p.scale) == rr.scale_of(0.2)
    assert map_bytes(p) == 8 * 512 * 512 * 30 and map_bytes(DriveMapParams(**UNIT)) == 8 * 256 and lib.himo_drivemap_bytes(None) == 0
    good = [dict(nx=16384, ny=16384, nz=2), dict(nx=1, ny=1, nz=256), dict(guard=0, min_votes=1, min_hits=1), dict(guard=8, min_votes=65535, min_hits=65535),
            dict(nx=2048, ny=1024, nz=256)]
    bad = [dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=1e-40), dict(y0=float("inf")), dict(z0=float("nan")), dict(nx=0),
           dict(nx=16385), dict(ny=0), dict(ny=16385), dict(nz=0), dict(nz=257), dict(nx=16384, ny=16384, nz=3), dict(nx=2049, ny=1024, nz=256),
           dict(guard=-1), dict(guard=9), dict(min_votes=0), dict(min_votes=65536), dict(min_hits=0), dict(min_hits=65536)]
    for kw in good:
        q = DriveMapParams(**kw)
        assert q.admitted() and map_bytes(q) == 8 * q.nx * q.ny * q.nz, kw
        assert lib.himo_drivemap_emit_workspace_bytes(ctypes.addressof(q)) > 0
    for kw in bad:
        q = DriveMapParams(**kw)
        assert not q.admitted() and map_bytes(q) == 0 and lib.himo_drivemap_emit_workspace_bytes(ctypes.addressof(q)) == 0, kw
    q = DriveMapParams()
    q.scale = 1279.0                                                       # not (float)(256.0 / voxel)
    assert not q.admitted() and map_bytes(q) == 0


# ---- (e) per-sensor origins ----------------------------------------------------------------------------------------------------------
def test_origins_frame_and_sensors():
    from himo_amd.drivemap import sweep_sources
    T = pose_at(10.0, -2.0, 0.5, yaw=np.pi / 2).astype(np.float32)
    src, org = sweep_sources(T, 5)
    assert src.dtype == np.uint8 and src.tolist() == [0] * 5 and org.dtype == np.float32 and org.shape == (16, 3)
    assert org[0].tolist() == [10.0, -2.0, 0.5] and not org[1:].any()
    # ranks among the sweep's sorted distinct ids: the row order of the stored centres (np.unique order)
    ids = np.array([9, 2, 5, 5, 9, 2, 2], np.uint8)
    centres = np.array([[3.5, 0.0, 0.5], [0.0, 1.2, 0.0], [0.0, -1.2, 0.0]])                # of ids 2, 5, 9
    src, org = sweep_sources(T, 7, "sensors", ids, centres)
    assert src.tolist() == [2, 0, 1, 1, 2, 0, 0]
    assert np.allclose(org[:3], [[10.0, 1.5, 1.0], [8.8, -2.0, 0.5], [11.2, -2.0, 0.5]], atol=1e-5) and not org[3:].any()
    assert not sweep_sources(T, 7, "sensors", ids, np.concatenate([centres, [[9.0, 9.0, 9.0]]]))[1][3:].any()           # a spare row is not used
    with pytest.raises(KeyError, match="SensorsCenter.*sweep 17"):
        sweep_sources(T, 7, "sensors", ids, None, where="sweep 17")
    with pytest.raises(ValueError, match="17 distinct sensor ids"):
        sweep_sources(T, 34, "sensors", np.arange(34) % 17, np.zeros((17, 3)))
    with pytest.raises(ValueError, match="2 centre rows for 3 distinct"):
        sweep_sources(T, 7, "sensors", ids, centres[:2])
    with pytest.raises(ValueError, match="origins"):
        sweep_sources(T, 7, "lidars")
    assert sweep_sources(T, 16, "sensors", np.arange(16) * 3, np.ones((16, 3)))[0].tolist() == list(range(16))


# ---- (f) the toy drive ---------------------------------------------------------------------------------------------------------------
def toy_drive(n_sweeps, box_speed):
    """the whole-drive restatement over ``n_sweeps`` of the toy drive with the box at ``box_speed``: (clouds, kinds, poses, per-sweep
    dynamic flags of the asked targets)"""
    from himo_amd.drivemap import scene_extent, sweep_sources
    old = toy.BOX_SPEED
    toy.BOX_SPEED = box_speed
    try:
        sweeps = [ray_cast_sweep(k) for k in range(n_sweeps)]
    finally:
        toy.BOX_SPEED = old
    clouds, kinds, poses = [s[0] for s in sweeps], [s[1] for s in sweeps], [s[2] for s in sweeps]
    p = scene_extent(poses, range_m=46.0)                                  # (no return is further than 45 m)
    rule = {k: getattr(p, k) for k in ref.DEFAULTS}
    T = ref.relative_poses(poses)
    dm = ref.DriveMap(**rule)
    moved = []
    for k in range(n_sweeps):
        moved.append(rr.move(clouds[k], T[k]))
        src, org = sweep_sources(T[k], len(moved[k]))
        dm.carve(moved[k], src, org, k)
    return clouds, kinds, poses, lambda t: dm.query(moved[t], kinds[t] == GROUND)


def v1_flags(clouds, kinds, poses, t, window=5):
    nb = rr.neighbours(t, len(clouds), window)
    origins, own = np.zeros((16, 3), np.float32), []
    for s, k in enumerate(nb):
        T = rr.relative_pose(poses[t], poses[k])
        origins[s] = T[:3, 3]
        own.append(rr.move(clouds[k], T))
    return rr.dynamic_flags(clouds[t], kinds[t] == GROUND, own, origins)


@pytest.fixture(scope="module")
def fast_box():
    return toy_drive(30, 10.0)


@pytest.fixture(scope="module")
def slow_box():
    return toy_drive(60, 2.0)


def shares(kind, dyn):
    return float(dyn[kind == BOX].mean()), float(dyn[kind == WALL].mean())


def test_toy_drive_fast_box(fast_box):
    clouds, kinds, poses, query = fast_box
    dyn, fv, hv = query(15)
    box, wall = shares(kinds[15], dyn)
    print(f"\n30 sweeps, box 10 m/s, sweep 15: {100 * box:.1f} % of the box, {100 * wall:.2f} % of the wall DYNAMIC")
    assert box >= 0.80, f"box share {box:.3f} (the prototype measured 0.873)"
    assert wall <= 0.01, f"wall share {wall:.4f} (the prototype measured 0.000)"
    assert not dyn[kinds[15] == GROUND].any() and (hv[kinds[15] != GROUND] >= 1).all()      # its own rays are part of the map


def test_toy_drive_parked_box():
    clouds, kinds, poses, query = toy_drive(30, 0.0)
    dyn, _, _ = query(15)
    box, wall = shares(kinds[15], dyn)
    assert box == 0.0, f"parked box share {box:.3f} (the prototype measured 0.000)"
    assert wall <= 0.01, f"wall share {wall:.4f}"


def test_toy_drive_slow_box_against_v1(slow_box):
    clouds, kinds, poses, query = slow_box
    dyn, _, _ = query(30)
    box, wall = shares(kinds[30], dyn)
    v1_box, v1_wall = shares(kinds[30], v1_flags(clouds, kinds, poses, 30)[0])
    print(f"\n60 sweeps, box 2 m/s, sweep 30: whole drive {100 * box:.1f} % / v1 {100 * v1_box:.1f} % of the box; wall {100 * wall:.2f} % / {100 * v1_wall:.2f} %")
    assert box >= 0.75, f"whole-drive box share {box:.3f} (the prototype measured 0.840)"
    assert v1_box <= 0.50, f"v1 box share {v1_box:.3f} (the prototype measured 0.386)"
    assert wall <= 0.01, f"wall share {wall:.4f} (the prototype measured 0.000)"
