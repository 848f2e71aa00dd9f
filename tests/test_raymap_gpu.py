"""The free-space labeller on the GPU: ``himo_raymap_carve`` / ``himo_raymap_query`` bit for bit against the numpy restatement of
their written rule (tests/raymap_ref.py; parity with the reference's generator is unpinned) -- map words, votes and flags -- over
the ray counts at which blocks and waves fill, contended words, every slot, split calls, both pitches, the hand-worked edge cases
and the refusals; ``dynamic_flags`` and ``cluster_labels`` on the toy scene of tests/test_raymap_cpu.py; then the program end to
end: it writes the labels, the loader serves them for both sweeps of a pair, and the training loop takes a step on them."""
import ctypes
import pickle
import warnings

import numpy as np
import pytest

import raymap_ref as ref
from test_raymap_cpu import GROUND, TARGET, UNIT, ray_cast_sweep, toy_flags

pytestmark = pytest.mark.gpu

GUARD, FILL = 1024, 0xA5                                         # guard bytes on both sides of every output, guard words round the map
SMALL = dict(UNIT, guard=1)                                      # the 8 x 8 x 4 grid


def device_params(**rule):
    from himo_amd.raymap import RaymapParams
    return RaymapParams(**rule)


def launch(pts, slot, origins, queries, skip=None, pitch=3, splits=1, call_pitch=None, params=None, **rule):
    """raw calls: carve ``pts`` in ``splits`` calls into a cleared, guarded map, then query ``queries``.
    -> (statuses, map words uint32 [nz, ny, nx], (dynamic, fv, hv) bytes, guards untouched?)"""
    import torch
    from himo_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    p = params if params is not None else device_params(**rule)
    call_pitch = pitch if call_pitch is None else call_pitch
    cells = int(p.nx) * int(p.ny) * int(p.nz) if params is None else 8 * 8 * 4
    wide = lambda a: np.concatenate([np.asarray(a, np.float32).reshape(-1, 3), np.full((len(a), pitch - 3), 7.0, np.float32)], axis=1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pts, d_q = up(wide(pts).reshape(-1)), up(wide(queries).reshape(-1))
    d_slot, d_org = up(np.asarray(slot, np.uint8)), up(np.asarray(origins, np.float32).reshape(16, 3))
    d_skip = None if skip is None else up(np.asarray(skip, np.uint8))
    grid = torch.full((GUARD + cells + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    grid[GUARD:GUARD + cells] = 0
    n, nq = len(pts), len(queries)
    outs = [torch.full((GUARD + nq + GUARD,), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
    statuses = []
    cuts = np.linspace(0, n, splits + 1).astype(np.int64)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        statuses.append(lib.himo_raymap_carve(int(hi - lo), d_pts.data_ptr() + 4 * pitch * int(lo), call_pitch, d_slot.data_ptr() + int(lo),
                                              d_org.data_ptr(), ctypes.addressof(p), grid.data_ptr() + 4 * GUARD, _lib.stream_handle()))
    statuses.append(lib.himo_raymap_status(_lib.stream_handle()))
    statuses.append(lib.himo_raymap_query(nq, d_q.data_ptr(), call_pitch, _lib.ptr(d_skip), ctypes.addressof(p), grid.data_ptr() + 4 * GUARD,
                                          outs[1].data_ptr() + GUARD, outs[2].data_ptr() + GUARD, outs[0].data_ptr() + GUARD, _lib.stream_handle()))
    torch.cuda.synchronize()
    g = grid.cpu().numpy().view(np.uint32)
    clean = bool((g[:GUARD] == 0x5A5A5A5A).all() and (g[GUARD + cells:] == 0x5A5A5A5A).all())
    got = []
    for o in outs:
        h = o.cpu().numpy()
        clean = clean and bool((h[:GUARD] == FILL).all() and (h[GUARD + nq:] == FILL).all())
        got.append(h[GUARD:GUARD + nq].copy())
    words = g[GUARD:GUARD + cells].copy()
    return statuses, (words.reshape(int(p.nz), int(p.ny), int(p.nx)) if params is None else words), tuple(got), clean


def assert_equals_the_restatement(pts, slot, origins, queries, skip=None, **kw):
    rule = {k: v for k, v in kw.items() if k in ref.DEFAULTS}
    statuses, words, (dyn, fv, hv), clean = launch(pts, slot, origins, queries, skip, **kw)
    assert statuses == [0] * len(statuses) and clean
    want = ref.new_map(**rule)
    ref.carve(want, pts, slot, origins, **rule)
    assert np.array_equal(words, want), f"{int((words != want).sum())} of {want.size} map words differ"
    wd, wf, wh = ref.query(want, queries, skip, **rule)
    assert set(np.unique(dyn)) <= {0, 1}
    assert np.array_equal(fv, wf) and np.array_equal(hv, wh) and np.array_equal(dyn.astype(bool), wd)
    return want, wd


def rays(seed, n, lo=-3.0, hi=11.0, z=(-1.5, 5.5), org=(-2.0, 10.0)):
    """random rays round the 8 x 8 x 4 grid: every slot, some ends and origins outside, ends on voxel boundaries, a few rays that
    take no part"""
    rng = np.random.default_rng(seed)
    origins = rng.uniform(org[0], org[1], (16, 3)).astype(np.float32)
    origins[:, 2] = rng.uniform(-1.0, 5.0, 16)
    origins[3] = (4.0, 2.0, 1.0)
    pts = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    pts[:, 2] = rng.uniform(z[0], z[1], n)
    pts[::7] = np.floor(pts[::7])
    slot = (np.arange(n) % 16).astype(np.uint8)                   # all 16 slots in one call once n >= 16
    rng.shuffle(slot)
    slot[5::23] = 255
    if n > 40:
        pts[11], pts[29] = (np.nan, 1, 1), (1, np.inf, 1)
    queries = np.concatenate([pts, rng.uniform(-1.0, 9.0, (64, 3)).astype(np.float32)])
    queries[np.isnan(queries) | np.isinf(queries)] = 2.5
    return pts, slot, origins, queries


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("pitch", [3, 4])
def test_ray_counts_and_both_pitches(gpu, n, pitch):
    pts, slot, origins, queries = rays(n, n)
    want, _ = assert_equals_the_restatement(pts, slot, origins, queries, pitch=pitch, **SMALL)
    assert n < 63 or ((want & 0xFFFF).any() and (want >> 16).any())


def test_many_lanes_or_the_same_words(gpu):
    rng = np.random.default_rng(9)
    n = 4096
    origins = np.tile(np.array([0.4, 0.6, 0.5], np.float32), (16, 1))
    pts = rng.uniform((5.0, 5.0, 2.0), (7.0, 7.0, 3.0), (n, 3)).astype(np.float32)
    slot = rng.integers(0, 16, n).astype(np.uint8)
    queries = rng.uniform(0.0, 8.0, (2000, 3)).astype(np.float32)
    queries[:, 2] = rng.uniform(0.0, 4.0, 2000)
    skip = (rng.random(2000) < 0.2).astype(np.uint8)
    for guard, mv in ((0, 2), (2, 16)):
        want, dyn = assert_equals_the_restatement(pts, slot, origins, queries, skip, pitch=4, **dict(UNIT, guard=guard, min_votes=mv))
        assert (want[0, 0, 0] & 0xFFFF) == 0xFFFF                 # every sweep saw through the origin's voxel
    assert dyn.any()


def test_two_carve_calls_equal_one(gpu):
    pts, slot, origins, queries = rays(77, 1000)
    one = launch(pts, slot, origins, queries, **SMALL)
    two = launch(pts, slot, origins, queries, splits=2, **SMALL)
    five = launch(pts[::-1].copy(), slot[::-1].copy(), origins, queries, splits=5, pitch=4, **SMALL)
    for st, words, out, clean in (one, two, five):
        assert st == [0] * len(st) and clean
        assert np.array_equal(words, one[1]) and all(np.array_equal(a, b) for a, b in zip(out, one[2]))
    assert_equals_the_restatement(pts, slot, origins, queries, splits=3, **SMALL)


def test_hand_worked_edge_cases(gpu):
    origins = np.zeros((16, 3), np.float32)
    origins[0], origins[1], origins[2], origins[4] = (0.5, 0.5, 0.5), (3.0, 0.5, 0.5), (-2.5, 0.5, 0.5), (5.5, 0.5, 0.5)
    origins[5], origins[6], origins[7] = (np.nan, 0.5, 0.5), (2.0, 2.0, 0.04), (16383.0, 1.0, 1.0)
    big = np.float32(16384.0)
    cases = [((5.5, 0.5, 0.5), 0),                                # axis-aligned
             ((2.5, 2.5, 2.5), 0),                                # the exact diagonal: x, then y, then z
             ((0.5, 0.5, 0.5), 1),                                # from a voxel boundary in the negative direction
             ((1.0, 1.0, 0.04), 6),                               # ... in two axes at once
             ((2.5, 0.5, 0.5), 2),                                # origin outside the grid
             ((10.5, 0.5, 0.5), 4),                               # end outside the grid
             ((np.nan, 1, 1), 0), ((1, np.inf, 1), 0), ((1, 1, -np.inf), 0), ((big, 1, 1), 0), ((1, -big, 1), 0),
             ((np.nextafter(big, np.float32(0)), 1, 1), 7),       # the last usable value, from an origin as far out
             ((40.5, 0.7, 0.5), 0), ((-30.5, 0.5, 2.5), 4),       # far outside: the walk leaves the grid, in either direction, and may stop
             ((5.5, 0.5, 0.5), 5),                                # an unusable origin
             ((5.5, 0.5, 0.5), 255),                              # no part
             ((0.5, 0.5, 0.5), 0)]                                # origin and end in one voxel: a HIT and nothing else
    pts = np.array([c[0] for c in cases], np.float32)
    slot = np.array([c[1] for c in cases], np.uint8)
    queries = np.concatenate([np.nan_to_num(pts, nan=1.5, posinf=1.5, neginf=1.5), pts[6:11]])
    for guard in (0, 1, 2):
        want, _ = assert_equals_the_restatement(pts, slot, origins, queries, **dict(UNIT, guard=guard))
        free0 = [x for x in range(8) if want[0, 0, x] & 1]
        assert free0[:5 - guard] == list(range(5 - guard)) and (want[0, 0, 5] >> 16) & 1 and (want[2, 2, 2] >> 16) & 1
        assert (want[0, 0, 0] >> 16) & 1 and want[0, 0, 7] & (1 << 4)
    # each case alone, so that no other ray's marks can hide a difference
    for k in range(len(cases)):
        assert_equals_the_restatement(pts[k:k + 1], slot[k:k + 1], origins, queries, **dict(UNIT, guard=0))


def test_default_grid_once(gpu):
    rng = np.random.default_rng(3)
    n = 3000
    origins = rng.uniform(-1.5, 1.5, (16, 3)).astype(np.float32)
    r, az = rng.uniform(0.5, 75.0, n), rng.uniform(-np.pi, np.pi, n)
    pts = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-3.5, 3.5, n)], axis=1).astype(np.float32)
    slot = rng.integers(0, 10, n).astype(np.uint8)
    queries = np.concatenate([pts, (pts * rng.uniform(0.1, 0.9, (n, 1))).astype(np.float32)])
    skip = (rng.random(len(queries)) < 0.1).astype(np.uint8)
    want, dyn = assert_equals_the_restatement(pts, slot, origins, queries, skip, pitch=4)
    assert want.shape == (30, 512, 512) and dyn.any()


def test_refusals_write_nothing(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.raymap import RaymapParams, map_bytes
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_raymap_params") == ctypes.sizeof(RaymapParams) == 40
    assert map_bytes(RaymapParams()) == 4 * 512 * 512 * 30 and map_bytes(RaymapParams(**SMALL)) == 4 * 256
    assert lib.himo_raymap_map_bytes(None) == 0
    pts, slot, origins, queries = rays(41, 300)

    def untouched(result, carve_refused=True):
        st, words, out, clean = result
        return clean and (not carve_refused or not words.any()) and all((o == FILL).all() for o in out)

    bad = [dict(voxel=0.0), dict(voxel=-0.2), dict(voxel=float("nan")), dict(x0=float("inf")), dict(z0=float("nan")), dict(nx=0), dict(ny=1025),
           dict(nz=65), dict(nz=0), dict(guard=-1), dict(guard=9), dict(min_votes=0), dict(min_votes=17), dict(voxel=1e-40)]
    for kw in bad:
        p = RaymapParams(**{**SMALL, **kw})
        assert map_bytes(p) == 0, kw
        res = launch(pts, slot, origins, queries, params=p)
        assert res[0][0] == _lib.ERR_INVALID_ARGUMENT and res[0][-1] == _lib.ERR_INVALID_ARGUMENT and untouched(res), kw
    assert map_bytes(RaymapParams(nx=1024, ny=1024, nz=17)) == 0 and map_bytes(RaymapParams(nx=1024, ny=1024, nz=16)) == 4 << 24
    p = RaymapParams(**SMALL)
    p.scale = 255.0                                               # not (float)(256.0 / voxel)
    res = launch(pts, slot, origins, queries, params=p)
    assert map_bytes(p) == 0 and res[0][0] == res[0][-1] == _lib.ERR_INVALID_ARGUMENT and untouched(res)
    for cp in (5, 2, 0):
        res = launch(pts, slot, origins, queries, call_pitch=cp, **SMALL)
        assert res[0][0] == res[0][-1] == _lib.ERR_INVALID_ARGUMENT and res[0][1] == 0 and untouched(res), cp
    # a slot byte of 16: found on the device.  The asynchronous call itself returns OK; the refusal is himo_raymap_status's answer,
    # once, and the call has marked nothing
    for where in (0, 150, 299):
        wrong = slot.copy()
        wrong[where] = 16
        st, words, out, clean = launch(pts, wrong, origins, queries, **SMALL)
        assert st == [0, _lib.ERR_INVALID_ARGUMENT, 0] and clean and not words.any(), where
        assert not out[0].any() and not out[1].any() and not out[2].any()           # (the query of the untouched map)
        assert lib.himo_raymap_status(_lib.stream_handle()) == 0
    # ... a refused call among good ones refuses only itself
    wrong = slot.copy()
    wrong[200] = 254
    st, words, _, clean = launch(pts, wrong, origins, queries, splits=3, **SMALL)
    want = ref.new_map(**SMALL)
    ref.carve(want, pts[:200], slot[:200], origins, **SMALL)
    assert st == [0, 0, 0, _lib.ERR_INVALID_ARGUMENT, 0] and clean and np.array_equal(words, want)
    # the Python entry points
    from himo_amd import raymap
    with pytest.raises(ValueError):
        raymap.new_map(RaymapParams(voxel=0.0))
    dev = torch.device("cuda", 0)
    grid = raymap.new_map(p := RaymapParams(**SMALL))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    raymap.carve(up(pts), up(wrong), up(origins), p, grid)
    with pytest.raises(ValueError, match="16..254"):
        raymap.status()
    assert not grid.any().item()
    raymap.carve(up(pts), up(slot), up(origins), p, grid)
    raymap.status()
    want = ref.new_map(**SMALL)
    ref.carve(want, pts, slot, origins, **SMALL)
    assert np.array_equal(grid.cpu().numpy().view(np.uint32), want)
    dyn, fv, hv = raymap.query(up(queries), p, grid)
    wd, wf, wh = ref.query(want, queries, **SMALL)
    assert np.array_equal(dyn.cpu().numpy().astype(bool), wd) and np.array_equal(fv.cpu().numpy(), wf) and np.array_equal(hv.cpu().numpy(), wh)


# ---- the toy scene ---------------------------------------------------------------------------------------------------------------
def test_dynamic_flags_and_cluster_labels_on_the_toy_scene(gpu):
    from himo_amd import raymap
    sweeps = [ray_cast_sweep(k) for k in range(11)]
    clouds, kinds, poses = [s[0] for s in sweeps], [s[1] for s in sweeps], [s[2] for s in sweeps]
    grounds = [k == GROUND for k in kinds]
    dyn, fv, hv, moved = raymap.dynamic_flags(clouds, poses, grounds, TARGET, return_moved=True)
    assert len(moved) == 10 and [tuple(m.shape) for m in moved] == [(len(clouds[k]), 3) for k in ref.neighbours(TARGET, 11)]
    wd, wf, wh = toy_flags(clouds, kinds, poses, moved=[m.cpu().numpy() for m in moved])
    assert np.array_equal(dyn.cpu().numpy().astype(bool), wd) and np.array_equal(fv.cpu().numpy(), wf) and np.array_equal(hv.cpu().numpy(), wh)
    kind = kinds[TARGET]
    assert wd[kind == 2].mean() >= 0.80 and wd[kind == 1].mean() <= 0.10
    labels, ids = raymap.cluster_labels(clouds[TARGET], grounds[TARGET], dyn, return_ids=True)
    labels, ids = labels.cpu().numpy(), ids.cpu().numpy()
    assert labels.dtype == np.int32 and np.array_equal(labels, ref.cluster_labels(ids, wd))
    assert set(labels[kind == 2].tolist()) == {1} and (labels[kind != 2] == 0).all()
    # a scene of one sweep has no neighbours: nothing is dynamic
    alone = raymap.dynamic_flags(clouds[:1], poses[:1], grounds[:1], 0)
    assert not alone[0].any().item() and not alone[1].any().item()
    with pytest.raises(ValueError):
        raymap.dynamic_flags(clouds, poses, grounds, TARGET, window=9)


# ---- the program -------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(gpu, tmp_path, capsys):
    from himo_amd import h5lite, raymap
    from himo_amd.dataset import open_dataset
    from himo_amd.seflow import spec
    from himo_amd.seflow.fit import fit, train_fields
    from himo_amd.synthetic import make_scene, write_h5_scenes
    root = tmp_path / "scenes"
    root.mkdir()
    scenes = [make_scene(80 + s, 12, n_points=3000, scene_id=f"rm{s}", cloud="rings") for s in range(2)]
    write_h5_scenes(root, scenes)
    done = raymap.main(str(root))
    printed = capsys.readouterr().out
    assert sorted(done) == ["rm0", "rm1"] and all(s["sweeps"] == 12 and s["points"] == 36_000 for s in done.values())
    assert printed.count("sweeps/s") == 2
    with pytest.raises(FileExistsError):
        raymap.main(str(root))
    with pytest.raises(FileExistsError):
        raymap.main(str(root), key="other")                       # the flags are there already
    again = raymap.main(str(root), overwrite=True)
    assert {k: {n: v for n, v in s.items() if n != "seconds"} for k, s in again.items()} == \
           {k: {n: v for n, v in s.items() if n != "seconds"} for k, s in done.items()}
    for frames in scenes:
        with h5lite.File(root / f"{frames[0]['scene_id']}.h5") as f:
            for fr in frames:
                g = f[str(fr["timestamp"])]
                lab, dyn = g["ray_label"], g["ray_dynamic"]
                assert lab.dtype == np.int32 and dyn.dtype == np.uint8 and lab.shape == dyn.shape == (3000,)
                lab, dyn = lab[:], dyn[:]
                assert lab.min() >= 0 and set(np.unique(dyn)) <= {0, 1} and not dyn[fr["gm0"]].any() and not lab[fr["gm0"]].any()
    # one sweep's flags against the restatement fed the same moved points
    clouds, poses, grounds = [fr["pc0"] for fr in scenes[0]], [fr["pose0"] for fr in scenes[0]], [fr["gm0"] for fr in scenes[0]]
    dyn, fv, hv, moved = raymap.dynamic_flags(clouds, poses, grounds, 1, return_moved=True)
    origins = np.zeros((16, 3), np.float32)
    for s, k in enumerate(ref.neighbours(1, 12)):
        origins[s] = ref.relative_pose(poses[1], poses[k])[:3, 3]
    wd, wf, wh = ref.dynamic_flags(clouds[1][:, :3], grounds[1], [m.cpu().numpy() for m in moved], origins)
    assert len(moved) == 6 and np.array_equal(dyn.cpu().numpy().astype(bool), wd) and np.array_equal(fv.cpu().numpy(), wf)
    with h5lite.File(root / "rm0.h5") as f:
        assert np.array_equal(f[str(scenes[0][1]["timestamp"])]["ray_dynamic"][:].astype(bool), wd)
    # the loader serves the labels of both sweeps of a pair, and the training loop takes a step on them
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # (the last sweep of a scene has no successor)
        ds = open_dataset(root, fields=train_fields("ray_label"), zero_copy=True)
    try:
        f0 = ds[0]
        assert "ray_label" in f0 and "ray_label_next" in f0 and len(f0["ray_label_next"]) == len(f0["pc1"])
        out = fit(ds, spec.init_params(3), epochs=1, batch_size=2, max_points=3000, device=gpu, log=None, ssl_label="ray_label", max_steps=1)
    finally:
        ds.close()
    assert out["history"][-1]["steps"] == 1 and np.isfinite(out["history"][-1]["train_loss"])
    # a scene without ground masks is refused by name
    bare = tmp_path / "bare"
    bare.mkdir()
    tree = {str(fr["timestamp"]): {"lidar": fr["pc0"], "pose": fr["pose0"]} for fr in scenes[0][:3]}
    h5lite.write_file(bare / "rm0.h5", tree)
    with open(bare / "index_total.pkl", "wb") as fh:
        pickle.dump([["rm0", ts] for ts in tree], fh)
    with pytest.raises(KeyError, match="himo_amd.ground_seg"):
        raymap.main(str(bare))
