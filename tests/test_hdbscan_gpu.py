"""HDBSCAN, v1 on the GPU (himo_amd/seflow/ssl_label.py::hdbscan, csrc/hdbscan.hip) against the numpy restatement of the rule
(tests/hdbscan_ref.py): the squared core distances bit for bit, the minimum spanning tree as a set of (lo, hi) with bit-equal
weights, and the labels; then the programs that take ``--cluster hdbscan``, each against a host restatement that swaps only the
clustering call.  PARITY UNPINNED vs the reference (its generator is absent); tests/test_hdbscan_cpu.py holds the rule to sklearn."""
import numpy as np
import pytest
import torch

import hdbscan_ref as ref

pytestmark = pytest.mark.gpu

_REF = {}


def want_of(name, x, m, k, skip=None):
    """the restatement of a named case, computed once"""
    if name not in _REF:
        _REF[name] = ref.hdbscan(x[:, :3], m, k, skip)
    return _REF[name]


def cloud(seed, n, box=40.0, n_blobs=6):
    """n points: blobs of very different densities (a LiDAR sweep's near and far objects) plus uniform clutter, shuffled"""
    rng = np.random.default_rng(seed)
    sizes = np.maximum((n * 0.8 * rng.dirichlet(np.ones(n_blobs))).astype(int), 1)
    parts = [rng.normal(rng.uniform(-box, box, 3) * [1, 1, .05], rng.uniform(.1, 1.2), (int(s), 3)) for s in sizes]
    parts.append(rng.uniform([-box, -box, -2.0], [box, box, 2.0], (n - int(sizes.sum()), 3)))
    x = np.concatenate(parts).astype(np.float32)
    return x[rng.permutation(n)]


def lattice():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def duplicates():
    rng = np.random.default_rng(5)
    return np.concatenate([np.tile(np.float32([[3.0, -2.0, 0.5]]), (50, 1)), rng.normal([-4.0, 4.0, 0.0], 0.3, (30, 3)).astype(np.float32)])


def run(gpu, x, m, k, skip=None):
    from himo_amd.seflow.ssl_label import hdbscan
    sk = None if skip is None else torch.from_numpy(skip).to(gpu)
    labels, count, tree = hdbscan(torch.from_numpy(x).to(gpu), m, k, skip=sk, return_tree=True)
    return labels.cpu().numpy(), int(count.item()), tree


def check(gpu, name, x, m, k, skip=None):
    want = want_of(name, x, m, k, skip)
    labels, count, tree = run(gpu, x, m, k, skip)
    assert labels.dtype == np.int32 and labels.shape == (len(x),)
    assert np.array_equal(tree["index"], want["index"])
    got_c2 = tree["core2"].cpu().numpy()
    assert np.array_equal(got_c2.view(np.uint32), want["core2"].view(np.uint32)), np.flatnonzero(got_c2 != want["core2"])[:10]
    e = tree["edges"]
    e = e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))] if len(e) else e.reshape(0, 3)
    assert e.shape == want["edges"].shape and np.array_equal(e, want["edges"]), (e.shape, want["edges"].shape)
    assert np.array_equal(labels, want["labels"]) and count == want["count"]
    return want, tree


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_fewer_points_than_anything_needs(gpu, p):
    """|P| of 1, 2, k - 1 and k (k = 4), among skipped rows"""
    x = cloud(11, 40)
    skip = np.ones(40, dtype=bool); skip[[5, 17, 18, 33][:p]] = False
    want, tree = check(gpu, f"few{p}", x, 2, 4, skip)
    assert len(tree["edges"]) == (3 if p == 4 else 0) and (want["count"] == 0 or p == 4)
    if p == 2:
        want, tree = check(gpu, "two_k1", x, 2, 1, skip)            # two points, k = 1: one edge, still no cluster (the root is never one)
        assert len(tree["edges"]) == 1


def test_no_points_at_all(gpu):
    labels, count, tree = run(gpu, np.zeros((0, 3), np.float32), 5, 5)
    assert labels.shape == (0,) and count == 0 and len(tree["edges"]) == 0
    check(gpu, "all_skipped", cloud(12, 30), 5, 5, np.ones(30, dtype=bool))


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_either_side_of_a_tile_and_of_a_block(gpu, n):
    want, tree = check(gpu, f"n{n}", cloud(n, n), 10, 4)
    assert want["count"] >= 2 and 1 <= tree["rounds"] <= int(np.ceil(np.log2(n)))


def test_lattice_where_every_weight_ties(gpu):
    want, _ = check(gpu, "lattice", lattice(), 10, 4)
    assert len(np.unique(want["edges"][:, 0])) == 1


def test_duplicates_and_zero_distances(gpu):
    want, _ = check(gpu, "dup", duplicates(), 10, 5)
    assert want["count"] == 2 and (want["edges"][:, 0] == 0).sum() == 49


@pytest.mark.parametrize("k", [1, 4, 20, 32])
def test_core_neighbour_counts(gpu, k):
    want, _ = check(gpu, f"k{k}", cloud(70 + k, 300), 12, k)
    assert want["count"] >= 1
    if k == 1:
        assert not want["core2"][np.isfinite(want["core2"])].any()


def test_pitch_four_with_skipped_and_nan_rows(gpu):
    """the original indices are not the compacted ones"""
    rng = np.random.default_rng(3)
    x = np.concatenate([cloud(21, 400), rng.uniform(0, 1, (400, 1)).astype(np.float32)], axis=1)
    skip = rng.uniform(size=400) < 0.3
    x[rng.choice(400, 25, replace=False), rng.integers(0, 3, 25)] = np.nan
    want, tree = check(gpu, "pitch4", x, 8, 4, skip)
    assert len(want["index"]) < 300 and want["count"] >= 2 and (want["labels"][skip] == 0).all()
    assert np.isinf(tree["core2"].cpu().numpy()[skip]).all()
    strided = torch.from_numpy(np.concatenate([x, x], axis=1)).to(gpu)[:, :4]         # row stride 8: no copy is made
    from himo_amd.seflow.ssl_label import hdbscan
    again, _ = hdbscan(strided, 8, 4, skip=torch.from_numpy(skip).to(gpu))
    assert np.array_equal(again.cpu().numpy(), want["labels"])


def test_one_huge_component_and_a_far_small_one(gpu):
    """two dense blobs 60 m apart and a 12-point group: the last rounds join few, very unequal components"""
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.normal([-30, 0, 0], 0.4, (300, 3)), rng.normal([30, 0, 0], 0.4, (280, 3)),
                        rng.normal([0, 25, 0], 0.8, (12, 3))]).astype(np.float32)
    x = x[rng.permutation(len(x))]
    want, _ = check(gpu, "far", x, 10, 5)
    assert want["count"] == 3


def test_points_outside_the_bev_grid(gpu):
    x = cloud(31, 300, box=200.0)
    x[:5] *= 40.0
    want, _ = check(gpu, "outside", x, 10, 4)
    assert np.abs(x[:, :2]).max() > 1000 and want["count"] >= 1


def test_many_blocks_and_the_full_number_of_rounds(gpu):
    x = cloud(4099, 4099, n_blobs=14)
    want, tree = check(gpu, "n4099", x, 20, 20)
    assert want["count"] >= 3 and 2 <= tree["rounds"] <= 13
    labels, count, again = run(gpu, x, 20, 20)                          # a pure function of the input (atomics inside, fixed result)
    assert np.array_equal(labels, want["labels"]) and again["rounds"] == tree["rounds"]


def test_refusals_launch_nothing(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import ssl_label
    x = torch.from_numpy(cloud(1, 64)).to(gpu)
    for m, k in ((1, 4), (5, 0), (5, 33)):
        with pytest.raises(ValueError):
            ssl_label.hdbscan(x, m, k)
    lib = _lib.load()
    assert lib.himo_hdbscan_workspace_bytes(-1, 8, 8) == 0 and lib.himo_hdbscan_workspace_bytes(64, 0, 8) == 0
    need = int(lib.himo_hdbscan_workspace_bytes(64, 8, 8))
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    out = torch.full((4 + 64 + 3 * 63,), -7, dtype=torch.int32, device=gpu)
    at = lambda w: out.data_ptr() + 4 * w
    call = lambda n=64, pitch=3, k=4, counts=at(0), wsp=ws.data_ptr(), nbytes=need: lib.himo_hdbscan_mst(
        n, x.data_ptr(), pitch, None, k, counts, at(4), None, at(68), wsp, nbytes, _lib.stream_handle())
    assert call(n=-1) == _lib.ERR_INVALID_ARGUMENT and call(pitch=2) == _lib.ERR_INVALID_ARGUMENT
    assert call(k=0) == _lib.ERR_INVALID_ARGUMENT and call(k=33) == _lib.ERR_INVALID_ARGUMENT and call(counts=None) == _lib.ERR_INVALID_ARGUMENT
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE and call(wsp=None) == _lib.ERR_WORKSPACE and call(wsp=ws.data_ptr() + 4) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (out == -7).all().item() and not ws.any().item()
    assert call() == _lib.OK


def test_dbscan_is_unchanged(gpu):
    """dbscan.hip now takes its union-find from the header hdbscan.hip shares: its labels still equal the oracle's"""
    import dbscan_oracle
    from himo_amd.seflow.ssl_label import dbscan
    rng = np.random.default_rng(4_000)                                  # the first case of tests/test_ssl_label_gpu.py
    sizes = rng.integers(5, 400, 12)
    parts = [rng.normal(rng.uniform(-45.0, 45.0, 3) * np.array([1, 1, 0.05]), 0.25 * rng.uniform(0.5, 2.0), (int(k), 3)) for k in sizes]
    noise = rng.uniform([-45.0, -45.0, -2.5], [45.0, 45.0, 2.5], (max(4_000 - int(sizes.sum()), 0), 3))
    pts = np.concatenate(parts + [noise]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    skip = np.random.default_rng(4_001).uniform(size=len(pts)) < 0.1
    got, k = dbscan(torch.from_numpy(pts).to(gpu), 0.5, 8, torch.from_numpy(skip).to(gpu))
    want = dbscan_oracle.dbscan(pts, 0.5, 8, skip)
    assert int(k.item()) == want.max() > 0 and np.array_equal(got.cpu().numpy(), want)


# ---- the programs ------------------------------------------------------------------------------------------------------------------
M, K = 10, 4                                                            # the programs' tiny scenes hold a 16- and a 20-point object


def grid_object(ny, nz, spacing, at, seed):
    """ny x nz returns on a plane facing the sensor, ``spacing`` apart with a few millimetres of noise"""
    gy, gz = np.meshgrid(np.arange(ny) * spacing, np.arange(nz) * spacing, indexing="ij")
    flat = np.stack([np.zeros(ny * nz), gy.ravel(), gz.ravel()], axis=1) + np.asarray(at, dtype=np.float64)
    return flat + np.random.default_rng(seed).normal(0, 0.004, flat.shape)


def ray_scene():
    """three sweeps from one standing sensor: a wall at x = 48 m in all of them; a DENSE object (8 x 8 returns 0.25 m apart) at 30 m and a
    SPARSE one (4 x 4 returns 0.8 m apart, wider than ssl_label.EPS) at 40 m, both somewhere else in the neighbour sweeps, so the
    neighbours' rays to the wall cross the places the target sweep (1) sees them at.  -> (clouds, poses, grounds, kind of every target
    row: 0 wall, 1 dense, 2 sparse)"""
    wy, wz = np.meshgrid(np.arange(-6.0, 6.0, 0.2), np.arange(-0.5, 3.2, 0.2), indexing="ij")
    clouds = []
    for t in range(3):
        wall = np.stack([np.full(wy.size, 48.0), wy.ravel(), wz.ravel()], axis=1) + np.random.default_rng(40 + t).normal(0, 0.004, (wy.size, 3))
        shift = 0.0 if t == 1 else 5.0
        dense = grid_object(8, 8, 0.25, (30.0, 1.0 + shift, 0.0), 50 + t)
        sparse = grid_object(4, 4, 0.8, (40.0, -4.0 - shift, 0.0), 60 + t)
        clouds.append(np.concatenate([wall, dense, sparse]).astype(np.float32))
    kind = np.concatenate([np.zeros(wy.size, int), np.ones(64, int), np.full(16, 2)])
    return clouds, [np.eye(4)] * 3, [np.zeros(len(c), dtype=bool) for c in clouds], kind


def test_raymap_program_with_hdbscan(gpu, tmp_path):
    """``python -m himo_amd.raymap --cluster hdbscan`` labels the sparse far object that DBSCAN leaves as noise; both runs equal the
    restatement of rule F with only the clustering call swapped; the default is DBSCAN, as before"""
    import raymap_ref
    from himo_amd import h5lite, raymap
    clouds, poses, grounds, kind = ray_scene()
    root = tmp_path / "scenes"
    root.mkdir()
    stamps = [str(1000 + t) for t in range(3)]
    h5lite.write_file(root / "toy.h5", {ts: {"lidar": c, "pose": p, "ground_mask": g} for ts, c, p, g in zip(stamps, clouds, poses, grounds)})
    raymap._cli(["--data_dir", str(root), "--window", "1", "--key", "hd_label", "--dynamic_key", "hd_dynamic", "--cluster", "hdbscan",
                 "--min_cluster_size", str(M), "--min_samples", str(K)])
    raymap._cli(["--data_dir", str(root), "--window", "1"])                                   # the default: DBSCAN
    raymap.main(str(root), window=1, key="db_label", dynamic_key="db_dynamic", cluster="dbscan")
    for bad in (["--cluster", "optics"], ["--cluster", "HDBSCAN"]):
        with pytest.raises(ValueError, match="one of dbscan, hdbscan"):
            raymap._cli(["--data_dir", str(root), "--overwrite"] + bad)
    with h5lite.File(root / "toy.h5") as f:
        g = f[stamps[1]]
        hd, default, db, dyn = g["hd_label"][:], g["ray_label"][:], g["db_label"][:], g["hd_dynamic"][:].astype(bool)
        assert np.array_equal(dyn, g["ray_dynamic"][:].astype(bool))
    assert dyn[kind == 1].mean() >= 0.8 and dyn[kind == 2].mean() >= 0.8 and dyn[kind == 0].mean() <= 0.05
    skip = raymap_ref.cluster_skip(clouds[1], grounds[1])
    want_db = raymap_ref.cluster_labels(raymap_ref.dbscan(clouds[1], skip=skip), dyn)
    want_hd = raymap_ref.cluster_labels(ref.hdbscan(clouds[1], M, K, skip)["labels"], dyn)
    assert np.array_equal(default, want_db) and np.array_equal(db, want_db) and np.array_equal(hd, want_hd)
    assert (db[kind == 2] == 0).all() and len(set(hd[kind == 2].tolist())) == 1 and hd[kind == 2][0] > 0     # the sparse far object
    assert len(set(db[kind == 1].tolist())) == 1 and db[kind == 1][0] > 0 and len(set(hd[kind == 1].tolist())) == 1 and hd[kind == 1][0] > 0
    assert (db[kind == 0] == 0).all() and (hd[kind == 0] == 0).all()


def test_icpflow_with_hdbscan(gpu, monkeypatch):
    """``IcpFlow(cluster="hdbscan")`` (``save --model icpflow --cluster hdbscan``) moves the sparse far object that DBSCAN leaves under
    the identity; both equal tests/icpflow_ref.py with only the clustering call swapped"""
    import icpflow_ref
    from himo_amd.icpflow import IcpFlow
    from himo_amd.seflow.ssl_label import _moved
    dense, sparse = grid_object(8, 8, 0.25, (12.0, 1.0, 0.2), 1), grid_object(5, 4, 0.8, (40.0, -4.0, 0.2), 2)
    pc0 = np.concatenate([dense, sparse]).astype(np.float32)
    pc1 = np.concatenate([dense + [0.5, 0.25, 0.0], sparse + [1.0, 0.5, 0.0]]).astype(np.float32)
    gm, eye = np.zeros(len(pc0), dtype=bool), np.eye(4)
    a = _moved(torch.from_numpy(pc0).to(gpu), eye).cpu().numpy()
    far = np.arange(len(pc0)) >= 64
    flows = {}
    for how in ("dbscan", "hdbscan"):
        icp = IcpFlow(gpu, cluster=how, min_cluster_size=M, min_samples=K) if how == "hdbscan" else IcpFlow(gpu)
        flow = icp.fit(pc0, pc1, gm, gm, eye, eye).cpu().numpy()
        with monkeypatch.context() as mp:
            if how == "hdbscan":
                mp.setattr(icpflow_ref, "dbscan", lambda pts, eps, min_pts, skip: ref.hdbscan(pts, M, K, skip)["labels"])
            want = icpflow_ref.fit(pc0, pc1, gm, gm, eye, eye, a=a)
        assert np.array_equal(icp.last_labels, want["labels"]) and np.array_equal(icp.last_status, want["status"])
        assert np.abs(flow - want["flow"]).max() <= 1e-4
        flows[how] = flow
    assert not flows["dbscan"][far].any()                                # noise under DBSCAN: the identity, and the poses are equal
    assert np.abs(flows["hdbscan"][far] - [1.0, 0.5, 0.0]).max() <= 0.02
    assert np.abs(flows["dbscan"][~far] - [0.5, 0.25, 0.0]).max() <= 0.02 and np.abs(flows["hdbscan"][~far] - [0.5, 0.25, 0.0]).max() <= 0.02
    with pytest.raises(ValueError, match="one of dbscan, hdbscan"):
        IcpFlow(gpu, cluster="optics")
    from himo_amd import save
    with pytest.raises(ValueError, match="cluster"):
        save.main(dataset_path="nowhere", model="icpflow", cluster="optics")


def test_auto_labels_takes_the_keyword(gpu):
    from himo_amd.seflow import ssl_label
    pc0, pc1, g0, g1, P0, P1 = __import__("icpflow_ref").seeded_pair(7, 1500, 6)
    a0, a1 = ssl_label.auto_labels(pc0, pc1, g0, g1, P0, P1)
    b0, b1 = ssl_label.auto_labels(pc0, pc1, g0, g1, P0, P1, cluster="dbscan")
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    h0, h1, top = ssl_label.auto_labels(pc0, pc1, g0, g1, P0, P1, cluster="hdbscan", min_cluster_size=M, min_samples=K, return_top=True)
    assert h0.shape == a0.shape and h0.dtype == torch.int32 and int(top.item()) == max(int(h0.max()), int(h1.max()))
    assert not h0[torch.from_numpy(g0).to(gpu)].any().item()
    with pytest.raises(ValueError, match="one of dbscan, hdbscan"):
        ssl_label.auto_labels(pc0, pc1, g0, g1, P0, P1, cluster="optics")
