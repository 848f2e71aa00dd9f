"""The cluster-rigid refinement without a GPU: the checker itself (tests/rigidrefine_ref.py, the numpy restatement of the rule in
``himo_amd/rigid_refine.py``) against an independent Kabsch and on the scene the rule was tried on, the margins of the seeded cases
that tests/test_rigid_refine_gpu.py holds the device to, and the host logic of the package (parameters, the program's refusals, the
struct mirror)."""
import ctypes

import numpy as np
import pytest

import icpflow_ref
import rigidrefine_ref as ref


def run(scene, **kw):
    return ref.refine(scene["pc0"], scene["flow"], scene["gm0"], scene["pose0"], scene["pose1"], scene["labels"], **kw)


def mpe(flow, scene, rows):
    return float(np.linalg.norm(flow[rows].astype(np.float64) - scene["true_flow"][rows], axis=1).mean())


# ---- (a) the closed form against an independent Kabsch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw, t", [(0.05, (1.3, -0.7, 0.08)), (-0.02, (-2.6, 3.1, -0.04)), (0.0, (0.5, 0.25, 0.0))])
def test_noise_free_cluster_gives_the_kabsch_transform(yaw, t):
    sc = ref.build_scene([dict(n=200, centre=(12.0, -7.0, 0.4), dims=(4.0, 2.0, 1.5), yaw=yaw, t=t)], seed=3, sigma=0.0)
    r = run(sc)
    assert r["status"][0, 0].tolist()[:2] == [ref.ACCEPTED, 200] and (r["claim"] == 1).all()
    q = (sc["pc0"][:, :3] + sc["flow"]).astype(np.float32)
    want = ref.kabsch_2d(r["a"], q)
    assert np.abs(r["transforms"][0, 0] - want).max() <= 1e-12
    assert np.abs(r["transforms"][0, 0, :2] - [np.cos(yaw), np.sin(yaw)]).max() <= 1e-5        # (float32 inputs)
    assert np.abs(r["flow"].astype(np.float64) - sc["true_flow"]).max() <= 1e-4


# ---- (b) the scene the rule was tried on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_static", [0, 200, 450])
def test_vehicle_alone_and_merged_with_static_points(n_static):
    sc = ref.vehicle_scene(n_static)
    r = run(sc)
    vehicle = sc["part"] == 0
    before, after = mpe(sc["flow"], sc, vehicle), mpe(r["flow"], sc, vehicle)
    print(f"\n{n_static} static points: vehicle MPE {before:.4f} m -> {after:.4f} m (ratio {after / before:.3f}); margins {r['margins']}")
    assert after <= 0.25 * before
    assert r["flow"][~vehicle].tobytes() == r["ego_flow"][~vehicle].tobytes()                   # every static row: a - pc0, bit for bit
    states = r["status"][0, :, 0].tolist()
    if n_static == 450:                                            # the static part wins the first vote
        assert states == [ref.STATIC, ref.ACCEPTED]
        assert r["status"][0, :, 1].tolist() == [450, 300]
    elif n_static == 200:
        assert states == [ref.ACCEPTED, ref.STATIC]
    else:
        assert states == [ref.ACCEPTED, ref.FAILED]
    assert r["margins"]["e2"] > 1e-6 and r["margins"]["static"] > 1e-6 and r["margins"]["ratio"] > 1e-6


# ---- (c) more parts than models ---------------------------------------------------------------------------------------------------------
def test_third_part_of_a_three_part_cluster_keeps_its_bytes():
    sc = ref.three_part_scene()
    r = run(sc, models=2)
    assert r["status"][0, :, 0].tolist() == [ref.ACCEPTED, ref.ACCEPTED]
    third = sc["part"] == 2
    assert (r["claim"][sc["part"] == 0] == 1).all() and (r["claim"][sc["part"] == 1] == 2).all() and (r["claim"][third] == 0).all()
    assert r["flow"][third].view(np.int32).tobytes() == sc["flow"][third].view(np.int32).tobytes()
    for k in (0, 1):
        assert mpe(r["flow"], sc, sc["part"] == k) < 0.5 * mpe(sc["flow"], sc, sc["part"] == k)
    r3 = run(sc, models=3, min_ratio=0.2)                           # ... and with a third model it is claimed too
    assert r3["status"][0, :, 0].tolist() == [ref.ACCEPTED] * 3 and (r3["claim"][third] == 3).all()


# ---- (d) the vote's tie rule ------------------------------------------------------------------------------------------------------------
def test_vote_ties_go_to_the_smaller_radius_then_the_lower_ky_kx():
    def rows(bins):
        a = np.zeros((len(bins), 3), np.float32)
        q = np.float32([[0.25 * kx, 0.25 * ky, 0.0] for kx, ky in bins])
        return a, q
    kx, ky, counts = ref.vote(*rows([(3, 0)] * 4 + [(0, -2)] * 4 + [(1, 1)] * 3))
    assert (kx, ky) == (0, -2) and counts.max() == 4               # equal counts: the smaller kx^2 + ky^2
    kx, ky, _ = ref.vote(*rows([(2, 1)] * 5 + [(-1, 2)] * 5 + [(1, -2)] * 5 + [(-2, -1)] * 5))
    assert (kx, ky) == (1, -2)                                     # equal radius: the lowest (ky, kx)
    kx, ky, _ = ref.vote(*rows([(2, 1)] * 5 + [(-1, 2)] * 5))
    assert (kx, ky) == (2, 1)
    assert ref.vote(*rows([(17, 0)] * 6 + [(0, -17)] * 2))[:2] == (0, 0)                        # outside the window: no votes
    assert ref.vote(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))[:2] == (0, 0)
    # half to even at the bin edges: 0.125 / 0.25 = 0.5 -> 0, 0.375 / 0.25 = 1.5 -> 2
    a, q = np.zeros((2, 3), np.float32), np.float32([[0.125, 0.375, 0], [0.125, 0.375, 0]])
    assert ref.vote(a, q)[:2] == (0, 2)


# ---- the seeded cases of the GPU test: constructed labels are DBSCAN's, decisions have margins ---------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_seeded_cases_have_margins_and_their_labels_are_the_clusterings(name):
    build, kw, ctor = ref.CASES[name]
    sc = build()
    r = run(sc, **kw)
    m = r["margins"]
    print(f"\n{name}: {len(sc['pc0'])} rows, {len(r['status'])} clusters, states {np.bincount(r['status'][:, :, 0].ravel(), minlength=5).tolist()}, margins {m}")
    assert m["e2"] > 1e-6 and m["static"] > 1e-6 and m["ratio"] > 1e-6 and m["count"] >= 1
    if ctor.get("cluster") == "hdbscan":
        import hdbscan_ref
        from himo_amd.seflow.ssl_label import HDB_MIN_CLUSTER, HDB_MIN_SAMPLES
        part = ref.participates(r["a"], sc["flow"], sc["gm0"])
        assert np.array_equal(hdbscan_ref.hdbscan(r["a"], HDB_MIN_CLUSTER, HDB_MIN_SAMPLES, skip=~part)["labels"], sc["labels"])
        return
    # every constructed cluster is one DBSCAN cluster on its own, and no two come within eps of each other
    eps, min_pts = ctor.get("eps", icpflow_ref.EPS), ctor.get("min_pts", icpflow_ref.MIN_PTS)
    a, labels = r["a"], sc["labels"]
    C = int(labels.max(initial=0))
    lo, hi = np.zeros((C, 3)), np.zeros((C, 3))
    for k in range(C):
        pts = a[labels == k + 1]
        assert (icpflow_ref.dbscan(pts, eps, min_pts) == 1).all(), f"cluster {k + 1} of {len(pts)} rows is not one DBSCAN cluster"
        lo[k], hi[k] = pts.min(0), pts.max(0)
    gap = np.maximum(lo[:, None, :] - hi[None, :, :], lo[None, :, :] - hi[:, None, :]).max(-1)
    gap[np.arange(C), np.arange(C)] = np.inf
    assert C == 0 or gap.min(initial=np.inf) > eps
    loose = a[(labels == 0) & ref.participates(a, sc["flow"], sc["gm0"])]
    assert len(loose) == 0                                        # every participating row is in a cluster: nothing else could join one


def test_seeded_cases_cover_what_they_are_there_for():
    r = run(ref.eight_scene())
    assert r["status"][0, 0].tolist()[:2] == [ref.ACCEPTED, 8]
    sc = ref.seven_scene()
    r = run(sc)
    assert r["status"][0].tolist() == [[ref.FAILED, 7, 2, 1], [ref.NOT_RUN, 0, 0, 0]] and r["flow"].tobytes() == sc["flow"].tobytes()
    sc = ref.sizes_scene()
    r = run(sc)
    assert np.bincount(sc["labels"])[1:8].tolist() == list(ref.SIZES) and len(r["status"]) == len(ref.SIZES) + ref.N_SMALL
    assert (r["status"][:, 0, 0] == ref.ACCEPTED).all() and not np.array_equal(r["a"], sc["pc0"][:, :3])
    sc = ref.merged_scene()
    r = run(sc)
    assert r["status"][:, :, 0].tolist() == [[ref.STATIC, ref.ACCEPTED], [ref.STATIC, ref.ACCEPTED], [ref.ACCEPTED, ref.ACCEPTED]]
    assert r["status"][:2, :, 1].tolist() == [[120, 180], [180, 120]]          # (the static part's votes share a bin, the turning part's spread: static first, both times)
    sc = ref.static_scene()
    r = run(sc)
    assert r["status"][0, 0, 0] == ref.STATIC and r["flow"].tobytes() == r["ego_flow"].tobytes() and r["flow"].tobytes() != sc["flow"].tobytes()
    sc = ref.passthrough_scene()
    r = run(sc)
    assert r["status"][:, 0, 0].tolist() == [ref.ACCEPTED, ref.FAILED] and r["status"][1, 0].tolist() == [ref.FAILED, 0, 0, 0]
    kept = r["claim"] == 0
    assert kept.sum() == 4 + 60 + 80 + 90 and r["flow"][kept].view(np.int32).tobytes() == sc["flow"][kept].view(np.int32).tobytes()


# ---- (e) the parameters -------------------------------------------------------------------------------------------------------------------
def test_rigid_params_refuse_what_the_rule_does_not_admit():
    from himo_amd.rigid_refine import RigidParams
    p = RigidParams()
    assert {k: getattr(p, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    for bad in (dict(bin=0.0), dict(bin=-0.25), dict(tol=float("nan")), dict(tol=float("inf")), dict(min_ratio=0), dict(static_disp=1e-60),
                dict(static_disp="0.05"), dict(half=0), dict(half=65), dict(half=16.0), dict(iters=0), dict(min_inliers=0), dict(models=0),
                dict(models=5), dict(models=True), dict(bin=1e60)):
        with pytest.raises(ValueError, match="RigidParams"):
            RigidParams(**bad)
    ok = RigidParams(half=64, models=4, tol=0.1, iters=1)
    c = ok.c_struct()
    assert (c.half, c.models, c.iters, c.min_inliers) == (64, 4, 1, 8) and c.tol == np.float32(0.1) and c.static_disp == np.float32(0.05)
    with pytest.raises(Exception):
        ok.tol = 0.2                                               # frozen


# ---- (g) the struct mirror ------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_has_the_c_struct_size():
    from himo_amd import _lib
    from himo_amd.rigid_refine import _CParams
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_rigid_params") == ctypes.sizeof(_CParams) == 32
    assert lib.himo_rigid_refine_workspace_bytes(1000, 10, 16, 2) >= 2 * 12000 + 1000
    assert lib.himo_rigid_refine_workspace_bytes(1000, 10, 64, 2) >= 10 * 129 * 129 * 4          # the counters that do not fit the LDS
    for bad in ((-1, 1, 16, 2), (10, -1, 16, 2), (10, 1, 0, 2), (10, 1, 65, 2), (10, 1, 16, 0), (10, 1, 16, 5), (2 ** 31, 1, 16, 2)):
        assert lib.himo_rigid_refine_workspace_bytes(*bad) == 0, bad


# ---- (f) the program's refusals: all before the GPU is asked for ----------------------------------------------------------------------------
def _npz_dataset(root, with_gm0=True, extra=()):
    from himo_amd.dataset import NpzDataset
    frames = []
    for k in range(2):
        sc = ref.static_scene(seed=80 + k)
        f = {"scene_id": "s0", "timestamp": 1000 + k, "pc0": sc["pc0"], "pose0": sc["pose0"], "pose1": sc["pose1"], "noisy": sc["flow"]}
        if with_gm0:
            f["gm0"] = sc["gm0"]
        for name in extra:
            f[name] = sc["flow"]
        frames.append(f)
    NpzDataset.write(root, frames)
    return frames


def test_program_refusals_come_before_the_gpu(tmp_path, monkeypatch):
    from himo_amd import _lib, rigid_refine

    def no_gpu():
        raise AssertionError("the program asked for the GPU before it refused")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    plain = tmp_path / "plain"
    _npz_dataset(plain)
    with pytest.raises(ValueError, match="raw"):
        rigid_refine.main(str(plain), "raw")
    with pytest.raises(ValueError, match="key of its own"):
        rigid_refine.main(str(plain), "noisy", out_name="noisy")
    with pytest.raises(ValueError, match="raw"):
        rigid_refine.main(str(plain), "noisy", out_name="raw")
    with pytest.raises(ValueError, match="raw"):
        rigid_refine._cli(["--data_dir", str(plain), "--res_name", "raw"])
    with pytest.raises(ValueError, match="RigidParams.models"):
        rigid_refine._cli(["--data_dir", str(plain), "--res_name", "noisy", "--models", "5"])
    bare = tmp_path / "bare"
    _npz_dataset(bare, with_gm0=False)
    with pytest.raises(KeyError, match="himo_amd.ground_seg"):
        rigid_refine.main(str(bare), "noisy")
    done = tmp_path / "done"
    _npz_dataset(done, extra=("noisy_rigid", "other"))
    with pytest.raises(FileExistsError, match="--overwrite"):
        rigid_refine.main(str(done), "noisy")
    with pytest.raises(FileExistsError, match="--overwrite"):
        rigid_refine._cli(["--data_dir", str(done), "--res_name", "noisy", "--out_name", "other"])
    # nothing was written by a refused run
    with np.load(done / "s0" / "1000.npz") as z:
        assert sorted(z.files) == sorted(["pc0", "pose0", "pose1", "noisy", "gm0", "noisy_rigid", "other"])
    # a result nobody stored: every sweep is passed over, nothing is launched
    totals = rigid_refine.main(str(plain), "absent")
    assert totals["sweeps"] == 0 and totals["skipped"] == 2


def test_without_a_gpu_it_raises(monkeypatch):
    import torch
    from himo_amd.rigid_refine import RigidRefine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RigidRefine()
