"""The ICP-Flow baseline without a GPU: the numpy restatement of "cluster-rigid ICP, v1" (tests/icpflow_ref.py) on hand-derived
scenes, the vote's edge cases, the failure and rejection paths, the host side of the program, and the soundness of every seeded input
the GPU tests use (their discrete decisions have margins, so a flip on the device would be a bug and not a rounding accident)."""
import ctypes
import pickle
import re

import numpy as np
import pytest

import icpflow_ref as ref
from conftest import REPO

f32 = np.float32
HAND = dict(eps=ref.HAND_EPS, min_pts=ref.HAND_MIN_PTS)


# ---- 1. hand-derived recovery ---------------------------------------------------------------------------------------------------------
def test_yaw_and_translation_are_recovered():
    pc0, pc1, g0, g1, P0, P1, disp = ref.hand_scene(5.0, (2.0, 0.5, 0.1))
    r = ref.fit(pc0, pc1, g0, g1, P0, P1, **HAND)
    assert r["labels"][:29].tolist() == [1] * 29 and r["labels"][29:].tolist() == [2] * 29
    assert r["status"].tolist() == [[ref.ACCEPTED, 29, 8, 2], [ref.ACCEPTED, 29, 0, 0]]
    want = np.array([np.cos(np.deg2rad(5.0)), np.sin(np.deg2rad(5.0)), 2.0, 0.5, 0.1])
    assert np.abs(r["T"][0] - want).max() <= 1e-6, np.abs(r["T"][0] - want).max()
    assert np.abs(r["T"][1] - [1, 0, 0, 0, 0]).max() <= 1e-6
    assert np.abs(r["flow"][:29].astype(np.float64) - disp).max() <= 1e-4
    assert np.abs(r["flow"][29:]).max() <= 1e-4                    # the far static cluster, copied unchanged
    assert r["margins"].ok(), r["margins"]


def test_pure_translation_of_the_top_speed_bucket():
    pc0, pc1, g0, g1, P0, P1, disp = ref.hand_scene(0.0, (3.5, 0.0, 0.0))
    r = ref.fit(pc0, pc1, g0, g1, P0, P1, **HAND)
    assert r["status"].tolist() == [[ref.ACCEPTED, 29, 14, 0], [ref.ACCEPTED, 29, 0, 0]]
    assert np.abs(r["T"][0] - [1, 0, 3.5, 0, 0]).max() <= 1e-6
    assert np.abs(r["flow"][:29].astype(np.float64) - disp).max() <= 1e-4


# ---- 2. vote edge cases ---------------------------------------------------------------------------------------------------------------
def _one_vote(d, **kw):
    """the (kx, ky) bins one pair at offset ``d`` votes for, as a list"""
    counts, peaks, _ = ref.vote(np.zeros((1, 3), f32), [1], 1, np.asarray([d], f32), **kw)
    half = ref.params(**kw)["half"]
    ky, kx = np.nonzero(counts[0])
    return [(int(x) - half, int(y) - half) for x, y in zip(kx, ky)], peaks[0].tolist()


def test_half_bin_boundaries_round_half_to_even():
    assert _one_vote((0.125, 0.375, 0))[0] == [(0, 2)]             # 0.5 -> 0, 1.5 -> 2
    assert _one_vote((0.625, -0.125, 0))[0] == [(2, 0)]            # 2.5 -> 2, -0.5 -> -0
    assert _one_vote((0.875, -0.375, 0))[0] == [(4, -2)]           # 3.5 -> 4, -1.5 -> -2


def test_the_outermost_bin_votes_and_the_next_does_not():
    assert _one_vote((4.0, -4.0, 0))[0] == [(16, -16)]
    assert _one_vote((4.25, 0, 0))[0] == [] and _one_vote((0, -4.25, 0))[0] == []
    assert _one_vote((4.125, 0, 0))[0] == [(16, 0)]                # 16.5 rounds to 16: still inside
    assert _one_vote((0.25, 0, 0), half=1)[0] == [(1, 0)] and _one_vote((0.5, 0, 0), half=1)[0] == []


def test_z_gate_is_inclusive():
    assert _one_vote((0.5, 0.5, 1.0))[0] == [(2, 2)] and _one_vote((0.5, 0.5, -1.0))[0] == [(2, 2)]
    assert _one_vote((0.5, 0.5, float(np.nextafter(f32(1.0), f32(2.0)))))[0] == []


def test_ties_go_to_the_bin_nearer_zero_then_the_lower_ky_kx():
    pts = np.zeros((1, 3), f32)
    two = np.array([[0.75, 0.5, 0], [-0.25, 0.25, 0]], f32)       # bins (3, 2) and (-1, 1): one vote each
    assert ref.vote(pts, [1], 1, two)[1][0].tolist() == [-1, 1]
    ring = np.array([[0.25, 0, 0], [-0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0]], f32)      # four bins at distance 1
    counts, peaks, unique = ref.vote(pts, [1], 1, ring)
    assert peaks[0].tolist() == [0, -1] and not unique[0]          # the lowest ky, then the lowest kx
    assert ref.vote(pts, [1], 1, np.concatenate([ring, ring[:1]]))[1][0].tolist() == [1, 0]


def test_a_cluster_without_votes_takes_zero():
    counts, peaks, unique = ref.vote(np.zeros((3, 3), f32), [1, 1, 2], 3, np.array([[30.0, 0, 0]], f32))
    assert counts.sum() == 0 and peaks.tolist() == [[0, 0]] * 3 and unique.all()
    assert ref.vote(np.zeros((2, 3), f32), [1, 1], 1, np.zeros((0, 3), f32))[1].tolist() == [[0, 0]]


# ---- 3. failure and rejection ---------------------------------------------------------------------------------------------------------
def test_a_cluster_whose_target_is_absent_fails_and_keeps_the_ego_flow_bit_for_bit():
    pc0, pc1, g0, g1, _, _, _ = ref.hand_scene(5.0, (2.0, 0.5, 0.1))
    pose1 = ref.yaw_pose(1.5, (0.8, -0.1, 0.0))
    far = pc1[29:].astype(np.float64)
    inv1 = np.linalg.inv(pose1)
    pc1 = (far @ inv1[:3, :3].T + inv1[:3, 3]).astype(f32)         # only the static cluster, seen from pose1
    r = ref.fit(pc0, pc1, g0, np.zeros(len(pc1), bool), np.eye(4), pose1, **HAND)
    assert r["status"][0].tolist() == [ref.FAILED, 0, 0, 0] and r["status"][1, 0] == ref.ACCEPTED
    assert r["flow"][:29].tobytes() == r["ego_flow"][:29].tobytes() and np.abs(r["ego_flow"][:29]).max() > 0.5
    assert np.abs(r["flow"][29:] - r["ego_flow"][29:]).max() <= 1e-4       # the static cluster's fit is the identity to rounding


@pytest.mark.parametrize("kept, state", [(15, ref.ACCEPTED), (14, ref.REJECTED)])
def test_half_the_target_removed_sits_on_either_side_of_min_ratio(kept, state):
    """29 points; a kept target point makes exactly one inlier (the others are 0.6 m from their neighbours' targets but max_dist is
    0.25 here): 15 / 29 = 0.517 is accepted, 14 / 29 = 0.483 rejected"""
    pc0, pc1, g0, g1, P0, P1, _ = ref.hand_scene(0.0, (1.0, 0.25, 0.0))
    pc1 = np.concatenate([pc1[29 - kept:29], pc1[29:]])         # (the last rows: the lattice's alias shifts find fewer partners)
    r = ref.fit(pc0, pc1, g0, np.zeros(len(pc1), bool), P0, P1, max_dist=0.25, **HAND)
    assert r["status"][0].tolist() == [state, kept, 4, 1]
    moved = np.abs(r["flow"][:29] - [1.0, 0.25, 0.0]).max() <= 1e-4
    assert moved == (state == ref.ACCEPTED) and (state == ref.ACCEPTED or not r["flow"][:29].any())


@pytest.mark.parametrize("kept, state", [(8, ref.ACCEPTED), (7, ref.FAILED)])
def test_min_inliers_and_one_less(kept, state):
    pc0, pc1, g0, g1, P0, P1, _ = ref.hand_scene(0.0, (1.0, 0.25, 0.0))
    pc1 = np.concatenate([pc1[29 - kept:29], pc1[29:]])         # (the last rows: the lattice's alias shifts find fewer partners)
    r = ref.fit(pc0, pc1, g0, np.zeros(len(pc1), bool), P0, P1, max_dist=0.25, min_ratio=0.2, **HAND)
    assert r["status"][0].tolist() == [state, kept, 4, 1]
    assert (np.abs(r["flow"][:29] - [1.0, 0.25, 0.0]).max() <= 1e-4) if state == ref.ACCEPTED else not r["flow"][:29].any()


# ---- 4. host side ---------------------------------------------------------------------------------------------------------------------
def test_params_refusals_and_the_struct_mirror():
    from himo_amd import _lib
    from himo_amd.icpflow import IcpParams, _CParams
    p = IcpParams()
    assert {k: getattr(p, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    for bad in (dict(bin=0.0), dict(bin=-0.25), dict(bin=float("nan")), dict(z_gate=float("inf")), dict(max_dist=0), dict(min_ratio=-1.0),
                dict(half=0), dict(half=65), dict(min_inliers=0), dict(iters=0), dict(iters=2.5), dict(bin=1e-60), dict(max_dist=1e60)):
        with pytest.raises(ValueError):
            IcpParams(**bad)
    assert IcpParams(half=64).half == 64
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_icp_params") == ctypes.sizeof(_CParams) == 28
    c = p.c_struct()
    assert (c.bin, c.half, c.z_gate, c.max_dist, c.min_inliers, c.min_ratio, c.iters) == (0.25, 16, 1.0, 1.0, 8, 0.5, 10)
    assert lib.himo_icp_workspace_bytes(1000, 7) > 0 and lib.himo_icp_workspace_bytes(-1, 7) == 0 and lib.himo_icp_workspace_bytes(10, -1) == 0


def test_exports_are_declared_in_the_header_and_bound():
    from himo_amd import _lib
    header = (REPO / "include" / "himo_amd.h").read_text()
    for name in ("himo_icp_workspace_bytes", "himo_icp_vote", "himo_icp_step", "himo_icp_apply"):
        m = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert m, f"include/himo_amd.h does not declare {name}"
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert "cluster-rigid ICP, v1" in header and "FLAGS_icpflow := -ffp-contract=off" in (REPO / "himo_amd" / "csrc" / "Makefile").read_text()


def test_parity_is_said_to_be_unpinned_everywhere():
    from himo_amd import icpflow
    for words in ("cluster-rigid ICP, v1", "PARITY UNPINNED", "round half to even", "kx^2 + ky^2", "min_ratio", "bit for bit"):
        assert words in icpflow.__doc__, words
    assert "PARITY UNPINNED" in (REPO / "include" / "himo_amd.h").read_text().split("ICP-Flow baseline")[1][:1200]
    assert "PARITY UNPINNED" in (REPO / "himo_amd" / "csrc" / "icpflow.hip").read_text()[:600]
    design = (REPO / "DESIGN.md").read_text()
    assert design.count("icpflow") >= 2 and "parity unpinned" in design.lower()


def test_save_names_the_ground_segmenter_when_masks_are_missing(tmp_path):
    from himo_amd import h5lite, save
    from himo_amd.synthetic import make_scene
    tree = {}
    for f in make_scene(5, 3, n_points=500, scene_id="s0"):
        tree[str(f["timestamp"])] = {"lidar": f["pc0"], "lidar_dt": f["lidar_dt"], "pose": f["pose0"]}
    h5lite.write_file(tmp_path / "s0.h5", tree)
    with open(tmp_path / "index_total.pkl", "wb") as fh:
        pickle.dump([["s0", ts] for ts in sorted(tree)], fh)
    with pytest.raises(KeyError, match="python -m himo_amd.ground_seg"):
        save.main(dataset_path=str(tmp_path), model="icpflow")


def test_unknown_model_text_lists_icpflow():
    from himo_amd import save
    with pytest.raises(ValueError, match="icpflow"):
        save.main(dataset_path="nowhere", model="nsfp")


def test_nothing_in_the_package_imports_the_checker():
    for p in (REPO / "himo_amd").rglob("*.py"):
        assert not re.search(r"^\s*(import|from)\s+\S*icpflow_ref", p.read_text(), re.M), p


# ---- 5. the GPU tests' seeded inputs are sound ----------------------------------------------------------------------------------------
SEED, EGO = 3, ref.yaw_pose(2.0, (3.0, 0.2, 0.0))


@pytest.mark.parametrize("pose1", [None, EGO], ids=["identity", "ego"])
def test_seeded_pair_has_margins(pose1):
    r = ref.fit(*ref.seeded_pair(SEED, 3000, 12, pose1))
    mg = r["margins"]
    print(f"\nseeded pair: {len(r['status'])} clusters, states {np.bincount(r['status'][:, 0], minlength=3).tolist()}, {mg}")
    assert len(r["status"]) >= 12 and mg.nn_gap >= 1e-4 and mg.dist >= 1e-4 and mg.count >= 1 and mg.ratio >= 1e-4 and mg.peaks_unique
    moving = np.abs(r["T"][:, 2:4]).max(1) > 0.5
    assert moving.sum() >= 6 and (r["status"][:, 0] == ref.ACCEPTED).sum() >= 12


def test_hand_scenes_have_margins():
    for yaw, t in ((5.0, (2.0, 0.5, 0.1)), (0.0, (3.5, 0.0, 0.0))):
        pc0, pc1, g0, g1, P0, P1, _ = ref.hand_scene(yaw, t)
        assert ref.fit(pc0, pc1, g0, g1, P0, P1, **HAND)["margins"].ok()


VOTE_CASES = [(1, 1), (63, 2), (64, 1), (65, 3), (255, 4), (256, 1), (257, 5), (1000, 7)]


@pytest.mark.parametrize("n, C", VOTE_CASES)
def test_vote_cases_are_well_formed(n, C):
    pts, labels, tgt = ref.vote_case(n, n, C)
    assert len(pts) == n and labels.min() >= 1 and labels.max() <= C and (np.diff(labels) >= 0).all()
    counts, peaks, _ = ref.vote(pts, labels, C, tgt)
    assert counts.sum() > 0 or n < 8


@pytest.mark.parametrize("size", ref.STEP_SIZES)
def test_step_cases_have_margins_and_a_measured_bar(size):
    m, labels, tgt, d2, idx = ref.step_case(size)
    _, _, second = ref.nearest(m, tgt)
    max_d2 = f32(1.0)
    assert ((second - d2) / second).min() >= 1e-4 and (np.abs(d2 - max_d2) / max_d2).min() >= 1e-4
    n_in = int((d2[:size] <= max_d2).sum())
    assert abs(n_in - 8) >= 1 or size == 8
    s = ref.step_spread(m, labels, 2, tgt, d2, idx)
    print(f"\nstep case {size}: inliers {n_in}, spread s = {s:.2e}, bar = {max(16 * s, 1e-12):.2e}")
    assert s < 1e-12 / 16                                          # the floor is the bar for every case (table in icpflow_ref.py)


def test_host_side_refusals_need_no_device():
    """every refusal is decided on the host before anything is launched: the same calls answer without a GPU"""
    from himo_amd import _lib
    lib = _lib.load()
    from himo_amd.icpflow import IcpParams
    keep = IcpParams().c_struct()
    p = ctypes.addressof(keep)
    off = np.int64([0, 5, 9])
    fake = 1 << 20                                                  # a non-NULL, aligned address that is never dereferenced
    vote = lambda n=9, pitch=3, C=2, h=off.ctypes.data, nt=4, ws=fake, wb=1 << 30, prm=p: lib.himo_icp_vote(
        n, fake, pitch, C, h, fake, nt, fake, prm, fake, fake, fake, fake, ws, wb, None)
    INV, WS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_WORKSPACE
    assert [vote(pitch=2), vote(pitch=5), vote(n=-1), vote(nt=-1), vote(C=-1), vote(n=10), vote(h=None), vote(prm=None)] == [INV] * 8
    assert vote(h=np.int64([0, 6, 5]).ctypes.data, n=5) == INV and vote(h=np.int64([1, 5, 9]).ctypes.data) == INV
    assert [vote(ws=None), vote(wb=16), vote(ws=fake + 8)] == [WS] * 3
    assert vote(n=0, h=np.int64([0, 0, 0]).ctypes.data) == _lib.OK and vote(C=0, n=0) == _lib.OK
    step = lambda n=9, C=2, h=off.ctypes.data, wb=1 << 30: lib.himo_icp_step(n, fake, C, h, fake, 4, fake, fake, fake, p, 0, fake, fake, None, fake, wb, None)
    assert [step(n=-1), step(C=-1), step(n=8), step(h=None)] == [INV] * 4 and step(wb=16) == WS and step(C=0, n=0) == _lib.OK
    apply = lambda n=9, pitch=3, mode=0, bp=3, out=fake: lib.himo_icp_apply(n, fake, pitch, fake, 2, fake, fake, mode, fake, bp, out, None)
    assert [apply(pitch=2), apply(n=-1), apply(mode=2), apply(mode=1, bp=5), apply(out=None)] == [INV] * 5 and apply(n=0) == _lib.OK
