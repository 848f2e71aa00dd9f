"""The ground segmenter without a GPU: the checker ``tests/groundseg_ref.py`` (the numpy restatement of "ray ground filter, v1")
on scenes whose answer follows from the rule by hand -- all noise-free, ``sensor_height=1.8`` -- and the host half of
``himo_amd.ground_seg``: the export's declaration, the struct mirror, and the program with the mask producer replaced."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import groundseg_ref as ref

REPO = Path(__file__).resolve().parents[1]
H = 1.8
GZ = np.float32(-H)


def rings(r_lo, r_hi, step=0.25, n_az=1440, z=lambda x, y, r: np.full_like(x, -H)):
    """points on concentric rings every ``step`` m (two per 0.5 m range bin) at ``n_az`` azimuths (0.25 degrees: several per segment,
    the narrowest of which spans 0.64 degrees), so that every cell between r_lo and r_hi holds surface points"""
    r, az = np.meshgrid(np.arange(r_lo, r_hi, step), np.linspace(-np.pi, np.pi, n_az, endpoint=False), indexing="ij")
    x, y = (r * np.cos(az)).ravel(), (r * np.sin(az)).ravel()
    return np.stack([x, y, z(x, y, r.ravel())], axis=1).astype(np.float32)


def test_flat_plane_with_boxes_above_it():
    plane = rings(2.0, 40.0)
    rng = np.random.default_rng(0)
    boxes = []
    for cx, cy in ((8.0, 0.0), (-12.0, 9.0), (3.0, -20.0), (-25.0, -25.0)):
        n = 400
        boxes.append(np.stack([cx + rng.uniform(-2, 2, n), cy + rng.uniform(-1, 1, n), -H + rng.uniform(0.5, 2.1, n)], axis=1))
    xyz = np.concatenate([plane] + boxes).astype(np.float32)
    perm = rng.permutation(len(xyz))                              # the answer does not depend on the order of the rows
    mask, G = ref.ground_mask(xyz[perm], True, sensor_height=H)
    want = np.zeros(len(xyz), bool)
    want[:len(plane)] = True
    assert np.array_equal(mask, want[perm])
    assert (G == GZ).all()                                        # every cell's height is the plane's, also where boxes stand


def test_five_percent_grade_is_all_ground():
    # a plane of 5 % grade through (0, 0, -1.8).  By hand: the first prototype of a segment (r ~ 2) lies at most 0.05 * 2 = 0.1 from
    # -1.8, inside 0.15 * 2 + 0.05.  Two points of cells in adjacent bins of a segment differ by at most 0.5 + 0.5 m in range and, out
    # to 30 m, 30 * 0.0222 = 0.67 m across the segment: 0.05 * that is below 0.2, so whether a prototype is accepted (its own height) or
    # rejected (its neighbour's), every point of the cell lies within ground_thresh of the cell's height.
    xyz = rings(2.0, 30.0, z=lambda x, y, r: -H + 0.05 * x)
    mask, G = ref.ground_mask(xyz, True, sensor_height=H)
    assert mask.all()
    assert G.min() < -H - 1.0 and G.max() > -H + 1.0              # the heights follow the slope


def test_vertical_wall_is_ground_only_at_its_foot():
    plane = rings(2.0, 30.0)
    y, z = np.meshgrid(np.arange(-5.0, 5.0, 0.05), -H + 0.1 * np.arange(31), indexing="ij")
    wall = np.stack([np.full(y.size, 20.0), y.ravel(), z.ravel()], axis=1).astype(np.float32)
    xyz = np.concatenate([plane, wall])
    mask = ref.ground_mask(xyz, sensor_height=H)
    assert mask[:len(plane)].all()
    want = (wall[:, 2] - GZ).astype(np.float32) <= np.float32(0.2)          # z + 1.8 <= 0.2, in float32 as rule D computes it
    assert np.array_equal(mask[len(plane):], want)
    assert 0 < want.sum() < len(want) and wall[want, 2].max() < -1.55 and wall[~want, 2].min() > -1.65


def test_a_one_metre_step_is_rejected_and_stays_non_ground():
    # ground at -1.8 out to 30 m, a surface 1 m higher from 30 m on.  The last accepted prototype is the inner ring of its bin (the
    # two rings tie in z; the lower index wins) at r = 29.5; a raised one is accepted only once 0.15 * (r - 29.5) + 0.05 >= 1, that is
    # from r = 35.84 on: up to 35.5 m every raised cell is rejected, carries -1.8, and its points are 1 m above that.
    xyz = rings(2.0, 35.6, z=lambda x, y, r: np.where(r < 30.0 - 1e-6, -H, -H + 1.0))
    mask, G = ref.ground_mask(xyz, True, sensor_height=H)
    r = np.hypot(xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64))
    assert mask[r < 29.9].all() and not mask[r > 29.9].any()
    assert (r > 29.9).sum() > 1000
    assert (G == GZ).all()
    far = rings(2.0, 40.0, z=lambda x, y, r: np.where(r < 30.0 - 1e-6, -H, -H + 1.0))
    far_mask = ref.ground_mask(far, sensor_height=H)
    rf = np.hypot(far[:, 0].astype(np.float64), far[:, 1].astype(np.float64))
    assert far_mask[rf > 36.4].all() and not far_mask[(rf > 29.9) & (rf < 35.8)].any()       # the rule's own limit, stated


def test_prototype_ties_go_to_the_lower_index():
    # two points of one cell (bin 18 of the segment along +x) tie in z at r = 10.1 and r = 10.4; the next bin's point lies 0.1 m
    # higher at r = 10.6: accepted iff 0.1 <= 0.15 * (10.6 - r_prev) + 0.05, which holds for r_prev = 10.1 (0.125) and fails for 10.4 (0.08)
    a, b, c = [10.1, 0.01, -H], [10.4, 0.01, -H], [10.6, 0.01, -H + 0.1]
    for pts, accepted in (([a, b, c], True), ([b, a, c], False)):
        xyz = np.array(pts, dtype=np.float32)
        G, cell, proto = ref.cell_ground(xyz, sensor_height=H)
        assert cell[0] == cell[1] == 18 * 360 and cell[2] == 19 * 360
        assert proto[cell[0]] == 0
        assert G.reshape(-1)[cell[2]] == (xyz[2, 2] if accepted else GZ)
        assert ref.ground_mask(xyz, sensor_height=H).tolist() == [True, True, True]          # (0.1 above the carried height is ground too)


def test_segments_grow_round_the_circle_and_unbinned_points_are_never_ground():
    az = np.deg2rad(np.arange(0.25, 360.0, 0.5))
    xyz = np.stack([5.2 * np.cos(az), 5.2 * np.sin(az), np.full(az.size, -H)], axis=1).astype(np.float32)      # mid-bin: (5.2 - 1) / 0.5 = 8.4
    _, cell = ref.cells(xyz)
    seg = cell % 360
    assert (cell // 360 == 8).all() and (np.diff(seg) >= 0).all() and seg[0] == 0 and seg[-1] == 359 and len(set(seg)) == 360
    odd = np.array([[0.5, 0.5, -H], [np.nan, 3, -H], [3, np.inf, -H], [3, 3, np.nan], [200.0, 0, -H], [1e30, 1e30, -H], [0, 0, -H]], np.float32)
    assert (ref.cells(odd)[1] == -1).all() and not ref.ground_mask(odd, sensor_height=H).any()
    assert ref.ground_mask(np.zeros((0, 3), np.float32)).shape == (0,)


# ---- the export and the struct -------------------------------------------------------------------------------------------------
def test_export_is_declared_in_the_header_and_bound():
    from himo_amd import _lib
    header = (REPO / "include" / "himo_amd.h").read_text()
    for name in ("himo_ground_seg_batch", "himo_ground_seg_workspace_bytes"):
        m = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert m, f"include/himo_amd.h does not declare {name}"
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(m.group(1).split(",")), name
    assert _lib.SIGNATURES["himo_ground_seg_batch"][0] is ctypes.c_int and _lib.SIGNATURES["himo_ground_seg_workspace_bytes"][0] is ctypes.c_size_t
    assert "parity unpinned" in header.lower()
    assert "FLAGS_groundseg := -ffp-contract=off" in (REPO / "himo_amd" / "csrc" / "Makefile").read_text()


def test_params_mirror_has_the_c_struct_size_and_the_documented_defaults():
    from himo_amd import _lib
    from himo_amd.ground_seg import GroundParams
    assert ctypes.sizeof(GroundParams) == 32
    assert _lib.load().himo_abi_sizeof(b"himo_ground_params") == ctypes.sizeof(GroundParams)
    p = GroundParams()
    got = {k: getattr(p, k) for k, _ in GroundParams._fields_}
    assert got == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in ref.DEFAULTS.items()}
    assert p.segments == 360 and GroundParams(sensor_height=1.8).sensor_height == np.float32(1.8)
    lib = _lib.load()
    cells = 256 * 360
    assert lib.himo_ground_seg_workspace_bytes(3, ctypes.addressof(p)) >= 3 * cells * 12
    assert lib.himo_ground_seg_workspace_bytes(0, ctypes.addressof(p)) == 0
    for bad in (dict(r_min=0.0), dict(bin_size=-1.0), dict(n_bins=0), dict(K=0), dict(K=513), dict(n_bins=4097), dict(max_slope=float("nan")),
                dict(sensor_height=float("inf"))):
        assert lib.himo_ground_seg_workspace_bytes(1, ctypes.addressof(GroundParams(**bad))) == 0, bad
    assert lib.himo_ground_seg_workspace_bytes(1, None) == 0


def test_the_rule_is_written_into_the_module_docstring():
    from himo_amd import ground_seg
    doc = ground_seg.__doc__
    for words in ("ray ground filter, v1", "PARITY UNPINNED", "fabs(z - g_prev) <= max_slope * (r - r_prev) + step_tol", "ground_thresh",
                  "ties to the lowest point index", "UNVERIFIED", "Known limits"):
        assert words in doc, words
    assert "UNVERIFIED" in ground_seg._parser().format_help()


# ---- the program's host side, with the mask producer replaced ----------------------------------------------------------------------
def _fake_masks(sweeps, params=None, device=None, return_cell_ground=False):
    return [ref.ground_mask(np.asarray(s)[:, :3], sensor_height=float(params.sensor_height)) for s in sweeps]


def _write_scenes(root, seg_raw=True):
    from himo_amd import h5lite
    from himo_amd.synthetic import make_frame
    trees = {}
    for sc in range(2):
        tree = {}
        for k in range(3):
            f = make_frame(10 * sc + k, n_points=1500, cloud="rings")
            tree[str(f["timestamp"])] = {"lidar": f["pc0"], "pose": f["pose0"], "flow": f["flow"]}
            if seg_raw:
                tree[str(f["timestamp"])]["seg_raw"] = (np.arange(1500) % 7).astype(np.uint8)
        h5lite.write_file(Path(root) / f"scene{sc}.h5", tree)
        trees[f"scene{sc}"] = tree
    return trees


def _need_hdf5():
    from himo_amd.save import h5_writer
    mod, how = h5_writer()
    assert mod is not None, how                                    # (the package's other in-place writers need it too)


def test_program_writes_bool_masks_into_the_scene_files(tmp_path, monkeypatch, capsys):
    from himo_amd import ground_seg, h5lite
    _need_hdf5()
    monkeypatch.setattr(ground_seg, "ground_masks", _fake_masks)
    trees = _write_scenes(tmp_path)
    done = ground_seg.main(str(tmp_path), sensor_height=H, batch=2)
    assert sorted(done) == ["scene0", "scene1"] and all(s["sweeps"] == 3 and s["points"] == 4500 for s in done.values())
    out = capsys.readouterr().out
    assert out.count("3 sweeps, 4500 points") == 2 and "% ground" in out
    for scene, tree in trees.items():
        with h5lite.File(tmp_path / f"{scene}.h5") as f:
            assert sorted(f.keys()) == sorted(tree)
            for ts, group in tree.items():
                got = f[ts]["ground_mask"]
                assert got.dtype == np.dtype(bool) and got._bool            # the 8-bit FALSE / TRUE enum, as h5py stores it
                assert np.array_equal(got[:], ref.ground_mask(group["lidar"][:, :3], sensor_height=H))
                assert sorted(f[ts].keys()) == sorted(list(group) + ["ground_mask"])
                for name, a in group.items():                              # the foreign datasets are untouched
                    b = f[ts][name][:]
                    assert b.dtype == a.dtype and b.tobytes() == np.ascontiguousarray(a).tobytes(), (ts, name)


def test_program_refuses_an_existing_key_without_overwrite_and_honours_key(tmp_path, monkeypatch):
    from himo_amd import ground_seg, h5lite
    _need_hdf5()
    monkeypatch.setattr(ground_seg, "ground_masks", _fake_masks)
    trees = _write_scenes(tmp_path, seg_raw=False)
    ground_seg._cli(["--data_dir", str(tmp_path), "--sensor_height", str(H)])
    with pytest.raises(FileExistsError, match="--overwrite"):
        ground_seg._cli(["--data_dir", str(tmp_path), "--sensor_height", str(H)])
    # another key is another dataset; the refusal concerns the key that is asked for
    ground_seg._cli(["--data_dir", str(tmp_path), "--sensor_height", "0.0", "--key", "gm_h0"])
    # --overwrite replaces: a different height gives a different mask under the same name
    ground_seg._cli(["--data_dir", str(tmp_path), "--sensor_height", "1.0", "--overwrite", "--batch", "1"])
    ts, group = next(iter(trees["scene1"].items()))
    with h5lite.File(tmp_path / "scene1.h5") as f:
        assert sorted(f[ts].keys()) == sorted(list(group) + ["ground_mask", "gm_h0"])
        assert np.array_equal(f[ts]["ground_mask"][:], ref.ground_mask(group["lidar"][:, :3], sensor_height=1.0))
        assert np.array_equal(f[ts]["gm_h0"][:], ref.ground_mask(group["lidar"][:, :3], sensor_height=0.0))
        assert not np.array_equal(f[ts]["ground_mask"][:], ref.ground_mask(group["lidar"][:, :3], sensor_height=H))
    d = ground_seg._parser().parse_args(["--data_dir", "x"])
    assert (d.sensor_height, d.key, d.overwrite, d.batch) == (0.0, "ground_mask", False, 32)


def test_program_without_an_hdf5_library_raises_naming_the_problem(tmp_path, monkeypatch):
    from himo_amd import ground_seg, save
    monkeypatch.setattr(ground_seg, "ground_masks", _fake_masks)
    monkeypatch.setattr(save, "h5_writer", lambda: (None, "no HDF5 library"))
    _write_scenes(tmp_path, seg_raw=False)
    before = {p.name: p.read_bytes() for p in tmp_path.iterdir()}
    with pytest.raises(RuntimeError, match="needs an HDF5 library"):
        ground_seg.main(str(tmp_path), sensor_height=H)
    assert {p.name: p.read_bytes() for p in tmp_path.iterdir()} == before            # no side file, nothing modified
    with pytest.raises(FileNotFoundError):
        ground_seg.main(str(tmp_path / "nothing_here"))


def test_extractor_options_default_off():
    from himo_amd import extract_sca as ex
    d = ex._parser().parse_args([])
    assert d.ground_mask is False and d.sensor_height == 0.0
    a = ex._parser().parse_args(["--ground_mask", "--sensor_height", "1.8"])
    assert a.ground_mask is True and a.sensor_height == 1.8
    assert "UNVERIFIED" in ex._parser().format_help()


def test_nothing_in_the_package_imports_the_checker():
    for p in (REPO / "himo_amd").rglob("*.py"):
        assert not re.search(r"^\s*(import|from)\s+\S*groundseg_ref", p.read_text(), re.M), p
