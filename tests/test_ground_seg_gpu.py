"""The ground segmenter on the GPU: ``himo_ground_seg_batch`` bit for bit against the numpy restatement of its written rule
(tests/groundseg_ref.py; parity with the reference's own segmenter is unpinned) -- masks and, where asked for, the cells'
ground heights -- over the sizes at which the kernels change path, the edge values of rule A, ragged batches and the refusals;
then the program end to end: scenes without ``ground_mask`` cannot be trained on, the program writes the masks, the loader, the
training loop and the evaluator take them; and the extractor's ``--ground_mask`` writes the same masks."""
import ctypes
import os
import pickle
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import groundseg_ref as ref
from conftest import REPO

pytestmark = pytest.mark.gpu

H = 1.8
GUARD, FILL = 4096, 0xA5


def launch(sweeps, dev, pitch=3, want_cells=True, ws_bytes=None, mask_off=0, xyz_off=0, **kw):
    """raw call: (status, mask bytes [T], cell heights [F, n_bins, 8K] or None, guards untouched?, offsets)"""
    import torch
    from himo_amd import _lib
    from himo_amd.ground_seg import GroundParams
    lib = _lib.load()
    call_pitch = kw.pop("call_pitch", pitch)
    p = GroundParams(**{"sensor_height": H, **kw})
    offs = np.zeros(len(sweeps) + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in sweeps])
    T = int(offs[-1])
    rows = [np.concatenate([np.asarray(s, np.float32).reshape(-1, 3), np.full((len(s), pitch - 3), 7.0, np.float32)], axis=1) for s in sweeps]
    host = np.concatenate(rows).reshape(-1) if rows else np.zeros(0, np.float32)
    xyz = torch.full((xyz_off + host.size + 4,), float("nan"), dtype=torch.float32, device=dev)
    xyz[xyz_off:xyz_off + host.size] = torch.from_numpy(host).to(dev)
    mask = torch.full((2 * GUARD + T + 16,), FILL, dtype=torch.uint8, device=dev)
    at = GUARD + mask_off
    cells = torch.full((len(sweeps), p.n_bins, 8 * p.K), float(np.float32(-np.float32(H))), dtype=torch.float32, device=dev) if want_cells else None
    need = int(lib.himo_ground_seg_workspace_bytes(len(sweeps), ctypes.addressof(p)))
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=dev)
    st = lib.himo_ground_seg_batch(len(sweeps), T, offs.ctypes.data, torch.from_numpy(offs).to(dev).data_ptr(), xyz.data_ptr() + 4 * xyz_off,
                                   call_pitch, ctypes.addressof(p), mask.data_ptr() + at, _lib.ptr(cells), ws.data_ptr(),
                                   need if ws_bytes is None else ws_bytes, _lib.stream_handle())
    torch.cuda.synchronize()
    h = mask.cpu().numpy()
    clean = bool((h[:at] == FILL).all() and (h[at + T:] == FILL).all())
    return st, h[at:at + T].copy(), None if cells is None else cells.cpu().numpy(), clean, offs


def assert_equals_the_restatement(sweeps, dev, **kw):
    st, mask, cells, clean, offs = launch(sweeps, dev, **kw)
    assert st == 0 and clean
    rule = {k: v for k, v in kw.items() if k in ref.DEFAULTS}
    hits = 0
    for k, s in enumerate(sweeps):
        want, G = ref.ground_mask(np.asarray(s, np.float32).reshape(-1, 3), True, sensor_height=H, **rule)
        got = mask[int(offs[k]):int(offs[k + 1])]
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), want), f"mask of sweep {k}: {int((got.astype(bool) != want).sum())} of {len(want)} points differ"
        if cells is not None:
            assert cells[k].tobytes() == G.tobytes(), f"cell heights of sweep {k}: {int((cells[k].view(np.uint32) != G.view(np.uint32)).sum())} cells differ"
        hits += int(want.sum())
    return hits


def rings_sweep(seed, n):
    from himo_amd.synthetic import make_frame
    return make_frame(seed, n_points=n, cloud="rings")


def seeded(seed, n):
    """ground-like points with walls and clutter, out to beyond the last bin"""
    rng = np.random.default_rng(seed)
    r, az = rng.uniform(0.2, 140.0, n) ** rng.choice([1.0, 0.5], n), rng.uniform(-np.pi, np.pi, n)
    z = np.where(rng.random(n) < 0.7, -H + 0.03 * r * np.cos(az) + rng.normal(0, 0.03, n), rng.uniform(-2.5, 3.0, n))
    return np.stack([r * np.cos(az), r * np.sin(az), z], axis=1).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("pitch", [3, 4])
def test_small_sizes_and_both_pitches(gpu, n, pitch):
    hits = assert_equals_the_restatement([seeded(n, n)], gpu, pitch=pitch)
    assert n < 63 or hits > 0


def test_unaligned_points_and_mask_take_the_element_paths(gpu):
    assert_equals_the_restatement([seeded(5, 1031)], gpu, pitch=4, xyz_off=1, mask_off=1)
    assert_equals_the_restatement([seeded(6, 1031)], gpu, pitch=3, mask_off=3)


def test_all_points_in_one_cell_with_a_tie(gpu):
    rng = np.random.default_rng(1)
    n = 4096
    r, az = rng.uniform(10.05, 10.45, n), rng.uniform(0.001, 0.02, n)
    xyz = np.stack([r * np.cos(az), r * np.sin(az), -H + rng.uniform(0.0, 1.0, n)], axis=1).astype(np.float32)
    xyz[[3000, 700], 2] = np.float32(-H - 0.01)                    # the two lowest tie; 700 is the prototype
    _, cell = ref.cells(xyz)
    assert len(set(cell)) == 1 and cell[0] >= 0
    assert ref.cell_ground(xyz, sensor_height=H)[2][cell[0]] == 700
    assert_equals_the_restatement([xyz], gpu)
    assert_equals_the_restatement([xyz[::-1].copy()], gpu, pitch=4)


def test_axes_diagonals_origin_and_range_edges(gpu):
    one = np.float32(1.0)
    lo, hi = np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2))
    last = np.float32(1.0 + 256 * 0.5)                              # the outer edge of the last bin
    pts = []
    for d in (2.0, 7.3, 50.0):
        pts += [[d, 0, -H], [-d, 0, -H], [0, d, -H], [0, -d, -H], [d, d, -H], [-d, d, -H], [d, -d, -H], [-d, -d, -H], [d, -0.0, -H], [-0.0, d, -H]]
    pts += [[0, 0, -H], [-0.0, 0.0, -H], [0, 0, 0]]
    for r in (lo, one, hi, last, np.nextafter(last, np.float32(0)), np.nextafter(last, np.float32(1e9)), np.float32(1e30), np.float32(3e38)):
        pts += [[r, 0, -H], [0, -r, -H], [-r, 0, -H + 0.1]]
    for z in (0.0, -0.0, np.nan, np.inf, -np.inf):
        pts += [[3, 1, z], [-1, 3, z]]
    for bad in (np.nan, np.inf, -np.inf):
        pts += [[bad, 2, -H], [2, bad, -H], [bad, bad, bad]]
    xyz = np.array(pts, dtype=np.float32)
    assert_equals_the_restatement([xyz], gpu)
    assert_equals_the_restatement([xyz], gpu, pitch=4)
    # z = +-0.0 as the ground itself: -0.0 precedes +0.0 among a cell's points
    zeros = np.array([[5.2, 0.1, 0.0], [5.3, 0.1, -0.0], [5.25, 0.1, 0.0], [6.2, 0.1, -0.0], [6.3, 0.1, 0.0]], np.float32)
    assert ref.cell_ground(zeros, sensor_height=0.0)[2][ref.cells(zeros)[1][0]] == 1
    st, mask, cells, clean, _ = launch([zeros], gpu, sensor_height=0.0)
    want, G = ref.ground_mask(zeros, True, sensor_height=0.0)
    assert st == 0 and clean and np.array_equal(mask.astype(bool), want) and cells[0].tobytes() == G.tobytes()


def test_ragged_batch_with_an_empty_sweep_and_other_parameters(gpu):
    from himo_amd import _lib
    from himo_amd.ground_seg import GroundParams
    sweeps = [seeded(11, 1500), np.zeros((0, 3), np.float32), seeded(12, 2049)]
    assert_equals_the_restatement(sweeps, gpu)
    assert_equals_the_restatement(sweeps[::-1], gpu, pitch=4)
    assert_equals_the_restatement(sweeps, gpu, n_bins=37, K=7, bin_size=1.25, r_min=0.5, max_slope=0.3, step_tol=0.02, ground_thresh=0.1)
    p = GroundParams(sensor_height=H)
    need = _lib.load().himo_ground_seg_workspace_bytes(3, ctypes.addressof(p))
    assert need >= 3 * 256 * 360 * 12 and need == _lib.load().himo_ground_seg_workspace_bytes(3, ctypes.addressof(GroundParams()))
    st, _, _, clean, _ = launch([np.zeros((0, 3), np.float32)] * 2, gpu)          # nothing to do is not an error
    assert st == 0 and clean


@pytest.fixture(scope="module")
def rings_120k():
    f = rings_sweep(7, 120_000)
    return f, ref.ground_mask(f["pc0"][:, :3], True, sensor_height=H)


def test_rings_sweeps_and_two_runs_give_the_same_bytes(gpu, rings_120k):
    small = rings_sweep(3, 20_000)
    assert assert_equals_the_restatement([small["pc0"][:, :3]], gpu, pitch=4) > 5000
    f, (want, G) = rings_120k
    runs = [launch([f["pc0"][:, :3], small["pc0"][:, :3]], gpu, pitch=4) for _ in range(2)]
    for st, mask, cells, clean, offs in runs:
        assert st == 0 and clean
        assert np.array_equal(mask[:120_000].astype(bool), want) and cells[0].tobytes() == G.tobytes()
    assert runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2].tobytes() == runs[1][2].tobytes()
    agree = float((want == f["gm0"]).mean())
    print(f"\nground_seg on a 120 000-point rings sweep: {100 * want.mean():.2f} % ground, agreement with the synthetic's own gm0 "
          f"{100 * agree:.2f} % (a figure, not a gate)")


def test_python_entry_points(gpu, rings_120k):
    import torch
    from himo_amd.ground_seg import GroundParams, ground_mask, ground_masks
    f, (want, G) = rings_120k
    p = GroundParams(sensor_height=H)
    other = seeded(21, 777)
    masks, cells = ground_masks([f["pc0"], np.concatenate([other, np.ones((777, 2), np.float32)], axis=1), np.zeros((0, 4), np.float32)], p,
                                return_cell_ground=True)
    assert [m.dtype for m in masks] == [np.dtype(bool)] * 3 and [len(m) for m in masks] == [120_000, 777, 0]
    assert np.array_equal(masks[0], want) and cells[0].tobytes() == G.tobytes()
    assert np.array_equal(masks[1], ref.ground_mask(other, sensor_height=H))
    assert (cells[2] == np.float32(-H)).all()
    one = ground_mask(torch.from_numpy(other).to(gpu), p)
    assert one.dtype == np.dtype(bool) and np.array_equal(one, masks[1])
    assert ground_masks([], p) == []
    with pytest.raises(ValueError):
        ground_masks([other], GroundParams(r_min=0.0))
    with pytest.raises(ValueError):
        ground_masks([other[:, :2]], p)


def test_refusals_launch_nothing(gpu):
    from himo_amd import _lib
    sweeps = [seeded(31, 300), seeded(32, 500)]
    for kw, status in ((dict(call_pitch=2), _lib.ERR_INVALID_ARGUMENT), (dict(call_pitch=5), _lib.ERR_INVALID_ARGUMENT),
                       (dict(call_pitch=0), _lib.ERR_INVALID_ARGUMENT), (dict(ws_bytes=1024), _lib.ERR_WORKSPACE),
                       (dict(ws_bytes=2 * 256 * 360 * 12 - 256), _lib.ERR_WORKSPACE), (dict(K=0), _lib.ERR_INVALID_ARGUMENT),
                       (dict(bin_size=0.0), _lib.ERR_INVALID_ARGUMENT)):
        st, mask, cells, clean, _ = launch(sweeps, gpu, **kw)
        assert st == status, kw
        assert clean and (mask == FILL).all() and (cells == np.float32(-H)).all(), kw
    st, mask, _, clean, _ = launch(sweeps, gpu)
    assert st == 0 and clean and not (mask == FILL).any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _scenes_without_masks(root):
    from himo_amd import h5lite
    from himo_amd.synthetic import make_scene
    root.mkdir(parents=True)
    index, clouds = [], {}
    for sc in range(2):
        tree = {}
        for f in make_scene(40 + sc, 3, n_points=8_000, scene_id=f"gs{sc}", cloud="rings"):
            ts = str(f["timestamp"])
            tree[ts] = {"lidar": f["pc0"], "lidar_dt": f["lidar_dt"], "lidar_id": f["lidar_id"], "pose": f["pose0"], "flow": f["flow"],
                        "flow_is_valid": f["flow_is_valid"], "flow_category_indices": f["flow_category_indices"],
                        "flow_instance_id": f["flow_instance_id"]}
            index.append([f"gs{sc}", ts])
            clouds[(f"gs{sc}", ts)] = f["pc0"]
        h5lite.write_file(root / f"gs{sc}.h5", tree)
    with open(root / "index_total.pkl", "wb") as fh:
        pickle.dump(index, fh)
    return clouds


def test_scenes_become_trainable_and_evaluable(gpu, tmp_path, capsys):
    import warnings
    from himo_amd import ground_seg
    from himo_amd.dataset import HDF5Dataset
    from himo_amd.seflow import spec
    from himo_amd.seflow.fit import fit, train_fields
    root = tmp_path / "av2_scenes"
    clouds = _scenes_without_masks(root)

    def train_one_step():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                        # (the last sweep of a scene has no successor)
            ds = HDF5Dataset(root, fields=train_fields("seflow_auto"), zero_copy=True)
        try:
            return fit(ds, spec.init_params(3), epochs=1, batch_size=2, max_points=8_000, device=gpu, log=None, ssl_label="seflow_auto", max_steps=1)
        finally:
            ds.close()

    with pytest.raises(KeyError, match="himo_amd.ground_seg"):
        train_one_step()
    done = ground_seg.main(str(root), sensor_height=H, batch=2)
    assert sorted(done) == ["gs0", "gs1"] and all(s["sweeps"] == 3 and s["points"] == 24_000 and 0 < s["ground"] < s["points"] for s in done.values())
    assert capsys.readouterr().out.count("% ground") == 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ds = HDF5Dataset(root, eval=True)
    seen = 0
    for i in range(len(ds)):
        f = ds[i]
        want = ref.ground_mask(clouds[(f["scene_id"], str(f["timestamp"]))][:, :3], sensor_height=H)
        assert f["gm0"].dtype == np.dtype(bool) and np.array_equal(f["gm0"], want)
        seen += 1
    ds.close()
    assert seen >= 4
    out = train_one_step()
    assert out["history"][-1]["steps"] == 1 and np.isfinite(out["history"][-1]["train_loss"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, "-m", "himo_amd.eval", "--data_dir", str(root), "--res_name", "raw"], env=env, cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert (tmp_path / "res-av2.json").exists()


def test_extractor_writes_the_masks_the_program_writes(gpu, tmp_path):
    from himo_amd import extract_sca as ex, ground_seg, h5lite
    from test_extract_sca_gpu import RAW, SCA, _tree
    kw = dict(origin_data=str(RAW), metadata_pkl=str(RAW / "metadata.pkl"), nproc=2, batch_sweeps=3, lidar_ext_dir=str(SCA / "lidar_ext"),
              name_mapping=str(SCA / "name_mapping.json"))
    ex.main(output_dir=str(tmp_path / "with"), ground_mask=True, sensor_height=0.4, **kw)
    ex.main(output_dir=str(tmp_path / "plain"), **kw)
    (tmp_path / "plain" / "index_total.pkl").unlink()
    ground_seg.main(str(tmp_path / "plain"), sensor_height=0.4, batch=5)
    a, b = _tree(tmp_path / "with"), _tree(tmp_path / "plain")
    assert a == b and sum(k[2] == "ground_mask" for k in a) == 8
    golden = _tree(SCA / "h5")
    assert {k: v for k, v in a.items() if k[2] != "ground_mask"} == golden          # the option adds a dataset and changes nothing else
    with h5lite.File(tmp_path / "with" / "batch_11.h5") as f:
        m, pc = f["0001"]["ground_mask"], f["0001"]["lidar"][:]
        assert m.dtype == np.dtype(bool) and np.array_equal(m[:], ref.ground_mask(pc[:, :3], sensor_height=0.4))
    (tmp_path / "one").mkdir()
    with open(RAW / "metadata.pkl", "rb") as fh:
        meta = [m for m in pickle.load(fh) if m["sample_idx"] == "batch_12"]
    ex.process_one(str(RAW), tmp_path / "one", "batch_12", meta, lidar_ext_dir=str(SCA / "lidar_ext"), name_mapping=str(SCA / "name_mapping.json"),
                   ground_params=ground_seg.GroundParams(sensor_height=0.4))
    assert _tree(tmp_path / "one") == {k: v for k, v in a.items() if k[0] == "batch_12.h5"}
