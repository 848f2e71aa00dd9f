"""The ground-truth zip writer on the GPU (tools/test/save_zip_gt.py): the kernel's record-batch bodies against the reference's
stored outputs (bitwise) and against ``feather.write_table`` of the oracle's columns (byte for byte), the program serial and
overlapped, the save_zip_gt -> score loop on the golden frames, real HDF5 scene files, and two ranks on one GPU."""
import os
import shutil
import socket
import subprocess
import sys
from pathlib import Path
from zipfile import ZIP_STORED, ZipFile

import numpy as np
import pytest

from conftest import GOLDEN, golden_frames

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
H5 = GOLDEN / "h5"
SCHEMAS = [(True, True), (False, True), (True, False), (False, False)]
# n % 8 in 0..7, n = 1, one sweep of >= 120 000 points, sweeps longer than a block and block-straddling neighbours
RAGGED = [8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 7, 120_003, 1031, 2047, 4096, 15]


def _run(frames, data_name):
    import torch
    from himo_amd.compdis import CompDisEngine, FrameBatch
    batch = FrameBatch.from_frames(frames, "flow", with_masks=True, with_labels=True, host_ego=True)
    body, at, (names, dtypes) = CompDisEngine(max_frames=len(frames)).run_gt(batch, data_name)
    torch.cuda.synchronize()
    return batch, body.cpu().numpy(), at, names, dtypes


def _oracle_file(oracle, f, data_name):
    from himo_amd import feather, save_zip_gt
    g = oracle.gt_frame(f, data_name)
    inst = f.get("flow_instance_id")
    return feather.write_table(save_zip_gt.frame_table(g["comp_dis"], g["eval_mask"], f.get("flow_category_indices"),
                                                       None if inst is None else np.asarray(inst).astype(np.uint32),
                                                       g["gt_flow_norm"], g["pc0"]))


def _assert_files(oracle, frames, data_name):
    from himo_amd import feather
    batch, body, at, names, dtypes = _run(frames, data_name)
    assert at[-1] == len(body)
    for k, f in enumerate(frames):
        n = len(f["pc0"])
        head, tail, body_len, _ = feather.framing(names, dtypes, n)
        assert at[k + 1] - at[k] == body_len
        mine = head + body[at[k]:at[k + 1]].tobytes() + tail
        want = _oracle_file(oracle, f, data_name)
        assert mine == want, (k, n, names)
    return names


@pytest.mark.parametrize("data_name", ["av2", "scania"])
def test_pinned_values_of_every_golden_sweep(gpu, gold, data_name):
    from himo_amd import save_zip_gt
    frames = golden_frames(gold, data_name)
    if data_name == "scania":
        assert any(len(f["pc0"]) == 2047 for f in frames)                  # an odd row count: every column is followed by pad bytes
    batch, body, at, names, dtypes = _run(frames, data_name)
    assert len(names) == 10
    for i, f in enumerate(frames):
        n = len(f["pc0"])
        c = save_zip_gt.body_columns(body[at[i]:at[i + 1]], names, dtypes, n)
        cd = np.stack([c["comp_dis_x_m"], c["comp_dis_y_m"], c["comp_dis_z_m"]], axis=1)
        ref_cd = gold[f"{data_name}/{i}/ref_gt_comp_dis"]
        assert cd.dtype == np.float32 and np.array_equal(cd, ref_cd.astype(np.float32)), i
        assert c["eval_mask"].dtype == np.uint8 and np.array_equal(c["eval_mask"], gold[f"{data_name}/{i}/ref_eval_mask"].astype(np.uint8)), i
        assert np.array_equal(c["gt_flow_norm"], gold[f"{data_name}/{i}/ref_gt_flow_norm"]), i
        assert np.array_equal(np.stack([c["pc0_x"], c["pc0_y"], c["pc0_z"]], axis=1), f["pc0"][:, :3]), i
        assert np.array_equal(c["flow_category_indices"], f["flow_category_indices"]), i
        assert np.array_equal(c["flow_instance_id"], f["flow_instance_id"].astype(np.uint32)), i


@pytest.mark.parametrize("data_name", ["av2", "scania"])
@pytest.mark.parametrize("category,instance", SCHEMAS)
def test_golden_files_are_the_host_encoders_bytes(gpu, gold, oracle, data_name, category, instance):
    frames = [dict(f) for f in golden_frames(gold, data_name)]
    for f in frames:
        if not category:
            del f["flow_category_indices"]
        if not instance:
            del f["flow_instance_id"]
    assert len(_assert_files(oracle, frames, data_name)) == 8 + category + instance


@pytest.mark.parametrize("category,instance", SCHEMAS)
def test_ragged_batch_files_are_the_host_encoders_bytes(gpu, oracle, category, instance):
    from himo_amd.synthetic import make_frame
    frames = [make_frame(300 + i, n_points=n, data_name="scania") for i, n in enumerate(RAGGED)]
    assert {n % 8 for n in RAGGED} == set(range(8)) and 1 in RAGGED and max(RAGGED) >= 120_000
    for f in frames:
        if not category:
            del f["flow_category_indices"]
        if not instance:
            del f["flow_instance_id"]
    for data_name in ("av2", "scania"):
        _assert_files(oracle, frames, data_name)


def test_xyz_rows_and_float32_poses(gpu, oracle):
    """(N,3) point rows take the kernel's any-stride loads; float32 poses the float32 chain numpy runs for them (sweeps of two rows
    and more there: numpy hands a ONE-row float32 product to sgemv, whose accumulation is not the k-ordered one of sgemm)"""
    from himo_amd.synthetic import make_frame
    frames = [make_frame(400 + i, n_points=n) for i, n in enumerate([5000, 1, 1027, 14])]
    xyz = [dict(f, pc0=np.ascontiguousarray(f["pc0"][:, :3])) for f in frames]
    _assert_files(oracle, xyz, "av2")
    f32 = [dict(f, pose0=f["pose0"].astype(np.float32), pose1=f["pose1"].astype(np.float32)) for f in frames if len(f["pc0"]) > 1]
    _assert_files(oracle, f32, "av2")


def test_overlapped_writer_writes_the_serial_loops_files(gpu, oracle, tmp_path):
    """run_dataset's feeder -> kernel -> drain form (head, the device-written body, tail) writes byte-identical files to the serial
    loop through the host encoder, over ragged sweeps, a short last batch and sweeps that lack a label column; the reference's
    three errors arrive with the earlier batches on disk."""
    from himo_amd import save_zip_gt
    from himo_amd.synthetic import SyntheticDataset
    ds = SyntheticDataset(11, n_points=20_000, ragged=True, data_name="scania")

    class Edited:
        def __init__(self, edit):
            self.edit = edit

        def __len__(self):
            return len(ds)

        def __getitem__(self, i):
            f = dict(ds[i])
            self.edit(i, f)
            return f

    def drop_labels(i, f):
        if i == 5:
            del f["flow_category_indices"]
        if i in (6, 10):
            del f["flow_instance_id"]
    outs = []
    for overlap in (False, True):
        out = tmp_path / f"o{int(overlap)}"
        out.mkdir()
        assert save_zip_gt.run_dataset(Edited(drop_labels), "scania", out, batch_frames=4, overlap=overlap) == 11
        outs.append(out)
    names = sorted(p.relative_to(outs[0]) for p in outs[0].rglob("*.feather"))
    assert len(names) == 11 and names == sorted(p.relative_to(outs[1]) for p in outs[1].rglob("*.feather"))
    for n in names:
        assert (outs[0] / n).read_bytes() == (outs[1] / n).read_bytes(), n
    f5 = Edited(drop_labels)[5]
    assert (outs[1] / f5["scene_id"] / f"{f5['timestamp']}.feather").read_bytes() == _oracle_file(oracle, f5, "scania")

    def broken(how):
        def edit(i, f):
            if i == 9 and how == "empty":
                f["lidar_dt"] = f["lidar_dt"][:0]
            if i == 9 and how == "flow":
                del f["flow"]
            if i == 9 and how == "valid":
                del f["flow_is_valid"]
        return Edited(edit)
    for how, exc in (("empty", ValueError), ("flow", KeyError), ("valid", KeyError)):
        for overlap in (False, True):
            out = tmp_path / f"{how}{int(overlap)}"
            out.mkdir()
            with pytest.raises(exc, match="empty sequence" if how == "empty" else "flow" if how == "flow" else "flow_is_valid"):
                save_zip_gt.run_dataset(broken(how), "scania", out, batch_frames=4, overlap=overlap)
            assert len(list(out.rglob("*.feather"))) == 8                # batches 0 and 1 were complete


@pytest.mark.parametrize("data_name", ["av2", "scania"])
def test_the_loop_closes_on_the_golden_frames(gpu, gold, eval_gold, data_name, tmp_path):
    """save_zip_gt.run_dataset -> zip -> score against the reference-written prediction zip = the reference's scores.json."""
    from himo_amd import save_zip_gt
    from himo_amd.dataset import ListDataset
    from himo_amd.score import score
    frames = golden_frames(gold, data_name)
    out = tmp_path / f"{data_name}_gt"                                     # the scorer takes the data set's name from the path
    out.mkdir()
    assert save_zip_gt.run_dataset(ListDataset(frames), data_name, out, batch_frames=3) == len(frames)
    z = save_zip_gt.zip_res(out, output_file=str(out / "flow-submit.zip"))
    with ZipFile(z) as mine, ZipFile(GOLDEN / f"{data_name}_gt.zip") as ref:
        assert set(mine.namelist()) == set(ref.namelist()) and all(i.compress_type == ZIP_STORED for i in mine.infolist())
    got = score(z, str(GOLDEN / f"{data_name}_pred.zip"), output_dir=str(tmp_path / "scores"))
    ref = eval_gold[f"{data_name}/scores"]
    for k, v in ref.items():
        if isinstance(v, float):
            assert got[k] == pytest.approx(v, rel=2e-6), k
        else:
            assert got[k] == v, k
    assert got["num_instances"] > 0


@pytest.mark.parametrize("data_name", ["av2", "scania"])
def test_main_on_real_hdf5_scene_files(gpu, oracle, tmp_path, data_name):
    from himo_amd import feather, save_zip, save_zip_gt
    from himo_amd.dataset import open_dataset
    from himo_amd.score import score
    root = tmp_path / data_name / "himo"
    shutil.copytree(H5, root)
    out = tmp_path / data_name / "gt"
    save_zip_gt.main(str(root), str(out), batch_frames=3)
    z = out / "flow-submit.zip"
    ds = open_dataset(root, vis_name="seflowpp_best", eval=True)
    with ZipFile(z) as zf:
        assert sorted(zf.namelist()) == sorted(f"{ds[i]['scene_id']}/{ds[i]['timestamp']}.feather" for i in range(len(ds)))
        assert len(ds) == 4 and all(i.compress_type == ZIP_STORED for i in zf.infolist())
        for i in range(len(ds)):
            f = ds[i]
            data = zf.read(f"{f['scene_id']}/{f['timestamp']}.feather")
            assert data == _oracle_file(oracle, f, data_name), i
            t = feather.read_table(data)
            g = oracle.gt_frame(f, data_name)
            assert np.array_equal(t["gt_flow_norm"], g["gt_flow_norm"]) and np.array_equal(t["eval_mask"], g["eval_mask"].astype(np.uint8))
    assert not [p for p in out.iterdir() if p.is_dir()]                    # the scene folders are gone
    save_zip.main(str(root), "seflowpp_best", batch_frames=4)
    got = score(str(z), str(root / "results" / "seflowpp_best-submit.zip"), output_dir=str(tmp_path / "scores"))
    assert got["num_frames"] == 4 and (tmp_path / "scores" / "scores.json").exists()


def _torchrun(module, *args, cwd, nproc=2):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HIMO_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=str(REPO))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "HIMO_DIST_FORCE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), "-m", module, *args], env=env, cwd=cwd, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (module, out.stderr[-3000:])
    return out


def test_two_ranks_on_one_gpu_write_every_sweep_once(gpu, oracle, tmp_path):
    """the program as two ranks sharing this box's GPU (gloo collectives: RCCL refuses two ranks per device)"""
    from himo_amd.dataset import open_dataset
    root = tmp_path / "scania" / "val"
    shutil.copytree(H5, root)
    out = tmp_path / "scania" / "gt"
    _torchrun("himo_amd.save_zip_gt", "--data_dir", str(root), "--output_dir", str(out), "--batch_frames", "1", cwd=tmp_path)
    assert [p.name for p in out.iterdir()] == ["flow-submit.zip"]
    ds = open_dataset(root, vis_name="", eval=True)
    with ZipFile(out / "flow-submit.zip") as zf:
        assert sorted(zf.namelist()) == sorted(f"{ds[i]['scene_id']}/{ds[i]['timestamp']}.feather" for i in range(len(ds)))
        for i in range(len(ds)):
            f = ds[i]
            assert zf.read(f"{f['scene_id']}/{f['timestamp']}.feather") == _oracle_file(oracle, f, "scania"), i
