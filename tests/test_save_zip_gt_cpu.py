"""The ground-truth zip writer's host side without a GPU (tools/test/save_zip_gt.py): the body layout the kernel places its
stores with, the framing around a body, the host encoder's round trip, and the sharded program over gloo with the device
arithmetic replaced by the oracle INSIDE THESE TESTS ONLY."""
import ctypes
import os
import socket
import sys
from pathlib import Path
from zipfile import ZipFile

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
SCHEMAS = [(True, True), (False, True), (True, False), (False, False)]
ROWS = list(range(18)) + [2047, 120_000]


def _columns(rng, n, category, instance):
    from himo_amd import feather
    names, dtypes = feather.gt_schema(category, instance)
    cols = {}
    for name, dt in zip(names, dtypes):
        if dt.kind == "f":
            cols[name] = rng.normal(size=n).astype(dt)
        else:
            cols[name] = rng.integers(0, 2 if name == "eval_mask" else np.iinfo(dt).max, size=n, dtype=dt)
    return names, dtypes, cols


@pytest.mark.parametrize("category,instance", SCHEMAS)
def test_kernel_layout_is_the_framings_spans(category, instance):
    """himo_gt_column_starts / himo_gt_body_bytes (the host+device function compdis_gt.hip addresses its columns with) and the
    launcher's d_body_offsets equal feather._framing's spans / body lengths."""
    from himo_amd import _lib, feather
    from himo_amd.compdis import gt_body_offsets
    lib = _lib.load()
    names, dtypes = feather.gt_schema(category, instance)
    bits = (_lib.GT_HAS_CATEGORY if category else 0) | (_lib.GT_HAS_INSTANCE if instance else 0)
    assert len(names) == 8 + category + instance
    lengths = []
    for n in ROWS:
        head, tail, body_len, spans = feather._framing(names, dtypes, n)
        assert feather.framing(names, dtypes, n) == (head, tail, body_len, spans)
        starts = (ctypes.c_int64 * _lib.GT_MAX_COLUMNS)()
        assert lib.himo_gt_column_starts(n, bits, starts) == body_len == lib.himo_gt_body_bytes(n, bits)
        present = [s for s in starts if s >= 0]
        assert present == [off for off, _ in spans] and all(s % 8 == 0 for s in present)
        absent = [k for k, s in enumerate(starts) if s < 0]
        assert absent == [k for k, (nm, _) in enumerate(feather.GT_COLUMNS) if nm not in names]
        lengths.append(body_len)
    offsets = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
    at = gt_body_offsets(offsets, dtypes)
    assert at.dtype == np.int64 and at[0] == 0 and np.array_equal(np.diff(at), lengths) and np.all(at % 8 == 0)


@pytest.mark.parametrize("category,instance", SCHEMAS)
def test_head_body_tail_is_a_feather_file(category, instance):
    from himo_amd import feather
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 2047):
        names, dtypes, cols = _columns(rng, n, category, instance)
        head, tail, body_len, spans = feather.framing(names, dtypes, n)
        body = np.zeros(body_len, np.uint8)
        for (off, nbytes), name in zip(spans, names):
            body[off:off + nbytes] = cols[name].view(np.uint8)
        data = head + body.tobytes() + tail
        assert data == feather.write_table(cols)
        back = feather.read_table(data)
        assert list(back) == list(names)
        for name, dt in zip(names, dtypes):
            assert back[name].dtype == dt and np.array_equal(back[name], cols[name])
        try:
            import pyarrow as pa
            import pyarrow.ipc as ipc
        except ImportError:
            continue
        t = ipc.open_file(pa.BufferReader(data)).read_all()
        assert t.column_names == list(names)
        for name, dt in zip(names, dtypes):
            assert t.schema.field(name).type == pa.from_numpy_dtype(dt) and np.array_equal(t[name].to_numpy(), cols[name])


def test_write_output_file_round_trip(tmp_path):
    from himo_amd import feather, save_zip_gt
    rng = np.random.default_rng(2)
    n = 37
    cd, pc0 = rng.normal(size=(n, 3)), rng.normal(size=(n, 4)).astype(np.float32)
    mask, cat = rng.uniform(size=n) > 0.5, rng.integers(0, 30, n).astype(np.int64)
    inst, norm = rng.integers(0, 2 ** 32, n, dtype=np.uint64), rng.uniform(size=n)
    out = tmp_path / "out"
    save_zip_gt.write_output_file(cd, ("s0", "100"), out, mask, flow_category_indices=cat, flow_instance_id=inst, gt_flow_norm=norm, pc0=pc0[:, :3])
    save_zip_gt.write_output_file(cd, ("s0", "200"), out, mask)
    save_zip_gt.write_output_file(cd, ("s1", "300"), out, mask, flow_instance_id=inst, pc0=pc0[:, :3])
    full = feather.read_table((out / "s0" / "100.feather").read_bytes())
    assert list(full) == [nm for nm, _ in feather.GT_COLUMNS]
    assert [full[nm].dtype for nm in full] == [np.dtype(dt) for _, dt in feather.GT_COLUMNS]
    assert np.array_equal(full["gt_flow_norm"], norm.astype(np.float32)) and np.array_equal(full["pc0_y"], pc0[:, 1])
    assert list(feather.read_table((out / "s0" / "200.feather").read_bytes())) == list(feather.GT_COLUMNS[k][0] for k in range(4))
    assert list(feather.read_table((out / "s1" / "300.feather").read_bytes())) == [
        "comp_dis_x_m", "comp_dis_y_m", "comp_dis_z_m", "eval_mask", "flow_instance_id", "pc0_x", "pc0_y", "pc0_z"]
    z = save_zip_gt.zip_res(out, output_file=str(out / "flow-submit.zip"))
    with ZipFile(z) as zf:
        assert sorted(zf.namelist()) == ["s0/100.feather", "s0/200.feather", "s1/300.feather"]
    assert not (out / "s0").exists()
    got = save_zip_gt.read_output_zip(z, ("s0", "100"))
    assert got[0].dtype == np.float32 and np.array_equal(got[0], cd.astype(np.float32))
    assert got[1].dtype == bool and np.array_equal(got[1], mask)
    assert got[2].dtype == np.uint8 and np.array_equal(got[2], cat.astype(np.uint8))
    assert got[3].dtype == np.uint32 and np.array_equal(got[3], inst.astype(np.uint32))
    bare = save_zip_gt.read_output_zip(z, ("s0", "200"))
    assert bare[2] is None and bare[3] is None and np.array_equal(bare[1], mask)
    half = save_zip_gt.read_output_zip(z, ("s1", "300"))
    assert half[2] is None and np.array_equal(half[3], inst.astype(np.uint32))
    with pytest.raises(KeyError):
        save_zip_gt.read_output_zip(z, ("s0", "999"))


# ---- two gloo ranks, the device arithmetic replaced by the oracle ----------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cpu_gt_double():
    """test double for CompDisEngine.run_gt: the oracle computes, feather.write_table lays the body out; host logic is the real one"""
    import torch
    import himo_oracle as oracle
    from himo_amd import compdis, feather, save_zip_gt

    class CpuEngine:
        def __init__(self, *a, **k):
            pass

        def run_gt(self, batch, data_name, sensor_dt=0.1):
            names, dtypes = feather.gt_schema(batch.category is not None, batch.instance is not None)
            bodies = []
            for f in batch._frames:
                g = oracle.gt_frame(f, data_name, sensor_dt)
                table = save_zip_gt.frame_table(g["comp_dis"], g["eval_mask"], f.get("flow_category_indices"), f.get("flow_instance_id"),
                                                g["gt_flow_norm"], g["pc0"])
                head, tail, body_len, _ = feather.framing(names, dtypes, len(g["comp_dis"]))
                data = feather.write_table(table)
                bodies.append(np.frombuffer(data[len(head):len(head) + body_len], np.uint8))
            at = compdis.gt_body_offsets(batch.offsets_host, dtypes)
            assert [len(b) for b in bodies] == list(np.diff(at))
            return torch.from_numpy(np.concatenate(bodies).copy()), at, (names, dtypes)

    real = compdis.FrameBatch.from_frames.__func__

    def from_frames(cls, frames, res_name="flow", device=None, upload=None, **kw):
        b = real(cls, frames, res_name, device=torch.device("cpu"), **kw)
        b._frames = list(frames)
        return b

    compdis.CompDisEngine = CpuEngine
    compdis.FrameBatch.from_frames = classmethod(from_frames)
    save_zip_gt.OVERLAP = False                                # the feeder / drain threads need HIP streams and pinned memory


def _frames(n=7):
    from himo_amd.synthetic import make_frame
    frames = [make_frame(i, n_points=400 + 13 * i, scene_id=f"scene{i // 4}") for i in range(n)]
    del frames[2]["flow_category_indices"]                     # sweeps that lack a label column get a file without it
    del frames[5]["flow_instance_id"]
    return frames


def _worker_cli(rank, world, port, data_dir, out_dir, fail_rank):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "LOCAL_RANK": str(rank),
                       "WORLD_SIZE": str(world)})
    sys.path.insert(0, str(REPO))
    sys.path.insert(0, str(REPO / "oracle"))
    import torch.distributed as dist
    _cpu_gt_double()
    from himo_amd import save_zip_gt
    if rank == fail_rank:
        def broken(*a, **k):
            raise OSError("disk full on this rank")
        save_zip_gt.write_output_file = broken
    try:
        save_zip_gt._cli(["--data_dir", data_dir, "--output_dir", out_dir, "--batch_frames", "2"])
        Path(out_dir, f"ok{rank}").write_text("done")
    except BaseException as e:
        Path(out_dir, f"err{rank}").write_text(type(e).__name__)
    assert not dist.is_initialized()                             # the entry point left the group it joined


def test_two_ranks_write_every_sweep_once_and_rank_0_zips(tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, str(REPO / "oracle"))
    import himo_oracle as oracle
    from himo_amd import feather, save_zip_gt
    from himo_amd.dataset import NpzDataset
    root, out = tmp_path / "av2" / "demo", tmp_path / "av2" / "gt"
    frames = _frames()
    NpzDataset.write(root, frames)
    mp.spawn(_worker_cli, args=(2, _free_port(), str(root), str(out), -1), nprocs=2, join=True)
    assert (out / "ok0").exists() and (out / "ok1").exists()
    z = out / "flow-submit.zip"
    with ZipFile(z) as zf:
        assert sorted(zf.namelist()) == sorted(f"{f['scene_id']}/{f['timestamp']}.feather" for f in frames)
        tables = {n: feather.read_table(zf.read(n)) for n in zf.namelist()}
    for i, f in enumerate(frames):
        g = oracle.gt_frame(f, "av2")
        cd, mask, cat, inst = save_zip_gt.read_output_zip(str(z), (f["scene_id"], str(f["timestamp"])))
        assert np.array_equal(cd, g["comp_dis"]) and np.array_equal(mask, g["eval_mask"])
        assert (cat is None) == (i == 2) and (inst is None) == (i == 5)
        t = tables[f"{f['scene_id']}/{f['timestamp']}.feather"]
        assert np.array_equal(t["gt_flow_norm"], g["gt_flow_norm"]) and np.array_equal(t["pc0_z"], f["pc0"][:, 2])


def test_a_failing_rank_leaves_no_zip_and_hangs_nobody(tmp_path):
    import torch.multiprocessing as mp
    from himo_amd.dataset import NpzDataset
    root, out = tmp_path / "av2" / "demo", tmp_path / "av2" / "gt"
    NpzDataset.write(root, _frames())
    mp.spawn(_worker_cli, args=(2, _free_port(), str(root), str(out), 1), nprocs=2, join=True)     # returns: nobody hangs
    assert (out / "err1").read_text() == "OSError" and (out / "err0").read_text() == "RuntimeError"
    assert not (out / "flow-submit.zip").exists()
