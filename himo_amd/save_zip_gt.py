"""Drop-in for the reference's ``tools/test/save_zip_gt.py``: ground-truth flow -> ground-truth compensation distances,
evaluation mask, labels and points -> one Feather file per sweep -> a *stored* zip, the first argument of
``python -m himo_amd.score --gt_zip G --pred_zip P``.

Same public names and wire format as the reference:
    read_output_zip(zip_path, (scene_id, ts)) -> (comp_dis, eval_mask, category | None, instance | None)   save_zip_gt.py:34-62
    write_output_file(comp_dis, (scene_id, ts), output_dir, eval_mask, ...)                                save_zip_gt.py:64-108
    zip_res(res_folder, output_file)                                                                       save_zip_gt.py:111-127
    main(data_dir, output_dir, res_name)                                                                   save_zip_gt.py:129-180

``res_name`` names the zip (``<output_dir>/<res_name>-submit.zip``) and nothing else: the ``est_flow`` the reference derives from
it is never written, so the result key is not read.  The arithmetic runs on the device (himo_amd/csrc/compdis_gt.hip), which
writes every sweep's record-batch BODY in its file layout: a file is ``head + body + tail`` with the framing of
``feather.framing`` (schema and row count alone), so no column is touched again on the host.  With ``torch.distributed``
initialised the sweeps are sharded across ranks (frame i -> rank i % world), every rank writes its files, rank 0 zips.
"""
from __future__ import annotations

from pathlib import Path
from typing import Tuple
from zipfile import ZipFile

import numpy as np

from . import feather
from .save_zip import zip_res  # noqa: F401  (zip_res: the reference's public name, same function as save_zip's)

COMP_DIS_COLUMNS = ("comp_dis_x_m", "comp_dis_y_m", "comp_dis_z_m")
PC0_COLUMNS = ("pc0_x", "pc0_y", "pc0_z")


def read_output_zip(zip_path: str, sweep_uuid: Tuple[str, int]):
    """(N,3) float32 compensation distances, (N,) bool evaluation mask and the two label columns (None where the file has
    none) of one sweep; a missing member raises ``KeyError`` like ``ZipFile.open`` does in the reference."""
    with ZipFile(zip_path, "r") as myzip:
        with myzip.open(f"{sweep_uuid[0]}/{sweep_uuid[1]}.feather") as f:
            table = feather.read_table(f.read())
    comp_dis = np.stack([table[c].astype(np.float32) for c in COMP_DIS_COLUMNS], axis=1)
    eval_mask = table["eval_mask"].astype(bool)
    category = table["flow_category_indices"].astype(np.uint8) if "flow_category_indices" in table else None
    instance = table["flow_instance_id"].astype(np.uint32) if "flow_instance_id" in table else None
    return comp_dis, eval_mask, category, instance


def frame_table(compensation_dis, eval_mask, flow_category_indices=None, flow_instance_id=None, gt_flow_norm=None, pc0=None) -> dict:
    """the ordered columns of save_zip_gt.py:89-105 (optional ones left out when ``None``)"""
    cd = np.asarray(compensation_dis)
    cols = {name: cd[:, k].astype(np.float32) for k, name in enumerate(COMP_DIS_COLUMNS)}
    cols["eval_mask"] = np.asarray(eval_mask).astype(np.uint8)
    if flow_category_indices is not None:
        cols["flow_category_indices"] = np.asarray(flow_category_indices).astype(np.uint8)
    if flow_instance_id is not None:
        cols["flow_instance_id"] = np.asarray(flow_instance_id).astype(np.uint32)
    if gt_flow_norm is not None:
        cols["gt_flow_norm"] = np.asarray(gt_flow_norm).astype(np.float32)
    if pc0 is not None:
        p = np.asarray(pc0)
        for k, name in enumerate(PC0_COLUMNS):
            cols[name] = p[:, k].astype(np.float32)
    return cols


def write_output_file(compensation_dis, sweep_uuid: Tuple[str, int], output_dir: Path, eval_mask, flow_category_indices=None,
                      flow_instance_id=None, gt_flow_norm=None, pc0=None) -> None:
    """``<output_dir>/<scene_id>/<timestamp>.feather`` through the host encoder (``feather.write_table``)."""
    output_log_dir = Path(output_dir) / sweep_uuid[0]
    output_log_dir.mkdir(exist_ok=True, parents=True)
    table = frame_table(compensation_dis, eval_mask, flow_category_indices, flow_instance_id, gt_flow_norm, pc0)
    with open(output_log_dir / f"{sweep_uuid[1]}.feather", "wb") as fh:
        fh.write(feather.write_table(table))


def body_columns(body: np.ndarray, names, dtypes, rows: int) -> dict:
    """{column: array} views of one sweep's record-batch body (a uint8 array laid out by ``feather.framing``)"""
    _, spans = feather.body_layout(dtypes, rows)
    return {n: body[off:off + nbytes].view(np.dtype(dt).newbyteorder("<")) for n, dt, (off, nbytes) in zip(names, dtypes, spans)}


def _schema_key(frame) -> tuple:
    return "flow_category_indices" in frame, "flow_instance_id" in frame


OVERLAP = True          # read / stage / copy ahead and write behind on background threads (False: the reference's plain serial loop)


def run_dataset(dataset, data_name: str, output_dir: Path, batch_frames: int = 32, overlap: bool | None = None, sensor_dt: float = 0.1) -> int:
    """Shared body of ``main``: iterate ``dataset`` (frame i on rank i % world), batch sweeps into HBM, run the fused ground-truth
    kernel, write one Feather per sweep.  Returns the sweeps written by this rank.

    As ``save_zip.run_dataset``: with ``overlap`` (default) a feeder thread reads, packs and copies the frames two batches ahead
    (``feeder.BatchFeeder``), the launch thread enqueues the kernel, and each sweep's body leaves through a pinned buffer to four
    writer threads (``feeder.ResultDrain``) that write ``head``, the pinned view and ``tail``; ``overlap=False`` is the serial loop,
    which decodes the columns and goes through ``write_output_file``.  A batch holds sweeps of one schema: the reference decides
    per sweep whether a label column exists (save_zip_gt.py:172-173), so sweeps that lack one form a batch of their own."""
    from .compdis import CompDisEngine, FrameBatch
    from .sweeps import FeatherSink, draining, fed, sharded_batches

    overlap = OVERLAP if overlap is None else overlap
    eng = CompDisEngine(max_frames=batch_frames)

    def batches():
        for keys in sharded_batches(dataset, batch_frames):
            frames = [dataset[i] for i in keys]
            for f in frames:
                if len(f["lidar_dt"]) == 0:
                    raise ValueError("max() arg is an empty sequence")       # save_zip_gt.py:164
            kinds = []
            for f in frames:
                if _schema_key(f) not in kinds:
                    kinds.append(_schema_key(f))
            for kind in kinds:
                yield [f for f in frames if _schema_key(f) == kind]

    def build(frames, upload):
        staged = {} if upload is None else {"device": eng.device, "upload": upload}
        return frames, FrameBatch.from_frames(frames, "flow", with_masks=True, with_labels=True, host_ego=True, **staged)
    drain = None
    if overlap:
        from .feeder import ResultDrain
        files = FeatherSink(output_dir)     # (a writer thread's ``body`` is a view of the drain's pinned buffer, gone when the sink returns)
        drain = ResultDrain(lambda key, body: files.write(key[0], key[1], [key[2], memoryview(body), key[3]]), device=eng.device, threads=4,
                            copy=False)
    written = 0
    feed = fed(batches(), build, device=eng.device if overlap else None, overlap=overlap)
    with draining(feed, drain):
        for frames, batch in feed:
            body, at, (names, dtypes) = eng.run_gt(batch, data_name, sensor_dt=sensor_dt)
            if drain is None:
                body = body.cpu().numpy()       # one D2H copy per batch
            o = batch.offsets_host
            for k, f in enumerate(frames):
                key, rows, part = (f["scene_id"], str(f["timestamp"])), int(o[k + 1] - o[k]), body[int(at[k]):int(at[k + 1])]
                if drain is None:               # the serial loop decodes the columns and goes through the host encoder
                    c = body_columns(part, names, dtypes, rows)
                    write_output_file(np.stack([c[n] for n in COMP_DIS_COLUMNS], axis=1), key, output_dir, c["eval_mask"],
                                      flow_category_indices=c.get("flow_category_indices"), flow_instance_id=c.get("flow_instance_id"),
                                      gt_flow_norm=c["gt_flow_norm"], pc0=np.stack([c[n] for n in PC0_COLUMNS], axis=1))
                else:
                    head, tail, _, _ = feather.framing(names, dtypes, rows)
                    drain.put(key + (head, tail), part)
                written += 1
    return written


def main(data_dir: str = "/home/kin/data/av2/h5py/sensor/himo/demo", output_dir: str = "/home/kin/data/av2/h5py/sensor/himo/results",
         res_name: str = "flow", batch_frames: int = 32, allow_dropped_eval: bool | None = None):
    """save_zip_gt.py:129-180.  Under ``torchrun`` (one rank per GPU) the sweeps are sharded i % world, every rank writes its own
    Feather files, and rank 0 zips once all of them are on disk (a rank that fails still reaches the rendezvous, so nobody zips
    a partial result or waits for a dead process)."""
    from . import distenv
    from .dataset import EVAL_FIELDS, open_dataset
    from .utils import check_valid

    data_dir, output_dir = Path(data_dir), Path(output_dir)
    output_dir.mkdir(exist_ok=True, parents=True)
    data_name, _ = check_valid(str(data_dir), res_name, None)

    def loop():
        # vis_name="": the estimate named by res_name is not read (the reference computes an est_flow from it and drops it)
        dataset = open_dataset(data_dir, vis_name="", eval=True, allow_dropped_eval=allow_dropped_eval, fields=EVAL_FIELDS)
        run_dataset(dataset, data_name, output_dir, batch_frames=batch_frames)
    with distenv.process_group() as (rank, world):
        distenv.run_shard(loop, "its Feather files, but no ground-truth zip was written")
        if rank == 0:
            zip_res(output_dir, output_file=f"{output_dir}/{res_name}-submit.zip")
        if world > 1:
            distenv.all_ranks_ok(True)                           # nobody leaves before the zip exists


def _cli(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="ground-truth flow -> GT comp_dis, mask, labels -> ground-truth zip for the scorer (MI355X path)")
    ap.add_argument("--data_dir", default="/home/kin/data/av2/h5py/sensor/himo/demo")
    ap.add_argument("--output_dir", default="/home/kin/data/av2/h5py/sensor/himo/results")
    ap.add_argument("--res_name", default="flow")
    ap.add_argument("--batch_frames", type=int, default=32)
    ap.add_argument("--allow_dropped_eval", action="store_true", default=None,
                    help="skip index_eval.pkl sweeps that have no successor sweep in their h5 scene instead of failing")
    a = ap.parse_args(argv)
    main(a.data_dir, a.output_dir, a.res_name, a.batch_frames, a.allow_dropped_eval)


if __name__ == "__main__":
    from .sweeps import timed
    timed(_cli)
