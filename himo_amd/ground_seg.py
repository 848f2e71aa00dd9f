"""The ground segmenter: the per-point ``ground_mask`` that every program of this package consumes (the loader serves it as
``gm0`` / ``gm1``: ``eval`` and ``save_zip_gt`` build the evaluation mask from ``~gm0``, ``seflow.fit`` with
``ssl_label=seflow_auto`` clusters the non-ground points of both sweeps).

PARITY UNPINNED.  The reference's extractor takes the mask from a ground-segmentation pass in its absent ``OpenSceneFlow``
submodule; that algorithm is not readable.  Like the network, this stage follows the build's own written rule, below, and is
checked bit for bit against a numpy restatement of it (``tests/groundseg_ref.py``), never against the reference.

The rule -- "ray ground filter, v1" (normative)
================================================
Designed so that the device and numpy decide every point identically: no transcendental function touches the point path, and
every float operation rounds on its own (``himo_amd/csrc/groundseg.hip`` is built with ``-ffp-contract=off``; ``sqrtf`` and the
float32 divisions are correctly rounded).

Parameters (``GroundParams``): ``sensor_height`` 0.0 m (the ground is expected at z = -sensor_height under the vehicle),
``r_min`` 1.0 m, ``bin_size`` 0.5 m, ``n_bins`` 256, ``K`` 45 (8 K = 360 segments), ``max_slope`` 0.15, ``step_tol`` 0.05 m,
``ground_thresh`` 0.2 m.  Admitted: r_min > 0, bin_size > 0, 1 <= n_bins <= 4096, 1 <= K <= 512, every float finite.

A. Cell of a point (all arithmetic float32).  ``r = sqrtf(x*x + y*y)``.  A point is UNBINNED, and never ground, if any of x, y,
   z is non-finite, if ``r < r_min``, or if its range bin ``b = (int)((r - r_min) / bin_size)`` is ``>= n_bins`` (decided on the
   float quotient ``q``: unbinned unless ``q < n_bins``, which also catches a range that overflowed to infinity).  The segment
   comes from signs and magnitudes only: the octant from ``(x < 0, y < 0, |y| > |x|)`` (octants are counted round the circle from
   +x towards +y; -0.0 is not negative), ``t = min(|x|,|y|) / max(|x|,|y|)``, ``k = min(K-1, (int)(t*K))``, mirrored to
   ``K-1-k`` in the odd octants so that the segment index ``octant*K + k`` grows monotonically round the circle.
   ``max(|x|,|y|) == 0`` cannot happen once ``r >= r_min`` holds.  Segments are equal in TANGENT, not in angle (the ones at the
   diagonals are narrower): accepted.
B. Prototype of a cell: its point of lowest z, ties to the lowest point index; it carries that point's ``(r, z)``.  "Lowest" is
   the order of the 64-bit key ``(ordered bits of z) << 32 | index`` the device minimises, in which -0.0 precedes +0.0.
C. Walk, once per segment over the bins in ascending order, in float64 on float32 inputs.  The state starts at
   ``(r_prev, g_prev) = (0, (float)-sensor_height)``.  A non-empty bin with prototype ``(r, z)`` is ACCEPTED iff
   ``fabs(z - g_prev) <= max_slope * (r - r_prev) + step_tol``; then its ground height is ``G = z`` and the state becomes
   ``(r, z)``.  On rejection -- and for a bin without points -- ``G = g_prev`` and the state is unchanged.  Every ``G`` is a
   float32 value exactly.  The cells of a sweep WITHOUT points all hold ``(float)-sensor_height``.
D. Decision: a binned point is ground iff ``z - G[cell] <= ground_thresh`` (one float32 subtraction, one compare).

Known limits.  A below-ground outlier (a multipath return) can become its cell's prototype; the slope test then rejects it and
the cell carries the previous height, so the outlier itself is still ground by rule D.  Overhanging structure above accepted
ground (a bridge, a branch) is non-ground only through rule D's threshold, not through any test of its own.  The
``sensor_height`` default of 0.0 m is an UNVERIFIED assumption about the Scania vehicle frame (origin on the ground under the
vehicle); the synthetic sweeps of this package have the sensor at the origin 1.8 m above the ground (``--sensor_height 1.8``).

The program: ``python -m himo_amd.ground_seg --data_dir D [--sensor_height H] [--key ground_mask] [--overwrite] [--batch 32]``
walks the ``<scene>.h5`` files of ``D``, reads only ``lidar``, and writes ``<timestamp>/<key>`` as bool (the 8-bit FALSE / TRUE
enum, as h5py stores it) INTO the scene file.  There is no CPU path and no side-file convention for masks.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np


class GroundParams(ctypes.Structure):
    """mirror of ``himo_ground_params`` (include/himo_amd.h)"""
    _fields_ = [("sensor_height", ctypes.c_float), ("r_min", ctypes.c_float), ("bin_size", ctypes.c_float), ("n_bins", ctypes.c_int32),
                ("K", ctypes.c_int32), ("max_slope", ctypes.c_float), ("step_tol", ctypes.c_float), ("ground_thresh", ctypes.c_float)]

    def __init__(self, sensor_height=0.0, r_min=1.0, bin_size=0.5, n_bins=256, K=45, max_slope=0.15, step_tol=0.05, ground_thresh=0.2):
        super().__init__(sensor_height, r_min, bin_size, n_bins, K, max_slope, step_tol, ground_thresh)

    @property
    def segments(self) -> int:
        return 8 * int(self.K)


def workspace_bytes(n_frames: int, params: GroundParams) -> int:
    from . import _lib
    return int(_lib.load().himo_ground_seg_workspace_bytes(int(n_frames), ctypes.addressof(params)))


def segment_batch(pc, offsets_host: np.ndarray, offsets, params: GroundParams, mask=None, cell_ground=None, workspace=None):
    """Launch ``himo_ground_seg_batch`` on the current stream over a packed device tensor ``pc`` [T, 3 or 4] float32 whose sweep f
    owns the rows ``offsets_host[f]:offsets_host[f+1]`` (``offsets``: the same values on the device).  Returns the uint8 device
    mask [T] (``mask`` when given).  ``cell_ground``: a float32 device tensor [F, n_bins, 8K] to receive the cells' heights (the
    rows of a sweep without points are left as they are).  Asynchronous; the workspace must outlive the launch."""
    import torch
    from . import _lib
    lib = _lib.load()
    n, total = len(offsets_host) - 1, int(offsets_host[-1])
    if pc.dim() != 2 or pc.shape[1] not in (3, 4) or pc.dtype != torch.float32 or not pc.is_contiguous():
        raise ValueError(f"points are contiguous float32 rows of 3 or 4 columns, not {tuple(pc.shape)} {pc.dtype}")
    if mask is None:
        mask = torch.empty(total, dtype=torch.uint8, device=pc.device)
    need = workspace_bytes(n, params)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=pc.device)
    st = lib.himo_ground_seg_batch(n, total, offsets_host.ctypes.data, _lib.ptr(offsets), _lib.ptr(pc), int(pc.shape[1]),
                                   ctypes.addressof(params), _lib.ptr(mask), _lib.ptr(cell_ground), _lib.ptr(workspace),
                                   workspace.numel(), _lib.stream_handle())
    _lib.check(st, "himo_ground_seg_batch")
    return mask


def ground_masks(sweeps, params: GroundParams | None = None, device=None, return_cell_ground: bool = False):
    """``ground_mask`` of every sweep of ``sweeps`` -- float32 ``(N, >=3)`` numpy arrays or device tensors, x y z first -- in ONE
    launch: a list of bool arrays.  ``return_cell_ground``: also the float32 [len(sweeps), n_bins, 8K] ground heights of the
    cells.  There is no CPU path."""
    import torch
    from . import _lib
    from .sweeps import host_upload, sweep_offsets
    params = params if params is not None else GroundParams()
    dev = device if device is not None else _lib.require_gpu()
    sweeps = list(sweeps)
    for k, s in enumerate(sweeps):
        if len(s.shape) != 2 or s.shape[1] < 3:
            raise ValueError(f"sweep {k}: points are rows of x, y, z[, ...], not {tuple(s.shape)}")
    if not sweeps:
        return ([], np.zeros((0, int(params.n_bins), params.segments), np.float32)) if return_cell_ground else []
    if workspace_bytes(len(sweeps), params) == 0:
        raise ValueError("ground_masks: parameters outside r_min > 0, bin_size > 0, 1 <= n_bins <= 4096, 1 <= K <= 512, finite floats")
    pitch = 4 if all(s.shape[1] == 4 for s in sweeps) else 3
    offsets_host = sweep_offsets(s.shape[0] for s in sweeps)
    if all(isinstance(s, np.ndarray) for s in sweeps):
        pc = host_upload(dev)([s[:, :pitch] for s in sweeps], np.float32)
    else:
        pc = torch.cat([(torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)) if isinstance(s, np.ndarray) else s)[:, :pitch]
                        .to(device=dev, dtype=torch.float32) for s in sweeps], dim=0).contiguous()
    offsets = host_upload(dev)([offsets_host], np.int64)
    cell = None
    if return_cell_ground:
        cell = torch.full((len(sweeps), int(params.n_bins), params.segments), float(np.float32(-np.float32(params.sensor_height))),
                          dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        mask = segment_batch(pc, offsets_host, offsets, params, cell_ground=cell)
        host_mask = mask.cpu().numpy().astype(bool)                       # (the copy waits for the launch)
    out = [host_mask[int(offsets_host[k]):int(offsets_host[k + 1])] for k in range(len(sweeps))]
    return (out, cell.cpu().numpy()) if return_cell_ground else out


def ground_mask(pc, params: GroundParams | None = None, device=None, return_cell_ground: bool = False):
    """``ground_masks`` for one sweep: a bool array [N] (and, with ``return_cell_ground``, the float32 [n_bins, 8K] heights)"""
    out = ground_masks([pc], params, device, return_cell_ground)
    return (out[0][0], out[1][0]) if return_cell_ground else out[0]


# --------------------------------------------------------------------------------------------------------------------------
# the program
# --------------------------------------------------------------------------------------------------------------------------
def segment_scene(path, params: GroundParams, key: str = "ground_mask", overwrite: bool = False, batch: int = 32, opener=None) -> dict:
    """One scene file: read every sweep's ``lidar`` (nothing else), compute the masks ``batch`` sweeps per launch, and only once
    the reads are done open the file for modification and write ``<timestamp>/<key>``.  Returns {"sweeps", "points", "ground"}."""
    from .dataset import h5_reader
    from .stored import h5_module, put_keys
    path = Path(path)
    masks = []
    with h5_reader().File(path, "r") as f:
        stamps = sorted(f.keys())
        have = [ts for ts in stamps if key in f[ts]]
        if have and not overwrite:
            raise FileExistsError(f"{path}: {len(have)} of {len(stamps)} sweeps already hold '{key}' (--overwrite replaces them)")
        for lo in range(0, len(stamps), max(1, int(batch))):
            part = stamps[lo:lo + max(1, int(batch))]
            masks += ground_masks([np.asarray(f[ts]["lidar"][:], dtype=np.float32) for ts in part], params)
    if opener is None:
        mod = h5_module(f"{path}: writing '{key}' into a scene file")
        opener = lambda p: mod.File(p, "a")                               # noqa: E731
    with opener(path) as f:
        for ts, m in zip(stamps, masks):
            put_keys(f, ts, {key: np.asarray(m, dtype=bool)})
    points = int(sum(len(m) for m in masks))
    return {"sweeps": len(stamps), "points": points, "ground": int(sum(int(m.sum()) for m in masks))}


def main(data_dir: str, sensor_height: float = 0.0, key: str = "ground_mask", overwrite: bool = False, batch: int = 32,
         params: GroundParams | None = None) -> dict:
    """The program.  Under ``torchrun`` (one rank per GPU) the scenes are dealt round-robin to the ranks, so every file has one
    writer.  Returns {scene: {"sweeps", "points", "ground"}} of this rank."""
    from . import distenv
    from .stored import h5_module
    params = params if params is not None else GroundParams(sensor_height=sensor_height)
    scenes = sorted(Path(data_dir).glob("*.h5"))
    if not scenes:
        raise FileNotFoundError(f"{data_dir}: no <scene>.h5 files")
    mod = h5_module(f"writing '{key}' into the scene files of {data_dir}")
    done = {}
    with distenv.process_group() as (rank, world):
        def loop():
            for path in scenes[rank::world]:
                s = done[path.stem] = segment_scene(path, params, key, overwrite, batch, opener=lambda p: mod.File(p, "a"))
                share = s["ground"] / s["points"] if s["points"] else 0.0
                print(f"{path.stem}: {s['sweeps']} sweeps, {s['points']} points, {100.0 * share:.1f} % ground -> '{key}'")

        distenv.run_shard(loop, "its scene files")
    return done


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="write <timestamp>/ground_mask into the <scene>.h5 files of a directory (ray ground filter, v1; "
                                             "parity with the reference's segmenter unpinned; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files; only 'lidar' is read")
    ap.add_argument("--sensor_height", type=float, default=0.0,
                    help="the ground is expected at z = -sensor_height under the vehicle; the default 0.0 is an UNVERIFIED assumption about "
                         "the Scania vehicle frame (the synthetic sweeps want 1.8)")
    ap.add_argument("--key", default="ground_mask", help="dataset name to write")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing <key> instead of refusing the scene")
    ap.add_argument("--batch", type=int, default=32, help="sweeps per launch")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.sensor_height, a.key, a.overwrite, a.batch)


if __name__ == "__main__":
    _cli()
