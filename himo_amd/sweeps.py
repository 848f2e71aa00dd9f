"""What the dataset programs (``save_zip``, ``save_zip_gt``, ``eval_seg``, ``eval_flow``, ``extract_sca``, ...) share on the host:

* packing: sweeps laid end to end (``sweep_offsets``, ``SweepPacker``), every device tensor made by one ``upload(parts, dtype)``
  call -- ``host_upload`` by default, the staging hook of ``feeder.BatchFeeder`` when the batch is fed;
* the loop: this rank's share of a dataset in batches (``sharded_batches``), by whole scenes (``sharded_scenes``) or as item indices
  (``sharded_items``), the batches built on the calling thread or two ahead
  by ``feeder.BatchFeeder`` (``fed``), warnings that travel with a missing key (``MissingKey``), the order in which feeder and
  ``feeder.ResultDrain`` are closed (``draining``) and the one-Feather-file-per-sweep writer (``FeatherSink``);
* ``timed``: the "Time used" tail of the command lines.

No arithmetic happens here and nothing touches the device except through ``upload``.
"""
from __future__ import annotations

import threading
import time
from contextlib import contextmanager
from functools import cached_property
from pathlib import Path

import numpy as np

from . import distenv


# ---- packing ---------------------------------------------------------------------------------------------------------------
def sweep_offsets(counts) -> np.ndarray:
    """int64 [F+1]: sweep f owns rows ``offsets[f]:offsets[f + 1]`` of a batch laid end to end"""
    counts = list(counts)
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets


def host_upload(dev):
    """default ``upload(parts, dtype)``: concatenate on the host, one synchronous copy to ``dev``"""
    import torch

    def up(parts, dtype):
        host = np.concatenate([np.asarray(p).astype(dtype, copy=False) for p in parts], axis=0)
        return torch.from_numpy(np.ascontiguousarray(host)).to(dev, non_blocking=False)
    return up


class SweepPacker:
    """The sweeps of ``frames`` (host dicts) laid end to end: ``frames[k][count_key]`` has one row per point of sweep k, and every
    array packed with ``cat`` must have as many.  ``upload(parts, dtype) -> device tensor`` of the row-wise concatenation of ``parts``
    converted to ``dtype`` (None: ``host_upload(device)``) makes every tensor, one call each.  A missing key is a ``KeyError``."""

    def __init__(self, frames, upload=None, device=None, count_key: str = "pc0"):
        self.frames = list(frames)
        if not self.frames:
            raise ValueError("empty batch")
        if upload is None:
            from . import _lib
            upload = host_upload(device if device is not None else _lib.require_gpu())
        self.upload = upload
        self.counts = [int(np.asarray(f[count_key]).shape[0]) for f in self.frames]
        self.offsets_host = sweep_offsets(self.counts)

    @cached_property
    def offsets(self):
        """``offsets_host`` on the device (uploaded when first read)"""
        return self.upload([self.offsets_host], np.int64)

    def cat(self, key, dtype, width=None, labels: bool = False):
        """every sweep's ``key`` end to end as ``dtype``; ``width``: the row length the arrays must have; ``labels``: flat uint8 labels
        (``eval_seg.as_labels_u8``)"""
        host = np.asarray
        if labels:
            from .eval_seg import as_labels_u8 as host
        parts = []
        for f, n in zip(self.frames, self.counts):
            a = host(f[key])
            if a.shape[0] != n or (width is not None and a.shape[1:] != (width,)):
                raise ValueError(f"{f.get('scene_id')} at {f.get('timestamp')}: {key} has shape {a.shape} for a sweep of {n} points")
            parts.append(a)
        return self.upload(parts, dtype)

    def stack(self, key, dtype):
        """[F, ...]: every sweep's ``key`` (a 4x4 pose) stacked as ``dtype``"""
        return self.upload([np.stack([np.asarray(f[key], dtype=dtype) for f in self.frames])], dtype)


# ---- the loop --------------------------------------------------------------------------------------------------------------
def sharded_batches(dataset, batch_frames: int) -> list:
    """The index lists of this rank's batches: item i of ``dataset`` belongs to rank i % world, ``batch_frames`` items per batch"""
    rank, world = distenv.rank_world()
    mine = range(rank, len(dataset), world)
    return [list(mine[lo:lo + batch_frames]) for lo in range(0, len(mine), batch_frames)]


def scene_items(ds) -> dict:
    """scene -> its item indices, from the dataset's index: scenes in the order they first appear, items in index order"""
    scenes = {}
    for i, (scene, _) in enumerate(ds.index):
        scenes.setdefault(scene, []).append(i)
    return scenes


def sharded_scenes(ds) -> list:
    """This rank's ``(scene, items)``: scene number n of ``scene_items`` belongs to rank n % world, so a scene file has one writer"""
    rank, world = distenv.rank_world()
    return [(scene, items) for n, (scene, items) in enumerate(scene_items(ds).items()) if n % world == rank]


def sharded_items(ds, whole_scenes: bool) -> list:
    """This rank's item indices, ascending: item i % world (the npz container: a file per sweep), or with ``whole_scenes`` the items
    of ``sharded_scenes``"""
    rank, world = distenv.rank_world()
    if not whole_scenes:
        return list(range(rank, len(ds), world))
    return sorted(i for _, items in sharded_scenes(ds) for i in items)


def fed(source, build, device=None, overlap: bool = True):
    """``build(item, upload)`` for every item of ``source``, in order.  ``overlap=False``: on the calling thread, ``upload`` None (the
    packers then copy for themselves).  ``overlap=True``: read, packed and copied two items ahead by ``feeder.BatchFeeder``, which is
    closed however the iteration ends -- an error of the source or of the consumer, ``close()`` of this generator, or the last item."""
    if not overlap:
        for item in source:
            yield build(item, None)
        return
    from .feeder import BatchFeeder
    feed = BatchFeeder(source, build, device=device)
    try:
        yield from feed
    finally:
        feed.close()


class MissingKey(Exception):
    """raised by a batch source for the key a sweep lacks: carries the warnings printed before the reference's KeyError to the
    thread that prints"""

    def __init__(self, key, lines):
        super().__init__(key)
        self.key, self.lines = key, list(lines)


def raise_missing(e: MissingKey):
    """in the ``except MissingKey`` of the calling thread: print the lines ``e`` carries, then the reference's ``KeyError``"""
    for line in e.lines:
        print(line)
    raise KeyError(e.key) from None


@contextmanager
def draining(feed, drain):
    """Around a loop that takes batches from ``feed`` (a ``fed`` generator) and puts results into ``drain`` (a ``feeder.ResultDrain``,
    or None).  The loop raised: the feed is closed, the drain is closed with its own error dropped -- the sweeps already computed
    still reach the disk, as in a serial loop -- and the loop's error goes on.  It ended: the drain is closed and its error raised."""
    try:
        yield
    except BaseException:
        feed.close()
        if drain is not None:
            try:
                drain.close()
            except BaseException:
                pass
        raise
    if drain is not None:
        drain.close()


class FeatherSink:
    """``<output_dir>/<scene>/<stamp>.feather`` written from any number of threads: a scene's folder is made once"""

    def __init__(self, output_dir):
        self.dir = Path(output_dir)
        self._made, self._lock = set(), threading.Lock()

    def write(self, scene, stamp, buffers) -> None:
        scene_dir = self.dir / scene
        if scene not in self._made:
            with self._lock:
                scene_dir.mkdir(exist_ok=True, parents=True)
                self._made.add(scene)
        with open(scene_dir / f"{stamp}.feather", "wb") as fh:
            for buf in buffers:
                fh.write(buf)


# ---- the command lines -----------------------------------------------------------------------------------------------------
def timed(cli):
    """the ``__main__`` tail: run ``cli()``, print the time it took and, where it returns metrics with a ``loop`` record, the loop's rate"""
    start_time = time.time()
    got = cli()
    print(f"Time used: {time.time() - start_time:.2f} s")
    loop = getattr(got, "loop", None)
    if loop is not None:
        print(f"Evaluation loop: {loop['sweeps'] / max(loop['seconds'], 1e-9):.0f} sweeps/s ({loop['sweeps']} sweeps in {loop['seconds']:.2f} s)")
    return got
