"""Frame sources with the ``len`` / ``[i]`` protocol of the reference's ``HDF5Dataset``
(constructed at save_zip.py:111 and eval.py:279 as ``HDF5Dataset(dir, vis_name=<res>, eval=True)``).

The reference's loader lives in the EMPTY ``OpenSceneFlow`` submodule, so the h5 layout below is
taken from the in-tree writers and consumers only:
    per-scene file ``<scene_id>.h5`` with one group per timestamp holding ``lidar`` (N,4) f32,
    ``lidar_dt`` (N,) f32, ``lidar_id`` u8, ``pose`` (4,4) f64, ``ground_mask`` bool, ``flow`` (N,3) f32,
    ``flow_is_valid``, ``flow_category_indices`` u8, ``flow_instance_id`` u32 and result datasets
    named after the checkpoint (dataprocess/extract_sca.py:76-93, tools/test/repack_h5_scania.py:23-36,
    downstream/eval_seg.py:205-225); frame order from ``index_total.pkl`` / ``index_eval.pkl``
    (lists of ``[scene_id, timestamp]``, tools/pkl_extract.py:5-19).
``pose1`` is the pose of the next timestamp in the same scene (the flow is pc0 -> pc1).

``h5py`` is not installed in the build image, so the scene files are opened with ``h5py`` when it is importable and with
this package's own dependency-free reader otherwise (``h5lite``: pinned against files written by the real HDF5 library,
tests/test_h5lite.py, tests/golden/h5).  Results a run could not put INTO a scene file (no HDF5 library to modify it with)
live in a result file beside it -- ``<dir>/results_h5/<res_name>/<scene_id>.h5``, same ``<timestamp>/<res_name>`` layout,
written by ``save.H5ResultSink`` -- and the loader looks there when the scene file does not hold ``<res_name>``.
``NpzDataset`` is this package's own container for the same dicts.
"""
from __future__ import annotations

import os
import pickle
from pathlib import Path

import numpy as np

FRAME_KEYS = ("pc0", "pose0", "pose1", "lidar_dt", "gm0", "flow", "flow_is_valid",
              "flow_category_indices", "flow_instance_id", "lidar_id")


class ListDataset:
    def __init__(self, frames):
        self.frames = list(frames)

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i]


POSE_KEY = "pose"            # the recorded pose of a sweep: dataset ``pose`` of its group (``pose0`` / ``pose1`` of an npz sweep)


def resolve_pose_key(pose_key: str | None) -> str:
    """``pose_key`` of the loaders: the name given, else the environment variable ``HIMO_POSE_KEY`` when set, else ``"pose"``"""
    key = pose_key if pose_key is not None else os.environ.get("HIMO_POSE_KEY") or POSE_KEY
    if not isinstance(key, str) or not key:
        raise ValueError(f"pose_key={pose_key!r}: the name of a stored [4, 4] pose")
    return key


def _no_pose(key: str, where: str) -> KeyError:
    return KeyError(f"{key}: {where} holds no such pose (`python -m himo_amd.odometry --data_dir ... --out_key {key}` writes estimated poses)")


class NpzDataset:
    """``<dir>/<scene_id>/<timestamp>.npz`` + ``index_total.pkl`` (same index format as the reference).
    ``pose_key`` (``resolve_pose_key``): with a name other than ``"pose"``, ``pose0`` is served from ``<pose_key>`` of the sweep's npz
    and ``pose1`` from ``<pose_key>_next`` (an npz sweep carries its own successor's pose); a sweep without them is a ``KeyError``."""

    def __init__(self, directory, vis_name: str = "", eval: bool = False, pose_key: str | None = None):  # noqa: A002
        self.directory = Path(directory)
        self.index = load_index(self.directory, eval=eval)
        self.vis_name = vis_name
        self.pose_key = resolve_pose_key(pose_key)

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        scene_id, ts = self.index[i]
        with np.load(self.directory / scene_id / f"{ts}.npz") as z:
            d = {k: z[k] for k in z.files}
        if self.pose_key != POSE_KEY:
            for frame_key, name in (("pose0", self.pose_key), ("pose1", self.pose_key + "_next")):
                if name not in d:
                    raise _no_pose(name, f"{scene_id}/{ts}")
                d[frame_key] = d[name]
        d["scene_id"], d["timestamp"] = scene_id, int(ts)
        return d

    @staticmethod
    def write(directory, frames, eval_subset=None):
        directory = Path(directory)
        index = []
        for f in frames:
            (directory / f["scene_id"]).mkdir(parents=True, exist_ok=True)
            arrays = {k: np.asarray(v) for k, v in f.items() if k not in ("scene_id", "timestamp")}
            np.savez(directory / f["scene_id"] / f"{f['timestamp']}.npz", **arrays)
            index.append([f["scene_id"], str(f["timestamp"])])
        with open(directory / "index_total.pkl", "wb") as fh:
            pickle.dump(index, fh)
        if eval_subset is not None:
            with open(directory / "index_eval.pkl", "wb") as fh:
                pickle.dump([index[i] for i in eval_subset], fh)


def h5_reader():
    """The module that opens scene files read-only: ``h5py`` when importable, else this package's ``h5lite``."""
    try:
        import h5py
        return h5py
    except ImportError:
        from . import h5lite
        return h5lite


def _open_h5(path):
    return h5_reader().File(path, "r")


def result_file(directory, res_name: str, scene_id: str) -> Path:
    """Where a scene's ``<res_name>`` results live when they could not be written into ``<scene_id>.h5`` itself."""
    return Path(directory) / "results_h5" / res_name / f"{scene_id}.h5"


def scene_stamp(in_scene) -> np.ndarray:
    """uint64[2] = (1 if the scene file held the array else 0, CRC-32 of its bytes): what ``save.H5ResultSink`` records beside a result
    it could not write into the scene file, and what ``HDF5Dataset`` compares the scene file's array with later."""
    import zlib
    if in_scene is None:
        return np.zeros(2, dtype=np.uint64)
    return np.array([1, zlib.crc32(np.ascontiguousarray(in_scene).view(np.uint8).reshape(-1))], dtype=np.uint64)


def allow_dropped_eval_default() -> bool:
    return os.environ.get("HIMO_ALLOW_DROPPED_EVAL", "0") not in ("", "0", "false", "False")


def load_index(directory, eval: bool = False) -> list:  # noqa: A002
    """``index_eval.pkl`` (when ``eval`` and present) else ``index_total.pkl``: a pickled list of ``[scene_id, timestamp]``
    pairs, timestamps as str or int (tools/pkl_extract.py:5-19 prints exactly this structure; the reference ships
    assets/docs/av2/index_eval.pkl: 70 frames of 13 scenes)."""
    directory = Path(directory)
    name = "index_eval.pkl" if eval and (directory / "index_eval.pkl").exists() else "index_total.pkl"
    with open(directory / name, "rb") as f:
        return [[str(s), str(t)] for s, t in pickle.load(f)]


# the frame keys ``save`` (network inference over a dataset) consumes: the sweep, its pose / time stamps, and the next sweep
SAVE_FIELDS = ("pc0", "pose0", "lidar_dt", "pose1", "pc1")


# what the segmentation evaluator reads beside its result names (downstream/eval_seg.py:219): labels and the mask, no points, no poses
SEG_FIELDS = ("flow_category_indices", "seg_valid")

# frame keys the loader derives itself (renamed datasets, the successor sweep's): never looked up in a group under these names
_LOADER_KEYS = frozenset(("scene_id", "timestamp", "pc0", "pose0", "pose1", "pc1", "gm0", "gm1", "lidar_dt", "flow_instance_id_next"))


# ... and the ones the evaluator reads (eval.py:282-310: the sweep, its poses and time stamps, the ground truth, the masks and ids -- not
# the next sweep's points); the estimate's key (``res_name``) joins them
EVAL_FIELDS = ("pc0", "pose0", "pose1", "lidar_dt", "gm0", "flow", "flow_is_valid", "flow_category_indices", "flow_instance_id")

# ... and the ones the scene-flow evaluator reads beside its result names (eval_flow.py): no time stamps, no instance ids
FLOW_EVAL_FIELDS = ("pc0", "pose0", "pose1", "gm0", "flow", "flow_is_valid", "flow_category_indices")


class _OpenFiles:
    """The most recently used scene files, kept OPEN (a walk reads every sweep of a scene in turn, and each sweep three times:
    as next, current and history): re-opening per item meant an mmap, a superblock parse and a group walk each time -- three
    quarters of an item's 3.8 ms.  Thread-safe; a file evicted while arrays still view its mapping
    (``h5lite.Dataset.view``) is left to the garbage collector."""

    def __init__(self, opener, keep: int = 8):
        import collections
        import threading
        self._open, self._keep = opener, keep
        self._files, self._lock = collections.OrderedDict(), threading.Lock()

    def get(self, path):
        key = str(path)
        with self._lock:
            got = self._files.get(key)
            if got is not None:
                self._files.move_to_end(key)
                return got[0]
        handle = self._open(path)                              # (outside the lock: another thread may open it too -- one of them stays)
        # an opener may hand back the mapping itself (h5py.File, h5lite.File) or a context manager that yields it
        f = handle if hasattr(handle, "__getitem__") else handle.__enter__()
        with self._lock:
            have = self._files.get(key)
            if have is not None:
                other, f = (f, handle), have[0]
            else:
                other = None
                self._files[key] = (f, handle)
                while len(self._files) > self._keep:
                    _, old = self._files.popitem(last=False)
                    self._close(old)
        if other is not None:
            self._close(other)
        return f

    @staticmethod
    def _close(entry):
        f, handle = entry
        try:
            if handle is f:
                f.close()
            else:
                handle.__exit__(None, None, None)
        except Exception:
            pass

    def forget(self, path):
        """close ``path`` if open (before something else rewrites the file)"""
        with self._lock:
            entry = self._files.pop(str(path), None)
        if entry is not None:
            self._close(entry)

    def close(self):
        with self._lock:
            files, self._files = list(self._files.values()), type(self._files)()
        for entry in files:
            self._close(entry)


class HDF5Dataset:
    """h5 scene files -> frame dicts (see module docstring for the provenance of the layout).

    ``pose1`` / ``pc1`` come from the next timestamp of the same scene in ``index_total.pkl``; a frame with no successor
    (the last sweep of a scene) has no ``pose1`` to remove ego motion with (save_zip.py:115), so it is dropped from the
    index at construction -- iterating the dataset never yields a frame the consumers cannot process.
    ``opener(path)`` returns the scene file as a read-only mapping ``{timestamp: {name: array-like}}`` (or a context manager
    yielding one); the default is ``h5py.File(path, "r")``, or ``h5lite.File(path)`` where h5py is not installed.  Scene files stay open between items
    (the ``keep_open`` most recent; ``close()`` / ``forget(scene_id)`` release them).
    ``fields``: the frame keys to read (None = everything the group holds; ``SAVE_FIELDS`` for inference -- labels, masks and
    ground-truth flow are then not touched).  ``zero_copy``: arrays the file stores as one plain run come back as READ-ONLY
    views of the file mapping (``h5lite`` only; consumers that stage frames into their own buffers, like
    ``feeder.SampleFeeder``, then copy each sweep once instead of twice).
    A name in ``fields`` that is none of the loader's own keys is served from the dataset of that name in the sweep's group when
    there is one, with its on-disk dtype (``seg_valid``, the segmentation results of downstream/eval_seg.py:219).
    A name ``<name>_next`` in ``fields`` is served from dataset ``<name>`` of the NEXT sweep's group when that group holds it (stored
    labels of both sweeps of a pair: ``seflow.fit --ssl_label <name>``).
    ``allow_dropped_eval`` (default: env ``HIMO_ALLOW_DROPPED_EVAL``, else False): see the KeyError below.
    ``need_next=False``: for consumers that read a sweep alone (no ``pose1`` / ``pc1``): every index entry stays, the last sweep
    of a scene included, and asking such an item for a successor's key is a KeyError.
    ``pose_key`` (``resolve_pose_key``: the name, else env ``HIMO_POSE_KEY``, else ``"pose"``): the dataset of a sweep's group that
    ``pose0`` is read from, and of its successor's group for ``pose1`` (``pose_odom`` of ``python -m himo_amd.odometry``); a sweep
    without it is a KeyError that names that program.  With ``"pose"`` every byte read is what it always was."""

    carries_next = True        # every item holds its successor's ``pc1`` / ``pose1``: a walk never reads item i + 1 for them

    def __init__(self, directory, vis_name="", eval: bool = False, n_frames: int = 2, opener=None,  # noqa: A002
                 allow_dropped_eval: bool | None = None, fields=None, zero_copy: bool = False, keep_open: int = 8,
                 need_next: bool = True, pose_key: str | None = None):
        self.pose_key = resolve_pose_key(pose_key)
        self._files = _OpenFiles(opener if opener is not None else _open_h5, keep=keep_open)
        # reader PROCESSES (feeder.ReaderPool) may inherit this object through fork(): h5lite holds a read-only file mapping and
        # nothing else; libhdf5's global state under h5py does not survive a fork with files open
        self.fork_safe = opener is None and h5_reader().__name__.rsplit(".", 1)[-1] == "h5lite"
        self.fields = None if fields is None else frozenset(fields)
        self.zero_copy = zero_copy
        self._result_choice = {}
        if allow_dropped_eval is None:
            allow_dropped_eval = allow_dropped_eval_default()
        self.directory = Path(directory)
        self.vis_name = list(vis_name) if isinstance(vis_name, (list, tuple)) else [vis_name]
        total = load_index(self.directory, eval=False)
        self._next = {}
        for (s0, t0), (s1, t1) in zip(total[:-1], total[1:]):
            if s0 == s1:
                self._next[(s0, t0)] = t1
        wanted = load_index(self.directory, eval=eval)
        if not need_next:
            self.index, self.dropped = [[s, t] for s, t in wanted], []
            return
        self.index = [[s, t] for s, t in wanted if (s, t) in self._next]
        # Entries without a successor sweep cannot be processed (no pose1: save_zip.py:115 / eval.py:284).  The last sweep
        # of every scene in index_total.pkl is such an entry and is dropped with a note; an entry of the EVAL list is a
        # sweep the leaderboard expects a result for (tools/test/score.py:572-588 counts it missing), so dropping one
        # silently would shrink the submission: that raises unless the caller opts in.
        self.dropped = [(s, t) for s, t in wanted if (s, t) not in self._next]
        from_eval_list = eval and (self.directory / "index_eval.pkl").exists()
        if self.dropped:
            msg = (f"{len(self.dropped)} of {len(wanted)} index entries have no successor sweep in their scene and cannot be "
                   f"processed: {self.dropped[:5]}{' ...' if len(self.dropped) > 5 else ''}")
            if from_eval_list and not allow_dropped_eval:
                raise KeyError("pose1: " + msg + " (index_eval.pkl names them; pass allow_dropped_eval=True / --allow_dropped_eval / HIMO_ALLOW_DROPPED_EVAL=1 to skip them)")
            import warnings
            warnings.warn(msg, stacklevel=2)

    def __len__(self):
        return len(self.index)

    def scene_path(self, scene_id: str) -> Path:
        return self.directory / f"{scene_id}.h5"

    def close(self):
        self._files.close()

    def forget(self, scene_id: str):
        """release the open handles of a scene (a writer is about to modify its file, or the result file beside it) and what
        was decided about where its results live"""
        self._files.forget(self.scene_path(scene_id))
        for key in [k for k in self._result_choice if k[1] == scene_id]:
            self._files.forget(result_file(self.directory, key[0], scene_id))
            del self._result_choice[key]

    def _array(self, ds):
        if self.zero_copy:
            view = getattr(ds, "view", None)
            if view is not None:
                a = view()
                if a is not None:
                    return a
        return np.asarray(ds[:])

    def _result_source(self, name: str, scene_id: str):
        """Which file answers for ``<res_name>`` of a scene when BOTH the scene file and a result file beside it
        (``result_file``) exist.  This package's in-place writer removes the side entries it supersedes
        (``save.H5ResultSink._supersede_beside``), but another tool -- the reference's ``save.py``, h5py, h5copy -- that writes
        ``<res_name>`` into the scene file later knows nothing of the side file: preferring it blindly would score stale flows.
        "side": the side file is the newer file.  "scene-newer": the scene file was modified after it -- which says nothing about
        ``<res_name>`` (a touch, a copy, another result name written in place): ``read`` then decides per sweep from the stamp the
        side writer left (``scene_stamp``: was the in-scene array there, and with which bytes, when the side result was written)."""
        key = (name, scene_id)
        got = self._result_choice.get(key)
        if got is None:
            side = result_file(self.directory, name, scene_id)
            got = "scene"
            if side.exists():
                got = "side"
                scene = self.scene_path(scene_id)
                if scene.exists() and scene.stat().st_mtime_ns > side.stat().st_mtime_ns:
                    got = "scene-newer"
            self._result_choice[key] = got
        return got

    def __getitem__(self, i):
        return self.read(i)

    def _pose(self, g, scene_id, ts):
        if self.pose_key != POSE_KEY and self.pose_key not in g:
            raise _no_pose(self.pose_key, f"{scene_id}/{ts}")
        return np.asarray(g[self.pose_key][:])

    def read(self, i, fields=None):
        """item ``i`` restricted to ``fields`` (None: the dataset's own ``fields``) -- a caller that needs only part of a frame it
        has no other use for (the training loop's history sweep: ``pc0`` and ``pose0``) does not touch the rest"""
        scene_id, ts = self.index[i]
        want = self.fields if fields is None else frozenset(fields)
        need = (lambda k: True) if want is None else want.__contains__
        f = self._files.get(self.scene_path(scene_id))
        g = f[ts]
        d = {"scene_id": scene_id, "timestamp": int(ts)}
        if need("pc0"):
            d["pc0"] = self._array(g["lidar"])
        if need("pose0"):
            d["pose0"] = self._pose(g, scene_id, ts)
        if need("lidar_dt"):
            d["lidar_dt"] = self._array(g["lidar_dt"]) if "lidar_dt" in g else np.zeros(g["lidar"].shape[0], np.float32)
        if need("gm0") and "ground_mask" in g:
            d["gm0"] = np.asarray(g["ground_mask"][:]).astype(bool)        # the loader's rename
        for k in ("flow", "flow_is_valid", "flow_category_indices", "flow_instance_id", "lidar_id", "ego_motion"):
            if need(k) and k in g:
                d[k] = self._array(g[k])
        for name in self.vis_name:
            if name and name != "raw" and need(name):
                src = self._result_source(name, scene_id)
                if src != "scene":
                    r = self._files.get(result_file(self.directory, name, scene_id))
                    in_side = ts in r and name in r[ts]
                    if in_side and src == "scene-newer" and name in g:
                        stamp = np.asarray(r[ts][name + "@scene"][:]) if (name + "@scene") in r[ts] else None
                        if stamp is not None and np.array_equal(stamp, scene_stamp(g[name][:])):
                            d[name] = self._array(r[ts][name])         # the in-scene array is the one the side result replaced: still older
                        else:
                            import warnings
                            warnings.warn(f"{scene_id}.h5 was modified after the result file beside it ({result_file(self.directory, name, scene_id)}) "
                                          f"and its '{name}' for sweep {ts} is not the one that file replaced: using the scene file's; delete or "
                                          f"merge the side file", stacklevel=2)
                    elif in_side:
                        d[name] = self._array(r[ts][name])
                if name not in d and name in g:
                    d[name] = self._array(g[name])
        if want is not None:                                   # any other dataset of the sweep's group, asked for by its own name
            for k in sorted(want - _LOADER_KEYS):
                if k not in d and k in g:
                    d[k] = self._array(g[k])
        # any other requested field ``<name>_next``: dataset ``<name>`` of the successor's group (stored labels of the next sweep)
        others_next = [] if want is None else sorted(k for k in want - _LOADER_KEYS if k.endswith("_next") and len(k) > 5 and k not in d)
        if not (any(need(k) for k in ("pose1", "pc1", "gm1", "flow_instance_id_next")) or others_next):
            return d
        nxt = f[self._next[(scene_id, ts)]]
        if need("pose1"):
            d["pose1"] = self._pose(nxt, scene_id, self._next[(scene_id, ts)])
        if need("pc1"):
            d["pc1"] = self._array(nxt["lidar"])
        if need("gm1") and "ground_mask" in nxt:               # the label generator needs both sweeps' ground masks (seflow/ssl_label.py)
            d["gm1"] = np.asarray(nxt["ground_mask"][:]).astype(bool)
        if need("flow_instance_id_next") and "flow_instance_id" in nxt:        # the training loop clusters both sweeps (seflow/fit.py)
            d["flow_instance_id_next"] = self._array(nxt["flow_instance_id"])
        for k in others_next:
            if k[:-5] in nxt:
                d[k] = self._array(nxt[k[:-5]])
        return d


def open_dataset(directory, vis_name="", eval: bool = False, allow_dropped_eval: bool | None = None, pose_key: str | None = None,  # noqa: A002
                 **h5_options):
    """The frame source behind ``HDF5Dataset(dir, vis_name=<res>, eval=True)`` at save_zip.py:111 / eval.py:279: the h5
    scene files when the directory holds them, this package's npz container (``NpzDataset.write``) when it holds that.
    ``allow_dropped_eval`` only concerns h5 scene files: an npz frame carries its own ``pose1`` / ``pc1``, so no entry of
    an npz index can lack a successor.  ``pose_key``: the stored pose both loaders serve ``pose0`` / ``pose1`` from
    (``resolve_pose_key``: None = env ``HIMO_POSE_KEY`` when set, else ``"pose"``)."""
    directory = Path(directory)
    if any(directory.glob("*/*.npz")) and not any(directory.glob("*.h5")):
        return NpzDataset(directory, vis_name=vis_name, eval=eval, pose_key=pose_key)
    return HDF5Dataset(directory, vis_name=vis_name, eval=eval, allow_dropped_eval=allow_dropped_eval, pose_key=pose_key, **h5_options)
