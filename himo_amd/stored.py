"""What the box / track programs (``ground_seg``, ``raymap``, ``accumulate``, ``rigid_refine``, ``box_fit``, ``eval_box``, ``track``,
``track_flow``, ``eval_xsensor``) share about the named arrays stored beside the sweeps -- ``<timestamp>/<key>`` of a scene file, or a
key of a sweep's npz:

* the names: the ``--res_names`` split (``result_names``);
* reading without the sweep: which keys an item holds (``present``) and the arrays themselves (``arrays``);
* the refusals the programs word alike (``check_box_rows``, ``check_track_rows``, ``check_point_labels``, ``check_pose``,
  ``at_least_one``, ``check_motion_min``);
* writing: the HDF5 library that can modify a scene file, or the refusal (``h5_module``), the replace-a-key loop on an open file
  (``put_keys``), the npz update (``put_npz``) and the sink that holds a scene's arrays back until the scene is done (``KeySink``);
* the tables' ``fmt`` and ``ratio``.

Flow-shaped results -- ``(N, 3)`` float32 rows of ``pc0`` -- go through ``save.H5ResultSink`` / ``save.NpzResultSink``, which write with
``put_keys`` / ``put_npz`` too.  Nothing here touches the device.
"""
from __future__ import annotations

import math
import os
from pathlib import Path

import numpy as np


# ---- the names ---------------------------------------------------------------------------------------------------------------------------
def result_names(res_names, raw_ok: bool) -> list:
    """``--res_names``: a comma-separated string or a sequence -> the names, empties dropped; none, or one twice, is refused"""
    names = [s for s in (res_names.split(",") if isinstance(res_names, str) else list(res_names)) if s]
    if not names or len(set(names)) != len(names):
        raise ValueError(f"res_names={res_names!r}: one or more different names" + (" ('raw' = the points as recorded)" if raw_ok else ""))
    return names


# ---- reading without the sweep -----------------------------------------------------------------------------------------------------------
def _is_npz(ds) -> bool:
    from .dataset import NpzDataset
    return isinstance(ds, NpzDataset)


def present(ds, i, names) -> set:
    """which of ``names`` item ``i`` of the dataset holds, without reading the sweep"""
    if _is_npz(ds):
        scene_id, ts = ds.index[i]
        with np.load(ds.directory / scene_id / f"{ts}.npz") as z:
            return set(z.files) & set(names)
    return set(ds.read(i, fields=tuple(names))) & set(names)


def arrays(ds, i, keys) -> dict:
    """the stored arrays ``keys`` of item ``i`` that exist, read without the sweep itself"""
    if _is_npz(ds):
        scene_id, ts = ds.index[i]
        with np.load(ds.directory / scene_id / f"{ts}.npz") as z:
            return {k: np.asarray(z[k]) for k in keys if k in z.files}
    d = ds.read(i, fields=tuple(keys))
    return {k: np.asarray(d[k]) for k in keys if k in d}


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def check_box_rows(b, key: str, where: str, most: int | None) -> None:
    """float32 [F][12] rows, at most ``most`` of them (None: any number)"""
    if b.ndim != 2 or b.shape[1] != 12 or b.dtype != np.float32:
        raise ValueError(f"{key}: {where} holds {b.dtype} {b.shape}, not float32 [F][12] box rows")
    if most is not None and len(b) > most:
        raise ValueError(f"{key}: {where} holds {len(b)} boxes: at most {most} per sweep")


def check_track_rows(t, b, key: str, box_key: str, where: str, hint: str) -> None:
    """``t``: the stored track rows of the boxes ``b``; ``hint``: the command that writes fresh ones"""
    if t.ndim != 2 or t.shape[1] != 6 or t.dtype != np.float64:
        raise ValueError(f"{key}: {where} holds {t.dtype} {t.shape}, not float64 [F][6] track rows")
    if len(t) != len(b):
        raise ValueError(f"{key}: {where} holds {len(t)} rows for the {len(b)} boxes of {box_key}: stale tracks (run `{hint}` after box_fit)")


def check_point_labels(lab, key: str, where: str, rows: int | None = None) -> None:
    """one integer per point; ``rows``: the sweep's number of points, where the caller knows it"""
    if lab.ndim != 1 or lab.dtype.kind not in "iu" or (rows is not None and len(lab) != rows):
        raise ValueError(f"{key}: {where} holds {lab.dtype} {lab.shape}, not one integer per point" +
                         ("" if rows is None else f" of its {rows} points"))


def check_pose(have: dict, where: str) -> None:
    if "pose0" not in have or np.asarray(have["pose0"]).shape != (4, 4):
        raise ValueError(f"pose0: {where} holds no [4, 4] pose")


def at_least_one(name: str, v, what: str = "") -> None:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name}={v!r}: at least 1{what}")


def check_motion_min(v) -> None:
    if not (math.isfinite(v) and v >= 0):
        raise ValueError(f"motion_min={v}: finite and >= 0")


# ---- writing -----------------------------------------------------------------------------------------------------------------------------
def h5_module(what: str):
    """the module that can open a scene file with ``"a"`` (``save.h5_writer``), or the refusal that begins with ``what``"""
    from . import save
    mod, how = save.h5_writer()
    if mod is None:
        raise RuntimeError(f"{what} needs an HDF5 library (h5py, or libhdf5 for himo_amd.h5c; HIMO_LIBHDF5 names one): {how}")
    return mod


def put_keys(h, ts, arrays: dict) -> None:
    """``arrays`` into group ``ts`` of the open scene file ``h``; a key the group holds already is replaced"""
    g = h[str(ts)]
    for key, a in arrays.items():
        if key in g:
            del g[key]
        g.create_dataset(key, data=a)


def put_npz(root, scene_id: str, ts, arrays: dict) -> None:
    """``arrays``, with their own dtypes, into a sweep's npz beside what it holds.  Written aside, then renamed: a reader thread may be
    reading this very file"""
    path = Path(root) / scene_id / f"{ts}.npz"
    with np.load(path) as z:
        have = {k: z[k] for k in z.files}
    have.update(arrays)
    tmp = path.with_name(path.stem + ".writing.npz")
    np.savez(tmp, **have)
    os.replace(tmp, path)


class KeySink:
    """``put(scene_id, ts, key, array)`` for the arrays a program stores beside the sweeps of ``ds`` (opened on ``root``).  Into the npz
    container an array is written at once.  Into scene files a scene's arrays are held back until ``put`` names another scene or
    ``close()`` is called; then the dataset lets go of the file (``ds.forget``), the file is opened once and every sweep's arrays go in
    through ``put_keys`` -- so it is never open for reading and for writing at the same time.  Constructing one for scene files looks
    for the HDF5 library (``h5_module``, whose refusal begins with ``what``): do it in the refusal pass."""

    def __init__(self, ds, root, what: str | None = None):
        self.ds, self.root = ds, Path(root)
        self._mod = None if _is_npz(ds) else h5_module(what or f"writing into the scene files of {root}")
        self._scene, self._pending = None, {}

    def put(self, scene_id: str, ts, key: str, array) -> None:
        if self._mod is None:
            put_npz(self.root, scene_id, ts, {key: array})
            return
        if scene_id != self._scene:
            self.close()
            self._scene = scene_id
        self._pending.setdefault(str(ts), {})[key] = array

    def close(self) -> None:
        if self._pending:
            self.ds.forget(self._scene)
            with self._mod.File(self.ds.scene_path(self._scene), "a") as h:
                for ts, arrays in self._pending.items():
                    put_keys(h, ts, arrays)
            self._pending = {}


# ---- the tables --------------------------------------------------------------------------------------------------------------------------
def fmt(v, spec: str = ".3f") -> str:
    return "-" if v is None else format(v, spec)


def ratio(a, b):
    return a / b if b else None
