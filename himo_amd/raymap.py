"""The free-space labeller: per-point ``0 = static / > 0 = dynamic cluster id`` labels from the space OTHER sweeps saw through,
written into the scene files so that ``seflow.fit --ssl_label ray_label`` trains on them (the labels of ``ssl_label=seflow_auto``,
``himo_amd/seflow/ssl_label.py``, compare two sweeps by nearest neighbours: anything slower than about 3.5 m/s is static there by
construction, and only the non-overlapping sliver of a moving object is labelled).

PARITY UNPINNED.  The reference's generator is in its absent ``OpenSceneFlow`` submodule; only the option's name is in the tree.
This stage follows the build's own written rule, below, and is checked bit for bit against a numpy restatement of it
(``tests/raymap_ref.py``), never against the reference.  It makes no claim about the reference's labels.

The rule -- "free-space ray map, v1" (normative)
=================================================
Designed so that the device and numpy decide every voxel and every point identically.  All float arithmetic is float32 and every
operation rounds on its own (``himo_amd/csrc/raymap.hip`` is built with ``-ffp-contract=off``); everything after rule A is integer.

Parameters (``RaymapParams``, mirrored as ``himo_raymap_params``): grid minimum ``(x0, y0, z0)`` (-51.2, -51.2, -3.0), ``voxel`` 0.2 m,
``nx, ny, nz`` 512, 512, 30, ``guard`` 2, ``min_votes`` 2.  The struct carries ``scale = (float)(256.0 / voxel)``, computed in double on
the host.  Admitted: finite floats, voxel > 0, 1 <= nx, ny <= 1024, 1 <= nz <= 64, nx*ny*nz <= 2^24, 0 <= guard <= 8,
1 <= min_votes <= 16; anything else is refused with a non-zero status and no write.

A. Quantisation.  A coordinate ``c`` on an axis with grid minimum ``m`` becomes ``f = (c - m) * scale``: one subtraction, one
   multiplication.  A point is UNUSABLE if any ``f`` is non-finite or ``|f| >= 4194304.0f``.  Otherwise ``u = (int)floorf(f)``, in
   sub-voxel units of 256 per voxel; its voxel index on that axis is ``u >> 8`` (arithmetic shift).  A voxel is IN GRID if all three
   indices are inside ``[0, n)``.
B. Rays.  A ray goes from an origin ``o`` to an end point ``p``, a return of a neighbour sweep already moved into the map frame, and
   carries a slot ``s`` in 0..15: the neighbour sweep it belongs to.  A ray takes part only if both ``o`` and ``p`` are usable and its
   slot byte is not 255.  With ``A, B`` the quantised origin and end, ``v = A >> 8`` the start voxel and ``e = B >> 8`` the end voxel,
   per axis: ``d = B - A``, ``step = sign(d)``, ``den = |d|``, ``r = |e - v|`` (the steps still owed on that axis) and
   ``num = |(v + (step > 0 ? 1 : 0)) * 256 - A|``.
C. Walk.  While any ``r > 0``: (1) visit the current voxel; (2) among the axes with ``r > 0`` take the one with the smallest
   ``num/den``, compared by cross-multiplication in 64-bit integers, ``num_i * den_j < num_j * den_i``, a tie to the lowest axis
   index; (3) step that axis: ``v += step``, ``num += 256``, ``r -= 1``.  The end voxel ``e`` is never visited by the walk, which takes
   exactly ``sum |e - v|`` steps.  The kernel may stop early once the walk has left the grid on the axis it is stepping along, in the
   direction of that step: the set of voxels marked does not change.  All products stay below 2^48.
D. Marks.  The map is one uint32 word per voxel, laid out ``[nz][ny][nx]``.  A visited voxel gets FREE bit ``s`` if it is in grid and
   its Chebyshev index distance to ``e`` is ``> guard``; the end voxel gets HIT bit ``16 + s`` if it is in grid.  Marks are OR-ed in,
   so they are order-independent; successive carve calls accumulate; the caller clears the map.
E. Query.  For the word ``w`` of a target point's voxel, ``fv = popcount((w & 0xFFFF) & ~(w >> 16))`` -- the sweeps that saw through
   the voxel and did not also return from it -- and ``hv = popcount(w >> 16)``.  The point is DYNAMIC iff its skip byte is 0, it is
   usable, its voxel is in grid, ``fv >= min_votes`` and ``fv > hv``.  ``fv`` and ``hv`` are 0 for a skipped, an unusable or an
   out-of-grid point.
F. Labels of a target sweep (``cluster_labels``; host glue on existing kernels).  DBSCAN through ``ssl_label.dbscan`` with its ``EPS``
   and ``MIN_PTS`` over the target's points that are not ground, are finite and lie inside ``RANGE_NET`` in x and y.  A DBSCAN
   cluster with ``n`` points, of which ``k`` are DYNAMIC, is a dynamic cluster iff ``k >= 3`` and ``4*k >= n`` (``min_dynamic = 3``,
   ``share = (1, 4)``).  Dynamic clusters are renumbered 1..K in ascending order of their DBSCAN id; every other point is 0,
   including DYNAMIC points that DBSCAN left as noise.  ``cluster_labels(cluster="hdbscan", min_cluster_size=, min_samples=)`` /
   ``--cluster hdbscan`` takes the clusters from ``ssl_label.hdbscan`` ("HDBSCAN, v1"; parity unpinned) over the same points instead;
   the default is DBSCAN, and nothing else of this rule changes.
G. The map of a target sweep ``t`` in a scene (``dynamic_flags``).  The neighbours are the sweeps ``t-window .. t+window`` of the same
   scene without ``t``, clipped to the scene (``window`` 5: at most 10 neighbours; admitted up to 8).  Neighbour ``k`` gets slot = its
   rank among the neighbours; its points are moved with ``T = inv(pose_t) @ pose_k``, computed in float64 on the host, rounded to
   float32 and applied by ``himo_rigid_transform``; the ray origin is ``(float)T[:3, 3]``.  Ground returns of the neighbours DO cast
   rays (they carve the space above the road); target ground points are never DYNAMIC: they are passed as skip.

A slot byte in 16..254 is a refused call, found on the device (``himo_raymap_carve`` is asynchronous): the call marks nothing and the
refusal is reported by ``status()`` -- ``himo_raymap_status`` -- which waits for the stream (include/himo_amd.h).

Known limits.  The origin is the sweep's frame origin: the per-LiDAR centres of the Scania files (``lidar_center`` /
``SensorsCenter``) are not used.  There is no sub-sweep timing.  There is no neighbourhood inflation beyond ``guard``.  There is no
free-space evidence across scenes.  Every target gets a fresh map from at most 10 neighbours: no map persists along the drive.

Where the defaults come from.  A numpy prototype of this rule was run on a ray-cast toy scene, on the CPU only: sweeps of 32 beams x
900 azimuths over a ground plane, a wall at 8 m and a 4 x 2 x 1.6 m box, the map carved from 10 neighbour sweeps.  With ``guard`` 2
and ego speed 5 m/s the rule flagged 3.1 % of the wall points and 93.6 % of the points of the box moving at 10 m/s.  A parked box was
tried only with ``guard`` 1, at ego speed 10 m/s: 4.8 % of its points were flagged, and 6.5 % of the wall.  Without the ``fv > hv``
clause the wall share was 3.7 % (guard 2) to 13 % (guard 1).  NOTHING HAS BEEN MEASURED ON FIELD DATA.

The program: ``python -m himo_amd.raymap --data_dir D [--window 5] [--key ray_label] [--dynamic_key ray_dynamic] [--overwrite]
[--cluster dbscan|hdbscan [--min_cluster_size M --min_samples K]]`` walks
the ``<scene>.h5`` files of ``D``, reads ``lidar``, ``pose`` and ``ground_mask`` of every sweep (``python -m himo_amd.ground_seg``
writes the masks) and writes ``<timestamp>/<key>`` (int32, rule F) and ``<timestamp>/<dynamic_key>`` (uint8, the flags of rule E)
INTO the scene file.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import time
from pathlib import Path

import numpy as np

MIN_DYNAMIC, SHARE = 3, (1, 4)
MAX_WINDOW = 8


class RaymapParams(ctypes.Structure):
    """mirror of ``himo_raymap_params`` (include/himo_amd.h); ``scale`` follows from ``voxel``"""
    _fields_ = [("x0", ctypes.c_float), ("y0", ctypes.c_float), ("z0", ctypes.c_float), ("voxel", ctypes.c_float), ("scale", ctypes.c_float),
                ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("guard", ctypes.c_int32), ("min_votes", ctypes.c_int32)]

    def __init__(self, x0=-51.2, y0=-51.2, z0=-3.0, voxel=0.2, nx=512, ny=512, nz=30, guard=2, min_votes=2):
        v = float(np.float32(voxel))
        with np.errstate(all="ignore"):
            scale = float(np.float32(np.float64(256.0) / np.float64(v))) if v != 0.0 else float("inf")
        super().__init__(x0, y0, z0, voxel, scale, nx, ny, nz, guard, min_votes)

    @property
    def shape(self) -> tuple:
        return int(self.nz), int(self.ny), int(self.nx)


_REFUSED = ("raymap: parameters outside finite floats, voxel > 0, 1 <= nx, ny <= 1024, 1 <= nz <= 64, nx*ny*nz <= 2^24, "
            "0 <= guard <= 8, 1 <= min_votes <= 16")


def map_bytes(params: RaymapParams) -> int:
    from . import _lib
    return int(_lib.load().himo_raymap_map_bytes(ctypes.addressof(params)))


def new_map(params: RaymapParams, device=None):
    """a cleared map: an int32 device tensor [nz, ny, nx] (the bits of the uint32 words of rule D)"""
    import torch
    from . import _lib
    if map_bytes(params) == 0:
        raise ValueError(_REFUSED)
    return torch.zeros(params.shape, dtype=torch.int32, device=device if device is not None else _lib.require_gpu())


def _points(pts):
    import torch
    if pts.dim() != 2 or pts.shape[1] not in (3, 4) or pts.dtype != torch.float32 or not pts.is_contiguous():
        raise ValueError(f"points are contiguous float32 rows of 3 or 4 columns, not {tuple(pts.shape)} {pts.dtype}")
    return pts


def _the_map(grid, params):
    import torch
    if grid.dtype != torch.int32 or tuple(grid.shape) != params.shape or not grid.is_contiguous():
        raise ValueError(f"the map is a contiguous int32 tensor {params.shape}, not {tuple(grid.shape)} {grid.dtype}")
    return grid


def carve(pts, slot, origins, params: RaymapParams, grid):
    """Launch ``himo_raymap_carve`` on the current stream: OR the marks of the rays ``origins[slot[i]] -> pts[i]`` into ``grid``
    (``new_map``).  ``pts``: device float32 [n, 3 or 4] in the map's frame, ``slot``: device uint8 [n] (0..15, 255 = no part),
    ``origins``: device float32 [16, 3].  Asynchronous; a slot byte in 16..254 refuses the whole call ON THE DEVICE: see ``status``."""
    import torch
    from . import _lib
    _points(pts), _the_map(grid, params)
    if slot.dtype != torch.uint8 or slot.shape != (pts.shape[0],) or not slot.is_contiguous():
        raise ValueError(f"slots are contiguous uint8 [{pts.shape[0]}], not {tuple(slot.shape)} {slot.dtype}")
    if origins.dtype != torch.float32 or tuple(origins.shape) != (16, 3) or not origins.is_contiguous():
        raise ValueError(f"origins are contiguous float32 [16, 3], not {tuple(origins.shape)} {origins.dtype}")
    st = _lib.load().himo_raymap_carve(int(pts.shape[0]), _lib.ptr(pts), int(pts.shape[1]), _lib.ptr(slot), _lib.ptr(origins),
                                       ctypes.addressof(params), _lib.ptr(grid), _lib.stream_handle())
    _lib.check(st, "himo_raymap_carve")
    return grid


def status() -> None:
    """Wait for the current stream and raise ValueError if a ``carve`` call on this device was refused for a slot byte in 16..254
    since the last ``status()`` (such a call marked nothing)."""
    from . import _lib
    _lib.check(_lib.load().himo_raymap_status(_lib.stream_handle()), "himo_raymap_carve: a slot byte in 16..254")


def query(pts, params: RaymapParams, grid, skip=None):
    """Launch ``himo_raymap_query`` on the current stream: (dynamic, fv, hv), uint8 device tensors [n], for the points ``pts`` (device
    float32 [n, 3 or 4] in the map's frame).  ``skip``: device uint8 / bool [n], non-zero = never DYNAMIC.  Asynchronous."""
    import torch
    from . import _lib
    _points(pts), _the_map(grid, params)
    n = int(pts.shape[0])
    if skip is not None:
        skip = skip.to(torch.uint8).contiguous()
        if skip.shape != (n,):
            raise ValueError(f"skip is [{n}], not {tuple(skip.shape)}")
    dyn, fv, hv = (torch.empty(n, dtype=torch.uint8, device=pts.device) for _ in range(3))
    st = _lib.load().himo_raymap_query(n, _lib.ptr(pts), int(pts.shape[1]), _lib.ptr(skip), ctypes.addressof(params), _lib.ptr(grid),
                                       _lib.ptr(fv), _lib.ptr(hv), _lib.ptr(dyn), _lib.stream_handle())
    _lib.check(st, "himo_raymap_query")
    return dyn, fv, hv


def _device_points(pc, dev):
    import torch
    t = pc if isinstance(pc, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32))
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"points are rows of x, y, z[, ...], not {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float32)[:, :3].contiguous()


def neighbours(t: int, n_sweeps: int, window: int = 5) -> list:
    """rule G: the neighbour sweeps of target ``t``, in slot order"""
    if not 0 <= int(window) <= MAX_WINDOW:
        raise ValueError(f"window={window}: 0..{MAX_WINDOW} (a map word holds 16 sweeps)")
    if not 0 <= t < n_sweeps:
        raise IndexError(f"target sweep {t} of {n_sweeps}")
    return [k for k in range(max(0, t - window), min(n_sweeps, t + window + 1)) if k != t]


def dynamic_flags(sweeps, poses, grounds, t: int, params: RaymapParams | None = None, window: int = 5, return_moved: bool = False,
                  grid=None):
    """Rule G for target sweep ``t`` of one scene: (dynamic, fv, hv), uint8 device tensors over the target's points.  ``sweeps``: the
    scene's sweeps in order, (n, >= 3) float32 arrays or tensors in their own frames; ``poses``: their 4x4 world poses; ``grounds``:
    their ground masks (only the target's is used).  ``return_moved``: also the list of the neighbours' points moved into the target's
    frame, device float32 [n_k, 3] in slot order.  ``grid``: a map to clear and use (``new_map``).  Asynchronous."""
    import torch
    from . import _lib
    from .seflow.ssl_label import _moved
    dev = _lib.require_gpu()
    params = params if params is not None else RaymapParams()
    nb = neighbours(int(t), len(sweeps), window)
    grid = new_map(params, dev) if grid is None else _the_map(grid, params).zero_()
    target = _device_points(sweeps[t], dev)
    g = grounds[t]
    skip = (g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g).astype(np.uint8))).to(device=dev, dtype=torch.uint8)
    inv_t = np.linalg.inv(np.asarray(poses[t], dtype=np.float64))
    origins = np.zeros((16, 3), dtype=np.float32)
    moved = []
    for s, k in enumerate(nb):
        T = (inv_t @ np.asarray(poses[k], dtype=np.float64)).astype(np.float32)
        origins[s] = T[:3, 3]
        moved.append(_moved(_device_points(sweeps[k], dev), T))
    if moved:
        pts = torch.cat(moved, dim=0)
        slot = torch.cat([torch.full((m.shape[0],), s, dtype=torch.uint8, device=dev) for s, m in enumerate(moved)])
        carve(pts, slot, torch.from_numpy(origins).to(dev), params, grid)
    out = query(target, params, grid, skip)
    return out + (moved,) if return_moved else out


def cluster_labels(points, ground, dynamic, min_dynamic: int = MIN_DYNAMIC, share: tuple = SHARE, return_ids: bool = False,
                   cluster: str = "dbscan", min_cluster_size: int | None = None, min_samples: int | None = None):
    """Rule F: int32 device labels [n] of a target sweep from its points (device (n, >= 3) float32), its ground mask and the DYNAMIC
    flags of rule E.  ``return_ids``: also the cluster ids the labels were derived from.  ``cluster``: "dbscan" (the default) or
    "hdbscan" with ``min_cluster_size`` / ``min_samples`` (``ssl_label.HDB_MIN_CLUSTER`` / ``HDB_MIN_SAMPLES`` when None).  Waits for
    the cluster count."""
    import torch
    from . import _lib
    from .seflow.ssl_label import CLUSTERINGS, EPS, HDB_MIN_CLUSTER, HDB_MIN_SAMPLES, MIN_PTS, RANGE_NET, cluster_points
    if cluster not in CLUSTERINGS:
        raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
    dev = _lib.require_gpu()
    p = _device_points(points, dev)
    n = p.shape[0]
    up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)
    dyn = up(dynamic).reshape(-1) != 0
    if n == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return (z, z.clone()) if return_ids else z
    skip = (up(ground).reshape(-1) != 0) | ~torch.isfinite(p).all(dim=1) | ~(p[:, :2].abs().amax(dim=1) <= RANGE_NET)
    ids, _ = cluster_points(p, skip, cluster, EPS, MIN_PTS, HDB_MIN_CLUSTER if min_cluster_size is None else min_cluster_size,
                            HDB_MIN_SAMPLES if min_samples is None else min_samples)
    idx = ids.to(torch.int64)
    top = int(idx.max().item()) + 1
    size = torch.bincount(idx, minlength=top)
    hits = torch.bincount(idx[dyn], minlength=top)
    moving = (hits >= int(min_dynamic)) & (int(share[1]) * hits >= int(share[0]) * size)
    moving[0] = False                                               # noise and the points that took no part
    renumber = torch.cumsum(moving.to(torch.int64), 0) * moving
    labels = renumber[idx].to(torch.int32)
    return (labels, ids) if return_ids else labels


# --------------------------------------------------------------------------------------------------------------------------
# the program
# --------------------------------------------------------------------------------------------------------------------------
def label_scene(path, params: RaymapParams | None = None, window: int = 5, key: str = "ray_label", dynamic_key: str = "ray_dynamic",
                overwrite: bool = False, opener=None, cluster: str = "dbscan", min_cluster_size: int | None = None,
                min_samples: int | None = None) -> dict:
    """One scene file: read ``lidar``, ``pose`` and ``ground_mask`` of every sweep, compute the labels of every sweep, and only once
    the reads are done open the file for modification and write ``<timestamp>/<key>`` (int32) and ``<timestamp>/<dynamic_key>``
    (uint8).  Returns {"sweeps", "points", "dynamic", "clusters", "seconds"} (seconds: upload, carving, clustering and the copy back;
    no file time)."""
    import torch
    from . import _lib
    from .dataset import h5_reader
    from .stored import h5_module, put_keys
    path = Path(path)
    params = params if params is not None else RaymapParams()
    neighbours(0, 1, window)
    clouds, poses, grounds = [], [], []
    with h5_reader().File(path, "r") as f:
        stamps = sorted(f.keys())
        have = [ts for ts in stamps if key in f[ts] or dynamic_key in f[ts]]
        if have and not overwrite:
            raise FileExistsError(f"{path}: {len(have)} of {len(stamps)} sweeps already hold '{key}' or '{dynamic_key}' (--overwrite replaces them)")
        for ts in stamps:
            g = f[ts]
            if "ground_mask" not in g:
                raise KeyError(f"ground_mask: {path} sweep {ts} has no ground mask (`python -m himo_amd.ground_seg` writes them)")
            clouds.append(np.asarray(g["lidar"][:], dtype=np.float32))
            poses.append(np.asarray(g["pose"][:], dtype=np.float64))
            grounds.append(np.asarray(g["ground_mask"][:]).astype(np.uint8))
    dev = _lib.require_gpu()
    t0 = time.perf_counter()
    labels, flags = [], []
    with torch.cuda.device(dev):
        on_dev = [_device_points(c, dev) for c in clouds]
        masks = [torch.from_numpy(g).to(dev) for g in grounds]
        grid = new_map(params, dev)
        for t in range(len(stamps)):
            dyn, _, _ = dynamic_flags(on_dev, poses, masks, t, params, window, grid=grid)
            lab = cluster_labels(on_dev[t], masks[t], dyn, cluster=cluster, min_cluster_size=min_cluster_size, min_samples=min_samples)
            labels.append(lab.cpu().numpy().astype(np.int32))
            flags.append(dyn.cpu().numpy().astype(np.uint8))
    seconds = time.perf_counter() - t0
    if opener is None:
        mod = h5_module(f"{path}: writing '{key}' into a scene file")
        opener = lambda p: mod.File(p, "a")                               # noqa: E731
    with opener(path) as f:
        for ts, lab, dyn in zip(stamps, labels, flags):
            put_keys(f, ts, {key: lab, dynamic_key: dyn})
    return {"sweeps": len(stamps), "points": int(sum(len(x) for x in labels)), "dynamic": int(sum(int(x.sum()) for x in flags)),
            "clusters": int(sum(int(x.max(initial=0)) for x in labels)), "seconds": seconds}


def main(data_dir: str, window: int = 5, key: str = "ray_label", dynamic_key: str = "ray_dynamic", overwrite: bool = False,
         params: RaymapParams | None = None, cluster: str = "dbscan", min_cluster_size: int | None = None,
         min_samples: int | None = None) -> dict:
    """The program.  Under ``torchrun`` (one rank per GPU) the scenes are dealt round-robin to the ranks, so every file has one
    writer.  Returns {scene: what ``label_scene`` returned} of this rank."""
    from . import distenv
    from .seflow.ssl_label import CLUSTERINGS
    from .stored import h5_module
    if cluster not in CLUSTERINGS:
        raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
    params = params if params is not None else RaymapParams()
    scenes = sorted(Path(data_dir).glob("*.h5"))
    if not scenes:
        raise FileNotFoundError(f"{data_dir}: no <scene>.h5 files")
    mod = h5_module(f"writing '{key}' into the scene files of {data_dir}")
    done = {}
    with distenv.process_group() as (rank, world):
        def loop():
            for path in scenes[rank::world]:
                s = done[path.stem] = label_scene(path, params, window, key, dynamic_key, overwrite, opener=lambda p: mod.File(p, "a"),
                                                  cluster=cluster, min_cluster_size=min_cluster_size, min_samples=min_samples)
                share = s["dynamic"] / s["points"] if s["points"] else 0.0
                rate = s["sweeps"] / s["seconds"] if s["seconds"] > 0 else float("inf")
                print(f"{path.stem}: {s['sweeps']} sweeps, {s['points']} points, {100.0 * share:.1f} % dynamic, {s['clusters']} clusters "
                      f"-> '{key}', '{dynamic_key}'  ({rate:.1f} sweeps/s)")

        distenv.run_shard(loop, "its scene files")
    return done


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="write <timestamp>/ray_label and <timestamp>/ray_dynamic into the <scene>.h5 files of a directory "
                                             "(free-space ray map, v1; parity with the reference's generator unpinned; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files; 'lidar', 'pose' and 'ground_mask' are read")
    ap.add_argument("--window", type=int, default=5, help=f"neighbour sweeps on each side of a target (0..{MAX_WINDOW})")
    ap.add_argument("--key", default="ray_label", help="dataset name of the int32 cluster labels (seflow.fit --ssl_label <key>)")
    ap.add_argument("--dynamic_key", default="ray_dynamic", help="dataset name of the uint8 per-point flags of rule E")
    ap.add_argument("--overwrite", action="store_true", help="replace existing datasets instead of refusing the scene")
    ap.add_argument("--cluster", default="dbscan", help="the clustering of rule F: 'dbscan' (the default) or 'hdbscan' (HDBSCAN, v1; parity "
                                                        "unpinned); anything else is refused")
    ap.add_argument("--min_cluster_size", type=int, default=None, help="--cluster hdbscan: the smallest cluster (ssl_label.HDB_MIN_CLUSTER)")
    ap.add_argument("--min_samples", type=int, default=None, help="--cluster hdbscan: the core neighbour count, 1..32 (ssl_label.HDB_MIN_SAMPLES)")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.window, a.key, a.dynamic_key, a.overwrite, cluster=a.cluster, min_cluster_size=a.min_cluster_size,
         min_samples=a.min_samples)


if __name__ == "__main__":
    _cli()
