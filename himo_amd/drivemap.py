"""The whole-drive free-space map: ONE voxel map carved from every sweep of a scene, each sweep ray-walked once, that (1) labels
every point ``0 = static / > 0 = dynamic cluster id`` by the space the rest of the drive saw through, written into the scene files so
that ``seflow.fit --ssl_label map_label`` trains on it, and (2) names the voxels that are reliably static: the map of the drive with
the traffic removed, which ``view`` can show.  ``himo_amd.raymap`` ("free-space ray map, v1") builds a fresh map for every target
sweep from at most +-5 neighbours and walks every sweep up to ten times; this stage stands beside it and changes nothing of it.

PARITY UNPINNED.  The reference has no such stage (its label generator is in its absent ``OpenSceneFlow`` submodule).  This stage
follows the build's own written rule, below, and is checked bit for bit against a numpy restatement of it (``tests/drivemap_ref.py``),
never against the reference.  NOTHING HAS BEEN TRIED ON FIELD DATA.

The rule -- "free-space drive map, v1" (normative)
===================================================
Rules A (float32 quantisation to 256 sub-voxel units, unusable at ``|f| >= 2^22``), B (the ray set-up) and C (the integer walk with
64-bit cross-multiplication, ties to the lowest axis, the early stop once a ray has left the grid for good) of "free-space ray map,
v1" hold unchanged: the module docstring of ``himo_amd/raymap.py`` is their text, and ``himo_amd/csrc/drivemap.hip`` (built with
``-ffp-contract=off``) restates their few lines.

Parameters (``DriveMapParams``, mirrored as ``himo_drivemap_params``): grid minimum ``(x0, y0, z0)``, ``voxel`` 0.2 m, ``scale =
(float)(256.0 / voxel)`` computed in double on the host, ``nx, ny, nz``, ``guard`` 2, ``min_votes`` 2, ``min_hits`` 2.  Admitted: finite
floats, voxel > 0, 1 <= nx, ny <= 16384 (the 2^22 sub-voxel limit at 256 per voxel), 1 <= nz <= 256, nx*ny*nz <= 2^29,
0 <= guard <= 8, 1 <= min_votes <= 65535, 1 <= min_hits <= 65535; anything else is refused with a non-zero status and no write.

G'. Frame and extent (``scene_extent``; host, float64).  The map's frame is the frame of the scene's first sweep: ``T_k = inv(pose_0)
    @ pose_k``, rounded to float32 and applied by ``himo_rigid_transform``, as rule G of v1 does.  With ``lo`` / ``hi`` the least /
    greatest translation of the ``T_k`` (float64, before the rounding) per axis, the grid spans ``lo - range .. hi + range`` (``range``
    51.2 m) in x and y and ``lo + z_lo .. hi + z_hi`` (-3 .. 3 m) in z.  With ``v = (double)(float)voxel``: the minimum on an axis is
    ``floor(low / v) * v`` (snapped down to a multiple of the voxel), rounded to float32; the count is ``ceil((high - minimum) / v)``,
    at least 1.  A scene whose grid is not admitted, or whose map (8 bytes per voxel) exceeds ``--max_map_gib`` (4), is refused by
    name before any launch: raise the voxel or split the scene.
B'. Rays of sweep ``s`` (0 <= s <= 65534).  Every return of sweep ``s``, ground returns included, casts a ray from ``origins[src[i]]``
    to the moved point; ``src`` is uint8 [n], ``origins`` float32 [16][3] in the map frame.  A byte of 255 takes no part.  A byte in
    16..254 refuses the whole call on the device, exactly as v1's slot byte does, reported by ``status()``.  ``--origins frame`` (the
    default): every ``src`` is 0 and ``origins[0] = T_s[:3, 3]``.  ``--origins sensors``: ``src[i]`` is the rank of ``lidar_id[i]``
    among the sweep's sorted distinct ids -- the row order of the stored ``SensorsCenter`` (``extract_sca.sensors_center``) -- and
    ``origins[r]`` is ``SensorsCenter[r]`` moved by the float32 ``T_s`` in float64 on the host, rounded to float32.  A sweep without
    ``SensorsCenter``, with more than 16 ids, or with fewer centre rows than ids is refused by name.
D'. Counts per voxel, defined sweep by sweep.  Sweep ``s`` marks a voxel FREE if some ray of ``s`` visits it, in grid, with Chebyshev
    index distance to that ray's end voxel ``> guard``; it marks a voxel HIT if some ray of ``s`` ends in it.  ``hit_n`` is the number
    of sweeps that marked the voxel HIT; ``free_n`` the number that marked it FREE and not HIT -- v1's ``(w & 0xFFFF) & ~(w >> 16)``
    with one slot per sweep and no limit of 16.  The result does not depend on ray order, on how a sweep's rays are split over calls,
    or on carving the same rays of a sweep twice.  PRECONDITION: sweep numbers on one map do not decrease from call to call
    (``DriveMap.carve`` raises ValueError; include/himo_amd.h says so to C callers).  The realisation: one uint64 per voxel,
    ``[nz][ny][nx]``: ``stamp (s + 1) : 16 | 0 : 14 | HIT, FREE : 2 | free_n : 16 | hit_n : 16``, changed by a compare-and-swap on
    the whole word behind a plain load, issued only when the word would change.  A new stamp sets the state and bumps one counter;
    under the same stamp FREE after HIT changes nothing and HIT after FREE gives state HIT, ``free_n - 1``, ``hit_n + 1``: equal
    calls give equal bytes on every run.  The caller clears the map.
E'. Query.  For a point moved into the map frame, with ``fv = free_n`` and ``hv = hit_n`` of its voxel (both 0 for a skipped, an
    unusable or an out-of-grid point): the point is DYNAMIC iff it is not skipped, ``fv >= min_votes`` and ``fv > hv``.  The
    querying sweep's own rays are part of the map, so ``hv >= 1`` for its in-grid points.
F.  Labels are exactly v1's rule F through ``raymap.cluster_labels`` (DBSCAN, or ``--cluster hdbscan``; at least 3 and at least a
    quarter of a cluster DYNAMIC), over the sweep's points in ITS OWN frame; target ground points are passed as skip.
S.  Static map.  A voxel is STATIC iff ``hit_n >= min_hits`` and not (``free_n >= min_votes`` and ``free_n > hit_n``).  ``emit``
    writes one row per STATIC voxel in ascending linear voxel index ``(vz*ny + vy)*nx + vx``: float32 ``[x, y, z, 0]`` with ``x =
    ((float)vx + 0.5f) * voxel + x0``, every operation rounding on its own, beside it ``hits`` and ``free`` as int32.  The order is
    part of the rule (count, scan, write; no atomic ticket).  The call takes a row capacity and returns the count through a device
    word; nothing beyond the capacity is written, and ``DriveMap.emit`` raises with the count it needs.

What is known, from a numpy prototype on the CPU only (the toy drive of ``tests/test_raymap_cpu.py``: 60 sweeps, ego 5 m/s, guard
2, min_votes 2; the share of the box's points flagged DYNAMIC at target sweeps 10 / 30 / 50, whole drive against v1 at window 5):
  1 m/s: 11.0 / 66.4 / 87.8 % against 0.0 / 51.3 / 17.1 %;  2 m/s: 55.0 / 84.0 / 91.1 % against 0.0 / 38.6 / 69.6 %;
  3 m/s: 75.1 / 77.1 / 89.7 % against 0.0 / 9.8 / 42.9 %;  10 m/s (30 sweeps, targets 5 / 15): 90.7 / 87.3 % against 87.2 / 85.5 %.
The wall was 0.0 % everywhere under both rules, and a parked box is 0.0 % under both.
Known limits.  At the LAST sweep of a 30-sweep drive the share of the 10 m/s box drops to 40 %: nothing has seen through those voxels
yet.  On a 30-sweep drive the 2 m/s box at sweep 15 is 0 % under both rules: an object must vacate a voxel for longer than it
occupied it (``fv > hv``).  Per-LiDAR origins: on a three-sensor toy rig (offsets 3.5 m / +-1.2 m / 0.5 m, 20 sweeps) origins at the
sensors rather than at the frame origin changed the box share from 89.5-91.6 % to 92.0-92.1 % and the wall share from 0.03 % to
0.00 %; that is all that is known about them.  The dense grid bounds the drive (16384 voxels per axis, ``--max_map_gib``).

Not part of v1: centroids or colours per voxel; a hashed or tiled map for drives that exceed the dense grid; excluding the querying
sweep's own rays; evidence across scenes; sub-sweep timing of the origin; feeding the map to ``odometry`` or ``accumulate``; a
``--scope drive`` switch inside ``raymap``; an in-feeder ``seflow_ray`` label source.

The program: ``python -m himo_amd.drivemap --data_dir D [--key map_label] [--dynamic_key map_dynamic] [--origins frame|sensors]
[--pose_key pose] [--voxel 0.2] [--guard 2] [--min_votes 2] [--min_hits 2] [--range 51.2] [--z_lo -3] [--z_hi 3] [--max_map_gib 4]
[--cluster dbscan|hdbscan --min_cluster_size M --min_samples K] [--map_out O] [--json PATH] [--overwrite]`` walks the ``<scene>.h5``
files of ``D``.  Per scene it reads ``lidar``, the pose key and ``ground_mask`` (``python -m himo_amd.ground_seg`` writes the masks),
and ``lidar_id`` + ``SensorsCenter`` for ``--origins sensors``; carves every sweep once, in order; queries every sweep and clusters;
and only then opens the file and writes ``<timestamp>/<key>`` (int32, rule F) and ``<timestamp>/<dynamic_key>`` (uint8, rule E').
``--map_out O`` also writes ``O/<scene>.h5`` with one group, the first sweep's timestamp -- ``lidar`` [M, 4] (rule S), ``pose`` = the
first sweep's, ``lidar_dt`` and ``ground_mask`` zeros, ``map_hits`` / ``map_free`` int32 -- and ``O/index_total.pkl``, so that ``python
-m himo_amd.view --data_dir O --res_names raw --color_by label:map_hits`` renders it.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
import time
from pathlib import Path

import numpy as np

ORIGINS = ("frame", "sensors")
MAX_SWEEP = 65534
RANGE, Z_LO, Z_HI, MAX_MAP_GIB = 51.2, -3.0, 3.0, 4.0


class DriveMapParams(ctypes.Structure):
    """mirror of ``himo_drivemap_params`` (include/himo_amd.h); ``scale`` follows from ``voxel``"""
    _fields_ = [("x0", ctypes.c_float), ("y0", ctypes.c_float), ("z0", ctypes.c_float), ("voxel", ctypes.c_float), ("scale", ctypes.c_float),
                ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("guard", ctypes.c_int32), ("min_votes", ctypes.c_int32),
                ("min_hits", ctypes.c_int32)]

    def __init__(self, x0=-51.2, y0=-51.2, z0=-3.0, voxel=0.2, nx=512, ny=512, nz=30, guard=2, min_votes=2, min_hits=2):
        v = float(np.float32(voxel))
        with np.errstate(all="ignore"):
            scale = float(np.float32(np.float64(256.0) / np.float64(v))) if v != 0.0 else float("inf")
        super().__init__(x0, y0, z0, voxel, scale, nx, ny, nz, guard, min_votes, min_hits)

    @property
    def shape(self) -> tuple:
        return int(self.nz), int(self.ny), int(self.nx)

    def admitted(self) -> bool:
        """the host's statement of what ``himo_drivemap_bytes`` admits"""
        if not all(math.isfinite(f) for f in (self.x0, self.y0, self.z0, self.voxel, self.scale)) or not self.voxel > 0:
            return False
        if np.float32(self.scale) != np.float32(np.float64(256.0) / np.float64(np.float32(self.voxel))):
            return False
        if not (1 <= self.nx <= 16384 and 1 <= self.ny <= 16384 and 1 <= self.nz <= 256 and self.nx * self.ny * self.nz <= 1 << 29):
            return False
        return 0 <= self.guard <= 8 and 1 <= self.min_votes <= 65535 and 1 <= self.min_hits <= 65535


_REFUSED = ("drivemap: parameters outside finite floats, voxel > 0, 1 <= nx, ny <= 16384, 1 <= nz <= 256, nx*ny*nz <= 2^29, "
            "0 <= guard <= 8, 1 <= min_votes <= 65535, 1 <= min_hits <= 65535")


def map_bytes(params: DriveMapParams) -> int:
    from . import _lib
    return int(_lib.load().himo_drivemap_bytes(ctypes.addressof(params)))


def _points(pts):
    import torch
    if pts.dim() != 2 or pts.shape[1] not in (3, 4) or pts.dtype != torch.float32 or not pts.is_contiguous():
        raise ValueError(f"points are contiguous float32 rows of 3 or 4 columns, not {tuple(pts.shape)} {pts.dtype}")
    return pts


class DriveMap:
    """A cleared map of ``params`` on ``device`` (``.words``: int64 device tensor [nz, ny, nx], the bits of the uint64 words of rule
    D') and the calls on it.  Everything but ``status`` and ``emit`` is asynchronous on the current stream."""

    def __init__(self, params: DriveMapParams, device=None):
        import torch
        from . import _lib
        if not params.admitted() or map_bytes(params) == 0:
            raise ValueError(_REFUSED)
        self.params = params
        self.device = device if device is not None else _lib.require_gpu()
        self.words = torch.zeros(params.shape, dtype=torch.int64, device=self.device)
        self.sweep = -1
        self._ws = None

    def clear(self):
        self.words.zero_()
        self.sweep = -1
        return self

    def carve(self, pts, src, origins, sweep: int):
        """``himo_drivemap_carve``: the rays ``origins[src[i]] -> pts[i]`` of sweep ``sweep``.  ``pts``: device float32 [n, 3 or 4] in the
        map's frame, ``src``: device uint8 [n] (0..15, 255 = no part), ``origins``: device float32 [16, 3].  Sweep numbers do not
        decrease from call to call (ValueError).  A src byte in 16..254 refuses the whole call ON THE DEVICE: see ``status``."""
        import torch
        from . import _lib
        _points(pts)
        sweep = int(sweep)
        if not 0 <= sweep <= MAX_SWEEP:
            raise ValueError(f"sweep {sweep}: 0..{MAX_SWEEP}")
        if sweep < self.sweep:
            raise ValueError(f"sweep {sweep} after sweep {self.sweep}: sweep numbers on one map do not decrease (rule D')")
        if src.dtype != torch.uint8 or src.shape != (pts.shape[0],) or not src.is_contiguous():
            raise ValueError(f"src is contiguous uint8 [{pts.shape[0]}], not {tuple(src.shape)} {src.dtype}")
        if origins.dtype != torch.float32 or tuple(origins.shape) != (16, 3) or not origins.is_contiguous():
            raise ValueError(f"origins are contiguous float32 [16, 3], not {tuple(origins.shape)} {origins.dtype}")
        st = _lib.load().himo_drivemap_carve(int(pts.shape[0]), _lib.ptr(pts), int(pts.shape[1]), _lib.ptr(src), _lib.ptr(origins), sweep,
                                             ctypes.addressof(self.params), _lib.ptr(self.words), _lib.stream_handle())
        _lib.check(st, "himo_drivemap_carve")
        self.sweep = sweep
        return self

    def status(self) -> None:
        """Wait for the current stream and raise ValueError if a ``carve`` call on this device was refused for a src byte in 16..254
        since the last ``status()`` (such a call marked nothing)."""
        from . import _lib
        _lib.check(_lib.load().himo_drivemap_status(_lib.stream_handle()), "himo_drivemap_carve: a src byte in 16..254")

    def query(self, pts, skip=None):
        """``himo_drivemap_query``: (dynamic uint8, fv uint16, hv uint16), device tensors [n], for ``pts`` (device float32 [n, 3 or 4] in
        the map's frame).  ``skip``: device uint8 / bool [n], non-zero = never DYNAMIC."""
        import torch
        from . import _lib
        _points(pts)
        n = int(pts.shape[0])
        if skip is not None:
            skip = skip.to(torch.uint8).contiguous()
            if skip.shape != (n,):
                raise ValueError(f"skip is [{n}], not {tuple(skip.shape)}")
        dyn = torch.empty(n, dtype=torch.uint8, device=pts.device)
        fv, hv = (torch.empty(n, dtype=torch.uint16, device=pts.device) for _ in range(2))
        st = _lib.load().himo_drivemap_query(n, _lib.ptr(pts), int(pts.shape[1]), _lib.ptr(skip), ctypes.addressof(self.params),
                                             _lib.ptr(self.words), _lib.ptr(fv), _lib.ptr(hv), _lib.ptr(dyn), _lib.stream_handle())
        _lib.check(st, "himo_drivemap_query")
        return dyn, fv, hv

    def emit(self, capacity: int | None = None):
        """``himo_drivemap_emit`` (rule S): (rows float32 [M, 4], hits int32 [M], free int32 [M]) device tensors, in ascending voxel
        index.  ``capacity`` None: a first call counts, a second writes exactly M rows; a number: ValueError, naming M, if M exceeds it.
        Waits for the count."""
        import torch
        from . import _lib
        lib = _lib.load()
        if self._ws is None:
            need = int(lib.himo_drivemap_emit_workspace_bytes(ctypes.addressof(self.params)))
            self._ws = torch.empty(max(need, 4) // 4 + 1, dtype=torch.int32, device=self.device)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)

        def call(cap, rows, hits, free):
            st = lib.himo_drivemap_emit(ctypes.addressof(self.params), _lib.ptr(self.words), int(cap), _lib.ptr(rows), _lib.ptr(hits),
                                        _lib.ptr(free), _lib.ptr(count), _lib.ptr(self._ws), self._ws.numel() * 4, _lib.stream_handle())
            _lib.check(st, "himo_drivemap_emit")
            return int(count.item())

        if capacity is None:
            capacity = call(0, None, None, None)
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError(f"capacity={capacity}: at least 0")
        rows = torch.empty((capacity, 4), dtype=torch.float32, device=self.device)
        hits, free = (torch.empty(capacity, dtype=torch.int32, device=self.device) for _ in range(2))
        m = call(capacity, rows if capacity else None, hits if capacity else None, free if capacity else None)
        if m > capacity:
            raise ValueError(f"himo_drivemap_emit: the map holds {m} STATIC voxels, the capacity is {capacity} rows")
        return rows[:m], hits[:m], free[:m]

    def counts(self):
        """(free_n, hit_n) of every voxel: int32 device tensors [nz, ny, nx] (torch arithmetic on the words; for inspection)"""
        import torch
        return ((self.words >> 16) & 0xFFFF).to(torch.int32), (self.words & 0xFFFF).to(torch.int32)


# --------------------------------------------------------------------------------------------------------------------------
# the host side of the rule
# --------------------------------------------------------------------------------------------------------------------------
def relative_poses(poses) -> list:
    """rule G': ``T_k = inv(pose_0) @ pose_k`` in float64 (the list returned), to be rounded to float32 where they are applied"""
    inv0 = np.linalg.inv(np.asarray(poses[0], dtype=np.float64))
    return [inv0 @ np.asarray(p, dtype=np.float64) for p in poses]


def scene_extent(poses, voxel: float = 0.2, guard: int = 2, min_votes: int = 2, min_hits: int = 2, range_m: float = RANGE,
                 z_lo: float = Z_LO, z_hi: float = Z_HI, max_map_gib: float = MAX_MAP_GIB, where: str = "the scene") -> DriveMapParams:
    """Rule G': the parameters of the map of a scene with these 4x4 world poses, or the refusal (ValueError) that names ``where``."""
    if len(poses) < 1:
        raise ValueError(f"{where}: no sweeps")
    if len(poses) > MAX_SWEEP + 1:
        raise ValueError(f"{where}: {len(poses)} sweeps; a map counts at most {MAX_SWEEP + 1} (split the scene)")
    if not (math.isfinite(voxel) and float(np.float32(voxel)) > 0.0):
        raise ValueError(f"voxel={voxel}: finite and > 0")
    if not (math.isfinite(range_m) and range_m >= 0 and math.isfinite(z_lo) and math.isfinite(z_hi) and z_lo <= z_hi):
        raise ValueError(f"range={range_m}, z_lo={z_lo}, z_hi={z_hi}: finite, range >= 0, z_lo <= z_hi")
    t = np.stack([T[:3, 3] for T in relative_poses(poses)])
    if not np.isfinite(t).all():
        raise ValueError(f"{where}: a pose is not finite")
    v = float(np.float32(voxel))
    low = t.min(axis=0) + np.array([-range_m, -range_m, z_lo])
    high = t.max(axis=0) + np.array([range_m, range_m, z_hi])
    minimum = np.floor(low / v) * v
    n = np.maximum(np.ceil((high - minimum) / v), 1.0)
    nx, ny, nz = (int(min(c, 2 ** 31 - 1)) for c in n)
    p = DriveMapParams(float(minimum[0]), float(minimum[1]), float(minimum[2]), voxel, nx, ny, nz, guard, min_votes, min_hits)
    advice = "raise --voxel or split the scene"
    if not p.admitted():
        raise ValueError(f"{where}: a grid of {nx} x {ny} x {nz} voxels of {voxel:g} m (guard {guard}, min_votes {min_votes}, min_hits {min_hits}) "
                         f"is not admitted ({_REFUSED[10:]}): {advice}")
    gib = 8.0 * nx * ny * nz / 2 ** 30
    if gib > max_map_gib:
        raise ValueError(f"{where}: the map of {nx} x {ny} x {nz} voxels takes {gib:.2f} GiB, more than --max_map_gib {max_map_gib:g}: {advice}")
    return p


def sweep_sources(T32, n: int, origins: str = "frame", lidar_id=None, centers=None, where: str = "the sweep") -> tuple:
    """Rule B': (src uint8 [n], origins float32 [16, 3]) of a sweep of ``n`` returns whose float32 transform into the map frame is
    ``T32``.  ``sensors``: ``lidar_id`` [n] and ``centers`` = the stored ``SensorsCenter`` [ids, 3] of the sweep."""
    if origins not in ORIGINS:
        raise ValueError(f"--origins {origins!r}: one of {', '.join(ORIGINS)}")
    T32 = np.asarray(T32, dtype=np.float32)
    table = np.zeros((16, 3), dtype=np.float32)
    if origins == "frame":
        table[0] = T32[:3, 3]
        return np.zeros(int(n), dtype=np.uint8), table
    if centers is None:
        raise KeyError(f"SensorsCenter: {where} holds no sensor centres (--origins sensors needs them; --origins frame does not)")
    if lidar_id is None:
        raise KeyError(f"lidar_id: {where} holds no sensor ids (--origins sensors needs them; --origins frame does not)")
    lidar_id = np.asarray(lidar_id).reshape(-1)
    if len(lidar_id) != int(n):
        raise ValueError(f"lidar_id: {where} holds {len(lidar_id)} ids for {n} returns")
    ids = np.unique(lidar_id)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    if len(ids) > 16:
        raise ValueError(f"lidar_id: {where} holds {len(ids)} distinct sensor ids; the origin table has 16 rows")
    if len(centers) < len(ids):
        raise ValueError(f"SensorsCenter: {where} holds {len(centers)} centre rows for {len(ids)} distinct sensor ids")
    T64 = T32.astype(np.float64)
    table[:len(ids)] = (centers[:len(ids)] @ T64[:3, :3].T + T64[:3, 3]).astype(np.float32)
    return np.searchsorted(ids, lidar_id).astype(np.uint8), table


def carve_drive(dm: DriveMap, sweeps, T, origins: str = "frame", lidar_ids=None, centers=None, where: str = "scene") -> tuple:
    """Rules G' and B' for one scene: move every sweep (device float32 [n_k, 3] in its own frame) by ``(float)T[k]`` and carve it into
    ``dm`` as sweep ``k``, in order.  Returns (the moved sweeps, [(src, origins16) host arrays per sweep]).  Asynchronous."""
    import torch
    from .seflow.ssl_label import _moved
    sources = [sweep_sources(np.asarray(T[k], np.float32), len(sweeps[k]), origins, None if lidar_ids is None else lidar_ids[k],
                             None if centers is None else centers[k], f"{where} sweep {k}") for k in range(len(sweeps))]
    moved = []
    for k, (pc, (src, table)) in enumerate(zip(sweeps, sources)):
        m = _moved(pc, np.asarray(T[k], np.float32))
        dm.carve(m, torch.from_numpy(src).to(dm.device), torch.from_numpy(table).to(dm.device), k)
        moved.append(m)
    return moved, sources


# --------------------------------------------------------------------------------------------------------------------------
# the program
# --------------------------------------------------------------------------------------------------------------------------
def label_scene(path, key: str = "map_label", dynamic_key: str = "map_dynamic", origins: str = "frame", pose_key: str = "pose",
                voxel: float = 0.2, guard: int = 2, min_votes: int = 2, min_hits: int = 2, range_m: float = RANGE, z_lo: float = Z_LO,
                z_hi: float = Z_HI, max_map_gib: float = MAX_MAP_GIB, overwrite: bool = False, opener=None, cluster: str = "dbscan",
                min_cluster_size: int | None = None, min_samples: int | None = None, map_out=None) -> dict:
    """One scene file: read every sweep, carve every sweep once, query and cluster every sweep, and only once the reads are done open
    the file for modification and write ``<timestamp>/<key>`` (int32) and ``<timestamp>/<dynamic_key>`` (uint8).  ``map_out``: a
    directory that receives ``<scene>.h5`` with the static map (the caller writes its index).  Returns {"sweeps", "points", "dynamic",
    "clusters", "static_voxels", "map_mib", "seconds", "first"} (seconds: upload, carving, queries, clustering, emit and the copies
    back; no file time)."""
    import torch
    from . import _lib, h5lite
    from .dataset import h5_reader
    from .raymap import _device_points, cluster_labels
    from .stored import h5_module, put_keys
    path = Path(path)
    if origins not in ORIGINS:
        raise ValueError(f"--origins {origins!r}: one of {', '.join(ORIGINS)}")
    clouds, poses, grounds, ids, centres = [], [], [], [], []
    with h5_reader().File(path, "r") as f:
        stamps = sorted(f.keys())
        have = [ts for ts in stamps if key in f[ts] or dynamic_key in f[ts]]
        if have and not overwrite:
            raise FileExistsError(f"{path}: {len(have)} of {len(stamps)} sweeps already hold '{key}' or '{dynamic_key}' (--overwrite replaces them)")
        for ts in stamps:
            g = f[ts]
            if "ground_mask" not in g:
                raise KeyError(f"ground_mask: {path} sweep {ts} has no ground mask (`python -m himo_amd.ground_seg` writes them)")
            if pose_key not in g:
                raise KeyError(f"{pose_key}: {path} sweep {ts} holds no such pose (--pose_key; pose_odom: python -m himo_amd.odometry)")
            if origins == "sensors":
                for name in ("SensorsCenter", "lidar_id"):
                    if name not in g:
                        raise KeyError(f"{name}: {path} sweep {ts} holds no such key (--origins sensors needs it; --origins frame does not)")
                ids.append(np.asarray(g["lidar_id"][:]))
                centres.append(np.asarray(g["SensorsCenter"][:], dtype=np.float64))
            clouds.append(np.asarray(g["lidar"][:], dtype=np.float32))
            poses.append(np.asarray(g[pose_key][:], dtype=np.float64))
            grounds.append(np.asarray(g["ground_mask"][:]).astype(np.uint8))
    params = scene_extent(poses, voxel, guard, min_votes, min_hits, range_m, z_lo, z_hi, max_map_gib, where=str(path))
    T = relative_poses(poses)
    if origins == "sensors":                                              # the refusals of rule B', before any launch
        for k in range(len(stamps)):
            sweep_sources(np.asarray(T[k], np.float32), len(clouds[k]), origins, ids[k], centres[k], f"{path} sweep {stamps[k]}")
    dev = _lib.require_gpu()
    t0 = time.perf_counter()
    labels, flags = [], []
    with torch.cuda.device(dev):
        on_dev = [_device_points(c, dev) for c in clouds]
        masks = [torch.from_numpy(g).to(dev) for g in grounds]
        dm = DriveMap(params, dev)
        moved, _ = carve_drive(dm, on_dev, T, origins, ids or None, centres or None, str(path))
        dm.status()
        for k in range(len(stamps)):
            dyn, _, _ = dm.query(moved[k], masks[k])
            lab = cluster_labels(on_dev[k], masks[k], dyn, cluster=cluster, min_cluster_size=min_cluster_size, min_samples=min_samples)
            labels.append(lab.cpu().numpy().astype(np.int32))
            flags.append(dyn.cpu().numpy().astype(np.uint8))
        rows, hits, free = (a.cpu().numpy() for a in dm.emit())
    seconds = time.perf_counter() - t0
    if opener is None:
        mod = h5_module(f"{path}: writing '{key}' into a scene file")
        opener = lambda p: mod.File(p, "a")                               # noqa: E731
    with opener(path) as f:
        for ts, lab, dyn in zip(stamps, labels, flags):
            put_keys(f, ts, {key: lab, dynamic_key: dyn})
    if map_out is not None and stamps:
        tree = {stamps[0]: {"lidar": rows.astype(np.float32), "pose": poses[0], "lidar_dt": np.zeros(len(rows), np.float32),
                            "ground_mask": np.zeros(len(rows), np.uint8), "map_hits": hits.astype(np.int32), "map_free": free.astype(np.int32)}}
        h5lite.write_file(Path(map_out) / f"{path.stem}.h5", tree)
    return {"sweeps": len(stamps), "points": int(sum(len(x) for x in labels)), "dynamic": int(sum(int(x.sum()) for x in flags)),
            "clusters": int(sum(int(x.max(initial=0)) for x in labels)), "static_voxels": int(len(rows)),
            "map_mib": 8.0 * params.nx * params.ny * params.nz / 2 ** 20, "seconds": seconds, "first": stamps[0] if stamps else None}


def _line(scene: str, s: dict, key: str, dynamic_key: str) -> str:
    share = s["dynamic"] / s["points"] if s["points"] else 0.0
    rate = s["sweeps"] / s["seconds"] if s["seconds"] > 0 else float("inf")
    return (f"{scene}: {s['sweeps']} sweeps, {s['points']} points, {100.0 * share:.1f} % dynamic, {s['clusters']} clusters, "
            f"{s['static_voxels']} static voxels, map {s['map_mib']:.1f} MiB -> '{key}', '{dynamic_key}'  ({rate:.1f} sweeps/s)")


def main(data_dir: str, key: str = "map_label", dynamic_key: str = "map_dynamic", origins: str = "frame", pose_key: str = "pose",
         voxel: float = 0.2, guard: int = 2, min_votes: int = 2, min_hits: int = 2, range_m: float = RANGE, z_lo: float = Z_LO,
         z_hi: float = Z_HI, max_map_gib: float = MAX_MAP_GIB, cluster: str = "dbscan", min_cluster_size: int | None = None,
         min_samples: int | None = None, map_out: str | None = None, json_path: str | None = None, overwrite: bool = False) -> dict:
    """The program.  Under ``torchrun`` (one rank per GPU) the scenes are dealt round-robin to the ranks, so every file has one
    writer.  Returns {scene: what ``label_scene`` returned} of every rank (what ``--json`` writes)."""
    from . import distenv
    from .accumulate import _write_index
    from .seflow.ssl_label import CLUSTERINGS
    from .stored import h5_module
    if cluster not in CLUSTERINGS:
        raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
    if origins not in ORIGINS:
        raise ValueError(f"--origins {origins!r}: one of {', '.join(ORIGINS)}")
    root = Path(data_dir)
    out_root = None if map_out is None else Path(map_out)
    if out_root is not None and out_root.resolve() == root.resolve():
        raise ValueError(f"--map_out {map_out}: the static maps are written beside the input, never into it (--map_out equals --data_dir)")
    scenes = sorted(root.glob("*.h5"))
    if not scenes:
        raise FileNotFoundError(f"{data_dir}: no <scene>.h5 files")
    mod = h5_module(f"writing '{key}' into the scene files of {data_dir}")
    done = {}
    with distenv.process_group() as (rank, world):
        def loop():
            if out_root is not None:
                out_root.mkdir(parents=True, exist_ok=True)
            for path in scenes[rank::world]:
                s = done[path.stem] = label_scene(path, key, dynamic_key, origins, pose_key, voxel, guard, min_votes, min_hits, range_m, z_lo,
                                                  z_hi, max_map_gib, overwrite, opener=lambda p: mod.File(p, "a"), cluster=cluster,
                                                  min_cluster_size=min_cluster_size, min_samples=min_samples, map_out=out_root)
                print(_line(path.stem, s, key, dynamic_key))

        distenv.run_shard(loop, "its scene files")
        every = distenv.gathered(done, lambda a, b: {**a, **b})
        if rank == 0:
            if out_root is not None and every:
                _write_index(out_root, [[sc, every[sc]["first"]] for sc in sorted(every) if every[sc]["first"] is not None])
            if json_path:
                import json
                Path(json_path).write_text(json.dumps({"scenes": every}, indent=1) + "\n")
    return every


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="write <timestamp>/map_label and <timestamp>/map_dynamic into the <scene>.h5 files of a directory from "
                                             "ONE free-space map per scene, and optionally the scene's static map (free-space drive map, v1; "
                                             "parity unpinned: the reference has no such stage; nothing has been tried on field data; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files; 'lidar', the pose key and 'ground_mask' are read")
    ap.add_argument("--key", default="map_label", help="dataset name of the int32 cluster labels (seflow.fit --ssl_label <key>)")
    ap.add_argument("--dynamic_key", default="map_dynamic", help="dataset name of the uint8 per-point flags of rule E'")
    ap.add_argument("--origins", default="frame", choices=ORIGINS, help="ray origins: the sweep's frame origin, or the stored SensorsCenter row "
                                                                        "of each return's lidar_id")
    ap.add_argument("--pose_key", default="pose", help="the stored pose the map frame is taken from (pose_odom: python -m himo_amd.odometry)")
    ap.add_argument("--voxel", type=float, default=0.2, help="voxel edge, m")
    ap.add_argument("--guard", type=int, default=2, help="voxels in front of a return (Chebyshev) that its ray does not carve (0..8)")
    ap.add_argument("--min_votes", type=int, default=2, help="sweeps that must have seen through a voxel and not returned from it")
    ap.add_argument("--min_hits", type=int, default=2, help="sweeps that must have returned from a voxel of the static map")
    ap.add_argument("--range", type=float, default=RANGE, dest="range_m", help="metres of map round the drive's path in x and y")
    ap.add_argument("--z_lo", type=float, default=Z_LO, help="metres of map below the lowest sweep origin")
    ap.add_argument("--z_hi", type=float, default=Z_HI, help="metres of map above the highest sweep origin")
    ap.add_argument("--max_map_gib", type=float, default=MAX_MAP_GIB, help="refuse a scene whose map (8 bytes per voxel) is larger")
    ap.add_argument("--cluster", default="dbscan", help="the clustering of rule F: 'dbscan' (the default) or 'hdbscan' (HDBSCAN, v1; parity "
                                                        "unpinned); anything else is refused")
    ap.add_argument("--min_cluster_size", type=int, default=None, help="--cluster hdbscan: the smallest cluster (ssl_label.HDB_MIN_CLUSTER)")
    ap.add_argument("--min_samples", type=int, default=None, help="--cluster hdbscan: the core neighbour count, 1..32 (ssl_label.HDB_MIN_SAMPLES)")
    ap.add_argument("--map_out", default=None, metavar="O", help="also write O/<scene>.h5 (the STATIC voxels as one sweep, with map_hits / map_free) "
                                                                 "and O/index_total.pkl")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the per-scene numbers to PATH")
    ap.add_argument("--overwrite", action="store_true", help="replace existing datasets instead of refusing the scene")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    return main(a.data_dir, a.key, a.dynamic_key, a.origins, a.pose_key, a.voxel, a.guard, a.min_votes, a.min_hits, a.range_m, a.z_lo, a.z_hi,
                a.max_map_gib, a.cluster, a.min_cluster_size, a.min_samples, a.map_out, a.json, a.overwrite)


if __name__ == "__main__":
    _cli()
