"""Multi-sweep accumulation: the compensated sweeps ``t - window .. t`` of a scene moved into the frame of sweep ``t`` and reduced to
one centroid per occupied voxel, each carrying the least time lag of its rows -- the input TransFusion-L (nuScenes style) and the
WaffleIron runs of the reference's ``downstream/README.md`` consume, and, with ground and dynamic rows skipped, a static cloud for
mapping.  ``comp_dis`` matters most here: an uncompensated vehicle is laid over itself once per sweep.

PARITY UNPINNED.  The reference has no such program in its tree (``h5sf.py`` and ``eval_h5.py`` live in absent forks).  This stage
follows the build's own written rule, below, and is checked bit for bit against a numpy restatement of it
(``tests/accumulate_ref.py``), never against the reference.

The rule -- "sweep accumulation, v1" (normative)
================================================
All float arithmetic rounds after every operation (``himo_amd/csrc/accumulate.hip`` is built with ``-ffp-contract=off``; the two
fused multiply-adds of rule B are written as such); everything after rule C is integer, so the result does not depend on the order
in which rows arrive.

Parameters (``AccumParams``, mirrored as ``himo_accum_params``): grid minimum ``(x0, y0, z0)`` (-51.2, -51.2, -3.0), ``voxel`` 0.1 m,
``nx, ny, nz`` 1024, 1024, 80, the ego box ``ego_min``, ``ego_max`` (``compdis.EGO_BOX`` of the data set).  The struct carries
``scale = (float)(256.0 / voxel)``, computed in double on the host, as ``RaymapParams`` does.  Admitted: every float finite,
voxel > 0, scale equal to that expression and finite, 1 <= nx, ny <= 4096, 1 <= nz <= 256; anything else is refused with a non-zero
status and no launch.  A voxel key is ``(iz << 24) | (iy << 12) | ix``, 32 bits.

A. Input rows.  A source sweep is ``float[n][pitch]``, pitch 3 or 4 (x, y, z first), with an optional skip byte per row, a row-major
   4x4 float32 transform ``T`` from the source's frame to the target's and an integer ``lag`` in 0..255.  A row takes part iff its skip
   byte is 0, its three coordinates are finite, and it is not strictly inside the ego box: the six strict inequalities of
   ``utils.ego_pts_mask``, tested on the row as given (in the SOURCE's frame: the vehicle's own returns, wherever it was).
B. Move.  ``q = R p + t`` with the arithmetic of ``himo_rigid_transform`` -- one device function for both (``csrc/rigid_math.h``):
   ``q0 = fma(z, T02, fma(y, T01, x * T00)) + T03``, ``q1 = fma(z, T12, fma(x, T10, y * T11)) + T13``,
   ``q2 = fma(z, T22, fma(x, T20, y * T21)) + T23``; a product, two fused multiply-adds and a sum, each rounding once.
C. Quantise: raymap rule A on this grid.  ``f = (c - m) * scale``; the row is unusable if any ``f`` is non-finite or
   ``|f| >= 4194304.0f``; ``u = (int)floorf(f)``, the voxel index is ``u >> 8`` and the sub-voxel offset ``u & 255``.  A row whose voxel
   is outside ``[0, n)`` on any axis is dropped.
D. Reduce.  Every occupied voxel carries ``count`` (its rows), ``Sx, Sy, Sz`` (the integer sums of their sub-voxel offsets) and
   ``lag`` (the least lag of its rows).  Successive insert calls accumulate until the table is cleared.  At most 2^24 rows may be
   inserted between two clears, so that the 32-bit sums cannot overflow (255 * 2^24 < 2^32); ``Accumulator`` counts them and refuses
   more.
E. Emit.  One output row per occupied voxel, in ascending key order.  The centroid per axis in float64, every operation rounding on
   its own, then one rounding to float32:
   ``x = (float)((double)x0 + (((double)(256 * ix) + 0.5) + (double)Sx / (double)count) * ((double)voxel / 256.0))`` with ``x0`` and
   ``voxel`` the float32 values of the struct; beside it ``lag`` (uint8), ``count`` (int32) and the key.  (``voxel`` 1, minimum 0, one
   point at 0.5: ``u = 128``, ``x = 0.501953125``.)
G. The cloud of a target sweep ``t`` of a scene (``accumulate_target``).  The sources are the sweeps ``k = max(0, t - window) .. t``
   of the same scene, ``0 <= window <= 31``.  Source ``k`` is moved with ``T = inv(pose_t) @ pose_k``, computed in float64 on the host
   and rounded to float32 (as raymap rule G), and inserted with ``lag = t - k``.  The table's capacity is the next power of two at or
   above twice the window's row count (16 at least).

The container is an open-addressing hash table in device memory (``himo_accum_*`` in include/himo_amd.h; the layout and the hash are
in the header of the ``.hip`` file).  Its probe loop is bounded: a table too small for the voxels offered is a refusal reported by
``himo_accum_status`` -- ``Accumulator.result`` raises ``ValueError`` -- never a hang.  The ascending-key order is a ``torch.sort`` of
the emitted key column and gathers by its permutation: rows are moved, no arithmetic is done on point data in Python.

The program: ``python -m himo_amd.accumulate --data_dir D --out_dir O [--res_name seflowpp_best | raw] [--window 10] [--voxel 0.1]
[--drop_ground] [--drop_label KEY] [--data_name av2|scania] [--overwrite]``.  For every scene file of ``D`` the targets are the sweeps
that have a successor (their flow is defined).  Source ``k`` is compensated by the pinned path, ``CompDisEngine.run_frame(...,
refined=True)`` with the stored ``<res_name>`` (``raw``: the points as recorded; a missing key is the ``KeyError`` the other programs
raise), then rule G.  ``--drop_ground`` skips rows whose ``ground_mask`` is set, ``--drop_label KEY`` rows whose stored integer label
``KEY`` (``ray_label``, say) is non-zero: together a static, ground-free cloud; a missing mask or label is a ``KeyError`` naming the
program that writes it.  Output: ``O/<scene>.h5`` (refused if it exists, without ``--overwrite``) and ``O/index_total.pkl``, ordinary
scene files the package's loader reads; per target ``<timestamp>/lidar`` float32 [M, 4] (x, y, z, ``lag * 0.1`` s),
``<timestamp>/pose`` (the target's, bytes unchanged), ``<timestamp>/lidar_dt`` (zeros [M]: an accumulated cloud is already
compensated) and ``<timestamp>/acc_count`` int32 [M]; beside them ``<timestamp>/ground_mask``, all False (v1 marks no centroid as
ground; the viewer and the evaluators ask every sweep for a mask).  ``python -m himo_amd.view --data_dir O --res_names raw --color_by
label:acc_count`` shows such a cloud coloured by rows per voxel (the default ``--color_by lidar`` wants a ``lidar_id`` per point, which
a centroid has not).
Under ``torchrun`` the scenes are dealt round-robin to the ranks.  There is no CPU path.

Not part of v1: moving dynamic points along their flow to the target's time; intensity or any other per-point attribute in the
output (v2, below, adds both, and a label, when asked); future sweeps as sources; a map that persists along a drive;
a world-frame output; an in-line switch of ``save``.

The additions -- "sweep accumulation, v2" (normative; opt-in; v1 bit for bit when nothing is asked)
====================================================================================================
PARITY UNPINNED, as v1 is: the reference has no such program, and v2 is checked bit for bit against a numpy restatement of the text
below (``tests/accumulate2_ref.py``), never against the reference.  The table keeps its size and its hash: words 6 and 7 of every
32-byte slot, unused and cleared to 0 in v1, hold ``Sa`` and ``tag``.  An insert that carries none of ``motion``, ``attr`` and
``label`` is v1's insert, and ``himo_accum_insert`` / ``himo_accum_emit`` launch the same kernels with every v2 statement compiled
out.  All float32 steps round after every operation; the fused multiply-adds are written as ``fmaf``.

A2. Advect (after rule A, before rule B; optional per insert call).  A call may carry ``motion``, float32 ``[n][3]``: the row's own
   displacement per sweep period, free of ego motion, in the source frame's axes -- added to the row as ``refine_pts`` adds
   ``comp_dis`` -- and ``motion_min2``, a float32.  A row with a non-finite motion component takes no part.  Otherwise
   ``s = (mx*mx + my*my) + mz*mz``, each operation rounded, and the row is moved iff ``s >= motion_min2``:
   ``x' = fmaf((float)lag, mx, x)``, likewise ``y`` and ``z`` (so ``lag = 0`` leaves the target's own rows untouched exactly).  Rule A's
   ego-box test stays on the row AS GIVEN.  ``motion_min2 = (float)((double)motion_min * (double)motion_min)`` is computed on the
   host; ``motion_min`` is finite and ``>= 0``.
I. The motion of a stored flow (``flow_motion``, ``himo_accum_motion``).  From the raw ``pc0`` rows (pitch 3 or 4), a stored flow
   ``[n][3]`` that INCLUDES ego motion and ``E = inv(pose1) @ pose0``, computed in float64 on the host and rounded to float32 as in
   rule G: ``q = rigid_apply(E, p)`` (rule B's arithmetic), ``d = q - p``, ``m = flow - d``: three rounded subtractions a row after
   the shared move.  This is ``est_flow`` of the reference's ``save_zip.py:115-117`` on this build's written arithmetic.
H. Attributes.  A call may carry ``attr``, float32 with a stride in floats (column 3 of raw ``[n][4]`` ``lidar`` rows is read in
   place, stride 4), with ``attr_scale``, finite and ``> 0``; and ``label``, int32 ``[n]``.
   ``g = v * attr_scale``; ``q = 0`` if ``!(g > 0)`` (NaN, negatives and zero), ``q = 255`` if ``g >= 255``, else
   ``q = (uint)floorf(g + 0.5f)``; slot word 6 accumulates ``Sa += q`` (255 * 2^24 fits in 32 bits under rule D's row cap).
   ``lab = label`` if ``0 < label < 2^24``, else 0; ``tag = ((255 - lag) << 24) | lab``; slot word 7 takes ``max(tag)``: the label of
   the freshest row, the largest label among ties -- integer, and independent of the order of arrival.  The merge of runs of
   neighbouring lanes carries both: it sums ``Sa`` and takes the greatest ``tag``.
   Rows inserted without an attribute, by v1's entry point or by v2 with a null pointer, count as intensity 0: they add to ``count``
   and nothing to ``Sa``.  Rows inserted without a label, likewise, count as label 0 and leave word 7 alone: a voxel that only such
   rows reached has label 0, and they do not displace the label of a labelled row, however fresh they are.  (A row whose label is
   GIVEN as 0, or outside ``0 < label < 2^24``, does take part with ``lab = 0``: fresher than a labelled row, it makes the voxel's
   label 0.)
E2. Emit.  Beside v1's columns, optionally ``intensity = (float)(((double)Sa / (double)count) / (double)attr_scale)`` and
   ``label = tag & 0xFFFFFF`` (int32).  (``voxel`` 1, scale 1: rows of intensity 100.4 and 201.0 in one voxel quantise to 100 and
   201, the emitted value is 150.5.  Scale 255: one row of 0.5 gives ``g = 127.5``, ``q = 128``, emitted ``(float)(128.0 / 255.0)``.)

``Accumulator.add(..., motion=, motion_min=, intensity=, intensity_scale=, label=)`` and ``result_ex()`` (``result()`` and the
intensity and label columns), ``accumulate_target(..., motions=, intensities=, labels=, motion_min=, intensity_scale=)`` and
``flow_motion(pc0, flow, pose0, pose1)`` are the Python side.  One ``intensity_scale`` holds from a ``clear()`` to the next.

The program's v2 flags, all off by default -- with none given the files are byte-identical to v1's: ``[--advect] [--motion_key KEY]
[--motion_min 0.05] [--intensity] [--intensity_scale 1.0] [--carry_label KEY] [--bin_dir B]``.  ``--advect`` moves the rows of source
``k`` by rule A2 with the motion (rule I) of the stored flow ``--motion_key`` (default: ``--res_name``; ``--advect`` with ``--res_name
raw`` and no ``--motion_key`` is a ``ValueError`` before any GPU work, a missing key the ``KeyError`` of a missing ``res_name``;
``<res>_rigid`` from ``himo_amd.rigid_refine`` is the coherent choice: one motion per cluster) where it is at least ``--motion_min``
metres a sweep (0.05, the project's static threshold, ``RigidParams.static_disp``).  ``--intensity`` reads column 3 of the ``lidar``
rows and writes ``<timestamp>/acc_intensity`` float32 [M]; ``--carry_label KEY`` a stored integer label (``ray_label``,
``flow_instance_id``; a missing key names the program that writes it) and writes ``<timestamp>/acc_label`` int32 [M], which
``python -m himo_amd.view --color_by label:acc_label`` shows as it stands.  ``--bin_dir B`` additionally writes
``B/<scene>/<timestamp>.bin``, little-endian float32 [M][5] = x, y, z, intensity, ``lag * 0.1``: the nuScenes sweep row that OpenPCDet
reads (the intensity column is zeros without ``--intensity``); a host-only write.  ``lidar``, ``pose``, ``lidar_dt``, ``acc_count``
and ``ground_mask`` stay exactly as v1 writes them.

Nothing of v2 has been tried on field data.  Constant-velocity extrapolation over 10 sweeps multiplies the per-sweep error of the
flow by up to 10: a 5 cm error a sweep lays the oldest copy of a vehicle 0.5 m off.

Not part of v2: chaining flows sweep to sweep, with a neighbour lookup at each step, instead of one constant-velocity step; rotating
a cluster about its centre; future sweeps as sources; more than one attribute or label; a count of moved rows per voxel (word 7 is
taken); a persistent map; a world-frame output; an in-line switch of ``save``.
"""
from __future__ import annotations

import ctypes
import time
from pathlib import Path

import numpy as np

MAX_WINDOW = 31
MAX_ROWS = 1 << 24                  # rule D: rows between two clears
MIN_CAPACITY, MAX_CAPACITY = 1 << 4, 1 << 26
LAG_SECONDS = 0.1                   # the sweep period the lag column is written in


class AccumParams(ctypes.Structure):
    """mirror of ``himo_accum_params`` (include/himo_amd.h); ``scale`` follows from ``voxel``.  ``check()`` raises for what the library
    refuses."""
    _fields_ = [("x0", ctypes.c_float), ("y0", ctypes.c_float), ("z0", ctypes.c_float), ("voxel", ctypes.c_float), ("scale", ctypes.c_float),
                ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("ego_min", ctypes.c_float * 3),
                ("ego_max", ctypes.c_float * 3)]

    def __init__(self, x0=-51.2, y0=-51.2, z0=-3.0, voxel=0.1, nx=1024, ny=1024, nz=80, ego_min=None, ego_max=None, data_name="av2"):
        from .compdis import EGO_BOX
        lo, hi = EGO_BOX["scania" if data_name == "scania" else "av2"]
        v = float(np.float32(voxel))
        with np.errstate(all="ignore"):
            scale = float(np.float32(np.float64(256.0) / np.float64(v))) if v != 0.0 else float("inf")
        three = lambda a: (ctypes.c_float * 3)(*[float(x) for x in a])        # noqa: E731
        super().__init__(x0, y0, z0, voxel, scale, nx, ny, nz, three(lo if ego_min is None else ego_min), three(hi if ego_max is None else ego_max))

    def check(self) -> "AccumParams":
        floats = [self.x0, self.y0, self.z0, self.voxel, self.scale, *self.ego_min, *self.ego_max]
        ok = all(np.isfinite(f) for f in floats) and self.voxel > 0
        if ok:
            with np.errstate(all="ignore"):
                ok = np.float32(self.scale) == np.float32(np.float64(256.0) / np.float64(np.float32(self.voxel)))
        ok = ok and 1 <= self.nx <= 4096 and 1 <= self.ny <= 4096 and 1 <= self.nz <= 256
        if not ok:
            raise ValueError("accumulate: parameters outside finite floats, voxel > 0, scale == (float)(256.0 / voxel), 1 <= nx, ny <= 4096, "
                             "1 <= nz <= 256")
        return self


def capacity_for(rows: int) -> int:
    """rule G: the next power of two at or above twice ``rows``, inside what the library admits"""
    cap = MIN_CAPACITY
    while cap < 2 * int(rows) and cap < MAX_CAPACITY:
        cap <<= 1
    return cap


def sources(t: int, n_sweeps: int, window: int = 10) -> list:
    """rule G: the source sweeps of target ``t``, oldest first"""
    if not 0 <= int(window) <= MAX_WINDOW:
        raise ValueError(f"window={window}: 0..{MAX_WINDOW}")
    if not 0 <= t < n_sweeps:
        raise IndexError(f"target sweep {t} of {n_sweeps}")
    return list(range(max(0, t - int(window)), t + 1))


class Accumulator:
    """A voxel table on ``device``: ``clear()``, ``add(points, T, lag, skip=None)`` any number of times, ``result()``.  ``capacity``: a
    power of two in 2^4 .. 2^26, at least the number of voxels that will be occupied (``capacity_for``).  Everything is asynchronous on
    the current stream but ``result()``, which waits once."""

    def __init__(self, device=None, params: AccumParams | None = None, capacity: int = 1 << 22):
        import torch
        from . import _lib
        self.params = (params if params is not None else AccumParams()).check()
        self.lib = _lib.load()
        self.capacity = int(capacity)
        nbytes = int(self.lib.himo_accum_table_bytes(self.capacity))
        if nbytes == 0:
            raise ValueError(f"accumulate: capacity {capacity} is not a power of two in 2^4 .. 2^26")
        self.device = device if device is not None else _lib.require_gpu()
        self.table = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device)
        self._n_rows = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._host = _lib.pinned_empty(1, torch.int32)
        self.rows = 0
        self.clear()

    def clear(self) -> None:
        from . import _lib
        _lib.check(self.lib.himo_accum_clear(_lib.ptr(self.table), self.capacity, _lib.stream_handle()), "himo_accum_clear")
        self.rows = 0
        self.intensity_scale = None                 # rule H: the one scale of the attributes inserted since

    def add(self, points, T, lag: int, skip=None, motion=None, motion_min: float = 0.0, intensity=None, intensity_scale: float = 1.0,
            label=None) -> None:
        """insert one source sweep: ``points`` device float32 [n, 3 or 4] in its own frame, ``T`` its 4x4 transform into the target's
        frame (rounded to float32 here), ``lag`` 0..255, ``skip`` device uint8 / bool [n] (non-zero = the row takes no part).
        v2, each optional: ``motion`` device float32 [n, 3] (rule A2; rows moving less than ``motion_min`` a sweep stay), ``intensity``
        device float32 [n], a strided view such as ``points[:, 3]`` included, quantised at ``intensity_scale`` (rule H), ``label``
        device int32 [n].  With none of the three this is v1's insert."""
        import torch
        from . import _lib
        if points.dim() != 2 or points.shape[1] not in (3, 4) or points.dtype != torch.float32 or not points.is_contiguous():
            raise ValueError(f"points are contiguous float32 rows of 3 or 4 columns, not {tuple(points.shape)} {points.dtype}")
        n = int(points.shape[0])
        if skip is not None:
            skip = skip.to(torch.uint8).contiguous()
            if skip.shape != (n,):
                raise ValueError(f"skip is [{n}], not {tuple(skip.shape)}")
        if self.rows + n > MAX_ROWS:
            raise ValueError(f"accumulate: {self.rows} + {n} rows since the last clear() exceed 2^24 (the 32-bit sums of rule D)")
        T32 = np.ascontiguousarray(np.asarray(T).astype(np.float32)).reshape(16)
        T_ptr = T32.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        if motion is None and intensity is None and label is None:
            st = self.lib.himo_accum_insert(n, _lib.ptr(points), int(points.shape[1]), _lib.ptr(skip), T_ptr, int(lag), ctypes.addressof(self.params),
                                            _lib.ptr(self.table), self.capacity, _lib.stream_handle())
            _lib.check(st, "himo_accum_insert")
            self.rows += n
            return
        if motion is not None and (motion.shape != (n, 3) or motion.dtype != torch.float32 or not motion.is_contiguous()):
            raise ValueError(f"motion is contiguous float32 [{n}, 3], not {tuple(motion.shape)} {motion.dtype}")
        if not (np.isfinite(motion_min) and motion_min >= 0):
            raise ValueError(f"motion_min={motion_min}: finite and >= 0")
        with np.errstate(all="ignore"):
            min2 = float(np.float32(np.float64(motion_min) * np.float64(motion_min)))       # rule A2: squared in double on the host
        stride = 1
        if intensity is not None:
            if intensity.shape != (n,) or intensity.dtype != torch.float32 or (n > 1 and intensity.stride(0) < 1):
                raise ValueError(f"intensity is float32 [{n}] at a positive stride, not {tuple(intensity.shape)} {intensity.dtype}")
            scale = float(np.float32(intensity_scale))
            if not (np.isfinite(scale) and scale > 0):
                raise ValueError(f"intensity_scale={intensity_scale}: finite and > 0")
            if self.intensity_scale not in (None, scale):
                raise ValueError(f"intensity_scale={scale}: {self.intensity_scale} has been used since the last clear()")
            stride = int(intensity.stride(0)) if n > 1 else 1
        else:
            scale = 1.0
        if label is not None and (label.shape != (n,) or label.dtype != torch.int32 or not label.is_contiguous()):
            raise ValueError(f"label is contiguous int32 [{n}], not {tuple(label.shape)} {label.dtype}")
        st = self.lib.himo_accum_insert_ex(n, _lib.ptr(points), int(points.shape[1]), _lib.ptr(skip), T_ptr, int(lag), ctypes.addressof(self.params),
                                           _lib.ptr(self.table), self.capacity, _lib.ptr(motion), min2, _lib.ptr(intensity), stride, scale,
                                           _lib.ptr(label), _lib.stream_handle())
        _lib.check(st, "himo_accum_insert_ex")
        if intensity is not None:
            self.intensity_scale = scale
        self.rows += n

    def _emit(self, ex: bool):
        import torch
        from . import _lib
        room = min(self.rows, self.capacity + 1)
        dev = self.device
        keys = torch.empty(room, dtype=torch.int32, device=dev)
        xyz = torch.empty((room, 3), dtype=torch.float32, device=dev)
        lag = torch.empty(room, dtype=torch.uint8, device=dev)
        count = torch.empty(room, dtype=torch.int32, device=dev)
        at = lambda t: _lib.ptr(t) if room else None              # noqa: E731
        if ex:
            inten = torch.empty(room, dtype=torch.float32, device=dev)
            label = torch.empty(room, dtype=torch.int32, device=dev)
            st = self.lib.himo_accum_emit_ex(_lib.ptr(self.table), self.capacity, ctypes.addressof(self.params), room, _lib.ptr(self._n_rows), at(keys),
                                             at(xyz), at(lag), at(count), 1.0 if self.intensity_scale is None else self.intensity_scale, at(inten),
                                             at(label), _lib.stream_handle())
            _lib.check(st, "himo_accum_emit_ex")
        else:
            st = self.lib.himo_accum_emit(_lib.ptr(self.table), self.capacity, ctypes.addressof(self.params), room, _lib.ptr(self._n_rows), at(keys),
                                          at(xyz), at(lag), at(count), _lib.stream_handle())
            _lib.check(st, "himo_accum_emit")
        self._host.copy_(self._n_rows, non_blocking=True)
        _lib.check(self.lib.himo_accum_status(_lib.stream_handle()),                      # (waits for the stream: the count has arrived too)
                   f"himo_accum_insert: the table of capacity {self.capacity} was full")
        m = int(self._host[0])
        keys64 = keys[:m].to(torch.int64) & 0xFFFFFFFF
        keys64, order = torch.sort(keys64)
        out = (xyz[:m][order], lag[:m][order], count[:m][order], keys64)
        return out + (inten[:m][order], label[:m][order]) if ex else out

    def result(self):
        """(xyz float32 [M, 3], lag uint8 [M], count int32 [M], keys int64 [M]): device tensors, one row per occupied voxel in
        ascending key order.  Waits for the stream once, for the row count and the status; raises ValueError if the table was full."""
        return self._emit(False)

    def result_ex(self):
        """``result()`` and rule E2's columns: (xyz, lag, count, keys, intensity float32 [M], label int32 [M]), sorted by key as
        ``result()`` sorts.  The intensity is divided by the ``intensity_scale`` of the inserts since the last ``clear()`` (1 when none
        carried an intensity: the column is zeros then)."""
        return self._emit(True)


def device_rows(pc, dev):
    import torch
    t = pc if isinstance(pc, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32))
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"points are rows of x, y, z[, ...], not {tuple(t.shape)}")
    t = t.to(device=dev, dtype=torch.float32)
    return t.contiguous() if t.shape[1] in (3, 4) else t[:, :3].contiguous()


def flow_motion(pc0, flow, pose0, pose1):
    """Rule I: a sweep's own motion per sweep period, device float32 [n, 3], from its raw rows ``pc0`` ((n, >= 3) array or device
    tensor), a stored ``flow`` [n, 3] that includes ego motion, and the poses of the sweep and of its successor."""
    import torch
    from . import _lib
    dev = pc0.device if isinstance(pc0, torch.Tensor) and pc0.is_cuda else _lib.require_gpu()
    pts = device_rows(pc0, dev)
    n = int(pts.shape[0])
    fl = flow if isinstance(flow, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32))
    fl = fl.to(device=dev, dtype=torch.float32).contiguous()
    if fl.shape != (n, 3):
        raise ValueError(f"flow is [{n}, 3], not {tuple(fl.shape)}")
    E = (np.linalg.inv(np.asarray(pose1, dtype=np.float64)) @ np.asarray(pose0, dtype=np.float64)).astype(np.float32)
    E = np.ascontiguousarray(E).reshape(16)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.load().himo_accum_motion(n, _lib.ptr(pts), int(pts.shape[1]), _lib.ptr(fl), E.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           _lib.ptr(out), _lib.stream_handle())
    _lib.check(st, "himo_accum_motion")
    return out


def _device_column(a, dev, dtype):
    import torch
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32 if dtype == torch.int32 else np.float32, copy=False)).to(dev)


def accumulate_target(sweeps, poses, t: int, window: int = 10, params: AccumParams | None = None, skips=None, acc: Accumulator | None = None,
                      motions=None, intensities=None, labels=None, motion_min: float = 0.0, intensity_scale: float = 1.0):
    """Rule G for target sweep ``t`` of one scene: what ``Accumulator.result`` returns.  ``sweeps``: the scene's (compensated) sweeps in
    order, (n, >= 3) float32 arrays or device tensors in their own frames (only the sources are touched); ``poses``: their 4x4 world
    poses; ``skips``: per sweep None or a uint8 / bool mask of rows to leave out; ``acc``: a table to clear and use (its capacity must
    do), else one of ``capacity_for`` the window's rows.
    v2: ``motions``, ``intensities``, ``labels``: per sweep None or [n, 3] float32 / [n] float32 / [n] integer arrays or device tensors
    (rules A2 and H; ``motion_min`` and ``intensity_scale`` hold for every source).  With ``intensities`` or ``labels`` given the return
    is what ``Accumulator.result_ex`` returns."""
    import torch
    from . import _lib
    dev = acc.device if acc is not None else _lib.require_gpu()
    src = sources(int(t), len(sweeps), window)
    pts = {k: device_rows(sweeps[k], dev) for k in src}
    of = lambda seq, k, dtype: None if seq is None else _device_column(seq[k], dev, dtype)        # noqa: E731
    if acc is None:
        acc = Accumulator(dev, params, capacity_for(sum(int(p.shape[0]) for p in pts.values())))
    else:
        acc.clear()
    inv_t = np.linalg.inv(np.asarray(poses[t], dtype=np.float64))
    for k in src:
        T = (inv_t @ np.asarray(poses[k], dtype=np.float64)).astype(np.float32)
        s = None if skips is None or skips[k] is None else skips[k]
        if s is not None and not isinstance(s, torch.Tensor):
            s = torch.from_numpy(np.ascontiguousarray(s).astype(np.uint8))
        mo, it, la = of(motions, k, torch.float32), of(intensities, k, torch.float32), of(labels, k, torch.int32)
        acc.add(pts[k], T, t - k, None if s is None else s.to(dev), motion=None if mo is None else mo.contiguous(), motion_min=motion_min,
                intensity=it, intensity_scale=intensity_scale, label=None if la is None else la.contiguous())
    return acc.result() if intensities is None and labels is None else acc.result_ex()


# --------------------------------------------------------------------------------------------------------------------------
# the program
# --------------------------------------------------------------------------------------------------------------------------
def _writers(key: str) -> str:
    return "`python -m himo_amd.ground_seg` writes the masks" if key == "ground_mask" else \
        "`python -m himo_amd.raymap` writes ray_label / ray_dynamic"


MOTION_MIN = 0.05                   # --motion_min: the project's static threshold [m a sweep] (RigidParams.static_disp)


def _motion_key(res_name: str, advect: bool, motion_key: str | None):
    """the stored flow ``--advect`` moves by, or None; refuses ``raw`` (no flow is stored under that name)"""
    if not advect:
        return None
    key = motion_key if motion_key else res_name
    if key == "raw":
        raise ValueError("--advect needs a stored flow to move by: --res_name raw has none, name one with --motion_key (<res>_rigid of "
                         "`python -m himo_amd.rigid_refine` is the coherent choice)")
    return key


def write_bin(path, xyz, intensity, lag) -> None:
    """``--bin_dir``: little-endian float32 [M][5] = x, y, z, intensity, lag * 0.1 -- the nuScenes sweep row OpenPCDet reads"""
    rows = np.empty((len(xyz), 5), dtype="<f4")
    rows[:, :3], rows[:, 3] = xyz, 0.0 if intensity is None else intensity
    rows[:, 4] = lag.astype(np.float32) * np.float32(LAG_SECONDS)
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    rows.tofile(path)


def accumulate_scene(dataset, items: list, out_path, res_name: str = "seflowpp_best", window: int = 10, params: AccumParams | None = None,
                     drop_ground: bool = False, drop_label: str | None = None, opener=None, advect: bool = False, motion_key: str | None = None,
                     motion_min: float = MOTION_MIN, intensity: bool = False, intensity_scale: float = 1.0, carry_label: str | None = None,
                     bin_dir=None) -> dict:
    """One scene: ``items`` are the dataset's indices of its sweeps that have a successor, in order (the targets, and the sources).
    Compensates every sweep once, accumulates every target, then writes ``out_path``.  Returns {"sweeps", "rows_in", "rows_out",
    "seconds"} (seconds: upload, compensation, accumulation and the copy back; no file time).  The keywords from ``advect`` on are the
    program's v2 flags; with none of them set this is v1, call for call."""
    import torch
    from . import _lib
    from .compdis import CompDisEngine
    params = (params if params is not None else AccumParams()).check()
    sources(0, 1, window)
    motion_key = _motion_key(res_name, advect, motion_key)
    v2 = bool(motion_key or intensity or carry_label)
    dev = _lib.require_gpu()
    frames = [dataset[i] for i in items]
    scene = frames[0]["scene_id"] if frames else Path(out_path).stem
    for f in frames:
        if res_name != "raw" and res_name not in f:
            raise KeyError(res_name)                                              # as save_zip / eval on a scene without the result
        if drop_ground and "gm0" not in f:
            raise KeyError(f"ground_mask: {scene} sweep {f['timestamp']} has no ground mask ({_writers('ground_mask')})")
        if drop_label and drop_label not in f:
            raise KeyError(f"{drop_label}: {scene} sweep {f['timestamp']} has no such label ({_writers(drop_label)})")
        if motion_key and motion_key not in f:
            raise KeyError(motion_key)
        if carry_label and carry_label not in f:
            raise KeyError(f"{carry_label}: {scene} sweep {f['timestamp']} has no such label ({_writers(carry_label)})")
        if intensity and np.asarray(f["pc0"]).shape[1] < 4:
            raise ValueError(f"--intensity: the lidar rows of {scene} sweep {f['timestamp']} have no fourth column")
    t0 = time.perf_counter()
    out, rows_in = [], 0
    with torch.cuda.device(dev):
        engine = CompDisEngine()
        moved, skips, motions, intens, labels = [], [], [], [], []
        for f in frames:
            pc0 = device_rows(f["pc0"], dev)
            motions.append(flow_motion(pc0, f[motion_key], f["pose0"], f["pose1"]) if motion_key else None)
            if intensity:                                                     # column 3 of the raw rows, read in place where they have four
                intens.append(pc0[:, 3] if pc0.shape[1] == 4 else _device_column(np.asarray(f["pc0"])[:, 3], dev, torch.float32))
            else:
                intens.append(None)
            labels.append(_device_column(np.asarray(f[carry_label]), dev, torch.int32) if carry_label else None)
            if res_name == "raw":
                moved.append(pc0)
            else:
                flow = torch.from_numpy(np.ascontiguousarray(f[res_name], dtype=np.float32)).to(dev)
                dt = torch.from_numpy(np.ascontiguousarray(f["lidar_dt"], dtype=np.float32)).to(dev)
                moved.append(engine.run_frame(pc0, flow, dt, f["pose0"], f["pose1"], refined=True)[1])
            skip = None
            if drop_ground:
                skip = torch.from_numpy(np.ascontiguousarray(f["gm0"]).astype(np.uint8)).to(dev)
            if drop_label:
                lab = torch.from_numpy(np.ascontiguousarray(np.asarray(f[drop_label]) != 0).astype(np.uint8)).to(dev)
                skip = lab if skip is None else skip | lab
            skips.append(skip)
        poses = [np.asarray(f["pose0"]) for f in frames]
        most = max((sum(int(moved[k].shape[0]) for k in sources(t, len(frames), window)) for t in range(len(frames))), default=0)
        acc = Accumulator(dev, params, capacity_for(most))
        for t in range(len(frames)):
            if v2:
                xyz, lag, count, _, inten, lab = accumulate_target(moved, poses, t, window, skips=skips, acc=acc, motions=motions if motion_key else None,
                                                                   intensities=intens, labels=labels, motion_min=motion_min,
                                                                   intensity_scale=intensity_scale)
                extra = (inten.cpu().numpy() if intensity else None, lab.cpu().numpy() if carry_label else None)
            else:
                xyz, lag, count, _ = accumulate_target(moved, poses, t, window, skips=skips, acc=acc)
                extra = (None, None)
            rows_in += acc.rows
            out.append((xyz.cpu().numpy(), lag.cpu().numpy(), count.cpu().numpy()) + extra)
    seconds = time.perf_counter() - t0
    if opener is None:
        from .stored import h5_module
        mod = h5_module(f"{out_path}: writing a scene file")
        opener = lambda p: mod.File(p, "a")                                   # noqa: E731
    with opener(out_path) as h:
        for f, (xyz, lag, count, inten, lab) in zip(frames, out):
            g = h.create_group(str(f["timestamp"]))
            lidar = np.empty((len(xyz), 4), dtype=np.float32)
            lidar[:, :3], lidar[:, 3] = xyz, lag.astype(np.float32) * np.float32(LAG_SECONDS)
            g.create_dataset("lidar", data=lidar)
            g.create_dataset("pose", data=np.asarray(f["pose0"]))
            g.create_dataset("lidar_dt", data=np.zeros(len(xyz), dtype=np.float32))
            g.create_dataset("acc_count", data=count.astype(np.int32))
            g.create_dataset("ground_mask", data=np.zeros(len(xyz), dtype=bool))    # no centroid is marked: the viewer and the evaluators ask for a mask
            if inten is not None:
                g.create_dataset("acc_intensity", data=inten.astype(np.float32))
            if lab is not None:
                g.create_dataset("acc_label", data=lab.astype(np.int32))
    if bin_dir is not None:
        for f, (xyz, lag, count, inten, lab) in zip(frames, out):
            write_bin(Path(bin_dir) / str(scene) / f"{f['timestamp']}.bin", xyz, inten, lag)
    return {"sweeps": len(frames), "rows_in": rows_in, "rows_out": int(sum(len(o[0]) for o in out)), "seconds": seconds}


def _write_index(out_dir: Path, entries: list) -> None:
    """``index_total.pkl`` of the output directory: what it held for other scenes, then ``entries``"""
    import pickle
    path = out_dir / "index_total.pkl"
    mine = {s for s, _ in entries}
    kept = []
    if path.exists():
        with open(path, "rb") as fh:
            kept = [[str(s), str(t)] for s, t in pickle.load(fh) if str(s) not in mine]
    with open(path, "wb") as fh:
        pickle.dump(sorted(kept + [[s, t] for s, t in entries], key=lambda e: (e[0], int(e[1]))), fh)


def main(data_dir: str, out_dir: str, res_name: str = "seflowpp_best", window: int = 10, voxel: float = 0.1, drop_ground: bool = False,
         drop_label: str | None = None, data_name: str = "av2", overwrite: bool = False, params: AccumParams | None = None,
         advect: bool = False, motion_key: str | None = None, motion_min: float = MOTION_MIN, intensity: bool = False,
         intensity_scale: float = 1.0, carry_label: str | None = None, bin_dir: str | None = None) -> dict:
    """The program.  Under ``torchrun`` (one rank per GPU) the scenes are dealt round-robin to the ranks, so every file has one writer;
    rank 0 writes the index once every rank is through.  Returns {scene: what ``accumulate_scene`` returned} of this rank."""
    import warnings
    from . import distenv
    from .dataset import HDF5Dataset
    from .stored import check_motion_min, h5_module
    from .sweeps import scene_items
    if data_name not in ("av2", "scania"):
        raise ValueError(f"data_name={data_name!r}: av2 or scania")
    if params is None:
        # the default grid's extent at any voxel size: 102.4 x 102.4 x 8 m
        v = float(voxel)
        cells = lambda extent, top: max(1, min(top, int(round(extent / v)))) if v > 0 and np.isfinite(v) else 0      # noqa: E731
        params = AccumParams(voxel=v, nx=cells(102.4, 4096), ny=cells(102.4, 4096), nz=cells(8.0, 256), data_name=data_name)
    params.check()
    sources(0, 1, window)
    motion_key = _motion_key(res_name, advect, motion_key)
    check_motion_min(motion_min)
    if not (np.isfinite(np.float32(intensity_scale)) and np.float32(intensity_scale) > 0):
        raise ValueError(f"intensity_scale={intensity_scale}: finite and > 0")
    if not sorted(Path(data_dir).glob("*.h5")):
        raise FileNotFoundError(f"{data_dir}: no <scene>.h5 files")
    mod = h5_module(f"writing scene files into {out_dir}")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    fields = {"pc0", "pose0", "pose1", "lidar_dt"} | ({"gm0"} if drop_ground else set()) | ({drop_label} if drop_label else set())
    fields |= {res_name} if res_name != "raw" else set()
    fields |= ({motion_key} if motion_key else set()) | ({carry_label} if carry_label else set())
    stored = [k for k in dict.fromkeys([res_name, motion_key]) if k and k != "raw"]       # the stored flows read, each once
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # (the last sweep of a scene has no successor: no target)
        ds = HDF5Dataset(data_dir, vis_name=stored if stored else "", fields=tuple(fields))
    by_scene = scene_items(ds)
    scenes = sorted(by_scene)
    have = [s for s in scenes if (out_dir / f"{s}.h5").exists()]               # (looked up before the ranks meet: none has written yet)
    done = {}
    with distenv.process_group() as (rank, world):
        def loop():
            if have and not overwrite:
                raise FileExistsError(f"{out_dir}: {len(have)} of {len(scenes)} scene files exist already, {have[0]}.h5 among them (--overwrite replaces them)")
            for s in scenes[rank::world]:
                path = out_dir / f"{s}.h5"
                if path.exists():
                    path.unlink()                                             # --overwrite: the file is written anew
                r = done[s] = accumulate_scene(ds, by_scene[s], path, res_name, window, params, drop_ground, drop_label,
                                               opener=lambda p: mod.File(p, "a"), advect=advect, motion_key=motion_key, motion_min=motion_min,
                                               intensity=intensity, intensity_scale=intensity_scale, carry_label=carry_label, bin_dir=bin_dir)
                rate = r["sweeps"] / r["seconds"] if r["seconds"] > 0 else float("inf")
                print(f"{s}: {r['sweeps']} sweeps, {r['rows_in']} rows in, {r['rows_out']} rows out  ({rate:.1f} sweeps/s)")

        distenv.run_shard(loop, "its scene files", closing=(ds,))
        if rank == 0:
            _write_index(out_dir, [[s, t] for s, t in ds.index])
    return done


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="accumulate the compensated sweeps t - window .. t of every scene into the frame of sweep t, one "
                                             "centroid per voxel (sweep accumulation, v1; parity unpinned: the reference has no such program; "
                                             "MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files and index_total.pkl")
    ap.add_argument("--out_dir", required=True, help="directory the accumulated <scene>.h5 files and their index_total.pkl are written to")
    ap.add_argument("--res_name", default="seflowpp_best", help="the stored flow the sweeps are compensated by; raw = the points as recorded")
    ap.add_argument("--window", type=int, default=10, help=f"past sweeps beside the target (0..{MAX_WINDOW})")
    ap.add_argument("--voxel", type=float, default=0.1, help="voxel edge [m] of the 102.4 x 102.4 x 8 m grid")
    ap.add_argument("--drop_ground", action="store_true", help="leave out rows whose ground_mask is set (python -m himo_amd.ground_seg)")
    ap.add_argument("--drop_label", default=None, metavar="KEY", help="leave out rows whose stored integer label KEY is non-zero (ray_label: "
                                                                      "python -m himo_amd.raymap)")
    ap.add_argument("--data_name", default="av2", choices=("av2", "scania"), help="whose ego box is cut out of every source sweep")
    ap.add_argument("--overwrite", action="store_true", help="replace scene files that exist in --out_dir instead of refusing")
    v2 = ap.add_argument_group("sweep accumulation, v2 (opt-in; parity unpinned; with none of these the files are v1's, byte for byte)")
    v2.add_argument("--advect", action="store_true", help="move every source row along its own motion to the target's time: lag times the stored "
                                                          "flow less the ego motion, one constant-velocity step")
    v2.add_argument("--motion_key", default=None, metavar="KEY", help="the stored flow --advect moves by (default: --res_name); <res>_rigid from "
                                                                      "python -m himo_amd.rigid_refine is the coherent choice, one motion per cluster")
    v2.add_argument("--motion_min", type=float, default=MOTION_MIN, help="rows that move less than this [m per sweep] stay where they are (the "
                                                                         "project's static threshold)")
    v2.add_argument("--intensity", action="store_true", help="carry column 3 of the lidar rows: <timestamp>/acc_intensity, float32 [M], the mean "
                                                             "of a voxel's rows after quantisation to 0..255")
    v2.add_argument("--intensity_scale", type=float, default=1.0, help="what an intensity is multiplied by before it is rounded into 0..255 (255 "
                                                                       "for intensities in 0..1)")
    v2.add_argument("--carry_label", default=None, metavar="KEY", help="carry the stored integer label KEY (ray_label, flow_instance_id): "
                                                                       "<timestamp>/acc_label, int32 [M], the label of a voxel's freshest row")
    v2.add_argument("--bin_dir", default=None, metavar="B", help="additionally write B/<scene>/<timestamp>.bin, little-endian float32 [M][5] = x, y, "
                                                                 "z, intensity, lag * 0.1 (the nuScenes sweep row OpenPCDet reads); the intensity "
                                                                 "column is zeros without --intensity")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.out_dir, a.res_name, a.window, a.voxel, a.drop_ground, a.drop_label, a.data_name, a.overwrite, advect=a.advect,
         motion_key=a.motion_key, motion_min=a.motion_min, intensity=a.intensity, intensity_scale=a.intensity_scale, carry_label=a.carry_label,
         bin_dir=a.bin_dir)


if __name__ == "__main__":
    _cli()
