"""Sweep odometry: the pose of every sweep of a scene from the sweeps alone, by whole-sweep 6-DoF scan-to-map ICP on the GPU
(``python -m himo_amd.odometry``, stored key ``pose_odom``).  Every program of this package takes the ego motion out of a sweep pair
with the stored ``<timestamp>/pose``; this one makes such poses for drives whose logger stored no localisation, and checks stored ones
(``--gt_key pose``).  The reference's README names "ICP alignment" as the alternative route (README.md:36-38); it has no such program.

PARITY UNPINNED.  This stage follows the build's own written rule, below, and is checked against a numpy / Python restatement of it
(``tests/odometry_ref.py``), never against the reference.  It is opt-in: nothing calls it unless asked, and no existing output changes.
Nothing has been tried on field data.

The rule -- "sweep odometry, v1" (normative)
============================================
Every float operation rounds on its own (``himo_amd/csrc/odometry.hip`` is built with ``-ffp-contract=off``); only ``+ - * /`` and
``sqrt`` appear, all correctly rounded; no transcendental is used on the device.

Parameters (``OdomParams``; this build's own choices): ``voxel`` 0.5 m, ``window`` 10, ``max_dist`` 1.0 m, ``gm_scale`` 0.25 m^2,
``min_pairs`` 20, ``iters`` 20, ``eps_t2`` 1e-10 m^2, ``eps_r2`` 1e-12, ``min_ratio`` 0.3, ``init`` "model"; the vote's ``bin`` 0.25 m,
``half`` 16, ``z_gate`` 1.0 m (``IcpParams``).  Admitted: every number finite and positive, ``1 <= window <= accumulate.MAX_WINDOW``,
``0.0625 <= voxel``, ``0.125 <= max_dist`` (the grids below stay inside what ``accumulate`` and the search admit), ``iters <= 1024``,
``half <= 64``, ``min_ratio <= 1``.

0. Inputs and scope.  A scene is its sweeps ``k = 0 .. K-1`` in index order: ``pc_k (N_k, >=3)`` float32 and, optionally, a skip byte
   per row.  A row takes part iff its skip byte is 0, it is finite and it is not strictly inside the ego box: rule A of ``accumulate``
   ("sweep accumulation, v1"), reused as it is.  Ground rows take part: they are what fixes z, roll and pitch.
1. Downsampling, by the existing table.  The source ``S_k`` is ``accumulate_target`` of sweep ``k`` alone with the identity; the local
   map ``M_k`` is ``accumulate_target`` of the sweeps ``max(0, k - window) .. k - 1`` moved into the frame of sweep ``k - 1`` by the
   ESTIMATED poses (``accumulate`` rule G with the window ``window - 1``).  Both use ONE ``AccumParams`` grid: minimum (-64, -64, -8),
   ``voxel``, ``ceil(128 / voxel)`` cells in x and y and ``ceil(16 / voxel)`` in z.  Rows come out as centroids in ascending key order:
   that order is the row order of everything below, and with it every tie and every sum.
2. Initial transform ``T`` (float64 3x4, sweep ``k`` -> frame ``k - 1``).  For ``k >= 2`` the previous relative transform (constant
   velocity).  For ``k = 1``, and after a sweep that was not accepted, the peak of the translation vote of "cluster-rigid ICP, v1" rule 2
   (``himo_icp_vote``) with ``S_k`` as ONE cluster against ``M_k``: ``T = [I | (kx bin, ky bin, 0)]``.  ``init="vote"`` takes the vote for
   every sweep; ``init="model"`` is the default just described.
3. One iteration.  The BEV search grid has the cell edge ``max_dist`` (float32), the minimum (-64, -64) and ``ceil(128 / max_dist)``
   cells a side; the cell of a coordinate is ``clamp((int)floorf((v - v0) * inv_cell), 0, g - 1)`` in float32 with
   ``inv_cell = 1.0f / max_dist`` (rows outside the grid belong to the border cells).  For every row ``p`` of ``S_k``:
   ``m = float32(T p)``, each component evaluated in float64 as ``((T0 x + T1 y) + T2 z) + T3``;
   ``q`` = the nearest row of ``M_k`` among the rows whose cell is within one cell of ``m``'s in x and in y (the 3 x 3 cells), by
   ``d2 = (dx*dx + dy*dy) + dz*dz`` in float32; ties keep the lowest row;
   ``p`` is an inlier iff such a row exists and ``d2 <= max_dist^2``, the product rounded once in float32.  A row whose ``m`` has a
   non-finite component takes no part.
   Over the inliers, in float64 (``m`` and ``q`` widened): ``r = q - m``, ``rr = (rx*rx + ry*ry) + rz*rz``, ``u = s / (s + rr)`` with
   ``s = gm_scale`` widened, ``w = u * u`` (the Geman-McClure weight).  The Jacobian of a small motion ``(t, omega)`` at ``m`` is
   ``J = [I | -[m]x]``.  The sums: the 21 upper entries of ``H = sum w J^T J`` --
   ``H00 = H11 = H22 = sum w``; ``H04 = sum w mz``, ``H05 = sum -(w my)``, ``H13 = sum -(w mz)``, ``H15 = sum w mx``,
   ``H23 = sum w my``, ``H24 = sum -(w mx)``; ``H33 = sum w (my*my + mz*mz)``, ``H34 = sum -(w (mx*my))``, ``H35 = sum -(w (mx*mz))``,
   ``H44 = sum w (mx*mx + mz*mz)``, ``H45 = sum -(w (my*mz))``, ``H55 = sum w (mx*mx + my*my)``; the rest 0 --
   the 6 of ``g = sum w J^T r`` -- ``w rx, w ry, w rz, w (my*rz - mz*ry), w (mz*rx - mx*rz), w (mx*ry - my*rx)`` --
   ``cost = sum w rr`` and the count ``n``.  The ORDER of the sums is not part of the rule: the device takes them in a fixed shape
   (per-block partials through ``blockops.h``, then one fixed pass over the partials; no floating-point atomics: the same bytes on
   every run), the restatement in row order; they agree to rounding.
   Then: ``n < min_pairs``: the status becomes FAILED_PAIRS and ``T`` stays.  Otherwise ``H xi = g`` by an unpivoted Cholesky in
   float64 (column by column: ``d = Hjj - sum_k Ljk Ljk`` subtracted in ascending ``k``, ``Ljj = sqrt(d)``,
   ``Lij = (Hji - sum_k Lik Ljk) / Ljj``; forward and back substitution the same way); a pivot ``d`` that is not finite or not ``> 0``,
   or a component of ``xi`` that is not finite, gives FAILED_SOLVE and ``T`` stays.  With ``xi = (t_xi, omega)``, ``a = 0.5 omega``,
   ``b = 2 a``, ``aa = (ax*ax + ay*ay) + az*az``: ``D = ((1 - aa) I + b a^T + [b]x) / (1 + aa)`` entry by entry -- the Cayley map,
   rational, and orthogonal to rounding -- e.g. ``D00 = ((1 - aa) + bx*ax) / (1 + aa)``, ``D01 = (bx*ay - bz) / (1 + aa)``.
   ``R <- D R`` and ``t <- D t + t_xi``, every entry ``(Di0 a + Di1 b) + Di2 c`` (``+ t_xi`` last).  The status becomes CONVERGED iff
   ``(tx*tx + ty*ty) + tz*tz < eps_t2`` and the same of ``omega`` ``< eps_r2``.  A step launched on a state that is CONVERGED or
   FAILED writes nothing.
4. Registration.  One binning of ``M_k``, then ``iters`` steps, enqueued with no host wait in between (``himo_odom_register``: nothing
   in the call chain allocates or synchronises, and the workspace is the caller's).  The sweep is ACCEPTED iff it has not failed and
   ``n / |S_k| >= min_ratio`` (float64 quotient against ``min_ratio`` as float32) on its last pass.  A sweep that is not accepted takes
   the constant-velocity prediction (the identity for ``k = 1``) and is counted in the table.
5. Chain.  ``pose_k = pose_{k-1} @ T_k`` in float64 numpy on the host; ``pose_0`` is the stored ``pose`` of the first sweep when the
   scene holds one, else the identity.  The registration has one host wait per sweep -- the state, read through pinned memory behind an
   event, as ``icpflow`` reads its counts: the next map is built with the new pose.  (Each of the two accumulations of a sweep waits
   once as well, for its row count, as ``Accumulator.result`` always does.)

Not part of v1: de-skewing by ``lidar_dt`` (a program of its own: ``python -m himo_amd.deskew --pose_key pose_odom``), point-to-plane or normals, an adaptive threshold, a map that persists beyond the window,
loop closure, several scenes in flight, IMU or wheel input, any use of ``SensorsCenter``.

The program: ``python -m himo_amd.odometry --data_dir D [--out_key pose_odom] [--window 10] [--voxel 0.5] [--skip_label KEY]
[--init model|vote] [--gt_key pose] [--json PATH] [--overwrite]``.  It walks whole scenes (``sweeps.sharded_scenes``; every sweep is
read alone, ``need_next=False``, the last one of a scene included) and writes ``<timestamp>/<out_key>`` float64 [4, 4] through
``stored.KeySink``; into the npz container, whose sweeps carry their own successor's pose, also ``<out_key>_next`` (the last sweep
of a scene gets one iff its npz holds ``pc1``, registered as one more sweep).  ``--out_key pose`` is refused, and an existing key
without ``--overwrite``.  It prints, per scene and over all, the sweeps registered, accepted and fallen back, the mean iterations and
the mean inlier share; with ``--gt_key`` also the relative pose error against the stored poses per sweep pair -- mean and max
translation [m] and rotation [degrees] (``math.acos`` on the host only) -- and the end-point drift as a share of the path length.
``--skip_label ray_label`` leaves labelled movers out; a missing key is the ``KeyError`` the other programs raise.  Under ``torchrun``
the scenes are dealt to the ranks as elsewhere.  There is no CPU path.

Consuming the poses: ``open_dataset(..., pose_key="pose_odom")`` or the environment variable ``HIMO_POSE_KEY`` (``dataset.py``) makes
every existing program read ``pose0`` / ``pose1`` from the estimated key.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

RUNNING, CONVERGED, FAILED_PAIRS, FAILED_SOLVE = 0, 1, 2, 3
STATUS_NAMES = ("running", "converged", "failed_pairs", "failed_solve")
GRID_X0, GRID_Y0, GRID_Z0, GRID_XY, GRID_Z = -64.0, -64.0, -8.0, 128.0, 16.0
INITS = ("model", "vote")


class _CParams(ctypes.Structure):
    """mirror of ``himo_odom_params`` (include/himo_amd.h)"""
    _fields_ = [("x0", ctypes.c_float), ("y0", ctypes.c_float), ("max_dist", ctypes.c_float), ("gw", ctypes.c_int32), ("gh", ctypes.c_int32),
                ("gm_scale", ctypes.c_float), ("min_pairs", ctypes.c_int32), ("iters", ctypes.c_int32), ("eps_t2", ctypes.c_double),
                ("eps_r2", ctypes.c_double)]


class _CState(ctypes.Structure):
    """mirror of ``himo_odom_state`` (include/himo_amd.h)"""
    _fields_ = [("T", ctypes.c_double * 12), ("cost", ctypes.c_double), ("xi", ctypes.c_double * 6), ("sums", ctypes.c_double * 28),
                ("status", ctypes.c_int32), ("iters", ctypes.c_int32), ("pairs", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@dataclass(frozen=True)
class OdomParams:
    """the parameters of "sweep odometry, v1"; refuses what the rule does not admit before anything is launched"""
    voxel: float = 0.5
    window: int = 10
    max_dist: float = 1.0
    gm_scale: float = 0.25
    min_pairs: int = 20
    iters: int = 20
    eps_t2: float = 1e-10
    eps_r2: float = 1e-12
    min_ratio: float = 0.3
    init: str = "model"
    bin: float = 0.25
    half: int = 16
    z_gate: float = 1.0
    data_name: str = "av2"

    def __post_init__(self):
        from .accumulate import MAX_WINDOW
        for name in ("voxel", "max_dist", "gm_scale", "eps_t2", "eps_r2", "min_ratio", "bin", "z_gate"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
                raise ValueError(f"OdomParams.{name}={v!r}: a finite, positive number")
            if name not in ("eps_t2", "eps_r2"):
                with np.errstate(all="ignore"):
                    as32 = float(np.float32(v))
                if not math.isfinite(as32) or not as32 > 0:
                    raise ValueError(f"OdomParams.{name}={v!r}: not a positive float32")
        for name in ("window", "min_pairs", "iters", "half"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"OdomParams.{name}={v!r}: a positive integer")
        if self.window > MAX_WINDOW:
            raise ValueError(f"OdomParams.window={self.window}: 1..{MAX_WINDOW}")
        if self.iters > 1024:
            raise ValueError(f"OdomParams.iters={self.iters}: at most 1024")
        if self.half > 64:
            raise ValueError(f"OdomParams.half={self.half}: at most 64")
        if self.voxel < 0.0625:
            raise ValueError(f"OdomParams.voxel={self.voxel}: at least 0.0625 m (the grid's 128 m a side in at most 4096 voxels, 16 m in 256)")
        if self.max_dist < 0.125:
            raise ValueError(f"OdomParams.max_dist={self.max_dist}: at least 0.125 m (the search grid's 128 m a side in at most 1024 cells)")
        if self.min_ratio > 1:
            raise ValueError(f"OdomParams.min_ratio={self.min_ratio}: at most 1")
        if self.init not in INITS:
            raise ValueError(f"OdomParams.init={self.init!r}: one of {', '.join(INITS)}")
        if self.data_name not in ("av2", "scania"):
            raise ValueError(f"OdomParams.data_name={self.data_name!r}: av2 or scania")

    def search_cells(self) -> int:
        return max(1, int(math.ceil(GRID_XY / float(np.float32(self.max_dist)))))

    def c_struct(self) -> _CParams:
        g = self.search_cells()
        return _CParams(GRID_X0, GRID_Y0, self.max_dist, g, g, self.gm_scale, int(self.min_pairs), int(self.iters), float(self.eps_t2),
                        float(self.eps_r2))

    def accum_params(self):
        """rule 1: the ONE grid of both downsamplings"""
        from .accumulate import AccumParams
        v = float(self.voxel)
        cells = lambda extent, top: max(1, min(top, int(math.ceil(extent / v))))        # noqa: E731
        return AccumParams(x0=GRID_X0, y0=GRID_Y0, z0=GRID_Z0, voxel=v, nx=cells(GRID_XY, 4096), ny=cells(GRID_XY, 4096), nz=cells(GRID_Z, 256),
                           data_name=self.data_name).check()

    def icp_params(self):
        from .icpflow import IcpParams
        return IcpParams(bin=self.bin, half=self.half, z_gate=self.z_gate)


@dataclass
class Registration:
    """what one registration left: ``T`` float64 [3, 4] (sweep -> map frame), the status, the passes run, the inliers and cost of the
    last pass, the source rows, rule 4's verdict"""
    T: np.ndarray
    status: int
    iters: int
    pairs: int
    cost: float
    rows: int
    accepted: bool
    xi: np.ndarray
    sums: np.ndarray
    init: str = ""                   # set by ``scene``: "model" or "vote"
    T44: np.ndarray | None = None    # set by ``scene``: the relative transform the chain took

    @property
    def share(self) -> float:
        return self.pairs / self.rows if self.rows else 0.0


def as44(T) -> np.ndarray:
    out = np.eye(4)
    out[:3] = np.asarray(T, np.float64).reshape(3, 4)
    return out


STATE_BYTES = ctypes.sizeof(_CState)


class SweepOdometry:
    """``SweepOdometry(device, params).register(src, map, T_init)`` -> ``Registration``; ``.scene(sweeps, skips, pose_first)`` -> (poses
    float64 [K, 4, 4], the ``Registration`` of every sweep k >= 1).  There is no CPU path."""

    def __init__(self, device=None, params: OdomParams | None = None):
        import torch
        from . import _lib
        self.params = params if params is not None else OdomParams()
        self.lib = _lib.load()
        for name, mirror in (("himo_odom_params", _CParams), ("himo_odom_state", _CState)):
            if self.lib.himo_abi_sizeof(name.encode()) != ctypes.sizeof(mirror):
                raise ImportError(f"{name}: the ctypes mirror does not have the library's size")
        self.device = device if device is not None else _lib.require_gpu()
        self._c = self.params.c_struct()
        self._icp = self.params.icp_params().c_struct()
        self._accum = self.params.accum_params()
        self.state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=self.device)
        self._host = _lib.pinned_empty(STATE_BYTES, torch.uint8)
        self._ws = None
        self._vote = None
        self.stage_events = None             # set to a list to have register() append (stage, start event, end event) triples

    # ---- the raw calls (also what the tests drive) -------------------------------------------------------------------------------
    def workspace(self, n_map: int):
        """the grow-only workspace, large enough for a map of ``n_map`` rows and for the vote against it"""
        import torch
        need = max(int(self.lib.himo_odom_workspace_bytes(int(n_map), ctypes.addressof(self._c))), int(self.lib.himo_icp_workspace_bytes(int(n_map), 1)), 16)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + need // 4, dtype=torch.uint8, device=self.device)
        return self._ws

    def init_state(self, T_init=None, d_vote=None) -> None:
        from . import _lib
        T = None if T_init is None else np.ascontiguousarray(np.asarray(T_init, np.float64).reshape(-1)[:12])
        _lib.check(self.lib.himo_odom_init(None if T is None else T.ctypes.data, _lib.ptr(d_vote), _lib.ptr(self.state), _lib.stream_handle()),
                   "himo_odom_init")

    def read_state(self) -> _CState:
        """the registration's one host wait: the state through pinned memory behind an event"""
        import torch
        self._host.copy_(self.state, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record(torch.cuda.current_stream(self.device))
        landed.synchronize()
        return _CState.from_buffer_copy(self._host.numpy().tobytes())

    def _rows(self, pts, widths):
        import torch
        t = pts if isinstance(pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32))
        t = t.to(device=self.device, dtype=torch.float32)
        if t.dim() != 2 or t.shape[1] not in widths:
            raise ValueError(f"rows of {' or '.join(map(str, widths))} float32 columns, not {tuple(t.shape)}")
        return t.contiguous()

    def _mark(self, stage, start):
        import torch
        if self.stage_events is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(self.device))
        if start is not None:
            self.stage_events.append((stage, start, ev))
        return ev

    def vote(self, src, mp):
        """rule 2's vote, enqueued: the device double[5] transform ``himo_icp_vote`` writes for the one cluster (None without rows)"""
        import torch
        from . import _lib
        n, m = int(src.shape[0]), int(mp.shape[0])
        if n == 0:
            return None
        W = 2 * int(self.params.half) + 1
        if self._vote is None:
            dev = self.device
            self._vote = (torch.empty((1, W, W), dtype=torch.int32, device=dev), torch.empty((1, 2), dtype=torch.int32, device=dev),
                          torch.empty((1, 5), dtype=torch.float64, device=dev), torch.empty((1, 4), dtype=torch.int32, device=dev),
                          torch.zeros(2, dtype=torch.int64, device=dev))
        counts, peak, Tm, status, d_off = self._vote
        h_off = np.array([0, n], np.int64)
        d_off.copy_(torch.from_numpy(h_off), non_blocking=False)
        ws = self.workspace(m)
        _lib.check(self.lib.himo_icp_vote(n, _lib.ptr(src), int(src.shape[1]), 1, h_off.ctypes.data, _lib.ptr(d_off), m, _lib.ptr(mp) if m else None,
                                          ctypes.addressof(self._icp), _lib.ptr(counts), _lib.ptr(peak), _lib.ptr(Tm), _lib.ptr(status), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_handle()), "himo_icp_vote")
        return Tm

    def register(self, src, mp, T_init=None, vote: bool = False) -> Registration:
        """rules 2-4 for one sweep: ``src`` [n, 3 or 4] and ``mp`` [m, 3] float32 rows (arrays or device tensors), ``T_init`` the
        3x4 / 4x4 start (None: the identity); ``vote``: the translation x, y of the start comes from rule 2's vote instead"""
        import torch
        from . import _lib
        with torch.cuda.device(self.device):
            src, mp = self._rows(src, (3, 4)), self._rows(mp, (3,))
            n, m = int(src.shape[0]), int(mp.shape[0])
            ws = self.workspace(m)
            t0 = self._mark("vote", None)
            d_vote = self.vote(src, mp) if vote else None
            self.init_state(T_init, d_vote)
            t1 = self._mark("vote", t0)
            _lib.check(self.lib.himo_odom_register(n, _lib.ptr(src) if n else None, int(src.shape[1]), m, _lib.ptr(mp) if m else None,
                                                   ctypes.addressof(self._c), _lib.ptr(self.state), _lib.ptr(ws), ws.numel(), _lib.stream_handle()),
                       "himo_odom_register")
            self._mark("register", t1)
            return self.result(n)

    def result(self, rows: int) -> Registration:
        st = self.read_state()
        ok = st.status in (RUNNING, CONVERGED) and rows > 0 and st.pairs / rows >= float(np.float32(self.params.min_ratio))
        return Registration(np.array(st.T, np.float64).reshape(3, 4), int(st.status), int(st.iters), int(st.pairs), float(st.cost), int(rows), bool(ok),
                            np.array(st.xi, np.float64), np.array(st.sums, np.float64))

    def scene(self, sweeps, skips=None, pose_first=None):
        """rules 1-5 over one scene: ``sweeps`` in index order ((n, >= 3) float32 arrays or device tensors), ``skips`` per sweep None or a
        uint8 / bool mask of rows to leave out, ``pose_first`` the 4x4 pose of sweep 0 (None: the identity).  Returns (poses float64
        [K, 4, 4], [Registration of sweep k for k = 1 .. K-1]); a ``Registration`` carries ``init`` ("model" / "vote") and ``T44``, the
        relative transform the chain took (the prediction where the sweep was not accepted)."""
        import torch
        from .accumulate import Accumulator, accumulate_target, capacity_for, device_rows
        p = self.params
        eye = np.eye(4)
        poses = [eye.copy() if pose_first is None else np.asarray(pose_first, np.float64).reshape(4, 4).copy()]
        out = []
        if len(sweeps) == 0:
            return np.zeros((0, 4, 4)), out
        with torch.cuda.device(self.device):
            pts = [device_rows(s, self.device) for s in sweeps]
            sk = [None] * len(pts) if skips is None else [None if s is None else (s if isinstance(s, torch.Tensor) else torch.from_numpy(
                np.ascontiguousarray(s).astype(np.uint8))).to(self.device) for s in skips]
            counts = [int(x.shape[0]) for x in pts]
            w = int(p.window)
            most = max((sum(counts[max(0, k - w):k]) for k in range(1, len(pts))), default=0)
            acc_src = Accumulator(self.device, self._accum, capacity_for(max(counts)))
            acc_map = Accumulator(self.device, self._accum, capacity_for(most))
            prev, failed = None, True
            for k in range(1, len(pts)):
                S = accumulate_target([pts[k]], [eye], 0, 0, skips=[sk[k]], acc=acc_src)[0]
                M = accumulate_target(pts[:k], poses[:k], k - 1, w - 1, skips=sk[:k], acc=acc_map)[0]
                use_vote = p.init == "vote" or prev is None or failed
                r = self.register(S, M, None if use_vote else prev[:3], vote=use_vote)
                r.init = "vote" if use_vote else "model"
                r.T44 = as44(r.T) if r.accepted else (eye.copy() if prev is None else prev)
                out.append(r)
                poses.append(poses[-1] @ r.T44)
                prev, failed = r.T44, not r.accepted
        return np.stack(poses), out


# --------------------------------------------------------------------------------------------------------------------------
# the tables
# --------------------------------------------------------------------------------------------------------------------------
def rotation_angle_deg(R) -> float:
    """the angle of a rotation matrix in degrees (``math.acos`` of the clipped half trace less a half; host only)"""
    c = (float(np.trace(np.asarray(R, np.float64)[:3, :3])) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def rpe_table(est, gt) -> dict:
    """The relative pose error of the chain ``est`` against ``gt`` (both [K, 4, 4]) per sweep pair: ``E_k = inv(inv(gt_{k-1}) gt_k) @
    (inv(est_{k-1}) est_k)``; its translation norm [m] and rotation angle [degrees], as sums and maxima (``pairs`` of them), and the
    end-point drift: the norm of the translation of ``inv(inv(gt_0) gt_last) @ (inv(est_0) est_last)`` beside the path length, the sum
    of the norms of gt's relative translations."""
    est, gt = np.asarray(est, np.float64), np.asarray(gt, np.float64)
    if est.shape != gt.shape or est.ndim != 3 or est.shape[1:] != (4, 4):
        raise ValueError(f"pose chains of one shape [K, 4, 4], not {est.shape} and {gt.shape}")
    out = {"pairs": 0, "t_sum": 0.0, "t_max": 0.0, "r_sum": 0.0, "r_max": 0.0, "drift": 0.0, "path": 0.0}
    inv = np.linalg.inv
    for k in range(1, len(est)):
        a, b = inv(est[k - 1]) @ est[k], inv(gt[k - 1]) @ gt[k]
        e = inv(b) @ a
        t, r = float(np.linalg.norm(e[:3, 3])), rotation_angle_deg(e)
        out["pairs"] += 1
        out["t_sum"] += t
        out["r_sum"] += r
        out["t_max"], out["r_max"] = max(out["t_max"], t), max(out["r_max"], r)
        out["path"] += float(np.linalg.norm(b[:3, 3]))
    if len(est) > 1:
        e = inv(inv(gt[0]) @ gt[-1]) @ (inv(est[0]) @ est[-1])
        out["drift"] = float(np.linalg.norm(e[:3, 3]))
    return out


def new_sums() -> dict:
    return {"scenes": 0, "sweeps": 0, "accepted": 0, "fallen": 0, "iters": 0, "share": 0.0, "pairs": 0, "t_sum": 0.0, "t_max": 0.0, "r_sum": 0.0,
            "r_max": 0.0, "drift": 0.0, "path": 0.0}


def scene_sums(regs, rpe: dict | None) -> dict:
    s = new_sums()
    s["scenes"] = 1
    s["sweeps"], s["accepted"] = len(regs), sum(1 for r in regs if r.accepted)
    s["fallen"] = s["sweeps"] - s["accepted"]
    s["iters"], s["share"] = sum(r.iters for r in regs), float(sum(r.share for r in regs))
    if rpe is not None:
        s.update(rpe)
    return s


def fold_sums(a: dict, b: dict) -> dict:
    """two running sums as one: counts and sums add, maxima take the larger"""
    return {k: max(a[k], b[k]) if k.endswith("_max") else a[k] + b[k] for k in a}


def numbers_of(s: dict, with_gt: bool) -> dict:
    from .stored import ratio
    out = {"scenes": s["scenes"], "sweeps": s["sweeps"], "accepted": s["accepted"], "fallen_back": s["fallen"],
           "mean_iters": ratio(s["iters"], s["sweeps"]), "mean_inlier_share": ratio(s["share"], s["sweeps"])}
    if with_gt:
        out.update({"rpe_pairs": s["pairs"], "rpe_t_mean_m": ratio(s["t_sum"], s["pairs"]), "rpe_t_max_m": s["t_max"] if s["pairs"] else None,
                    "rpe_r_mean_deg": ratio(s["r_sum"], s["pairs"]), "rpe_r_max_deg": s["r_max"] if s["pairs"] else None,
                    "drift_m": s["drift"], "path_m": s["path"], "drift_share": ratio(s["drift"], s["path"])})
    return out


def _line(name: str, n: dict, with_gt: bool) -> str:
    from .stored import fmt
    text = (f"  {name}: {n['sweeps']} sweeps registered, {n['accepted']} accepted, {n['fallen_back']} fallen back, mean iterations "
            f"{fmt(n['mean_iters'], '.1f')}, mean inlier share {fmt(n['mean_inlier_share'])}")
    if with_gt:
        text += (f"; RPE translation mean {fmt(n['rpe_t_mean_m'], '.4f')} max {fmt(n['rpe_t_max_m'], '.4f')} m, rotation mean "
                 f"{fmt(n['rpe_r_mean_deg'], '.4f')} max {fmt(n['rpe_r_max_deg'], '.4f')} deg, end-point drift {fmt(n['drift_share'], '.5f')} of "
                 f"{fmt(n['path_m'], '.2f')} m")
    return text


# --------------------------------------------------------------------------------------------------------------------------
# the program
# --------------------------------------------------------------------------------------------------------------------------
def main(data_dir: str, out_key: str = "pose_odom", window: int = 10, voxel: float = 0.5, skip_label: str | None = None, init: str = "model",
         gt_key: str | None = None, json_path: str | None = None, overwrite: bool = False, data_name: str = "av2", **params) -> dict:
    """The program (module docstring).  Returns what ``--json`` writes: {"scenes": {scene: numbers}, "all": numbers} over every rank."""
    from . import distenv, stored
    from .dataset import NpzDataset, open_dataset
    from .sweeps import sharded_scenes
    if not out_key or out_key in ("pose", "pose0", "pose1") or out_key.endswith("_next"):
        raise ValueError(f"--out_key {out_key}: the estimated poses are stored beside the recorded `pose`, never over it (pose_odom is the default; a "
                         "name that ends in _next is taken by the npz container's successor pose)")
    prm = OdomParams(voxel=voxel, window=window, init=init, data_name=data_name, **params)
    root = Path(data_dir)
    per_scene = {}
    with distenv.process_group() as (rank, world):
        fields = ("pc0",) + ((skip_label,) if skip_label else ())
        ds = open_dataset(root, vis_name="", eval=False, fields=fields, need_next=False, pose_key="pose")    # (no pose is read through the loader)
        npz = isinstance(ds, NpzDataset)
        stored_pose = "pose0" if npz else "pose"                     # the recorded pose of a sweep under the container's own name
        gt_name = None if gt_key is None else (stored_pose if gt_key == "pose" else gt_key)
        mine = sharded_scenes(ds)

        def loop():
            # the refusals, before anything touches the GPU or a file is written
            sink = stored.KeySink(ds, root, f"writing '{out_key}' into the scene files of {data_dir}")
            for sc, items in mine:
                for i in items:
                    where = "/".join(map(str, ds.index[i]))
                    have = stored.present(ds, i, [out_key] + ([skip_label] if skip_label else []) + ([gt_name] if gt_name else []))
                    if skip_label and skip_label not in have:
                        raise KeyError(f"{skip_label}: {where} has no such label (`python -m himo_amd.raymap` writes ray_label / ray_dynamic)")
                    if gt_name and gt_name not in have:
                        raise KeyError(f"{gt_key}: {where} holds no such pose to compare with")
                    if out_key in have and not overwrite:
                        raise FileExistsError(f"{where} already holds '{out_key}': pass --overwrite to replace it")
            if not mine:
                return
            odo = SweepOdometry(params=prm)
            for sc, items in mine:
                frames = [ds[i] for i in items]
                sweeps = [np.asarray(f["pc0"]) for f in frames]
                if npz and "pc1" in frames[-1]:
                    sweeps.append(np.asarray(frames[-1]["pc1"]))     # the container's last sweep carries its successor: one more pose
                skips = None
                if skip_label:
                    skips = [np.ascontiguousarray(np.asarray(f[skip_label]) != 0) for f in frames]
                    for f, s, pc in zip(frames, skips, sweeps):
                        stored.check_point_labels(np.asarray(f[skip_label]), skip_label, f"{sc}/{f['timestamp']}", rows=len(pc))
                    skips += [None] * (len(sweeps) - len(frames))
                first = stored.arrays(ds, items[0], [stored_pose]).get(stored_pose)
                poses, regs = odo.scene(sweeps, skips, first if first is not None and np.asarray(first).shape == (4, 4) else None)
                rpe = None
                if gt_name:
                    gt = np.stack([np.asarray(stored.arrays(ds, i, [gt_name])[gt_name], np.float64) for i in items])
                    if gt.shape[1:] != (4, 4):
                        raise ValueError(f"{gt_key}: {sc} holds {gt.shape[1:]} arrays, not [4, 4] poses")
                    rpe = rpe_table(poses[:len(items)], gt)
                per_scene[sc] = scene_sums(regs, rpe)
                for k, i in enumerate(items):
                    ts = ds.index[i][1]
                    sink.put(sc, ts, out_key, np.ascontiguousarray(poses[k]))
                    if npz and k + 1 < len(poses):
                        sink.put(sc, ts, out_key + "_next", np.ascontiguousarray(poses[k + 1]))
            sink.close()                                            # (on success only: a failed run leaves its last scene as it was)

        distenv.run_shard(loop, "its share of the scenes", closing=(ds,))
        every = distenv.gathered(per_scene, lambda a, b: {**a, **b})
        total = new_sums()
        for sc in sorted(every):
            total = fold_sums(total, every[sc])
        numbers = {"scenes": {sc: numbers_of(every[sc], bool(gt_name)) for sc in sorted(every)}, "all": numbers_of(total, bool(gt_name))}
        head = (f"odometry (sweep odometry, v1; parity unpinned), voxel {prm.voxel:g} m, window {prm.window}, max_dist {prm.max_dist:g} m, init "
                f"{prm.init}, key '{out_key}'" + (f", against '{gt_key}'" if gt_key else "") + ":")
        lines = [head] + [_line(sc, numbers["scenes"][sc], bool(gt_name)) for sc in sorted(every)] + [_line("all", numbers["all"], bool(gt_name))]
        distenv.report(rank, "\n".join(lines), numbers, json_path)
    return numbers


def _parser():
    import argparse
    from .accumulate import MAX_WINDOW
    d = OdomParams()
    ap = argparse.ArgumentParser(description="estimate the pose of every sweep of every scene by scan-to-map ICP and store <timestamp>/<out_key> "
                                             "float64 [4, 4] (sweep odometry, v1; parity unpinned: the reference has no such stage; nothing has "
                                             "been tried on field data; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--out_key", default="pose_odom", help="the key the poses are stored under (never `pose`)")
    ap.add_argument("--window", type=int, default=d.window, help=f"past sweeps in the local map (1..{MAX_WINDOW})")
    ap.add_argument("--voxel", type=float, default=d.voxel, help="voxel edge [m] of the downsampling grid")
    ap.add_argument("--skip_label", default=None, metavar="KEY", help="leave out rows whose stored integer label KEY is non-zero (ray_label: "
                                                                      "python -m himo_amd.raymap)")
    ap.add_argument("--init", default=d.init, choices=INITS, help="model: constant velocity, the vote for the first sweep and after a failure; "
                                                                  "vote: the translation vote for every sweep")
    ap.add_argument("--gt_key", default=None, metavar="KEY", help="also print the relative pose error against the stored poses KEY (pose)")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the tables' numbers to PATH")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing <out_key> instead of refusing")
    ap.add_argument("--data_name", default="av2", choices=("av2", "scania"), help="whose ego box is cut out of every sweep")
    ap.add_argument("--max_dist", type=float, default=d.max_dist, help="inlier distance and search cell edge [m]")
    ap.add_argument("--iters", type=int, default=d.iters, help="iterations per sweep at most")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    return main(a.data_dir, a.out_key, a.window, a.voxel, a.skip_label, a.init, a.gt_key, a.json, a.overwrite, a.data_name, max_dist=a.max_dist,
                iters=a.iters)


if __name__ == "__main__":
    _cli()
