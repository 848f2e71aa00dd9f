"""The ICP-Flow baseline: clustering plus one rigid fit per cluster -- the non-learning, non-optimising flow producer
(``python -m himo_amd.save --model icpflow``, result key ``icpflow``: the name the reference gives this family at
tools/view_instance.py:155-156; the alternative its README discusses as "dynamic segmentation + ICP alignment", README.md:36-38).
It needs no checkpoint, no training and no per-pair optimisation: the number every other row of the table is read against.

PARITY UNPINNED.  The reference's ICP-Flow code sits in its absent ``OpenSceneFlow`` submodule; only the key name is in the tree.
Like the ground segmenter, this stage follows the build's own written rule, below, and is checked against a numpy restatement of
it (``tests/icpflow_ref.py``), never against the reference.  No claim is made about the reference's numbers.

The rule -- "cluster-rigid ICP, v1" (normative)
================================================
Inputs per sweep pair: ``pc0 (N0, >=3)`` and ``pc1 (N1, >=3)`` float32, ``gm0`` / ``gm1`` bool ground masks, ``pose0`` / ``pose1``
4x4.  Output: ``(N0, 3)`` float32 flow INCLUDING ego motion, row-aligned with ``pc0`` -- the contract of the network's and
FastNSF's payload under ``<timestamp>/<res_name>``.  Every float operation rounds on its own (``himo_amd/csrc/icpflow.hip`` is
built with ``-ffp-contract=off``); only sqrt and division appear, both correctly rounded; no transcendental is used.

Parameters (``IcpParams``; this build's own): ``bin`` 0.25 m, ``half`` 16 (the vote covers +-4 m: 40 m/s at 10 Hz, the
evaluator's top speed bucket), ``z_gate`` 1.0 m, ``max_dist`` 1.0 m, ``min_inliers`` 8, ``min_ratio`` 0.5, ``iters`` 10.
Admitted: every value finite and positive, ``half <= 64``.

0. Common frame.  ``a`` is ``pc0`` moved by ``inv(pose1) @ pose0`` in float32 -- the call and rounding of ``fastnsf.py`` /
   ``ssl_label._moved`` (``himo_rigid_transform``); ``b`` is the xyz of ``pc1``.  A point TAKES PART iff it is not ground and lies
   inside ``ssl_label.RANGE_NET`` (|x|, |y| <= 51.2).  The target set ``B`` is the participating rows of ``b``, compacted in row
   order (``ssl_label._compact``).
1. Clusters.  ``ssl_label.dbscan(a, EPS, MIN_PTS, skip=~participates)`` over ALL participating points of ``a`` (not only dynamic
   candidates: the rigid fit of a static cluster is its own sanity check).  Labels run 1..C; label 0 and the points that take no
   part get the identity transform.  ``IcpFlow(cluster="hdbscan", min_cluster_size=, min_samples=)`` takes the clusters from
   ``ssl_label.hdbscan`` ("HDBSCAN, v1"; its own host wait for the edge list) instead: nothing else of the rule changes.
2. Translation vote (integers: exact).  Every clustered point ``a_i`` and every target point ``q_j`` with ``|q_z - a_z| <= z_gate``
   (one float32 subtraction) give ``kx = rint((q_x - a_x) / bin)`` and ``ky = rint((q_y - a_y) / bin)`` in float32: a true
   division, round half to even.  The pair votes for bin ``(kx, ky)`` of its cluster iff ``|kx|, |ky| <= half``; a cluster has
   ``(2 half + 1)^2`` int32 counters.  The peak is the highest count; ties go to the smallest ``kx^2 + ky^2``, then the lowest
   ``(ky, kx)``; a cluster without votes takes ``(0, 0)``.  ``t_init = (kx bin, ky bin, 0)`` in float64 (``bin`` as float32).
   The device reaches only the target points near each cluster point, through the BEV cell grid of ``B``; its counts equal the
   all-pairs counts exactly.
3. ICP iterations (``iters``).  Each cluster has a float64 transform ``(c, s, t)``, yaw plus 3-D translation, starting at
   ``c = 1, s = 0, t = t_init``.  Each iteration:
   ``m_i = float32(R a_i + t)`` evaluated in float64 as ``((c x - s y) + tx, (s x + c y) + ty, z + tz)``;
   ``j(i)`` = the exact nearest neighbour of ``m_i`` in ``B`` (``himo_nn_grid``, one call over all clustered points; ties keep the
   lowest row); inlier iff ``d2_i <= max_dist^2`` (float32; ``max_dist^2`` one float32 product);
   per cluster over its inliers, in float64: the count ``n``, the centroids ``m_bar`` and ``q_bar`` (sum / n),
   ``A = sum (m-m_bar)_x (q-q_bar)_x + (m-m_bar)_y (q-q_bar)_y`` and ``B = sum (m-m_bar)_x (q-q_bar)_y - (m-m_bar)_y (q-q_bar)_x``;
   if ``n < min_inliers`` the cluster STOPS and is marked failed; otherwise ``h = sqrt(A^2 + B^2)``, ``dc = A / h`` and
   ``ds = B / h`` (``(1, 0)`` when ``h == 0``), ``dt = q_bar - dR m_bar`` (z: ``q_bar_z - m_bar_z``), and the transform becomes
   ``R <- dR R``, ``t <- dR t + dt``.  The ORDER of the float64 sums is not part of the rule: the device takes them in a fixed
   shape (the same bytes on every run), the restatement in row order; they agree to rounding.
4. Acceptance.  After the last iteration one more search; a cluster keeps its transform iff it has not failed and
   ``inliers / size >= min_ratio`` (float64 quotient against ``min_ratio`` as float32), else it gets the identity.  The status word
   of a cluster: accepted (0), failed (1) or rejected (2); the inlier count of its last pass; the vote peak ``kx, ky``.
5. Flow.  ``flow_i = float32(R a_i + t) - pc0_i``, subtracted in float32.  A row under the identity is ``a_i - pc0_i``: the
   ego-motion flow alone, bit for bit -- what ``raw`` means downstream.

Not part of v1: a histogram over z, a full 3-D rotation, a multi-frame variant.

Python sequences launches and owns no arithmetic on point data.  One host wait per pair: the cluster count, the size of ``B`` and
the clusters' row ranges, read through pinned memory behind an event (as ``ssl_label.auto_labels`` reads its counts).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

ACCEPTED, FAILED, REJECTED = 0, 1, 2
MODE_MOVED, MODE_FLOW = 0, 1


class _CParams(ctypes.Structure):
    """mirror of ``himo_icp_params`` (include/himo_amd.h)"""
    _fields_ = [("bin", ctypes.c_float), ("half", ctypes.c_int32), ("z_gate", ctypes.c_float), ("max_dist", ctypes.c_float),
                ("min_inliers", ctypes.c_int32), ("min_ratio", ctypes.c_float), ("iters", ctypes.c_int32)]


@dataclass(frozen=True)
class IcpParams:
    """the parameters of "cluster-rigid ICP, v1"; refuses what the rule does not admit before anything is launched"""
    bin: float = 0.25
    half: int = 16
    z_gate: float = 1.0
    max_dist: float = 1.0
    min_inliers: int = 8
    min_ratio: float = 0.5
    iters: int = 10

    def __post_init__(self):
        for name in ("bin", "z_gate", "max_dist", "min_ratio"):
            v = getattr(self, name)
            if not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
                raise ValueError(f"IcpParams.{name}={v!r}: a finite, positive number")
            with np.errstate(all="ignore"):
                as32 = float(np.float32(v))
            if not math.isfinite(as32) or not as32 > 0:
                raise ValueError(f"IcpParams.{name}={v!r}: not a positive float32")
        for name in ("half", "min_inliers", "iters"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"IcpParams.{name}={v!r}: a positive integer")
        if self.half > 64:
            raise ValueError(f"IcpParams.half={self.half}: at most 64")

    def c_struct(self) -> _CParams:
        return _CParams(self.bin, int(self.half), self.z_gate, self.max_dist, int(self.min_inliers), self.min_ratio, int(self.iters))


_tls = __import__("threading").local()


def pinned_words(n: int):
    """this thread's pinned int64 buffer of at least ``n`` words (one outstanding read-back per thread)"""
    import torch
    buf = getattr(_tls, "words", None)
    if buf is None or buf.numel() < n:
        buf = _tls.words = torch.zeros(1 << max(int(n) - 1, 1).bit_length(), dtype=torch.int64).pin_memory()
    return buf


class IcpFlow:
    """``IcpFlow(device, params).fit(pc0, pc1, gm0, gm1, pose0, pose1)`` -> the (N0, 3) float32 flow as a device tensor (module
    docstring).  After a fit ``last_status`` (int32 [C, 4]: state, inliers, kx, ky), ``last_transforms`` (float64 [C, 5]: c, s,
    tx, ty, tz) and ``last_labels`` (int32 [N0]) describe it (host copies, made when asked for).  There is no CPU path."""

    def __init__(self, device=None, params: IcpParams | None = None, eps: float | None = None, min_pts: int | None = None,
                 cluster: str = "dbscan", min_cluster_size: int | None = None, min_samples: int | None = None):
        """``eps`` / ``min_pts``: the clustering of rule 1 when not ``ssl_label.EPS`` / ``MIN_PTS`` (sparser sweeps).  ``cluster``:
        "dbscan" (the default) or "hdbscan" with ``min_cluster_size`` / ``min_samples`` (``ssl_label.HDB_MIN_CLUSTER`` /
        ``HDB_MIN_SAMPLES`` when None)"""
        from . import _lib
        from .seflow.ssl_label import CLUSTERINGS, EPS, HDB_MIN_CLUSTER, HDB_MIN_SAMPLES, MIN_PTS
        if cluster not in CLUSTERINGS:
            raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
        self.cluster = cluster
        self.min_cluster_size = int(HDB_MIN_CLUSTER if min_cluster_size is None else min_cluster_size)
        self.min_samples = int(HDB_MIN_SAMPLES if min_samples is None else min_samples)
        if self.min_cluster_size < 2 or not 1 <= self.min_samples <= 32:
            raise ValueError(f"min_cluster_size={min_cluster_size!r} (>= 2), min_samples={min_samples!r} (1..32)")
        self.eps, self.min_pts = float(EPS if eps is None else eps), int(MIN_PTS if min_pts is None else min_pts)
        if not (math.isfinite(self.eps) and self.eps > 0 and self.min_pts >= 1):
            raise ValueError(f"eps={eps!r}, min_pts={min_pts!r}: a finite positive radius and a positive count")
        self.params = params if params is not None else IcpParams()
        self.lib = _lib.load()
        self.device = device if device is not None else _lib.require_gpu()
        self._c = self.params.c_struct()
        self._last = None
        self.stage_events = None             # set to a list to have fit() append (stage, start event, end event) triples

    # ---- the raw calls (also what the tests drive) -------------------------------------------------------------------------------
    def _mark(self, stage, start):
        import torch
        if self.stage_events is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(self.device))
        if start is not None:
            self.stage_events.append((stage, start, ev))
        return ev

    def fit(self, pc0, pc1, gm0, gm1, pose0, pose1):
        import torch
        from . import _lib
        from .seflow.ssl_label import RANGE_NET, _compact, _moved, cluster_points
        from .ssl_loss import GRID_CELL, GRID_H, GRID_W, GRID_X0, GRID_Y0
        lib, dev, s, P = self.lib, self.device, _lib.stream_handle, _lib.ptr
        up = lambda x, dt: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dt)
        p0, p1 = up(pc0, torch.float32), up(pc1, torch.float32)
        g0, g1 = up(gm0, torch.bool), up(gm1, torch.bool)
        if p0.dim() != 2 or p0.shape[1] < 3 or p1.dim() != 2 or p1.shape[1] < 3:
            raise ValueError(f"sweeps are rows of x, y, z[, ...], not {tuple(p0.shape)} / {tuple(p1.shape)}")
        if g0.shape != (p0.shape[0],) or g1.shape != (p1.shape[0],):
            raise ValueError(f"ground masks {tuple(g0.shape)} / {tuple(g1.shape)} do not match the sweeps' {p0.shape[0]} / {p1.shape[0]} rows")
        n0, n1 = p0.shape[0], p1.shape[0]
        base = p0[:, :3].contiguous()
        flow = torch.empty((n0, 3), dtype=torch.float32, device=dev)
        empty_i = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        self._last = (empty_i(0, 4), torch.zeros((0, 5), dtype=torch.float64, device=dev), empty_i(n0))
        if n0 == 0:
            return flow
        T = np.linalg.inv(np.asarray(pose1, np.float64)) @ np.asarray(pose0, np.float64)
        t0 = self._mark("clusters", None)
        a = _moved(p0, T)                                           # rule 0
        b = p1[:, :3].contiguous()
        use_a = ~(g0 | (a[:, :2].abs().amax(dim=1) > RANGE_NET))
        labels, count = cluster_points(a, ~use_a, self.cluster, self.eps, self.min_pts, self.min_cluster_size, self.min_samples)   # rule 1
        if n1:
            use_b = ~(g1 | (b[:, :2].abs().amax(dim=1) > RANGE_NET))
            buf_b, _, cnt_b = _compact(b, use_b)
        else:
            buf_b, cnt_b = torch.zeros((1, 3), dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        # the clustered rows sorted by label (stable: ascending row inside a cluster) and every label's first sorted row
        big = torch.iinfo(torch.int32).max
        order = torch.argsort(torch.where(labels > 0, labels, big), stable=True)
        sizes = torch.bincount(labels, minlength=n0 + 1)[1:n0 + 1]
        offsets = torch.zeros(n0 + 1, dtype=torch.int64, device=dev)
        torch.cumsum(sizes, 0, out=offsets[1:])
        host = pinned_words(n0 + 3)
        host[:n0 + 3].copy_(torch.cat([count.to(torch.int64), cnt_b.to(torch.int64), offsets]), non_blocking=True)
        landed = torch.cuda.Event()
        landed.record(torch.cuda.current_stream(dev))
        landed.synchronize()                                        # the pair's one host wait
        C, nb = int(host[0]), int(host[1])
        h_off = host[2:2 + C + 1].numpy().copy()
        nc = int(h_off[C])
        t1 = self._mark("clusters", t0)
        status = torch.zeros((C, 4), dtype=torch.int32, device=dev)
        Tm = torch.zeros((C, 5), dtype=torch.float64, device=dev)
        if C > 0:
            B = buf_b[:nb]
            rows = order[:nc]
            a_s, lab_s = a.index_select(0, rows), labels.index_select(0, rows)
            W = 2 * int(self.params.half) + 1
            counts = torch.empty((C, W, W), dtype=torch.int32, device=dev)
            peak = torch.empty((C, 2), dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(lib.himo_icp_workspace_bytes(nb, C)), 16), dtype=torch.uint8, device=dev)
            nn_ws = torch.empty(int(lib.himo_nn_grid_workspace_bytes(max(nc, nb, 1), GRID_W, GRID_H)), dtype=torch.uint8, device=dev)
            m = torch.empty((nc, 3), dtype=torch.float32, device=dev)
            d2 = torch.empty(nc, dtype=torch.float32, device=dev)
            idx = torch.empty(nc, dtype=torch.int32, device=dev)
            cp, d_off = ctypes.addressof(self._c), offsets[:C + 1]
            _lib.check(lib.himo_icp_vote(nc, P(a_s), 3, C, h_off.ctypes.data, P(d_off), nb, P(B), cp, P(counts), P(peak), P(Tm), P(status),
                                         P(ws), ws.numel(), s()), "himo_icp_vote")                       # rule 2
            t2 = self._mark("vote", t1)
            for it in range(int(self.params.iters) + 1):            # rule 3, then rule 4's closing pass
                _lib.check(lib.himo_icp_apply(nc, P(a_s), 3, P(lab_s), C, P(Tm), P(status), MODE_MOVED, None, 0, P(m), s()), "himo_icp_apply")
                _lib.check(lib.himo_nn_grid(nc, P(m), nb, P(B), GRID_X0, GRID_Y0, GRID_CELL, GRID_W, GRID_H, P(d2), P(idx), P(nn_ws),
                                            nn_ws.numel(), s()), "himo_nn_grid")
                _lib.check(lib.himo_icp_step(nc, P(m), C, h_off.ctypes.data, P(d_off), nb, P(B), P(idx), P(d2), cp,
                                             int(it == int(self.params.iters)), P(Tm), P(status), None, P(ws), ws.numel(), s()), "himo_icp_step")
            t1 = self._mark("iterations", t2)
            self._counts, self._peak = counts, peak
        _lib.check(lib.himo_icp_apply(n0, P(a), 3, P(labels), C, P(Tm), P(status), MODE_FLOW, P(base), 3, P(flow), s()), "himo_icp_apply")   # rule 5
        self._mark("apply", t1)
        self._last = (status, Tm, labels)
        return flow

    @property
    def last_status(self) -> np.ndarray:
        return self._last[0].cpu().numpy()

    @property
    def last_transforms(self) -> np.ndarray:
        return self._last[1].cpu().numpy()

    @property
    def last_labels(self) -> np.ndarray:
        return self._last[2].cpu().numpy()
