"""Cluster-rigid flow refinement: the stage between a flow producer and the consumers (``python -m himo_amd.rigid_refine --data_dir D
--res_name seflowpp_best`` writes ``<timestamp>/seflowpp_best_rigid``).  A stored ``(N, 3)`` flow displaces every point of a vehicle
by its own noisy estimate; the quantities this project scores are per-instance shape errors.  This stage projects the estimate onto at
most ``models`` rigid motions per cluster and gives a static cluster exactly the ego-motion flow -- what ``raw`` means downstream.

PARITY UNPINNED.  The reference has no such stage.  Like ``icpflow``, ``ground_seg``, ``raymap`` and ``hdbscan`` it follows the build's
own written rule, below, and is checked against a numpy restatement of it (``tests/rigidrefine_ref.py``), never against the reference.
No claim is made about the reference's numbers.  Timing: 2.1 ms per 120k-point synthetic sweep, the refinement's own four launches
0.33 ms of it (profiles/rigid_refine.txt); nothing has been measured on field data.

The rule -- "cluster-rigid refinement, v1" (normative)
=======================================================
Inputs per sweep: ``pc0 (N, >=3)`` float32, ``flow (N, 3)`` float32 INCLUDING ego motion (the stored-result contract), ``gm0 (N,)``
bool, ``pose0`` / ``pose1`` 4x4.  Output: ``(N, 3)`` float32 flow including ego motion, row-aligned with ``pc0``.  Every float operation
rounds on its own (``himo_amd/csrc/rigidrefine.hip`` is built with ``-ffp-contract=off``); only sqrt and division appear, both correctly
rounded; no transcendental is used.

Parameters (``RigidParams``; this build's own): ``bin`` 0.25 m (vote bin width), ``half`` 16 (the vote covers +-4 m per sweep, as
``IcpParams``), ``tol`` 0.25 m (inlier radius), ``iters`` 5 (refit passes), ``min_inliers`` 8, ``min_ratio`` 0.25 (of the cluster's
points, per model), ``static_disp`` 0.05 m (static snap threshold), ``models`` 2 (models per cluster).  Admitted: every value finite and
positive, ``half <= 64``, ``1 <= models <= 4``.  Anything else is refused before a launch.

0. Common frame.  ``a`` is ``pc0`` moved by ``inv(pose1) @ pose0`` in float32 (``himo_rigid_transform``, i.e. ``ssl_label._moved``: the
   call and rounding of icpflow rule 0).  ``q_i = pc0_i + flow_i``, one float32 addition per coordinate: where the estimate puts the
   point in ``pc1``'s frame.  A point TAKES PART iff it is not ground, ``|a_x|, |a_y| <= ssl_label.RANGE_NET`` and its three flow values
   are finite.
1. Clusters.  ``ssl_label.cluster_points(a, ~participates, cluster, EPS, MIN_PTS, ...)``, exactly as icpflow rule 1: DBSCAN by default,
   ``"hdbscan"`` on request; ``eps`` / ``min_pts`` are the constructor's.  Labels run 1..C; ``size_k`` = the number of rows with label k.
2. Rounds.  Each cluster runs rounds ``j = 1..models`` over its UNCLAIMED rows (initially all of them).
   2a. Vote (integers: exact).  ``r_i = q_i - a_i`` in float32; ``kx = rint(r_x / bin)``, ``ky = rint(r_y / bin)`` in float32: a true
       division, round half to even.  The row votes for ``(kx, ky)`` iff ``|kx|, |ky| <= half``.  The peak is the highest count; ties go
       to the smallest ``kx^2 + ky^2``, then the lowest ``(ky, kx)``; no votes gives ``(0, 0)``.  Start: ``c = 1, s = 0``,
       ``t = (kx bin, ky bin, 0)`` in float64 (``bin`` as float32).
   2b. Passes ``p = 0..iters``.  The model in float64 from the float32 ``a``: ``m_i = ((c x - s y) + tx, (s x + c y) + ty, z + tz)``;
       ``e2_i = ((q_x - m_x)^2 + (q_y - m_y)^2) + (q_z - m_z)^2`` in float64 -- pass 0 omits the z term (the start has no z).  A row is an
       inlier iff ``e2_i <= tol^2`` (``tol^2`` the float64 product of ``tol`` as float32).  For ``p < iters``: if the inlier count
       ``n < min_inliers`` the round FAILS; otherwise the model is refitted over the inliers in float64 from the original ``a`` (not
       incrementally): centroids ``a_bar``, ``q_bar`` (sum / n); ``A = sum (a-a_bar)_x (q-q_bar)_x + (a-a_bar)_y (q-q_bar)_y``;
       ``B = sum (a-a_bar)_x (q-q_bar)_y - (a-a_bar)_y (q-q_bar)_x``; ``h = sqrt(A^2 + B^2)``; ``c = A / h``, ``s = B / h`` (``(1, 0)`` when
       ``h == 0``); ``t = q_bar - R a_bar`` (z: ``q_bar_z - a_bar_z``).  The ORDER of the float64 sums is not part of the rule: the device
       takes them in a fixed shape (the same bytes on every run), the restatement in row order; they agree to rounding.  Pass ``iters``
       only tests: its inliers are the round's CLAIM.
   2c. Acceptance.  A round is accepted iff it has not failed, ``n >= min_inliers`` and ``n / size_k >= min_ratio`` (float64 quotient
       against ``min_ratio`` as float32); else it is REJECTED.  A failed or rejected round claims nothing and ends the cluster.
   2d. Static snap.  An accepted round with ``max over its claim of |m_i - a_i|^2 < static_disp^2`` (float64, ``((.)^2 + (.)^2) + (.)^2``)
       becomes STATIC: its transform is replaced by the identity.
   2e. Write.  Claimed rows get ``flow'_i = float32(R a_i + t) - pc0_i``, subtracted in float32; under the identity that is
       ``a_i - pc0_i``, the ego-motion flow bit for bit.  The claim leaves the cluster's unclaimed rows and the next round starts.
3. Every other row -- ground, out of range, a non-finite flow, label 0, unclaimed -- keeps the BYTES of its input flow.  Non-finite
   inputs never enter a sum.

Status per cluster and round: the state (accepted 0, failed 1, rejected 2, static 3, not run 4), the inlier count of the round's last
pass (the claim count of a round that claimed), ``kx``, ``ky``, and the float64 ``(c, s, tx, ty, tz)`` (the identity for a static round
and for one that was not run; the last model for a failed or rejected one).

Not part of v1: a z vote, 3-D rotation, soft weights, more than one sweep pair, a constant-twist (arc) compensation (the chord error at
0.05 rad per sweep is millimetres).  Not built: an in-line ``--rigid`` switch in ``save`` (it would put a host wait into the overlapped
batch loop), batching several sweeps per launch.

Python sequences launches and owns no arithmetic on point data.  One host wait per sweep: the cluster count and the clusters' row
ranges, read through pinned memory behind an event (as ``IcpFlow.fit`` reads them).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

ACCEPTED, FAILED, REJECTED, STATIC, NOT_RUN = 0, 1, 2, 3, 4
STATE_NAMES = ("accepted", "failed", "rejected", "static", "not run")
MAX_MODELS = 4


class _CParams(ctypes.Structure):
    """mirror of ``himo_rigid_params`` (include/himo_amd.h)"""
    _fields_ = [("bin", ctypes.c_float), ("half", ctypes.c_int32), ("tol", ctypes.c_float), ("iters", ctypes.c_int32),
                ("min_inliers", ctypes.c_int32), ("min_ratio", ctypes.c_float), ("static_disp", ctypes.c_float), ("models", ctypes.c_int32)]


@dataclass(frozen=True)
class RigidParams:
    """the parameters of "cluster-rigid refinement, v1"; refuses what the rule does not admit before anything is launched"""
    bin: float = 0.25
    half: int = 16
    tol: float = 0.25
    iters: int = 5
    min_inliers: int = 8
    min_ratio: float = 0.25
    static_disp: float = 0.05
    models: int = 2

    def __post_init__(self):
        for name in ("bin", "tol", "min_ratio", "static_disp"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
                raise ValueError(f"RigidParams.{name}={v!r}: a finite, positive number")
            with np.errstate(all="ignore"):
                as32 = float(np.float32(v))
            if not math.isfinite(as32) or not as32 > 0:
                raise ValueError(f"RigidParams.{name}={v!r}: not a positive float32")
        for name in ("half", "iters", "min_inliers", "models"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"RigidParams.{name}={v!r}: a positive integer")
        if self.half > 64:
            raise ValueError(f"RigidParams.half={self.half}: at most 64")
        if self.models > MAX_MODELS:
            raise ValueError(f"RigidParams.models={self.models}: at most {MAX_MODELS}")

    def c_struct(self) -> _CParams:
        return _CParams(self.bin, int(self.half), self.tol, int(self.iters), int(self.min_inliers), self.min_ratio, self.static_disp,
                        int(self.models))


class RigidRefine:
    """``RigidRefine(device, params).refine(pc0, flow, gm0, pose0, pose1)`` -> the refined (N, 3) float32 flow as a device tensor
    (module docstring).  After a call ``last_status`` (int32 [C, models, 4]: state, inliers, kx, ky), ``last_transforms`` (float64
    [C, models, 5]: c, s, tx, ty, tz), ``last_labels`` (int32 [N]) and ``last_claim`` (int8 [N]: 0 untouched, j = claimed by round j)
    describe it (host copies, made when asked for).  There is no CPU path."""

    def __init__(self, device=None, params: RigidParams | None = None, cluster: str = "dbscan", eps: float | None = None,
                 min_pts: int | None = None, min_cluster_size: int | None = None, min_samples: int | None = None):
        """``cluster``: "dbscan" (the default; ``eps`` / ``min_pts`` when not ``ssl_label.EPS`` / ``MIN_PTS``) or "hdbscan" with
        ``min_cluster_size`` / ``min_samples`` (``ssl_label.HDB_MIN_CLUSTER`` / ``HDB_MIN_SAMPLES`` when None)"""
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
        self.params = params if params is not None else RigidParams()
        self.lib = _lib.load()
        if self.lib.himo_abi_sizeof(b"himo_rigid_params") != ctypes.sizeof(_CParams):
            raise ImportError("himo_rigid_params: the library's layout is not this binding's; rebuild libhimo_amd.so")
        self.device = device if device is not None else _lib.require_gpu()
        self._c = self.params.c_struct()
        self._last = None
        self.last_clusters = 0                  # known on the host after the sweep's one wait

    def refine(self, pc0, flow, gm0, pose0, pose1):
        import torch
        from . import _lib
        from .icpflow import pinned_words
        from .seflow.ssl_label import RANGE_NET, _moved, cluster_points
        lib, dev, s, P = self.lib, self.device, _lib.stream_handle, _lib.ptr
        up = lambda x, dt: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dt)
        p0, fl, g0 = up(pc0, torch.float32), up(flow, torch.float32).contiguous(), up(gm0, torch.bool)
        if p0.dim() != 2 or p0.shape[1] < 3:
            raise ValueError(f"a sweep is rows of x, y, z[, ...], not {tuple(p0.shape)}")
        n0 = p0.shape[0]
        if fl.shape != (n0, 3) or g0.shape != (n0,):
            raise ValueError(f"flow {tuple(fl.shape)} / ground mask {tuple(g0.shape)} are not row-aligned with the sweep's {n0} rows")
        base = p0.contiguous() if p0.shape[1] == 4 else p0[:, :3].contiguous()
        M = int(self.params.models)
        out = torch.empty((n0, 3), dtype=torch.float32, device=dev)
        claim = torch.zeros(n0, dtype=torch.int8, device=dev)
        empty_i = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        self._last = (empty_i(0, M, 4), torch.zeros((0, M, 5), dtype=torch.float64, device=dev), empty_i(n0), claim)
        self.last_clusters = 0
        if n0 == 0:
            return out
        T = np.linalg.inv(np.asarray(pose1, np.float64)) @ np.asarray(pose0, np.float64)
        a = _moved(p0, T)                                           # rule 0
        use = ~(g0 | (a[:, :2].abs().amax(dim=1) > RANGE_NET)) & torch.isfinite(fl).all(dim=1)
        labels, count = cluster_points(a, ~use, self.cluster, self.eps, self.min_pts, self.min_cluster_size, self.min_samples)    # rule 1
        # the clustered rows sorted by label (stable: ascending row inside a cluster) and every label's first sorted row
        big = torch.iinfo(torch.int32).max
        order = torch.argsort(torch.where(labels > 0, labels, big), stable=True)
        sizes = torch.bincount(labels, minlength=n0 + 1)[1:n0 + 1]
        offsets = torch.zeros(n0 + 1, dtype=torch.int64, device=dev)
        torch.cumsum(sizes, 0, out=offsets[1:])
        host = pinned_words(n0 + 2)
        host[:n0 + 2].copy_(torch.cat([count.to(torch.int64), offsets]), non_blocking=True)
        landed = torch.cuda.Event()
        landed.record(torch.cuda.current_stream(dev))
        landed.synchronize()                                        # the sweep's one host wait
        C = int(host[0])
        h_off = host[1:1 + C + 1].numpy().copy()
        nc = int(h_off[C])
        status = torch.zeros((C, M, 4), dtype=torch.int32, device=dev)
        Tm = torch.zeros((C, M, 5), dtype=torch.float64, device=dev)
        rows = order[:nc]
        ws = torch.empty(max(int(lib.himo_rigid_refine_workspace_bytes(nc, C, int(self.params.half), M)), 16), dtype=torch.uint8, device=dev)
        _lib.check(lib.himo_rigid_refine(n0, P(base), int(base.shape[1]), P(fl), P(a), P(labels), nc, P(rows), C, h_off.ctypes.data,
                                         P(offsets), ctypes.addressof(self._c), P(status), P(Tm), P(claim), P(out), P(ws), ws.numel(), s()),
                   "himo_rigid_refine")                             # rules 2 and 3
        self._last = (status, Tm, labels, claim)
        self.last_clusters = C
        return out

    @property
    def last_status(self) -> np.ndarray:
        return self._last[0].cpu().numpy()

    @property
    def last_transforms(self) -> np.ndarray:
        return self._last[1].cpu().numpy()

    @property
    def last_labels(self) -> np.ndarray:
        return self._last[2].cpu().numpy()

    @property
    def last_claim(self) -> np.ndarray:
        return self._last[3].cpu().numpy()


# ---- the program ------------------------------------------------------------------------------------------------------------------------
def main(data_dir: str, res_name: str, out_name: str = "", cluster: str = "dbscan", min_cluster_size=None, min_samples=None,
         params: RigidParams | None = None, overwrite: bool = False) -> dict:
    """The program: for every sweep of ``data_dir`` that has ``res_name`` stored and a successor pose, ``<timestamp>/<out_name>``
    (default ``<res_name>_rigid``) = the refined flow, written through ``save``'s sinks; under ``torchrun`` whole scenes per rank (h5).
    Returns this rank's {"sweeps", "skipped", "clusters", "rounds": {state name: count}}."""
    from . import distenv, stored
    from .dataset import NpzDataset, open_dataset
    from .save import H5ResultSink, NpzResultSink
    from .sweeps import sharded_items
    if not res_name or res_name == "raw":
        raise ValueError(f"res_name={res_name!r}: 'raw' is the zero-motion key, not a stored flow; name the result to refine")
    out_name = out_name or f"{res_name}_rigid"
    if out_name == res_name:
        raise ValueError(f"out_name={out_name!r} is res_name: the refined flow goes under a key of its own")
    if out_name == "raw":
        raise ValueError("out_name='raw': that key means zero motion downstream")
    if cluster not in ("dbscan", "hdbscan"):
        raise ValueError(f"cluster={cluster!r}: 'dbscan' (the default) or 'hdbscan'")
    params = params if params is not None else RigidParams()
    root = Path(data_dir)
    totals = {"sweeps": 0, "skipped": 0, "clusters": 0, "rounds": {name: 0 for name in STATE_NAMES}}
    with distenv.process_group() as (rank, world):
        ds = open_dataset(root, vis_name=[res_name, out_name], eval=False, fields=("pc0", "pose0", "pose1", "gm0", res_name), zero_copy=True)
        npz = isinstance(ds, NpzDataset)
        mine = sharded_items(ds, whole_scenes=not npz)              # whole scenes per rank: every scene file has one writer
        drain = sink = None

        def loop():
            nonlocal drain, sink
            # the refusals, before anything touches the GPU or a file is written
            todo = []
            for i in mine:
                have = stored.present(ds, i, (res_name, out_name, "gm0"))
                if res_name not in have:
                    totals["skipped"] += 1
                    continue
                if out_name in have and not overwrite:
                    raise FileExistsError(f"{'/'.join(map(str, ds.index[i]))} already holds '{out_name}': pass --overwrite to replace it")
                if "gm0" not in have:
                    raise KeyError("gm0: the refinement needs the sweep's ground mask (`python -m himo_amd.ground_seg` writes it)")
                todo.append(i)
            if not todo:
                return
            import torch
            from .feeder import ResultDrain
            engine = RigidRefine(params=params, cluster=cluster, min_cluster_size=min_cluster_size, min_samples=min_samples)
            sink = NpzResultSink(root, out_name) if npz else H5ResultSink(root, out_name, before_write=ds.forget)
            drain = ResultDrain(lambda key, flow: sink(key[0], key[1], flow), device=engine.device)
            states = torch.zeros(len(STATE_NAMES), dtype=torch.int64, device=engine.device)
            for i in todo:
                f = ds[i]
                flow = engine.refine(np.asarray(f["pc0"]), np.asarray(f[res_name]), np.asarray(f["gm0"]), f["pose0"], f["pose1"])
                drain.put((i, f), flow)
                states += torch.bincount(engine._last[0][:, :, 0].reshape(-1).to(torch.int64), minlength=len(STATE_NAMES))
                totals["sweeps"] += 1
                totals["clusters"] += engine.last_clusters
            totals["rounds"] = dict(zip(STATE_NAMES, (int(v) for v in states.cpu())))

        distenv.run_shard(loop, "its share of the refined flows", closing=lambda: (drain, sink))
        who = f"rank {rank}: " if world > 1 else ""
        print(f"{who}rigid_refine '{res_name}' -> '{out_name}': {totals['sweeps']} sweeps ({totals['skipped']} without '{res_name}'), "
              f"{totals['clusters']} clusters, rounds " + ", ".join(f"{k} {v}" for k, v in totals["rounds"].items()))
    return totals


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="project a stored flow onto rigid motions per cluster (cluster-rigid refinement, v1; parity "
                                             "unpinned; MI355X path) and store it as <res_name>_rigid")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files (or this package's npz container)")
    ap.add_argument("--res_name", required=True, help="the stored flow to refine ('raw' is refused: it is not a stored flow)")
    ap.add_argument("--out_name", default="", help="the key to write (default <res_name>_rigid)")
    ap.add_argument("--cluster", default="dbscan", help="'dbscan' (the default) or 'hdbscan' (HDBSCAN, v1)")
    ap.add_argument("--min_cluster_size", type=int, default=None, help="--cluster hdbscan: the smallest cluster (ssl_label.HDB_MIN_CLUSTER)")
    ap.add_argument("--min_samples", type=int, default=None, help="--cluster hdbscan: the core neighbour count, 1..32 (ssl_label.HDB_MIN_SAMPLES)")
    d = RigidParams()
    ap.add_argument("--tol", type=float, default=d.tol, help="inlier radius, metres")
    ap.add_argument("--min_ratio", type=float, default=d.min_ratio, help="share of a cluster's points a model must claim")
    ap.add_argument("--static_disp", type=float, default=d.static_disp, help="a model that moves no claimed point this far is static, metres")
    ap.add_argument("--models", type=int, default=d.models, help=f"models per cluster, 1..{MAX_MODELS}")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing <out_name> instead of refusing")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    main(a.data_dir, a.res_name, a.out_name, a.cluster, a.min_cluster_size, a.min_samples,
         RigidParams(tol=a.tol, min_ratio=a.min_ratio, static_disp=a.static_disp, models=a.models), a.overwrite)


if __name__ == "__main__":
    _cli()
