"""Self-supervised cluster labels on the GPU -- this build's counterpart of ``+ssl_label=seflow_auto``
(assets/slurm/ssl-train-av2.sh:32, ssl-train-scania.sh:32): the per-point ``0 = static / > 0 = dynamic cluster id`` labels the
training loss consumes (``ssl_loss.SeFlowLoss``), generated from the sweeps themselves instead of read from ground truth.

PARITY UNPINNED.  The reference's generator (DUFOMap dynamic awareness + HDBSCAN clustering, per the SeFlow papers) lives in the
absent OpenSceneFlow submodule together with its dependencies; only the option's name is in the tree.  This build's own
specification, chosen so that every step is exact and order-independent:

  0. only points inside the network's BEV range (+-51.2 m in the common frame, ``RANGE_NET``) take part: the network gives the
     others no flow and the loss no gradient (``mask_rows``), so labelling them would only dilute the loss's per-cluster and
     per-point normalisations -- and a 200 m sweep would pile its far half into the border cells of the search grids.
  1. dynamic candidates of a sweep A against its neighbour sweep B (both in ONE frame: A is moved with ``inv(poseB) @ poseA``):
     non-ground points of A whose nearest non-ground point of B is further than ``dyn_dist`` x max(1, r / 30 m), r = the
     point's BEV range (0.35 m near the sensor: a point on a static surface has a return of the other sweep next to it once
     ego motion is removed, a point on an object faster than 3.5 m/s does not; beyond ~30 m the SAMPLING spacing of a spinning
     LiDAR exceeds 0.35 m, so the bar grows with range instead of declaring most far static returns candidates).
     Exact nearest neighbours through the BEV cell grid (csrc/nngrid.hip).
  2. clusters: DBSCAN(``eps``, ``min_pts``) over the candidates (csrc/dbscan.hip: labels are a pure function of the input --
     clusters numbered by their lowest CORE point index, a border point joins the neighbouring cluster of lowest such index).
     ``cluster="hdbscan"`` takes them from ``hdbscan`` ("HDBSCAN, v1", csrc/hdbscan.hip; its rule is in that function's docstring)
     instead, for objects too sparse at range for one radius; the default is DBSCAN.
  3. everything else -- ground, static, noise -- is label 0.

The oracle is sklearn.cluster.DBSCAN + scipy's cKDTree (oracle/dbscan_oracle.py); tests/test_ssl_label_gpu.py.
"""
from __future__ import annotations

import ctypes
import math
import time

import numpy as np
import torch

from .. import _lib
from ..ssl_loss import nn_grid

_lib.register({
    "himo_dbscan_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "himo_dbscan": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_float,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.c_void_p]),
    "himo_hdbscan_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "himo_hdbscan_mst": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "himo_hdbscan_tree": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "himo_rigid_transform": (ctypes.c_int, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_int, ctypes.c_void_p]),
})

EPS, MIN_PTS, DYN_DIST = 0.5, 8, 0.35
RANGE_XY = 52.0                     # the BEV cell grid covers +- this (points beyond it are binned into its border cells)
RANGE_NET = 51.2                    # the network's BEV range (assets/slurm/ssl-train-av2.sh:32 point_cloud_range): step 0
DYN_REF_RANGE = 30.0                # BEV range from which the dynamic-candidate bar grows linearly (step 1)
# HDBSCAN's defaults (``hdbscan``): a RECOLLECTION of the published label generator's settings, not a surveyed fact -- its code is in the
# absent OpenSceneFlow submodule
HDB_MIN_CLUSTER, HDB_MIN_SAMPLES = 20, 20
CLUSTERINGS = ("dbscan", "hdbscan")


def dbscan(points: torch.Tensor, eps: float = EPS, min_pts: int = MIN_PTS, skip: torch.Tensor | None = None):
    """(labels int32 (n,), number of clusters) of DBSCAN over the xyz of ``points`` (device (n, >= 3) float32).  ``skip``: bool /
    uint8 (n,), True = the point takes no part (label 0)."""
    lib, dev = _lib.load(), _lib.require_gpu()
    p = points.to(device=dev, dtype=torch.float32)
    if p.stride(-1) != 1 or p.stride(0) < 3:
        p = p.contiguous()
    n = p.shape[0]
    gw = gh = int(math.ceil(2 * RANGE_XY / eps))
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.himo_dbscan_workspace_bytes(n, gw, gh)), dtype=torch.uint8, device=dev)
    sk = None if skip is None else skip.to(device=dev, dtype=torch.uint8).contiguous()
    _lib.check(lib.himo_dbscan(n, _lib.ptr(p), int(p.stride(0)) if n else 3, _lib.ptr(sk), float(eps), int(min_pts), -RANGE_XY, -RANGE_XY, float(eps),
                               gw, gh, _lib.ptr(labels), _lib.ptr(count), _lib.ptr(ws), ws.numel(), _lib.stream_handle()), "himo_dbscan")
    return labels, count


_tls = __import__("threading").local()


def _pinned_tree(n_words: int):
    """this thread's pinned int32 buffer of at least ``n_words`` words for the tree phase of ``hdbscan``"""
    buf = getattr(_tls, "tree", None)
    if buf is None or buf.numel() < n_words:
        buf = _tls.tree = torch.zeros(1 << max(int(n_words) - 1, 1).bit_length(), dtype=torch.int32).pin_memory()
    return buf


def hdbscan(points: torch.Tensor, min_cluster_size: int = HDB_MIN_CLUSTER, min_samples: int = HDB_MIN_SAMPLES,
            skip: torch.Tensor | None = None, return_tree: bool = False):
    """(labels int32 (n,), number of clusters as a 1-element int32 device tensor) of HDBSCAN over the xyz of ``points`` (device
    (n, >= 3) float32) -- the shape of result ``dbscan`` gives.  ``skip``: bool / uint8 (n,), True = the point takes no part (label 0).
    ``return_tree``: also a dict {"core2": float32 (n,) device tensor, "edges": uint32-valued int64 host array (|P| - 1, 3) of
    (bits of w, lo, hi), "index": the original indices of P, "rounds": the Boruvka rounds taken, "tree_ms": the host phase's time}.

    PARITY UNPINNED, like this module's other steps: the rule below is this build's own.  The device phase is csrc/hdbscan.hip
    (``himo_hdbscan_mst``: compaction, exact core distances, the minimum spanning tree by Boruvka rounds over a tiled all-pairs
    kernel: QUADRATIC in the participating points per round), the host phase ``himo_hdbscan_tree`` inside the library.  ONE host wait:
    the edge list comes back through pinned memory behind an event on the current stream, and the labels go up again.

    The rule -- "HDBSCAN, v1" (normative)
    ======================================
    Inputs: ``xyz [n][pitch >= 3]`` float32, optional ``skip [n]``, ``min_cluster_size m >= 2``, ``min_samples k``, ``1 <= k <= 32``.
    A point whose skip flag is set, or that holds a NaN, takes no part and gets label 0.  P = the participating points.  If
    ``|P| < max(k, 2)``, every label is 0.

    1. Squared distance.  ``d2(i,j) = (dx*dx + dy*dy) + dz*dz`` in float32, every operation rounding on its own, ``dx = x_i - x_j``.
       All comparisons are on squared values; no square root is taken on the device.
    2. Core.  ``core2(i)`` = the k-th smallest of ``{d2(i,j) : j in P}``.  The point itself counts, so k = 1 gives 0 (sklearn's
       convention).
    3. Mutual reachability.  ``w(i,j) = max(core2(i), core2(j), d2(i,j))``.
    4. Edge order.  Edges are totally ordered by ``(w, lo, hi)``, ``lo < hi`` the original point indices.  Ties in ``w`` are the
       normal case -- every neighbour inside a point's core radius ties -- so the order is part of the rule.
    5. Tree.  The MST is the unique minimum spanning tree of the complete graph on P under that strict order.
    6. Dendrogram.  The MST edges in ascending order, merged: the component holding ``lo`` is the LEFT child, the one holding ``hi``
       the RIGHT child; the node's distance is ``sqrt((double)w)``.
    7. Condensed tree.  Walk from the root with an explicit stack, right pushed before left; ``lambda = 1 / max(distance, 1e-9)``.
       Both children ``>= m``: two new clusters are born at ``lambda``, left numbered before right.  Both ``< m``: all their points
       fall out of the current cluster at ``lambda``.  Otherwise the small side's points fall out and the big side continues under
       the same cluster id.
    8. Stability.  Float64: ``S(c) = sum over c's rows of (lambda_row - lambda_birth(c)) * size_row``, in the order the walk emitted
       the rows.
    9. Selection (excess of mass).  Clusters from the highest id down; the root is never selected.  A leaf is selected.  An inner
       cluster whose children's ``S`` sum is ``>`` its own takes that sum and stays unselected; otherwise it is selected and all its
       descendants are deselected (``allow_single_cluster=False``, no selection epsilon).
    10. Labels.  A point gets the nearest selected ancestor of the cluster it fell out of, or 0; clusters are numbered 1..K by their
        lowest point index.

    tests/hdbscan_ref.py restates it in numpy; tests/test_hdbscan_cpu.py holds it against sklearn.cluster.HDBSCAN (identical for
    k = 1, where no weight ties; sklearn orders tied merges by its Prim walk otherwise)."""
    lib, dev = _lib.load(), _lib.require_gpu()
    m, k = int(min_cluster_size), int(min_samples)
    if m < 2 or not 1 <= k <= 32:
        raise ValueError(f"hdbscan: min_cluster_size={min_cluster_size!r} (>= 2), min_samples={min_samples!r} (1..32)")
    p = points.to(device=dev, dtype=torch.float32)
    if p.stride(-1) != 1 or p.stride(0) < 3:
        p = p.contiguous()
    n = p.shape[0]
    gw = gh = int(math.ceil(2 * RANGE_XY / EPS))
    # one device block, so that one copy brings it back: counts [4], index [n], edges [max(n - 1, 0)][3]
    n_words = 4 + n + 3 * max(n - 1, 0)
    out = torch.empty(n_words, dtype=torch.int32, device=dev)
    core2 = torch.empty(n, dtype=torch.float32, device=dev) if return_tree else None
    ws = torch.empty(int(lib.himo_hdbscan_workspace_bytes(n, gw, gh)), dtype=torch.uint8, device=dev)
    sk = None if skip is None else skip.to(device=dev, dtype=torch.uint8).contiguous()
    at = lambda words: out.data_ptr() + 4 * words
    _lib.check(lib.himo_hdbscan_mst(n, _lib.ptr(p), int(p.stride(0)) if n else 3, _lib.ptr(sk), k, at(0), at(4), _lib.ptr(core2), at(4 + n),
                                    _lib.ptr(ws), ws.numel(), _lib.stream_handle()), "himo_hdbscan_mst")
    host = _pinned_tree(n_words + n + 1)
    host[:n_words].copy_(out, non_blocking=True)
    landed = torch.cuda.Event()
    landed.record(torch.cuda.current_stream(dev))
    landed.synchronize()                                        # the one host wait
    h = host.numpy()
    n_part, n_edges, rounds = int(h[0]), int(h[1]), int(h[2])
    labels_h = host[n_words:n_words + n]
    k_out = ctypes.c_int32(0)
    t0 = time.perf_counter()
    _lib.check(lib.himo_hdbscan_tree(n, n_part, host.data_ptr() + 16, n_edges, host.data_ptr() + 4 * (4 + n), m, k, labels_h.data_ptr(),
                                     ctypes.addressof(k_out)), "himo_hdbscan_tree")
    tree_ms = (time.perf_counter() - t0) * 1e3
    host[n_words + n] = k_out.value
    up = host[n_words:n_words + n + 1].to(dev, non_blocking=True)
    labels, count = up[:n], up[n:]
    if not return_tree:
        return labels, count
    edges = h[4 + n:4 + n + 3 * n_edges].view(np.uint32).astype(np.int64).reshape(-1, 3)
    return labels, count, {"core2": core2, "edges": edges, "index": h[4:4 + n_part].astype(np.int64), "rounds": rounds, "tree_ms": tree_ms}


def cluster_points(points: torch.Tensor, skip: torch.Tensor | None = None, cluster: str = "dbscan", eps: float = EPS, min_pts: int = MIN_PTS,
            min_cluster_size: int = HDB_MIN_CLUSTER, min_samples: int = HDB_MIN_SAMPLES):
    """``dbscan(points, eps, min_pts, skip)`` or ``hdbscan(points, min_cluster_size, min_samples, skip)`` by name: the one switch the
    label generators and the ICP-Flow baseline share.  An unknown name is refused."""
    if cluster == "dbscan":
        return dbscan(points, eps, min_pts, skip)
    if cluster == "hdbscan":
        return hdbscan(points, min_cluster_size, min_samples, skip)
    raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")


def _moved(pc: torch.Tensor, T: np.ndarray) -> torch.Tensor:
    lib, dev = _lib.load(), _lib.require_gpu()
    src = pc[:, :3].contiguous()
    out = torch.empty((src.shape[0], 3), dtype=torch.float32, device=dev)
    T32 = torch.from_numpy(np.ascontiguousarray(T, dtype=np.float32)).to(dev)
    _lib.check(lib.himo_rigid_transform(src.shape[0], _lib.ptr(src), 3, _lib.ptr(T32), _lib.ptr(out), 3, _lib.stream_handle()), "rigid")
    return out


def _pinned_counts():
    """this thread's pinned word pair for the sizes of the two compacted sweeps (one outstanding read-back per thread)"""
    buf = getattr(_tls, "counts", None)
    if buf is None:
        buf = _tls.counts = torch.zeros(2, dtype=torch.int32).pin_memory()
    return buf


def _compact(pts: torch.Tensor, use: torch.Tensor):
    """rows of ``pts`` with ``use`` set, in order, WITHOUT asking the host for their number: every row is copied to its rank among
    the kept rows, the others to a dump row at the end.  -> (buffer (n + 1, 3), destination row of every input row (n,) int64, the
    number of kept rows as a 1-element int32 device tensor)"""
    n = pts.shape[0]
    pos = torch.cumsum(use.to(torch.int32), 0, dtype=torch.int32)
    dest = torch.where(use, pos - 1, n).to(torch.int64)
    buf = torch.empty((n + 1, 3), dtype=torch.float32, device=pts.device)
    buf.index_copy_(0, dest, pts)                               # (the dump row takes whichever excluded row lands last: never read)
    return buf, dest, pos[-1:]


def auto_labels(pc0, pc1, ground0, ground1, pose0, pose1, eps: float = EPS, min_pts: int = MIN_PTS, dyn_dist: float = DYN_DIST,
                return_top: bool = False, cluster: str = "dbscan", min_cluster_size: int = HDB_MIN_CLUSTER,
                min_samples: int = HDB_MIN_SAMPLES):
    """(label0 (n0,), label1 (n1,)) int32 device tensors for the sweep pair (module docstring).  ``pc*``: (n, >= 3) float32 in their
    own sensor frames, ``ground*``: bool masks, ``pose*``: 4x4 world poses.  ``return_top``: also the highest label of the pair as a
    1-element int32 device tensor (= the larger of the two cluster counts the clustering kernels leave: no reduction over the labels).

    ONE host wait per pair -- the sizes of the two in-range non-ground subsets, which the nearest-neighbour search takes as host
    integers; they come back through pinned memory behind an event on the current stream (``cluster="hdbscan"`` -- step 2 by
    ``hdbscan(min_cluster_size, min_samples)`` instead of DBSCAN -- adds one wait per sweep for its edge list).  Everything else is enqueued without
    asking the device anything (no boolean-mask indexing: that copies a count back per use -- five waits per pair before round 6,
    each as long as the queue in front of it when a training step shares the device)."""
    dev = _lib.require_gpu()
    if cluster not in CLUSTERINGS:
        raise ValueError(f"cluster={cluster!r}: one of {', '.join(CLUSTERINGS)}")
    group = lambda pts, skip: cluster_points(pts, skip, cluster, eps, min_pts, min_cluster_size, min_samples)    # step 2
    up = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt)
    p0, p1 = up(pc0, torch.float32), up(pc1, torch.float32)
    g0, g1 = up(ground0, torch.bool), up(ground1, torch.bool)
    T = np.linalg.inv(np.asarray(pose1, np.float64)) @ np.asarray(pose0, np.float64)
    a = _moved(p0, T)                                           # pc0 in pc1's frame
    b = p1[:, :3].contiguous()
    if a.shape[0] == 0 or b.shape[0] == 0:                      # nothing to compare with: every non-ground in-range point is a candidate
        out = []
        for pts, g in ((a, g0), (b, g1)):
            skip = (g | (pts[:, :2].abs().amax(dim=1) > RANGE_NET)) if pts.shape[0] else torch.zeros(0, dtype=torch.bool, device=dev)
            out.append(group(pts, skip))
        return (out[0][0], out[1][0], torch.maximum(out[0][1], out[1][1])) if return_top else (out[0][0], out[1][0])
    far2 = float(dyn_dist) ** 2
    inv_ref2 = 1.0 / (DYN_REF_RANGE * DYN_REF_RANGE)
    use_a = ~(g0 | (a[:, :2].abs().amax(dim=1) > RANGE_NET))   # step 0
    use_b = ~(g1 | (b[:, :2].abs().amax(dim=1) > RANGE_NET))
    (buf_a, dest_a, cnt_a), (buf_b, dest_b, cnt_b) = _compact(a, use_a), _compact(b, use_b)
    host = _pinned_counts()
    host.copy_(torch.cat([cnt_a, cnt_b]), non_blocking=True)
    landed = torch.cuda.Event()
    landed.record(torch.cuda.current_stream(dev))
    landed.synchronize()                                        # the pair's one host wait
    na, nb = int(host[0]), int(host[1])
    a_in, b_in = buf_a[:na], buf_b[:nb]
    out = []
    for pts, use, dest, mine, other in ((a, use_a, dest_a, a_in, b_in), (b, use_b, dest_b, b_in, a_in)):
        skip = ~use
        if mine.shape[0] and other.shape[0]:
            n = pts.shape[0]
            d2 = torch.full((n + 1,), float("inf"), dtype=torch.float32, device=dev)
            d2[:mine.shape[0]] = nn_grid(mine, other, return_index=False)
            x, y = pts[:, 0], pts[:, 1]
            bar2 = far2 * torch.clamp((x * x + y * y) * inv_ref2, min=1.0)       # (dyn_dist * max(1, r / 30 m))^2, float32 as the oracle
            skip = skip | (d2[dest] <= bar2)                    # a close return in the other sweep: static (the dump row holds inf)
        out.append(group(pts, skip))
    return (out[0][0], out[1][0], torch.maximum(out[0][1], out[1][1])) if return_top else (out[0][0], out[1][0])
