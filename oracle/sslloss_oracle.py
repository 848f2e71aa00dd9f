"""CPU ORACLE for the self-supervised loss terms (stage a11) -- test infrastructure, NOT product code.

PARITY UNPINNED: the reference's `seflowppLoss` is in the absent OpenSceneFlow submodule; only
the term names and unit weights are in the tree (assets/slurm/ssl-train-av2.sh:33).  This restates THIS BUILD'S
specification (himo_amd/csrc/sslloss.hip header) with PyTorch CPU ops (autograd for the gradient) and scipy's
cKDTree for the correspondences.

``ssl_loss`` is the float32 restatement (cKDTree's tie order is arbitrary); ``ssl_loss_f64`` below is the float64 reference with the
tie rules made explicit ("ties: lowest row", "anchor ties: lowest index") and a closed-form gradient, which the conformance suite
(tests/test_sslloss_conformance_gpu.py) holds the kernels to at every point.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.spatial import cKDTree


def nearest(query: np.ndarray, ref: np.ndarray):
    """float32 squared distances + indices, exact (k=1)."""
    d, i = cKDTree(ref.astype(np.float64)).query(query.astype(np.float64), k=1)
    diff = query.astype(np.float32) - ref.astype(np.float32)[i]
    return (diff * diff).sum(1), i


def ssl_loss(pc0, pc1, flow, label0, label1):
    """-> ({term: float}, total float, grad (N0,3) float32)."""
    p0 = torch.from_numpy(np.ascontiguousarray(pc0[:, :3], dtype=np.float32))
    p1 = torch.from_numpy(np.ascontiguousarray(pc1[:, :3], dtype=np.float32))
    f = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).clone().requires_grad_(True)
    l0 = torch.from_numpy(np.asarray(label0).astype(np.int64))
    l1 = torch.from_numpy(np.asarray(label1).astype(np.int64))
    moved = p0 + f
    mv = moved.detach().numpy()

    def chamfer(a_t, a_np, b_t, b_np):
        if len(a_np) == 0 or len(b_np) == 0:
            return torch.zeros((), dtype=torch.float64)
        _, ia = nearest(a_np, b_np)
        _, ib = nearest(b_np, a_np)
        da = ((a_t - b_t[torch.from_numpy(ia)]) ** 2).sum(1)
        db = ((b_t - a_t[torch.from_numpy(ib)]) ** 2).sum(1)
        return da.double().mean() + db.double().mean()

    terms = {}
    terms["chamfer_dis"] = chamfer(moved, mv, p1, p1.numpy())
    st = l0 == 0
    terms["static_flow_loss"] = torch.linalg.vector_norm(f[st], dim=-1).double().mean() if st.any() else torch.zeros((), dtype=torch.float64)
    d0, d1 = l0 > 0, l1 > 0
    terms["dynamic_chamfer_dis"] = chamfer(moved[d0], mv[d0.numpy()], p1[d1], p1[d1].numpy())
    # cluster term
    norms = []
    if len(p0) and len(p1):
        raw_d, raw_i = nearest(p0.numpy(), p1.numpy())
        for lab in torch.unique(l0).tolist():
            if lab <= 0:
                continue
            members = torch.nonzero(l0 == lab).squeeze(1).numpy()
            ok = l1.numpy()[raw_i[members]] > 0
            if not ok.any():
                continue
            cand = members[ok]
            dmax = raw_d[cand].max()
            anchor = cand[raw_d[cand] == dmax].min()                   # ties: lowest index
            target = p1[raw_i[anchor]] - p0[anchor]
            norms.append(torch.linalg.vector_norm(f[torch.from_numpy(members)] - target, dim=-1))
    terms["cluster_based_pc0pc1"] = torch.cat(norms).double().mean() if norms else torch.zeros((), dtype=torch.float64)
    total = sum(terms.values())
    if total.requires_grad:
        total.backward()
        grad = f.grad.numpy()
    else:
        grad = np.zeros_like(flow, dtype=np.float32)
    return {k: float(v) for k, v in terms.items()}, float(total), grad


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference with an explicit tie rule (tests/test_sslloss_oracle.py checks it, tests/test_sslloss_conformance_gpu.py uses it)
# ---------------------------------------------------------------------------------------------------------------------------
TERMS = ("chamfer_dis", "static_flow_loss", "dynamic_chamfer_dis", "cluster_based_pc0pc1")
EXHAUSTIVE_PAIRS = 20_000_000          # above this many query x reference pairs a search goes through cKDTree (k = 2)
# wrong variants of the reference: the mistakes the case table must be able to see (tests/test_sslloss_oracle.py)
WRONG = ("ties_highest_row", "anchor_smallest", "anchor_tie_highest", "nc_all_dynamic", "b_grad_not_scattered",
         "big_labels_not_dynamic", "nd_swapped", "compaction_reversed")


def search_f64(q, r, highest=False):
    """Nearest row of ``r`` for every row of ``q`` in float64: (squared distances, rows, smallest relative gap between the best and
    the second-best DISTINCT squared distance over the queries).  Exact ties go to the lowest row (``highest``: a wrong variant).
    Searches above EXHAUSTIVE_PAIRS use cKDTree with k = 2, recompute both candidates and assert that no exact tie occurs."""
    q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
    nq, nr = len(q), len(r)
    d = np.empty(nq, np.float64)
    idx = np.empty(nq, np.int64)
    gap = np.inf
    if nq * nr > EXHAUSTIVE_PAIRS:
        _, cand = cKDTree(r).query(q, k=2)
        dd = ((q[:, None, :] - r[cand]) ** 2).sum(-1)
        assert (dd[:, 0] != dd[:, 1]).all(), "an exact tie in a search too large for the exhaustive rule"
        first = dd.argmin(1)
        rows = np.arange(nq)
        d, idx = dd[rows, first], cand[rows, first]
        second = dd[rows, 1 - first]
        with np.errstate(divide="ignore"):
            gap = float(((second - d) / d).min())
        assert gap > 1e-12, "cKDTree's own rounding could have decided this search"
        return d, idx, gap
    step = max(1, 4_000_000 // max(nr, 1))
    for s in range(0, nq, step):
        D = ((q[s:s + step, None, :] - r[None, :, :]) ** 2).sum(-1)
        best = D.min(1)
        hit = D == best[:, None]
        idx[s:s + step] = (nr - 1 - hit[:, ::-1].argmax(1)) if highest else hit.argmax(1)
        d[s:s + step] = best
        D[hit] = np.inf
        second = D.min(1)
        ok = np.isfinite(second) & (best > 0)
        if ok.any():
            gap = min(gap, float(((second[ok] - best[ok]) / best[ok]).min()))
    return d, idx, gap


class SslRef:
    """What ``ssl_loss_f64`` returns: ``terms`` {name: float}, ``total``, ``grad`` [n0, 3] float64, ``abs_sum`` [n0, 3] (per point and
    component, the sum of |contribution| over everything added into that gradient entry), ``n_scat`` [n0] (contributions scattered
    onto the point from the pc1 side), ``search_gap`` {search: smallest relative gap best / second-best distinct squared distance},
    ``anchor_gap`` {label: relative gap between the two largest distinct candidate raw distances}, and the correspondences
    (``corr``) for checks that hold them fixed."""


def ssl_loss_f64(pc0, pc1, flow, label0, label1, n_labels, wrong=None):
    """The specification of csrc/sslloss.hip in float64, gradient in closed form.  The one float32 step is part of the specification:
    ``moved = float32(pc0 + flow)``, promoted afterwards.  Ties: lowest row; anchor ties: lowest index.  Labels: 0 static; > 0 dynamic
    for the Chamfer subsets; 1 .. n_labels - 1 clusters; labels >= n_labels are dynamic for the Chamfer subsets, not part of the
    cluster term, not static; negative labels take part in the full Chamfer only.  ``wrong``: one of WRONG, a deliberately wrong variant."""
    assert wrong is None or wrong in WRONG
    p0_32 = np.ascontiguousarray(np.asarray(pc0)[:, :3], np.float32)
    f_32 = np.ascontiguousarray(flow, np.float32)
    p0, p1, f = p0_32.astype(np.float64), np.ascontiguousarray(np.asarray(pc1)[:, :3], np.float32).astype(np.float64), f_32.astype(np.float64)
    moved = (p0_32 + f_32).astype(np.float32).astype(np.float64)
    l0, l1 = np.asarray(label0).astype(np.int64), np.asarray(label1).astype(np.int64)
    n0, n1 = len(p0), len(p1)
    hi = wrong == "ties_highest_row"
    grad, abs_sum, n_scat = np.zeros((n0, 3)), np.zeros((n0, 3)), np.zeros(n0, np.int64)
    terms = dict.fromkeys(TERMS, 0.0)
    gaps, anchor_gap, corr = {}, {}, {}

    def add(rows, contrib, scattered=False):
        np.add.at(grad, rows, contrib)
        np.add.at(abs_sum, rows, np.abs(contrib))
        if scattered:
            np.add.at(n_scat, rows, 1)

    def chamfer(tag, a, b, rows_a, inv_a, inv_b, key):
        """a -> b and b -> a; ``rows_a``: the pc0 rows of ``a``"""
        d_ab, i_ab, gaps[tag + "_fwd"] = search_f64(a, b, hi)
        d_ba, i_ba, gaps[tag + "_bwd"] = search_f64(b, a, hi)
        corr[tag] = (i_ab, i_ba)
        terms[key] = float(d_ab.sum() * inv_a + d_ba.sum() * inv_b)
        add(rows_a, 2.0 * inv_a * (a - b[i_ab]))
        if wrong == "b_grad_not_scattered":
            add(rows_a, 2.0 * inv_b * (a - b[i_ab]))
        else:
            add(rows_a[i_ba], 2.0 * inv_b * (a[i_ba] - b), scattered=True)

    if n0 and n1:
        chamfer("full", moved, p1, np.arange(n0), 1.0 / n0, 1.0 / n1, "chamfer_dis")
    st = np.nonzero(l0 == 0)[0]
    if len(st):
        nrm = np.sqrt((f[st] ** 2).sum(1))
        terms["static_flow_loss"] = float(nrm.sum() / len(st))
        nz = nrm > 0
        add(st[nz], f[st[nz]] / (nrm[nz, None] * len(st)))
    big0, big1 = (l0 >= n_labels, l1 >= n_labels) if wrong == "big_labels_not_dynamic" else (False, False)
    dyn0, dyn1 = np.nonzero((l0 > 0) & ~big0)[0], np.nonzero((l1 > 0) & ~big1)[0]
    if wrong == "compaction_reversed":
        dyn0, dyn1 = dyn0[::-1], dyn1[::-1]
    corr["dyn0"], corr["dyn1"] = dyn0, dyn1
    if len(dyn0) and len(dyn1):
        inv0, inv1 = 1.0 / len(dyn0), 1.0 / len(dyn1)
        if wrong == "nd_swapped":
            inv0, inv1 = inv1, inv0
        chamfer("dyn", moved[dyn0], p1[dyn1], dyn0, inv0, inv1, "dynamic_chamfer_dis")
    if n0 and n1:
        d_r, i_r, gaps["raw"] = search_f64(p0, p1, hi)
        corr["raw"] = i_r
        anchors = {}
        for lab in np.unique(l0):
            if lab <= 0 or lab >= n_labels:
                continue
            members = np.nonzero(l0 == lab)[0]
            cand = members[l1[i_r[members]] > 0]
            if not len(cand):
                continue
            dc = d_r[cand]
            pick = dc.min() if wrong == "anchor_smallest" else dc.max()
            tied = cand[dc == pick]
            anchors[int(lab)] = int(tied.max() if wrong == "anchor_tie_highest" else tied.min())
            other = dc[dc != pick]
            if len(other) and wrong != "anchor_smallest":
                anchor_gap[int(lab)] = float((pick - other.max()) / pick)
        corr["anchors"] = anchors
        if anchors:
            in_cluster = np.nonzero(np.isin(l0, list(anchors)))[0]
            nc = int((l0 > 0).sum()) if wrong == "nc_all_dynamic" else len(in_cluster)
            a_of = np.array([anchors[int(l)] for l in l0[in_cluster]], np.int64)
            e = f[in_cluster] - (p1[i_r[a_of]] - p0[a_of])
            nrm = np.sqrt((e ** 2).sum(1))
            terms["cluster_based_pc0pc1"] = float(nrm.sum() / nc)
            nz = nrm > 0
            add(in_cluster[nz], e[nz] / (nrm[nz, None] * nc))
    out = SslRef()
    out.terms, out.total = terms, float(sum(terms[k] for k in TERMS))
    out.grad, out.abs_sum, out.n_scat, out.search_gap, out.anchor_gap, out.corr = grad, abs_sum, n_scat, gaps, anchor_gap, corr
    out.moved, out.n_dyn = moved, (len(dyn0), len(dyn1))
    return out
