"""The float64 reference of the self-supervised loss (oracle/sslloss_oracle.py: ssl_loss_f64) and the case table
(tests/sslloss_cases.py) checked without a GPU: the closed-form gradient against float64 autograd with the correspondences held
fixed, the reference against the older float32 oracle, the conditions the table promises (exact lattice distances, no ambiguous
correspondence or anchor in a random case, every claimed term > 0, every constructed edge really there), and the table's
sensitivity: each deliberately wrong variant of the reference misses the GPU tolerance on the case built for it."""
import numpy as np
import pytest
import torch

import sslloss_cases as sc
import sslloss_oracle as so


def _autograd(name):
    """the same loss through torch float64 autograd, correspondences taken from the reference and held fixed"""
    _, pc0, pc1, flow, lab0, lab1, n_labels = sc.case(name)
    ref = sc.reference(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    p0, p1 = t(pc0.astype(np.float64)), t(pc1.astype(np.float64))
    f = t(flow.astype(np.float64)).requires_grad_(True)
    moved = t(ref.moved) + (f - f.detach())                  # the float32-rounded value, derivative 1
    l0 = t(lab0.astype(np.int64))
    n0, n1 = len(pc0), len(pc1)
    zero = torch.zeros((), dtype=torch.float64)

    def norm(v):                                             # |v| with the zero sub-gradient at 0
        s = (v * v).sum(1)
        return torch.where(s > 0, s, torch.ones_like(s)).sqrt() * (s > 0)

    def chamfer(a, b, i_ab, i_ba, inv_a, inv_b):
        return ((a - b[t(i_ab)]) ** 2).sum() * inv_a + ((b - a[t(i_ba)]) ** 2).sum() * inv_b

    terms = dict.fromkeys(so.TERMS, zero)
    terms["chamfer_dis"] = chamfer(moved, p1, *ref.corr["full"], 1.0 / n0, 1.0 / n1)
    if (l0 == 0).any():
        terms["static_flow_loss"] = norm(f[l0 == 0]).mean()
    dyn0, dyn1 = t(ref.corr["dyn0"].copy()), t(ref.corr["dyn1"].copy())
    if len(dyn0) and len(dyn1):
        terms["dynamic_chamfer_dis"] = chamfer(moved[dyn0], p1[dyn1], *ref.corr["dyn"], 1.0 / len(dyn0), 1.0 / len(dyn1))
    parts = []
    for lab, a in ref.corr["anchors"].items():
        target = p1[int(ref.corr["raw"][a])] - p0[a]
        parts.append(norm(f[l0 == lab] - target))
    if parts:
        terms["cluster_based_pc0pc1"] = torch.cat(parts).mean()
    total = sum(terms.values())
    total.backward()
    return {k: float(v.detach()) for k, v in terms.items()}, f.grad.numpy()


@pytest.mark.parametrize("name", sc.NAMES)
def test_closed_form_gradient_is_the_autograd_gradient(name):
    ref = sc.reference(name)
    terms, grad = _autograd(name)
    for k in so.TERMS:
        assert terms[k] == pytest.approx(ref.terms[k], rel=1e-12, abs=0), k
    assert (np.abs(grad - ref.grad) <= 1e-12 * ref.abs_sum).all()
    assert ref.total == sum(ref.terms[k] for k in so.TERMS)


def test_agrees_with_the_float32_oracle_on_a_scene():
    """the bounds tests/test_ssl_loss_gpu.py::test_loss_terms_and_gradient holds the kernels to, on its smallest scene"""
    from test_ssl_loss_gpu import _scene
    pc0, pc1, flow, lab0, lab1 = _scene(5, 4000, 3500)
    ref = so.ssl_loss_f64(pc0, pc1, flow, lab0, lab1, int(lab0.max()) + 1)
    old_terms, old_total, old_grad = so.ssl_loss(pc0, pc1, flow, lab0, lab1)
    for k, v in old_terms.items():
        assert ref.terms[k] == pytest.approx(v, rel=2e-5, abs=1e-7), k
        assert v > 0, k
    assert ref.total == pytest.approx(old_total, rel=2e-5)
    assert np.abs(ref.grad - old_grad).max() <= 1e-6 + 1e-4 * np.abs(old_grad).max()


def test_the_table_has_the_sizes_and_families_it_is_meant_to():
    sizes = {(len(sc.case(n)[1]), len(sc.case(n)[2])) for n in sc.NAMES if n.startswith(("size_", "carry_"))}
    assert sizes == set(sc.SMALL_SIZES) | set(sc.CARRY_SIZES)
    for n0, n1 in sc.SMALL_SIZES:
        assert {f"size_{n0}x{n1}_lattice", f"size_{n0}x{n1}_random"} <= set(sc.NAMES)
    assert {sc.family(n) for n in sc.NAMES} == {"lattice", "random"}
    for n in sc.NAMES:                                       # workload-sized scenes stay in tests/test_ssl_loss_gpu.py
        assert n in sc.CARRY or max(len(sc.case(n)[1]), len(sc.case(n)[2])) <= 1000


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc.family(n) == "lattice"])
def test_lattice_distances_are_exact_in_float32(name):
    """every coordinate (moved included) is a multiple of 1/8, and three squared differences of two of them sum below 2^24 units"""
    _, pc0, pc1, flow, *_ = sc.case(name)
    moved = sc.reference(name).moved
    assert (moved == pc0.astype(np.float64) + flow.astype(np.float64)).all()          # the float32 sum was exact
    worst = 0.0
    for a in (pc0, pc1, flow, moved):
        assert (a * 8 == np.round(a * 8)).all()
        worst = max(worst, float(np.abs(a * 8).max()) if a.size else 0.0)
    assert 3 * (2 * worst) ** 2 < 2 ** 24


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc.family(n) == "random"])
def test_random_cases_have_no_ambiguous_correspondence_or_anchor(name):
    """a condition on the table, not a measurement: a seed that fails it is replaced"""
    ref = sc.reference(name)
    assert all(g >= sc.AMBIGUOUS for g in ref.search_gap.values()), ref.search_gap
    assert all(g >= sc.AMBIGUOUS for g in ref.anchor_gap.values()), ref.anchor_gap


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_claimed_term_is_exercised(name):
    ref = sc.reference(name)
    for k in so.TERMS:
        assert (ref.terms[k] > 0) == (k in sc.claims(name)), k
    assert np.isfinite(ref.grad).all() and sc.passes(sc.compare(ref, [*ref.terms.values(), ref.total], ref.grad))


def test_every_constructed_edge_is_really_there():
    ref, case = sc.reference, sc.case
    for name in sc.CARRY:                                    # dynamic rows past the first 1024 block counts, on the large side
        _, pc0, pc1, _, lab0, lab1, _ = case(name)
        big = lab0 if len(pc0) > len(pc1) else lab1
        assert len(big) > 1024 * 256 and (big[1024 * 256:] > 0).sum() >= 40 and (big[:1024 * 256] > 0).sum() > 1024
    for name in ("size_1x1_lattice", "size_1x1_random", "one_dynamic_point_each"):
        assert ref(name).n_dyn == (1, 1)
    assert ref("dynamic_in_pc0_only").n_dyn[0] > 0 and ref("dynamic_in_pc0_only").n_dyn[1] == 0
    assert ref("dynamic_in_pc1_only").n_dyn[0] == 0 and ref("dynamic_in_pc1_only").n_dyn[1] > 0
    assert ref("dynamic_rows_at_block_edges").corr["dyn0"].tolist() == [0, 63, 64, 255, 256, 299]
    lab0 = case("cluster_without_dynamic_neighbour")[4]
    assert (lab0 == 2).sum() > 20 and set(ref("cluster_without_dynamic_neighbour").corr["anchors"]) == {1}
    _, pc0, pc1, flow, lab0, lab1, n_labels = case("labels_above_n_labels")
    assert (lab0 >= n_labels).sum() > 50 and (lab1 >= n_labels).sum() > 50 and max(ref("labels_above_n_labels").corr["anchors"]) < n_labels
    assert set(case("sparse_ids")[4].tolist()) == {0, 1, 7, 1000} and set(ref("sparse_ids").corr["anchors"]) == {1, 7, 1000}
    for name in ("anchor_tie_and_anchor_at_zero", "flow_equals_cluster_target"):
        _, pc0, pc1, flow, lab0, lab1, _ = case(name)
        r = ref(name)
        d_r = ((pc0.astype(np.float64) - pc1.astype(np.float64)[r.corr["raw"]]) ** 2).sum(1)
        assert (r.corr["raw"] == np.arange(len(pc0))).all()
        one = np.nonzero(lab0 == 1)[0]
        assert d_r[10] == d_r[200] == d_r[one].max() == 1.0 and (d_r[one] == 1.0).sum() == 2       # the tie, and only these two
        assert r.corr["anchors"][1] == 10
        assert (d_r[lab0 == 2] == 0).all() and r.corr["anchors"][2] == np.nonzero(lab0 == 2)[0][0]  # an anchor at distance 0
    _, pc0, pc1, flow, lab0, *_ = case("flow_equals_cluster_target")
    assert (flow[lab0 == 1] == (pc1[10] - pc0[10])).all()
    _, pc0, pc1, flow, lab0, lab1, _ = case("every_pc1_point_twice")
    assert (pc1[:280] == pc1[280:]).all() and (lab1[280:] == 0).all() and (lab1[:280] > 0).any()
    _, pc0, pc1, flow, lab0, *_ = case("identical_pc0_pairs")
    assert (pc0[:150] == pc0[150:]).all() and (flow[:150] == flow[150:]).all() and (lab0[:150] == lab0[150:]).all()
    assert (ref("identical_pc0_pairs").n_scat[150:] == 0).all() and ref("identical_pc0_pairs").n_scat[:150].sum() > 330
    assert ref("fan_in").n_scat[5] == 2000 and ref("fan_in").n_scat.sum() == 2000
    _, pc0, pc1, flow, *_ = case("across_the_grid_edge")
    m = ref("across_the_grid_edge").moved
    inside = lambda a: (np.abs(a[:, :2]) < 52).all(1)
    assert np.abs(pc0[:, :2]).max() > 65 and (inside(pc0) & ~inside(m)).sum() > 10 and (~inside(pc0) & inside(m)).sum() > 10
    assert not case("zero_flow")[3].any()


# variant -> the case built to see it
WITNESS = {"ties_highest_row": "identical_pc0_pairs", "anchor_smallest": "one_cluster", "anchor_tie_highest": "anchor_tie_and_anchor_at_zero",
           "nc_all_dynamic": "cluster_without_dynamic_neighbour", "b_grad_not_scattered": "fan_in",
           "big_labels_not_dynamic": "labels_above_n_labels", "nd_swapped": "dynamic_rows_at_block_edges",
           "compaction_reversed": "identical_pc0_pairs"}


@pytest.mark.parametrize("wrong", so.WRONG)
def test_the_table_sees_each_wrong_variant(wrong):
    """a result computed by the wrong rule misses the tolerance the GPU suite applies, on the case built for that rule"""
    assert set(WITNESS) == set(so.WRONG)
    name = WITNESS[wrong]
    bad = so.ssl_loss_f64(*sc.case(name)[1:], wrong=wrong)
    c = sc.compare(sc.reference(name), [*bad.terms.values(), bad.total], bad.grad)
    assert not sc.passes(c) and (c["term"] > 1 or c["grad"] > 1 or not c["zeros"]), c
    seen = [n for n in sc.SMALL if not sc.passes(sc.compare(sc.reference(n), *(lambda b: ([*b.terms.values(), b.total], b.grad))(
        so.ssl_loss_f64(*sc.case(n)[1:], wrong=wrong))))]
    assert name in seen and len(seen) >= 1
    print(f"{wrong}: seen by {len(seen)} of {len(sc.SMALL)} cases")
