"""The float64 reference of the per-pair fit kernels (oracle/nsf_oracle.py) and its case tables checked without a GPU: the
closed-form backward pass against float64 autograd, the brute-force distance transform against scipy's exact Euclidean one,
the conditions the tables promise (every decision margin, the candidate cap, every constructed edge really there), that the
correct float32 twin passes every check of tests/test_nsf_conformance_gpu.py, and the checks' sensitivity: each deliberately
wrong variant of the twin misses the GPU test's bound on the case built for it."""
import numpy as np
import pytest
import torch

import nsf_oracle as no

F64 = torch.float64


def _passes(checks):
    bad = [rep for fam, name, arith, got, ref, bnd, r32, cols in checks
           for good, w, rr, rep in [no.verdict(arith, got, ref, bnd, r32, f"{fam}/{name}", cols=cols)] if not good]
    return not bad, bad


def _twin(case, variant=None, **kw):
    r = no.iteration(case.params, case.x, case.n, case.grid, torch.float32, variant, **kw)
    return dict(out=r["out"], dout=r["dout"], dsum=r["dsum"], m=r["m"], grads=r["grads"])


# ---- the reference itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_hidden,dead", [(63, 2, True), (64, 8, True), (65, 12, False)])
def test_closed_form_backward_is_the_autograd_gradient(n, n_hidden, dead):
    case = no.mlp_case(n, n_hidden, dead)
    params = [(w.double().requires_grad_(True), b.double().requires_grad_(True)) for w, b in case.params]
    zs, out = no.forward(params, case.x)
    lk = no.lookup(case.x[:, :3].double() + out[:, :3], case.grid)
    real = torch.arange(len(case.x)) < n
    total = torch.where(lk["keep"] & real, lk["D"], torch.zeros_like(lk["D"])).sum()
    total.backward()
    assert float(total.detach()) == pytest.approx(case.ref["dsum"], rel=1e-12)
    x64 = case.x.double()
    for k, ((w, b), (gw, gb)) in enumerate(zip(params, case.ref["grads"])):
        dz = case.ref["dout"].abs() if k == n_hidden else (case.ref["gs"][k] * (case.ref["zs"][k] > 0)).abs()
        hin = x64.abs() if k == 0 else case.ref["zs"][k - 1].clamp(min=0)
        assert (w.grad - gw).abs().max() <= 1e-12 * float((hin.T @ dz).max()), k
        assert (b.grad - gb).abs().max() <= 1e-12 * float(dz.sum(0).max()), k


def test_closed_form_backward_with_an_external_dout_is_the_autograd_gradient():
    case = no.mlp_case(65, 2, objective=False, seed=4)
    dout = torch.randn(len(case.x), 4, generator=torch.Generator().manual_seed(1)).double()
    params = [(w.double().requires_grad_(True), b.double().requires_grad_(True)) for w, b in case.params]
    (no.forward(params, case.x)[1] * dout).sum().backward()
    ref = no.iteration(case.params, case.x, case.n, dout=dout)
    for (w, b), (gw, gb) in zip(params, ref["grads"]):
        assert torch.allclose(w.grad, gw, rtol=1e-11, atol=1e-11) and torch.allclose(b.grad, gb, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("dims,window", [((37, 21, 9), 5), ((9, 30, 17), 40), ((64, 3, 1), 3)])
def test_brute_force_transform_is_the_exact_euclidean_one_below_the_window(dims, window):
    from scipy.ndimage import distance_transform_edt
    g = np.random.default_rng(sum(dims))
    occ = g.random(dims[::-1]) < 0.01
    occ.flat[g.integers(occ.size)] = True
    G = no.dt_brute(occ, window)
    d2 = np.rint(distance_transform_edt(~occ) ** 2).astype(np.int64)
    near = d2 < window * window                                  # nearer than the window: within it on every axis
    assert near.any() and np.array_equal(G[near].astype(np.int64), d2[near])
    assert (G[~near].astype(np.int64) >= d2[~near]).all()         # never nearer than the true distance; 0xFFFF where nothing is in reach
    assert no.dt_brute(np.zeros((3, 4, 5), bool), 2).min() == no.INF


def test_occupancy_follows_the_mark_rule():
    gr = no.grid((0.0, 0.0, 0.0), 0.25, (4, 3, 2), 1, 0.5)
    pts = np.asarray([[0.0, 0.0, 0.0], [1.0, 0.1, 0.1], [0.99, 0.74, 0.49], [np.nan, 0.1, 0.1], [-0.01, 0.1, 0.1], [0.1, 0.75, 0.1]], np.float32)
    occ = no.occupancy(pts, gr)
    assert occ.sum() == 2 and occ[0, 0, 0] and occ[1, 2, 3]       # the far faces, NaN and the negative side are dropped


# ---- what the tables promise -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_hidden,dead", sorted(set(no.FWD_CASES + no.BWD_CASES)))
def test_network_cases_keep_their_promises(n, n_hidden, dead):
    case = no.mlp_case(n, n_hidden, dead)
    ref, real = case.ref, torch.arange(len(case.x)) < n
    assert case.drawn <= no.CAP * n and len(case.x) == no.padded_rows(n) and not case.x[n:].any() and not case.x[:, 3].any()
    assert bool(no.relu_margin_ok([z[:n] for z in ref["zs"]], [e[:n] for e in case.E]).all())
    assert bool(case.lookup_ok[:n].all())
    assert all(bool(torch.isfinite(e).all()) for e in case.E) and bool(torch.isfinite(case.e_out).all())
    # the bound on out stays orders below the cell it has to resolve, and every gradient bound below the gradient's own scale
    assert float(case.e_out[:n].max()) < 0.01 * float(case.grid.cell)
    lk = ref["look"]
    if n >= 63:
        assert bool((lk["inside"] & ~lk["keep"] & real).any()), "no point beyond trunc"
        assert bool((~lk["inside"] & real).any()), "no point outside the volume"
        assert bool((lk["keep"] & real).any())
        assert any(bool((z[:n] <= 0).all(0).any()) for z in ref["zs"]) or not dead, "no dead unit"
    if dead:
        assert all(bool((ref["zs"][0][:n, j] <= 0).all()) for j in no.DEAD_FIRST)
        if n >= 63:
            row = int(torch.nonzero((case.x[:n, :3] == torch.tensor(no.SPECIAL_DEAD)).all(1))[0])
            assert bool((ref["zs"][0][row] < 0).all()), "the dead row is not dead"
            assert bool(lk["keep"][row]), "the dead row has no gradient to lose"


def test_the_tables_cover_what_they_claim():
    for cases in (no.FWD_CASES, no.BWD_CASES):
        assert {c[0] for c in cases} == {1, 63, 64, 65, 255, 256, 257, 321}
    assert {c[1] for c in no.FWD_CASES} == {1, 2, 8, 12} and {c[1] for c in no.BWD_CASES} == {2, 8, 12}
    assert any(no.padded_rows(n) // 64 > -(-n // 64) for n, _, _ in no.BWD_CASES), "no padding tile"
    assert any(no.padded_rows(n) // 256 > 1 for n, _, _ in no.BWD_CASES), "no second backward block"
    dims = [c[0] for c in no.DT_CASES]
    assert {d[0] for d in dims} == {1, 2, 255, 256, 257, 300}
    assert {d[1] for d in dims} == {1, 2, 63, 64, 65} == {d[2] for d in dims}
    assert {c[1] for c in no.DT_CASES} == {1, 3, 21, 40} and {c[2] for c in no.DT_CASES} == {0.1, 0.25}
    assert any(c[1] > max(c[0]) for c in no.DT_CASES), "no window larger than the volume"
    assert {c[3] for c in no.DT_CASES} == {"empty", "one", "faces", "nan_neg", "full", "sparse"}
    assert {c[1] for c in no.DT_LOSS_CASES} == {0, 1, 255, 256, 257, 1000}


@pytest.mark.parametrize("i", range(len(no.DT_CASES)))
def test_distance_transform_cases_keep_their_promises(i):
    gr = no.dt_case(i)
    kind, occ = gr.kind, no.occupancy(gr.targets, gr)
    if kind == "faces":                                           # at the threshold, exactly: the float32 quotient is the float64 one
        q = (gr.targets - gr.origin) / gr.cell
        assert np.array_equal(q.astype(np.float64), (gr.targets.astype(np.float64) - gr.origin) / float(gr.cell)) and (q == np.round(q)).any()
    else:
        assert bool(no.mark_margin_ok(gr.targets, gr).all())
    assert gr.G.shape == gr.dims[::-1] and np.array_equal(gr.G == 0, occ)
    if kind == "empty":
        assert len(gr.targets) == 0 and (gr.G == no.INF).all()
    if kind == "full":
        assert occ.all()
    if kind == "one":
        assert occ.sum() == 1
    if kind == "faces":                                           # three near faces and the near corner are kept, every far face dropped
        assert len(gr.targets) == 8 and occ.sum() == 4
    if kind in ("sparse", "nan_neg"):
        assert 0 < occ.sum() < len(gr.targets)                    # the negative side (and NaN) dropped
    if kind == "nan_neg":
        assert np.isnan(gr.targets).any(1).sum() == 4
    if min(gr.dims) > 2 * gr.window and kind == "sparse":
        assert (gr.G == no.INF).any()


@pytest.mark.parametrize("i,n,nan", no.DT_LOSS_CASES)
def test_lookup_cases_keep_their_promises(i, n, nan):
    gr = no.dt_case(i)
    pts, drawn = no.dt_points(gr, n, nan=nan)
    ref = no.dt_objective(pts, gr)
    assert drawn <= no.CAP * max(n, 1) and len(pts) == n
    if gr.dims[2] == 1:
        assert ref["m"] == 0 and ref["loss"] == 0.0 and not ref["grad"].any()
    elif n >= 255:
        lk = ref["look"]
        assert 0 < ref["m"] < n and bool((lk["inside"] & ~lk["keep"]).any()) and bool(lk["keep"].any())
    if nan:
        assert bool(torch.isnan(pts).any()) and not torch.isnan(ref["grad"]).any()
    twin = no.dt_objective(pts, gr, torch.float32)
    good, bad = _passes(no.dt_loss_checks(gr, pts, dict(loss=twin["loss"], grad=twin["grad"])))
    assert good, bad


def test_threshold_points_decide_as_documented():
    gr, pts = no.threshold_grid(), no.threshold_points()
    assert gr.G[3, 3, 5] == 4 and gr.G[3, 3, 3] == 0
    r = no.lookup(torch.tensor(list(pts.values())), gr)
    d = dict(zip(pts, range(len(pts))))
    assert not r["inside"][d["u_zero"]] and not r["inside"][d["u_last"]]
    i = d["u_integer"]
    assert r["inside"][i] and float(r["D"][i]) == 0.25 and r["keep"][i]             # the value of cell (4, 3, 3) itself: one cell
    i = d["d_is_trunc"]
    assert r["inside"][i] and float(r["D"][i]) == 0.5 == float(gr.trunc) and r["keep"][i] and bool(r["gr"][i].any())
    for dtype in (torch.float32, F64):                            # exactly representable: both precisions agree to the bit
        assert torch.equal(no.lookup(torch.tensor(list(pts.values())), gr, dtype)["u"].double(), r["u"])


def test_mask_threshold_case_has_its_zeros():
    case = no.mask_threshold_case()
    z0 = case.ref["zs"][0]
    assert not case.x[0].any() and all(float(z0[0, j]) == 0.0 for j in no.MASK_ZERO_BIAS)
    assert all(float(case.E[0][0, j]) == 0.0 for j in no.MASK_ZERO_BIAS)         # exact in either precision: the margin 0 >= 2 x 0 holds
    assert bool(no.relu_margin_ok([z[:4] for z in case.ref["zs"]], [e[:4] for e in case.E]).all()) and bool(case.lookup_ok[:4].all())
    assert bool(case.ref["look"]["keep"][0]) and bool(case.ref["gs"][0][0, list(no.MASK_ZERO_BIAS)].abs().min() > 0)
    assert all(float(case.ref["grads"][0][1][j]) != float((case.ref["gs"][0] * (z0 >= 0)).sum(0)[j]) for j in no.MASK_ZERO_BIAS)


# ---- the checks pass the float32 twin and fail the wrong ones ---------------------------------------------------------------
@pytest.mark.parametrize("n,n_hidden,dead", [(63, 2, True), (64, 8, True), (65, 12, False), (257, 8, False)])
def test_float32_twin_passes_every_check(n, n_hidden, dead):
    case = no.mlp_case(n, n_hidden, dead)
    good, bad = _passes(no.iteration_checks(case, _twin(case)))
    assert good, bad


def test_the_bound_of_the_split_products_covers_grad_oracle_s():
    """wgrad_coeff |A|^T |B| is grad_oracle.product_bound with the splits at their worst case: never below it on real operands"""
    import grad_oracle as go
    a, b = go.operands(3, (256, 128), (256, 128))
    mine = no.wgrad_coeff() * (a.double().abs().T @ b.double().abs())
    assert bool((mine >= go.product_bound("bf16x2", a.numpy(), b.numpy()) - go.TINY).all())
    assert float((mine / go.product_bound("bf16x2", a.numpy(), b.numpy())).median()) < 2.0


WRONG_NETWORK = ("mask_prev", "mask_ge", "pad_in_m", "bias_pad", "swap_rows")


@pytest.mark.parametrize("variant", WRONG_NETWORK)
def test_wrong_network_variants_miss_the_bounds(variant):
    case = no.mask_threshold_case() if variant == "mask_ge" else no.mlp_case(63, 2, True)
    good, bad = _passes(no.iteration_checks(case, _twin(case)))
    assert good, bad
    kw = {}
    if variant == "swap_rows":                                    # two rows of the first 32-row half that both carry a gradient
        rows = torch.nonzero(case.ref["look"]["keep"][:32])[:2, 0].tolist()
        r = no.iteration(case.params, case.x, case.n, case.grid, torch.float32)
        grads, _ = no.backward(case.params, case.x, r["zs"], r["dout"], torch.float32, "swap_rows", swap=rows)
        wrong = dict(grads=grads)
    else:
        wrong = _twin(case, variant, **kw)
    good, bad = _passes(no.iteration_checks(case, wrong))
    assert not good, f"{variant} passes every check"
    expect = dict(mask_prev="backward/", mask_ge="backward/db0", pad_in_m="objective/count", bias_pad="backward/db1", swap_rows="backward/dW1")[variant]
    assert any(expect in rep for rep in bad), (variant, bad)


@pytest.mark.parametrize("variant", ("trunc_lt", "inside_ge", "corner", "no_scale"))
def test_wrong_lookup_variants_miss_the_bounds(variant):
    if variant in ("trunc_lt", "inside_ge"):
        gr, exact = no.threshold_grid(), True
        pts = torch.tensor(list(no.threshold_points().values()))
    else:
        gr, exact = no.dt_case(4), False
        pts, _ = no.dt_points(gr, 257)
    ok = no.dt_objective(pts, gr, torch.float32)
    good, bad = _passes(no.dt_loss_checks(gr, pts, dict(loss=ok["loss"], grad=ok["grad"]), exact))
    assert good, bad
    w = no.dt_objective(pts, gr, torch.float32, variant)
    good, bad = _passes(no.dt_loss_checks(gr, pts, dict(loss=w["loss"], grad=w["grad"]), exact))
    assert not good, f"{variant} passes every check"


@pytest.mark.parametrize("step", (1, 1000))
def test_adam_twin_passes_and_adam_without_bias_correction_misses(step):
    g = torch.Generator().manual_seed(step)
    p, grad = torch.randn(4096, generator=g) * 0.1, torch.randn(4096, generator=g) * 10.0 ** (-4 * torch.rand(4096, generator=g))
    m, v = (torch.zeros(4096), torch.zeros(4096)) if step == 1 else (torch.randn(4096, generator=g) * 1e-2, torch.rand(4096, generator=g) * 1e-4)
    ref, bnd = no.adam(p, grad, m, v, step), no.adam_bound(p, grad, m, v, step)
    for variant, want in ((None, True), ("adam_nobc", False)):
        got = no.adam(p, grad, m, v, step, torch.float32, variant)
        res = [no.verdict("f32", a, r, bnd[k], None, k)[0] for a, r, k in zip(got, ref, ("p", "m", "v"))]
        assert all(res) == want and res[1] and res[2], (variant, res)
    # torch.optim.Adam's own order, in float64
    pt = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=float(no.ADAM["lr"]), betas=(float(no.ADAM["b1"]), float(no.ADAM["b2"])), eps=float(no.ADAM["eps"]))
    if step == 1:
        pt.grad = grad.double()
        opt.step()
        assert torch.allclose(pt.detach(), ref[0], rtol=1e-13, atol=1e-15)


def test_threshold_network_case_decides_in_the_fused_forward_s_own_lines():
    case = no.threshold_network_case()
    assert case.ref["m"] == 3 and not case.ref["out"].any() and float(case.e_out.max()) == 0.0
    good, bad = _passes(no.iteration_checks(case, _twin(case)))
    assert good, bad
    for variant in ("trunc_lt", "inside_ge"):
        good, bad = _passes(no.iteration_checks(case, _twin(case, variant)))
        assert not good, f"{variant} passes every check"
