"""The BatchNorm checker itself (oracle/bn_oracle.py), on CPU: the float32 twin of the kernels' arrangement must pass both
levels of the check on every case of tests/test_bn_conformance_gpu.py's matrix, each wrong variant of the twin must fail it on
a named case, and every case must keep its discrete facts away from the thresholds of the bound model.  This is what keeps the
tolerances of the GPU matrix honest for whoever edits them."""
import pytest
import torch
import torch.nn.functional as F

import bn_oracle as bo

OUTPUTS = bo.OUTPUTS_FWD + bo.OUTPUTS_BWD


def _verdicts(name, got):
    """{output: (passes, report)} of ``got`` (a dict like twin32's) on case ``name``"""
    c = bo.case(name)
    ref, bnd, twin = bo.refs(name)
    out = {}
    for key in OUTPUTS:
        if key not in ref:                                    # no running statistics in this case
            continue
        worst, rr, report = bo.check_map(got[key], ref[key], bnd[key], twin[key], f"{name} {key}")
        out[key] = (worst <= 1.0 and rr <= bo.R_ELEM, report)
    assert c["x"].shape == (c["n_img"] * c["rows"], c["ch"])
    return out


@pytest.mark.parametrize("name", bo.CASE_NAMES)
def test_the_twin_passes_both_levels(name):
    _, _, twin = bo.refs(name)
    for key, (good, report) in _verdicts(name, twin).items():
        assert good, report


@pytest.mark.parametrize("name", bo.CASE_NAMES)
def test_cases_stay_away_from_the_thresholds(name):
    """var + eps stays positive under its own error, and no pre-activation reaches the |t| where exp(-t^2 / 2) leaves float32's
    normal range (the GELU' budget's relative term assumes a normal exponential)"""
    c = bo.case(name)
    ref, _, _ = bo.refs(name)
    margin, tmax = bo.facts(c, ref)
    assert margin > 0.0, (name, margin)
    assert tmax < bo.T_EXP, (name, tmax)
    assert bool(torch.all(ref["var"] + c["eps"] > 0))
    if "edge" == bo.MATRIX[name][4] and c["n_img"] * c["rows"] > 1:
        assert bool((c["dy"] == 0).any()), "the edge statistics hold exact zeros in dy"


# wrong variant -> the case that must reject it, and the outputs it must be rejected on (any one of them)
REJECTED_BY = {
    "unbiased variance normalises": ("t2 c8", ("invstd", "xhat")),
    "biased variance feeds the running estimate": ("t2 c8", ("running_var",)),
    "momentum on the wrong term": ("t63 c32", ("running_mean", "running_var")),
    "eps outside the square root": ("t63 c32", ("invstd",)),
    "statistics per image": ("s40x3 c64", ("mean", "xhat")),
    "last partial row block dropped": ("t65 c64", ("mean", "dbeta")),
    "single-pass variance in float32": ("shifted mean", ("invstd",)),
    "dx without mean(g)": ("t63 c32", ("dx",)),
    "dx without xhat mean(g xhat)": ("t63 c32", ("dx",)),
    "dgamma from x": ("t63 c32", ("dgamma",)),
    "tanh-GELU derivative": ("t63 c32", ("dx", "dbeta")),
    "accumulate overwrites": ("t65 c68", ("dgamma", "dbeta")),
    "one quad of channels shifted by four": ("t64 c36", ("xhat", "y")),
}


def test_every_wrong_variant_is_listed():
    assert set(REJECTED_BY) == set(bo.WRONG)


@pytest.mark.parametrize("wrong", bo.WRONG)
def test_wrong_variants_are_rejected(wrong):
    name, keys = REJECTED_BY[wrong]
    v = _verdicts(name, bo.twin32(bo.case(name), wrong))
    for key in keys:
        assert not v[key][0], f"{wrong} passed the check on {key}: {v[key][1]}"


def test_dispatch_reproduces_the_block_counts_of_the_matrix():
    met = {name: bo.dispatch(m[0] * m[1], m[2]) for name, m in bo.MATRIX.items()}
    nbs = {d["nb"] for d in met.values()}
    assert {1, 2, 193, 257} <= nbs and max(nbs) >= 600, sorted(nbs)
    assert met["b193 c36"]["nb"] == 193 and met["b193 c36"]["four_chain_trips"] == 1
    assert met["b257 c8"]["nb"] == 257 and met["b257 c4"]["nb"] == 257
    assert met["b683 c36"]["rows_pb"] == 96 and met["b683 c36"]["nb"] == 683
    assert met["t65 c64"]["nb"] == 2 and met["t1 c4"]["nb"] == 1
    assert {d["qs"] for d in met.values()} == {3, 4, 5}
    assert {m[2] for m in bo.MATRIX.values()} == {4, 8, 32, 36, 64, 68, 128, 132, 256}
    # the image splits that make a step cross images, for each of the three G
    for name, G in (("s50x1 c128", 8), ("s40x3 c64", 16), ("s40x3 c4", 32), ("s7x9 c32", 32)):
        assert met[name]["G"] == G and bo.MATRIX[name][1] < G and bo.MATRIX[name][0] > 1, name
    assert met["s3x32 c8"]["G"] == bo.MATRIX["s3x32 c8"][1]
    assert {m[3] for m in bo.MATRIX.values()} == {"dense", "pitch4", "pitch32", "gap", "concat", "alias_xhat", "alias_dx"}


def test_the_constants_follow_the_specification():
    from himo_amd.seflow import spec
    assert (bo.BN_EPS, bo.BN_EPS_PFN) == (spec.BN_EPS, spec.BN_EPS_PFN)


@pytest.mark.parametrize("name", ["t63 c32", "t65 c68", "s40x3 c64"])
def test_reference_matches_float64_autograd(name):
    """reference(case) against F.batch_norm + F.gelu (exact erf) in float64: statistics, running estimates, y and all gradients"""
    c = bo.case(name)
    ref, _, _ = bo.refs(name)
    x = c["x"].double().clone().requires_grad_(True)
    ga, be = c["gamma"].double().clone().requires_grad_(True), c["beta"].double().clone().requires_grad_(True)
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    y = F.gelu(F.batch_norm(x, rm, rv, ga, be, training=True, momentum=float(torch.tensor(c["momentum"], dtype=torch.float32)),
                            eps=float(torch.tensor(c["eps"], dtype=torch.float32))))
    (y * c["dy"].double()).sum().backward()
    close = lambda a, b: torch.allclose(a, b, rtol=1e-10, atol=1e-10 * float(b.abs().max()))
    assert close(ref["y"], y.detach()) and close(ref["dx"], x.grad)
    acc = c["flags"] & 1
    assert close(ref["dgamma"] - (c["old_dgamma"].double() if acc else 0), ga.grad)
    assert close(ref["dbeta"] - (c["old_dbeta"].double() if acc else 0), be.grad)
    assert close(ref["running_mean"], rm) and close(ref["running_var"], rv)


def test_one_row_follows_the_kernels_rule():
    """total = 1: var = 0, xhat = 0, the running variance decays towards var = 0 unchanged (torch refuses this input)"""
    c = bo.case("t1 c4")
    ref, _, twin = bo.refs("t1 c4")
    m = float(torch.tensor(c["momentum"], dtype=torch.float32))
    assert bool(torch.all(ref["var"] == 0)) and bool(torch.all(ref["xhat"] == 0)) and bool(torch.all(twin["xhat"] == 0))
    assert torch.allclose(ref["running_var"], (1 - m) * c["rv"].double(), rtol=1e-15)
    assert bool(torch.all(ref["dx"] == 0))


def test_fold_twin_sits_inside_three_roundings():
    g = torch.Generator().manual_seed(5)
    own = 0.0                                                 # the shift's error over 3 u of its own magnitude
    for ch in (1, 4, 255, 256, 257):
        gamma, beta, mean = torch.randn(ch, generator=g), torch.randn(ch, generator=g), torch.randn(ch, generator=g) * 3
        var = torch.rand(ch, generator=g) * 10.0 ** (-6 * torch.rand(ch, generator=g))
        var[::3] = 0.0
        for eps in (bo.BN_EPS, bo.BN_EPS_PFN):
            s, h = bo.fold(gamma, beta, mean, var, eps)
            s32, h32 = bo.fold(gamma, beta, mean, var, eps, torch.float32)
            bs, bh = bo.fold_bound(gamma, beta, mean, var, eps)
            assert bool(torch.all((s32.double() - s).abs() <= bs)) and bool(torch.all((h32.double() - h).abs() <= bh)), (ch, eps)
            wrong = gamma.double() / (torch.sqrt(var.double()) + eps)              # eps outside the root
            assert not bool(torch.all((wrong - s).abs() <= bs)) or ch == 1
            mag = 3 * bo.U * (beta.double().abs() + (mean.double() * s).abs())
            own = max(own, float(((h32.double() - h).abs() / mag).max()))
    # the correctly rounded float32 formula misses 3 u of the shift's own magnitude: why fold_bound carries the scale's 3 u instead
    assert 1.0 < own < 1.5, own
