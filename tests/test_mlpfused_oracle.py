"""The reference of the layer-kernel path of the per-pair fit (oracle/mlpfused_oracle.py) checked without a GPU: the float32
twin passes every check of tests/test_mlpfused_conformance_gpu.py on every case that suite uses, each of the eight deliberately
wrong twins misses a bound or an equality on the case the GPU test uses for that purpose, the keep-best restatement is
himo_amd.nsfp.stop_rule on the scripted loss lists, and the constructed edges are really there.  The network cases are
nsf_oracle's, unchanged: |z| >= 2 E for every unit, at most CAP candidates per kept point (tests/test_nsf_oracle.py asserts that)."""
import math

import numpy as np
import pytest
import torch

import mlpfused_oracle as mo
import nsf_oracle as no

FWD = sorted(set(no.FWD_CASES))
BWD = sorted(set(no.BWD_CASES))
N_BLOCKS = (1, 7, 8, 9, 24, 25, 31, 32, 33, 57, 64, 65)


def _passes(checks):
    bad = [rep for fam, name, arith, got, ref, bnd, r32, cols in checks
           for good, w, rr, rep in [mo.verdict(fam, arith, got, ref, bnd, r32, f"{fam}/{name}", cols=cols)] if not good]
    return not bad, bad


# ---- the network ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_hidden,dead", FWD)
def test_float32_twin_passes_the_forward_checks(n, n_hidden, dead):
    case = no.mlp_case(n, n_hidden, dead)
    assert mo.padding_margin_ok(case), "a padding row's unit is nearer than 2 E to its threshold"
    t = mo.twin(case)
    good, bad = _passes(mo.mlpfused_checks(case, dict(H=t["H"], out=t["out"])))
    assert good, bad
    R = mo.block_rows(n)
    assert R == -(-n // 64) * 64 <= len(case.x) and all(len(h) == R for h in t["H"])


@pytest.mark.parametrize("n,n_hidden,dead", BWD)
def test_float32_twin_passes_the_backward_checks(n, n_hidden, dead):
    case = mo.mlp_case(n, n_hidden, dead)
    assert not case.dout[n:].any() and case.dout[:n].abs().min() > 0
    good, bad = _passes(mo.mlpfused_checks(case, mo.twin(case)))
    assert good, bad
    if dead and n >= 63:                                          # the fully dead row: H and dZ exactly zero in the reference
        row = int(torch.nonzero((case.x[:n, :3] == torch.tensor(no.SPECIAL_DEAD)).all(1))[0])
        assert all(not bool((z[row] > 0).any()) for z in case.ref["zs"][:1])
    for k in range(n_hidden):                                     # padding rows: dZ exactly zero is DEMANDED (bound zero)
        assert not bool(case.e_g[k][n:].any())


def test_mask_case_has_its_zeros_and_the_twin_passes():
    case = mo.mask_case()
    z0 = case.ref["zs"][0]
    assert all(float(z0[0, j]) == 0.0 for j in no.MASK_ZERO_BIAS) and mo.padding_margin_ok(case)
    assert bool(case.ref["gs"][0][0, list(no.MASK_ZERO_BIAS)].abs().min() > 0)       # a gradient arrives there and must be masked
    t = mo.twin(case)
    good, bad = _passes(mo.mlpfused_checks(case, t))
    assert good, bad
    # z > 0, not z >= 0: a twin that lets the gradient through at z == 0 misses dZ0 and db0
    wrong = dict(t)
    wrong["dZ"] = [case.ref32["gs"][k][:64] * (case.ref32["zs"][k][:64] >= 0) for k in range(case.n_hidden)]
    wrong["db"] = [mo.bias_sum_f32(d) for d in wrong["dZ"]]
    good, bad = _passes(mo.mlpfused_checks(case, wrong))
    assert not good and any("dZ0" in r for r in bad) and any("db0" in r for r in bad)


def test_bias_depth_counts_the_reduce_loops():
    assert [mo.reduce_chain(b) for b in (1, 8, 9, 24, 25, 32, 33, 57, 64, 65)] == [1, 1, 2, 3, 3, 1, 2, 4, 2, 3]
    assert mo.bias_depth(1) == 32 + 1 + 1 + 2 + 7
    rows = sorted(mo.mlp_row(rt, r, lh) for rt in (0, 1) for r in range(16) for lh in (0, 1))
    assert rows == list(range(64)) and all(mo.mlp_row(rt, r, 1) & 4 for rt in (0, 1) for r in range(16))


def _reduce_twin(n_blocks):
    c = mo.reduce_case(n_blocks)
    r = no.iteration(c.params, c.x, c.n, dtype=torch.float32, dout=c.dout)
    return [r["gs"][k] * (r["zs"][k] > 0) for k in range(2)]


@pytest.mark.parametrize("n_blocks", N_BLOCKS)
def test_float32_twin_passes_the_reduce_checks(n_blocks):
    dz = _reduce_twin(n_blocks)
    good, bad = _passes(mo.bias_reduce_checks(dz, [mo.bias_sum_f32(d) for d in dz], n_blocks))
    assert good, bad


# ---- Chamfer, the NSFP objective, keep-best ---------------------------------------------------------------------------------------
def _cham(c, dtype=np.float32, variant=None):
    return mo.chamfer(c.moved, c.pc1, c.d_a, c.i_a, c.d_b, c.i_b, c.trunc, dtype, variant)


@pytest.mark.parametrize("n0,n1", mo.CHAMFER_CASES)
def test_chamfer_cases_keep_their_promises_and_the_twin_passes(n0, n1):
    c = mo.chamfer_case(n0, n1)
    assert c.t2 == 0.25 and max(np.abs(c.moved).max(initial=0), np.abs(c.pc1).max(initial=0)) < 128
    for d, i in ((c.d_a, c.i_a), (c.d_b, c.i_b)):
        if len(d) >= 8:
            assert (d == c.t2).any() and (d == np.nextafter(c.t2, np.float32(np.inf))).any() and np.isinf(d).any() and np.isnan(d).any()
            assert (i[~np.isfinite(d)] == -1).all() and (i[np.isfinite(d)] >= 0).all()
    ref = _cham(c, np.float64)
    if n0 and n1:
        assert 0 < ref["kept_a"] < n0 or n0 == 1
        assert ref["kept_a"] == int((c.d_a <= c.t2).sum()) and ref["loss"] > 0
    else:
        assert ref["loss"] == 0.0 and not ref["grad"].any()
    if n1 > mo.FAN_IN:
        g = ref["grad"][mo.FAN_ROW]
        assert (c.i_b[:mo.FAN_IN] == mo.FAN_ROW).all() and (c.d_b[:mo.FAN_IN] <= c.t2).all()
        assert g[0] < 0 and g[1] == 0.0 and g[2] > 0
        q = _cham(c)["grad"][mo.FAN_ROW]
        assert q[0] < 0 and q[1] == 0.0 and q[2] > 0
    good, bad = _passes(mo.chamfer_checks(c, _cham(c)))
    assert good, bad


def test_nsfp_cases_keep_their_promises_and_the_twin_passes():
    for n0, n1 in mo.NSFP_CASES:
        c = mo.nsfp_case(n0, n1)
        ref = mo.nsfp_objective(c)
        assert c.out[:n0, :3].all() and not c.out[n0:].any() and not c.out[:, 3].any() and np.array_equal(ref["moved"], c.moved)
        assert ref["cp"].sum() == n0 and len(ref["lp"]) == no.padded_rows(n0) // 64 + (n1 + 255) // 256
        if n0 == 1:
            assert ref["cp"][:4].tolist() == [1, 0, 0, 0]
        if n1 and n0 >= 63:
            assert (ref["d_a"] == 0.25).any() and (ref["d_a"] == 0.3125).any()      # AT trunc^2 (kept) and the next lattice distance
        if n1 == 0:
            assert not ref["dout"].any() and not ref["lp"].any()
        t = mo.nsfp_objective(c, np.float32)
        good, bad = _passes(mo.nsfp_checks(c, dict(dout=t["dout"], lp=t["lp"])))
        assert good, bad


def test_keep_best_restatement_is_the_stop_rule():
    from himo_amd.nsfp import stop_rule
    for losses, patience, min_delta in mo.KEEP_SCRIPTS:
        run = mo.keep_best_run(losses, patience, min_delta)
        for t in range(1, len(losses) + 1):
            st = run[t - 1][0]
            assert (int(st[1]), int(st[3])) == stop_rule(losses[:t], patience, min_delta), (losses, t)
    a = mo.keep_best_run(*mo.KEEP_SCRIPTS[0])
    assert [imp for _, imp in a] == [True, True, False, False, False, False, False] and a[4][0] == (3.0, 2.0, 3.0, 5.0) == a[6][0]
    b = mo.keep_best_run(*mo.KEEP_SCRIPTS[1])
    assert [imp for _, imp in b] == [True, False, True, False, False, True, False, False, False] and b[-1][0][3] == 0.0
    assert mo.keep_best_run(*mo.KEEP_SCRIPTS[2])[-1][0] == (1.0, 1.0, 1.0, 2.0)
    assert any(math.isnan(v) for s in mo.KEEP_SCRIPTS for v in s[0])


# ---- each wrong twin is caught ------------------------------------------------------------------------------------------------
WRONG = ("drop_hm", "swap_tile_rows", "bias_half", "reduce_skip", "cham_lt", "scatter_last", "no_wb", "keep_le")


@pytest.mark.parametrize("variant", WRONG)
def test_wrong_twins_miss_a_check(variant):
    if variant in ("drop_hm", "swap_tile_rows", "bias_half"):
        case = mo.mlp_case(63, 2, True)
        good, bad = _passes(mo.mlpfused_checks(case, mo.twin(case)))
        assert good, bad
        good, bad = _passes(mo.mlpfused_checks(case, mo.twin(case, variant)))
        expect = dict(drop_hm="mlp_backward/dZ0", swap_tile_rows="mlp_forward/H0", bias_half="mlp_bias/db")[variant]
    elif variant == "reduce_skip":
        dz = _reduce_twin(32)
        good, bad = _passes(mo.bias_reduce_checks(dz, [mo.bias_sum_f32(d, variant) for d in dz], 32))
        expect = "bias_reduce/db"
    elif variant == "cham_lt":
        c = mo.chamfer_case(255, 257)
        good, bad = _passes(mo.chamfer_checks(c, _cham(c, variant=variant)))
        expect = "chamfer/"
    elif variant == "scatter_last":
        c = mo.chamfer_case(300, 2057)
        good, bad = _passes(mo.chamfer_checks(c, _cham(c, variant=variant)))
        expect = "chamfer/grad"
    elif variant == "no_wb":
        c = mo.nsfp_case(64, 255)
        t = mo.nsfp_objective(c, np.float32, variant)
        good, bad = _passes(mo.nsfp_checks(c, dict(dout=t["dout"], lp=t["lp"])))
        expect = "nsfp_objective/"
    else:
        differs = [mo.keep_best_run(*s, variant=variant) != mo.keep_best_run(*s) for s in mo.KEEP_SCRIPTS]
        assert differs[0] and differs[1]                          # L == best - min_delta exactly, and an equal loss under min_delta 0
        return
    assert not good, f"{variant} passes every check"
    assert any(expect in rep for rep in bad), (variant, bad)
