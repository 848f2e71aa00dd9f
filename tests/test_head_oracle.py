"""The head checker itself (oracle/head_oracle.py), on CPU.  A CPU emulation of the fused head -- operands split with
conv_oracle.split_terms, the kept products only, float32 accumulation, the kernel's stages in the kernel's order -- must pass
every stage check and every propagated check of tests/test_head_conformance_gpu.py in every arithmetic, and each emulated WRONG
head must fail the check named for it, at the row counts the GPU suite uses.  This is what keeps the bounds of the GPU matrix
honest for whoever edits them.

Checks (the names the mutation table refers to):
  stage checks      gather, x, xcopy, z, r, rhx, q, hx, pre1, y1, res   (head_oracle.stage_checks, teacher-forced)
  exact checks      res0   res is exactly 0 in dropped rows
                    drop   a dropped point's flow is xyz_t - pts bitwise
                    pad    padding rows of daq / dazr are exactly 0
  propagated checks e2e_res, e2e_flow, e2e_folded (forward); daq, dazr, dhx0 (backward)

Weight scale (head_oracle.WEIGHT_SCALE): spec.init_params times 1 / 8.  Unscaled, the absolute row sums of the head's matrices
are about 12 and the worst-case bound, multiplied by them at each of the nine products of four iterations, ends at 13 - 30
times the rms of the reference res; at 1 / 4 it is 0.7 - 2.3 %, at 1 / 8 about 0.1 % (0.01 % for dhx0).  Asserted below:
propagated bound at iters = 4 at most USEFUL = 1 / 100 of the rms of the reference res and dhx0, in every arithmetic and for
the folded form.  1 / 100 is what the end-to-end mutations need: each of them moves the affected rows by a quantity of the
order of the signal itself (another row's value, another iteration's state, a missing bias of 0.05), never by less than a
tenth of its rms.

The emulation evaluates the gates as conv_common.h's device functions do, step by step in float32.  That shows what the 1 / 8
weights cost: the q stage of a correct head misses the aggregate ratio there (tanh_f's cancellation at |v| ~ 0.05), so the
stage checks take their aggregate level from the unscaled weights (head_oracle.STAGE_SCALE) and, with the 1 / 8 weights, keep
it only for pre1, a bare product.  The low-order-term mutations are therefore run with the unscaled weights.

Mutations no honest end-to-end bound can catch, and the stage check that does: a dropped bf16 term, the m m product and the
fp16 weight scale change a product by 2^-16 .. 2^-18 relative, below the propagated worst case of four iterations -- they
are caught by the aggregate (rms) level of the stage checks q and pre1 (not z and r: a gate near 1 / 2 behind a slope of 1 / 4
rounds to 2^-25 itself, which hides a 2^-17 relative change of its small pre-activation).  r (1 - r) against z (1 - z) in dazr
differs by parts in a thousand with gates near 1 / 2: caught at dazr, below the propagated bound at dhx0.  The backward kernel takes no pid, so a dropped point
treated as cell 0 cannot show in dhx0 of himo_gru_head_backward; it shows in gather, res0 and drop.
"""
import numpy as np
import pytest
import torch

import conv_oracle as co
import head_oracle as ho

H = ho.HIDDEN
USEFUL = 1.0 / 100.0
N_FWD, N_BWD = 129, 97           # three forward blocks, the last with one row; four backward blocks, the last with one row
_CACHE = {}


def _weights(scale=ho.WEIGHT_SCALE):
    """1 / 8 (the default): the end-to-end checks and the bound level of the stage checks; ho.STAGE_SCALE: both levels of the
    stage checks (head_oracle.STAGE_SCALE says why)"""
    if ("w", scale) not in _CACHE:
        w = ho.weights(0, scale)
        w["scale"] = scale
        _CACHE[("w", scale)] = w
    return _CACHE[("w", scale)]


# conv_common.h's device functions step by step in float32, the exponential and the reciprocal correctly rounded (the best the
# hardware instructions could do): sigmoid_f = rcp(1 + exp(-v)), tanh_f = copysign((1 - e) rcp(1 + e), v), e = exp(-2 |v|)
_F = np.float32


def sigmoid_f(v):
    v = v.numpy().astype(_F)
    e = np.exp((-v).astype(np.float64)).astype(_F)
    return torch.from_numpy((_F(1) / (_F(1) + e)).astype(_F))


def tanh_f(v):
    v = v.numpy().astype(_F)
    e = np.exp((_F(-2) * np.abs(v)).astype(np.float64)).astype(_F)
    t = ((_F(1) - e) * (_F(1) / (_F(1) + e)).astype(_F)).astype(_F)
    return torch.from_numpy(np.copysign(t, v))


def _scene(n=N_FWD):
    if ("sc", n) not in _CACHE:
        _CACHE[("sc", n)] = ho.scene(n, n)
    return _CACHE[("sc", n)]


# ---- the emulation ---------------------------------------------------------------------------------------------------
def emul_gemm(arith, a, w, mut=None):
    """a [n, K] x w [K, cout] as gemm192 / hb_gemm do it: the split terms, the kept products, float32 sums"""
    a = a.float().contiguous()
    if mut == "halves":                                   # the 16-byte halves of rows 16..31 of each 32-row tile not swapped
        k = torch.arange(a.shape[1]) ^ 8
        odd = ((torch.arange(a.shape[0]) >> 4) & 1).bool()
        a = torch.where(odd[:, None], a[:, k], a)
    if arith == "f32":
        return a @ w.float()
    kept = list(co.KEPT[arith])
    if mut == "drop_l":
        kept = [p for p in kept if 2 not in p]
    if mut == "drop_mm":
        kept = [p for p in kept if p != (1, 1)]
    ta = co.split_terms(arith, a.numpy())
    tw = co.split_terms(arith, w.float().numpy(), weights=mut != "no_wscale")
    acc = None
    for i, j in kept:
        p = torch.from_numpy(ta[i]) @ torch.from_numpy(tw[j])
        acc = p if acc is None else acc + p
    return acc


def _fma_chain(cols, weights, bias):
    """s = c0 w0; s = fma(c_k, w_k, s) ...; s + b, every step rounded to float32 (float64 products of float32 are exact)"""
    s = (cols[0].double() * weights[0].double()).float()
    for c, w in zip(cols[1:], weights[1:]):
        s = (c.double() * w.double() + s.double()).float()
    return s + bias


def _gelu32(t):
    return (0.5 * t.double() * (1.0 + torch.erf(t.double() / np.sqrt(2.0)))).float()


def emulate(arith, sc, W, iters, mut=None, folded=False, w2=None, w2_pitch=3):
    """the fused head (gruhead.hip) on the CPU -> every save of himo_gru_head_train and the flow of the inference kernels"""
    n = sc["n"]
    pid = sc["pid"].clone()
    if mut == "drop_cell0":
        pid = pid.clamp(min=0)
    live = (pid >= 0)[:, None]
    c = pid.long().clamp(min=0)
    h = torch.where(live, torch.cat([sc["img0"][c], sc["img1"][c], sc["dec"][c]], 1), torch.zeros(n, H))
    if mut == "tail_last" and n % 64 > 1:                # a live row of the partial block reads point n - 1's cell
        cl = pid.long()[n - 1]
        row = [i for i in range(n - n % 64, n - 1) if pid[i] >= 0 and pid[i] != cl][0]
        h[row] = torch.cat([sc["img0"][cl], sc["img1"][cl], sc["dec"][cl]])
    if arith == "f16x2":
        h = torch.cat([ho.f16_two_term(h[:, :64]), h[:, 64:]], 1)
    o = sc["offsets"]
    if folded:
        x = torch.cat([o, torch.ones(n, 1), torch.zeros(n, 12)], 1)
        mats = {}
        for k in ("wzr", "wq", "w1"):
            f = ho.fold(W["w_off"], W["b_off"], W[k])
            if mut == "fold_no_131":
                f[H + 3] = 0
            mats[k] = f.float()
    else:
        x = _fma_chain([o[:, k:k + 1] for k in range(3)], [W["w_off"][k][None] for k in range(3)], 0 if mut == "no_b_off" else W["b_off"][None])
        mats = {k: W[k] for k in ("wzr", "wq", "w1")}
    T = iters + (mut == "iters+1") - (mut == "iters-1")
    sv = dict(hx=[torch.cat([h, x], 1)], rhx=[], z=[], r=[], q=[])
    gm = mut if mut in ("halves", "drop_l", "drop_mm", "no_wscale") else None
    bzr = W["bzr"].clone()
    if mut == "no_bz":
        bzr[:H] = 0
    if mut == "no_br":
        bzr[H:] = 0
    for t in range(T):
        g = sigmoid_f(emul_gemm(arith, torch.cat([h, x], 1), mats["wzr"], gm) + bzr)
        z, r = g[:, :H], g[:, H:]
        rh = h if mut == "rh_is_h" else r * h
        q = tanh_f(emul_gemm(arith, torch.cat([rh, x], 1), mats["wq"], gm) + (0 if mut == "no_bq" else W["bq"]))
        hn = z * h + (1.0 - z) * q if mut == "blend_swapped" else (1.0 - z) * h + z * q
        if mut == "swap_rows" and t == 0:                # accumulator element r = 5 of row tile 0: rows 9 (lh 0) and 13 (lh 1)
            hn[[9, 13]] = hn[[13, 9]]
        h = hn
        sv["z"].append(z); sv["r"].append(r); sv["q"].append(q); sv["rhx"].append(torch.cat([rh, x], 1)); sv["hx"].append(torch.cat([h, x], 1))
    if mut == "rhx_x_unsaved":                           # the copy loop of the x columns one iteration short (gruhead.hip:212)
        sv["rhx"][-1][:, H:] = 0
    pre1 = emul_gemm(arith, torch.cat([h, x], 1), mats["w1"], gm) + (0 if mut == "no_b1" else W["b1"])
    y1 = _gelu32(pre1)
    if mut == "gelu_quick":                              # x sigmoid(1.702 x) for the erf form
        y1 = pre1 * torch.sigmoid(1.702 * pre1)
    w2 = W["w2"] if w2 is None else w2                   # [32][w2_pitch'] as stored; read with ``w2_pitch``
    flat = torch.cat([w2.reshape(-1), torch.zeros(64)])     # (what lies behind a pitch-3 matrix read with pitch 4)
    w2r = torch.stack([flat[k * w2_pitch:k * w2_pitch + 3] for k in range(32)])
    res = _fma_chain([y1[:, k:k + 1] for k in range(32)], [w2r[k][None] for k in range(32)], W["b2"][None])
    res = torch.where(live, res, torch.zeros(n, 3))
    pf = sc["xyz_t"] - sc["pts"]
    sv.update(pre1=pre1, y1=y1, res=res, flow=torch.where(live, pf + res, pf))
    return sv


def emulate_backward(arith, dhx_last, sv, W, iters, mut=None):
    """gruheadbwd.hip on the CPU, float32"""
    g, dx = dhx_last[:, :H].clone(), dhx_last[:, H:].clone()
    wq_t, wzr_t = W["wq"].T.contiguous(), W["wzr"].T.contiguous()
    daq_s, dazr_s = [None] * iters, [None] * iters
    for t in range(iters - 1, -1, -1):
        z, r, q, h = sv["z"][t], sv["r"][t], sv["q"][t], sv["hx"][t][:, :H]
        daq = g * (1.0 if mut == "daq_no_z" else z) * (1.0 - q * q)
        dazz = (g * (q - h)) * z * (1.0 - z)
        dhp = g * (1.0 - z)
        if mut == "x_halves":                             # only the first K half of the x columns' products
            d_rhx = torch.cat([emul_gemm(arith, daq, wq_t[:, :H]), emul_gemm(arith, daq[:, :64], wq_t[:64, H:])], 1)
        else:
            d_rhx = emul_gemm(arith, daq, wq_t)
        drh = d_rhx[:, :H]
        dhp = dhp + drh * r
        gate = z * (1.0 - z) if mut == "dazr_z" else r * (1.0 - r)
        dazr = torch.cat([dazz, (drh * h) * gate], 1)
        if mut == "x_halves":
            d_hx = torch.cat([emul_gemm(arith, dazr, wzr_t[:, :H]), emul_gemm(arith, dazr[:, :H], wzr_t[:H, H:])], 1)
        else:
            d_hx = emul_gemm(arith, dazr, wzr_t)
        g = dhp + d_hx[:, :H]
        dx = dx + d_rhx[:, H:] + d_hx[:, H:]
        daq_s[t], dazr_s[t] = daq, dazr
    return torch.stack(daq_s), torch.stack(dazr_s), torch.cat([g, dx], 1)


# ---- the checks, by name ------------------------------------------------------------------------------------------------
def failed_checks(arith, sc, W, sv, iters, folded=False):
    """names of the forward checks ``sv`` (an emulation's saves and flow) fails"""
    bad = set()
    agg = W["scale"] == ho.STAGE_SCALE                    # the aggregate level of the stage checks: the network's weights only
    if not folded:
        for name, got, ref, bnd, r32 in ho.stage_checks(arith, sc, W, sv, len(sv["z"])):
            if not ho.verdict(arith, got, ref, bnd, r32, name, aggregate=agg or name in ho.BARE_STAGES)[0]:
                bad.add(name)
    key = ("prop", arith, sc["n"], iters, folded, W["scale"])
    if key not in _CACHE:
        _CACHE[key] = ho.propagate_forward(arith, sc, W, iters, folded)
    p = _CACHE[key]
    dropped = sc["pid"] < 0
    if not folded:
        if not ho.verdict(arith, sv["res"], p["res"], p["e_res"], None, "e2e_res")[0]:
            bad.add("e2e_res")
        if bool((sv["res"][dropped] != 0).any()):
            bad.add("res0")
    if not ho.verdict(arith, sv["flow"], p["flow"], p["e_flow"], None, "e2e_flow")[0]:
        bad.add("e2e_folded" if folded else "e2e_flow")
    if not torch.equal(sv["flow"][dropped], (sc["xyz_t"] - sc["pts"])[dropped]):
        bad.add("drop")
    return bad


def _bwd_inputs(n, iters, W):
    key = ("bwd", n, iters)
    if key not in _CACHE:
        sc = _scene(n)
        ref = ho.forward(sc, W, iters)
        sv = {k: [a.float() for a in ref[k]] for k in ("hx", "z", "r", "q")}
        d = torch.randn(n, ho.HX, generator=torch.Generator().manual_seed(n))
        d[sc["pid"] < 0] = 0
        _CACHE[key] = (sv, d)
    return _CACHE[key]


def failed_bwd_checks(arith, n, iters, W, got):
    sv, d = _bwd_inputs(n, iters, W)
    key = ("bprop", arith, n, iters)
    if key not in _CACHE:
        _CACHE[key] = ho.propagate_backward(arith, d, sv, W, iters)
    p = _CACHE[key]
    tw = ho.backward(d, sv, W, iters, torch.float32)
    bad = set()
    for name, g, t32 in zip(("daq", "dazr", "dhx0"), got, tw):
        if not ho.verdict(arith, g, p[name], p["e_" + name], t32, name)[0]:
            bad.add(name)
    return bad


# ---- (a) correct emulations pass ------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("n", [1, 65, N_FWD])
def test_correct_forward_emulation_passes_every_check(arith, n):
    sc = _scene(n)
    for W in (_weights(), _weights(ho.STAGE_SCALE)):
        for iters in (1, 4):
            assert failed_checks(arith, sc, W, emulate(arith, sc, W, iters), iters) == set(), (arith, n, iters, W["scale"])
    W = _weights()
    if arith != "f32":
        for iters in (0, 4, 6):
            assert failed_checks(arith, sc, W, emulate(arith, sc, W, iters, folded=True), iters, folded=True) == set(), (arith, n, iters)


def test_w2_pitch_4_is_the_same_matrix():
    W, sc = _weights(), _scene(65)
    w4 = torch.zeros(32, 4)
    w4[:, :3] = W["w2"]
    assert failed_checks("bf16x3", sc, W, emulate("bf16x3", sc, W, 2, w2=w4, w2_pitch=4), 2) == set()


@pytest.mark.parametrize("arith", ["f32", "bf16x3", "bf16x2"])
@pytest.mark.parametrize("n", [1, 33, N_BWD])
def test_correct_backward_emulation_passes_every_check(arith, n):
    W = _weights()
    for iters in (1, 4):
        sv, d = _bwd_inputs(n, iters, W)
        assert failed_bwd_checks(arith, n, iters, W, emulate_backward(arith, d, sv, W, iters)) == set(), (arith, n, iters)


# ---- (b) mutations fail the checks named for them ---------------------------------------------------------------------
# mutation -> (arithmetic, checks that must fail); a star: with the network's weights (ho.STAGE_SCALE), where the stage checks
# have their aggregate level -- the only level a lost low-order term shows at
FORWARD_MUTATIONS = {
    "drop_l": ("bf16x3*", {"q", "pre1"}), "drop_mm": ("bf16x3*", {"q", "pre1"}), "no_wscale": ("f16x2", {"pre1"}),
    "swap_rows": ("bf16x3", {"hx", "e2e_res", "e2e_flow"}), "halves": ("bf16x3", {"z", "q", "pre1", "e2e_res", "e2e_flow"}),
    "drop_cell0": ("bf16x3", {"gather", "res0", "drop"}),
    "no_bz": ("bf16x3", {"z"}), "no_br": ("bf16x3", {"r", "rhx"}), "no_bq": ("bf16x3", {"q", "hx"}),
    "rh_is_h": ("bf16x3", {"rhx", "e2e_res"}), "iters+1": ("bf16x3", {"e2e_res", "e2e_flow"}), "iters-1": ("bf16x3", {"e2e_res", "e2e_flow"}),
    "no_b1": ("f16x2", {"pre1", "y1", "e2e_res"}), "gelu_quick": ("f16x2", {"y1"}), "no_b_off": ("bf16x3", {"x"}), "rhx_x_unsaved": ("bf16x3", {"xcopy"}), "blend_swapped": ("f16x2", {"hx", "e2e_res"}),
}


@pytest.mark.parametrize("mut", sorted(FORWARD_MUTATIONS))
def test_forward_mutation_is_caught(mut):
    arith, must = FORWARD_MUTATIONS[mut]
    W, sc = _weights(ho.STAGE_SCALE if arith.endswith("*") else ho.WEIGHT_SCALE), _scene(N_FWD)
    arith = arith.rstrip("*")
    bad = failed_checks(arith, sc, W, emulate(arith, sc, W, 4, mut), 4)
    assert must <= bad, f"{mut}: expected {sorted(must)} to fail, failed: {sorted(bad)}"
    print(f"{mut} [{arith}]: caught by {sorted(bad)}")


def test_partial_block_reading_the_last_point_is_caught():
    W, sc = _weights(), _scene(127)
    bad = failed_checks("bf16x3", sc, W, emulate("bf16x3", sc, W, 4, "tail_last"), 4)
    assert {"gather", "e2e_res", "e2e_flow"} <= bad, sorted(bad)


def test_wrong_w2_pitch_is_caught_either_way():
    W, sc = _weights(), _scene(N_FWD)
    w4 = torch.zeros(32, 4)
    w4[:, :3] = W["w2"]
    for w2, pitch in ((w4, 3), (W["w2"], 4)):
        bad = failed_checks("bf16x3", sc, W, emulate("bf16x3", sc, W, 2, w2=w2, w2_pitch=pitch), 2)
        assert {"res", "e2e_res"} <= bad, (pitch, sorted(bad))


def test_folded_row_131_omitted_is_caught():
    W, sc = _weights(), _scene(N_FWD)
    bad = failed_checks("bf16x3", sc, W, emulate("bf16x3", sc, W, 4, "fold_no_131", folded=True), 4, folded=True)
    assert "e2e_folded" in bad, sorted(bad)


def test_sample_boundary_off_by_one_block_is_caught():
    """`bid > block_start[smp + 1]` for `>=`: the second sample's first block stays with the first sample (whose rows past n it
    does not write), so rows 0..63 of the second sample's flow keep what the buffer held -- here the guard's NaN"""
    W, sc = _weights(), _scene(N_FWD)
    sv = emulate("bf16x3", sc, W, 4)
    sv["flow"][:64] = float("nan")
    assert "e2e_flow" in failed_checks("bf16x3", sc, W, sv, 4)


BACKWARD_MUTATIONS = {"x_halves": {"dhx0"}, "dazr_z": {"dazr"}, "daq_no_z": {"daq", "dhx0"}}


@pytest.mark.parametrize("arith", ["bf16x3", "bf16x2"])
@pytest.mark.parametrize("mut", sorted(BACKWARD_MUTATIONS))
def test_backward_mutation_is_caught(arith, mut):
    W = _weights()
    sv, d = _bwd_inputs(N_BWD, 4, W)
    bad = failed_bwd_checks(arith, N_BWD, 4, W, emulate_backward(arith, d, sv, W, 4, mut))
    assert BACKWARD_MUTATIONS[mut] <= bad, f"{mut}: expected {sorted(BACKWARD_MUTATIONS[mut])} to fail, failed: {sorted(bad)}"


def pad_rows_zero(t, n):
    """the ``pad`` check of the GPU suite: rows [n, ceil64(n)) of a [iters, rows, C] gate gradient are exactly zero"""
    return not bool((t[:, n:(n + 63) // 64 * 64] != 0).any())


def test_nonzero_padding_row_is_caught():
    W = _weights()
    sv, d = _bwd_inputs(N_BWD, 2, W)
    daq, dazr, _ = emulate_backward("bf16x3", d, sv, W, 2)
    rows = (N_BWD + 63) // 64 * 64
    pad = lambda a: torch.cat([a, torch.zeros(a.shape[0], rows - N_BWD, a.shape[2])], 1)
    good = pad(daq)
    assert pad_rows_zero(good, N_BWD) and pad_rows_zero(pad(dazr), N_BWD)
    good[1, N_BWD] = 1e-30                                # one padding row written with the unmasked product
    assert not pad_rows_zero(good, N_BWD)


def test_small_weights_leave_the_aggregate_level_to_tanh():
    """why the stage checks take their aggregate level from the network's weights: a CORRECT head (tanh_f step by step, its
    exponential and reciprocal correctly rounded) misses conv_oracle.R["bf16x3"] = 2 at the q stage with the 1 / 8 weights --
    the cancellation in 1 - e -- and stays far inside it with the weights unscaled"""
    sc = _scene(N_FWD)
    ratio = {}
    for scale in (ho.WEIGHT_SCALE, ho.STAGE_SCALE):
        W = _weights(scale)
        sv = emulate("bf16x3", sc, W, 4)
        ratio[scale] = max(ho.verdict("bf16x3", g, r, b, r32, n)[2] for n, g, r, b, r32 in ho.stage_checks("bf16x3", sc, W, sv, 4) if n == "q")
    print(f"q stage rms ratio: {ratio}")
    assert ratio[ho.WEIGHT_SCALE] > co.R["bf16x3"] > 2 * ratio[ho.STAGE_SCALE], ratio


# ---- (c) the bounds are useful ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
def test_forward_bound_is_useful(arith):
    W, sc = _weights(), _scene(200)
    for folded in (False, True):
        p = ho.propagate_forward(arith, sc, W, 4, folded)
        live = sc["pid"] >= 0
        ratio = co.rms(p["e_res"][live]) / co.rms(p["res"][live])
        print(f"forward {arith} folded={folded}: rms bound / rms res = {ratio:.3g}, max bound {float(p['e_res'].max()):.3g}")
        assert ratio <= USEFUL, (arith, folded, ratio)
        assert float(p["e_res"].max()) <= USEFUL * co.rms(p["res"][live]) * 10, "a single element's bound is no larger than a tenth of the signal"


@pytest.mark.parametrize("arith", ["bf16x3", "bf16x2"])
def test_backward_bound_is_useful(arith):
    W = _weights()
    sv, d = _bwd_inputs(N_BWD, 4, W)
    p = ho.propagate_backward(arith, d, sv, W, 4)
    ratio = co.rms(p["e_dhx0"]) / co.rms(p["dhx0"])
    print(f"backward {arith}: rms bound / rms dhx0 = {ratio:.3g}")
    assert ratio <= USEFUL, (arith, ratio)
