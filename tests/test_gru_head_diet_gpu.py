"""The folded fp16 inference head, gru_head_kernel<2, 9, false> (csrc/gruhead.hip), after its instruction diet: the offset slab as one
matrix instruction (HIMO_HEAD_PACKED_SLAB), the gates' exponent arguments formed by one fused multiply-add on the unscaled accumulator
(HIMO_HEAD_GATE_FMA) and tanh as 1 - 2 / (1 + exp2(y)) (HIMO_HEAD_TANH_DIRECT).

Every case compares himo_gru_head_batch_folded with the float64 evaluation of spec.py steps 5-6 (oracle/head_oracle.py ``forward``) on the
same inputs, at the bar of the head's pin test tests/test_head_conformance_gpu.py: head_oracle.propagate_forward's per-element bound for
the f16x2 arithmetic with folded weights, judged by head_oracle.verdict.  Nothing is loosened; its helpers are imported from that module.

Cases are the smallest at which this code can go wrong: n around the 64-row block (1, 63, 64, 65, 129: partial last block, second
block), one sample and three unequal samples in one launch, iters 0 / 1 / 4, dropped rows (head_oracle.scene: pid = -1 in about 10 % of
the rows, among them block edges), offsets at +- half a voxel and 0 (lo(o) non-zero and zero), offset weights scaled so that the low
halves of the packed folded rows are normal, subnormal in fp16 and zero, gate pre-activations driven to +-30, +-88 and +-1e4 by the
biases (no NaN or inf, the gates saturate to the float64 values), and a bit-for-bit comparison of the packed slab with the three-term
slabs of the unfolded kernel where every partial sum is exact.
"""
import numpy as np
import pytest
import torch

import head_oracle as ho
import test_head_conformance_gpu as hc

pytestmark = pytest.mark.gpu

FMT, ARITH = 1, "f16x2"
HALF_VOXEL = torch.tensor([0.1, 0.1, 3.0])               # head_oracle.scene: offsets within a 0.2 x 0.2 x 6 m pillar


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import model, train                 # noqa: F401  (registers the signatures)
    return _lib.load()


class DevWeights(hc.Weights):
    """hc.Weights for a given weight set (its constructor takes head_oracle.weights(0, scale))"""

    def __init__(self, lib, gpu, W):
        self.W, self.scale = W, None
        self.g = {k: hc.gvec(gpu, W[k]) for k in ("w_off", "b_off", "bzr", "bq", "b1", "b2")}
        self.g["w2"] = hc.g2(gpu, W["w2"])
        self.pk = {FMT: {k: hc._pack(lib, gpu, W[k], FMT) for k in ("wzr", "wq", "w1")}}
        self.pkf = {FMT: {k: hc._pack(lib, gpu, ho.fold(W["w_off"], W["b_off"], W[k]).float(), FMT) for k in ("wzr", "wq", "w1")}}
        self.pkt = {}


def _scene(n, seed=0):
    """head_oracle.scene with the first live rows' offsets at +half a voxel, -half a voxel and 0; seed 0 keeps the scene's pose flow"""
    sc = ho.scene(1000 + 7 * seed + n, n)
    live = torch.nonzero(sc["pid"] >= 0).reshape(-1)
    for j, f in zip(live[:3].tolist(), (1.0, -1.0, 0.0)):
        sc["offsets"][j] = f * HALF_VOXEL
    if seed:                                             # no pose flow: the flow IS the head's residual, and the bound the head's alone
        sc["xyz_t"] = sc["pts"].clone()                  # (at 30 m the rounding of xyz_t - pts + res is most of the bound)
    return sc


def _run(lib, gpu, wts, scenes, iters, entry="folded"):
    ds = [hc.DevScene(gpu, sc, hc.LAYOUTS[1]) for sc in scenes]
    c = hc.Call([g for d in ds for g in d.inputs] + wts.guarded(), [d.flow for d in ds], wts.plain())
    assert hc._infer_call(lib, wts, entry, ds, FMT, iters) == 0
    c.check(f"{entry} n={[sc['n'] for sc in scenes]} iters={iters}")
    return [d.flow.get().reshape(sc["n"], 3) for d, sc in zip(ds, scenes)]


def _check(flow, sc, W, iters, case):
    assert bool(torch.isfinite(flow).all()), f"{case}: NaN or inf in the flow"
    p = ho.propagate_forward(ARITH, sc, W, iters, folded=True)
    good, worst, rr, report = ho.verdict(ARITH, flow, p["flow"], p["e_flow"], None, case)
    print(f"{case}: err/bound {worst:.3g}, max |err| {float((flow.double() - p['flow']).abs().max()):.3g}")
    assert good, report
    dropped = sc["pid"] < 0
    assert torch.equal(flow[dropped], (sc["xyz_t"] - sc["pts"])[dropped]), f"{case}: a dropped point's flow is not xyz_t - pts bitwise"


@pytest.fixture(scope="module")
def wts(lib, gpu):
    return DevWeights(lib, gpu, ho.weights(0, ho.WEIGHT_SCALE))


@pytest.mark.parametrize("iters", [0, 1, 4])
def test_rows_around_the_block_one_sample(lib, gpu, wts, iters):
    for n in (1, 63, 64, 65, 129):
        sc = _scene(n)
        flow, = _run(lib, gpu, wts, [sc], iters)
        _check(flow, sc, wts.W, iters, f"one sample n={n} iters={iters}")


@pytest.mark.parametrize("iters", [0, 1, 4])
def test_three_unequal_samples_in_one_launch(lib, gpu, wts, iters):
    scenes = [_scene(n, seed=1) for n in (65, 1, 129)]
    for flow, sc in zip(_run(lib, gpu, wts, scenes, iters), scenes):
        _check(flow, sc, wts.W, iters, f"three samples n={sc['n']} iters={iters}")


@pytest.mark.parametrize("off_scale", [1.0, 2.0 ** -7, 0.0])
def test_offset_weight_scales(lib, gpu, off_scale):
    """the folded rows F = [W_off W_x ; b_off W_x] are packed as hi / lo of 64 F: at scale 1 lo(64 F) is a normal fp16 number for
    most entries, at 2^-7 it lies below 2^-14 (subnormal), at 0 the rows and their low halves are zero"""
    W = ho.weights(0, ho.WEIGHT_SCALE)
    W["w_off"], W["b_off"] = W["w_off"] * off_scale, W["b_off"] * off_scale
    for k in ("wzr", "wq", "w1"):
        lo = ho.split_terms(ARITH, ho.fold(W["w_off"], W["b_off"], W[k]).float().numpy()[ho.HIDDEN:ho.HIDDEN + 4], weights=True)[1]
        lo = np.abs(lo.astype(np.float64)) * 64.0                  # split_terms returns the packed halves divided by the packing scale
        if off_scale == 1.0:
            assert (lo >= 2.0 ** -14).any()
        elif off_scale == 0.0:
            assert not lo.any()
        else:
            assert lo.any() and (lo < 2.0 ** -14).all()
    wts = DevWeights(lib, gpu, W)
    sc = _scene(65, seed=2)
    flow, = _run(lib, gpu, wts, [sc], 4)
    _check(flow, sc, W, 4, f"offset weights x{off_scale:g}")


@pytest.mark.parametrize("level", [30.0, 88.0, 1e4])
def test_saturated_gates(lib, gpu, level):
    """biases of +-level, the sign alternating over the columns (z and r in step, q a column out of step): every gate of every
    iteration is driven to one of its ends, both ends in every launch.  exp2's argument overflows to +-inf from 88 on; the gates must
    come out 0 / 1 / +-1, never NaN"""
    W = ho.weights(0, ho.WEIGHT_SCALE)
    sign = torch.where(torch.arange(256) % 2 == 0, 1.0, -1.0)
    W["bzr"] = (level * sign).float()
    W["bq"] = (-level * sign[:128]).float()
    W["bq"][64:] *= -1.0
    wts = DevWeights(lib, gpu, W)
    for n, iters in ((65, 4), (63, 1)):
        sc = _scene(n, seed=3)
        flow, = _run(lib, gpu, wts, [sc], iters)
        _check(flow, sc, W, iters, f"gates at +-{level:g} n={n} iters={iters}")


def _exact_problem(n):
    """Weights and a scene on which the decoder's first product is exact in both kernels (iters = 0: gather, dec1, GELU, dec2): small
    integers times powers of two, every product and every partial sum of the x64-scaled accumulation a multiple of 2^-7 below 2^13.
      w1's x rows pick x_j (weight 1) and 2^-11 x_(j+32): F_k,j = w_off[k][j] + 2^-11 w_off[k][j+32], so 64 F has a non-zero low half in
      rows 1..3 (hi lo products) and none in row 0, where w_off[0][32:] = 0; o0 = 2 + m 2^-11 has a non-zero low half (lo hi products),
      o1 and o2 are quarters.  The dropped lo lo products are zero on both sides: lo(o0) meets lo(64 F_0) = 0, lo(x) meets lo(64 w1) = 0."""
    g = torch.Generator().manual_seed(77 + n)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    W = ho.weights(0, ho.WEIGHT_SCALE)
    W["w_off"] = ri(-7, 7, 3, 64)
    W["w_off"][0] = ri(-1, 1, 64) * 7.0
    W["w_off"][0, 32:] = 0.0
    W["b_off"] = ri(-7, 7, 64)
    w1 = torch.zeros(192, 32)
    w1[:128] = ri(-3, 3, 128, 32) / 16.0
    w1[128 + torch.arange(32), torch.arange(32)] = 1.0
    w1[160 + torch.arange(32), torch.arange(32)] = 2.0 ** -11
    W["w1"] = w1
    sc = ho.scene(500 + n, n)
    sc["img0"], sc["img1"], sc["dec"] = ri(-16, 16, ho.CELLS, 32) / 8.0, ri(-16, 16, ho.CELLS, 32) / 8.0, ri(-16, 16, ho.CELLS, 64) / 8.0
    sc["offsets"] = torch.stack([2.0 + ri(0, 2047, n) * 2.0 ** -11, ri(-4, 4, n) / 4.0, ri(-4, 4, n) / 4.0], 1)
    return W, sc


def test_packed_slab_equals_the_three_term_slabs_bitwise(lib, gpu):
    """the folded kernel's packed slab (one matrix instruction) against the unfolded kernel's four x slabs of three terms each, where
    both are exact: the same pre-activation bits enter the same GELU and output code, so the flows must be bit-equal"""
    for n in (1, 65, 129):
        W, sc = _exact_problem(n)
        o, w = sc["offsets"].numpy(), W["w_off"].numpy()
        assert (ho.split_terms(ARITH, o)[1][:, 0] != 0).any() and not ho.split_terms(ARITH, o)[1][:, 1:].any()
        F = ho.fold(W["w_off"], W["b_off"], W["w1"])
        assert torch.equal(F.float().double(), F), "the folded rows are not exact in float32"
        lo = ho.split_terms(ARITH, F.float().numpy()[128:132], weights=True)[1]
        assert not lo[0].any() and lo[1:].any()
        x = (sc["offsets"].double() @ W["w_off"].double() + W["b_off"].double())
        assert torch.equal(x.float().double(), x) and np.array_equal(sum(t.astype(np.float64) for t in ho.split_terms(ARITH, x.float().numpy())), x.numpy())
        wts = DevWeights(lib, gpu, W)
        folded, = _run(lib, gpu, wts, [sc], 0, "folded")
        plain, = _run(lib, gpu, wts, [sc], 0, "batch")
        assert torch.equal(folded.view(torch.int32), plain.view(torch.int32)), f"n={n}: {int((folded != plain).sum())} flow values differ bitwise"
        _check(folded, sc, W, 0, f"exact problem n={n}")
