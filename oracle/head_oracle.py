"""Float64 reference and worst-case error model of the per-point GRU head (include/himo_amd.h: himo_gru_head,
himo_gru_head_batch, himo_gru_head_batch_folded, himo_gru_head_batch_guarded, himo_gru_head_train, himo_gru_head_backward,
himo_head_gather, himo_head_final; csrc/gruhead.hip, csrc/gruheadbwd.hip, csrc/head.hip).  CPU only.

The operation is himo_amd/seflow/spec.py steps 5-6 (compare oracle/seflow_oracle.py::head), in the widths of the header:
hidden 128 = 32 (pc0 image) + 32 (pc1 image) + 64 (decoder map) gathered channels, x = Linear(3,64)(offset), zr [192][256]
(z | r), q [192][128], dec1 [192][32], dec2 [32][3].  A weight set is a dict w_off, b_off, wzr, bzr, wq, bq, w1, b1, w2, b2
(``weights``); a scene is a dict pid, offsets, img0, img1, dec, xyz_t, pts (``scene``).  Every reference function takes
``dtype``: float64 is the reference, float32 the defined float32 twin of the aggregate level (conv_oracle.check).

Arithmetics (names, kept products and aggregate ratios of conv_oracle, taken over unchanged):
  forward   packed_format 0 = "bf16x3", 1 = "f16x2"; backward packed_format 0 = "bf16x3", 2 = "bf16x2".
  gemm192 (gruhead.hip:98-148): the A operand [h | x] is split value by value in a_store (gruhead.hip:84-94: split3 for
      three bf16 planes, split2 for two fp16 planes), the weights arrive packed (himo_conv_pack_weights_ex).  Kept products,
      as (term of A, term of W):
          FMT 3  gruhead.hip:128  HIMO_TERM(2,0) (0,2) (1,1) (1,0) (0,1) (0,0)   = conv_oracle.KEPT["bf16x3"]
          FMT 2  gruhead.hip:130  HIMO_TERM16(1,0) (0,1) (0,0)                   = conv_oracle.KEPT["f16x2"]
      all into one float32 accumulator per output; FMT 2 multiplies the accumulator by kF16AccScale = 2^-6
      (gruhead.hip:139-147; exact), undoing the 2^6 the weights were packed with (bf16x3.h:43).
  hb_gemm (gruheadbwd.hip:55-78): A = the gate gradients, split in hb_store (gruheadbwd.hip:42-52: split3, or h = RNE bf16,
      m = RNE bf16 of x - h).  Kept: NP 3 gruheadbwd.hip:72 = KEPT["bf16x3"]; NP 2 gruheadbwd.hip:73 (1,0) (0,1) (0,0) =
      KEPT["bf16x2"].
  The gates use conv_common.h's device functions -- sigmoid_f (conv_common.h:92, gruhead.hip:316-317), tanh_f
  (conv_common.h:93-97, gruhead.hip:340), gelu_exact (conv_common.h:67-77, gruhead.hip:368) -- the ones the convolution
  epilogues use, so conv_oracle.bound's budgets for them apply unchanged.

Stage bounds (``stage_checks``; teacher-forced).  himo_gru_head_train saves every stage.  A stage is one row product with an
epilogue whose operands are the kernel's OWN previous saves, so its bound is conv_oracle.bound / operand_bound of a 1x1
layer: z, r, r h from hx[t] (HIMO_EPI_GRU_ZR), q and h' from rhx[t], z[t], hx[t] (HIMO_EPI_GRU_Q), pre1 / y1 from
hx[iters] (HIMO_EPI_BIAS_GELU).  r and q themselves are not outputs of a convolution epilogue; their bounds are the
intermediate terms of conv_oracle.bound (bg, bq there) restated below.  Counted from the code:
  gather   bit copies (gruhead.hip:261-265, head.hip:35); FMT 2: the image columns are the two-term fp16 value
           (gruhead.hip:256, 266-276), the decoder columns bit copies.
  x        fmaf(o2, w2, fmaf(o1, w1, o0 * w0)) + b (gruhead.hip:208, 223; head.hip:44): one product, two fused steps, one
           sum = 4 roundings: gamma(4) (|o| |w_off| + |b_off|), gamma(k) = k u / (1 - k u).
  dec2     s = y0 w0; 31 x s = fmaf(y_k, w_k, s); s + b2 (gruhead.hip:384-387, 402-405; head.hip:69-72): 33 roundings:
           gamma(33) (|y1| |w2| + |b2|).
  flow     pose_flow = xyz_t - pts (one rounding), out = pose_flow + (s + b2) (one more): 2 u on either.
  the x columns of every saved hx[t] / rhx[t] are copies of one value (gruhead.hip:210-212): bit-equal to hx[0]'s.

Propagated bounds (``propagate_forward``, ``propagate_backward``).  The inference kernels save nothing, the backward saves
no dh_t, the folded weights are float32 roundings of the folded rows.  A per-element bound e on |kernel - reference| is
carried with the float64 reference:
  through a product:  e |W|  +  the product's own error for an operand of magnitude at most |a| + e (``gemm_mag_bound``: the
      terms of operand_bound with the operand's split taken at its worst case -- bf16: u_b = 2^-9 per term, so
      |h| <= (1 + u_b) |a|, |m| <= (1 + u_b) u_b |a|, |l| <= (1 + u_b) u_b^2 |a|, residual u_b^3 |a| (three terms) or u_b^2 |a|
      (two); fp16: u_h = 2^-11 relative or 2^-25 absolute (subnormal low halves, bf16x3.h:29-31) per term -- and the
      weights' split taken exactly);
  through sigmoid: Lipschitz 1/4, through tanh: Lipschitz 1, through GELU: conv_oracle.GELU_SLOPE, each plus the
      evaluation budget of conv_oracle.bound at the worst argument in reach;
  r h and (1 - z) h + z q: the exact bilinear expansion with its second-order terms,
      |r' h' - r h| <= |r| e_h + |h| e_r + e_r e_h,
      |h+' - h+| <= |1 - z| e_h + |q - h| e_z + e_z e_h + |z| e_q + e_z e_q;
  folded weights: the reference product x W_x equals [o, 1] F exactly (F = the float64 folded rows), the kernel multiplies by
      float32(F): + [|o|, 1] |float32(F) - F|;
  backward: linear in dhx_last given the saved states: through |Wq^T|, |Wzr^T| and the gate-derivative factors
      z (1 - q^2), z (1 - z) (q - h), r (1 - r) h, 1 - z, r, with grad_oracle.elementwise_bound's rounding counts; the x
      columns are the sum of 2 iters + 1 terms formed in two K halves (gruheadbwd.hip:108-111, 168, 177, 183-192):
      (2 iters + 2) u on their magnitudes.
No constant here was chosen from a GPU run.

Observed on an MI355X (information only -- no constant here was chosen from it): worst err/bound and worst rms ratio per
family and arithmetic from the module summary of tests/test_head_conformance_gpu.py.

    (no MI355X run of tests/test_head_conformance_gpu.py has been recorded for this revision yet)
"""
from __future__ import annotations

import math

import numpy as np
import torch

import conv_oracle as co
from conv_oracle import U, check, ok, rms, split_terms  # noqa: F401  (re-exported for the tests)

HIDDEN, XDIM, HX = 128, 64, 192
FWD_ARITH = {0: "bf16x3", 1: "f16x2"}                   # forward packed_format -> arithmetic
BWD_ARITH = {0: "bf16x3", 2: "bf16x2"}                  # backward packed_format -> arithmetic
TINY = 2.0 ** -125                                       # float32 results below the smallest normal may be flushed to zero
UB, UH, F16_ABS = 2.0 ** -9, 2.0 ** -11, 2.0 ** -25      # bf16 / fp16 unit roundoff; half the fp16 subnormal spacing


def gamma(k):
    """k accumulated float32 roundings: (1 + u)^k - 1 <= k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


def _t(a, dtype=torch.float64):
    return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dtype)


# ---- inputs shared by tests/test_head_oracle.py and tests/test_head_conformance_gpu.py -----------------------------------
# spec.init_params draws weights whose absolute row sums are about 12 (192 x 0.0625): a worst-case bound then grows twelvefold
# through each of the nine products of a four-iteration head and ends above the signal.  Scaled by 1 / 8 the row sums are 1.5
# (0.4 behind a sigmoid) and the propagated bound stays three decades under the result (tests/test_head_oracle.py, part (c)).
WEIGHT_SCALE = 0.125
# The aggregate level of a STAGE check (rms error within conv_oracle.R of the float32 twin's) presumes what it presumes for a
# convolution layer: that the product's error dominates the stage.  With the 1 / 8 weights it does not: q = tanh_f(v) has
# |v| ~ 0.05, where 1 - e (conv_common.h:95) cancels and leaves the absolute u e of conv_oracle.bound's tanh budget, 2 - 3
# times the float32 twin's relative rounding even with a correctly rounded exponential and reciprocal
# (tests/test_head_oracle.py::test_small_weights_leave_the_aggregate_level_to_tanh: 2.2 - 2.8 against 0.44 unscaled).  The
# stage checks therefore run with the network's own weights (scale 1), where R applies as it does to the GRU epilogues of
# tests/test_conv_conformance_gpu.py, and with the 1 / 8 weights at the bound level alone.
# pre1 is a bare product plus bias, no function behind it: it keeps both levels at either scale (and is where fp16 weights packed
# without their 2^6 scale show, which needs small weights: conv_oracle.R's note on f16x2).
STAGE_SCALE = 1.0
BARE_STAGES = ("pre1",)


def weights(seed=0, scale=WEIGHT_SCALE):
    """The head's parameters of himo_amd.seflow.spec.init_params(seed) in this module's names (float32), weight matrices
    multiplied by ``scale``."""
    from himo_amd.seflow import spec
    p = spec.init_params(seed)
    f = lambda k, s=1.0: torch.from_numpy(np.ascontiguousarray(p[k] * np.float32(s), dtype=np.float32))
    return dict(w_off=f("head.offset.weight", scale), b_off=f("head.offset.bias"),
                wzr=torch.cat([f("head.gru.z.weight", scale), f("head.gru.r.weight", scale)], 1).contiguous(),
                bzr=torch.cat([f("head.gru.z.bias"), f("head.gru.r.bias")]).contiguous(),
                wq=f("head.gru.q.weight", scale), bq=f("head.gru.q.bias"), w1=f("head.dec1.weight", scale), b1=f("head.dec1.bias"),
                w2=f("head.dec2.weight", scale), b2=f("head.dec2.bias"))


CELLS = 256               # a 16 x 16-cell grid


def scene(seed, n, cells=CELLS):
    """n points on a ``cells``-cell grid: about 10 % dropped (pid -1), among them the first row of the first block and the last
    row of every whole 64-row block; several points share a cell and a live point sits in cell 0.  Features N(0, 1) like a
    normalised map, offsets within a 0.2 m pillar, coordinates of a 100 m scene."""
    g = torch.Generator().manual_seed(10_000 + seed)
    pid = torch.randint(0, cells, (n,), generator=g, dtype=torch.int32)
    pid[torch.rand(n, generator=g) < 0.1] = -1
    if n > 1:
        pid[0] = -1
        pid[63::64] = -1
        pid[1] = 0
    else:
        pid[0] = 3
    if n > 4:
        pid[2] = pid[3] = 7
    if n > 64 and n % 64:
        pid[n - 1] = 5                                    # the last row of the partial block is live ...
        if n % 64 > 1:
            pid[n - 2] = -1                               # ... and its neighbour dropped
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(n=n, pid=pid, offsets=(torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([0.2, 0.2, 6.0]),
                img0=r(cells, 32), img1=r(cells, 32), dec=r(cells, 64), xyz_t=r(n, 3) * 30.0, pts=r(n, 3) * 30.0)


def f16_two_term(a):
    """the value an image feature enters the fp16-split head with: h + l of split2 (gruhead.hip:256, 272-274), float32"""
    t = split_terms("f16x2", np.asarray(a, np.float32))
    return torch.from_numpy(t[0] + t[1])


# ---- reference ------------------------------------------------------------------------------------------------------
def _gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def gather(sc, W, dtype=torch.float64):
    """[h0 | x] [n, 192]: the pillar's features (zeros for dropped points) and Linear(3, 64)(offset)"""
    pid = sc["pid"].long()
    live = (pid >= 0)[:, None]
    c = pid.clamp(min=0)
    h0 = torch.cat([_t(sc["img0"], dtype)[c], _t(sc["img1"], dtype)[c], _t(sc["dec"], dtype)[c]], 1)
    h0 = torch.where(live, h0, torch.zeros_like(h0))
    x = _t(sc["offsets"], dtype) @ _t(W["w_off"], dtype) + _t(W["b_off"], dtype)
    return torch.cat([h0, x], 1)


def gru_step(hx, W, dtype=torch.float64):
    """one GRU iteration on hx = [h | x] -> z, r, rhx = [r h | x], q, hx' = [(1 - z) h + z q | x]"""
    hx = _t(hx, dtype)
    h, x = hx[:, :HIDDEN], hx[:, HIDDEN:]
    g = torch.sigmoid(hx @ _t(W["wzr"], dtype) + _t(W["bzr"], dtype))
    z, r = g[:, :HIDDEN], g[:, HIDDEN:]
    rhx = torch.cat([r * h, x], 1)
    q = torch.tanh(rhx @ _t(W["wq"], dtype) + _t(W["bq"], dtype))
    return z, r, rhx, q, torch.cat([(1 - z) * h + z * q, x], 1)


def decode(hx, W, pid, dtype=torch.float64):
    """pre1 = hx W1 + b1, y1 = GELU(pre1), res [n, 3] = y1 W2 + b2 for live points, zeros for dropped ones"""
    pre1 = _t(hx, dtype) @ _t(W["w1"], dtype) + _t(W["b1"], dtype)
    y1 = _gelu(pre1)
    res = y1 @ _t(W["w2"], dtype) + _t(W["b2"], dtype)
    return pre1, y1, torch.where((pid >= 0)[:, None], res, torch.zeros_like(res))


def forward(sc, W, iters, dtype=torch.float64):
    """every stage of the head: hx [iters + 1], rhx, z, r, q [iters], pre1, y1, res, flow = (xyz_t - pts) + res"""
    hx = [gather(sc, W, dtype)]
    out = dict(rhx=[], z=[], r=[], q=[])
    for _ in range(iters):
        z, r, rhx, q, nxt = gru_step(hx[-1], W, dtype)
        out["z"].append(z); out["r"].append(r); out["rhx"].append(rhx); out["q"].append(q)
        hx.append(nxt)
    out["hx"] = hx
    out["pre1"], out["y1"], out["res"] = decode(hx[-1], W, sc["pid"], dtype)
    out["flow"] = (_t(sc["xyz_t"], dtype) - _t(sc["pts"], dtype)) + out["res"]
    return out


def fold(w_off, b_off, w):
    """the [144][cout] float64 matrix of himo_gru_head_batch_folded: rows 0..127 the hidden rows of w [192][cout], rows
    128..130 W_off W_x, row 131 b_off W_x, rows 132..143 zero"""
    w, w_off, b_off = _t(w), _t(w_off), _t(b_off)
    wx = w[HIDDEN:]
    return torch.cat([w[:HIDDEN], w_off @ wx, (b_off @ wx)[None], torch.zeros(12, w.shape[1], dtype=torch.float64)], 0)


def backward(dhx_last, sv, W, iters, dtype=torch.float64):
    """himo_gru_head_backward: d loss / d [h_T | x] and the saved hx, z, r, q (lists or stacks over t) ->
    daq [iters, n, 128], dazr [iters, n, 256], dhx0 [n, 192]"""
    d = _t(dhx_last, dtype)
    g, dx = d[:, :HIDDEN], d[:, HIDDEN:]
    wq_t, wzr_t = _t(W["wq"], dtype).T, _t(W["wzr"], dtype).T
    daq_s, dazr_s = [None] * iters, [None] * iters
    for t in range(iters - 1, -1, -1):
        z, r, q, h = _t(sv["z"][t], dtype), _t(sv["r"][t], dtype), _t(sv["q"][t], dtype), _t(sv["hx"][t], dtype)[:, :HIDDEN]
        daq = g * z * (1 - q * q)
        dazz = (g * (q - h)) * z * (1 - z)
        d_rhx = daq @ wq_t
        drh = d_rhx[:, :HIDDEN]
        dazr = torch.cat([dazz, (drh * h) * r * (1 - r)], 1)
        d_hx = dazr @ wzr_t
        g = g * (1 - z) + drh * r + d_hx[:, :HIDDEN]
        dx = dx + d_rhx[:, HIDDEN:] + d_hx[:, HIDDEN:]
        daq_s[t], dazr_s[t] = daq, dazr
    return torch.stack(daq_s), torch.stack(dazr_s), torch.cat([g, dx], 1)


# ---- stage bounds -----------------------------------------------------------------------------------------------------
def _nhwc(a):
    a = _t(a, torch.float32)
    return a.reshape(1, a.shape[0], 1, a.shape[1])


def _w11(w):
    w = _t(w, torch.float32)
    return w.reshape(1, 1, *w.shape)


def _rows(a):
    return None if a is None else a.reshape(a.shape[1], a.shape[3])


def _layer(arith, x, w, b, epilogue, aux_in=None, aux_out=None):
    """conv_oracle's reference, float32 twin and bound of the 1x1 layer y = epilogue(x w + b) on rows x"""
    n = lambda a: None if a is None else _nhwc(a)
    xs, ws = _nhwc(x), _w11(w)
    ref = co.conv_ref(xs, ws, b, 1, epilogue, aux_in=n(aux_in), aux_out=n(aux_out))
    ref32 = co.conv_ref(xs, ws, b, 1, epilogue, aux_in=n(aux_in), aux_out=n(aux_out), dtype=torch.float32)
    bnd = co.bound(arith, xs.numpy(), ws.numpy(), b, 1, epilogue, aux_in=n(aux_in), aux_out=n(aux_out), ref=ref)
    dv = co.operand_bound(arith, xs.numpy(), ws.numpy()) + U * ref["v"].abs()
    return ({k: _rows(v) for k, v in ref.items()}, {k: _rows(v) for k, v in ref32.items()}, {k: _rows(v) for k, v in bnd.items()},
            _rows(dv))


def x_bound(offsets, W):
    return gamma(4) * (_t(offsets).abs() @ _t(W["w_off"]).abs() + _t(W["b_off"]).abs()) + TINY


def dec2_bound(y1, W, e_y1=None):
    """the 33 roundings of the dec2 chain on |y1| |w2| + |b2| (+ an operand perturbation e_y1)"""
    y, w = _t(y1).abs(), _t(W["w2"]).abs()
    e = torch.zeros_like(y) if e_y1 is None else e_y1
    return e @ w + gamma(33) * ((y + e) @ w + _t(W["b2"]).abs()) + TINY


def stage_checks(arith, sc, W, sv, iters):
    """Every saved tensor of himo_gru_head_train (``sv``: hx [iters + 1][n, 192], rhx, z, r, q [iters], pre1, y1 [n, 32], res
    [n, 3 or 4]; float32, rows of the n points) against the reference of its stage on the kernel's own previous saves.

    Returns a list of (name, got, ref float64, bound, float32 twin or None).  A bound of zero demands bit equality; the
    caller runs ``verdict`` (or conv_oracle.ok) on each entry.  Names: gather, x, xcopy, z, r, rhx, q, hx, pre1, y1, res."""
    out = []
    live = (sc["pid"] >= 0)[:, None]
    hx0 = _t(sv["hx"][0], torch.float32)
    g = gather(sc, W)
    g32 = gather(sc, W, torch.float32)
    want = g[:, :HIDDEN]
    if arith == "f16x2":                                 # image columns enter as their two-term fp16 value
        img = torch.cat([f16_two_term(want[:, :64].float()).double(), want[:, 64:]], 1)
        want = img
    out.append(("gather", hx0[:, :HIDDEN], want, torch.zeros_like(want), None))
    out.append(("x", hx0[:, HIDDEN:], g[:, HIDDEN:], x_bound(sc["offsets"], W), g32[:, HIDDEN:]))
    for t in range(iters):
        hx, rhx, z, r, q = (_t(sv[k][t], torch.float32) for k in ("hx", "rhx", "z", "r", "q"))
        nxt = _t(sv["hx"][t + 1], torch.float32)
        for name, a in (("xcopy", rhx[:, HIDDEN:]), ("xcopy", nxt[:, HIDDEN:])):
            out.append((name, a, hx0[:, HIDDEN:].double(), torch.zeros(a.shape, dtype=torch.float64), None))
        h = hx[:, :HIDDEN]
        ref, r32, bnd, dv = _layer(arith, hx, W["wzr"], W["bzr"], 3, aux_in=h)
        out.append(("z", z, ref["y"], bnd["y"], r32["y"]))
        gr = torch.sigmoid(ref["v"][:, HIDDEN:])
        # conv_oracle.bound, epilogue 3: bg = dv / 4 + g u (6 + |v|) -- the gate itself, before it multiplies h
        out.append(("r", r, gr, 0.25 * dv[:, HIDDEN:] + gr * U * (6 + ref["v"][:, HIDDEN:].abs()), torch.sigmoid(r32["v"][:, HIDDEN:])))
        out.append(("rhx", rhx[:, :HIDDEN], ref["aux_out"], bnd["aux_out"] + TINY, r32["aux_out"]))
        ref, r32, bnd, dv = _layer(arith, rhx, W["wq"], W["bq"], 4, aux_in=z, aux_out=h)
        v = ref["v"]
        qr = torch.tanh(v)
        # conv_oracle.bound, epilogue 4: bq = dv + 2 e u (4 + 2 |v|) + 4 u |q|, e = exp(-2 |v|)
        out.append(("q", q, qr, dv + 2 * torch.exp(-2 * v.abs()) * U * (4 + 2 * v.abs()) + 4 * U * qr.abs(), torch.tanh(r32["v"])))
        out.append(("hx", nxt[:, :HIDDEN], ref["aux_out"], bnd["aux_out"] + TINY, r32["aux_out"]))
    hT = _t(sv["hx"][iters], torch.float32)
    ref, r32, bnd, dv = _layer(arith, hT, W["w1"], W["b1"], 2)
    out.append(("pre1", _t(sv["pre1"], torch.float32), ref["v"], dv, r32["v"]))
    out.append(("y1", _t(sv["y1"], torch.float32), ref["y"], bnd["y"], r32["y"]))
    y1 = _t(sv["y1"], torch.float32)
    res = y1.double() @ _t(W["w2"]) + _t(W["b2"])
    res32 = y1 @ W["w2"].float() + W["b2"].float()
    z3 = torch.zeros_like(res)
    out.append(("res", _t(sv["res"], torch.float32)[:, :3], torch.where(live, res, z3), torch.where(live, dec2_bound(y1, W), z3),
                torch.where(live, res32.double(), z3).float()))
    return out


MIN_AGGREGATE = 128


def verdict(arith, got, ref, bnd, ref32, case="", limit=None, aggregate=True):
    """both levels of conv_oracle.check -> (passed, worst, rms ratio, report).  Where the bound is zero the check is bit
    equality (err / bound = inf for any difference); the aggregate level needs a float32 twin and at least MIN_AGGREGATE outputs
    (grad_oracle.check_cols' argument: the ratio of two rms errors over k outputs is a statistic; over the 32 outputs of one
    row's pre1 a correct float32 product in another order reaches 2.2 against R = 2, over 128 the chance is below 1e-12)."""
    got, ref, bnd = _t(got), _t(ref), _t(bnd)
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    exact = bnd == 0
    if bool(exact.any()):
        bad = exact & (err > 0)
        if bool(bad.any()):
            i = tuple(int(v) for v in torch.nonzero(bad)[0])
            return False, math.inf, 0.0, f"{case} [{arith}]: {int(bad.sum())} elements differ where equality is demanded, first at {i}: got {float(got[i]):.9g} ref {float(ref[i]):.9g}"
        bnd = torch.where(exact, torch.ones_like(bnd), bnd)
    r32 = ref32 if (aggregate and ref32 is not None and ref.numel() >= MIN_AGGREGATE) else None
    worst, rr, report = check(got, ref, bnd, r32, arith, case, limit=limit)
    lim = co.R[arith] if limit is None else limit
    return worst <= 1.0 and rr <= lim, worst, rr, report


# ---- propagated bounds --------------------------------------------------------------------------------------------------
def _act_terms(arith, amag):
    """upper bounds of the |terms| an operand of magnitude <= amag splits into, and of its residual (see the docstring)"""
    if arith == "f32":
        return [amag], torch.zeros_like(amag)
    if arith in ("bf16x3", "bf16x2"):
        c = 1.0 + UB
        if arith == "bf16x2":
            return [c * amag, c * UB * amag], UB * UB * amag
        return [c * amag, c * UB * amag, c * UB * UB * amag], UB ** 3 * amag
    if arith == "f16x2":
        lo = UH * amag + F16_ABS                          # |a - h|
        return [(1 + UH) * amag + F16_ABS, (1 + UH) * lo + F16_ABS], UH * lo + F16_ABS
    raise ValueError(arith)


def gemm_mag_bound(arith, amag, w):
    """Per-output worst case of |acc - a w| for ANY float32 operand a with |a| <= amag [n, K] and the float32 weights w [K, cout]:
    conv_oracle.operand_bound with the operand's split at its worst case and the weights' split exact."""
    amag = _t(amag)
    w = np.asarray(_t(w, torch.float32).numpy(), np.float32)
    K = w.shape[0]
    aw = _t(np.abs(w))
    if arith == "f32":
        return (K + 2) * U * (amag @ aw) + TINY
    ws = split_terms(arith, w, weights=True)
    dw = _t(np.abs(w.astype(np.float64) - sum(t.astype(np.float64) for t in ws)))
    terms, resid = _act_terms(arith, amag)
    b = resid @ aw + amag @ dw + resid @ dw
    kept = co.KEPT[arith]
    for i in range(len(terms)):
        for j in range(len(ws)):
            if (i, j) not in kept:
                b = b + terms[i] @ _t(np.abs(ws[j]))
    sw = _t(sum(np.abs(t).astype(np.float64) for t in ws))
    return b + (len(kept) * K + 2) * U * (sum(terms) @ sw) + TINY


def _pre(arith, a, e, w, b, extra=None):
    """reference and bound of a w + b for a kernel operand within e of a"""
    w64 = _t(w)
    v = a @ w64 + (_t(b) if b is not None else 0)
    ev = e @ w64.abs() + gemm_mag_bound(arith, a.abs() + e, w)
    if extra is not None:
        ev = ev + extra
    if b is not None:
        ev = ev + U * (v.abs() + ev)                       # the bias add
    return v, ev


def _sigmoid_b(v, ev):
    g = torch.sigmoid(v)
    return g, 0.25 * ev + (g + 0.25 * ev) * U * (6 + v.abs() + ev)


def _tanh_b(v, ev):
    q = torch.tanh(v)
    e = torch.exp(-2 * (v.abs() - ev).clamp(min=0))
    return q, ev + 2 * e * U * (4 + 2 * (v.abs() + ev)) + 4 * U * (q.abs() + ev)


def propagate_forward(arith, sc, W, iters, folded=False):
    """float64 reference of res [n, 3] / flow [n, 3] and a per-element bound on what a kernel of ``arith`` may return for them
    (inference kernels, and the training kernel end to end).  folded: the kernel multiplies [h | o, 1, 0 ...] by the float32
    roundings of ``fold`` (K = 144)."""
    ref = forward(sc, W, iters)
    live = (sc["pid"] >= 0)[:, None]
    hx = ref["hx"][0]
    h, x = hx[:, :HIDDEN], hx[:, HIDDEN:]
    eh = torch.zeros_like(h)
    if arith == "f16x2":
        eh = torch.cat([(f16_two_term(h[:, :64].float()).double() - h[:, :64]).abs(), eh[:, 64:]], 1)
    n = h.shape[0]
    if folded:
        o1 = torch.cat([_t(sc["offsets"]), torch.ones(n, 1, dtype=torch.float64), torch.zeros(n, 12, dtype=torch.float64)], 1)
        xa, ex = o1, torch.zeros_like(o1)
        mats, extras = {}, {}
        for k in ("wzr", "wq", "w1"):
            f64 = fold(W["w_off"], W["b_off"], W[k])
            f32 = f64.float()
            mats[k] = f32
            extras[k] = o1.abs() @ (f32.double() - f64)[HIDDEN:].abs()
        # the reference's own x W_x is [o, 1] F: evaluate the reference product with F so that ``extras`` is the whole difference
        pre = lambda a_h, e_h, k, b: _pre_folded(arith, a_h, e_h, xa, mats[k], fold(W["w_off"], W["b_off"], W[k]), W[b], extras[k])
    else:
        xa, ex = x, x_bound(sc["offsets"], W)
        pre = lambda a_h, e_h, k, b: _pre(arith, torch.cat([a_h, xa], 1), torch.cat([e_h, ex], 1), W[k], W[b])
    for _ in range(iters):
        v, ev = pre(h, eh, "wzr", "bzr")
        g, eg = _sigmoid_b(v, ev)
        z, r, ez, er = g[:, :HIDDEN], g[:, HIDDEN:], eg[:, :HIDDEN], eg[:, HIDDEN:]
        rh = r * h
        erh = r * eh + h.abs() * er + er * eh
        erh = erh + U * (rh.abs() + erh)
        v, ev = pre(rh, erh, "wq", "bq")
        q, eq = _tanh_b(v, ev)
        hn = (1 - z) * h + z * q
        en = (1 - z).abs() * eh + (q - h).abs() * ez + ez * eh + z * eq + ez * eq
        en = en + 3 * U * (((1 - z).abs() + ez) * (h.abs() + eh) + (z + ez) * (q.abs() + eq))
        h, eh = hn, en
    t, et = pre(h, eh, "w1", "b1")
    y = _gelu(t)
    ey = co.GELU_SLOPE * et + 0.5 * (t.abs() + et) * (co.ERF_AS + 16 * U) + 4 * U * (y.abs() + co.GELU_SLOPE * et) + 1e-37
    z3 = torch.zeros(n, 3, dtype=torch.float64)
    eres = torch.where(live, dec2_bound(y, W, ey), z3)
    pf = _t(sc["xyz_t"]) - _t(sc["pts"])
    # dropped points: the one rounding of xyz_t - pts (the suites also compare those rows with the float32 difference bitwise)
    eflow = torch.where(live, eres + U * pf.abs() + U * (pf.abs() + ref["res"].abs() + eres + U * pf.abs()), U * pf.abs()) + TINY
    return dict(ref=ref, res=ref["res"], e_res=eres, flow=ref["flow"], e_flow=eflow, hx=torch.cat([h, x], 1), e_h=eh)


def _pre_folded(arith, h, eh, o1, w32, f64, b, extra):
    """[h | o, 1] float32(F) + b against the reference h W_h + [o, 1] F + b"""
    a = torch.cat([h, o1], 1)
    e = torch.cat([eh, torch.zeros_like(o1)], 1)
    v = a @ f64 + _t(b)
    ev = e @ w32.double().abs() + gemm_mag_bound(arith, a.abs() + e, w32) + extra
    return v, ev + U * (v.abs() + ev)


def propagate_backward(arith, dhx_last, sv, W, iters):
    """float64 reference of daq, dazr, dhx0 (``backward`` on the float32 inputs) and per-element bounds e_daq, e_dazr, e_dhx0"""
    d = _t(dhx_last)
    g, dx = d[:, :HIDDEN], d[:, HIDDEN:]
    eg = torch.zeros_like(g)
    wq_t, wzr_t = W["wq"].float().T.contiguous(), W["wzr"].float().T.contiguous()
    dxmag, edx = dx.abs(), torch.zeros_like(dx)
    e_daq, e_dazr = [None] * iters, [None] * iters
    for t in range(iters - 1, -1, -1):
        z, r, q, h = _t(sv["z"][t]), _t(sv["r"][t]), _t(sv["q"][t]), _t(sv["hx"][t])[:, :HIDDEN]
        gm = g.abs() + eg
        fq = z * (1 - q * q)
        daq = g * fq
        # grad_oracle.elementwise_bound gru_bwd1 with |g| <= |g| + eg
        edaq = eg * fq.abs() + U * (gm * z * (q * q + (1 - q * q).abs()) + 3 * gm * fq.abs())
        dz = g * (q - h)
        edz = eg * (q - h).abs() + 3 * U * gm * (q - h).abs()
        fz = z * (1 - z)
        dazz = dz * fz
        edazz = edz * fz + 5 * U * (dz.abs() + edz) * fz
        dhp = g * (1 - z)
        edhp = eg * (1 - z) + 3 * U * gm * (1 - z)
        d_rhx = daq @ wq_t.double()
        ed_rhx = edaq @ wq_t.double().abs() + gemm_mag_bound(arith, daq.abs() + edaq, wq_t)
        drh, edrh = d_rhx[:, :HIDDEN], ed_rhx[:, :HIDDEN]
        dhp2 = dhp + drh * r
        edhp2 = edhp + edrh * r + 2 * U * (dhp.abs() + edhp + (drh.abs() + edrh) * r)
        fr = h * r * (1 - r)
        dazr_r = drh * fr
        edazr_r = edrh * fr.abs() + 5 * U * (drh.abs() + edrh) * fr.abs()
        dazr, edazr = torch.cat([dazz, dazr_r], 1), torch.cat([edazz, edazr_r], 1)
        d_hx = dazr @ wzr_t.double()
        ed_hx = edazr @ wzr_t.double().abs() + gemm_mag_bound(arith, dazr.abs() + edazr, wzr_t)
        gn = dhp2 + d_hx[:, :HIDDEN]
        eg = edhp2 + ed_hx[:, :HIDDEN] + U * (dhp2.abs() + edhp2 + d_hx[:, :HIDDEN].abs() + ed_hx[:, :HIDDEN])
        g = gn
        dx = dx + d_rhx[:, HIDDEN:] + d_hx[:, HIDDEN:]
        edx = edx + ed_rhx[:, HIDDEN:] + ed_hx[:, HIDDEN:]
        dxmag = dxmag + (daq.abs() + edaq) @ wq_t.double().abs()[:, HIDDEN:] + (dazr.abs() + edazr) @ wzr_t.double().abs()[:, HIDDEN:]
        e_daq[t], e_dazr[t] = edaq + TINY, edazr + TINY
    edx = edx + (2 * iters + 2) * U * (dxmag + edx)
    daq, dazr, dhx0 = backward(dhx_last, sv, W, iters)
    return dict(daq=daq, dazr=dazr, dhx0=dhx0, e_daq=torch.stack(e_daq), e_dazr=torch.stack(e_dazr),
                e_dhx0=torch.cat([eg, edx], 1) + TINY)
