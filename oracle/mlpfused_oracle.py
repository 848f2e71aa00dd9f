"""Float64 reference and worst-case error model of the LAYER-KERNEL path of the per-pair fit (include/himo_amd.h:
himo_mlp_forward_fused, himo_mlp_backward_fused, himo_mlp_backward_fused_bias, himo_mlp_bias_workspace_bytes -- csrc/mlpfused.hip;
himo_chamfer_trunc and its size query -- csrc/fastnsf.hip; himo_nsfp_prepare, himo_nsfp_objective, himo_nsfp_keep_best and their
size queries -- csrc/nsfp.hip).  CPU only.  It stands on oracle/nsf_oracle.py: the float64 network, its float32 twin, the propagated
per-unit bounds (forward_bounds: E_k, E_out; backward_bounds: eg_k), the admitted cases (mlp_case, mask_threshold_case) and verdict.

Why nsf_oracle's product bounds carry over unchanged (read from both kernels): mlp_gemm (csrc/mlpfused.hip) issues, slab after slab
of 16 reduction steps, the three products low x high, high x low, high x high into ONE float32 accumulator -- the order of
nsf_fwd_gemm and of the backward product of csrc/nsffused.hip -- on the same himo_mlp_repack copies of the weights; the activations
are split by the same split2 (forward) and two-term bf16 (backward); the epilogue is the same fma(acc, 2^-6, b); the first layer
is the same 3 fma + product + bias (5 roundings), the last the same 128-step fma chain from the bias (gamma(129)), the gradient
through the last layer the same 4-term fma chain (gamma(4)).  So gemm_bound("f16x2" | "bf16x2"), E_k, E_out and eg_k are the bounds
here too.  What differs is what leaves the chip: H_k and dZ_k as plain [rows][128] float32, every one compared element by element.

Shapes.  EVERY [n][.] buffer of csrc/mlpfused.hip holds ceil(n / 64) * 64 rows and the padding rows are computed and stored like
the others; ``block_rows(n)``.  The cases of nsf_oracle are padded to whole blocks of 256 rows, a superset: rows [0, block_rows(n)) of
the case are used, the padding rows (x = 0: one more point) compared like any other row.

Bounds (u = 2^-24, u64 = 2^-53, gamma(k) = k u / (1 - k u); every constant is counted from the code, none was chosen from a GPU run):
  H_k      relu(z_k) within (E_k + TINY) where z_k > 0, exactly 0 where z_k <= 0 (admission: |z| >= 2 E, so the kernel's mask is
           the reference's as long as it is within E).
  out      E_out.
  dZ_k     g_k (z_k > 0) within eg_k where z_k > 0, exactly 0 elsewhere and on rows whose dout is 0.
  db_k     mlp_backward_kernel: a lane adds its 32 rows of a column one after the other to 0 (32 adds), the two half-waves are
           added (1): a block's partial.  mlp_bias_reduce_kernel: thread (group, column) walks blocks group, group + 8, ... in four
           chains of stride 32 and a stride-8 tail on chain 0 (``reduce_chain``: the adds on the longest chain), combines the chains
           in pairs (2) and thread 0 adds the eight groups one after the other (7).  A sum whose every path from a term to the
           result passes at most D adds is within gamma(D) sum |terms| of exact: D = 32 + 1 + reduce_chain(n_blocks) + 2 + 7
           (``bias_depth``).  The terms are the kernel's own dZ: sum over rows of eg_k, plus gamma(D) sum (|dZ| + eg_k).
  Chamfer  (chamfer_trunc_a_kernel / _b_kernel) a term c (m - p) with c = 2.0f / (float)n: the difference, the quotient and the
           product round once each: gamma(3) |term|.  A scattered term is rounded to an integer multiple of 2^-40: 2^-41 more, each.
           The integer sum is exact (two's complement, order-independent).  Its conversion to float32 rounds once (u |S|), the final
           g + S once (u |result|).  A row nobody is kept for: exactly 0.
           loss: every term d / n is one float64 rounding, block_sum is a 256-leaf tree (8 adds on a path), sum_partials_kernel a
           stride-256 loop (ceil(B / 256) adds) and the same tree (8): gamma64(17 + ceil(B / 256)) sum |terms| (+ 4 u64 |loss| for
           the reference's own float64 sum).
  NSFP     (nsfp_a_kernel / nsfp_b_kernel) dout = n0 dL/dout: 2.0f (m - p): the difference rounds, the doubling does not: gamma(1);
           a scattered term (double)(m - p) x (2 (n0 / n1) 2^40): the float32 difference (u), the float64 quotient and two products
           (4 u64), then the integer rounding (2^-41); the integer to float64 (u64), x 2^-40 exact, to float32 (u), g + S (u).
           loss_partial[tile] = a butterfly of 6 adds over float64 copies of d: gamma64(6); loss_partial[tiles + blk] = that, the
           two-level combine of the four waves and the product with n0 / n1 (itself rounded): gamma64(10).  count_partial: exact.
Decisions AT the threshold d == trunc^2 use exactly representable inputs (trunc = 0.5, t2 = 0.25; lattice coordinates).

Keep-best (nsfp_keep_best_kernel) is restated operation by operation (``keep_best_step``): the device state must EQUAL it.

Wrong twins (tests/test_mlpfused_oracle.py shows that each misses a bound or an equality on the case the GPU test uses):
  drop_hm      the bf16 high x low product of one backward layer dropped        swap_tile_rows  two rows of a 32-row tile swapped in H_k
  bias_half    db_k without the rows of the second half-wave (row & 4)         reduce_skip     the reduce skips blocks 24..31 (mod 32)
  cham_lt      Chamfer keeps d < t2                                             scatter_last    the scattered half keeps the last writer
  no_wb        the n0 / n1 factor missing from direction b                      keep_le         keep-best improves on L <= best - min_delta

Observed on an MI355X (information only -- no constant here was chosen from it): worst err/bound and worst rms ratio per family
from the module summary of tests/test_mlpfused_conformance_gpu.py (the kernels passed as they were):
    mlp_forward    f16x2 0.541, 1.79 (R 4)       mlp_backward  bf16x2 0.641, 28.8 (R 128); dZ_k bit-equal between the entry points
    mlp_bias       bf16x2 0.114, 37.7 (R 128)    bias_reduce   f32 0.0277, 0.706 (R 2)
    chamfer        0.663, 0.49 (R_ELEM 32)       nsfp_objective 0.0912, 0.167 (R_ELEM 32); moved, searches, counts bit-equal
    keep_best      equal to the restatement (38 steps)                 40 refusals, nothing written
"""
from __future__ import annotations

import copy
import math
from types import SimpleNamespace

import numpy as np
import torch

import grad_oracle as go
import nsf_oracle as no
from nsf_oracle import F64, HID, TINY, U, gamma

U64 = 2.0 ** -53
ROWS = 64
SCAT = 2.0 ** 40
R_ELEM = go.R_ELEM


def gamma64(k):
    return k * U64 / (1 - k * U64)


def block_rows(n):
    """rows every [n][.] buffer of csrc/mlpfused.hip holds: whole 64-row blocks"""
    return 0 if n <= 0 else -(-n // ROWS) * ROWS


def mlp_row(rt, r, lh):
    """csrc/mlpfused.hip mlp_row: the row of accumulator register r of row tile rt in half-wave lh"""
    return rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh


# ---- the cases -----------------------------------------------------------------------------------------------------------
def external_dout(case, seed=7):
    """a random gradient of the output whose padding rows are zero (tests/test_nsf_conformance_gpu.py _external_dout)"""
    g = torch.Generator().manual_seed(seed + case.n)
    d = torch.randn(len(case.x), 4, generator=g) * 10.0 ** (-3 * torch.rand(4, generator=g))
    d[case.n:] = 0.0
    return d


def external_case(base, key):
    """``base`` (an admitted case of nsf_oracle) with the backward pass of an external dout: reference, float32 twin and eg_k.  The
    forward bounds are the base's (they do not depend on dout).  Cached."""
    key = ("mlpfused", key)
    if key in no._CACHE:
        return no._CACHE[key]
    case = copy.copy(base)
    case.dout = dout = external_dout(base)
    case.ref = no.iteration(base.params, base.x, base.n, dout=dout)
    case.ref32 = no.iteration(base.params, base.x, base.n, dtype=torch.float32, dout=dout)
    case.e_dout = None
    case.e_grads, case.e_g = no.backward_bounds(base.params, base.x, case.ref, base.E, None)
    no._CACHE[key] = case
    return case


def mlp_case(n, n_hidden, dead=False):
    return external_case(no.mlp_case(n, n_hidden, dead), (n, n_hidden, dead))


def mask_case():
    return external_case(no.mask_threshold_case(), "mask")


def padding_margin_ok(case):
    """the padding rows (x = 0) are computed and compared too: their masks need the same margin as an admitted point's"""
    R = block_rows(case.n)
    return bool(no.relu_margin_ok([z[case.n:R] for z in case.ref["zs"]], [e[case.n:R] for e in case.E]).all())


# ---- the hidden layers' bias gradients ---------------------------------------------------------------------------------------
def reduce_chain(n_blocks):
    """adds on the longest chain of one thread of mlp_bias_reduce_kernel"""
    worst = 0
    for grp in range(8):
        b, t = grp, [0, 0, 0, 0]
        while b + 24 < n_blocks:
            t = [c + 1 for c in t]
            b += 32
        while b < n_blocks:
            t[0] += 1
            b += 8
        worst = max(worst, max(t))
    return worst


def bias_depth(n_blocks):
    return 32 + 1 + reduce_chain(n_blocks) + 2 + 7


def bias_sum_f32(dz, variant=None):
    """the float32 twin of db = column sums of dZ [64 n_blocks][128], in the kernels' order"""
    dz = np.ascontiguousarray(torch.as_tensor(dz).float().numpy(), np.float32)
    nb = len(dz) // ROWS
    blk = dz.reshape(nb, ROWS, HID)
    half = []
    for lh in (0, 1):
        c = np.zeros((nb, HID), np.float32)
        for rt in (0, 1):
            for r in range(16):
                c = c + blk[:, mlp_row(rt, r, lh), :]
        half.append(c)
    part = half[0] if variant == "bias_half" else half[0] + half[1]
    sh = []
    for grp in range(8):
        t = [np.zeros(HID, np.float32) for _ in range(4)]
        b = grp
        while b + 24 < nb:
            for q in range(4):
                if not (variant == "reduce_skip" and (b + 8 * q) % 32 >= 24):
                    t[q] = t[q] + part[b + 8 * q]
            b += 32
        while b < nb:
            if not (variant == "reduce_skip" and b % 32 >= 24):
                t[0] = t[0] + part[b]
            b += 8
        sh.append((t[0] + t[1]) + (t[2] + t[3]))
    r = sh[0]
    for g in range(1, 8):
        r = r + sh[g]
    return torch.from_numpy(r.astype(np.float32))


def bias_reduce_checks(dZ_dev, db_dev, n_blocks):
    """the column sums alone: db_dev[k] [128] against the float64 column sums of the kernel's OWN dZ_dev[k] [64 n_blocks][128]"""
    out = []
    D = bias_depth(n_blocks)
    for k, (dz, db) in enumerate(zip(dZ_dev, db_dev)):
        dz = torch.as_tensor(dz)
        assert len(dz) == ROWS * n_blocks
        out.append(("bias_reduce", f"db{k}", "f32", db, dz.double().sum(0), gamma(D) * dz.double().abs().sum(0) + TINY, bias_sum_f32(dz).double(), False))
    return out


def reduce_case(n_blocks, seed=11):
    """parameters and inputs of the n_blocks sweep: n = 64 n_blocks uniform points, two hidden layers, a random dout on every row"""
    g = torch.Generator().manual_seed(100 * seed + n_blocks)
    n = ROWS * n_blocks
    x = torch.zeros(n, 4)
    x[:, :3] = ((torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([10.0, 10.0, 2.5])).float()
    dout = torch.randn(n, 4, generator=g) * 10.0 ** (-3 * torch.rand(4, generator=g))
    return SimpleNamespace(n=n, n_hidden=2, params=no.mlp_params(seed, 2), x=x, dout=dout, grid=None, dead=False, seed=seed)


# ---- the network's checks -------------------------------------------------------------------------------------------------
def mlpfused_checks(case, got):
    """every comparison of the fused layer kernels' results ``got`` (dict H [k] [R, 128], out [R, 4], dZ [k] [R, 128], db [k] [128];
    missing keys are skipped; R = block_rows(n)) with ``case``: (family, name, arith, got, ref, bound, float32 twin, cols)"""
    n, ref, r32 = case.n, case.ref, case.ref32
    R = block_rows(n)
    on = [(z[:R] > 0) for z in ref["zs"]]
    out = []
    for k, h in enumerate(got.get("H", ())):
        out.append(("mlp_forward", f"H{k}", "f16x2", h, ref["zs"][k][:R].clamp(min=0), (case.E[k][:R] + TINY) * on[k],
                    r32["zs"][k][:R].clamp(min=0), False))
    if "out" in got:
        out.append(("mlp_forward", "out", "f16x2", got["out"], ref["out"][:R], case.e_out[:R] + TINY, r32["out"][:R], False))
    twin_dz = [r32["gs"][k][:R] * (r32["zs"][k][:R] > 0) for k in range(len(on))]
    for k, dz in enumerate(got.get("dZ", ())):
        eg = case.e_g[k][:R] * on[k]
        out.append(("mlp_backward", f"dZ{k}", "bf16x2", dz, ref["gs"][k][:R] * on[k], eg + TINY * (eg > 0), twin_dz[k], False))
    D = bias_depth(R // ROWS)
    for k, db in enumerate(got.get("db", ())):
        dz, eg = (ref["gs"][k][:R] * on[k]), case.e_g[k][:R] * on[k]
        bnd = eg.sum(0) + gamma(D) * (dz.abs() + eg).sum(0) + TINY
        out.append(("mlp_bias", f"db{k}", "bf16x2", db, dz[:n].sum(0), bnd, bias_sum_f32(twin_dz[k]).double(), False))
    return out


def bf16(t):
    return t.float().bfloat16().double()


def twin(case, variant=None, layer=1, rows=(1, 2)):
    """what the kernels return, from the float32 twin of ``case``; ``variant``: a deliberately wrong one (module docstring)"""
    r32, R, L = case.ref32, block_rows(case.n), case.n_hidden
    on = [(z[:R] > 0) for z in r32["zs"]]
    H = [z[:R].clamp(min=0) for z in r32["zs"]]
    dZ = [r32["gs"][k][:R] * on[k] for k in range(L)]
    if variant == "drop_hm":                                 # g_{layer-1} = dZ_layer W_layer^T without high(dZ) x low(W^T); what is below follows
        g = None
        for k in range(L - 1, -1, -1):
            if g is not None:
                dZ[k] = (g * on[k]).float()
            if k:
                wt = case.params[k][0].T.double()
                g = dZ[k].double() @ wt
                if k == layer:
                    g = g - bf16(dZ[k]) @ bf16(wt - bf16(wt))
    if variant == "swap_tile_rows":
        H[layer - 1] = H[layer - 1].clone()
        H[layer - 1][[rows[0], rows[1]]] = H[layer - 1][[rows[1], rows[0]]]
    db = [bias_sum_f32(dz, variant) for dz in dZ]
    return dict(H=H, out=r32["out"][:R], dZ=dZ, db=db)


# ---- truncated Chamfer on given correspondences ------------------------------------------------------------------------------
def _kept(d, t2, variant=None):
    with np.errstate(invalid="ignore"):
        return (d < t2) if variant == "cham_lt" else (d <= t2)


def chamfer(moved, pc1, d_a, i_a, d_b, i_b, trunc, dtype=np.float64, variant=None):
    """himo_chamfer_trunc as a function of its inputs: t2 = float32(trunc)^2 in float32; a term is kept iff d <= t2 (NaN, +inf
    dropped); loss = sum_kept d_a / n0 + sum_kept d_b / n1; grad_i = [a kept] 2/n0 (m_i - p_{i_a}) + sum_{j kept, i_b[j] = i} 2/n1
    (m_i - p_j).  n0 == 0 or n1 == 0: loss 0, gradient 0 (neither kernel keeps a term).  dtype float64: the reference with its
    bounds (grad, e_grad, loss, e_loss); float32: the twin in the kernels' own arithmetic."""
    n0, n1 = len(moved), len(pc1)
    t2 = np.float32(trunc) * np.float32(trunc)
    m32, p32 = np.asarray(moved, np.float32).reshape(n0, 3), np.asarray(pc1, np.float32).reshape(n1, 3)
    if n0 == 0 or n1 == 0:
        z = np.zeros((n0, 3))
        return dict(loss=0.0, e_loss=0.0, grad=z, e_grad=z.copy(), kept_a=0, kept_b=0)
    d_a, d_b = np.asarray(d_a, np.float32), np.asarray(d_b, np.float32)
    ka, kb = _kept(d_a, t2, variant), _kept(d_b, t2, variant)
    ia, ib = np.where(ka, i_a, 0), np.asarray(i_b)[kb]
    jb = np.nonzero(kb)[0]
    ta64 = [(d_a[ka].astype(np.float64) / n0), (d_b[kb].astype(np.float64) / n1)]
    loss = math.fsum(d_a[ka].astype(np.float64)) / n0 + math.fsum(d_b[kb].astype(np.float64)) / n1
    res = dict(loss=loss, kept_a=int(ka.sum()), kept_b=int(kb.sum()))
    if dtype == np.float64:
        m, p = m32.astype(np.float64), p32.astype(np.float64)
        ta = np.where(ka[:, None], 2.0 / n0 * (m - p[ia]), 0.0)
        tb = 2.0 / n1 * (m[ib] - p[jb])
        S, Sabs, cnt = np.zeros((n0, 3)), np.zeros((n0, 3)), np.zeros((n0, 1))
        np.add.at(S, ib, tb)
        np.add.at(Sabs, ib, np.abs(tb))
        np.add.at(cnt, ib, 1.0)
        grad = ta + S
        eS = gamma(3) * Sabs + cnt * 2.0 ** -41
        ea = gamma(3) * np.abs(ta)
        conv = U * (np.abs(S) + eS)
        live = (ka[:, None] | (cnt > 0)) & np.ones((1, 3), bool)
        e = ea + eS + conv + U * (np.abs(grad) + ea + eS + conv)
        blocks = (n0 + 255) // 256 + (n1 + 255) // 256
        mag = float(ta64[0].sum() + ta64[1].sum())
        res.update(grad=grad, e_grad=np.where(live, e + TINY, 0.0), e_loss=gamma64(17 + -(-blocks // 256)) * mag + 4 * U64 * abs(loss) + 1e-300)
        return res
    c0, c1 = np.float32(2.0) / np.float32(n0), np.float32(2.0) / np.float32(n1)
    ga = np.where(ka[:, None], c0 * (m32 - p32[ia]), np.float32(0.0)).astype(np.float32)
    q = np.rint((c1 * (m32[ib] - p32[jb])).astype(np.float64) * SCAT).astype(np.int64)
    scat = np.zeros((n0, 3), np.int64)
    if variant == "scatter_last":
        scat[ib] = q
    else:
        np.add.at(scat, ib, q)
    res.update(grad=(ga + (scat.astype(np.float64) * (1.0 / SCAT)).astype(np.float32)).astype(np.float32),
               loss=float(ta64[0].sum() + ta64[1].sum()))
    return res


CHAMFER_CASES = ((1, 1), (255, 257), (256, 256), (257, 255), (300, 0), (0, 300), (300, 2057))
CHAMFER_TRUNC = 0.5
FAN_ROW, FAN_IN = 123, 2000


def _hand_made(n, n_other, g, t2):
    """distances drawn independently of the geometry, rows 8 i .. 8 i + 3 exactly t2, the next float, +inf and NaN (the last two with
    index -1, which no kernel may read); indices uniform"""
    d = (torch.rand(n, generator=g) * 0.5).numpy().astype(np.float32)
    i = torch.randint(max(n_other, 1), (n,), generator=g).numpy().astype(np.int32)
    r = np.arange(n) % 8
    d[r == 0] = t2
    d[r == 1] = np.nextafter(t2, np.float32(np.inf))
    d[r == 2] = np.inf
    d[r == 3] = np.nan
    i[(r == 2) | (r == 3)] = -1
    return d, i


def chamfer_case(n0, n1):
    """inputs of himo_chamfer_trunc with hand-made correspondences (coordinates below 2^7).  (300, 2057): pc1 rows [0, 2000) all pull
    moved row 123 (at the origin, its own a-term dropped) -- towards -x (a negative sum), in exactly opposite pairs along y (a zero
    sum) and towards +z (a positive sum)"""
    g = torch.Generator().manual_seed(4000 + 7 * n0 + n1)
    t2 = np.float32(CHAMFER_TRUNC) * np.float32(CHAMFER_TRUNC)
    pts = lambda n: ((torch.rand(n, 3, generator=g) * 2 - 1) * 100.0).float().numpy()
    moved, pc1 = pts(n0), pts(n1)
    d_a, i_a = _hand_made(n0, n1, g, t2)
    d_b, i_b = _hand_made(n1, n0, g, t2)
    if n1 > FAN_IN:
        moved[FAN_ROW] = 0.0
        d_a[FAN_ROW], i_a[FAN_ROW] = np.inf, -1
        mag = (torch.rand(FAN_IN, 3, generator=g) * 60 + 1).float().numpy()
        pc1[:FAN_IN, 0] = mag[:, 0]
        pc1[:FAN_IN:2, 1], pc1[1:FAN_IN:2, 1] = mag[::2, 1], -mag[::2, 1]
        pc1[:FAN_IN, 2] = -mag[:, 2]
        d_b[:FAN_IN] = (torch.rand(FAN_IN, generator=g) * 0.25).numpy().astype(np.float32)
        d_b[:FAN_IN:8] = t2
        i_b[:FAN_IN] = FAN_ROW
    return SimpleNamespace(n0=n0, n1=n1, moved=moved, pc1=pc1, d_a=d_a, i_a=i_a, d_b=d_b, i_b=i_b, trunc=CHAMFER_TRUNC, t2=t2)


def chamfer_checks(c, got):
    """``got``: loss, grad [n0, 3] of himo_chamfer_trunc on chamfer_case c"""
    args = (c.moved, c.pc1, c.d_a, c.i_a, c.d_b, c.i_b, c.trunc)
    ref, t32 = chamfer(*args), chamfer(*args, dtype=np.float32)
    return [("chamfer", "grad", "f32", torch.as_tensor(got["grad"]).reshape(c.n0, 3), torch.from_numpy(ref["grad"]), torch.from_numpy(ref["e_grad"]),
             torch.from_numpy(t32["grad"]).double().reshape(c.n0, 3), False),
            ("chamfer", "loss", "f32", torch.tensor([got["loss"]], dtype=F64), torch.tensor([ref["loss"]], dtype=F64),
             torch.tensor([ref["e_loss"]], dtype=F64), None, False)]


# ---- the NSFP objective's scaling --------------------------------------------------------------------------------------------
NSFP_CASES = ((1, 1), (63, 1), (64, 255), (65, 256), (257, 257), (257, 0))
NSFP_TRUNC = 0.5
# a moved row = its pc1 row + one of these (multiples of 1/4): squared distances 0, 1/16, 3/16, 1/4 (kept: == trunc^2) and 5/16,
# 9/16 (the next lattice distances: dropped)
NSFP_OFFSETS = ((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.25, 0.0), (0.25, 0.25, 0.25), (0.0, -0.5, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.75),
                (-0.25, 0.5, 0.0), (0.0, 0.0, -0.5))


def nsfp_case(n0, n1):
    """lattice inputs of himo_nsfp_objective: pc1 on a lattice of spacing 2 m, moved rows at NSFP_OFFSETS from pc1 rows (several moved
    rows share a pc1 row when n0 > n1, and the other way round: exact ties, lowest row); out != 0 in multiples of 2^-10 and x0 = moved
    - out, so that float32(x0 + out) is the lattice point exactly.  x0 / out are [padded_rows(n0)][4], padding rows and column 3 zero"""
    g = torch.Generator().manual_seed(6000 + 7 * n0 + n1)
    k = max(n1, 1)
    idx = torch.randperm(12 * 12 * 3, generator=g)[:k].numpy()
    lat = np.stack([(idx % 12) * 2.0 - 11.0, (idx // 12 % 12) * 2.0 - 11.0, (idx // 144) * 2.0 - 2.0], 1).astype(np.float32)
    pc1 = lat[:n1]
    off = np.asarray(NSFP_OFFSETS, np.float32)
    moved = lat[np.arange(n0) % k] + off[(np.arange(n0) // k + np.arange(n0)) % len(off)]
    n_pad = no.padded_rows(n0)
    out = np.zeros((n_pad, 4), np.float32)
    o = (torch.randint(-1023, 1024, (n0, 3), generator=g).float() / 1024.0).numpy()
    o[o == 0] = 0.5
    out[:n0, :3] = o
    x0 = np.zeros((n_pad, 4), np.float32)
    x0[:n0, :3] = moved - o
    assert np.array_equal((x0 + out)[:n0, :3], moved)
    return SimpleNamespace(n0=n0, n1=n1, x0=x0, out=out, pc1=pc1, moved=moved.astype(np.float32), trunc=NSFP_TRUNC)


def nsfp_objective(c, dtype=np.float64, variant=None):
    """himo_nsfp_objective on nsfp_case c: moved = float32(x0 + out); exact nearest neighbours both ways (squared distances, ties to the
    lowest row; n1 == 0: +inf, -1); dout [n_pad][4] = n0 dL/dout (padding rows and column 3 zero); lp [tiles + ceil(n1 / 256)]: sum of
    the kept a of a tile, then (n0 / n1) sum of the kept b of 256 pc1 rows; cp: the real rows of a tile, then 0"""
    n0, n1, n_pad = c.n0, c.n1, len(c.x0)
    moved = (c.x0 + c.out)[:n0, :3].astype(np.float32)
    m, p = moved.astype(np.float64), c.pc1.astype(np.float64)
    tiles, blks = n_pad // 64, (n1 + 255) // 256
    t2 = np.float32(c.trunc) * np.float32(c.trunc)
    lp, cp = np.zeros(tiles + blks), np.zeros(tiles + blks, np.int32)
    cp[:tiles] = np.clip(n0 - 64 * np.arange(tiles), 0, 64)
    dout, e_dout, e_lp = np.zeros((n_pad, 4)), np.zeros((n_pad, 4)), np.zeros(tiles + blks)
    res = dict(moved=moved, lp=lp, cp=cp, dout=dout, e_dout=e_dout, e_lp=e_lp)
    if n1 == 0:
        res.update(d_a=np.full(n0, np.inf, np.float32), i_a=np.full(n0, -1, np.int32), d_b=np.zeros(0, np.float32), i_b=np.zeros(0, np.int32))
        return res
    d = ((m[:, None, :] - p[None, :, :]) ** 2).sum(2)
    ia, ib = d.argmin(1), d.argmin(0)
    a, b = d[np.arange(n0), ia], d[ib, np.arange(n1)]
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.array_equal(b.astype(np.float32).astype(np.float64), b)
    res.update(d_a=a.astype(np.float32), i_a=ia.astype(np.int32), d_b=b.astype(np.float32), i_b=ib.astype(np.int32))
    ka, kb = a <= t2, b <= t2
    wb = 1.0 if variant == "no_wb" else n0 / n1
    ibk, jb = ib[kb], np.nonzero(kb)[0]
    ak = np.where(ka, a, 0.0)
    pad = np.zeros(tiles * 64)
    pad[:n0] = ak
    lp[:tiles] = pad.reshape(tiles, 64).sum(1)
    e_lp[:tiles] = gamma64(6) * lp[:tiles]
    bk = np.zeros(blks * 256)
    bk[:n1] = np.where(kb, b, 0.0)
    lp[tiles:] = bk.reshape(blks, 256).sum(1) * wb
    e_lp[tiles:] = gamma64(10) * lp[tiles:]
    if dtype == np.float64:
        ta = np.where(ka[:, None], 2.0 * (m - p[ia]), 0.0)
        tb = 2.0 * wb * (m[ibk] - p[jb])
        S, Sabs, cnt = np.zeros((n0, 3)), np.zeros((n0, 3)), np.zeros((n0, 1))
        np.add.at(S, ibk, tb)
        np.add.at(Sabs, ibk, np.abs(tb))
        np.add.at(cnt, ibk, 1.0)
        g = ta + S
        ea = gamma(1) * np.abs(ta)
        eS = (U + 4 * U64) * Sabs * (1 + U) + cnt * 2.0 ** -41
        conv = (U + U64) * (np.abs(S) + eS)
        e = ea + eS + conv + U * (np.abs(g) + ea + eS + conv)
        live = (ka[:, None] | (cnt > 0)) & np.ones((1, 3), bool)
        dout[:n0, :3] = g
        e_dout[:n0, :3] = np.where(live, e + TINY, 0.0)
        return res
    ga = np.where(ka[:, None], np.float32(2.0) * (moved - c.pc1[ia]), np.float32(0.0)).astype(np.float32)
    q = np.rint((moved[ibk] - c.pc1[jb]).astype(np.float64) * (2.0 * wb * SCAT)).astype(np.int64)
    scat = np.zeros((n0, 3), np.int64)
    np.add.at(scat, ibk, q)
    dout[:n0, :3] = (ga + (scat.astype(np.float64) * (1.0 / SCAT)).astype(np.float32)).astype(np.float32)
    return res


def nsfp_checks(c, got):
    """``got``: dout [n_pad, 4], lp [parts] of himo_nsfp_objective on nsfp_case c: every dout element, every loss entry, and the loss
    through sum lp / n0.  (moved, the searches' results and cp are compared for EQUALITY by the caller: nsfp_objective(c) has them.)"""
    ref, t32 = nsfp_objective(c), nsfp_objective(c, np.float32)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    lp = np.asarray(got["lp"], np.float64)
    return [("nsfp_objective", "dout", "f32", f(got["dout"]), f(ref["dout"]), f(ref["e_dout"]), f(t32["dout"]), False),
            ("nsfp_objective", "lp", "f32", f(lp), f(ref["lp"]), f(ref["e_lp"]), None, False),
            ("nsfp_objective", "loss", "f32", f([lp.sum() / c.n0]), f([ref["lp"].sum() / c.n0]),
             f([(ref["e_lp"].sum() + gamma64(len(lp) + 1) * ref["lp"].sum()) / c.n0]), None, False)]


# ---- keep-best ---------------------------------------------------------------------------------------------------------------
KEEP_INIT = (math.inf, 0.0, 0.0, 0.0)


def keep_best_step(prev, loss, step, patience, min_delta, variant=None):
    """nsfp_keep_best_kernel: (best, best_iter, stale, stopped_at) after ``step`` and whether out is copied to best_out"""
    best, best_iter, stale0, stopped_at = prev
    stopped = stopped_at != 0.0
    better = (loss <= best - min_delta) if variant == "keep_le" else (loss < best - min_delta)
    improved = (not stopped) and better                      # (false for a NaN loss)
    stale = 0.0 if improved else stale0 + 1.0
    return (loss if improved else best, float(step) if improved else best_iter, stale0 if stopped else stale,
            stopped_at if stopped else (float(step) if (not improved and patience > 0 and stale >= patience) else 0.0)), improved


def keep_best_run(losses, patience, min_delta, variant=None):
    """-> [(state, improved)] after steps 1 .. T"""
    st, out = KEEP_INIT, []
    for t, loss in enumerate(losses, 1):
        st, imp = keep_best_step(st, float(loss), t, patience, min_delta, variant)
        out.append((st, imp))
    return out


NAN = float("nan")
# (losses, patience, min_delta): a strict improvement, one smaller than min_delta, a loss of exactly best - min_delta, a NaN, patience
# reached exactly (step 5), steps after the stop; an equal loss under min_delta 0 and patience 0 (never stops); patience 1
KEEP_SCRIPTS = (((4.0, 3.0, 2.875, 2.75, NAN, 1.0, 0.5), 3, 0.25),
                ((2.0, 2.0, 1.5, NAN, 1.5, 1.0, 3.0, 3.0, 3.0), 0, 0.0),
                ((1.0, 1.0, 0.5), 1, 0.0))


def verdict(fam, arith, got, ref, bnd, r32, case, cols=False):
    """nsf_oracle.verdict with the families' aggregate limits: conv_oracle.R[arith] for the products, grad_oracle.R_ELEM for the
    element-wise Chamfer / NSFP arithmetic (as tests/test_nsf_conformance_gpu.py passes for dt_loss and adam)"""
    return no.verdict(arith, got, ref, bnd, r32, case, limit=R_ELEM if fam in ("chamfer", "nsfp_objective") else None, cols=cols)
