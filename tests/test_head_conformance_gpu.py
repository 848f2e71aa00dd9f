"""Conformance of the per-point head over what its entry points admit: himo_gru_head_train, himo_gru_head_batch,
himo_gru_head_batch_folded, himo_gru_head_batch_guarded, himo_gru_head, himo_gru_head_backward, himo_head_gather and
himo_head_final (csrc/gruhead.hip, csrc/gruheadbwd.hip, csrc/head.hip).

For every call the library must either refuse it (the documented status, no output byte written) or return results within the
bounds of oracle/head_oracle.py against float64 -- the stage bound of every saved tensor against the kernel's own previous
save, the propagated bound end to end -- and within conv_oracle.R of the float32 twin, with the inputs bit-unchanged and no word
outside an output view written.  Operands and outputs live in NaN-filled guarded buffers (oracle/guarded.py): a read outside
an input view poisons a result, and NaN in a result is a failure of its own.  tests/test_head_oracle.py shows on the CPU that
these checks pass a correct head and fail the wrong ones.

Every case is tiny: a 16 x 16-cell grid, at most 200 points (head_oracle.scene: about 10 % dropped, among them the first row
and the last row of a block; shared cells; a point in cell 0).  Layouts are spread over the cases: img_pitch 32 / 96 (three
sweeps interleaved, the two pointers 32 and 64 floats into the pixel) / 112, dec_pitch 64 / 80, pc_stride 3 / 4 / 5.

Two weight sets (head_oracle.WEIGHT_SCALE, STAGE_SCALE): spec.init_params times 1 / 8, under which the propagated bounds are a
thousandth of the result, everywhere; and unscaled in himo_gru_head_train, where every stage check has both of its levels.
"""
import ctypes

import pytest
import torch

import conv_oracle as co
import head_oracle as ho
from guarded import Guarded, layout

pytestmark = pytest.mark.gpu

H, HX = ho.HIDDEN, ho.HX
STATS = {}        # (family, arith) -> [worst err / bound, worst rms ratio, checks, case of the first, case of the second]
KERNELS = {}      # kernel template instantiation -> calls that met it
REFUSED = []      # (family, case, status)
_REFS = {}

FWD_ROWS = (1, 63, 64, 65, 127, 128, 129, 200)
BWD_ROWS = (1, 31, 32, 33, 64, 65, 97)
LAYOUTS = ((32, 64, 3), (96, 80, 4), (112, 64, 5), (96, 64, 3), (32, 80, 5), (112, 80, 4))       # img_pitch, dec_pitch, pc_stride


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nhead conformance: per family and arithmetic, the largest err/bound and rms ratio over the matrix")
    for (fam, a), (w, r, n, wc, rc) in sorted(STATS.items()):
        print(f"  {fam:22s} {a:7s} err/bound {w:.3g}  rms ratio {r:.3g} (R {co.R[a]:g})  {n} checks\n    worst err/bound: {wc}\n    worst rms: {rc}")
    print("  kernels met: " + ", ".join(f"{k} x{v}" for k, v in sorted(KERNELS.items())))
    print(f"  refused: {len(REFUSED)}")
    for fam, case, st in REFUSED:
        print(f"    {fam}: {case}: status {st}")


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import model, train                 # noqa: F401  (registers the signatures)
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def _note(fam, arith, worst, rr, case):
    s = STATS.setdefault((fam, arith), [0.0, 0.0, 0, "", ""])
    if worst >= s[0]:
        s[0], s[3] = worst, case
    if rr >= s[1]:
        s[1], s[4] = rr, case
    s[2] += 1


def _met(kernel):
    KERNELS[kernel] = KERNELS.get(kernel, 0) + 1


def _ok(fam, arith, got, ref, bnd, ref32, case, aggregate=True):
    assert not bool(torch.isnan(torch.as_tensor(got)).any()), f"{case}: NaN in the result (a read outside an input view, or an output element never written)"
    good, worst, rr, report = ho.verdict(arith, got, ref, bnd, ref32, case, aggregate=aggregate)
    assert good, report
    _note(fam, arith, worst, rr, case)


def g2(gpu, values, pitch=None, off=0):
    """a [rows, cols] matrix at ``pitch`` (>= cols) words per row, ``off`` words past the aligned base; float32 or int32"""
    rows, cols = values.shape
    g = Guarded(layout(1, 1, 0, 0, rows, pitch or cols, cols), gpu, off=off)
    g.put(values if values.dtype == torch.int32 else values.float())
    return g


def gvec(gpu, values):
    return g2(gpu, values.reshape(1, -1))


def gout(gpu, n_stack, rows_view, rows_cap, c):
    """an output stack [n_stack][rows_cap][c] of which rows [0, rows_view) of every slice are the view"""
    return Guarded(layout(n_stack, n_stack, rows_cap * c, 0, rows_view, c, c), gpu)


class Call:
    """inputs bit-unchanged and nothing outside an output view written, after one library call"""

    def __init__(self, inputs, outputs, plain=()):
        self.inputs, self.outputs, self.plain = inputs, outputs, plain
        self.before = [g.buf.clone() for g in inputs]
        self.plain_before = [t.clone() for t in plain]

    def check(self, case):
        torch.cuda.synchronize()
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{case}: an input was written"
        for t, b in zip(self.plain, self.plain_before):
            assert torch.equal(t, b), f"{case}: a packed weight was written"
        for g in self.outputs:
            assert g.untouched_outside(), f"{case}: a write outside an output view (capacity rows, pitch gap or guard)"

    def refused(self, fam, case, st, allowed):
        torch.cuda.synchronize()
        assert st in allowed, f"{case}: status {st}, expected one of {allowed}"
        for g in self.outputs:
            assert g.untouched(), f"{case}: refused (status {st}) but wrote"
        REFUSED.append((fam, case, st))


# ---- weights -------------------------------------------------------------------------------------------------------------
def _pack(lib, gpu, w, fmt):
    w = w.float().contiguous().to(gpu)
    cin, cout = w.shape
    buf = torch.zeros(int(lib.himo_conv_packed_weight_bytes(1, cin, cout)) + 16, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    st = lib.himo_conv_pack_weights_ex(w.data_ptr(), 1, cin, cout, fmt, buf.data_ptr(), _s())
    assert st == 0, st
    torch.cuda.synchronize()
    return buf


class Weights:
    """the head's parameters on the device: small tensors guarded, packed copies plain (their layout is the packer's)"""

    def __init__(self, lib, gpu, scale=ho.WEIGHT_SCALE):
        self.W = W = ho.weights(0, scale)
        self.scale = scale
        self.g = {k: gvec(gpu, W[k]) for k in ("w_off", "b_off", "bzr", "bq", "b1", "b2")}
        self.g["w2"] = g2(gpu, W["w2"])
        w4 = torch.zeros(32, 4)
        w4[:, :3] = W["w2"]
        self.g["w2p4"] = g2(gpu, w4)
        self.pk, self.pkf, self.pkt = {}, {}, {}
        for fmt in (0, 1):
            self.pk[fmt] = {k: _pack(lib, gpu, W[k], fmt) for k in ("wzr", "wq", "w1")}
            self.pkf[fmt] = {k: _pack(lib, gpu, ho.fold(W["w_off"], W["b_off"], W[k]).float(), fmt) for k in ("wzr", "wq", "w1")}
        for fmt in (0, 2):
            self.pkt[fmt] = {k: _pack(lib, gpu, W[k].T, fmt) for k in ("wq", "wzr")}

    def guarded(self):
        return list(self.g.values())

    def plain(self):
        return [t for d in (self.pk, self.pkf, self.pkt) for f in d.values() for t in f.values()]


@pytest.fixture(scope="module")
def wts(lib, gpu):
    """spec.init_params times 1 / 8: the weights under which the propagated bounds mean something (head_oracle.WEIGHT_SCALE)"""
    return Weights(lib, gpu)


@pytest.fixture(scope="module")
def wts_net(lib, gpu):
    """spec.init_params unscaled: the weights under which the stage checks have their aggregate level (head_oracle.STAGE_SCALE)"""
    return Weights(lib, gpu, ho.STAGE_SCALE)


def split_encode(x):
    """float32 [..., C] (C % 16 == 0) -> (int32 words of the split activation format, float64 value h + l)"""
    h = x.half()
    l = (x - h.float()).half()
    g = x.shape[-1] // 16
    rec = torch.stack([h.reshape(*x.shape[:-1], g, 16), l.reshape(*x.shape[:-1], g, 16)], -2).reshape(*x.shape[:-1], 2 * x.shape[-1])
    return rec.view(torch.int32), h.double() + l.double()


# ---- scenes on the device ---------------------------------------------------------------------------------------------
class DevScene:
    def __init__(self, gpu, sc, lay, split=False, img=None):
        """``lay`` = (img_pitch, dec_pitch, pc_stride); split: the images in the split activation format; img: (img0, img1)
        to place for sc's"""
        self.sc, (self.img_pitch, self.dec_pitch, self.stride) = sc, lay
        n = sc["n"]
        i0, i1 = img if img is not None else (sc["img0"], sc["img1"])
        if split:
            i0, i1 = split_encode(i0)[0], split_encode(i1)[0]
        self.pid = g2(gpu, sc["pid"].reshape(1, -1))
        self.offsets = g2(gpu, sc["offsets"])
        if self.img_pitch == 96:                         # [history | pc0 | pc1] per cell, as the network lays its three sweeps out
            self.img = g2(gpu, torch.cat([i0, i1], 1), 96, off=32)
            self.p_img0, self.p_img1 = self.img.ptr, self.img.ptr + 4 * 32
            self.inputs = [self.img]
        else:
            self.img0, self.img1 = g2(gpu, i0, self.img_pitch), g2(gpu, i1, self.img_pitch)
            self.p_img0, self.p_img1 = self.img0.ptr, self.img1.ptr
            self.inputs = [self.img0, self.img1]
        self.dec = g2(gpu, sc["dec"], self.dec_pitch)
        self.xyz_t = g2(gpu, sc["xyz_t"])
        self.pts = g2(gpu, sc["pts"], self.stride)
        self.flow = Guarded(layout(1, 1, 0, 0, n, 3, 3), gpu)
        self.inputs += [self.pid, self.offsets, self.dec, self.xyz_t, self.pts]

    def sample(self):
        from himo_amd.seflow.model import HimoHeadSample
        return HimoHeadSample(self.sc["n"], self.pid.ptr, self.offsets.ptr, self.p_img0, self.p_img1, self.dec.ptr, self.xyz_t.ptr,
                              self.pts.ptr, self.stride, self.flow.ptr)


def _scene(n, seed=None):
    key = ("sc", n, seed)
    if key not in _REFS:
        _REFS[key] = ho.scene(n if seed is None else seed, n)
    return _REFS[key]


def _prop(arith, sc, W, iters, folded=False, tag=None):
    key = ("prop", arith, tag if tag is not None else sc["n"], iters, folded, float(W["wq"].abs().sum()))
    if key not in _REFS:
        _REFS[key] = ho.propagate_forward(arith, sc, W, iters, folded)
    return _REFS[key]


def _c64(n):
    return (n + 63) // 64 * 64


# ---- himo_gru_head_train --------------------------------------------------------------------------------------------------
class Saved:
    def __init__(self, gpu, n, iters, rows):
        v = _c64(n)
        self.g = dict(hx=gout(gpu, iters + 1, v, rows, HX), rhx=gout(gpu, iters, v, rows, HX), z=gout(gpu, iters, v, rows, H),
                      r=gout(gpu, iters, v, rows, H), q=gout(gpu, iters, v, rows, H), pre1=gout(gpu, 1, v, rows, 32),
                      y1=gout(gpu, 1, v, rows, 32), res=gout(gpu, 1, v, rows, 4))
        from himo_amd.seflow.train import HeadSaved
        self.c = HeadSaved(rows, *(self.g[k].ptr for k in ("hx", "rhx", "z", "r", "q", "pre1", "y1", "res")))

    def outputs(self):
        return list(self.g.values())


def _train_call(lib, wts, ds, fmt, iters, sv, w2_pitch=3, nonfinite=None, **over):
    g = wts.g
    a = dict(n=ds.sc["n"], pid=ds.pid.ptr, offsets=ds.offsets.ptr, img0=ds.p_img0, img1=ds.p_img1, img_pitch=ds.img_pitch, dec=ds.dec.ptr,
             dec_pitch=ds.dec_pitch, w_off=g["w_off"].ptr, b_off=g["b_off"].ptr, wzr=wts.pk[fmt & 1]["wzr"].data_ptr(), bzr=g["bzr"].ptr,
             wq=wts.pk[fmt & 1]["wq"].data_ptr(), bq=g["bq"].ptr, w1=wts.pk[fmt & 1]["w1"].data_ptr(), b1=g["b1"].ptr,
             w2=g["w2p4" if w2_pitch == 4 else "w2"].ptr, w2_pitch=w2_pitch, b2=g["b2"].ptr, iters=iters, fmt=fmt,
             saved=ctypes.addressof(sv.c), nonfinite=nonfinite)
    a.update(over)
    return lib.himo_gru_head_train(*a.values(), _s())


def _train_case(lib, gpu, wts, fmt, n, iters, lay, w2_pitch, cap):
    arith = ho.FWD_ARITH[fmt]
    W, sc = wts.W, _scene(n)
    rows = _c64(n) + cap
    agg = wts.scale == ho.STAGE_SCALE                     # head_oracle.STAGE_SCALE: where the stages' aggregate level applies
    case = f"train gru_head_kernel<{3 - fmt}, 12, true> weights x{wts.scale:g} n={n} iters={iters} rows={rows} img_pitch={lay[0]} dec_pitch={lay[1]} w2_pitch={w2_pitch}"
    ds, sv = DevScene(gpu, sc, lay), Saved(gpu, n, iters, rows)
    word = torch.zeros(1, dtype=torch.int32, device=gpu)
    c = Call(ds.inputs + wts.guarded(), sv.outputs(), wts.plain())
    st = _train_call(lib, wts, ds, fmt, iters, sv, w2_pitch, word.data_ptr())
    assert st == 0, f"{case}: status {st}"
    c.check(case)                                        # rows from ceil64(n) up to ``rows`` lie outside the views: untouched
    _met(f"gru_head_kernel<{3 - fmt}, 12, true>")
    assert int(word) == 0, f"{case}: the non-finite word was set on finite results"
    full = {k: g.get() for k, g in sv.g.items()}          # [stack, ceil64(n), c]
    got = {k: [full[k][t, :n] for t in range(full[k].shape[0])] for k in ("hx", "rhx", "z", "r", "q")}
    got.update(pre1=full["pre1"][0, :n], y1=full["y1"][0, :n], res=full["res"][0, :n])
    for name, a, ref, bnd, r32 in ho.stage_checks(arith, sc, W, got, iters):
        _ok(f"train {name}", arith, a, ref, bnd, r32, f"{case} {name}", aggregate=agg or name in ho.BARE_STAGES)
    p = _prop(arith, sc, W, iters)
    _ok("train res end to end", arith, got["res"][:, :3], p["res"], p["e_res"], None, case + " res end to end")
    res = full["res"][0]
    assert not bool((res[:n][sc["pid"] < 0] != 0).any()), f"{case}: res of a dropped row is not zero"
    assert not bool((res[n:] != 0).any()), f"{case}: res of a padding row is not zero"
    assert not bool((res[:, 3] != 0).any()), f"{case}: res column 3 is not zero"
    for k in ("hx", "rhx"):
        assert bool(torch.isfinite(full[k][:, n:]).all()), f"{case}: a padding row of {k} is not finite (the weight gradients read it)"


@pytest.mark.parametrize("fmt", [0, 1])
def test_gru_head_train(lib, gpu, wts, wts_net, fmt):
    """every row count around the 64-row block, iters 1..4, both w2 pitches, exact rows and 128 rows of capacity, the layouts;
    with the network's weights (both levels of every stage check) and with the 1 / 8 weights (a res bound that means something)"""
    for i, n in enumerate(FWD_ROWS):
        _train_case(lib, gpu, wts_net, fmt, n, 1 + (i + fmt) % 4, LAYOUTS[i % 6], 3 + (i + fmt) % 2, 128 * ((i // 2 + fmt) % 2))
        _train_case(lib, gpu, wts, fmt, n, 1 + (i + fmt + 2) % 4, LAYOUTS[(i + 3) % 6], 3 + (i + fmt + 1) % 2, 128 * ((i // 2 + fmt + 1) % 2))
    for iters in (1, 2, 3, 4):                              # every iteration count once more on a partial last block with capacity
        _train_case(lib, gpu, wts, fmt, 65, iters, LAYOUTS[(iters + 2 * fmt) % 6], 3 + iters % 2, 128 * (iters % 2))


def test_gru_head_train_nonfinite_word(lib, gpu, wts):
    """d_nonfinite: NULL is accepted; an infinite b2 entry sets bit 0; the kernel ORs, so a word preset to 2 ends as 3"""
    n, iters = 65, 2
    sc = _scene(n)
    for fmt in (0, 1):
        ds, sv = DevScene(gpu, sc, LAYOUTS[fmt]), Saved(gpu, n, iters, 128)
        c = Call(ds.inputs + wts.guarded(), sv.outputs(), wts.plain())
        assert _train_call(lib, wts, ds, fmt, iters, sv, 3, None) == 0
        c.check(f"train fmt={fmt} d_nonfinite NULL")
        p = _prop(ho.FWD_ARITH[fmt], sc, wts.W, iters)
        _ok("train res end to end", ho.FWD_ARITH[fmt], sv.g["res"].get()[0, :n, :3], p["res"], p["e_res"], None, f"train fmt={fmt} d_nonfinite NULL")
        b2 = gvec(gpu, torch.tensor([0.0, float("inf"), 0.0]))
        for preset, want in ((0, 1), (2, 3)):
            word = torch.full((1,), preset, dtype=torch.int32, device=gpu)
            sv2 = Saved(gpu, n, iters, 128)
            assert _train_call(lib, wts, ds, fmt, iters, sv2, 3, word.data_ptr(), b2=b2.ptr) == 0
            torch.cuda.synchronize()
            assert int(word) == want, f"train fmt={fmt}: word {preset} -> {int(word)} with an infinite b2, expected {want}"


# ---- the inference entry points -------------------------------------------------------------------------------------------
ENTRIES = ("batch", "folded", "guarded", "guarded_folded", "single")


def _infer_call(lib, wts, entry, scenes, fmt, iters, img_split=0, word=None, lay=None, **over):
    """one launch over ``scenes`` (DevScene or None for an empty sample given null pointers)"""
    from himo_amd.seflow.model import HimoHeadSample
    g = wts.g
    folded = entry in ("folded", "guarded_folded")
    pk = (wts.pkf if folded else wts.pk)[fmt & 1]
    arr = (HimoHeadSample * max(len(scenes), 1))()
    for i, d in enumerate(scenes):
        arr[i] = d.sample() if d is not None else HimoHeadSample(0, None, None, None, None, None, None, None, 3, None)
    first = next(d for d in scenes if d is not None)
    img_pitch, dec_pitch = lay if lay is not None else (first.img_pitch, first.dec_pitch)
    a = dict(wzr=pk["wzr"].data_ptr(), bzr=g["bzr"].ptr, wq=pk["wq"].data_ptr(), bq=g["bq"].ptr, w1=pk["w1"].data_ptr(), b1=g["b1"].ptr,
             w2=g["w2"].ptr, b2=g["b2"].ptr)
    a.update({k: v for k, v in over.items() if k in a})
    n_samples = over.get("n_samples", len(scenes))
    off = (over.get("w_off", g["w_off"].ptr), over.get("b_off", g["b_off"].ptr))
    tail = (iters, fmt, img_split)
    if entry == "single":
        d = first
        return lib.himo_gru_head(d.sc["n"], d.pid.ptr, d.offsets.ptr, d.p_img0, d.p_img1, img_pitch, d.dec.ptr, dec_pitch, *off, *a.values(),
                                 d.xyz_t.ptr, d.pts.ptr, over.get("pc_stride", d.stride), d.flow.ptr, iters, fmt, _s())
    head = (n_samples, ctypes.addressof(arr), img_pitch, dec_pitch)
    if entry == "batch":
        return lib.himo_gru_head_batch(*head, *off, *a.values(), *tail, _s())
    if entry == "folded":
        return lib.himo_gru_head_batch_folded(*head, *a.values(), *tail, _s())
    if entry == "guarded":
        return lib.himo_gru_head_batch_guarded(*head, *off, *a.values(), *tail, word, _s())
    return lib.himo_gru_head_batch_guarded(*head, None, None, *a.values(), *tail, word, _s())


def _kernel(entry, fmt):
    return f"gru_head_kernel<{3 - fmt}, {9 if 'folded' in entry else 12}>"


def _check_flow(fam, arith, d, p, case):
    sc = d.sc
    flow = d.flow.get().reshape(sc["n"], 3)
    _ok(fam, arith, flow, p["flow"], p["e_flow"], None, case)
    dropped = sc["pid"] < 0
    assert torch.equal(flow[dropped], (sc["xyz_t"] - sc["pts"])[dropped]), f"{case}: a dropped point's flow is not xyz_t - pts bitwise"
    return flow


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("entry", ENTRIES)
def test_inference_one_sample(lib, gpu, wts, entry, fmt):
    """iters 0, 1, 4 and 6 over the row counts and layouts, one sample per launch"""
    arith, folded = ho.FWD_ARITH[fmt], "folded" in entry
    k = ENTRIES.index(entry)
    for i, n in enumerate(FWD_ROWS):
        iters = (0, 1, 4, 6)[(i + k + fmt) % 4]
        lay = LAYOUTS[(i + k) % 6]
        case = f"{entry} {_kernel(entry, fmt)} n={n} iters={iters} img_pitch={lay[0]} dec_pitch={lay[1]} pc_stride={lay[2]}"
        d = DevScene(gpu, _scene(n), lay)
        word = torch.zeros(1, dtype=torch.int32, device=gpu)
        c = Call(d.inputs + wts.guarded(), [d.flow], wts.plain())
        st = _infer_call(lib, wts, entry, [d], fmt, iters, word=word.data_ptr())
        assert st == 0, f"{case}: status {st}"
        c.check(case)
        _met(_kernel(entry, fmt))
        _check_flow("flow folded" if folded else "flow", arith, d, _prop(arith, d.sc, wts.W, iters, folded), case)
        assert int(word) == 0, f"{case}: the non-finite word was set on finite results"


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("entry", ["batch", "folded"])
def test_inference_batches(lib, gpu, wts, entry, fmt):
    """three samples with an empty one in the middle (null pointers), and 16 samples of sizes from {0, 1, 63, 64, 65, 129}, each also
    bit-equal to the same entry point called on it alone (one kernel; a block's arithmetic does not depend on its block id)"""
    arith, folded, iters = ho.FWD_ARITH[fmt], entry == "folded", 4
    fam = "flow folded" if folded else "flow"
    lay = LAYOUTS[1 + fmt]
    ds = [DevScene(gpu, _scene(65), lay), None, DevScene(gpu, _scene(129), lay)]
    live = [d for d in ds if d is not None]
    c = Call([g for d in live for g in d.inputs] + wts.guarded(), [d.flow for d in live], wts.plain())
    assert _infer_call(lib, wts, entry, ds, fmt, iters) == 0
    c.check(f"{entry} fmt={fmt} 3 samples")
    _met(_kernel(entry, fmt))
    for d in live:
        _check_flow(fam, arith, d, _prop(arith, d.sc, wts.W, iters, folded), f"{entry} fmt={fmt} 3 samples, empty middle: n={d.sc['n']}")

    sizes = [65, 0, 1, 129, 63, 64, 0, 65, 1, 129, 64, 63, 0, 129, 1, 65]
    ds = [DevScene(gpu, _scene(n), lay) if n else None for n in sizes]
    live = [d for d in ds if d is not None]
    c = Call([g for d in live for g in d.inputs] + wts.guarded(), [d.flow for d in live], wts.plain())
    assert _infer_call(lib, wts, entry, ds, fmt, iters) == 0
    c.check(f"{entry} fmt={fmt} 16 samples")
    _met(_kernel(entry, fmt))
    alone = {}
    for i, d in enumerate(ds):
        if d is None:
            continue
        n = d.sc["n"]
        case = f"{entry} fmt={fmt} 16 samples: sample {i} n={n}"
        flow = _check_flow(fam, arith, d, _prop(arith, d.sc, wts.W, iters, folded), case)
        if n not in alone:
            one = DevScene(gpu, d.sc, lay)
            assert _infer_call(lib, wts, entry, [one], fmt, iters) == 0
            torch.cuda.synchronize()
            alone[n] = one.flow.words()
        assert torch.equal(d.flow.words(), alone[n]), f"{case}: differs bitwise from the same sample launched alone"


def test_split_image_layout_gives_the_float_layout_bits(lib, gpu, wts):
    """packed_format 1: images in the split activation format give the bits of the float32-layout call on the decoded image"""
    for entry, lay, n in (("batch", LAYOUTS[0], 129), ("folded", LAYOUTS[1], 65), ("guarded", LAYOUTS[3], 200)):
        sc = _scene(n)
        dec0, dec1 = split_encode(sc["img0"])[1].float(), split_encode(sc["img1"])[1].float()
        a = DevScene(gpu, sc, lay, split=True)
        b = DevScene(gpu, sc, lay, img=(dec0, dec1))
        case = f"img_split {entry} n={n} img_pitch={lay[0]}"
        for d, split in ((a, 1), (b, 0)):
            c = Call(d.inputs + wts.guarded(), [d.flow], wts.plain())
            assert _infer_call(lib, wts, entry, [d], 1, 4, img_split=split) == 0, case
            c.check(case)
            _met(_kernel(entry, 1))
        assert torch.equal(a.flow.words(), b.flow.words()), f"{case}: the two layouts differ bitwise"
        sc2 = dict(sc, img0=dec0, img1=dec1)
        _check_flow("flow folded" if entry == "folded" else "flow", "f16x2", b, _prop("f16x2", sc2, wts.W, 4, entry == "folded", tag=("dec", n)), case)


def test_guarded_nonfinite_word(lib, gpu, wts):
    """both forms: an infinite b2 entry sets bit 0 of the word, the other bits stay (OR); NULL is accepted"""
    sc = _scene(65)
    b2 = gvec(gpu, torch.tensor([float("inf"), 0.0, 0.0]))
    for entry in ("guarded", "guarded_folded"):
        for fmt in (0, 1):
            d = DevScene(gpu, sc, LAYOUTS[2])
            assert _infer_call(lib, wts, entry, [d], fmt, 1, word=None) == 0
            _check_flow("flow folded" if "folded" in entry else "flow", ho.FWD_ARITH[fmt], d, _prop(ho.FWD_ARITH[fmt], sc, wts.W, 1, "folded" in entry),
                        f"{entry} fmt={fmt} d_nonfinite NULL")
            for preset, want in ((0, 1), (2, 3)):
                word = torch.full((1,), preset, dtype=torch.int32, device=gpu)
                assert _infer_call(lib, wts, entry, [d], fmt, 1, word=word.data_ptr(), b2=b2.ptr) == 0
                torch.cuda.synchronize()
                assert int(word) == want, f"{entry} fmt={fmt}: word {preset} -> {int(word)} with an infinite b2, expected {want}"


# ---- himo_gru_head_backward -------------------------------------------------------------------------------------------
def _bwd_inputs(n, iters, W):
    """the float64-reference states rounded to float32 (no dependence on the forward kernel), a random dhx_last with zero rows
    for dropped points; padding rows [n, ceil64(n)): the states of point n - 1, dhx_last zero"""
    key = ("bwd", n, iters)
    if key not in _REFS:
        sc = _scene(n)
        ref = ho.forward(sc, W, iters)
        sv = {k: [a.float() for a in ref[k]] for k in ("hx", "z", "r", "q")}
        d = torch.randn(n, HX, generator=torch.Generator().manual_seed(500 + n))
        d[sc["pid"] < 0] = 0
        _REFS[key] = (sv, d)
    return _REFS[key]


def _padded(a, rows):
    return torch.cat([a, a[-1:].expand(rows - a.shape[0], -1)], 0)


def _bwd_case(lib, gpu, wts, fmt, n, iters, cap, **over):
    from himo_amd.seflow.train import HeadSaved
    arith = ho.BWD_ARITH.get(fmt)                        # None: a format the entry point refuses
    sv, d = _bwd_inputs(n, iters, wts.W)
    v = _c64(n)
    rows = v + cap
    case = f"backward gru_head_bwd_kernel<{3 if fmt == 0 else 2}> n={n} iters={iters} rows={rows}"

    def stack(k, c):                                        # [len][rows][c], rows [0, v) in the view
        g = gout(gpu, len(sv[k]), v, rows, c)
        g.put(torch.stack([_padded(a, v) for a in sv[k]]))
        return g
    gi = dict(hx=stack("hx", HX), z=stack("z", H), r=stack("r", H), q=stack("q", H))
    gd = gout(gpu, 1, v, rows, HX)
    gd.put(torch.cat([d, torch.zeros(v - n, HX)], 0))
    daq, dazr, dhx0 = gout(gpu, iters, v, rows, H), gout(gpu, iters, v, rows, 2 * H), gout(gpu, 1, v, rows, HX)
    saved = HeadSaved(rows, gi["hx"].ptr, None, gi["z"].ptr, gi["r"].ptr, gi["q"].ptr, None, None, None)
    c = Call(list(gi.values()) + [gd], [daq, dazr, dhx0], wts.plain())
    a = dict(n=n, iters=iters, dhx=gd.ptr, saved=ctypes.addressof(saved), wq=wts.pkt[fmt if fmt in (0, 2) else 0]["wq"].data_ptr(),
             wzr=wts.pkt[fmt if fmt in (0, 2) else 0]["wzr"].data_ptr(), fmt=fmt, daq=daq.ptr, dazr=dazr.ptr, dhx0=dhx0.ptr)
    if "rows" in over:
        saved.rows = over.pop("rows")
    if "call_iters" in over:                             # an iteration count the buffers were not sized for: refused before any access
        a["iters"] = over.pop("call_iters")
    if over.pop("null_saved", False):
        saved.d_z = None
    a.update(over)
    st = lib.himo_gru_head_backward(*a.values(), _s())
    return st, c, case, (daq, dazr, dhx0), arith


def _bwd_ok(lib, gpu, wts, fmt, n, iters, cap):
    st, c, case, outs, arith = _bwd_case(lib, gpu, wts, fmt, n, iters, cap)
    assert st == 0, f"{case}: status {st}"
    c.check(case)                                        # rows beyond ceil64(n) lie outside the views: untouched
    _met(f"gru_head_bwd_kernel<{3 if fmt == 0 else 2}>")
    sv, d = _bwd_inputs(n, iters, wts.W)
    key = ("bprop", arith, n, iters)
    if key not in _REFS:
        _REFS[key] = (ho.propagate_backward(arith, d, sv, wts.W, iters), ho.backward(d, sv, wts.W, iters, torch.float32))
    p, tw = _REFS[key]
    daq, dazr, dhx0 = (g.get() for g in outs)
    _ok("backward daq", arith, daq[:, :n], p["daq"], p["e_daq"], tw[0], case + " daq")
    _ok("backward dazr", arith, dazr[:, :n], p["dazr"], p["e_dazr"], tw[1], case + " dazr")
    _ok("backward dhx0", arith, dhx0[0, :n], p["dhx0"], p["e_dhx0"], tw[2], case + " dhx0")
    assert not bool((daq[:, n:] != 0).any()), f"{case}: a padding row of daq is not zero"
    assert not bool((dazr[:, n:] != 0).any()), f"{case}: a padding row of dazr is not zero"


@pytest.mark.parametrize("fmt", [0, 2])
def test_gru_head_backward(lib, gpu, wts, fmt):
    """32-row blocks sweeping whole 64-row blocks: every row count around both, iters 1..4, exact rows and capacity"""
    for i, n in enumerate(BWD_ROWS):
        _bwd_ok(lib, gpu, wts, fmt, n, 1 + (i + fmt // 2) % 4, 128 * ((i + fmt // 2) % 2))
    for iters in (1, 2, 3):
        _bwd_ok(lib, gpu, wts, fmt, 33, iters, 128 * (iters % 2))


# ---- himo_head_gather, himo_head_final ---------------------------------------------------------------------------------
def test_head_gather_and_final(lib, gpu, wts):
    """the unfused pair: gathered columns are bit copies (zeros for dropped points), the x columns -- computed for every point,
    dropped or not, as the fused kernels do (include/himo_amd.h) -- within their counted roundings, rhx's x columns the same
    bits; himo_head_final within the dec2 chain bound, pose flow alone for dropped points"""
    W = wts.W
    for i, n in enumerate((1, 65, 200)):
        lay = LAYOUTS[(2 * i + 1) % 6]
        sc = _scene(n)
        d = DevScene(gpu, sc, lay)
        pitch = 192 + 8 * i
        hx, rhx = Guarded(layout(1, 1, 0, 0, n, pitch, HX), gpu), Guarded(layout(1, 1, 0, 0, n, pitch, 64), gpu, off=128)
        case = f"head_gather n={n} img_pitch={lay[0]} dec_pitch={lay[1]} pitch={pitch}"
        c = Call(d.inputs + wts.guarded(), [hx, rhx])
        st = lib.himo_head_gather(n, d.pid.ptr, d.offsets.ptr, d.p_img0, d.p_img1, lay[0], d.dec.ptr, lay[1], wts.g["w_off"].ptr,
                                  wts.g["b_off"].ptr, hx.ptr, rhx.ptr - 4 * 128, pitch, _s())
        assert st == 0, f"{case}: status {st}"
        c.check(case)
        _met("head_gather_kernel")
        got = hx.get().reshape(n, HX)
        g, g32 = ho.gather(sc, W), ho.gather(sc, W, torch.float32)
        _ok("gather", "f32", got[:, :H], g[:, :H], torch.zeros(n, H, dtype=torch.float64), None, case + " gathered columns")
        _ok("gather x", "f32", got[:, H:], g[:, H:], ho.x_bound(sc["offsets"], W), g32[:, H:], case + " x columns")
        assert torch.equal(rhx.words().reshape(n, 64), hx.words().reshape(n, HX)[:, H:]), f"{case}: rhx[:, 128:] differs from hx[:, 128:]"

        y1 = torch.randn(n, 32, generator=torch.Generator().manual_seed(n))
        gy = g2(gpu, y1, 32 + 4 * i)
        case = f"head_final n={n} y1_pitch={32 + 4 * i} pc_stride={lay[2]}"
        c = Call(d.inputs + wts.guarded() + [gy], [d.flow])
        st = lib.himo_head_final(n, gy.ptr, 32 + 4 * i, wts.g["w2"].ptr, wts.g["b2"].ptr, d.pid.ptr, d.xyz_t.ptr, d.pts.ptr, lay[2], d.flow.ptr, _s())
        assert st == 0, f"{case}: status {st}"
        c.check(case)
        _met("head_final_kernel")
        live = (sc["pid"] >= 0)[:, None]
        pf = sc["xyz_t"].double() - sc["pts"].double()
        z3 = torch.zeros(n, 3, dtype=torch.float64)
        res = torch.where(live, y1.double() @ W["w2"].double() + W["b2"].double(), z3)
        eres = torch.where(live, ho.dec2_bound(y1, W), z3)
        # pose_flow rounds once, the sum once more (head.hip:77-78)
        bnd = eres + co.U * pf.abs() + torch.where(live, co.U * (pf.abs() * (1 + co.U) + res.abs() + eres), z3) + ho.TINY
        flow = d.flow.get().reshape(n, 3)
        _ok("head_final", "f32", flow, pf + res, bnd, None, case)
        dropped = sc["pid"] < 0
        assert torch.equal(flow[dropped], (sc["xyz_t"] - sc["pts"])[dropped]), f"{case}: a dropped point's flow is not xyz_t - pts bitwise"


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(lib, gpu, wts):
    """every documented refusal returns its status and writes no byte"""
    from himo_amd import _lib
    INV = (_lib.ERR_INVALID_ARGUMENT,)
    n, sc = 65, _scene(65)
    d = DevScene(gpu, sc, LAYOUTS[0])
    d16 = DevScene(gpu, sc, (40, 64, 3))                     # an image pitch that is no multiple of 16

    def train(name, fmt=0, iters=2, rows=128, ds=d, w2_pitch=3, **over):
        sv = Saved(gpu, n, max(min(iters, 4), 1), max(_c64(n), rows // 64 * 64))
        sv.c.rows = rows
        if over.pop("null_saved", False):
            sv.c.d_q = None
        c = Call([], sv.outputs())
        c.refused("gru_head_train", name, _train_call(lib, wts, ds, fmt, iters, sv, w2_pitch, None, **over), INV)

    train("iters 0", iters=0)
    train("iters 5", iters=5)
    train("packed_format 2", fmt=2)
    train("img_pitch 31", img_pitch=31)
    train("dec_pitch 63", dec_pitch=63)
    train("w2_pitch 5", w2_pitch=5)
    train("rows not a multiple of 64", rows=160)
    train("rows below ceil64(n)", rows=64)
    train("packed weights 8 bytes off alignment", wq=wts.pk[0]["wq"].data_ptr() + 8)
    train("a null saved tensor", null_saved=True)

    def infer(name, entry="batch", fmt=0, iters=2, ds=d, img_split=0, scenes=None, **over):
        scenes = [ds] if scenes is None else scenes
        c = Call([], [s.flow for s in scenes if s is not None])
        c.refused("gru_head " + entry, name, _infer_call(lib, wts, entry, scenes, fmt, iters, img_split=img_split, **over), INV)

    for entry in ("batch", "folded", "guarded", "guarded_folded"):
        infer("packed_format 2", entry, fmt=2)
        infer("img_split with packed_format 0", entry, fmt=0, img_split=1)
        infer("img_split with img_pitch 40", entry, fmt=1, img_split=1, ds=d16)
        infer("img_pitch 31", entry, lay=(31, 64))
        infer("dec_pitch 63", entry, lay=(32, 63))
        infer("n_samples 17", entry, scenes=[d], n_samples=17)
        infer("a packed weight 8 bytes off alignment", entry, w1=(wts.pkf if "folded" in entry else wts.pk)[0]["w1"].data_ptr() + 8)
    d2 = DevScene(gpu, sc, LAYOUTS[0])
    d2.stride = 2
    infer("pc_stride 2", "batch", ds=d2)
    infer("pc_stride 2", "single", ds=d2)
    infer("packed_format 2", "single", fmt=2)
    infer("d_w_off without d_b_off", "guarded", b_off=None)
    infer("d_b_off without d_w_off", "guarded", w_off=None)
    infer("iters -1", "batch", iters=-1)

    for name, kw in (("packed_format 1", dict(fmt=1)), ("iters 0", dict(iters=0)), ("iters 5", dict(iters=5)),
                     ("rows not a multiple of 64", dict(rows=160)), ("rows below ceil64(n)", dict(rows=64)),
                     ("a null saved tensor", dict(null_saved=True)),
                     ("packed weights 8 bytes off alignment", dict(wq=wts.pkt[0]["wq"].data_ptr() + 8))):
        fmt, iters = kw.pop("fmt", 0), kw.pop("iters", 2)
        if iters == 0:
            st, c, case, outs, _ = _bwd_case(lib, gpu, wts, fmt, n, 1, 0, call_iters=0, **kw)
        elif iters == 5:
            st, c, case, outs, _ = _bwd_case(lib, gpu, wts, fmt, n, 4, 0, call_iters=5, **kw)
        else:
            st, c, case, outs, _ = _bwd_case(lib, gpu, wts, fmt, n, iters, 0, **kw)
        c.refused("gru_head_backward", name, st, INV)
