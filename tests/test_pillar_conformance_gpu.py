"""Conformance of the pillar stage (csrc/pillar.hip) through its exported entry points, called directly: himo_pillarize,
himo_pillarize_multi(_ex), himo_pillar_occupancy_reset, himo_pillar_features_multi, himo_pfn_bn_stats(_multi, _groups),
himo_pfn_backward, himo_pfn_backward_bn(_multi, _groups), himo_head_scatter and the three workspace queries.

The discrete parts (transformed points, cells, offsets, per-cell ascending lists, scatter sums, the split record) are compared bit
for bit with the float32 emulation of oracle/pillar_oracle.py; the image, the BatchNorm statistics and the gradients against its
float64 references, within the derived worst-case bound and the aggregate ratio.  Every operand, output and workspace lives in a
NaN-filled guarded buffer (oracle/guarded.py); workspaces have exactly the size the library's own query returns; after every call
the inputs are bit-unchanged and nothing outside an output view or the workspace is written.  Refusals are cases the host code
returns for before any launch (read in pillar.hip): documented status, no output word written.
"""
import ctypes

import numpy as np
import pytest
import torch

import pillar_oracle as po
from guarded import Guarded, layout

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS, MOM = 1e-3, 0.1
INVALID, WORKSPACE, UNSUPPORTED = 1, 3, 6
STATS = {}        # family -> [worst err / bound, worst rms ratio, checks]
MET = {}          # entry point -> calls
REFUSED = []      # (entry point, case, status)
_SCENES = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\npillar conformance: per family, the largest err/bound and rms ratio over the matrix")
    for fam, (w, r, n) in sorted(STATS.items()):
        print(f"  {fam:28s} err/bound {w:.3g}  rms ratio {r:.3g}  {n} checks")
    print("  entry points met: " + ", ".join(f"{k} x{v}" for k, v in sorted(MET.items())))
    print(f"  refused: {len(REFUSED)}")
    for fn, case, st in REFUSED:
        print(f"    {fn}: {case}: status {st}")


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import model, train                 # noqa: F401  (registers the signatures)
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def call(lib, name, *args):
    MET[name] = MET.get(name, 0) + 1
    return getattr(lib, name)(*args)


def note(fam, worst, rr=0.0):
    s = STATS.setdefault(fam, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], worst), max(s[1], rr), s[2] + 1


def fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = po.build_scene(name) + (po.build_scene(name, seed=1)[2],)
    return _SCENES[name]


def grows(gpu, values, pitch=None, off=0, dtype=torch.float32):
    """[rows, cols] at ``pitch`` floats per row, ``off`` floats into the buffer; NaN-filled when values is a shape"""
    shape = values if isinstance(values, tuple) else values.shape
    g = Guarded(layout(1, 1, 0, 0, shape[0], pitch or shape[1], shape[1]), gpu, off=off)
    if not isinstance(values, tuple) and shape[0]:
        g.put(torch.from_numpy(np.ascontiguousarray(values)).to(dtype))
    return g


def gbytes(gpu, nbytes):
    return Guarded(layout(1, 1, 0, 0, 1, max((int(nbytes) + 3) // 4, 1), (int(nbytes) + 3) // 4), gpu)


class Sweep:
    """one sweep's guarded buffers: points at a row stride, per-point outputs, its 32 image channels, its workspace"""

    def __init__(self, lib, gpu, grid, pts, T, stride=3, pitch=32, choff=0, ws_points=None, keep=None):
        self.grid, self.pts, self.T, self.n, self.stride, self.pitch = grid, pts, np.ascontiguousarray(T, F32), pts.shape[0], stride, pitch
        n = self.n
        self.d_pts = grows(gpu, pts, stride)
        self.xyz, self.pid, self.off = grows(gpu, (n, 3)), grows(gpu, (n, 1)), grows(gpu, (n, 3))
        self.img = keep.img if keep else grows(gpu, (grid.cells, 32), pitch, choff)      # keep: a persistent image and workspace
        self.ws_bytes = int(call(lib, "himo_pillar_workspace_bytes", n if ws_points is None else ws_points, grid.W, grid.H))
        assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
        self.ws = keep.ws if keep else gbytes(gpu, self.ws_bytes)                       # starts NaN-filled
        self.rng, self.vox, self.cen = (np.ascontiguousarray(a, F32) for a in (grid.vmin, grid.voxel, grid.centre))

    def struct(self):
        from himo_amd.seflow.model import HimoSweep
        s = HimoSweep(n=self.n, d_pts=self.d_pts.ptr, pc_stride=self.stride, d_xyz_t=self.xyz.ptr, d_pid=self.pid.ptr,
                      d_offsets=self.off.ptr, d_image=self.img.ptr, d_workspace=self.ws.ptr)
        s.transform[:] = [float(v) for v in self.T.reshape(-1)]
        return s

    def outputs(self):
        return [self.xyz, self.pid, self.off, self.img]

    def lists(self):
        """the per-cell lists the forward pass left in the workspace (layout of pillar_ws / carve_bwd in pillar.hip)"""
        r16 = lambda b: (b + 15) // 16 * 16
        cells, n = self.grid.cells, self.n
        w = self.ws.words().numpy().reshape(-1)
        nblk = (cells + 1023) // 1024
        a_bs = 2 * r16(cells * 4) // 4
        a_o2 = a_bs + r16((nblk + 1) * 4) // 4 + 4 * r16(max(n, 1) * 4) // 4
        bs = w[a_bs:a_bs + nblk + 1].astype(np.int64)
        start = np.concatenate([w[:cells].astype(np.int64) + bs[np.arange(cells) // 1024], bs[nblk:nblk + 1]])
        return start, w[a_o2:a_o2 + int(start[-1])].astype(np.int64)

    def got(self, split=False):
        start, order = self.lists()
        img = (self.img.words().numpy() if split else self.img.get().numpy()).reshape(-1, 32)
        return dict(xyz_t=self.xyz.get().numpy().reshape(-1, 3), pid=self.pid.words().numpy().reshape(-1),
                    offsets=self.off.get().numpy().reshape(-1, 3), start=start, order=order, image=img)


class Call:
    """inputs bit-unchanged, nothing outside an output view or a workspace written"""

    def __init__(self, inputs, outputs, wss=()):
        self.inputs, self.outputs, self.wss = inputs, outputs, list(wss)
        self.before = [g.buf.clone() for g in inputs]

    def check(self, case):
        torch.cuda.synchronize()
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.buf, b), f"{case}: an input was written"
        for g in self.outputs + self.wss:
            assert g.untouched_outside(), f"{case}: a write outside an output view or past a workspace"

    def refused(self, fn, case, st, want):
        torch.cuda.synchronize()
        assert st == want, f"{fn} {case}: status {st}, documented {want}"
        for g in self.outputs + self.wss:
            assert g.untouched(), f"{fn} {case}: refused (status {st}) but wrote"
        REFUSED.append((fn, case, st))


def weights(gpu, p, keys=("w", "scale", "shift")):
    return [grows(gpu, np.asarray(p[k], F32).reshape(-1, 32)) for k in keys]


def pillarize(lib, sw, wg, case):
    c = Call([sw.d_pts] + wg, sw.outputs(), [sw.ws])
    st = call(lib, "himo_pillarize", sw.n, sw.d_pts.ptr, sw.stride, fp(sw.T), fp(sw.rng), fp(sw.vox), fp(sw.cen), sw.grid.W, sw.grid.H,
              wg[0].ptr, wg[1].ptr, wg[2].ptr, sw.xyz.ptr, sw.pid.ptr, sw.off.ptr, sw.img.ptr, sw.pitch, sw.ws.ptr, sw.ws_bytes, _s())
    assert st == 0, f"{case}: status {st}"
    c.check(case)


def multi(lib, sweeps, wg, flags, case, fn="himo_pillarize_multi_ex", ws_bytes=None):
    from himo_amd.seflow.model import HimoSweep
    arr = (HimoSweep * len(sweeps))(*[s.struct() for s in sweeps])
    s0 = sweeps[0]
    c = Call([s.d_pts for s in sweeps] + wg, [g for s in sweeps for g in s.outputs()], [s.ws for s in sweeps])
    args = [len(sweeps), ctypes.addressof(arr), s0.rng.ctypes.data, s0.vox.ctypes.data, s0.cen.ctypes.data, s0.grid.W, s0.grid.H,
            wg[0].ptr, wg[1].ptr, wg[2].ptr, s0.pitch, ws_bytes or s0.ws_bytes]
    st = call(lib, fn, *(args + ([] if fn == "himo_pillarize_multi" else [flags]) + [_s()]))
    assert st == 0, f"{case}: status {st}"
    c.check(case)


LAYOUTS = [(3, 32, 0), (4, 36, 0), (5, 96, 32)]          # (pc_stride, image pitch, channel offset)


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(po.SCENES))
def test_forward(lib, gpu, name):
    grid, T, pts, _ = scene(name)
    p = po.params(list(po.SCENES).index(name))
    stride, pitch, choff = LAYOUTS[list(po.SCENES).index(name) % 3]
    case = f"pillarize {name} n={pts.shape[0]} stride={stride} pitch={pitch}+{choff}"
    sw = Sweep(lib, gpu, grid, pts, T, stride, pitch, choff)
    wg = weights(gpu, p)
    pillarize(lib, sw, wg, case)
    note("image", *po.check_forward(sw.got(), pts, T, grid, p, case))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_forward_point_counts(lib, gpu, n):
    grid, T, pts, _ = scene("41x25")
    p = po.params(n)
    sw = Sweep(lib, gpu, grid, pts[:n], T, 3 + n % 3, 32)
    pillarize(lib, sw, weights(gpu, p), f"pillarize 41x25 n={n}")
    note("image", *po.check_forward(sw.got(), pts[:n], T, grid, p, f"n={n}"))


def test_forward_512(lib, gpu):
    grid = po.Grid(512, 512, (-51.2, -51.2, -3.0), (0.2, 0.2, 6.0))
    T = po.rigid("general")
    pts = po.scene(grid, [(0, 33), (grid.cells - 1, 65), (1023, 32), (1024, 2), (255, 31), (256, 97)], 0.01, 5, T, 11)
    p = po.params(99)
    sw = Sweep(lib, gpu, grid, pts, T, 4, 32)
    pillarize(lib, sw, weights(gpu, p), "pillarize 512x512")
    note("image", *po.check_forward(sw.got(), pts, T, grid, p, "512x512"))


# ---- multi-sweep launches and the split format -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sweeps,split,pitch", [(1, 0, 32), (3, 1, 48), (12, 0, 36), (12, 1, 96), (3, 0, 32)])
def test_multi_equals_single(lib, gpu, n_sweeps, split, pitch):
    grid, T, pts, ptsB = scene("65x1")
    p = po.params(3)
    wg = weights(gpu, p)
    ns = [pts.shape[0] - 7 * i for i in range(n_sweeps)]
    if n_sweeps > 1:
        ns[n_sweeps // 2] = 0                                # an empty sweep in the middle
    clouds = [(pts if i % 2 == 0 else ptsB)[:k] for i, k in enumerate(ns)]
    sweeps = [Sweep(lib, gpu, grid, c, T, 3 + i % 3, pitch, ws_points=max(ns)) for i, c in enumerate(clouds)]
    fn = "himo_pillarize_multi" if (not split and pitch == 32 and n_sweeps == 3) else "himo_pillarize_multi_ex"
    case = f"{fn} sweeps={n_sweeps} split={split} pitch={pitch}"
    multi(lib, sweeps, wg, split, case, fn)
    for i, (sw, c) in enumerate(zip(sweeps, clouds)):
        one = Sweep(lib, gpu, grid, c, T, 3, 32)
        pillarize(lib, one, wg, case + f" single {i}")
        a, b = sw.got(bool(split)), one.got()
        for k in ("xyz_t", "pid", "offsets", "start", "order"):
            po.exact(k, a[k], b[k], f"{case} sweep {i}")
        po.exact("image", a["image"], po.split_words(b["image"]) if split else b["image"], f"{case} sweep {i}")
    note("multi == single (bits)", 0.0)


# ---- incremental images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,split", [("65x1", 0), ("41x25", 1), ("41x25", 0)])
def test_incremental(lib, gpu, name, split):
    grid, T, ptsA, _ = scene(name)
    p = po.params(5)
    wg = weights(gpu, p)
    pid, _ = po.cells_of(po.transform(ptsA, T), grid)
    half = grid.cells // 2                                   # A: the lower cells, B: the upper ones (disjoint)
    A, B = ptsA[(pid >= 0) & (pid < half) | (pid < 0)], ptsA[pid >= half]
    pitch = 48 if split else 32
    nmax = max(A.shape[0], B.shape[0])
    keep = Sweep(lib, gpu, grid, A, T, 3, pitch, ws_points=nmax)
    st = call(lib, "himo_pillar_occupancy_reset", keep.ws.ptr, keep.ws_bytes, grid.W, grid.H, _s())
    assert st == 0
    for k, cloud in enumerate([A, B, A[:0], A, A]):
        case = f"incremental {name} split={split} pass {k}"
        cur = Sweep(lib, gpu, grid, cloud, T, 3, pitch, ws_points=nmax, keep=keep)
        multi(lib, [cur], wg, split | 2, case)
        fresh = Sweep(lib, gpu, grid, cloud, T, 3, pitch, ws_points=nmax)
        multi(lib, [fresh], wg, split, case + " fresh")
        po.exact("image", cur.img.words().numpy().reshape(-1, 32), fresh.img.words().numpy().reshape(-1, 32), case)
        pc, _ = po.cells_of(po.transform(cloud, T), grid)
        empty = np.bincount(pc[pc >= 0], minlength=grid.cells) == 0
        assert not cur.img.words().numpy().reshape(-1, 32)[empty].any(), f"{case}: a cell that emptied is not zero"
    note("incremental == fresh (bits)", 0.0)


# ---- scatter ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dhx_pitch,n_groups,g0,g1,pad", [("7x5", 128, 2, 0, 1, 0), ("41x25", 192, 3, 1, 2, 4), ("1x64", 192, 3, 2, 0, 8),
                                                            ("128x96", 128, 2, 1, 0, 0)])
def test_head_scatter(lib, gpu, name, dhx_pitch, n_groups, g0, g1, pad):
    grid, T, pts, _ = scene(name)
    case = f"head_scatter {name} dhx_pitch={dhx_pitch} groups={n_groups} ({g0},{g1}) pad={pad}"
    sw = Sweep(lib, gpu, grid, pts, T)
    pillarize(lib, sw, weights(gpu, po.params(0)), case)
    dhx = np.random.default_rng(11).standard_normal((pts.shape[0], 128)).astype(F32)
    d_dhx = grows(gpu, dhx, dhx_pitch)
    b0, dec = grows(gpu, (grid.cells, 32 * n_groups), 32 * n_groups + pad), grows(gpu, (grid.cells, 64), 64 + pad)
    c = Call([d_dhx, sw.ws], [b0, dec])
    st = call(lib, "himo_head_scatter", sw.n, grid.W, grid.H, sw.ws.ptr, d_dhx.ptr, dhx_pitch, b0.ptr, 32 * n_groups + pad, g0, g1, n_groups,
              dec.ptr, 64 + pad, _s())
    assert st == 0, case
    c.check(case)
    w0, w1 = po.scatter_ref(*po.cell_lists(sw.got()["pid"], grid.cells), dhx, g0, g1, n_groups)
    po.exact("d_b0", b0.get().numpy().reshape(w0.shape), w0, case)
    po.exact("d_dec", dec.get().numpy().reshape(w1.shape), w1, case)
    note("head_scatter (bits)", 0.0)


# ---- frozen backward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,acc,pitch", [("7x5", 0, 32), ("32x32", 1, 36), ("41x25", 0, 96), ("128x96", 1, 32), ("1x1", 0, 32)])
def test_pfn_backward(lib, gpu, name, acc, pitch):
    grid, T, pts, _ = scene(name)
    p = po.params(list(po.SCENES).index(name))
    case = f"pfn_backward {name} acc={acc} pitch={pitch}"
    sw = Sweep(lib, gpu, grid, pts, T)
    wg = weights(gpu, p)
    pillarize(lib, sw, wg, case)
    rng = np.random.default_rng(21)
    dimg, old = rng.standard_normal((grid.cells, 32)).astype(F32), rng.standard_normal((9, 32)).astype(F32)
    d_dimg, dw = grows(gpu, dimg, pitch), grows(gpu, old if acc else (9, 32))
    need = int(call(lib, "himo_pfn_backward_workspace_bytes"))
    ws = gbytes(gpu, need)
    c = Call([d_dimg, sw.ws, sw.xyz] + wg, [dw], [ws])
    st = call(lib, "himo_pfn_backward", sw.n, fp(sw.vox), fp(sw.cen), grid.W, grid.H, wg[0].ptr, wg[1].ptr, wg[2].ptr, sw.xyz.ptr, sw.ws.ptr,
              d_dimg.ptr, pitch, dw.ptr, acc, ws.ptr, need, _s())
    assert st == 0, case
    c.check(case)
    g = sw.got()
    ref = po.backward_ref([(g["xyz_t"], g["pid"], dimg)], grid, p["w"], p["scale"], p["shift"], old=(old, None, None) if acc else None)
    assert ref["undecided"] <= po.UNDECIDED_CAP * max(ref["pairs"], 1), case
    note("dW frozen", *po.verify("dW", dw.get().numpy(), *ref["dW"], case=case))


# ---- BatchNorm training path -----------------------------------------------------------------------------------------------------
def _ptrs(vals, typ=ctypes.c_void_p):
    return (typ * len(vals))(*vals)


def _bn_sweeps(lib, gpu, grid, T, pts, ptsB, fracs, wg, case):
    """the sweeps of a training-path case with their cell lists built: a fraction of the scene each (None: all of it, "one": a
    single in-range row)"""
    first = int(np.nonzero(po.cells_of(po.transform(pts, T), grid)[0] >= 0)[0][0])
    clouds = [pts[first:first + 1] if f == "one" else (pts if i % 2 == 0 else ptsB)[:(pts.shape[0] if f is None else int(f * pts.shape[0]))]
              for i, f in enumerate(fracs)]
    nmax = max(c.shape[0] for c in clouds)
    sweeps = [Sweep(lib, gpu, grid, c, T, 3, 32, ws_points=nmax) for c in clouds]
    for lo in range(0, len(sweeps), 12):
        multi(lib, sweeps[lo:lo + 12], wg, 0, case + " lists")
    return sweeps, [s.got() for s in sweeps]


BN_CASES = [  # (scene, n_sweeps, n_groups, point counts as fractions of the scene (None: all), running?, accumulate, entry-point form)
    ("7x5", 1, 1, [None], True, 0, "single"),
    ("65x1", 3, 3, [None, 0.5, 0.25], True, 1, "multi"),
    ("7x5", 2, 1, [None, 0.5], False, 0, "groups"),
    ("41x25", 6, 3, [None, 0.5, 0.0, 0.0, 0.3, 0.0], True, 0, "groups"),        # group 0 has an empty member, group 2 is all empty
    ("7x5", 16, 1, [None, 0.5] * 8, True, 1, "groups"),                          # 16 members, two walk launches
    ("65x1", 32, 2, [0.2, 0.1] * 16, False, 0, "groups"),
    ("7x5", 4, 2, [None, "one", 0.5, 0.0], True, 0, "groups"),                   # group 1: ONE in-range point and an empty member
]


@pytest.mark.parametrize("cfg", BN_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[6]}")
def test_bn_training_path(lib, gpu, cfg):
    name, S, G, fracs, running, acc, form = cfg
    grid, T, pts, ptsB = scene(name)
    p = po.params(40 + S)
    case = f"bn {name} sweeps={S} groups={G} {form} running={running} acc={acc}"
    wg = weights(gpu, p)
    sweeps, got = _bn_sweeps(lib, gpu, grid, T, pts, ptsB, fracs, wg, case)
    rng = np.random.default_rng(77)
    rm0, rv0 = rng.uniform(-0.1, 0.1, 32).astype(F32), rng.uniform(0.5, 1.5, 32).astype(F32)
    gam, bet = weights(gpu, p, ("gamma", "beta"))
    rm, rv = grows(gpu, rm0.reshape(1, 32)), grows(gpu, rv0.reshape(1, 32))
    outs = [grows(gpu, (G, 32)) for _ in range(4)]                    # scale, shift, mean, invstd
    one = int(call(lib, "himo_pfn_bn_workspace_bytes"))
    ws = gbytes(gpu, one * S)
    h_n = _ptrs([s.n for s in sweeps], ctypes.c_int64)
    h_x, h_w = _ptrs([s.xyz.ptr for s in sweeps]), _ptrs([s.ws.ptr for s in sweeps])
    s0 = sweeps[0]
    c = Call([s.ws for s in sweeps] + [s.xyz for s in sweeps] + [wg[0], gam, bet], outs + ([rm, rv] if running else []), [ws])
    tail = [gam.ptr, bet.ptr, EPS, MOM, rm.ptr if running else None, rv.ptr if running else None] + [o.ptr for o in outs] + [ws.ptr, one * S, _s()]
    if form == "single":
        st = call(lib, "himo_pfn_bn_stats", s0.n, fp(s0.vox), fp(s0.cen), grid.W, grid.H, wg[0].ptr, s0.xyz.ptr, s0.ws.ptr, *tail)
    elif form == "multi":
        st = call(lib, "himo_pfn_bn_stats_multi", S, h_n, h_x, h_w, s0.vox.ctypes.data, s0.cen.ctypes.data, grid.W, grid.H, wg[0].ptr, *tail)
    else:
        st = call(lib, "himo_pfn_bn_stats_groups", S, G, h_n, h_x, h_w, s0.vox.ctypes.data, s0.cen.ctypes.data, grid.W, grid.H, wg[0].ptr, *tail)
    assert st == 0, f"{case}: stats status {st}"
    c.check(case + " stats")
    sc, sh, mu, iv = (o.get().numpy().reshape(G, 32) for o in outs)
    r_m, r_v, e_m, e_v = rm0.astype(np.float64), rv0.astype(np.float64), np.zeros(32), np.zeros(32)
    for g_ in range(G):
        mem = [(got[i]["xyz_t"], got[i]["pid"]) for i in range(S) if i % G == g_]
        want = po.bn_stats_ref(mem, grid, p["w"], p["gamma"], p["beta"], EPS, MOM, r_m if running else None, r_v if running else None)
        for key, val in (("scale", sc), ("shift", sh), ("mean", mu), ("invstd", iv)):
            note(f"stats {key}", *po.verify(key, val[g_], *want[key], case=f"{case} group {g_}"))
        if running and sum(int((q >= 0).sum()) for _, q in mem):       # the groups update the running statistics one after another;
            e_m, e_v = want["running_mean"][1] + (1 - MOM) * e_m, want["running_var"][1] + (1 - MOM) * e_v      # an empty one leaves them
            r_m, r_v = want["running_mean"][0], want["running_var"][0]
    if running:
        note("stats running_mean", *po.verify("running_mean", rm.get().numpy().reshape(32), r_m, e_m + 1e-300, case=case))
        note("stats running_var", *po.verify("running_var", rv.get().numpy().reshape(32), r_v, e_v + 1e-300, case=case))
    # the feature kernel alone, per-SWEEP constants
    d_sc, d_sh = grows(gpu, sc[np.arange(S) % G]), grows(gpu, sh[np.arange(S) % G])
    for lo in range(0, S, 12):
        part = sweeps[lo:lo + 12]
        from himo_amd.seflow.model import HimoSweep
        arr = (HimoSweep * len(part))(*[s.struct() for s in part])
        for s in part:
            s.img.reset()
        cf = Call([s.d_pts for s in part] + [s.xyz for s in part] + [wg[0], d_sc, d_sh], [s.img for s in part], [s.ws for s in part])
        st = call(lib, "himo_pillar_features_multi", len(part), ctypes.addressof(arr), s0.rng.ctypes.data, s0.vox.ctypes.data, s0.cen.ctypes.data,
                  grid.W, grid.H, wg[0].ptr, d_sc.ptr + 128 * lo, d_sh.ptr + 128 * lo, 32, s0.ws_bytes, 0, _s())
        assert st == 0, f"{case}: features status {st}"
        cf.check(case + " features")
    for i, s in enumerate(sweeps):
        ref, bnd, ref32, ne = po.image_ref(got[i]["xyz_t"], got[i]["pid"], grid, p["w"], sc[i % G], sh[i % G])
        img = s.img.get().numpy().reshape(-1, 32)
        assert not img[~ne].view(np.int32).any(), f"{case}: sweep {i}: an empty cell is not zero"
        if ne.any():
            note("image (batch statistics)", *po.verify("image", img[ne], ref[ne], bnd[ne], ref32[ne], case=f"{case} sweep {i}"))
    # backward through the batch statistics
    dimg = rng.standard_normal((S, grid.cells, 32)).astype(F32)
    d_dimg = [grows(gpu, d) for d in dimg]
    old = [rng.standard_normal((9, 32)).astype(F32), rng.standard_normal((1, 32)).astype(F32), rng.standard_normal((1, 32)).astype(F32)]
    dw, dg, db = (grows(gpu, o if acc else o.shape) for o in old)
    h_d = _ptrs([d.ptr for d in d_dimg])
    cb = Call([s.ws for s in sweeps] + [s.xyz for s in sweeps] + d_dimg + outs + [wg[0]], [dw, dg, db], [ws])
    tail = [wg[0].ptr] + [o.ptr for o in outs]
    if form == "single":
        st = call(lib, "himo_pfn_backward_bn", s0.n, fp(s0.vox), fp(s0.cen), grid.W, grid.H, *tail, s0.xyz.ptr, s0.ws.ptr, d_dimg[0].ptr, 32,
                  dw.ptr, dg.ptr, db.ptr, acc, ws.ptr, one * S, _s())
    elif form == "multi":
        st = call(lib, "himo_pfn_backward_bn_multi", S, h_n, h_x, h_w, h_d, 32, s0.vox.ctypes.data, s0.cen.ctypes.data, grid.W, grid.H, *tail,
                  dw.ptr, dg.ptr, db.ptr, acc, ws.ptr, one * S, _s())
    else:
        st = call(lib, "himo_pfn_backward_bn_groups", S, G, h_n, h_x, h_w, h_d, 32, s0.vox.ctypes.data, s0.cen.ctypes.data, grid.W, grid.H, *tail,
                  dw.ptr, dg.ptr, db.ptr, acc, ws.ptr, one * S, _s())
    assert st == 0, f"{case}: backward status {st}"
    cb.check(case + " backward")
    ref = po.backward_ref([(got[i]["xyz_t"], got[i]["pid"], dimg[i]) for i in range(S)], grid, p["w"], sc, sh, mu, iv, G,
                          old=[o.reshape(-1, 32) if k == 0 else o.reshape(32) for k, o in enumerate(old)] if acc else None)
    assert ref["undecided"] <= po.UNDECIDED_CAP * max(ref["pairs"], 1), case
    note("bn dW", *po.verify("dW", dw.get().numpy(), *ref["dW"], case=case, limit=po.R_BN_DW))
    note("bn dgamma", *po.verify("dgamma", dg.get().numpy().reshape(32), *ref["dgamma"], case=case))
    note("bn dbeta", *po.verify("dbeta", db.get().numpy().reshape(32), *ref["dbeta"], case=case))


def test_own_groups_have_the_bits_of_single_calls(lib, gpu):
    """every sweep its own group (the _multi forms, and _groups with n_groups == n_sweeps) == n_sweeps single calls in order, the
    accumulate flag set from the second on: statistics, running statistics, dW, dgamma, dbeta bit for bit"""
    grid, T, pts, ptsB = scene("65x1")
    p = po.params(61)
    case = "own groups == single calls"
    wg = weights(gpu, p)
    S = 3
    sweeps, _ = _bn_sweeps(lib, gpu, grid, T, pts, ptsB, [None, 0.5, 0.25], wg, case)
    rng = np.random.default_rng(78)
    rm0, rv0 = rng.uniform(-0.1, 0.1, (1, 32)).astype(F32), rng.uniform(0.5, 1.5, (1, 32)).astype(F32)
    gam, bet = weights(gpu, p, ("gamma", "beta"))
    d_dimg = [grows(gpu, rng.standard_normal((grid.cells, 32)).astype(F32)) for _ in range(S)]
    one = int(call(lib, "himo_pfn_bn_workspace_bytes"))
    h_n = _ptrs([s.n for s in sweeps], ctypes.c_int64)
    h_x, h_w, h_d = _ptrs([s.xyz.ptr for s in sweeps]), _ptrs([s.ws.ptr for s in sweeps]), _ptrs([d.ptr for d in d_dimg])
    s0 = sweeps[0]
    vox, cen = s0.vox.ctypes.data, s0.cen.ctypes.data
    res = {}
    for form in ("single", "multi", "groups"):
        rm, rv = grows(gpu, rm0), grows(gpu, rv0)
        outs = [grows(gpu, (S, 32)) for _ in range(4)]
        dw, dg, db = grows(gpu, (9, 32)), grows(gpu, (1, 32)), grows(gpu, (1, 32))
        ws = gbytes(gpu, one * S)
        tail = [gam.ptr, bet.ptr, EPS, MOM, rm.ptr, rv.ptr] + [o.ptr for o in outs] + [ws.ptr, one * S, _s()]
        btail = [wg[0].ptr] + [o.ptr for o in outs] + [dw.ptr, dg.ptr, db.ptr, 0, ws.ptr, one * S, _s()]
        if form == "multi":
            st = call(lib, "himo_pfn_bn_stats_multi", S, h_n, h_x, h_w, vox, cen, grid.W, grid.H, wg[0].ptr, *tail)
            st |= call(lib, "himo_pfn_backward_bn_multi", S, h_n, h_x, h_w, h_d, 32, vox, cen, grid.W, grid.H, *btail)
        elif form == "groups":
            st = call(lib, "himo_pfn_bn_stats_groups", S, S, h_n, h_x, h_w, vox, cen, grid.W, grid.H, wg[0].ptr, *tail)
            st |= call(lib, "himo_pfn_backward_bn_groups", S, S, h_n, h_x, h_w, h_d, 32, vox, cen, grid.W, grid.H, *btail)
        else:
            st = 0
            for i, s in enumerate(sweeps):
                st |= call(lib, "himo_pfn_bn_stats", s.n, fp(s.vox), fp(s.cen), grid.W, grid.H, wg[0].ptr, s.xyz.ptr, s.ws.ptr, gam.ptr, bet.ptr,
                           EPS, MOM, rm.ptr, rv.ptr, *[o.ptr + 128 * i for o in outs], ws.ptr, one, _s())
            for i, s in enumerate(sweeps):
                st |= call(lib, "himo_pfn_backward_bn", s.n, fp(s.vox), fp(s.cen), grid.W, grid.H, wg[0].ptr, *[o.ptr + 128 * i for o in outs],
                           s.xyz.ptr, s.ws.ptr, d_dimg[i].ptr, 32, dw.ptr, dg.ptr, db.ptr, 1 if i else 0, ws.ptr, one, _s())
        assert st == 0, f"{case}: {form}: status {st}"
        torch.cuda.synchronize()
        for g in outs + [rm, rv, dw, dg, db, ws]:
            assert g.untouched_outside(), f"{case}: {form}: a write outside an output view or past the workspace"
        res[form] = {k: g.get().numpy() for k, g in zip(("scale", "shift", "mean", "invstd", "running_mean", "running_var", "dW", "dgamma",
                                                          "dbeta"), outs + [rm, rv, dw, dg, db])}
    for form in ("multi", "groups"):
        for k, want in res["single"].items():
            po.exact(k, res[form][k], want, f"{case}: {form}")
    note("own groups == single calls (bits)", 0.0)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(lib, gpu):
    grid, T, pts, _ = scene("7x5")
    p = po.params(0)
    wg = weights(gpu, p)
    nq = pts.shape[0]

    def single(case, want, n=None, stride=3, pitch=32, img_off=0, ws_short=0, ws_off=0, W=None, H=None, cloud=None):
        sw = Sweep(lib, gpu, grid, pts if cloud is None else cloud, T, max(stride, 3), max(pitch, 32), img_off)
        c = Call([], sw.outputs(), [sw.ws])
        st = lib.himo_pillarize(sw.n if n is None else n, sw.d_pts.ptr, stride, fp(sw.T), fp(sw.rng), fp(sw.vox), fp(sw.cen),
                                W or grid.W, H or grid.H, wg[0].ptr, wg[1].ptr, wg[2].ptr, sw.xyz.ptr, sw.pid.ptr, sw.off.ptr, sw.img.ptr, pitch,
                                sw.ws.ptr + ws_off, sw.ws_bytes - ws_short, _s())
        c.refused("himo_pillarize", case, st, want)

    single("n = -1", INVALID, n=-1)
    single("pc_stride 2", INVALID, stride=2)
    single("pitch 31", UNSUPPORTED, pitch=31)
    single("pitch 34", UNSUPPORTED, pitch=34)
    single("image 4 bytes off alignment", UNSUPPORTED, img_off=1)
    single("workspace one byte short of what n points need", WORKSPACE, ws_short=64 + 16 + 1)   # the query adds 64 bytes and the occupancy words
    single("workspace 4 bytes off alignment", WORKSPACE, ws_off=4)
    single("1025 x 1024 grid", UNSUPPORTED, W=1025, H=1024, cloud=pts[:0])
    single("65536 x 65536 grid (2^32 cells), n = 0", UNSUPPORTED, W=65536, H=65536, cloud=pts[:0])
    assert int(call(lib, "himo_pillar_workspace_bytes", 0, 65536, 65536)) == 0 and int(call(lib, "himo_pillar_workspace_bytes", 0, 1025, 1024)) == 0

    from himo_amd.seflow.model import HimoSweep

    def many(case, want, n_sweeps=2, flags=0, pitch=32, img_off=0, share=False, ws_short=0, fn="himo_pillarize_multi_ex"):
        sweeps = [Sweep(lib, gpu, grid, pts, T, 3, max(pitch, 32), img_off) for _ in range(max(n_sweeps, 1))]
        if share:
            sweeps[1].ws = sweeps[0].ws
        arr = (HimoSweep * len(sweeps))(*[s.struct() for s in sweeps])
        c = Call([], [g for s in sweeps for g in s.outputs()], [s.ws for s in sweeps])
        s0 = sweeps[0]
        st = getattr(lib, fn)(n_sweeps, ctypes.addressof(arr), s0.rng.ctypes.data, s0.vox.ctypes.data, s0.cen.ctypes.data, grid.W, grid.H,
                              wg[0].ptr, wg[1].ptr, wg[2].ptr, pitch, s0.ws_bytes - ws_short, flags, _s())
        c.refused(fn, case, st, want)

    many("0 sweeps", INVALID, n_sweeps=0)
    many("13 sweeps", INVALID, n_sweeps=13)
    many("split, pitch 40", INVALID, flags=1, pitch=40)
    many("split, image only 16-byte aligned", INVALID, flags=1, pitch=48, img_off=4)
    many("two sweeps share a workspace", INVALID, share=True)
    many("incremental, no room for the occupancy words", WORKSPACE, flags=2, ws_short=64 + 16)     # a multiple of 16: not the & 15 test
    many("incremental, workspace_bytes not a multiple of 16", WORKSPACE, flags=2, ws_short=8)
    many("features: 13 sweeps", INVALID, n_sweeps=13, fn="himo_pillar_features_multi")

    # backward forms: lists of a real forward pass, then refused calls
    sw = Sweep(lib, gpu, grid, pts, T)
    pillarize(lib, sw, wg, "refusals forward")
    dimg, dw = grows(gpu, np.zeros((grid.cells, 32), F32)), grows(gpu, (9, 32))
    need = int(call(lib, "himo_pfn_backward_workspace_bytes"))
    ws = gbytes(gpu, need)

    def bwd(case, want, n=nq, W=grid.W, H=grid.H, short=0):
        c = Call([], [dw], [ws])
        st = lib.himo_pfn_backward(n, fp(sw.vox), fp(sw.cen), W, H, wg[0].ptr, wg[1].ptr, wg[2].ptr, sw.xyz.ptr, sw.ws.ptr, dimg.ptr, 32, dw.ptr, 0,
                                   ws.ptr, need - short, _s())
        c.refused("himo_pfn_backward", case, st, want)

    bwd("workspace one byte short", WORKSPACE, short=1)
    bwd("n = -1", INVALID, n=-1)
    bwd("65536 x 65536 grid, n = 0", UNSUPPORTED, n=0, W=65536, H=65536)

    one = int(call(lib, "himo_pfn_bn_workspace_bytes"))
    gam, bet = weights(gpu, p, ("gamma", "beta"))
    outs = [grows(gpu, (3, 32)) for _ in range(4)]
    rm, rv = grows(gpu, (1, 32)), grows(gpu, (1, 32))
    dg, db = grows(gpu, (1, 32)), grows(gpu, (1, 32))
    wsb = gbytes(gpu, one * 34)

    def stats(case, want, S=3, G=3, short=0, ws_off=0, rmp=True, rvp=True, W=grid.W, H=grid.H, n=nq):
        c = Call([], outs + [rm, rv], [wsb])
        st = lib.himo_pfn_bn_stats_groups(S, G, _ptrs([n] * S, ctypes.c_int64), _ptrs([sw.xyz.ptr] * S), _ptrs([sw.ws.ptr] * S), sw.vox.ctypes.data,
                                          sw.cen.ctypes.data, W, H, wg[0].ptr, gam.ptr, bet.ptr, EPS, MOM, rm.ptr if rmp else None,
                                          rv.ptr if rvp else None, *[o.ptr for o in outs], wsb.ptr + ws_off, one * S - short, _s())
        c.refused("himo_pfn_bn_stats_groups", case, st, want)

    stats("n_sweeps % n_groups != 0", INVALID, S=4, G=3)
    stats("17 members per group", INVALID, S=34, G=2)
    stats("one running pointer NULL", INVALID, rvp=False)
    stats("workspace one byte short", WORKSPACE, short=1)
    stats("workspace 4 bytes off alignment", WORKSPACE, ws_off=4)
    stats("65536 x 65536 grid, n = 0", UNSUPPORTED, W=65536, H=65536, n=0)

    def bwd_bn(case, want, S=3, G=3, short=0, W=grid.W, H=grid.H, n=nq):
        c = Call([], [dw, dg, db], [wsb])
        st = lib.himo_pfn_backward_bn_groups(S, G, _ptrs([n] * S, ctypes.c_int64), _ptrs([sw.xyz.ptr] * S), _ptrs([sw.ws.ptr] * S),
                                             _ptrs([dimg.ptr] * S), 32, sw.vox.ctypes.data, sw.cen.ctypes.data, W, H, wg[0].ptr,
                                             *[o.ptr for o in outs], dw.ptr, dg.ptr, db.ptr, 0, wsb.ptr, one * S - short, _s())
        c.refused("himo_pfn_backward_bn_groups", case, st, want)

    bwd_bn("n_sweeps % n_groups != 0", INVALID, S=4, G=3)
    bwd_bn("workspace one byte short", WORKSPACE, short=1)
    bwd_bn("65536 x 65536 grid, n = 0", UNSUPPORTED, W=65536, H=65536, n=0)

    dhx = grows(gpu, np.zeros((nq, 128), F32))
    b0, dec = grows(gpu, (grid.cells, 96)), grows(gpu, (grid.cells, 64))

    def scat(case, want, g0=1, g1=2, G=3, W=grid.W, H=grid.H, n=nq):
        c = Call([], [b0, dec])
        st = lib.himo_head_scatter(n, W, H, sw.ws.ptr, dhx.ptr, 128, b0.ptr, 96, g0, g1, G, dec.ptr, 64, _s())
        c.refused("himo_head_scatter", case, st, want)

    scat("group0 = -1", INVALID, g0=-1)
    scat("group1 = n_groups", INVALID, g1=3)
    scat("group0 == group1", INVALID, g0=2, g1=2)
    scat("n_groups 1 (no two distinct groups)", INVALID, g0=0, g1=0, G=1)
    scat("65536 x 65536 grid, n = 0", UNSUPPORTED, W=65536, H=65536, n=0)
