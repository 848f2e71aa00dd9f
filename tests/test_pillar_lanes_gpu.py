"""The lane-per-cell path of pillar_feature_kernel (csrc/pillar.hip) and the two flag bits that came with it, through
himo_pillarize_multi_ex called directly.

A cell of 1 .. K points (K = kLaneK of pillar.hip) is worked by ONE lane, a cell of more by half a wavefront; the feature kernel's
blocks own 1024 cells, its waves one 64-cell occupancy word at a time.  The scenes put every population around K and around the
half-wave path's own thresholds (31, 32, 33, 97) into neighbouring cells and at cells 0, 63, 64 and the last, on grids with a
partial last block (41x25: 1025 cells, every 64 / 256 / 1024 boundary) and a second occupancy word holding one cell (65x1).

Checked: po.check_forward (transformed points, cells, offsets, cell offsets and ascending lists bit for bit against the float32
emulation of oracle/pillar_oracle.py, the image within its derived bound); the split image against the split of the checked
float32 image, word for word; HIMO_PILLAR_HALFWAVE_ONLY against the default path, every output word for word;
HIMO_PILLAR_NO_LISTS against the call without it.  Every operand, output and workspace lives in a NaN-filled guarded buffer
(oracle/guarded.py): inputs stay bit-unchanged and nothing outside an output view or a workspace is written.

The split format admits image pitches that are multiples of 16 floats only, so where the conformance file's second layout
(pitch 36) meets HIMO_IMAGE_SPLIT the pitch is 48, the one that file uses for its own split cases.
"""
import ctypes

import numpy as np
import pytest
import torch

import pillar_oracle as po
from guarded import Guarded, layout

pytestmark = pytest.mark.gpu

F32 = np.float32
K = 4                                                      # kLaneK of csrc/pillar.hip
SPLIT, INCREMENTAL, NO_LISTS, HALFWAVE_ONLY = 1, 2, 4, 8   # include/himo_amd.h
INVALID = 1
POPS = (1, 2, K - 1, K, K + 1, 31, 32, 33, 97)
LAYOUTS = [(3, 32, 0), (4, 36, 0), (5, 96, 32)]            # (pc_stride, image pitch, channel offset): tests/test_pillar_conformance_gpu.py
_CACHE = {}


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import model                      # noqa: F401  (registers the signatures)
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def grows(gpu, values, pitch=None, off=0):
    """[rows, cols] at ``pitch`` floats per row, ``off`` floats into the buffer; NaN-filled when values is a shape"""
    shape = values if isinstance(values, tuple) else values.shape
    g = Guarded(layout(1, 1, 0, 0, shape[0], pitch or shape[1], shape[1]), gpu, off=off)
    if not isinstance(values, tuple) and shape[0]:
        g.put(torch.from_numpy(np.ascontiguousarray(values)).to(torch.float32))
    return g


def _grid(name):
    return {"41x25": po._g(41, 25, "dyadic"), "65x1": po._g(65, 1, "dyadic"), "128x1": po._g(128, 1, "square"),
            "256x1": po._g(256, 1, "fifth"), "64x5": po._g(64, 5, "square")}[name]


def _placed(name):
    cells = _grid(name).cells
    if name == "41x25":        # the populations side by side, and one each at cell 0, both sides of every 64 / 256 / 1024 boundary, the last
        marks = [0, 63, 64, 255, 256, 1023, 1024]
        return [(100 + i, p) for i, p in enumerate(POPS)] + [(m, POPS[(2 * i + 1) % len(POPS)]) for i, m in enumerate(marks)] + \
               [(500 + i, POPS[len(POPS) - 1 - i]) for i in range(len(POPS))]
    if name == "65x1":         # the second occupancy word holds one cell
        return [(10 + i, p) for i, p in enumerate(POPS)] + [(0, K), (63, K + 1), (64, K - 1 if K > 2 else 2), (62, 1)]
    if name == "128x1":        # word 0: every cell one point; word 1: exactly one non-empty cell
        return [(c, 1) for c in range(64)] + [(c, 0) for c in range(64, 128)] + [(101, 3)]
    if name == "256x1":        # one block: more few-point cells than a wave has lanes, more single-point cells too, some crowded ones
        few = [(c, 2 + c % max(K - 1, 1)) for c in range(0, 70)]
        return few + [(c, 1) for c in range(70, 200)] + [(200, K + 1), (201, 33), (202, 97), (203, 32)] + [(c, 0) for c in range(204, 256)]
    if name == "64x5":         # words of one block with nothing in them between words that hold data
        return [(c, 0) for c in range(64, 192)] + [(3, K), (200, 2), (319, K + 1)]
    raise KeyError(name)


FILLER = {"41x25": 0.4, "65x1": 0.4, "128x1": 0.0, "256x1": 0.0, "64x5": 0.4}


def scene(name):
    """-> grid, T, pts, pts of another seed"""
    if name not in _CACHE:
        grid, T = _grid(name), po.rigid("general")
        _CACHE[name] = (grid, T) + tuple(po.scene(grid, _placed(name), FILLER[name], seed, T, 3) for seed in (5, 6))
    return _CACHE[name]


class Sweep:
    """one sweep's guarded buffers: points at a row stride, per-point outputs, its 32 image channels, occupancy words, workspace"""

    def __init__(self, lib, gpu, grid, pts, T, stride=3, pitch=32, choff=0, ws_points=None, keep=None, offsets=True):
        self.grid, self.pts, self.T, self.n, self.stride, self.pitch = grid, pts, np.ascontiguousarray(T, F32), pts.shape[0], stride, pitch
        n = self.n
        self.d_pts = grows(gpu, pts, stride)
        self.xyz, self.pid, self.off = grows(gpu, (n, 3)), grows(gpu, (n, 1)), grows(gpu, (n, 3))
        self.pass_offsets = offsets
        self.img = keep.img if keep else grows(gpu, (grid.cells, 32), pitch, choff)
        self.occ = grows(gpu, (1, 2 * ((grid.cells + 63) // 64)))
        self.ws_bytes = int(lib.himo_pillar_workspace_bytes(n if ws_points is None else ws_points, grid.W, grid.H))
        assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
        self.ws = keep.ws if keep else Guarded(layout(1, 1, 0, 0, 1, self.ws_bytes // 4, self.ws_bytes // 4), gpu)
        self.rng, self.vox, self.cen = (np.ascontiguousarray(a, F32) for a in (grid.vmin, grid.voxel, grid.centre))

    def struct(self):
        from himo_amd.seflow.model import HimoSweep
        s = HimoSweep(n=self.n, d_pts=self.d_pts.ptr, pc_stride=self.stride, d_xyz_t=self.xyz.ptr, d_pid=self.pid.ptr,
                      d_offsets=self.off.ptr if self.pass_offsets else None, d_image=self.img.ptr, d_workspace=self.ws.ptr,
                      d_occupancy=self.occ.ptr)
        s.transform[:] = [float(v) for v in self.T.reshape(-1)]
        return s

    def outputs(self):
        return [self.xyz, self.pid, self.off, self.img, self.occ]

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

    def got(self, split=False, lists=True):
        """every output as its words (the image as float32 unless split); occupancy: one bit per cell"""
        start, order = self.lists() if lists else (None, None)
        img = (self.img.words().numpy() if split else self.img.get().numpy()).reshape(-1, 32)
        occ = self.occ.words().numpy().reshape(-1).view(np.uint32)
        bits = ((occ[:, None] >> np.arange(32, dtype=np.uint32)[None]) & 1).reshape(-1)[:self.grid.cells].astype(np.int32)
        return dict(xyz_t=self.xyz.get().numpy().reshape(-1, 3), pid=self.pid.words().numpy().reshape(-1),
                    offsets=self.off.get().numpy().reshape(-1, 3), start=start, order=order, image=img, occupancy=bits)


def weights(gpu, p):
    return [grows(gpu, np.asarray(p[k], F32).reshape(-1, 32)) for k in ("w", "scale", "shift")]


def run(lib, sweeps, wg, flags, case, want=0):
    """himo_pillarize_multi_ex over ``sweeps``; inputs bit-unchanged, nothing outside an output view or a workspace written"""
    from himo_amd.seflow.model import HimoSweep
    arr = (HimoSweep * len(sweeps))(*[s.struct() for s in sweeps])
    s0 = sweeps[0]
    inputs = [s.d_pts for s in sweeps] + wg
    before = [g.buf.clone() for g in inputs]
    st = lib.himo_pillarize_multi_ex(len(sweeps), ctypes.addressof(arr), s0.rng.ctypes.data, s0.vox.ctypes.data, s0.cen.ctypes.data, s0.grid.W,
                                     s0.grid.H, wg[0].ptr, wg[1].ptr, wg[2].ptr, s0.pitch, s0.ws_bytes, flags, _s())
    torch.cuda.synchronize()
    assert st == want, f"{case}: status {st}, expected {want}"
    for g, b in zip(inputs, before):
        assert torch.equal(g.buf, b), f"{case}: an input was written"
    for s in sweeps:
        for g in s.outputs() + [s.ws]:
            assert g.untouched_outside(), f"{case}: a write outside an output view or past a workspace"
            if want:
                assert g.untouched(), f"{case}: refused (status {st}) but wrote"


def same(a, b, case, keys=("xyz_t", "pid", "offsets", "start", "order", "image", "occupancy")):
    for k in keys:
        po.exact(k, a[k], b[k], case)


def occupancy_ref(pts, T, grid):
    pid, _ = po.cells_of(po.transform(pts, T), grid)
    return (np.bincount(pid[pid >= 0], minlength=grid.cells) > 0).astype(np.int32)


def both_paths(lib, gpu, name, stride, pitch, choff, case, seed=0):
    """float32 and split, lane path and half-wave path: the float32 lane-path call against the oracle, the rest against it"""
    grid, T = scene(name)[:2]
    pts = scene(name)[2 + seed]
    p = po.params(17 + seed)
    wg = weights(gpu, p)
    a = Sweep(lib, gpu, grid, pts, T, stride, pitch, choff)
    run(lib, [a], wg, 0, case)
    ga = a.got()
    po.check_forward(ga, pts, T, grid, p, case)
    po.exact("occupancy", ga["occupancy"], occupancy_ref(pts, T, grid), case)
    b = Sweep(lib, gpu, grid, pts, T, stride, pitch, choff)
    run(lib, [b], wg, HALFWAVE_ONLY, case + " half-wave only")
    same(b.got(), ga, case + " half-wave only")
    sp = pitch if pitch % 16 == 0 else 48
    for flags in (SPLIT, SPLIT | HALFWAVE_ONLY):
        c = Sweep(lib, gpu, grid, pts, T, stride, sp, choff)
        run(lib, [c], wg, flags, f"{case} flags {flags}")
        gc = c.got(split=True)
        same(gc, ga, f"{case} flags {flags}", ("xyz_t", "pid", "offsets", "start", "order", "occupancy"))
        po.exact("split image", gc["image"], po.split_words(ga["image"]), f"{case} flags {flags}")


# ---- populations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["41x25", "65x1"])
@pytest.mark.parametrize("stride,pitch,choff", LAYOUTS)
def test_populations(lib, gpu, name, stride, pitch, choff):
    both_paths(lib, gpu, name, stride, pitch, choff, f"lanes {name} stride={stride} pitch={pitch}+{choff}")


# ---- extreme blocks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["128x1", "256x1", "64x5"])
def test_extreme_blocks(lib, gpu, name):
    """a word of single-point cells only and a word with one non-empty cell; more few-point (and single-point) cells in a block
    than a wave has lanes; empty words inside a block"""
    both_paths(lib, gpu, name, 3, 32, 0, f"lanes {name}")
    both_paths(lib, gpu, name, 4, 96, 32, f"lanes {name} pitch 96+32", seed=1)


@pytest.mark.parametrize("flags", [0, SPLIT])
def test_empty_sweep_in_a_twelve_sweep_call(lib, gpu, flags):
    grid, T, pts, ptsB = scene("65x1")
    p = po.params(3)
    wg = weights(gpu, p)
    ns = [pts.shape[0] - 5 * i for i in range(12)]
    ns[6] = 0
    clouds = [(pts if i % 2 == 0 else ptsB)[:k] for i, k in enumerate(ns)]
    pitch = 48 if flags else 36
    sweeps = [Sweep(lib, gpu, grid, c, T, 3 + i % 3, pitch, ws_points=max(ns)) for i, c in enumerate(clouds)]
    other = [Sweep(lib, gpu, grid, c, T, 3 + i % 3, pitch, ws_points=max(ns)) for i, c in enumerate(clouds)]
    run(lib, sweeps, wg, flags, f"12 sweeps flags {flags}")
    run(lib, other, wg, flags | HALFWAVE_ONLY, f"12 sweeps flags {flags} half-wave only")
    for i, (sw, ot, c) in enumerate(zip(sweeps, other, clouds)):
        case = f"12 sweeps flags {flags} sweep {i}"
        g = sw.got(bool(flags))
        same(ot.got(bool(flags)), g, case + " half-wave only")
        po.exact("occupancy", g["occupancy"], occupancy_ref(c, T, grid), case)
        if flags:
            one = Sweep(lib, gpu, grid, c, T, 3, 32)
            run(lib, [one], wg, 0, case + " float32")
            g1 = one.got()
            po.check_forward(g1, c, T, grid, p, case + " float32")
            same(g, g1, case, ("xyz_t", "pid", "offsets", "start", "order", "occupancy"))
            po.exact("split image", g["image"], po.split_words(g1["image"]), case)
        else:
            po.check_forward(g, c, T, grid, p, case)


# ---- HIMO_PILLAR_NO_LISTS -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, SPLIT, HALFWAVE_ONLY])
def test_no_lists(lib, gpu, extra):
    """image, occupancy, xyz_t and pid as without the bit; exact offsets where a sweep passes d_offsets; a sweep that passes NULL
    gets nothing written but its other outputs and its workspace"""
    grid, T, pts, ptsB = scene("41x25")
    p = po.params(9)
    wg = weights(gpu, p)
    clouds = [pts, ptsB, pts[:pts.shape[0] // 2]]
    nmax = max(c.shape[0] for c in clouds)
    pitch = 48 if extra & SPLIT else 36
    plain = [Sweep(lib, gpu, grid, c, T, 3, pitch, ws_points=nmax) for c in clouds]
    run(lib, plain, wg, extra, f"lists kept, flags {extra}")
    lean = [Sweep(lib, gpu, grid, c, T, 3, pitch, ws_points=nmax, offsets=(i == 1)) for i, c in enumerate(clouds)]
    run(lib, lean, wg, extra | NO_LISTS, f"no lists, flags {extra}")
    for i, (a, b, c) in enumerate(zip(plain, lean, clouds)):
        case = f"no lists, flags {extra}, sweep {i}"
        ga, gb = a.got(bool(extra & SPLIT)), b.got(bool(extra & SPLIT), lists=False)
        same(gb, ga, case, ("xyz_t", "pid", "image", "occupancy"))
        if i == 1:
            po.exact("offsets", gb["offsets"], po.cells_of(po.transform(c, T), grid)[1], case)
        else:
            assert b.off.untouched(), f"{case}: offsets written through a NULL d_offsets"


def test_null_offsets_without_the_bit_are_refused(lib, gpu):
    grid, T, pts, _ = scene("65x1")
    wg = weights(gpu, po.params(1))
    for flags in (0, SPLIT, HALFWAVE_ONLY, INCREMENTAL):
        sweeps = [Sweep(lib, gpu, grid, pts, T, 3, 48, offsets=(i == 0)) for i in range(2)]
        run(lib, sweeps, wg, flags, f"NULL d_offsets, flags {flags}", want=INVALID)
    empty = Sweep(lib, gpu, grid, pts[:0], T, 3, 32, offsets=False)          # n == 0: no per-point output is looked at
    run(lib, [empty], wg, 0, "NULL d_offsets, n = 0")


# ---- incremental images -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,split", [("65x1", 0), ("41x25", 1), ("41x25", 0)])
def test_incremental(lib, gpu, name, split):
    """passes A, B, empty, A, A over one persistent image equal a fresh image each time, and a cell that emptied is zero"""
    grid, T, ptsA, _ = scene(name)
    wg = weights(gpu, po.params(5))
    pid, _ = po.cells_of(po.transform(ptsA, T), grid)
    half = grid.cells // 2                                   # A: the lower cells and the points outside, B: the upper cells
    A, B = ptsA[(pid < half)], ptsA[pid >= half]
    pitch = 48 if split else 32
    nmax = max(A.shape[0], B.shape[0])
    keep = Sweep(lib, gpu, grid, A, T, 3, pitch, ws_points=nmax)
    assert lib.himo_pillar_occupancy_reset(keep.ws.ptr, keep.ws_bytes, grid.W, grid.H, _s()) == 0
    for k, cloud in enumerate([A, B, A[:0], A, A]):
        case = f"incremental {name} split={split} pass {k}"
        cur = Sweep(lib, gpu, grid, cloud, T, 3, pitch, ws_points=nmax, keep=keep)
        run(lib, [cur], wg, split | INCREMENTAL, case)
        fresh = Sweep(lib, gpu, grid, cloud, T, 3, pitch, ws_points=nmax)
        run(lib, [fresh], wg, split, case + " fresh")
        po.exact("image", cur.img.words().numpy().reshape(-1, 32), fresh.img.words().numpy().reshape(-1, 32), case)
        po.exact("occupancy", cur.got(bool(split))["occupancy"], occupancy_ref(cloud, T, grid), case)
        empty = occupancy_ref(cloud, T, grid) == 0
        assert not cur.img.words().numpy().reshape(-1, 32)[empty].any(), f"{case}: a cell that emptied is not zero"


# ---- the whole network --------------------------------------------------------------------------------------------------------------
def test_network_flow_is_the_same_with_the_switch(gpu):
    """SeFlowNet.head_offsets_only (HIMO_PILLAR_NO_LISTS, NULL d_offsets off the head's sweep): the same flow, bit for bit"""
    from himo_amd.seflow import spec
    from himo_amd.seflow.model import SeFlowNet
    from himo_amd.synthetic import make_frame
    net = SeFlowNet(spec.init_params(0), device=gpu, max_points=6_000, precision="f16x2", max_batch=2, autotune=False)
    assert net.head_offsets_only is False
    samples = []
    for k, cloud in enumerate(("uniform", "rings")):
        fh, f0, f1 = (make_frame(60 + 3 * k + i, n_points=n, cloud=cloud) for i, n in enumerate((4_000, 5_000 - 7 * k, 4_500)))
        up = lambda f: torch.from_numpy(np.ascontiguousarray(f["pc0"])).to(gpu)
        samples.append((up(fh), up(f0), up(f1), fh["pose0"], f0["pose0"], f0["pose1"]))
    flows = {}
    for on in (False, True, False):
        net.head_offsets_only = on
        for st in net._pt:
            st["offsets"].fill_(float("nan"))              # what a stale read would meet
        outs = [torch.full((s[1].shape[0], 3), float("nan"), device=gpu) for s in samples]
        net.forward_batch(samples, outs)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        if on in flows:
            assert all(torch.equal(a, b) for a, b in zip(flows[on], outs))
        flows.setdefault(on, outs)
        if on:                                             # the sweeps off the head's slot got no offsets
            for st in net._pt:
                assert bool(torch.isnan(st["offsets"][0]).all()) and bool(torch.isnan(st["offsets"][2]).all())
    assert all(torch.equal(a, b) for a, b in zip(flows[False], flows[True]))
    net.head_offsets_only = True
    with pytest.raises(ValueError):                        # nobody wrote the offsets of another slot
        net.head_batch([s[1] for s in samples], flows[True], slot0=2, slot1=1)
