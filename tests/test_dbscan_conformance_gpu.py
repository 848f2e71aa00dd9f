"""Conformance of himo_dbscan (csrc/dbscan.hip) through the C ABI, at the places where a cell-grid DBSCAN goes wrong and a random
cloud never is: neighbours across cell boundaries that float32 binning puts two cells apart, exact and near ties of the distance
test, the tile edges of the two-launch scan, the 4096-block cap, min_pts across 64-lane chunks, duplicates, the border rule,
pitches, offsets, grids that are not the production one, and every refusal.

Every accepted call must give the labels of the brute-force reference (oracle/dbscan_exact.py; its agreement with the sklearn
oracle is tests/test_dbscan_oracle.py) and n_clusters == labels.max(), leave its inputs bit-unchanged, write no byte outside
``labels`` / ``n_clusters`` / the workspace, and give the same bits when called again.  xyz, labels and n_clusters live in NaN-filled
guarded buffers (oracle/guarded.py), skip and the workspace in guarded byte buffers; the workspace has exactly the size the
library's query returns and is filled with garbage (another garbage for the second call).  A refused call gets the documented
status and writes nothing at all.

The module prints a summary: the cases per family, which of them differed, and what the generators found.
"""
import math

import numpy as np
import pytest
import torch

import dbscan_exact as de
from guarded import Guarded, GuardedBytes, layout

pytestmark = pytest.mark.gpu

CASES = {}        # family -> number of cases run
DIFFERED = []     # (family, case, what)
GENERATED = {}    # generator -> what it returned
_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\ndbscan conformance: cases per family")
    for fam, k in CASES.items():
        bad = [d for d in DIFFERED if d[0] == fam]
        print(f"  {fam:34s} {k:4d} cases, {len(bad)} differed")
        for _, case, what in bad[:12]:
            print(f"      {case}: {what}")
        if len(bad) > 12:
            print(f"      ... and {len(bad) - 12} more")
    print("  generators: " + "; ".join(f"{k}: {v}" for k, v in GENERATED.items()))


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib
    from himo_amd.seflow import ssl_label                    # noqa: F401  (registers the signatures)
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def prod_grid(eps):
    side = int(math.ceil(104.0 / eps))
    return (-52.0, -52.0, eps, side, side)


def _garbage(ws, seed):
    g = torch.Generator().manual_seed(seed)
    ws.put(torch.randint(0, 256, (ws.nbytes,), dtype=torch.uint8, generator=g))


class Operands:
    """one call's buffers: xyz at ``pitch`` floats per row, ``off`` floats past an aligned base; skip: None (NULL) or bytes"""

    def __init__(self, lib, gpu, pts, skip, grid, pitch=3, off=0, skip_off=0, ws_extra=0):
        n = len(pts)
        self.n, self.pitch, self.grid = n, pitch, grid
        self.xyz = Guarded(layout(1, 1, 0, 0, n, pitch, 3), gpu, off=off)
        if n:
            self.xyz.put(torch.from_numpy(np.ascontiguousarray(pts[:, :3], dtype=np.float32)))
        self.labels = Guarded(layout(1, 1, 0, 0, 1, max(n, 1), n), gpu)
        self.count = Guarded(layout(1, 1, 0, 0, 1, 1, 1), gpu)
        self.skip = None
        if skip is not None:
            self.skip = GuardedBytes(n, gpu, off=skip_off)
            self.skip.put(torch.from_numpy(np.asarray(skip, np.uint8)))
        self.need = int(lib.himo_dbscan_workspace_bytes(n, grid[3], grid[4]))
        self.ws = GuardedBytes(self.need + ws_extra, gpu)
        _garbage(self.ws, 1)
        self.snap()

    def snap(self):
        self.before = [t.buf.clone() for t in (self.xyz, self.skip) if t is not None]
        self.ws_before = self.ws.buf.clone()

    def call(self, lib, eps, min_pts, **change):
        a = dict(n=self.n, xyz=self.xyz.ptr, pitch=self.pitch, skip=self.skip.ptr if self.skip is not None else None, eps=eps, min_pts=min_pts,
                 x0=self.grid[0], y0=self.grid[1], cell=self.grid[2], gw=self.grid[3], gh=self.grid[4], labels=self.labels.ptr,
                 count=self.count.ptr, ws=self.ws.ptr, ws_bytes=self.need)
        a.update(change)
        st = lib.himo_dbscan(a["n"], a["xyz"], a["pitch"], a["skip"], a["eps"], a["min_pts"], a["x0"], a["y0"], a["cell"], a["gw"], a["gh"],
                             a["labels"], a["count"], a["ws"], a["ws_bytes"], _s())
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                               # a HIP error is sticky: nothing after it in this process means anything
            pytest.exit(f"HIP error after himo_dbscan ({a['n']} rows, grid {a['gw']}x{a['gh']}): {e}", returncode=3)
        return st

    def inputs_unchanged(self):
        return all(torch.equal(t.buf, b) for t, b in zip([t for t in (self.xyz, self.skip) if t is not None], self.before))

    def nothing_written(self):
        return self.inputs_unchanged() and self.labels.untouched() and self.count.untouched() and torch.equal(self.ws.buf, self.ws_before)


def run(lib, gpu, fam, case, pts, eps, min_pts, want, skip=None, grid=None, **kw):
    """one accepted call, checked in full; a difference is recorded for the summary and returned as text (None: all held)"""
    grid = grid or prod_grid(eps)
    o = Operands(lib, gpu, pts, skip, grid, **kw)
    CASES[fam] = CASES.get(fam, 0) + 1
    what = None
    st = o.call(lib, eps, min_pts)
    if st != 0:
        what = f"status {st}"
    else:
        got, k = o.labels.words().reshape(-1).numpy(), int(o.count.words().reshape(-1)[0])
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            what = f"{len(bad)} of {len(want)} labels differ, first rows {bad[:4].tolist()} got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}"
        elif k != (int(want.max()) if len(want) else 0):
            what = f"n_clusters {k}, labels.max() {int(want.max()) if len(want) else 0}"
        elif not o.inputs_unchanged():
            what = "an input was written"
        elif not (o.labels.untouched_outside() and o.count.untouched_outside()):
            what = "a write outside labels / n_clusters"
        elif not o.ws.untouched_outside():
            what = "a write past the workspace size the query returned"
        else:
            o.labels.reset()
            o.count.reset()
            _garbage(o.ws, 2)
            st = o.call(lib, eps, min_pts)
            if st != 0 or not np.array_equal(o.labels.words().reshape(-1).numpy(), got) or int(o.count.words().reshape(-1)[0]) != k:
                what = "a second call gave other bits"
    if what:
        DIFFERED.append((fam, case, what))
    return what and f"{case}: {what}"


def ref(key, pts, eps, min_pts, skip=None):
    """the brute-force labels, computed once per input"""
    if key not in _REFS:
        _REFS[key] = de.dbscan_exact(pts, eps, min_pts, skip)
    return _REFS[key]


def _none(failures):
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


# ---- a. neighbours that float32 binning puts two cells apart ----------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.5, 0.4, 0.3, 1.0])
def test_cell_hazard_pairs(lib, gpu, eps):
    """EVERY generated pair exactly-or-nearly eps apart whose cells under floor((x - x0) * (1 / cell)) differ by two, along x and along y, each
    isolated: one cluster each at min_pts 2; at min_pts 3, triples whose middle point is the only core point and whose other two
    lie across such boundaries in x and in y"""
    GENERATED[f"cell-hazard pairs eps {eps}"] = len(de.cell_hazard_pairs(eps))
    out = []
    for min_pts in (2, 3):
        pts = de.hazard_cloud(eps, min_pts=min_pts)
        assert len(pts) == 2 * min_pts * len(de.cell_hazard_pairs(eps))              # every generated pair, along x and along y
        want = ref(("hazard", eps, min_pts), pts, eps, min_pts)
        assert want.min() == 1 and np.all(np.bincount(want)[1:] == min_pts)          # every pair / triple is one cluster
        out.append(run(lib, gpu, "a cell-hazard pairs", f"eps={eps} min_pts={min_pts} n={len(pts)}", pts, eps, min_pts, want))
    _none(out)


# ---- b. exact ties ----------------------------------------------------------------------------------------------------------------
def test_exact_ties(lib, gpu):
    """eps = 0.625 on multiples of 1/8: d2 == eps2 exactly is a neighbour, one step more is not; across and inside cells"""
    name, pts, eps, min_pts, skip, want = de.hand_built()[0]
    assert name.startswith("exact ties") and np.array_equal(ref("ties", pts, eps, min_pts), want)
    _none([run(lib, gpu, "b exact ties", f"grid {g}", pts, eps, min_pts, want, grid=g)
           for g in (prod_grid(eps), (-52.0, -52.0, 1.25, 84, 84), (-51.9375, -52.3125, 0.625, 168, 168))])


# ---- c. pairs on which a contracted a*b + c decides otherwise ---------------------------------------------------------------------
@pytest.mark.parametrize("eps,direction", [(0.5, "in_out"), (0.4, "out_in")])
def test_contraction_sensitive_pairs(lib, gpu, eps, direction):
    """isolated pairs that the unfused float32 sum (dx*dx + dy*dy) + dz*dz puts on one side of eps*eps and every contraction of it
    on the other: in_out pairs are clusters, out_in pairs noise"""
    p, q = de.contraction_pairs(eps, direction)
    GENERATED[f"contraction pairs eps {eps} {direction}"] = len(p)
    assert len(p) >= 32
    pts = np.concatenate([p, q])
    want = ref(("contraction", eps, direction), pts, eps, 2)
    assert np.array_equal(want, np.tile(np.arange(1, len(p) + 1), 2) if direction == "in_out" else np.zeros(2 * len(p)))
    _none([run(lib, gpu, "c contraction-sensitive pairs", f"eps={eps} {direction} pairs={len(p)}", pts, eps, 2, want)])


# ---- d. the scans' edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_scan_edges_in_n(lib, gpu, n):
    """about n / 2 clusters whose lowest indices straddle the tiles of the is_root scan (4096 values per tile, 4 per thread, 64-lane waves)"""
    pts = de.isolated_pairs(n, n)
    want = ref(("pairs", n), pts, 0.5, 2)
    assert want.max() == (n - (n % 2 + 2 * min(3, n // 16))) // 2
    _none([run(lib, gpu, "d scan edges, n", f"n={n} clusters={want.max()}", pts, 0.5, 2, want)])


def _strip(seed, n, x0, y0, w, h, eps):
    """blobs and noise over the w x h m of a grid and 3 % past its far edges (the last cells get points whatever the internal cell)"""
    rng = np.random.default_rng(seed)
    nb = max(4, n // 120)
    ext = np.array([w * 1.03, h * 1.03])
    c = rng.uniform(0, 1, (nb, 2)) * ext
    c[0], c[1] = ext - 0.2 * eps, (ext[0] - 0.3 * eps, 0.4 * eps)
    which = rng.integers(0, nb, n - n // 4)
    xy = np.concatenate([c[which] + rng.normal(0, 0.5 * eps, (len(which), 2)), rng.uniform(0, 1, (n // 4, 2)) * ext])
    pts = np.concatenate([xy + [x0, y0], rng.normal(0, 0.4 * eps, (n, 1))], 1)
    return pts[rng.permutation(n)].astype(np.float32)


@pytest.mark.parametrize("gw,gh", [(1, 1), (65, 63), (64, 64), (4097, 1), (1, 4097), (520, 520)])
def test_scan_edges_in_cells(lib, gpu, gw, gh):
    """grids of 1, 4095, 4096 and 4097 cells (one scan tile, its last value, one value into the second) and of 67 tiles (the
    offsets kernel walks the tile sums 64 at a time), with points in the last cells"""
    eps, x0, y0 = 0.5, -130.0, -7.25
    n = 600 if gw * gh == 1 else 2400
    pts = _strip(gw * 7 + gh, n, x0, y0, max(gw * eps, 12.0), max(gh * eps, 12.0), eps)
    want = ref(("strip", gw, gh), pts, eps, 5)
    assert want.max() >= 2
    _none([run(lib, gpu, "d scan edges, cells", f"grid {gw}x{gh} n={n}", pts, eps, 5, want, grid=(x0, y0, eps, gw, gh))])


# ---- e. one large structured case -------------------------------------------------------------------------------------------------
def test_large_lattice(lib, gpu):
    """524 288 isolated pairs + one singleton on a lattice of multiples of 1/16 (every distance exact: a pair is eps apart, a tie):
    n > 4096 * 256 rows (the block cap of the wave-per-row kernels), 257 scan tiles of is_root and 256 of the cells.  Expected
    labels in O(n): a pair's label is the rank of its lower row index."""
    eps = 0.0625
    i = np.arange(256)
    sx, sy, sz = np.meshgrid(-32.0 + 0.25 * i, -32.0 + 0.25 * i, np.arange(8.0), indexing="ij")
    first = np.stack([sx.ravel(), sy.ravel(), sz.ravel()], 1)
    m = len(first)
    along_x = (np.arange(m) % 2 == 0)[:, None]
    second = first + np.where(along_x, [eps, 0, 0], [0, eps, 0])
    pts = np.concatenate([first, second, [[-32.0 + 0.125, -32.0 + 0.125, 0.5]]]).astype(np.float32)
    n = len(pts)
    assert m == 524_288 and n > 4096 * 256 and np.all(pts * 16 == np.round(pts * 16))
    perm = np.random.default_rng(11).permutation(n)
    pts = pts[perm]
    pair = np.where(perm < 2 * m, perm % m, -1)                 # the pair of every row; -1 the singleton
    rows = np.argsort(pair, kind="stable")[1:].reshape(m, 2)    # the two rows of every pair, ascending
    rank = np.empty(m, np.int64)
    rank[np.argsort(rows[:, 0])] = np.arange(1, m + 1)
    want = np.where(pair >= 0, rank[pair], 0).astype(np.int32)
    _none([run(lib, gpu, "e large lattice", f"n={n}", pts, eps, 2, want, grid=(-32.0, -32.0, eps, 1024, 1024))])


# ---- f. min_pts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_pts", [64, 65, 200])
def test_min_pts_across_chunks(lib, gpu, min_pts):
    """a blob of 300 points (240 dense, 60 around them) on a corner of four cells, 2 m across: the count and its early exit run over
    several 64-lane chunks and rows of cells; neighbourhoods of exactly 64, 199 and 200 points occur"""
    rng = np.random.default_rng(21)
    centre = [-20.0, -20.0, 0.0]
    pts = np.concatenate([rng.normal(centre, 0.18, (240, 3)), rng.normal(centre, 0.45, (60, 3)), rng.uniform(-22, -18, (40, 3))]).astype(np.float32)
    want = ref(("blob300", min_pts), pts, 0.5, min_pts)
    assert want.max() == 1 and 0 < (want == 0).sum()
    _none([run(lib, gpu, "f min_pts", f"blob of 300, min_pts={min_pts} in cluster={int((want == 1).sum())}", pts, 0.5, min_pts, want)])


def test_hand_built_inputs(lib, gpu):
    """min_pts = 1 with inf / NaN / skipped rows, counts equal to and one short of min_pts, 300 identical points, the border
    rule (lowest root wins; clusters touching through a border point stay apart; a border point does not number its cluster),
    NaN in z only, +-inf rows, points 1e6 m outside the grid on every side"""
    out = []
    for name, pts, eps, min_pts, skip, want in de.hand_built()[1:]:
        assert np.array_equal(ref(name, pts, eps, min_pts, skip), want), name
        fam = "g border rule" if name.startswith("border") else ("f min_pts" if "min_pts" in name or "core" in name else "h layout and grid")
        out.append(run(lib, gpu, fam, name, pts, eps, min_pts, want, skip=skip))
    _none(out)


# ---- h. layout and grid -----------------------------------------------------------------------------------------------------------
def _mixed_cloud():
    """blobs + the cell-hazard pairs of (a) + NaN / inf rows"""
    if "mixed" not in _REFS:
        pts = np.concatenate([de.blobs(31, 1500), de.hazard_cloud(0.5, min_pts=2)])
        pts[3::101, 2] = np.nan
        pts[7::173, 0] = np.inf
        pts[11::191, 1] = -np.inf
        _REFS["mixed"] = pts[np.random.default_rng(31).permutation(len(pts))]
    return _REFS["mixed"]


@pytest.mark.parametrize("pitch,off,skip_mode", [(3, 0, "null"), (3, 1, "bytes"), (4, 2, "bytes"), (5, 3, "null"), (7, 1, "bytes")])
def test_pitch_offset_skip(lib, gpu, pitch, off, skip_mode):
    """rows ``pitch`` floats apart from a base 4 * off bytes past a 16-byte boundary (the gaps hold NaN); skip NULL, or bytes of
    0 / 2 / 255 from an odd address"""
    pts = _mixed_cloud()
    skip = None
    if skip_mode == "bytes":
        skip = np.random.default_rng(5).choice(np.array([0] * 14 + [2, 255], np.uint8), len(pts))
    want = ref(("mixed", skip_mode), pts, 0.5, 2, skip)
    assert want.max() > 10
    _none([run(lib, gpu, "h layout and grid", f"pitch={pitch} off={off} skip={skip_mode}", pts, 0.5, 2, want, skip=skip, pitch=pitch, off=off,
               skip_off=1)])


@pytest.mark.parametrize("grid", [(-52.0, -52.0, 0.5, 208, 208), (-52.0, -52.0, 1.0, 104, 104), (-52.0, -52.0, 0.685, 152, 152),
                                  (-52.0, -52.0, 0.5, 208, 100), (-60.5, -41.25, 0.5, 230, 190), (-10.0, 5.0, 0.75, 7, 3)])
def test_same_labels_under_any_grid(lib, gpu, grid):
    """one cloud, the same labels whatever the grid: cell = eps, 2 eps, 1.37 eps, a non-square grid, x0 != y0, a grid most points lie outside"""
    pts = _mixed_cloud()
    out = []
    for min_pts in (2, 8):
        want = ref(("mixed any grid", min_pts), pts, 0.5, min_pts)
        out.append(run(lib, gpu, "h layout and grid", f"grid={grid} min_pts={min_pts}", pts, 0.5, min_pts, want, grid=grid))
    _none(out)


# ---- i. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(lib, gpu):
    """every documented refusal: its status, and not one byte written anywhere (no launch); n = 0 writes n_clusters = 0 and nothing else"""
    from himo_amd import _lib
    INV, WS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_WORKSPACE
    pts = de.blobs(41, 300)
    skip = np.zeros(len(pts), np.uint8)
    o = Operands(lib, gpu, pts, skip, prod_grid(0.5), ws_extra=16)
    table = {"n < 0": (dict(n=-1), INV), "pitch 2": (dict(pitch=2), INV), "eps 0": (dict(eps=0.0), INV), "eps < 0": (dict(eps=-0.5), INV),
             "eps NaN": (dict(eps=float("nan")), INV), "min_pts 0": (dict(min_pts=0), INV), "cell < eps": (dict(cell=0.49999), INV),
             "cell NaN": (dict(cell=float("nan")), INV), "grid_w 0": (dict(gw=0), INV),
             "grid_w * grid_h > 2^26": (dict(gw=16384, gh=4097), INV),
             # the narrower set: a side of more than 2^15 cells (the binning margin does not hold), eps * eps not a normal finite float
             "grid_w > 2^15": (dict(gw=32769, gh=1), INV), "grid_h > 2^15": (dict(gw=1, gh=32769), INV),
             "eps * eps subnormal": (dict(eps=1e-20, cell=1.0), INV), "eps * eps infinite": (dict(eps=1e20, cell=1e20), INV),
             "xyz NULL": (dict(xyz=None), INV), "labels NULL": (dict(labels=None), INV),
             "workspace NULL": (dict(ws=None), WS), "workspace one byte short": (dict(ws_bytes=o.need - 1), WS),
             "workspace 8 bytes off 16-byte alignment": (dict(ws=o.ws.ptr + 8), WS)}
    out = []
    for name, (change, status) in table.items():
        CASES["i refusals"] = CASES.get("i refusals", 0) + 1
        st = o.call(lib, **dict(dict(eps=0.5, min_pts=8), **change))
        what = None if st == status else f"status {st}, expected {status}"
        if not o.nothing_written():
            what = (what + ", " if what else "") + f"refused (status {st}) but wrote"
            o = Operands(lib, gpu, pts, skip, prod_grid(0.5), ws_extra=16)
        if what:
            DIFFERED.append(("i refusals", name, what))
            out.append(f"{name}: {what}")
    assert lib.himo_dbscan_workspace_bytes(-1, 8, 8) == 0 and lib.himo_dbscan_workspace_bytes(8, 0, 8) == 0
    assert lib.himo_dbscan_workspace_bytes(8, 32769, 1) == 0 and lib.himo_dbscan_workspace_bytes(8, 32768, 1) > 0
    # n = 0: accepted, n_clusters = 0, nothing else written (xyz and labels may be NULL)
    CASES["i refusals"] += 1
    e = Operands(lib, gpu, np.zeros((0, 3), np.float32), None, prod_grid(0.5))
    st = e.call(lib, 0.5, 8, xyz=None, labels=None)
    if not (st == 0 and int(e.count.words().reshape(-1)[0]) == 0 and e.count.untouched_outside() and e.labels.untouched()
            and torch.equal(e.ws.buf, e.ws_before)):
        DIFFERED.append(("i refusals", "n = 0", f"status {st}"))
        out.append(f"n = 0: status {st}, n_clusters words {e.count.words().tolist()}")
    _none(out)
