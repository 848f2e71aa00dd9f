"""The whole-drive free-space map on the GPU: ``himo_drivemap_carve`` / ``_query`` / ``_emit`` bit for bit against the numpy restatement
of their written rule (tests/drivemap_ref.py; the reference has no such stage) -- the counts of every voxel, the votes and flags of
every query, the emitted rows, their order and their count -- over the ray counts at which blocks and waves fill, contended words,
split and repeated calls, more than 255 sweeps, every src byte, both pitches, the edge cases and the refusals; the toy drive of
tests/test_raymap_cpu.py through ``DriveMap`` in both origin modes; then the program end to end."""
import ctypes
import json
import pickle
import re
import warnings

import numpy as np
import pytest

import drivemap_ref as ref
from test_raymap_cpu import GROUND, UNIT, ray_cast_sweep
from test_raymap_gpu import rays

pytestmark = pytest.mark.gpu

GUARD, FILL, PAT64 = 1024, 0xA5, 0x5A5A5A5A5A5A5A5A             # guard bytes on both sides of every output, guard words round the map
SMALL = dict(UNIT, guard=1, min_votes=2, min_hits=2)             # the 8 x 8 x 4 grid


def device_params(**rule):
    from himo_amd.drivemap import DriveMapParams
    return DriveMapParams(**rule)


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def wide(a, pitch):
    a = np.asarray(a, np.float32).reshape(-1, 3)
    return np.concatenate([a, np.full((len(a), pitch - 3), 7.0, np.float32)], axis=1).reshape(-1)


class Rig:
    """a cleared map between guard words and every output between guard bytes; the raw calls; what they left"""

    def __init__(self, nq=0, cap=0, params=None, cells=None, **rule):
        import torch
        from himo_amd import _lib
        self.lib, self.dev, self.stream = _lib.load(), torch.device("cuda", 0), _lib.stream_handle()
        self.p = params if params is not None else device_params(**rule)
        self.shape = (int(self.p.nz), int(self.p.ny), int(self.p.nx)) if cells is None else (cells,)
        self.cells, self.nq, self.cap = int(np.prod(self.shape)), int(nq), int(cap)
        self.map = torch.full((GUARD + self.cells + GUARD,), PAT64, dtype=torch.int64, device=self.dev)
        self.map[GUARD:GUARD + self.cells] = 0
        byte_buf = lambda n: torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device=self.dev)
        self.sizes = dict(dyn=self.nq, fv=2 * self.nq, hv=2 * self.nq, rows=16 * self.cap, hits=4 * self.cap, free=4 * self.cap, count=8)
        self.out = {k: byte_buf(n) for k, n in self.sizes.items()}
        need = int(self.lib.himo_drivemap_emit_workspace_bytes(ctypes.addressof(self.p)))
        self.ws = torch.zeros(max(need, 4096) // 4 + 1, dtype=torch.int32, device=self.dev)
        self.ws_bytes = need
        self.P = ctypes.addressof(self.p)
        self.held = []                                                     # the inputs of the asynchronous calls stay alive

    def hold(self, a):
        self.held.append(up(a))
        return self.held[-1].data_ptr()

    def ptr(self, name):
        return self.map.data_ptr() + 8 * GUARD if name == "map" else self.out[name].data_ptr() + GUARD

    def carve(self, ends, srcs, origins, sweep, pitch=3, call_pitch=None, **over):
        n = len(srcs)
        a = dict(n=n, pts=self.hold(wide(ends, pitch)) if n else self.map.data_ptr(), pitch=pitch if call_pitch is None else call_pitch,
                 src=self.hold(np.asarray(srcs, np.uint8)) if n else self.map.data_ptr(),
                 org=self.hold(np.asarray(origins, np.float32).reshape(16, 3)), sweep=int(sweep), P=self.P, map=self.ptr("map"))
        a.update(over)
        return self.lib.himo_drivemap_carve(a["n"], a["pts"], a["pitch"], a["src"], a["org"], a["sweep"], a["P"], a["map"], self.stream)

    def status(self):
        return self.lib.himo_drivemap_status(self.stream)

    def query(self, queries, skip=None, pitch=3, call_pitch=None, **over):
        a = dict(n=len(queries), pts=self.hold(wide(queries, pitch)) if len(queries) else self.map.data_ptr(),
                 pitch=pitch if call_pitch is None else call_pitch, skip=None if skip is None else self.hold(np.asarray(skip, np.uint8)),
                 P=self.P, map=self.ptr("map"), fv=self.ptr("fv"), hv=self.ptr("hv"), dyn=self.ptr("dyn"))
        a.update(over)
        return self.lib.himo_drivemap_query(a["n"], a["pts"], a["pitch"], a["skip"], a["P"], a["map"], a["fv"], a["hv"], a["dyn"], self.stream)

    def emit(self, capacity=None, **over):
        a = dict(P=self.P, map=self.ptr("map"), cap=self.cap if capacity is None else capacity, rows=self.ptr("rows"), hits=self.ptr("hits"),
                 free=self.ptr("free"), count=self.ptr("count"), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        return self.lib.himo_drivemap_emit(a["P"], a["map"], a["cap"], a["rows"], a["hits"], a["free"], a["count"], a["ws"], a["ws_bytes"], self.stream)

    def read(self):
        """-> (words uint64, {name: bytes between the guards}, every guard untouched?)"""
        import torch
        torch.cuda.synchronize()
        g = self.map.cpu().numpy().view(np.uint64)
        clean = bool((g[:GUARD] == PAT64).all() and (g[GUARD + self.cells:] == PAT64).all())
        got = {}
        for k, n in self.sizes.items():
            h = self.out[k].cpu().numpy()
            clean = clean and bool((h[:GUARD] == FILL).all() and (h[GUARD + n:] == FILL).all())
            got[k] = h[GUARD:GUARD + n].copy()
        return g[GUARD:GUARD + self.cells].reshape(self.shape).copy(), got, clean

    def untouched(self):
        words, got, clean = self.read()
        return clean and not words.any() and all((b == FILL).all() for b in got.values())


def assert_equals_the_restatement(calls, queries, skip=None, pitch=3, refused=(), **rule):
    """``calls``: [(pts, src, origins16, sweep)] in order; ``refused``: the indices of the calls the device must refuse (a src byte)"""
    from himo_amd import _lib
    want = ref.DriveMap(**rule)
    for k, (pts, src, origins, sweep) in enumerate(calls):
        if k in refused:
            with pytest.raises(ValueError):
                want.carve(pts, src, origins, sweep)
        else:
            want.carve(pts, src, origins, sweep)
    rows, hits, free = want.emit()
    rig = Rig(nq=len(queries), cap=len(rows), **rule)
    for k, (pts, src, origins, sweep) in enumerate(calls):
        assert rig.carve(pts, src, origins, sweep, pitch=pitch) == 0
        assert rig.status() == (_lib.ERR_INVALID_ARGUMENT if k in refused else 0), k
    assert rig.query(queries, skip, pitch=pitch) == 0 and rig.emit() == 0
    words, got, clean = rig.read()
    assert clean
    free_n, hit_n = ref.counts_of_words(words)
    wf, wh = want.counts()
    assert np.array_equal(free_n, wf) and np.array_equal(hit_n, wh), f"{int(((free_n != wf) | (hit_n != wh)).sum())} of {wf.size} voxels differ"
    assert not ((words >> np.uint64(34)) & np.uint64(0x3FFF)).any()                       # the 14 bits the word leaves at 0
    wd, qf, qh = want.query(queries, skip)
    assert np.array_equal(got["fv"].view(np.uint16), qf) and np.array_equal(got["hv"].view(np.uint16), qh)
    assert set(np.unique(got["dyn"])) <= {0, 1} and np.array_equal(got["dyn"].astype(bool), wd)
    assert int(got["count"].view(np.int64)[0]) == len(rows)
    assert np.array_equal(got["rows"].view(np.float32).reshape(-1, 4), rows) and np.array_equal(got["hits"].view(np.int32), hits)
    assert np.array_equal(got["free"].view(np.int32), free)
    return want, words, wd


def sweeps_of_rays(seed, n, n_sweeps=3):
    """``n_sweeps`` sweeps of ``n`` random rays round the 8 x 8 x 4 grid (tests/test_raymap_gpu.py's: every src 0..15, 255 for a few, ends
    and origins outside, ends on voxel boundaries, NaN and inf), and queries"""
    calls, queries = [], []
    for s in range(n_sweeps):
        pts, src, origins, q = rays(1000 * seed + s, n)
        calls.append((pts, src, origins, 2 * s))                                            # (sweep numbers need not be consecutive)
        queries.append(q)
    return calls, np.concatenate(queries)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("pitch", [3, 4])
def test_ray_counts_and_both_pitches(gpu, n, pitch):
    calls, queries = sweeps_of_rays(n + 1, n)
    skip = (np.arange(len(queries)) % 5 == 0).astype(np.uint8)
    want, words, _ = assert_equals_the_restatement(calls, queries, skip, pitch=pitch, **SMALL)
    free_n, hit_n = want.counts()
    assert n < 63 or (free_n.max() >= 2 and hit_n.any())
    assert n < 1 or set(np.unique(words >> np.uint64(48)).tolist()) <= {0, 1, 3, 5}         # the stamps: sweep + 1


def through_and_into_one_voxel():
    """1000 rays of one sweep THROUGH voxel (4, 4, 1) and 1000 ending IN it"""
    rng = np.random.default_rng(12)
    inside = rng.uniform((4.05, 4.05, 1.05), (4.95, 4.95, 1.95), (1000, 3)).astype(np.float32)
    beyond = (np.float32(0.5) + (inside - np.float32(0.5)) * np.float32(1.6)).astype(np.float32)     # the same directions, further out
    origins = np.tile(np.array([0.5, 0.5, 0.5], np.float32), (16, 1))
    return beyond, inside, origins


def test_one_contended_voxel_in_both_orders_split_and_repeated(gpu):
    beyond, inside, origins = through_and_into_one_voxel()
    src = (np.arange(2000) % 16).astype(np.uint8)
    queries = np.concatenate([inside[:50], beyond[:50]])
    rule = dict(SMALL, guard=0)
    base = None
    for first, second in ((beyond, inside), (inside, beyond)):
        pts = np.concatenate([first, second])
        one = [(pts, src, origins, 7)]
        two = [(pts[:1000], src[:1000], origins, 7), (pts[1000:], src[1000:], origins, 7)]
        three = two + [(pts, src, origins, 7)]                                              # the same 2000 rays again: idempotent
        for calls in (one, two, three):
            want, words, _ = assert_equals_the_restatement(calls, queries, **rule)
            base = words if base is None else base
            assert np.array_equal(words, base)                                              # the same BYTES, not only the same counts
        free_n, hit_n = want.counts()
        assert free_n[1, 4, 4] == 0 and hit_n[1, 4, 4] == 1 and free_n[0, 0, 0] == 1
    # the next sweep sees through the voxel only; the one after that ends in it only
    calls = [(np.concatenate([beyond, inside]), src, origins, 7), (beyond, src[:1000], origins, 8), (inside, src[:1000], origins, 9)]
    want, _, _ = assert_equals_the_restatement(calls, queries, **rule)
    assert want.counts()[0][1, 4, 4] == 1 and want.counts()[1][1, 4, 4] == 2


def test_300_sweeps_count_past_255(gpu):
    origins = np.tile(np.array([0.5, 0.5, 0.5], np.float32), (16, 1))
    calls = [(np.array([[6.5, 0.5, 0.5]] if s % 3 else [[3.5, 0.5, 0.5]], np.float32), np.array([s % 16], np.uint8), origins, s) for s in range(300)]
    queries = np.array([[x + 0.5, 0.5, 0.5] for x in range(8)], np.float32)
    want, words, dyn = assert_equals_the_restatement(calls, queries, **dict(SMALL, min_votes=200, min_hits=100))
    free_n, hit_n = want.counts()
    assert free_n[0, 0, 0] == 300 and hit_n[0, 0, 3] == 100 and free_n[0, 0, 3] == 200 and hit_n[0, 0, 6] == 200
    assert dyn.tolist() == [True, True, True, True, True, False, False, False]             # (voxel 3: 200 > 100; voxel 5: inside the guard of 6)
    assert int(words[0, 0, 0] >> np.uint64(48)) == 300


def test_every_src_byte(gpu):
    from himo_amd import _lib
    pts, src, origins, queries = rays(41, 300)
    assert set(src.tolist()) == set(range(16)) | {255}
    assert_equals_the_restatement([(pts, src, origins, 0)], queries, **SMALL)
    # a src byte of 16: found on the device.  The asynchronous call itself returns OK; the refusal is himo_drivemap_status's answer,
    # once, and the call has marked nothing
    for where, byte in ((0, 16), (150, 200), (299, 254)):
        wrong = src.copy()
        wrong[where] = byte
        rig = Rig(nq=len(queries), **SMALL)
        assert rig.carve(pts, wrong, origins, 3) == 0 and rig.status() == _lib.ERR_INVALID_ARGUMENT and rig.status() == 0
        assert rig.untouched()
    # ... a refused call among good ones refuses only itself
    wrong = src.copy()
    wrong[10] = 16
    calls = [(pts[:100], src[:100], origins, 0), (pts, wrong, origins, 1), (pts[100:], src[100:], origins, 1)]
    assert_equals_the_restatement(calls, queries, refused=(1,), **SMALL)


def test_hand_worked_edge_cases(gpu):
    origins = np.zeros((16, 3), np.float32)
    origins[0], origins[1], origins[2], origins[4] = (0.5, 0.5, 0.5), (3.0, 0.5, 0.5), (-2.5, 0.5, 0.5), (5.5, 0.5, 0.5)
    origins[5], origins[6], origins[7], origins[8] = (np.nan, 0.5, 0.5), (2.0, 2.0, 0.04), (16383.0, 1.0, 1.0), (0.5, np.inf, 0.5)
    big = np.float32(16384.0)
    origins[9], origins[10] = (big, 0.5, 0.5), (0.5, 0.5, -40.5)
    cases = [((5.5, 0.5, 0.5), 0), ((2.5, 2.5, 2.5), 0), ((0.5, 0.5, 0.5), 1), ((1.0, 1.0, 0.04), 6),
             ((2.5, 0.5, 0.5), 2),                                # origin outside the grid
             ((10.5, 0.5, 0.5), 4),                               # end outside the grid
             ((np.nan, 1, 1), 0), ((1, np.inf, 1), 0), ((1, 1, -np.inf), 0), ((big, 1, 1), 0), ((1, -big, 1), 0),
             ((np.nextafter(big, np.float32(0)), 1, 1), 7),       # the last usable value, from an origin as far out
             ((40.5, 0.7, 0.5), 0), ((-30.5, 0.5, 2.5), 4),       # far outside: the walk leaves the grid, in either direction, and may stop
             ((5.5, 0.5, 0.5), 5), ((5.5, 0.5, 0.5), 8), ((5.5, 0.5, 0.5), 9),      # unusable origins: NaN, inf, the 2^22 limit
             ((3.5, 3.5, 3.5), 10),                               # an origin far below the grid
             ((5.5, 0.5, 0.5), 255),                              # no part
             ((0.5, 0.5, 0.5), 0)]                                # origin and end in one voxel: a HIT and nothing else
    pts = np.array([c[0] for c in cases], np.float32)
    src = np.array([c[1] for c in cases], np.uint8)
    queries = np.concatenate([np.nan_to_num(pts, nan=1.5, posinf=1.5, neginf=1.5), pts[6:11]])
    skip = np.zeros(len(queries), np.uint8)
    skip[1] = 1
    for guard in (0, 1, 2):
        rule = dict(SMALL, guard=guard, min_votes=1, min_hits=1)
        want, _, _ = assert_equals_the_restatement([(pts, src, origins, 0), (pts[:6], src[:6], origins, 1)], queries, skip, **rule)
        free_n, hit_n = want.counts()
        assert hit_n[0, 0, 5] == 2 and hit_n[2, 2, 2] == 2 and hit_n[3, 3, 3] == 1 and free_n[0, 0, 7] == 2
    for k in range(len(cases)):                                   # each case alone, so that no other ray's marks can hide a difference
        assert_equals_the_restatement([(pts[k:k + 1], src[k:k + 1], origins, 5)], queries, **dict(SMALL, guard=0, min_hits=1))


LARGER = dict(x0=-20.0, y0=-12.5, z0=-3.0, voxel=0.2, nx=203, ny=127, nz=13, guard=2, min_votes=2, min_hits=1)      # 335153 voxels: 163.6 tiles


def larger_grid_calls():
    """four sweeps of 3000 LiDAR-like rays from three origins each, the rig 2 m further on every sweep"""
    rng = np.random.default_rng(3)
    calls = []
    for s in range(4):
        n = 3000
        origins = np.zeros((16, 3), np.float32)
        origins[:3] = rng.uniform(-1.5, 1.5, (3, 3)) + (2.0 * s, 0.0, -1.0)
        r, az = rng.uniform(0.5, 30.0, n), rng.uniform(-np.pi, np.pi, n)
        pts = (np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-3.5, 0.0, n)], axis=1) + (2.0 * s, 0.0, 0.0)).astype(np.float32)
        calls.append((pts, rng.integers(0, 3, n).astype(np.uint8), origins, s))
    return calls, np.concatenate([c[0] for c in calls])[::3]


def test_a_larger_grid_that_is_no_multiple_of_the_tile(gpu):
    calls, queries = larger_grid_calls()
    want, _, dyn = assert_equals_the_restatement(calls, queries, pitch=4, **LARGER)
    assert want.static().sum() > 100 and dyn.any()


def test_emit_capacities_and_an_empty_map(gpu):
    import torch
    from himo_amd.drivemap import DriveMap
    calls, _ = sweeps_of_rays(5, 400)
    rule = dict(SMALL, min_hits=1)
    want = ref.DriveMap(**rule)
    for c in calls:
        want.carve(*c)
    rows, hits, free = want.emit()
    m = len(rows)
    assert m > 20
    for cap in (m, m - 1, 0, m + 7):
        rig = Rig(cap=cap, **rule)
        for c in calls:
            assert rig.carve(*c) == 0
        assert rig.emit() == 0
        _, got, clean = rig.read()
        k = min(cap, m)
        assert clean and int(got["count"].view(np.int64)[0]) == m, cap                      # the count it needs, whatever the capacity
        assert np.array_equal(got["rows"].view(np.float32).reshape(-1, 4)[:k], rows[:k]) and (got["rows"][16 * k:] == FILL).all()
        assert np.array_equal(got["hits"].view(np.int32)[:k], hits[:k]) and (got["hits"][4 * k:] == FILL).all()
        assert np.array_equal(got["free"].view(np.int32)[:k], free[:k]) and (got["free"][4 * k:] == FILL).all()
    # capacity 0 takes NULL rows; an empty map emits nothing
    rig = Rig(cap=4, **rule)
    assert rig.emit(capacity=0, rows=None, hits=None, free=None) == 0
    _, got, clean = rig.read()
    assert clean and int(got["count"].view(np.int64)[0]) == 0 and (got["rows"] == FILL).all()
    assert rig.emit() == 0
    _, got, clean = rig.read()
    assert clean and int(got["count"].view(np.int64)[0]) == 0 and (got["rows"] == FILL).all() and (got["hits"] == FILL).all()
    # the Python class: exact by default, a refusal that names the count otherwise; sweep numbers do not decrease
    dm = DriveMap(device_params(**rule))
    for pts, src, origins, sweep in calls:
        dm.carve(up(pts), up(src), up(origins), sweep)
    dm.status()
    got = [a.cpu().numpy() for a in dm.emit()]
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], hits) and np.array_equal(got[2], free)
    assert [len(a) for a in dm.emit(capacity=m + 5)] == [m, m, m]
    with pytest.raises(ValueError, match=f"{m} STATIC voxels"):
        dm.emit(capacity=m - 1)
    with pytest.raises(ValueError, match="do not decrease"):
        dm.carve(up(calls[0][0]), up(calls[0][1]), up(calls[0][2]), calls[-1][3] - 1)
    with pytest.raises(ValueError):
        dm.carve(up(calls[0][0]), up(calls[0][1]), up(calls[0][2]), 65535)
    wf, wh = want.counts()
    free_n, hit_n = dm.counts()
    assert np.array_equal(free_n.cpu().numpy(), wf) and np.array_equal(hit_n.cpu().numpy(), wh)
    wrong = calls[0][1].copy()
    wrong[3] = 77
    dm.carve(up(calls[0][0]), up(wrong), up(calls[0][2]), calls[-1][3])
    with pytest.raises(ValueError, match="16..254"):
        dm.status()
    assert torch.equal(dm.counts()[0].cpu(), torch.from_numpy(wf.astype(np.int32)))
    assert not dm.clear().words.any().item() and dm.sweep == -1 and len(dm.emit()[0]) == 0
    with pytest.raises(ValueError):
        DriveMap(device_params(nz=257))


def test_refusals_write_nothing(gpu):
    from himo_amd import _lib
    from himo_amd.drivemap import DriveMapParams, map_bytes
    INV = _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().himo_abi_sizeof(b"himo_drivemap_params") == ctypes.sizeof(DriveMapParams) == 44
    pts, src, origins, queries = rays(41, 300)
    nq = len(queries)
    # parameters
    bad = [dict(voxel=0.0), dict(voxel=-0.2), dict(voxel=float("nan")), dict(x0=float("inf")), dict(z0=float("nan")), dict(nx=0), dict(ny=16385),
           dict(nz=257), dict(nz=0), dict(guard=-1), dict(guard=9), dict(min_votes=0), dict(min_votes=65536), dict(min_hits=0), dict(min_hits=65536),
           dict(voxel=1e-40), dict(nx=16384, ny=16384, nz=3)]
    params = [DriveMapParams(**{**SMALL, **kw}) for kw in bad]
    params.append(DriveMapParams(**SMALL))
    params[-1].scale = 255.0                                      # not (float)(256.0 / voxel)
    for p in params:
        rig = Rig(nq=nq, cap=8, params=p, cells=256)
        rig.ws_bytes = 4096
        assert map_bytes(p) == 0
        assert [rig.carve(pts, src, origins, 0), rig.status(), rig.query(queries), rig.emit()] == [INV, 0, INV, INV] and rig.untouched()
    rig = Rig(nq=nq, cap=8, **SMALL)
    assert rig.carve(pts, src, origins, 0, P=None) == rig.query(queries, P=None) == rig.emit(P=None) == INV
    # arguments: the pitch, the sweep number, the counts, NULL, alignment, the workspace
    some = rig.hold(np.zeros(64, np.float32))
    for cp in (5, 2, 0):
        assert rig.carve(pts, src, origins, 0, call_pitch=cp) == rig.query(queries, call_pitch=cp) == INV, cp
    for sweep in (-1, 65535, 1 << 20):
        assert rig.carve(pts, src, origins, sweep) == INV, sweep
    assert rig.carve(pts, src, origins, 0, n=-1) == rig.query(queries, n=-1) == rig.emit(capacity=-1) == INV
    assert rig.carve(pts, src, origins, 0, n=1 << 31) == rig.query(queries, n=1 << 31) == _lib.ERR_UNSUPPORTED
    for name in ("pts", "src", "org", "map"):
        assert rig.carve(pts, src, origins, 0, **{name: None}) == INV, name
    for name, off in (("pts", 2), ("org", 2), ("map", 4)):
        assert rig.carve(pts, src, origins, 0, **{name: (rig.ptr("map") if name == "map" else some) + off}) == INV, name
    for name in ("pts", "map"):
        assert rig.query(queries, **{name: None}) == INV, name
    for name, off in (("pts", 2), ("map", 4), ("fv", 1), ("hv", 1)):
        assert rig.query(queries, **{name: (rig.ptr(name) if name != "pts" else some) + off}) == INV, name
    for name in ("map", "count", "ws", "rows", "hits", "free"):
        assert rig.emit(**{name: None}) == INV, name
    for name, off in (("map", 4), ("count", 4), ("rows", 2), ("hits", 2), ("free", 2)):
        assert rig.emit(**{name: rig.ptr(name) + off}) == INV, name
    assert rig.emit(ws=rig.ws.data_ptr() + 2) == INV
    assert rig.emit(ws_bytes=rig.ws_bytes - 1) == _lib.ERR_WORKSPACE and rig.emit(ws_bytes=0) == _lib.ERR_WORKSPACE
    assert rig.status() == 0 and rig.untouched()
    # n = 0 is OK and launches nothing; NULL outputs of the query are left out
    assert rig.carve(pts[:0], src[:0], origins, 0, pts=None, src=None, org=None, map=None) == 0 and rig.query(queries[:0], pts=None, map=None) == 0
    assert rig.untouched()
    assert rig.carve(pts, src, origins, 0) == 0 and rig.query(queries, fv=None, dyn=None) == 0
    words, got, clean = rig.read()
    want = ref.DriveMap(**SMALL)
    want.carve(pts, src, origins, 0)
    assert clean and (got["fv"] == FILL).all() and (got["dyn"] == FILL).all() and np.array_equal(got["hv"].view(np.uint16), want.query(queries)[2])


# ---- the toy drive -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_drive():
    sweeps = [ray_cast_sweep(k) for k in range(11)]
    return [s[0] for s in sweeps], [s[1] for s in sweeps], [s[2] for s in sweeps]


@pytest.mark.parametrize("origins", ["frame", "sensors"])
def test_toy_drive_through_the_class(gpu, toy_drive, origins):
    import torch
    from himo_amd.drivemap import DriveMap, carve_drive, relative_poses, scene_extent
    from himo_amd.raymap import _device_points
    clouds, kinds, poses = toy_drive
    ids = [((np.arange(len(c)) % 3) * 4 + 2).astype(np.uint8) for c in clouds]                # sensor ids 2, 6, 10
    centres = [np.array([[3.5, 0.0, 0.5], [0.0, 1.2, 0.0], [0.0, -1.2, 0.0]]) for _ in clouds]
    p = scene_extent(poses, range_m=46.0)
    T = relative_poses(poses)
    on_dev = [_device_points(c, gpu) for c in clouds]
    words = []
    for run in range(2):
        dm = DriveMap(p, gpu)
        moved, sources = carve_drive(dm, on_dev, T, origins, ids, centres)
        dm.status()
        words.append(dm.words.clone())
    assert torch.equal(words[0], words[1])                                                   # two runs: the same bytes, nothing masked
    rule = {k: getattr(p, k) for k in ref.DEFAULTS}
    want = ref.DriveMap(**rule)
    for k, (m, (src, table)) in enumerate(zip(moved, sources)):
        assert (src.max() == 0 and not table[1:].any()) if origins == "frame" else (set(src.tolist()) == {0, 1, 2} and table[:3].any(axis=1).all())
        want.carve(m.cpu().numpy(), src, table, k)
    free_n, hit_n = ref.counts_of_words(dm.words.cpu().numpy().view(np.uint64))
    wf, wh = want.counts()
    assert np.array_equal(free_n, wf) and np.array_equal(hit_n, wh) and wf.max() >= 5
    for t in (0, 5, 10):
        dyn, fv, hv = dm.query(moved[t], torch.from_numpy(kinds[t] == GROUND).to(gpu))
        wd, qf, qh = want.query(moved[t].cpu().numpy(), kinds[t] == GROUND)
        assert np.array_equal(dyn.cpu().numpy().astype(bool), wd) and np.array_equal(fv.cpu().numpy(), qf) and np.array_equal(hv.cpu().numpy(), qh)
    assert want.query(moved[5].cpu().numpy(), kinds[5] == GROUND)[0].any()
    rows, hits, free = want.emit()
    got = [a.cpu().numpy() for a in dm.emit()]
    assert len(rows) > 1000 and np.array_equal(got[0], rows) and np.array_equal(got[1], hits) and np.array_equal(got[2], free)


# ---- the program -------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(gpu, tmp_path, capsys):
    from himo_amd import drivemap, h5lite
    from himo_amd.dataset import open_dataset
    from himo_amd.raymap import _device_points
    from himo_amd.seflow.fit import train_fields
    from himo_amd.synthetic import make_scene, write_h5_scenes
    root, out = tmp_path / "scenes", tmp_path / "maps"
    root.mkdir()
    scenes = [make_scene(90 + s, 6, n_points=3000, scene_id=f"dm{s}", cloud="rings") for s in range(2)]
    write_h5_scenes(root, scenes)
    with pytest.raises(ValueError, match="--map_out"):
        drivemap.main(str(root), map_out=str(root))
    js = tmp_path / "numbers.json"
    done = drivemap._cli(["--data_dir", str(root), "--map_out", str(out), "--json", str(js)])
    printed = capsys.readouterr().out
    assert sorted(done) == ["dm0", "dm1"] and all(s["sweeps"] == 6 and s["points"] == 18_000 for s in done.values())
    numbers = json.loads(js.read_text())["scenes"]
    for sc, s in done.items():
        line = [ln for ln in printed.splitlines() if ln.startswith(f"{sc}:")]
        assert len(line) == 1 and "sweeps/s" in line[0]
        m = re.match(rf"{sc}: (\d+) sweeps, (\d+) points, ([\d.]+) % dynamic, (\d+) clusters, (\d+) static voxels, map ([\d.]+) MiB", line[0])
        assert [int(m.group(k)) for k in (1, 2, 4, 5)] == [numbers[sc][k] for k in ("sweeps", "points", "clusters", "static_voxels")]
        assert m.group(3) == f"{100.0 * numbers[sc]['dynamic'] / numbers[sc]['points']:.1f}" and m.group(6) == f"{numbers[sc]['map_mib']:.1f}"
        assert {k: v for k, v in numbers[sc].items() if k != "seconds"} == {k: v for k, v in s.items() if k != "seconds"}
        assert s["static_voxels"] > 0
    with pytest.raises(FileExistsError):
        drivemap.main(str(root))
    with pytest.raises(FileExistsError):
        drivemap.main(str(root), key="other")                     # the flags are there already
    again = drivemap.main(str(root), overwrite=True)
    strip = lambda d: {k: {n: v for n, v in s.items() if n != "seconds"} for k, s in d.items()}
    assert strip(again) == strip(done)
    for frames in scenes:
        with h5lite.File(root / f"{frames[0]['scene_id']}.h5") as f:
            for fr in frames:
                g = f[str(fr["timestamp"])]
                lab, dyn = g["map_label"], g["map_dynamic"]
                assert lab.dtype == np.int32 and dyn.dtype == np.uint8 and lab.shape == dyn.shape == (3000,)
                lab, dyn = lab[:], dyn[:]
                assert lab.min() >= 0 and set(np.unique(dyn)) <= {0, 1} and not dyn[fr["gm0"]].any() and not lab[fr["gm0"]].any()
    # the stored flags of one sweep against the restatement fed the device's own moved points
    clouds, poses, grounds = [fr["pc0"] for fr in scenes[0]], [fr["pose0"] for fr in scenes[0]], [fr["gm0"] for fr in scenes[0]]
    p = drivemap.scene_extent(poses)
    dm = drivemap.DriveMap(p, gpu)
    moved, sources = drivemap.carve_drive(dm, [_device_points(c, gpu) for c in clouds], drivemap.relative_poses(poses))
    want = ref.DriveMap(**{k: getattr(p, k) for k in ref.DEFAULTS})
    for k, (m, (src, table)) in enumerate(zip(moved, sources)):
        want.carve(m.cpu().numpy(), src, table, k)
    wd, _, _ = want.query(moved[2].cpu().numpy(), grounds[2])
    with h5lite.File(root / "dm0.h5") as f:
        assert np.array_equal(f[str(scenes[0][2]["timestamp"])]["map_dynamic"][:].astype(bool), wd)
    assert int(want.static().sum()) == done["dm0"]["static_voxels"]
    # the loader serves the labels of both sweeps of a pair
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # (the last sweep of a scene has no successor)
        ds = open_dataset(root, fields=train_fields("map_label"), zero_copy=True)
        try:
            f0 = ds[0]
            assert "map_label" in f0 and "map_label_next" in f0 and len(f0["map_label_next"]) == len(f0["pc1"])
        finally:
            ds.close()
        # the static maps open as a dataset of one sweep per scene
        with open(out / "index_total.pkl", "rb") as fh:
            assert pickle.load(fh) == [[f"dm{s}", str(scenes[s][0]["timestamp"])] for s in range(2)]
        ms = open_dataset(out, fields=("pc0", "pose0", "map_hits", "map_free"), need_next=False)
        try:
            assert len(ms) == 2
            for i in range(2):
                item = ms[i]
                n = done[item["scene_id"]]["static_voxels"]
                assert item["pc0"].shape[0] == n and item["map_hits"].dtype == np.int32 and len(item["map_hits"]) == len(item["map_free"]) == n
                assert (item["map_hits"] >= 2).all() and np.allclose(item["pose0"], scenes[i][0]["pose0"])
        finally:
            ms.close()
    # per-sensor origins: refused by name on files without the centres, before anything is written; served once they are there
    with pytest.raises(KeyError, match="SensorsCenter"):
        drivemap.main(str(root), key="s_label", dynamic_key="s_dynamic", origins="sensors")
    with h5lite.File(root / "dm0.h5") as f:
        assert all("s_label" not in f[ts] and "s_dynamic" not in f[ts] for ts in f.keys())
    rig = tmp_path / "rig"
    rig.mkdir()
    centres = np.array([[3.5, 0.0, 0.5], [0.0, 1.2, 0.0], [0.0, -1.2, 0.0], [-1.0, 0.0, 0.3], [1.0, 0.6, 0.2], [1.0, -0.6, 0.2]], np.float32)
    tree = {str(fr["timestamp"]): {"lidar": fr["pc0"], "pose": fr["pose0"], "ground_mask": fr["gm0"], "lidar_id": fr["lidar_id"],
                                   "SensorsCenter": centres[:len(np.unique(fr["lidar_id"]))]} for fr in scenes[0]}
    h5lite.write_file(rig / "dm0.h5", tree)
    sens = drivemap.main(str(rig), origins="sensors")
    assert sens["dm0"]["sweeps"] == 6 and sens["dm0"]["static_voxels"] > 0
    # a scene without ground masks is refused by name
    bare = tmp_path / "bare"
    bare.mkdir()
    h5lite.write_file(bare / "dm0.h5", {ts: {"lidar": g["lidar"], "pose": g["pose"]} for ts, g in list(tree.items())[:3]})
    with pytest.raises(KeyError, match="himo_amd.ground_seg"):
        drivemap.main(str(bare))
