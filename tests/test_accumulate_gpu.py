"""The sweep accumulator on the GPU: ``himo_accum_*`` bit for bit against the numpy restatement of their written rule
(tests/accumulate_ref.py; parity with the reference is unpinned: it has no such program) -- keys, counts, lags and the float32 bits of
the centroids after sorting by key -- over the row counts at which waves and blocks fill, contended voxels, merged runs of lanes, long
probe chains, colliding keys, a full table, split calls, several sources, both pitches, a short output and every refusal; the shared
move against ``himo_rigid_transform``; ``Accumulator`` / ``accumulate_target`` on a toy scene; then the program end to end."""
import ctypes
import warnings

import numpy as np
import pytest

import accumulate_ref as ref
from test_accumulate_cpu import EYE, UNIT, key

pytestmark = pytest.mark.gpu

GUARD, FILL, WORD = 1024, 0xA5, 0x5A5A5A5A                       # guard elements on both sides of every output and of the table
f32 = np.float32


def device_params(**rule):
    from himo_amd.accumulate import AccumParams
    return AccumParams(**rule)


def ac_hash(k, capacity):
    """the kernel's hash, restated: Fibonacci multiplicative on the 32-bit key"""
    return ((int(k) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - int(capacity).bit_length() + 1)


def launch(calls, capacity=64, max_rows=None, pitch=3, call_pitch=None, splits=1, params=None, lag_override=None, **rule):
    """raw calls: clear a guarded table, insert every (rows, T, lag[, skip]) of ``calls`` in ``splits`` calls each, ask for the status,
    emit into guarded outputs.  -> (statuses [clear, inserts ..., status, emit], rows reported, (keys, xyz, lag, count) as emitted,
    guards and everything past the emitted rows untouched?, the table's words)"""
    import torch
    from himo_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    p = params if params is not None else device_params(**rule)
    call_pitch = pitch if call_pitch is None else call_pitch
    words = 8 * (max(int(capacity), 0) + 1) if lib.himo_accum_table_bytes(int(capacity)) else 8 * 65
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    table = torch.full((GUARD + words + GUARD,), WORD, dtype=torch.int32, device=dev)
    t_ptr = table.data_ptr() + 4 * GUARD
    offered = sum(len(c[0]) for c in calls)
    room = offered if max_rows is None else max_rows
    outs = dict(n=torch.full((GUARD + 1 + GUARD,), WORD, dtype=torch.int32, device=dev),
                keys=torch.full((GUARD + room + GUARD,), WORD, dtype=torch.int32, device=dev),
                xyz=torch.full((GUARD + 3 * room + GUARD,), 7.25, dtype=torch.float32, device=dev),
                lag=torch.full((GUARD + room + GUARD,), FILL, dtype=torch.uint8, device=dev),
                count=torch.full((GUARD + room + GUARD,), WORD, dtype=torch.int32, device=dev))
    at = lambda name: outs[name].data_ptr() + GUARD * outs[name].element_size()
    stream = _lib.stream_handle()
    statuses = [lib.himo_accum_clear(t_ptr, int(capacity), stream)]
    keep = []
    for c in calls:
        rows, T, lag = np.asarray(c[0], f32).reshape(-1, 3), np.ascontiguousarray(c[1], f32).reshape(16), int(c[2])
        skip = c[3] if len(c) > 3 else None
        wide = np.concatenate([rows, np.full((len(rows), pitch - 3), 7.0, f32)], axis=1)
        d_rows, d_skip = up(wide.reshape(-1)), None if skip is None else up(np.asarray(skip, np.uint8))
        keep += [d_rows, d_skip]
        cuts = np.linspace(0, len(rows), splits + 1).astype(np.int64)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            statuses.append(lib.himo_accum_insert(int(hi - lo), d_rows.data_ptr() + 4 * pitch * int(lo), call_pitch,
                                                  None if d_skip is None else d_skip.data_ptr() + int(lo), T.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                  lag if lag_override is None else lag_override, ctypes.addressof(p), t_ptr, int(capacity), stream))
    statuses.append(lib.himo_accum_status(stream))
    statuses.append(lib.himo_accum_emit(t_ptr, int(capacity), ctypes.addressof(p), room, at("n"), at("keys"), at("xyz"), at("lag"), at("count"), stream))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    tw = table.cpu().numpy().view(np.uint32)
    clean = bool((tw[:GUARD] == WORD).all() and (tw[GUARD + words:] == WORD).all())
    n_word = host["n"][GUARD]
    clean = clean and bool((host["n"][:GUARD] == WORD).all() and (host["n"][GUARD + 1:] == WORD).all())
    wrote = 0 if statuses[-1] != 0 else min(int(n_word), room)
    clean = clean and (statuses[-1] == 0 or int(n_word) == WORD)     # a refused emit leaves the count alone too
    fills = dict(keys=(1, WORD), xyz=(3, f32(7.25)), lag=(1, FILL), count=(1, WORD))
    got = []
    for name, (per, fill) in fills.items():
        h = host[name]
        clean = clean and bool((h[:GUARD] == fill).all() and (h[GUARD + per * wrote:] == fill).all())     # (the right guard and the unwritten rows)
        got.append(h[GUARD:GUARD + per * wrote].copy())
    keys, xyz, lag, count = got
    return statuses, int(n_word) if statuses[-1] == 0 else None, (keys.view(np.uint32).astype(np.int64), xyz.reshape(-1, 3), lag, count), clean, \
        tw[GUARD:GUARD + words].copy()


def by_key(out):
    keys, xyz, lag, count = out
    order = np.argsort(keys, kind="stable")
    return keys[order], xyz[order], lag[order], count[order]


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def assert_equals_the_restatement(calls, **kw):
    rule = {k: v for k, v in kw.items() if k in ref.DEFAULTS}
    statuses, n, out, clean, _ = launch(calls, **kw)
    assert statuses == [0] * len(statuses) and clean
    want = ref.accumulate(calls, **rule)
    got = by_key(out)
    assert n == len(want[0]) == len(got[0]) and len(set(got[0].tolist())) == n
    assert np.array_equal(got[0], want[0]), "keys differ"
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[2], want[2]), "counts or lags differ"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "centroid bits differ"
    return want


def yaw_pose(yaw, x, y, z=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, z], [0, 0, 0, 1]], np.float64)


def rows_round_the_grid(seed, n):
    """random rows round the 8 x 8 x 4 grid: on voxel faces (every seventh), outside the grid, non-finite, inside the ego box"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1.5, 9.5, (n, 3)).astype(f32)
    rows[:, 2] = rng.uniform(-0.75, 4.75, n)
    rows[::7] = np.floor(rows[::7])
    if n > 40:
        rows[11], rows[29], rows[33] = (np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf)
        rows[13], rows[14] = (2.5, 2.5, 1.5), (2.0, 2.5, 1.5)     # inside the ego box, and on it
    skip = (rng.random(n) < 0.15).astype(np.uint8)
    return rows, skip


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 3000])
def test_row_counts_and_both_pitches(gpu, n):
    rows, skip = rows_round_the_grid(n, n)
    T = ref.relative_pose(yaw_pose(0.3, 0.4, -0.2, 0.1), yaw_pose(0.1, 0.0, 0.3))
    for pitch, t, s in ((3, EYE, None), (4, T, skip)):
        want = assert_equals_the_restatement([(rows, t, 2, s)] if s is not None else [(rows, t, 2)], pitch=pitch, capacity=1024, **UNIT)
        assert n < 63 or len(want[0]) > 5
    if n == 3000:                                                 # (identity: the rows on faces and in the ego box stay where they were put)
        inside = ref.takes_part(rows, **UNIT)
        assert not inside[13] and inside[14] and not inside[11] and (~inside).sum() < 40


def test_contended_voxels_and_merged_runs_of_lanes(gpu):
    rng = np.random.default_rng(9)
    one = rng.uniform((5.0, 5.0, 2.0), (6.0, 6.0, 3.0), (4096, 3)).astype(f32)
    want = assert_equals_the_restatement([(one, EYE, 5)], **UNIT)
    assert want[0].tolist() == [key(5, 5, 2)] and want[3].tolist() == [4096]
    eight = rng.uniform((4.0, 4.0, 1.0), (6.0, 6.0, 3.0), (4096, 3)).astype(f32)
    want = assert_equals_the_restatement([(eight, EYE, 5)], pitch=4, **UNIT)
    assert len(want[0]) == 8 and want[3].sum() == 4096
    # rows in scan order: runs of 1 .. 9 rows of one voxel, some across wave and block boundaries, broken by rows that take no part
    centres = rng.integers(0, (8, 8, 4), (700, 3))
    runs = rng.integers(1, 10, 700)
    rows = (np.repeat(centres, runs, axis=0) + rng.uniform(0.0, 1.0, (int(runs.sum()), 3))).astype(f32)
    rows[5::37] = np.nan
    rows[100:164] = rows[100]                                      # one whole wave and more in one voxel
    skip = np.zeros(len(rows), np.uint8)
    skip[17::53] = 1
    assert_equals_the_restatement([(rows, EYE, 0, skip)], capacity=512, **UNIT)


def test_long_probe_chains_wrap_round_the_table(gpu):
    every = [(ix, iy, iz) for iz in range(4) for iy in range(8) for ix in range(8)]
    late = [v for v in every if ac_hash(key(*v), 64) >= 60]        # more keys than the slots they hash to have before the table's end
    rest = [v for v in every if ac_hash(key(*v), 64) < 60]
    assert len(late) >= 8
    voxels = late + rest[:40 - len(late)] if len(late) < 40 else late[:40]
    rng = np.random.default_rng(4)
    rows = (np.array(voxels, np.float64)[rng.integers(0, len(voxels), 900)] + rng.uniform(0, 1, (900, 3))).astype(f32)
    rows[:len(voxels)] = (np.array(voxels, np.float64) + 0.5).astype(f32)
    ego_out = dict(UNIT, ego_min=(-9.0, -9.0, -9.0), ego_max=(-8.0, -8.0, -8.0))
    want = assert_equals_the_restatement([(rows, EYE, 1)], capacity=64, **ego_out)
    assert len(want[0]) == len(voxels) == 40
    # the table itself: every key sits at or after its hash, cyclically, with no empty slot in between
    _, _, _, _, tw = launch([(rows, EYE, 1)], capacity=64, **ego_out)
    slots = tw.reshape(65, 8)
    held = {int(k): i for i, k in enumerate(slots[:64, 0]) if k != 0xFFFFFFFF}
    assert sorted(held) == want[0].tolist() and slots[64, 1] == 0
    wrapped = 0
    for k, i in held.items():
        h = ac_hash(k, 64)
        d = (i - h) % 64
        assert all(slots[(h + j) % 64, 0] != 0xFFFFFFFF for j in range(d))
        wrapped += i < h
    assert wrapped >= 1


def test_keys_that_collide_under_the_hash(gpu):
    grid = dict(UNIT, nx=64, ny=64, nz=4, ego_min=(-9.0, -9.0, -9.0), ego_max=(-8.0, -8.0, -8.0))
    buckets = {}
    for iz in range(4):
        for iy in range(64):
            for ix in range(64):
                buckets.setdefault(ac_hash(key(ix, iy, iz), 64), []).append((ix, iy, iz))
    worst = max(buckets.values(), key=len)[:24]
    assert len(worst) == 24 and len({ac_hash(key(*v), 64) for v in worst}) == 1
    rng = np.random.default_rng(6)
    rows = (np.array(worst, np.float64)[rng.integers(0, 24, 600)] + rng.uniform(0, 1, (600, 3))).astype(f32)
    rows[:24] = (np.array(worst, np.float64) + 0.25).astype(f32)
    want = assert_equals_the_restatement([(rows, EYE, 9)], capacity=64, **grid)
    assert len(want[0]) == 24


def test_a_full_table_is_a_reported_refusal(gpu):
    from himo_amd import _lib
    lib = _lib.load()
    voxels = [(ix, iy, 0) for iy in range(3) for ix in range(8)][:17]
    rows = (np.array(voxels, np.float64) + 0.5).astype(f32)
    ego_out = dict(UNIT, ego_min=(-9.0, -9.0, -9.0), ego_max=(-8.0, -8.0, -8.0))
    statuses, n, out, clean, _ = launch([(rows, EYE, 0)], capacity=16, **ego_out)
    assert statuses == [0, 0, _lib.ERR_INVALID_ARGUMENT, 0] and clean      # the calls returned; the status call reports; the guards stand
    assert n == 16 and set(out[0].tolist()) < {key(*v) for v in voxels}
    assert lib.himo_accum_status(_lib.stream_handle()) == 0        # reported once
    # sixteen keys fit exactly, and a status call after a clean insert is OK
    statuses, n, out, clean, _ = launch([(rows[:16], EYE, 0)], capacity=16, **ego_out)
    assert statuses == [0, 0, 0, 0] and clean and n == 16
    assert same(by_key(out), ref.accumulate([(rows[:16], EYE, 0)], **ego_out))
    # the Python class raises, once
    import torch
    from himo_amd.accumulate import Accumulator
    acc = Accumulator(gpu, device_params(**ego_out), 16)
    acc.add(torch.from_numpy(rows).to(gpu), EYE, 0)
    with pytest.raises(ValueError, match="full"):
        acc.result()
    acc.clear()
    acc.add(torch.from_numpy(rows[:5]).to(gpu), EYE, 0)
    assert acc.result()[3].tolist() == sorted(key(*v) for v in voxels[:5])


def test_split_calls_several_sources_and_the_same_bytes_twice(gpu):
    rows, skip = rows_round_the_grid(21, 2500)
    more, _ = rows_round_the_grid(22, 1200)
    last, skip2 = rows_round_the_grid(23, 1700)
    T1 = ref.relative_pose(yaw_pose(0.2, 1.0, 0.5), yaw_pose(-0.1, 0.2, 0.1, 0.05))
    T2 = ref.relative_pose(yaw_pose(0.2, 1.0, 0.5), yaw_pose(0.5, -0.7, 0.9))
    calls = [(rows, EYE, 0, skip), (more, T1, 3), (last, T2, 7, skip2)]
    want = assert_equals_the_restatement(calls, capacity=1024, **UNIT)
    assert {0} < set(want[2].tolist()) <= {0, 3, 7}                # (most voxels are reached by the lag-0 source: a few are not)
    runs = [launch(calls, capacity=1024, **UNIT), launch(calls, capacity=1024, **UNIT), launch(calls, capacity=1024, splits=3, pitch=4, **UNIT),
            launch(calls[::-1], capacity=512, splits=2, **UNIT)]
    for st, n, out, clean, _ in runs:
        assert st == [0] * len(st) and clean and same(by_key(out), want)
    # skip NULL against a skip of zeros, and against dropping the skipped rows by hand
    none = launch([(rows, T1, 1)], capacity=1024, **UNIT)
    zeros = launch([(rows, T1, 1, np.zeros(len(rows), np.uint8))], capacity=1024, **UNIT)
    given = launch([(rows, T1, 1, skip)], capacity=1024, **UNIT)
    by_hand = launch([(rows[skip == 0], T1, 1)], capacity=1024, **UNIT)
    assert same(by_key(none[2]), by_key(zeros[2])) and same(by_key(given[2]), by_key(by_hand[2])) and not same(by_key(none[2]), by_key(given[2]))


def test_the_default_grid_and_the_last_key(gpu):
    rng = np.random.default_rng(3)
    n = 3000
    r, az = rng.uniform(0.5, 75.0, n), rng.uniform(-np.pi, np.pi, n)
    rows = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-3.5, 5.5, n)], axis=1).astype(f32)
    T = ref.relative_pose(yaw_pose(0.05, 12.0, 0.4), yaw_pose(0.02, 2.0, 0.1))
    want = assert_equals_the_restatement([(rows, T, 4), (rows, EYE, 0)], capacity=8192, pitch=4)
    assert len(want[0]) > 3000 and (want[0] >> 24).max() >= 79
    # the largest admitted grid: its last voxel's key is the all-ones word, which the table holds in a slot of its own
    wide = dict(UNIT, nx=4096, ny=4096, nz=256)
    rows = np.array([(4095.5, 4095.5, 255.5), (4095.25, 4095.75, 255.5), (0.5, 0.5, 128.5), (0.5, 0.5, 0.5), (4094.5, 4095.5, 255.5)], f32)
    want = assert_equals_the_restatement([(rows, EYE, 2), (rows[:1], EYE, 1)], capacity=16, **wide)
    assert want[0][-1] == 0xFFFFFFFF and want[3][-1] == 3 and want[2][-1] == 1


def test_emit_with_less_room_than_rows(gpu):
    rows, _ = rows_round_the_grid(31, 1500)
    want = ref.accumulate([(rows, EYE, 6)], **UNIT)
    for room in (0, 1, 50, len(want[0]) - 1):
        statuses, n, out, clean, _ = launch([(rows, EYE, 6)], capacity=1024, max_rows=room, **UNIT)
        assert statuses == [0, 0, 0, 0] and clean                   # (clean: nothing past ``room`` rows, in any output)
        assert n == len(want[0]) > room and len(out[0]) == room and len(set(out[0].tolist())) == room
        where = np.searchsorted(want[0], out[0])
        assert np.array_equal(want[0][where], out[0]) and np.array_equal(want[1][where].view(np.uint32), out[1].view(np.uint32))
        assert np.array_equal(want[2][where], out[2]) and np.array_equal(want[3][where], out[3])


def test_refusals_write_nothing(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.accumulate import Accumulator, AccumParams
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_accum_params") == ctypes.sizeof(AccumParams) == 56
    rows, skip = rows_round_the_grid(41, 300)
    calls = [(rows, EYE, 1, skip)]
    bad_arg = _lib.ERR_INVALID_ARGUMENT

    def untouched(result, cleared=True):
        st, n, out, clean, tw = result
        slots = tw.reshape(-1, 8)
        empty = (slots[:, 0] == 0xFFFFFFFF).all() and not slots[:, 1:5].any() if cleared else (tw == WORD).all()
        return clean and bool(empty) and n is None and all(len(o) == 0 for o in out)

    bad = [dict(voxel=0.0), dict(voxel=-0.2), dict(voxel=float("nan")), dict(x0=float("inf")), dict(z0=float("nan")), dict(nx=0), dict(nx=4097),
           dict(ny=4097), dict(nz=257), dict(nz=0), dict(voxel=1e-40), dict(ego_min=(float("nan"), 0.0, 0.0)), dict(ego_max=(0.0, 0.0, float("inf")))]
    for kw in bad:
        res = launch(calls, params=AccumParams(**{**UNIT, **kw}))
        assert res[0] == [0, bad_arg, 0, bad_arg] and untouched(res), kw
    p = AccumParams(**UNIT)
    p.scale = 255.0                                                # not (float)(256.0 / voxel)
    res = launch(calls, params=p)
    assert res[0] == [0, bad_arg, 0, bad_arg] and untouched(res)
    for cp in (5, 2, 0):
        res = launch(calls, call_pitch=cp, max_rows=0, **UNIT)
        assert res[0] == [0, bad_arg, 0, 0] and res[1] == 0 and res[3], cp
    for lag in (-1, 256):
        res = launch(calls, lag_override=lag, max_rows=0, **UNIT)
        assert res[0] == [0, bad_arg, 0, 0] and res[1] == 0 and res[3], lag
    for cap in (0, 8, 24, 63, 1 << 27, -64):                       # a refused capacity: not even the clear runs
        assert lib.himo_accum_table_bytes(cap) == 0
        res = launch(calls, capacity=cap, **UNIT)
        assert res[0] == [bad_arg] * 2 + [0, bad_arg] and untouched(res, cleared=False), cap
    stream = _lib.stream_handle()
    table = torch.full((8 * 17 + 4,), WORD, dtype=torch.int32, device=gpu)
    d_rows, out = torch.from_numpy(rows).to(gpu), torch.full((64,), WORD, dtype=torch.int32, device=gpu)
    T = EYE.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pp, tp, op = ctypes.addressof(p := AccumParams(**UNIT)), table.data_ptr(), out.data_ptr()
    assert lib.himo_accum_clear(None, 16, stream) == lib.himo_accum_clear(tp + 4, 16, stream) == bad_arg                  # NULL, misaligned
    assert lib.himo_accum_insert(-1, d_rows.data_ptr(), 3, None, T, 0, pp, tp, 16, stream) == bad_arg
    assert lib.himo_accum_insert(300, None, 3, None, T, 0, pp, tp, 16, stream) == bad_arg
    assert lib.himo_accum_insert(300, d_rows.data_ptr(), 3, None, None, 0, pp, tp, 16, stream) == bad_arg
    assert lib.himo_accum_insert(300, d_rows.data_ptr(), 3, None, T, 0, None, tp, 16, stream) == bad_arg
    assert lib.himo_accum_insert(300, d_rows.data_ptr(), 3, None, T, 0, pp, None, 16, stream) == bad_arg
    assert lib.himo_accum_insert(300, d_rows.data_ptr(), 3, None, T, 0, pp, tp + 8, 16, stream) == bad_arg
    assert lib.himo_accum_insert(299, d_rows.data_ptr() + 2, 3, None, T, 0, pp, tp, 16, stream) == bad_arg
    assert lib.himo_accum_insert((1 << 31), d_rows.data_ptr(), 3, None, T, 0, pp, tp, 16, stream) == _lib.ERR_UNSUPPORTED
    assert lib.himo_accum_insert(0, None, 3, None, T, 0, pp, tp, 16, stream) == 0                                           # n == 0: OK, no launch
    assert lib.himo_accum_emit(None, 16, pp, 4, op, op + 64, op + 128, op + 192, op + 224, stream) == bad_arg
    assert lib.himo_accum_emit(tp, 16, pp, -1, op, op + 64, op + 128, op + 192, op + 224, stream) == bad_arg
    assert lib.himo_accum_emit(tp, 16, pp, 4, None, op + 64, op + 128, op + 192, op + 224, stream) == bad_arg
    assert lib.himo_accum_emit(tp, 16, pp, 4, op, None, op + 128, op + 192, op + 224, stream) == bad_arg
    assert lib.himo_accum_emit(tp, 16, pp, 4, op, op + 64, op + 128, None, op + 224, stream) == bad_arg
    assert lib.himo_accum_emit(tp, 16, pp, 4, op + 2, op + 64, op + 128, op + 192, op + 224, stream) == bad_arg
    assert lib.himo_accum_emit(tp, 16, pp, 4, op, op + 64, op + 130, op + 192, op + 224, stream) == bad_arg
    assert lib.himo_accum_status(stream) == 0
    torch.cuda.synchronize()
    assert (table == WORD).all().item() and (out == WORD).all().item()
    # the Python entry points refuse before they launch
    with pytest.raises(ValueError):
        Accumulator(gpu, AccumParams(voxel=0.0), 64)
    with pytest.raises(ValueError):
        Accumulator(gpu, AccumParams(**UNIT), 48)
    acc = Accumulator(gpu, AccumParams(**UNIT), 64)
    for wrong in (d_rows[:, :2], d_rows.double(), d_rows.t()):
        with pytest.raises(ValueError):
            acc.add(wrong, EYE, 0)
    with pytest.raises(ValueError):
        acc.add(d_rows, EYE, 256)
    with pytest.raises(ValueError):
        acc.add(d_rows, EYE, 0, skip=torch.zeros(5, dtype=torch.uint8, device=gpu))
    acc.rows = (1 << 24) - 299                                     # rule D: 2^24 rows between two clears, counted here
    with pytest.raises(ValueError, match="2\\^24"):
        acc.add(d_rows, EYE, 0)
    xyz, lag, count, keys = acc.result()
    assert xyz.shape == (0, 3) and lag.numel() == count.numel() == keys.numel() == 0


def test_the_move_is_himo_rigid_transforms(gpu):
    """one device function (csrc/rigid_math.h), one restatement (accumulate_ref.rigid_move): the existing entry point gives its bits"""
    import torch
    from himo_amd.seflow.ssl_label import _moved
    rng = np.random.default_rng(12)
    pts = rng.uniform(-60.0, 60.0, (5000, 3)).astype(f32)
    pts[:, 2] = rng.uniform(-3.0, 5.0, 5000)
    for a, b in ((yaw_pose(0.3, 4.0, -2.0, 0.3), yaw_pose(-0.2, 1.0, 0.5)), (yaw_pose(1.9, -30.0, 12.0), yaw_pose(0.01, 0.1, 0.0, 0.02))):
        T = np.linalg.inv(a) @ b
        T[2, 0], T[2, 1], T[0, 2] = 0.0123, -0.0456, 0.0789        # (no zero terms: every product counts)
        got = _moved(torch.from_numpy(pts).to(gpu), T).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.rigid_move(pts, T.astype(f32)).view(np.uint32))


# ---- the toy scene ---------------------------------------------------------------------------------------------------------------
def toy_scene(seed=2, n_sweeps=4, n=3000):
    rng = np.random.default_rng(seed)
    poses = [yaw_pose(0.04 * k, 1.1 * k, 0.07 * k * k, 0.01 * k) for k in range(n_sweeps)]
    sweeps, skips = [], []
    for k in range(n_sweeps):
        r, az = rng.uniform(0.3, 60.0, n), rng.uniform(-np.pi, np.pi, n)
        pc = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-3.2, 4.0, n), rng.uniform(0, 1, n)], axis=1).astype(f32)
        pc[::97, 0] = np.nan
        sweeps.append(pc)
        skips.append((rng.random(n) < 0.3).astype(np.uint8))
    return sweeps, poses, skips


def test_accumulate_target_on_a_toy_scene(gpu):
    from himo_amd import accumulate as acc
    sweeps, poses, skips = toy_scene()
    for t, window, sk in ((3, 10, None), (3, 2, skips), (0, 10, None), (2, 0, skips)):
        xyz, lag, count, keys = acc.accumulate_target(sweeps, poses, t, window, skips=sk)
        want = ref.accumulate_target([s[:, :3] for s in sweeps], poses, t, window, skips=sk)
        assert xyz.dtype.is_floating_point and lag.dtype.itemsize == 1 and str(count.dtype) == "torch.int32" and xyz.is_cuda
        assert same((keys.cpu().numpy(), xyz.cpu().numpy(), lag.cpu().numpy(), count.cpu().numpy()), want)
        assert set(want[2].tolist()) == set(range(min(t, window) + 1))
    with pytest.raises(ValueError):
        acc.accumulate_target(sweeps, poses, 3, 32)
    # a table of the caller's, used twice: the second target does not see the first one's rows
    table = acc.Accumulator(gpu, None, acc.capacity_for(4 * 3000))
    for t in (3, 1):
        got = acc.accumulate_target(sweeps, poses, t, 10, acc=table)
        want = ref.accumulate_target([s[:, :3] for s in sweeps], poses, t, 10)
        assert same((got[3].cpu().numpy(), got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()), want)


# ---- the program -------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(gpu, tmp_path, capsys):
    import torch
    from himo_amd import accumulate as acc
    from himo_amd.compdis import CompDisEngine
    from himo_amd.dataset import HDF5Dataset
    from himo_amd.synthetic import make_scene, write_h5_scenes
    root = tmp_path / "scenes"
    root.mkdir()
    scenes = [make_scene(60 + s, 5, n_points=2000, scene_id=f"ac{s}", cloud="rings") for s in range(2)]
    write_h5_scenes(root, scenes)

    def compensated(fr):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)
        return CompDisEngine().run_frame(up(fr["pc0"]), up(fr["flow"]), up(fr["lidar_dt"]), fr["pose0"], fr["pose1"], refined=True)[1].cpu().numpy()

    def check(out_dir, window, sweeps_of, skips_of):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ds = HDF5Dataset(out_dir, fields=("pc0", "pose0", "lidar_dt", "gm0", "acc_count"), need_next=False)
        try:
            assert len(ds) == 8                                    # the four sweeps of each scene that have a successor
            rows = 0
            for i in range(len(ds)):
                d = ds[i]
                frames = scenes[int(d["scene_id"][2:])]
                t = [fr["timestamp"] for fr in frames].index(d["timestamp"])
                poses = [fr["pose0"] for fr in frames]
                keys, xyz, lag, count = ref.accumulate_target(sweeps_of(frames), poses, t, window, skips=skips_of(frames))
                lidar = d["pc0"]
                assert lidar.dtype == np.float32 and lidar.shape == (len(keys), 4) and np.array_equal(lidar[:, :3].view(np.uint32), xyz.view(np.uint32))
                assert np.array_equal(lidar[:, 3], lag.astype(f32) * f32(0.1)) and np.array_equal(np.rint(lidar[:, 3] / 0.1), lag)
                assert d["acc_count"].dtype == np.int32 and np.array_equal(d["acc_count"], count)
                assert d["lidar_dt"].shape == (len(keys),) and not d["lidar_dt"].any()
                assert d["gm0"].shape == (len(keys),) and not d["gm0"].any()
                assert d["pose0"].dtype == poses[t].dtype and d["pose0"].tobytes() == np.asarray(poses[t]).tobytes()
                rows += len(keys)
            return rows
        finally:
            ds.close()

    raw = tmp_path / "raw"
    done = acc.main(str(root), str(raw), res_name="raw", window=2)
    printed = capsys.readouterr().out
    assert sorted(done) == ["ac0", "ac1"] and all(s["sweeps"] == 4 and s["rows_in"] == 2000 * (1 + 2 + 3 + 3) for s in done.values())
    assert printed.count("sweeps/s") == 2 and "rows out" in printed
    rows = check(raw, 2, lambda frames: [fr["pc0"][:, :3] for fr in frames], lambda frames: None)
    assert rows == sum(s["rows_out"] for s in done.values()) > 8 * 2000
    # the viewer shows such a file as it stands
    from himo_amd import view
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # (the last target of a scene has no successor in O)
        listing = view.main(str(raw), str(tmp_path / "png"), res_names="raw", index=1, color_by="label:acc_count")
    assert len(listing) == 1 and listing[0]["panels"] == ["raw"] and listing[0]["points"][0] > 2000 and listing[0]["pixels"][0] > 500
    assert (tmp_path / "png" / listing[0]["file"]).stat().st_size > 1000
    with pytest.raises(FileExistsError):
        acc.main(str(root), str(raw), res_name="raw", window=2)
    again = acc.main(str(root), str(raw), res_name="raw", window=2, overwrite=True)
    assert {k: (s["rows_in"], s["rows_out"]) for k, s in again.items()} == {k: (s["rows_in"], s["rows_out"]) for k, s in done.items()}
    # a stored flow, no ground, no labelled rows: the sweeps compensated by the pinned path, then the same rule
    static = tmp_path / "static"
    done = acc.main(str(root), str(static), res_name="flow", window=10, drop_ground=True, drop_label="flow_instance_id")
    skips = lambda frames: [(fr["gm0"] | (fr["flow_instance_id"] != 0)).astype(np.uint8) for fr in frames]
    rows = check(static, 10, lambda frames: [compensated(fr) for fr in frames], skips)
    assert 0 < rows == sum(s["rows_out"] for s in done.values())
    # what is missing is named
    with pytest.raises(KeyError, match="no_such_flow"):
        acc.main(str(root), str(tmp_path / "o1"), res_name="no_such_flow")
    with pytest.raises(KeyError, match="himo_amd.raymap"):
        acc.main(str(root), str(tmp_path / "o2"), res_name="raw", drop_label="ray_label")
