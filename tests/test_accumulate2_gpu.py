"""Sweep accumulation, v2, on the GPU: ``himo_accum_insert_ex`` / ``himo_accum_emit_ex`` / ``himo_accum_motion`` bit for bit against
the numpy restatement of their written rule (tests/accumulate2_ref.py; parity with the reference is unpinned: it has no such
program) -- keys, counts, lags, the float32 bits of the centroids and of the intensities, and the labels, after sorting by key -- over
the row counts at which waves and blocks fill, both pitches and attribute strides, a run of one voxel across a wave's edge, waves in
which no lane merges, motions that leave the grid, v1 and v2 inserts mixed in one table, a short output, either v2 output left out,
every refusal, and colliding and wrapping probe chains; ``Accumulator.result_ex`` / ``accumulate_target`` / ``flow_motion`` on a toy
scene; the translating body that is why the feature exists; then the program end to end."""
import ctypes
import warnings

import numpy as np
import pytest

import accumulate2_ref as ref2
import accumulate_ref as ref
from test_accumulate2_cpu import FAR_EGO, translating_body
from test_accumulate_cpu import EYE, UNIT, key
from test_accumulate_gpu import FILL, GUARD, WORD, ac_hash, device_params, rows_round_the_grid, toy_scene, yaw_pose
from test_accumulate_gpu import launch as launch_v1

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = ("keys", "xyz", "lag", "count", "intensity", "label")


def call(rows, lag=0, T=EYE, **extras):
    """one insert: ``rows`` [n, 3], and any of skip, motion, motion_min, attr, attr_scale, label; ``v1=True`` goes through
    ``himo_accum_insert``"""
    return dict(rows=np.asarray(rows, f32).reshape(-1, 3), T=T, lag=lag, **extras)


def rule_of(c):
    return {k: v for k, v in c.items() if k != "v1"}


def launch(calls, capacity=64, max_rows=None, pitch=3, attr_stride=1, emit_scale=1.0, want=(True, True), override=None, params=None, **rule):
    """raw calls: clear a guarded table, insert every call (``himo_accum_insert_ex``, or ``himo_accum_insert`` for ``v1=True``), ask for
    the status, ``himo_accum_emit_ex`` into guarded outputs (``want``: whether the intensity / label pointer is passed).  With pitch 4
    and stride 4 the attribute is column 3 of the rows, read in place.  ``override``: arguments of every insert_ex replaced by name.
    -> (statuses [clear, inserts ..., status, emit], rows reported, the six columns as emitted, guards and everything past the emitted
    rows untouched?, the table's words)"""
    import torch
    from himo_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    p = params if params is not None else device_params(**rule)
    words = 8 * (int(capacity) + 1)
    assert lib.himo_accum_table_bytes(int(capacity)) == 4 * words
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731
    table = torch.full((GUARD + words + GUARD,), WORD, dtype=torch.int32, device=dev)
    t_ptr = table.data_ptr() + 4 * GUARD
    room = sum(len(c["rows"]) for c in calls) if max_rows is None else max_rows
    outs = dict(n=torch.full((GUARD + 1 + GUARD,), WORD, dtype=torch.int32, device=dev),
                keys=torch.full((GUARD + room + GUARD,), WORD, dtype=torch.int32, device=dev),
                xyz=torch.full((GUARD + 3 * room + GUARD,), 7.25, dtype=torch.float32, device=dev),
                lag=torch.full((GUARD + room + GUARD,), FILL, dtype=torch.uint8, device=dev),
                count=torch.full((GUARD + room + GUARD,), WORD, dtype=torch.int32, device=dev),
                intensity=torch.full((GUARD + room + GUARD,), 7.25, dtype=torch.float32, device=dev),
                label=torch.full((GUARD + room + GUARD,), WORD, dtype=torch.int32, device=dev))
    at = lambda name: outs[name].data_ptr() + GUARD * outs[name].element_size()      # noqa: E731
    stream = _lib.stream_handle()
    statuses = [lib.himo_accum_clear(t_ptr, int(capacity), stream)]
    keep = []
    for c in calls:
        rows, n = c["rows"], len(c["rows"])
        T = np.ascontiguousarray(c["T"], f32).reshape(16).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        attr = None if c.get("attr") is None else np.asarray(c["attr"], f32).reshape(n)
        in_place = attr is not None and pitch == 4 and attr_stride == 4
        wide = np.concatenate([rows, np.full((n, pitch - 3), 7.0, f32)], axis=1)
        if in_place:
            wide[:, 3] = attr
        d_rows = up(wide.reshape(-1))
        d_skip = None if c.get("skip") is None else up(np.asarray(c["skip"], np.uint8))
        d_motion = None if c.get("motion") is None else up(np.asarray(c["motion"], f32).reshape(n, 3))
        d_label = None if c.get("label") is None else up(np.asarray(c["label"], np.int32).reshape(n))
        d_attr = None
        if attr is not None and not in_place:
            strided = np.full((n, attr_stride), -3.0, f32)
            strided[:, 0] = attr
            d_attr = up(strided.reshape(-1))
        keep += [d_rows, d_skip, d_motion, d_label, d_attr]
        ptr = lambda t: None if t is None else t.data_ptr()                          # noqa: E731
        if c.get("v1"):
            statuses.append(lib.himo_accum_insert(n, d_rows.data_ptr(), pitch, ptr(d_skip), T, int(c["lag"]), ctypes.addressof(p), t_ptr, int(capacity),
                                                  stream))
            continue
        args = dict(motion=ptr(d_motion), motion_min2=float(ref2.motion_min2(c.get("motion_min", 0.0))),
                    attr=d_rows.data_ptr() + 12 if in_place else ptr(d_attr), stride=attr_stride, scale=float(f32(c.get("attr_scale", 1.0))),
                    label=ptr(d_label))
        args.update(override or {})
        statuses.append(lib.himo_accum_insert_ex(n, d_rows.data_ptr(), pitch, ptr(d_skip), T, int(c["lag"]), ctypes.addressof(p), t_ptr, int(capacity),
                                                 args["motion"], args["motion_min2"], args["attr"], args["stride"], args["scale"], args["label"], stream))
    statuses.append(lib.himo_accum_status(stream))
    statuses.append(lib.himo_accum_emit_ex(t_ptr, int(capacity), ctypes.addressof(p), room, at("n"), at("keys"), at("xyz"), at("lag"), at("count"),
                                           float(emit_scale), at("intensity") if want[0] else None, at("label") if want[1] else None, stream))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    tw = table.cpu().numpy().view(np.uint32)
    clean = bool((tw[:GUARD] == WORD).all() and (tw[GUARD + words:] == WORD).all())
    n_word = host["n"][GUARD]
    clean = clean and bool((host["n"][:GUARD] == WORD).all() and (host["n"][GUARD + 1:] == WORD).all())
    wrote = 0 if statuses[-1] != 0 else min(int(n_word), room)
    clean = clean and (statuses[-1] == 0 or int(n_word) == WORD)     # a refused emit leaves the count alone too
    fills = dict(keys=(1, WORD), xyz=(3, f32(7.25)), lag=(1, FILL), count=(1, WORD), intensity=(1, f32(7.25)), label=(1, WORD))
    got = []
    for name, (per, fill) in fills.items():
        h = host[name]
        mine = wrote if (name != "intensity" or want[0]) and (name != "label" or want[1]) else 0      # a NULL output: nothing is written at all
        clean = clean and bool((h[:GUARD] == fill).all() and (h[GUARD + per * mine:] == fill).all())
        got.append(h[GUARD:GUARD + per * mine].copy())
    got[0], got[1] = got[0].view(np.uint32).astype(np.int64), got[1].reshape(-1, 3)
    return statuses, int(n_word) if statuses[-1] == 0 else None, tuple(got), clean, tw[GUARD:GUARD + words].copy()


def by_key(out):
    order = np.argsort(out[0], kind="stable")
    return tuple(o[order] if len(o) == len(order) else o for o in out)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), f"{name} differ"


def assert_equals_the_restatement(calls, emit_scale=1.0, **kw):
    rule = {k: v for k, v in kw.items() if k in ref.DEFAULTS}
    statuses, n, out, clean, _ = launch(calls, emit_scale=emit_scale, **kw)
    assert statuses == [0] * len(statuses) and clean
    want = ref2.accumulate([rule_of(c) for c in calls], emit_scale, **rule)
    got = by_key(out)
    assert n == len(want[0]) == len(got[0]) and len(set(got[0].tolist())) == n
    assert_same(got, want)
    return want


def extras_for(seed, rows, scale=255.0, big=False):
    """a motion (a few non-finite, a few tiny), an intensity (NaN, negative and past the top among them) and a label (negative, 0 and
    past 2^24 among them) per row"""
    rng = np.random.default_rng(1000 + seed)
    n = len(rows)
    motion = rng.uniform(-0.6, 0.6, (n, 3)).astype(f32) * f32(20.0 if big else 1.0)
    motion[::5] *= f32(0.01)
    attr = rng.uniform(-0.05, 1.1, n).astype(f32) * f32(255.0 / scale)
    label = rng.integers(-3, 40, n).astype(np.int32)
    if n > 40:
        motion[7, 0], motion[19, 2], motion[23, 1] = np.nan, np.inf, -np.inf
        attr[3], attr[9] = np.nan, np.inf
        label[4], label[6], label[10] = 1 << 24, (1 << 24) - 1, -(1 << 31)
    return dict(motion=motion, motion_min=0.05, attr=attr, attr_scale=scale, label=label)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_row_counts_both_pitches_and_both_strides(gpu, n):
    rows, skip = rows_round_the_grid(n, n)
    T = ref.relative_pose(yaw_pose(0.3, 0.4, -0.2, 0.1), yaw_pose(0.1, 0.0, 0.3))
    for pitch, stride, t, s, scale in ((3, 1, EYE, None, 255.0), (4, 4, T, skip, 255.0), (4, 1, T, None, 1.0), (3, 4, EYE, skip, 100.0)):
        c = call(rows, 2, t, skip=s, **extras_for(n, rows, scale))
        want = assert_equals_the_restatement([c], scale, pitch=pitch, attr_stride=stride, capacity=1024, **UNIT)
        assert n < 63 or (len(want[0]) > 5 and len(set(want[5].tolist())) > 3 and len(set(want[4].tolist())) > 5)


def test_a_run_of_one_voxel_across_a_waves_edge_and_waves_without_a_merge(gpu):
    rng = np.random.default_rng(9)
    one = rng.uniform((5.0, 5.0, 2.0), (6.0, 6.0, 3.0), (130, 3)).astype(f32)       # 130 rows, one voxel: lanes 0..63, 64..127, 128, 129
    c = call(one, 5, attr=rng.uniform(0.0, 300.0, 130).astype(f32), label=rng.integers(1, 1000, 130).astype(np.int32))
    want = assert_equals_the_restatement([c], **UNIT)
    assert want[0].tolist() == [key(5, 5, 2)] and want[3].tolist() == [130] and want[5].tolist() == [int(c["label"].max())]
    # the same rows behind 40 of another voxel: the run starts mid-wave and crosses two wave edges
    lead = rng.uniform((1.0, 1.0, 0.0), (2.0, 2.0, 1.0), (40, 3)).astype(f32)
    both = call(np.concatenate([lead, one]), 5, attr=np.concatenate([np.full(40, 7.0, f32), c["attr"]]),
                label=np.concatenate([np.full(40, 2000, np.int32), c["label"]]))
    want = assert_equals_the_restatement([both], pitch=4, attr_stride=4, **UNIT)
    assert want[3].tolist() == [40, 130] and want[5].tolist() == [2000, int(c["label"].max())] and want[4][0] == 7.0
    # alternating keys: no lane has its neighbour's voxel, so no wave merges
    a, b = rng.uniform((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (150, 3)), rng.uniform((6.0, 6.0, 3.0), (7.0, 7.0, 4.0), (150, 3))
    rows = np.stack([a, b], axis=1).reshape(-1, 3).astype(f32)
    want = assert_equals_the_restatement([call(rows, 3, **extras_for(5, rows, 255.0) | dict(motion=None))], 255.0, **UNIT)
    assert want[0].tolist() == [key(0, 0, 0), key(6, 6, 3)] and want[3].tolist() == [150, 150]


def test_motions_out_of_the_grid_past_the_limit_and_onto_faces(gpu):
    rows, skip = rows_round_the_grid(51, 600)
    ex = extras_for(51, rows, 255.0, big=True)                     # lag 3 x up to 12 m: most rows leave the 8 x 8 x 4 grid
    m = ex["motion"]
    m[30:40] = (f32(1.0e30), 0, 0)                                 # finite, and far past 2^22 sub-voxel units
    m[40:44] = (f32(3.0e38), f32(3.0e38), 0)                       # s overflows to +inf: moved, to a non-finite place
    on = np.arange(50, 90)
    rows[on] = np.floor(rows[on]) + f32(0.25)                      # ... and onto voxel faces: x + 3 * m is a whole number exactly
    m[on] = np.array((0.25, 0.25, 0.25), f32)
    calls = [call(rows, 3, skip=skip, **dict(ex, motion=m))]
    want = assert_equals_the_restatement(calls, 255.0, capacity=1024, **FAR_EGO)
    moved, finite = ref2.advect(rows, m, 3, ref2.motion_min2(0.05))
    assert finite.sum() == 600 - 3 and not np.isfinite(moved[40:44]).all()
    assert (moved[on] == np.floor(moved[on])).all()                # 0.25 + 3 * 0.25: on a face
    still = ref2.accumulate([dict(rule_of(calls[0]), motion=None)], 255.0, **FAR_EGO)
    assert 20 < len(want[0]) < len(still[0])


def test_v1_and_v2_inserts_in_one_table(gpu):
    rows, skip = rows_round_the_grid(61, 900)
    more, _ = rows_round_the_grid(62, 700)
    last, _ = rows_round_the_grid(63, 500)
    T = ref.relative_pose(yaw_pose(0.2, 1.0, 0.5), yaw_pose(-0.1, 0.2, 0.1, 0.05))
    calls = [call(rows, 4, T, skip=skip, **extras_for(61, rows)), call(more, 0, v1=True), call(last, 2, T, label=extras_for(63, last)["label"]),
             call(more, 1, T, attr=extras_for(62, more)["attr"], attr_scale=255.0)]
    want = assert_equals_the_restatement(calls, 255.0, capacity=2048, **UNIT)
    assert (want[5] == 0).any() and (want[5] != 0).any() and (want[4] != 0).any()
    assert_equals_the_restatement(calls[::-1], 255.0, capacity=1024, pitch=4, attr_stride=4, **UNIT)      # integer sums: any order
    assert_same(by_key(launch(calls[::-1], capacity=1024, emit_scale=255.0, **UNIT)[2]), want)


def test_insert_ex_without_extras_is_insert(gpu):
    rows, skip = rows_round_the_grid(71, 2000)
    more, _ = rows_round_the_grid(72, 1100)
    T = ref.relative_pose(yaw_pose(0.2, 1.0, 0.5), yaw_pose(0.5, -0.7, 0.9))
    plain = [call(rows, 0, skip=skip), call(more, 3, T)]
    ex = launch(plain, capacity=1024, **UNIT)
    old = launch([dict(c, v1=True) for c in plain], capacity=1024, **UNIT)
    assert ex[0] == old[0] == [0] * 5 and ex[3] and old[3]
    assert_same(by_key(ex[2]), by_key(old[2]))
    assert not ex[2][4].any() and not ex[2][5].any()               # intensity 0 and label 0
    # ... and is what v1's own emit gives: the very launcher of the v1 tests
    st, n, out, clean, _ = launch_v1([(rows, EYE, 0, skip), (more, T, 3)], capacity=1024, **UNIT)
    order = np.argsort(out[0], kind="stable")
    assert st == [0] * 5 and clean and n == ex[1]
    assert_same(by_key(ex[2])[:4], tuple(o[order] for o in out))
    # words 6 and 7 of every slot are still the zeros the clear wrote
    assert not ex[4].reshape(-1, 8)[:, 6:].any() and not old[4].reshape(-1, 8)[:, 6:].any()


def test_emit_ex_with_less_room_than_rows_and_with_either_output_left_out(gpu):
    rows, _ = rows_round_the_grid(31, 1500)
    c = call(rows, 6, **extras_for(31, rows))
    want = ref2.accumulate([rule_of(c)], 255.0, **UNIT)
    for room in (0, 1, 50, len(want[0]) - 1):
        statuses, n, out, clean, _ = launch([c], capacity=1024, max_rows=room, emit_scale=255.0, **UNIT)
        assert statuses == [0, 0, 0, 0] and clean                   # (clean: nothing past ``room`` rows, in any output)
        assert n == len(want[0]) > room and len(out[0]) == room and len(set(out[0].tolist())) == room
        where = np.searchsorted(want[0], out[0])
        assert_same(out, tuple(w[where] for w in want))
    for wanted in ((True, False), (False, True), (False, False)):
        statuses, n, out, clean, _ = launch([c], capacity=1024, want=wanted, emit_scale=255.0, **UNIT)
        assert statuses == [0, 0, 0, 0] and clean and n == len(want[0])        # (clean: the output left out kept every fill byte)
        got = by_key(out)
        assert_same(got[:4], want[:4])
        assert len(out[4]) == (n if wanted[0] else 0) and len(out[5]) == (n if wanted[1] else 0)
        if wanted[0]:
            assert np.array_equal(bits(got[4]), bits(want[4]))
        if wanted[1]:
            assert np.array_equal(got[5], want[5])
    # a bad scale beside a NULL intensity pointer is not looked at
    statuses, n, out, clean, _ = launch([c], capacity=1024, want=(False, True), emit_scale=0.0, **UNIT)
    assert statuses == [0, 0, 0, 0] and clean and np.array_equal(by_key(out)[5], want[5])


def test_refusals_write_nothing(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.accumulate import Accumulator, AccumParams
    lib, bad = _lib.load(), _lib.ERR_INVALID_ARGUMENT
    rows, skip = rows_round_the_grid(41, 300)
    c = call(rows, 1, skip=skip, **extras_for(41, rows))

    def untouched(res):
        st, n, out, clean, tw = res
        slots = tw.reshape(-1, 8)
        return clean and bool((slots[:, 0] == 0xFFFFFFFF).all()) and not slots[:, 1:5].any() and not slots[:, 6:].any()

    nan, inf = float("nan"), float("inf")
    for override in (dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(stride=0), dict(stride=-4), dict(motion_min2=-1e-9),
                     dict(motion_min2=nan), dict(motion_min2=inf), dict(motion=2), dict(attr=6), dict(label=1)):
        res = launch([c], override=override, **UNIT)               # (motion, attr, label: an address that is no multiple of 4)
        assert res[0] == [0, bad, 0, 0] and res[1] == 0 and untouched(res), override
    # the pointers, misaligned for real
    stream = _lib.stream_handle()
    table = torch.full((8 * 17 + 4,), WORD, dtype=torch.int32, device=gpu)
    d_rows = torch.from_numpy(np.concatenate([rows, rows[:, :1]], axis=1)).to(gpu)
    d_motion, d_label = torch.zeros((300, 3), device=gpu), torch.ones(300, dtype=torch.int32, device=gpu)
    out = torch.full((96,), WORD, dtype=torch.int32, device=gpu)
    T = EYE.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pp, tp, op, rp = ctypes.addressof(p := AccumParams(**UNIT)), table.data_ptr(), out.data_ptr(), d_rows.data_ptr()
    ok_args = lambda: [300, rp, 4, None, T, 0, pp, tp, 16, d_motion.data_ptr(), 0.0, rp + 12, 4, 1.0, d_label.data_ptr(), stream]      # noqa: E731
    for at, off in ((9, 2), (11, 1), (14, 2), (7, 8), (1, 2)):    # motion, attr, label, table, rows
        args = ok_args()
        args[at] += off
        assert lib.himo_accum_insert_ex(*args) == bad, at
    for at, value in ((0, -1), (2, 5), (5, 256), (5, -1), (8, 24), (6, None), (4, None), (7, None), (1, None), (12, 0), (13, 0.0), (13, nan), (10, -1.0)):
        args = ok_args()
        args[at] = value
        assert lib.himo_accum_insert_ex(*args) == bad, (at, value)
    args = ok_args()
    args[0] = 1 << 31
    assert lib.himo_accum_insert_ex(*args) == _lib.ERR_UNSUPPORTED
    args[0], args[1] = 0, None
    assert lib.himo_accum_insert_ex(*args) == 0                    # n == 0: OK, no launch
    emit = lambda **kw: lib.himo_accum_emit_ex(*[kw.get(k, v) for k, v in dict(t=tp, cap=16, p=pp, room=4, n=op, keys=op + 64, xyz=op + 128, lag=op + 192,      # noqa: E731
                                                                                    count=op + 224, scale=1.0, inten=op + 256, label=op + 320, s=stream).items()])
    for kw in (dict(scale=0.0), dict(scale=-2.0), dict(scale=nan), dict(scale=inf), dict(inten=op + 258), dict(label=op + 321), dict(t=None), dict(room=-1),
               dict(n=None), dict(keys=None), dict(lag=None), dict(n=op + 2), dict(xyz=op + 130), dict(cap=24), dict(p=None), dict(t=tp + 8)):
        assert emit(**kw) == bad, kw
    d_flow, d_out = torch.zeros((300, 3), device=gpu), torch.full((904,), 7.25, device=gpu)
    motion = lambda **kw: lib.himo_accum_motion(*[kw.get(k, v) for k, v in dict(n=300, pts=rp, pitch=4, flow=d_flow.data_ptr(), E=T,      # noqa: E731
                                                                                 out=d_out.data_ptr() + 8, s=stream).items()])
    for kw in (dict(n=-1), dict(pitch=2), dict(pitch=5), dict(pts=None), dict(flow=None), dict(E=None), dict(out=None), dict(pts=rp + 2),
               dict(flow=d_flow.data_ptr() + 1), dict(out=d_out.data_ptr() + 6)):
        assert motion(**kw) == bad, kw
    assert motion(n=1 << 31) == _lib.ERR_UNSUPPORTED and motion(n=0, pts=None) == 0
    assert lib.himo_accum_status(stream) == 0
    torch.cuda.synchronize()
    assert (table == WORD).all().item() and (out == WORD).all().item() and (d_out == 7.25).all().item()
    # the Python entry points refuse before they launch
    acc = Accumulator(gpu, AccumParams(**UNIT), 1024)
    d3 = d_rows[:, :3].contiguous()
    for kw in (dict(motion=d_motion[:5]), dict(motion=d_motion.double()), dict(motion=d_motion, motion_min=-1.0), dict(motion=d_motion, motion_min=nan),
               dict(intensity=d_rows[:5, 3]), dict(intensity=d_rows[:, 3].double()), dict(intensity=d_rows[:, 3], intensity_scale=0.0),
               dict(intensity=d_rows[:, 3], intensity_scale=inf), dict(label=d_label[:7]), dict(label=d_label.long())):
        with pytest.raises(ValueError):
            acc.add(d3, EYE, 0, **kw)
    acc.add(d3, EYE, 0, intensity=d_rows[:, 3], intensity_scale=2.0)
    with pytest.raises(ValueError, match="since the last clear"):
        acc.add(d3, EYE, 1, intensity=d_rows[:, 3], intensity_scale=4.0)
    acc.clear()
    assert acc.rows == 0 and acc.result_ex()[4].numel() == 0


def test_colliding_and_wrapping_probe_chains_with_attributes(gpu):
    every = [(ix, iy, iz) for iz in range(4) for iy in range(8) for ix in range(8)]
    late = [v for v in every if ac_hash(key(*v), 64) >= 60]        # more keys than the slots they hash to have before the table's end
    rest = [v for v in every if ac_hash(key(*v), 64) < 60]
    voxels = (late + rest)[:40]
    rng = np.random.default_rng(4)
    rows = (np.array(voxels, np.float64)[rng.integers(0, 40, 900)] + rng.uniform(0, 1, (900, 3))).astype(f32)
    rows[:40] = (np.array(voxels, np.float64) + 0.5).astype(f32)
    ex = extras_for(4, rows)
    c = call(rows, 1, attr=ex["attr"], attr_scale=255.0, label=ex["label"])
    want = assert_equals_the_restatement([c], 255.0, capacity=64, attr_stride=4, **FAR_EGO)
    assert len(want[0]) == 40
    _, _, _, _, tw = launch([c], capacity=64, emit_scale=255.0, **FAR_EGO)
    slots = tw.reshape(65, 8)
    held = {int(k): i for i, k in enumerate(slots[:64, 0]) if k != 0xFFFFFFFF}
    assert sorted(held) == want[0].tolist() and sum(i < ac_hash(k, 64) for k, i in held.items()) >= 1          # a chain wrapped round
    assert int(slots[:64, 6].sum()) == int(ref2.quantise_attr(ex["attr"], 255.0).sum())                        # word 6 is Sa
    # keys that collide under the hash: 24 voxels of one bucket
    grid = dict(FAR_EGO, nx=64, ny=64, nz=4)
    buckets = {}
    for iz in range(4):
        for iy in range(64):
            for ix in range(64):
                buckets.setdefault(ac_hash(key(ix, iy, iz), 64), []).append((ix, iy, iz))
    worst = max(buckets.values(), key=len)[:24]
    rows = (np.array(worst, np.float64)[rng.integers(0, 24, 600)] + rng.uniform(0, 1, (600, 3))).astype(f32)
    rows[:24] = (np.array(worst, np.float64) + 0.25).astype(f32)
    ex = extras_for(6, rows)
    want = assert_equals_the_restatement([call(rows, 9, attr=ex["attr"], attr_scale=255.0, label=ex["label"])], 255.0, capacity=64, pitch=4, attr_stride=4,
                                         **grid)
    assert len(want[0]) == 24
    # a full table is still a reported refusal, with the guards standing
    from himo_amd import _lib
    voxels = [(ix, iy, 0) for iy in range(3) for ix in range(8)][:17]
    rows = (np.array(voxels, np.float64) + 0.5).astype(f32)
    statuses, n, out, clean, _ = launch([call(rows, 0, attr=np.full(17, 9.0, f32), label=np.arange(1, 18))], capacity=16, **FAR_EGO)
    assert statuses == [0, 0, _lib.ERR_INVALID_ARGUMENT, 0] and clean and n == 16 and set(out[4].tolist()) == {9.0}


def test_the_motion_of_a_stored_flow(gpu):
    from himo_amd import accumulate as acc
    rng = np.random.default_rng(8)
    pose0, pose1 = yaw_pose(0.30, 4.0, -2.0, 0.1), yaw_pose(0.33, 4.9, -1.7, 0.12)
    for n, cols in ((0, 4), (1, 3), (257, 4), (3001, 3), (3000, 5)):
        pc0 = rng.uniform(-60.0, 60.0, (n, cols)).astype(f32)
        flow = rng.uniform(-3.0, 3.0, (n, 3)).astype(f32)
        got = acc.flow_motion(pc0, flow, pose0, pose1)
        assert got.is_cuda and got.shape == (n, 3) and np.array_equal(bits(got.cpu().numpy()), bits(ref2.flow_motion(pc0, flow, pose0, pose1)))
    with pytest.raises(ValueError):
        acc.flow_motion(pc0, flow[:5], pose0, pose1)


def test_result_ex_and_accumulate_target_on_a_toy_scene(gpu):
    import torch
    from himo_amd import accumulate as acc
    sweeps, poses, skips = toy_scene()
    rng = np.random.default_rng(5)
    motions = [rng.uniform(-1.5, 1.5, (len(s), 3)).astype(f32) * (rng.random((len(s), 1)) < 0.3) for s in sweeps]
    motions[1][::50, 1] = np.nan
    labels = [rng.integers(0, 25, len(s)).astype(np.int32) for s in sweeps]
    xyz = [s[:, :3] for s in sweeps]
    inten = [s[:, 3] for s in sweeps]
    for t, window, sk, mo in ((3, 10, None, motions), (3, 2, skips, None), (0, 10, None, motions), (2, 0, skips, motions)):
        got = acc.accumulate_target(sweeps, poses, t, window, skips=sk, motions=mo, intensities=inten, labels=labels, motion_min=0.05, intensity_scale=255.0)
        want = ref2.accumulate_target(xyz, poses, t, window, skips=sk, motions=mo, intensities=inten, labels=labels, motion_min=0.05, intensity_scale=255.0)
        assert len(got) == 6 and all(g.is_cuda for g in got) and str(got[4].dtype) == "torch.float32" and str(got[5].dtype) == "torch.int32"
        host = [g.cpu().numpy() for g in got]
        assert_same((host[3], host[0], host[1], host[2], host[4], host[5]), want)
        assert 0.0 < host[4].mean() < 1.0 and len(set(host[5].tolist())) == 25
    # motions alone: still the 4-tuple; nothing asked: v1, call for call
    got = acc.accumulate_target(sweeps, poses, 3, 10, motions=motions, motion_min=0.05)
    want = ref2.accumulate_target(xyz, poses, 3, 10, motions=motions, motion_min=0.05)
    assert len(got) == 4 and np.array_equal(got[3].cpu().numpy(), want[0]) and np.array_equal(bits(got[0].cpu().numpy()), bits(want[1]))
    plain = acc.accumulate_target(sweeps, poses, 3, 10)
    assert not np.array_equal(plain[3].cpu().numpy(), want[0])
    # the class: a strided view of the rows as the intensity, read in place; result() after v2 inserts is v1's four columns
    table = acc.Accumulator(gpu, None, acc.capacity_for(3000))
    d = torch.from_numpy(sweeps[0]).to(gpu)
    table.add(d, np.eye(4), 0, intensity=d[:, 3], intensity_scale=255.0, label=torch.from_numpy(labels[0]).to(gpu))
    want = ref2.accumulate([dict(rows=xyz[0], T=np.eye(4), lag=0, attr=inten[0], attr_scale=255.0, label=labels[0])], 255.0)
    six, four = [g.cpu().numpy() for g in table.result_ex()], [g.cpu().numpy() for g in table.result()]
    assert_same((six[3], six[0], six[1], six[2], six[4], six[5]), want)
    assert_same((four[3], four[0], four[1], four[2]), want[:4])


def test_a_translating_body_lands_on_the_targets_own_rows(gpu):
    from himo_amd import accumulate as acc
    from himo_amd.accumulate import AccumParams
    sweeps, poses, motions, grid = translating_body()
    p = AccumParams(**grid)
    alone = [g.cpu().numpy() for g in acc.accumulate_target(sweeps, poses, 4, 0, params=p)]
    moved = [g.cpu().numpy() for g in acc.accumulate_target(sweeps, poses, 4, 4, params=p, motions=motions)]
    still = [g.cpu().numpy() for g in acc.accumulate_target(sweeps, poses, 4, 4, params=p)]
    assert len(alone[3]) == 8 and np.array_equal(moved[3], alone[3]) and moved[2].tolist() == [5] * 8 and not moved[1].any()
    assert np.array_equal(bits(moved[0]), bits(alone[0]))
    assert len(still[3]) == 40 and still[2].tolist() == [1] * 40
    want = ref2.accumulate_target(sweeps, poses, 4, 4, motions=motions, **grid)
    assert_same((moved[3], moved[0], moved[1], moved[2]), want[:4])
    assert np.array_equal(still[3], ref2.accumulate_target(sweeps, poses, 4, 4, **grid)[0])


# ---- the program -------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(gpu, tmp_path):
    import torch
    from himo_amd import accumulate as acc
    from himo_amd import view
    from himo_amd.compdis import CompDisEngine
    from himo_amd.dataset import HDF5Dataset
    from himo_amd.synthetic import make_scene, write_h5_scenes
    root = tmp_path / "scenes"
    root.mkdir()
    scenes = [make_scene(60 + s, 5, n_points=2000, scene_id=f"ac{s}", cloud="rings") for s in range(2)]
    write_h5_scenes(root, scenes)

    def compensated(fr):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)                 # noqa: E731
        return CompDisEngine().run_frame(up(fr["pc0"]), up(fr["flow"]), up(fr["lidar_dt"]), fr["pose0"], fr["pose1"], refined=True)[1].cpu().numpy()

    def datasets(out_dir, extra=()):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ds = HDF5Dataset(out_dir, fields=("pc0", "pose0", "lidar_dt", "gm0", "acc_count") + tuple(extra), need_next=False)
        try:
            assert len(ds) == 8
            return {(d["scene_id"], d["timestamp"]): d for d in (ds[i] for i in range(len(ds)))}
        finally:
            ds.close()

    v2, bins = tmp_path / "v2", tmp_path / "bins"
    done = acc.main(str(root), str(v2), res_name="flow", window=3, advect=True, motion_key="flow", intensity=True, intensity_scale=255.0,
                    carry_label="flow_instance_id", bin_dir=str(bins))
    assert sorted(done) == ["ac0", "ac1"]
    files = datasets(v2, ("acc_intensity", "acc_label"))
    moved_somewhere = 0
    for frames in scenes:
        comp = [compensated(fr) for fr in frames[:4]]
        poses = [fr["pose0"] for fr in frames[:4]]
        motions = [ref2.flow_motion(fr["pc0"], fr["flow"], fr["pose0"], fr["pose1"]) for fr in frames[:4]]
        inten = [fr["pc0"][:, 3] for fr in frames[:4]]
        labels = [fr["flow_instance_id"].astype(np.int32) for fr in frames[:4]]
        for t in range(4):
            keys, xyz, lag, count, intensity, label = ref2.accumulate_target(comp, poses, t, 3, motions=motions, intensities=inten, labels=labels,
                                                                             motion_min=0.05, intensity_scale=255.0)
            d = files[(frames[t]["scene_id"], frames[t]["timestamp"])]
            lidar = d["pc0"]
            assert lidar.dtype == np.float32 and lidar.shape == (len(keys), 4) and np.array_equal(bits(lidar[:, :3].copy()), bits(xyz))
            assert np.array_equal(lidar[:, 3], lag.astype(f32) * f32(0.1)) and np.array_equal(d["acc_count"], count)
            assert d["acc_intensity"].dtype == np.float32 and np.array_equal(bits(d["acc_intensity"]), bits(intensity))
            assert d["acc_label"].dtype == np.int32 and np.array_equal(d["acc_label"], label)
            assert not d["lidar_dt"].any() and not d["gm0"].any() and d["pose0"].tobytes() == np.asarray(poses[t]).tobytes()
            # the .bin file: the columns of the scene file, little-endian float32 [M][5]
            raw = (bins / frames[t]["scene_id"] / f"{frames[t]['timestamp']}.bin").read_bytes()
            want = np.concatenate([lidar[:, :3], d["acc_intensity"][:, None], lidar[:, 3:4]], axis=1).astype("<f4")
            assert raw == want.tobytes() and len(raw) == 20 * len(keys)
            still = ref2.accumulate_target(comp, poses, t, 3)
            moved_somewhere += t > 0 and not np.array_equal(still[0], keys)
            assert (label != 0).any() and 0.2 < intensity.mean() < 0.8
    assert moved_somewhere == 6                                    # every target with a past sweep: the instances' rows went elsewhere
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # (the last target of a scene has no successor in O)
        listing = view.main(str(v2), str(tmp_path / "png"), res_names="raw", index=1, color_by="label:acc_label")
    assert len(listing) == 1 and listing[0]["panels"] == ["raw"] and listing[0]["points"][0] > 2000 and listing[0]["pixels"][0] > 500
    assert (tmp_path / "png" / listing[0]["file"]).stat().st_size > 1000

    # no new flag: the bytes of every dataset are v1's, produced here through the unchanged v1 path (himo_accum_insert / himo_accum_emit
    # by way of Accumulator.add without extras and result())
    plain = tmp_path / "plain"
    acc.main(str(root), str(plain), res_name="flow", window=3)
    files = datasets(plain)
    for frames in scenes:
        comp = [torch.from_numpy(compensated(fr)).to(gpu) for fr in frames[:4]]
        poses = [np.asarray(fr["pose0"]) for fr in frames[:4]]
        for t in range(4):
            table = acc.Accumulator(gpu, None, acc.capacity_for(4 * 2000))
            inv_t = np.linalg.inv(poses[t].astype(np.float64))
            for k in acc.sources(t, 4, 3):
                table.add(comp[k], (inv_t @ poses[k].astype(np.float64)).astype(np.float32), t - k)
            xyz, lag, count, _ = [g.cpu().numpy() for g in table.result()]
            d = files[(frames[t]["scene_id"], frames[t]["timestamp"])]
            assert set(d) == {"scene_id", "timestamp", "pc0", "pose0", "lidar_dt", "gm0", "acc_count"}      # no acc_intensity, no acc_label
            lidar = np.concatenate([xyz, (lag.astype(f32) * f32(0.1))[:, None]], axis=1).astype(f32)
            assert d["pc0"].tobytes() == lidar.tobytes() and d["acc_count"].tobytes() == count.astype(np.int32).tobytes()
            assert d["lidar_dt"].tobytes() == np.zeros(len(xyz), f32).tobytes() and d["gm0"].tobytes() == np.zeros(len(xyz), bool).tobytes()
            assert d["pose0"].tobytes() == poses[t].tobytes()
            want = ref.accumulate_target([c.cpu().numpy() for c in comp], poses, t, 3)
            assert np.array_equal(bits(xyz), bits(want[1])) and np.array_equal(count, want[3])
    # what is missing is named
    with pytest.raises(KeyError, match="no_such_flow"):
        acc.main(str(root), str(tmp_path / "o1"), res_name="flow", advect=True, motion_key="no_such_flow")
    with pytest.raises(KeyError, match="himo_amd.raymap"):
        acc.main(str(root), str(tmp_path / "o2"), res_name="raw", carry_label="ray_label")
    with pytest.raises(ValueError, match="motion_key"):
        acc.main(str(root), str(tmp_path / "o3"), res_name="raw", advect=True)
