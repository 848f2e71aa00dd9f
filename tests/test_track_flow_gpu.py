"""Track flow on the GPU: ``himo_trackflow_plan`` and ``himo_trackflow_apply`` through ctypes on guarded buffers against the
pure-Python restatement of the rule (tests/trackflow_ref.py), fed the same tables, at the sizes and inputs where the kernels take another
path.  Plan outputs and flows match bit for bit (floats compared as their integer bit patterns, so that untouched NaN rows count); no case
is left out.  Then ``TrackFlow`` and the program end to end."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest

import trackflow_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64                                      # elements before and after every output, and 256 bytes around the workspace
FILL_I, FILL_F = 0x7A7A7A7A, 7.25
f32 = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = bits(got), bits(want)
    assert g.tobytes() == w.tobytes(), (what, np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:8])


class Guarded:
    """device outputs with guard elements on both sides: ``at(k)`` the address of output k, ``read()`` -> ({k: array}, intact)"""

    def __init__(self, gpu, sizes):
        import torch
        self.sizes = sizes
        self.buf = {k: torch.full((m + 2 * GUARD,), FILL_F if t.is_floating_point else FILL_I, dtype=t, device=gpu) for k, (m, t) in sizes.items()}

    def at(self, k):
        return self.buf[k].data_ptr() + GUARD * self.buf[k].element_size()

    def read(self):
        out, intact = {}, True
        for k, (m, t) in self.sizes.items():
            fill = FILL_F if t.is_floating_point else FILL_I
            intact = intact and bool((self.buf[k][:GUARD] == fill).all() and (self.buf[k][GUARD + m:] == fill).all())
            out[k] = self.buf[k][GUARD:GUARD + m].cpu().numpy()
        return out, intact


# ---- the plan (rules B-D) ---------------------------------------------------------------------------------------------------------------------
PLAN_NAMES = ("state", "m", "shift", "disp", "u")


def plan_tables(scenes):
    counts = [len(s.id) for sc in scenes for s in sc]
    sweep_off = np.concatenate([[0], np.cumsum([len(sc) for sc in scenes])]).astype(np.int64)
    det_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    id_off = np.concatenate([[0], np.cumsum([max([int(s.id.max()) + 1 for s in sc if len(s.id)] + [0]) for sc in scenes])]).astype(np.int64)
    flat = [s for sc in scenes for s in sc]
    cat = lambda k, tail, dt: np.ascontiguousarray(np.concatenate([np.asarray(s[k], dt).reshape((-1,) + tail) for s in flat])) if flat else np.zeros((0,) + tail, dt)      # noqa: E731
    return dict(boxes=cat(0, (12,), f32), id=cat(1, (), np.int32), w=cat(2, (3,), np.float64), U=cat(3, (9,), np.float64), sorted_id=cat(4, (), np.int32),
                sorted_row=cat(5, (), np.int32), sweep_off=sweep_off, det_off=det_off, id_off=id_off)


class RawPlan:
    """one call of ``himo_trackflow_plan`` on guarded buffers: ``status``, the five outputs as numpy arrays, ``intact``"""

    def __init__(self, gpu, scenes, **params):
        import torch
        from himo_amd import _lib
        from himo_amd.track_flow import TrackFlowParams
        lib, P = _lib.load(), _lib.ptr
        t = plan_tables(scenes)
        n, rows = len(scenes), len(t["id"])
        prm = TrackFlowParams(**params).c_struct()
        dev = {k: torch.from_numpy(v).to(gpu) for k, v in t.items()}
        g = Guarded(gpu, {"state": (rows, torch.int32), "m": (rows, torch.int32), "shift": (3 * rows, torch.float32), "disp": (3 * rows, torch.float32),
                          "u": (3 * rows, torch.float64)})
        host = [t[k].ctypes.data for k in ("sweep_off", "det_off", "id_off")]
        need = int(lib.himo_trackflow_workspace_bytes(n, *host))
        ws = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=gpu)
        with torch.cuda.device(gpu):
            self.status = lib.himo_trackflow_plan(n, host[0], P(dev["sweep_off"]), host[1], P(dev["det_off"]), host[2], P(dev["id_off"]), P(dev["id"]),
                                                  P(dev["w"]), P(dev["boxes"]), P(dev["U"]), ctypes.addressof(prm), *[g.at(k) for k in PLAN_NAMES],
                                                  ws.data_ptr() + 256, need, _lib.stream_handle())
        torch.cuda.synchronize()
        out, ok = g.read()
        self.need, self.intact = need, ok and bool((ws[:256] == 0x5A).all() and (ws[256 + need:] == 0x5A).all())
        self.state, self.m = out["state"], out["m"]
        self.shift, self.disp, self.u = out["shift"].reshape(-1, 3), out["disp"].reshape(-1, 3), out["u"].reshape(-1, 3)

    def outputs(self):
        return tuple(getattr(self, k) for k in PLAN_NAMES)


def plan_same(raw, want):
    assert raw.status == 0 and raw.intact
    for k, got, w in zip(PLAN_NAMES, raw.outputs(), want):
        same_bits(got, w, k)


def made_sweep(rng, ids, k, first=0, dirty=True):
    """the prepared tables of sweep k of a scene whose box rows carry the track ids ``ids`` (in that row order)"""
    F = len(ids)
    b = np.zeros((F, 12), f32)
    b[:, 7:9] = rng.uniform(-20, 20, (F, 2))
    b[:, 9] = rng.uniform(-0.5, 0.5, F)
    slow = rng.random(F) < 0.25
    b[slow, 7:10] = rng.uniform(-0.3, 0.3, (int(slow.sum()), 3))   # some static ones, some about the threshold of 0.5 m/s
    b[:, 10] = rng.permutation(4 * F + 5)[:F] + 1
    if dirty and F >= 8:
        b[3, 7], b[5, 9], b[6, 8] = np.nan, np.inf, -np.inf         # velocities that are not finite: not USABLE
        b[7, 10] = b[2, 10]                                         # a label id twice
    t = np.zeros((F, 6))
    t[:, 0] = ids
    return ref.prepare(b, t, ref.ego_pose(k), ref.ego_pose(first))


@functools.lru_cache(maxsize=None)
def plan_case():
    """three scenes (and an empty one) that cross every path of the plan: the window clipped at both scene ends, tracks with missed sweeps
    inside the window, a track of length min_len - 1 beside one of min_len, an id present in one sweep only, a sweep with 0 boxes and
    sweeps with 512, rows without a track, velocities that are not finite"""
    rng = np.random.default_rng(81)
    K, pool = 11, 40
    first = []
    for k in range(K):
        seen = [t for t in range(pool) if rng.random() < 0.8]       # every track misses sweeps here and there
        if k == 4:
            seen.append(100)                                        # an id present in sweep 4 only
        if k in (1, 2):
            seen.append(101)                                        # length 2 = min_len - 1
        if k in (1, 2, 4):
            seen.append(102)                                        # length 3 = min_len, with a missed sweep in between
        seen += [-1] * 6
        ids = np.array(seen)[rng.permutation(len(seen))]
        first.append(made_sweep(rng, ids if k != 6 else ids[:0], k))     # sweep 6 holds no box
    full = [made_sweep(rng, rng.permutation(512), k) for k in range(2)] + [made_sweep(rng, rng.permutation(512)[:300], 2)] + \
        [made_sweep(rng, np.arange(512), 3)]
    third = [made_sweep(rng, np.array([0, 1, 2, 0, -1, 1, 2, 5, 5, 3]), 0, dirty=False)]      # one sweep; ids twice in a sweep: the lowest row counts
    scenes = [first, [], full, third]
    cases = [dict(half=0), dict(half=2), dict(half=8), dict(half=1, min_len=1, motion_min=0.0, sensor_dt=0.05), dict(half=2, min_len=4)]
    return scenes, cases, [ref.plan(scenes, **kw) for kw in cases]


@pytest.mark.parametrize("case", range(5))
def test_plan_over_scenes_and_sweeps_of_every_shape_in_one_call(gpu, case):
    scenes, cases, wants = plan_case()
    want = wants[case]
    if case == 1:                                                   # the cases do what they are for
        t = plan_tables(scenes)
        lo = lambda n, k: int(t["det_off"][int(t["sweep_off"][n]) + k])      # noqa: E731
        state, m = want[0], want[1]
        assert {0, 1, 2} <= set(state.tolist()) and m.max() == 5 and 1 in m.tolist() and 2 in m.tolist()
        for k, tid in ((4, 100), (1, 101), (2, 101)):               # present once; one short of min_len
            r = lo(0, k) + int(np.flatnonzero(scenes[0][k].id == tid)[0])
            assert state[r] == 0 and m[r] == 0
        r = lo(0, 2) + int(np.flatnonzero(scenes[0][2].id == 102)[0])
        assert state[r] != 0 and m[r] == 3                          # sweeps 1, 2 and 4 of the window 0..4; sweep 3 missed
        assert (state[lo(2, 0):lo(2, 0) + 512] != 0).sum() > 500 and (state[lo(3, 0):] == 0).all()
    plan_same(RawPlan(gpu, scenes, **cases[case]), want)


def test_plan_scenes_alone_equal_the_batch_and_a_second_run_gives_the_same_bytes(gpu):
    scenes, cases, wants = plan_case()
    one, two = RawPlan(gpu, scenes, **cases[1]), RawPlan(gpu, scenes, **cases[1])
    for a, b in zip(one.outputs(), two.outputs()):
        assert bits(a).tobytes() == bits(b).tobytes()
    t = plan_tables(scenes)
    lo, hi = int(t["det_off"][int(t["sweep_off"][2])]), int(t["det_off"][int(t["sweep_off"][3])])
    alone = RawPlan(gpu, [scenes[2]], **cases[1])
    assert alone.status == 0 and alone.intact
    for got, w in zip(alone.outputs(), wants[1]):
        assert bits(got).tobytes() == bits(w[lo:hi]).tobytes()
    assert RawPlan(gpu, []).status == 0 and RawPlan(gpu, [[], []]).status == 0
    nothing = RawPlan(gpu, [[made_sweep(np.random.default_rng(1), np.zeros(0), 0)] * 3])      # sweeps without a box
    assert nothing.status == 0 and nothing.intact and nothing.state.shape == (0,)


def test_plan_refusals_leave_the_outputs_untouched(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.track_flow import TrackFlowParams, _CParams
    lib, P = _lib.load(), _lib.ptr
    rng = np.random.default_rng(82)
    scenes = [[made_sweep(rng, rng.permutation(12), k) for k in range(3)], [made_sweep(rng, rng.permutation(9), k) for k in range(2)]]
    t = plan_tables(scenes)
    n, rows = 2, len(t["id"])
    dev = {k: torch.from_numpy(v).to(gpu) for k, v in t.items()}
    outs = {"state": torch.full((rows,), 7, dtype=torch.int32, device=gpu), "m": torch.full((rows,), 7, dtype=torch.int32, device=gpu),
            "shift": torch.full((rows, 3), 7.0, dtype=torch.float32, device=gpu), "disp": torch.full((rows, 3), 7.0, dtype=torch.float32, device=gpu),
            "u": torch.full((rows, 3), 7.0, dtype=torch.float64, device=gpu)}
    prm = TrackFlowParams().c_struct()
    need = int(lib.himo_trackflow_workspace_bytes(n, t["sweep_off"].ctypes.data, t["det_off"].ctypes.data, t["id_off"].ctypes.data))
    assert need >= 4 * 21 and need % 256 == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=gpu)
    order = ("n", "h_so", "d_so", "h_do", "d_do", "h_io", "d_io", "id", "w", "boxes", "U", "prm", "state", "m", "shift", "disp", "u", "ws", "ws_bytes")

    def call(**kw):
        a = dict(n=n, h_so=t["sweep_off"].ctypes.data, d_so=P(dev["sweep_off"]), h_do=t["det_off"].ctypes.data, d_do=P(dev["det_off"]),
                 h_io=t["id_off"].ctypes.data, d_io=P(dev["id_off"]), id=P(dev["id"]), w=P(dev["w"]), boxes=P(dev["boxes"]), U=P(dev["U"]),
                 prm=ctypes.addressof(prm), ws=P(ws), ws_bytes=ws.numel(), **{k: P(v) for k, v in outs.items()})
        a.update(kw)
        return lib.himo_trackflow_plan(*[a[k] for k in order], _lib.stream_handle())
    late, falling, rows_late, rows_falling, ids_late, ids_falling, over = (t[k].copy() for k in ("sweep_off", "sweep_off", "det_off", "det_off", "id_off",
                                                                                                  "id_off", "det_off"))
    late[0], falling[1], rows_late[0], rows_falling[2], ids_late[0], ids_falling[1], over[1:] = 1, 6, 1, 0, 1, 50, t["det_off"][1:] + 513

    def params(**kw):
        c = TrackFlowParams().c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    bad = [params(sensor_dt=0.0), params(sensor_dt=-0.1), params(sensor_dt=math.nan), params(sensor_dt=math.inf), params(motion_min=-1e-9),
           params(motion_min=math.nan), params(motion_min=math.inf), params(half=-1), params(half=9), params(min_len=0), params(mode=2), params(mode=-1),
           params(reserved=1)]
    refused = [dict(n=-1), dict(prm=None), dict(h_so=None), dict(h_do=None), dict(h_io=None), dict(h_so=late.ctypes.data), dict(h_so=falling.ctypes.data),
               dict(h_do=rows_late.ctypes.data), dict(h_do=rows_falling.ctypes.data), dict(h_io=ids_late.ctypes.data), dict(h_io=ids_falling.ctypes.data),
               dict(d_so=None), dict(d_do=None), dict(d_io=None), dict(d_so=P(dev["sweep_off"]) + 4), dict(id=None), dict(w=None), dict(boxes=None),
               dict(U=None), dict(state=None), dict(m=None), dict(shift=None), dict(disp=None), dict(u=None), dict(w=P(dev["w"]) + 4),
               dict(u=P(outs["u"]) + 4), dict(state=P(outs["state"]) + 2), dict(shift=P(outs["shift"]) + 1)] + [dict(prm=ctypes.addressof(b)) for b in bad]
    for kw in refused:
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, kw
    assert call(h_do=over.ctypes.data) == _lib.ERR_UNSUPPORTED      # a sweep above the cap
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=P(ws) + 8)):
        assert call(**kw) == _lib.ERR_WORKSPACE, kw
    assert lib.himo_trackflow_workspace_bytes(n, late.ctypes.data, t["det_off"].ctypes.data, t["id_off"].ctypes.data) == 0
    assert lib.himo_trackflow_workspace_bytes(n, t["sweep_off"].ctypes.data, over.ctypes.data, t["id_off"].ctypes.data) == 0
    assert lib.himo_trackflow_workspace_bytes(n, t["sweep_off"].ctypes.data, t["det_off"].ctypes.data, ids_falling.ctypes.data) == 0
    assert lib.himo_trackflow_workspace_bytes(-1, None, None, None) == 0 and lib.himo_trackflow_workspace_bytes(0, None, None, None) == 256
    assert ctypes.sizeof(_CParams) == lib.himo_abi_sizeof(b"himo_trackflow_params")
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs.values()) and bool((ws == 0x5A).all())
    # nothing to do: HIMO_OK, nothing written; then the same call, admitted, writes
    assert call(n=0, h_so=None, h_do=None, h_io=None) == _lib.OK
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs.values())
    assert call() == _lib.OK
    torch.cuda.synchronize()
    for k, want in zip(PLAN_NAMES, ref.plan(scenes)):
        same_bits(outs[k].cpu().numpy().reshape(want.shape), want, k)


# ---- the points (rule E) ------------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 257, 1025)           # points per sweep of the launch: the wave edges, a block of 1024 rows plus one; 1475 rows = a whole tile
                                                # that crosses all seven sweeps and a partial one
BOXES = (3, 3, 5, 0, 4, 6, 512)                 # boxes per sweep: none, and the cap


def point_sweep(rng, N, F, k, pitch):
    """one sweep of N points and F boxes: (prepared tables, its plan, pc0 [N, pitch], flow, labels, E)"""
    # the sweep is the middle one of three with the same boxes at other velocities, so that the smoothed velocity is not the box's own
    vel = rng.uniform(-20, 20, (3, F, 3))
    t = np.zeros((F, 6))
    t[:, 0] = np.arange(F)
    if F >= 3:
        still = np.concatenate([[False, True, False], rng.random(F - 3) < 0.15])
        vel[:, still] = rng.uniform(-0.2, 0.2, (3, int(still.sum()), 3))      # STATIC: below 0.5 m/s in every sweep
        t[2, 0] = -1                                                # NONE
        t[F // 2 + 1:, 0] = np.where(rng.random(F - F // 2 - 1) < 0.2, -1, t[F // 2 + 1:, 0])
    three = []
    for j in range(3):
        b = np.zeros((F, 12), f32)
        b[:, 7:10] = vel[j]
        b[:, 10] = np.arange(F) if j != 1 else rng.permutation(6 * F + 7)[:F] + 2
        three.append(ref.prepare(b, t, ref.ego_pose(k + j - 1, turn=0.03), ref.ego_pose(k - 1, turn=0.03)))
    pose0, pose1 = ref.ego_pose(k, turn=0.03), ref.ego_pose(k + 1, turn=0.03)
    s, b = three[1], three[1].boxes
    pl = ref.plan_scene(three, half=1, min_len=3)[1]
    pc0 = rng.uniform(-50, 50, (N, pitch)).astype(f32)
    flow = rng.normal(0, 1, (N, 3)).astype(f32)
    ids = b[:, 10].astype(np.int64)
    if F:                                                           # labels: the smallest and the largest id, every box, 0, negative, absent
        choice = np.concatenate([ids, [ids.min(), ids.max(), ids[0], ids[1 % F], 0, 0, -int(ids[0]), 1, int(ids.max()) + 1, 2 ** 31 - 1, -2 ** 31]])
    else:
        choice = np.array([0, 5, -5, 77])
    label = rng.choice(choice, N).astype(np.int32)
    if N >= 60:
        label[:6] = [ids.min(), ids.max(), 0, -int(ids[0]), int(ids.max()) + 1, ids[0]] if F else 0
        rows = np.flatnonzero(label == ids[0])[:4] if F else []     # rows of a MOVING box whose flow is not finite keep their bytes
        for j, r in enumerate(rows):
            flow.view(np.uint32)[r, j % 3] = (0x7FC12345, 0x7F800000, 0xFF800000, 0xFFC00001)[j]
        flow.view(np.uint32)[N - 1, 2] = 0x7FA00001                 # and one anywhere
    return s, pl, pc0, flow, label, ref.ego_transform(pose0, pose1)


@functools.lru_cache(maxsize=None)
def point_case(pitch):
    rng = np.random.default_rng(90 + pitch)
    sweeps = [point_sweep(rng, N, F, k, pitch) for k, (N, F) in enumerate(zip(SIZES, BOXES))]
    wants = {}
    for mode in (0, 1):
        outs = [ref.apply_sweep(pc0, flow, label, E, s, pl, mode) for s, pl, pc0, flow, label, E in sweeps]
        wants[mode] = (np.concatenate([o[0] for o in outs]), np.array([[o[1], o[2]] for o in outs], np.int32))
    return sweeps, wants


class RawApply:
    """one call of ``himo_trackflow_apply`` on guarded buffers over ``sweeps`` (``point_sweep``'s tuples): ``status``, ``out``, ``counts``,
    ``intact``.  ``skew``: the flow and the output start 4 bytes off a 16-byte boundary (the narrow path)."""

    def __init__(self, gpu, sweeps, mode=0, skew=False, lead=0, **over):
        import torch
        from himo_amd import _lib
        from himo_amd.track_flow import TrackFlowParams
        lib, P = _lib.load(), _lib.ptr
        ns = len(sweeps)
        pitch = sweeps[0][2].shape[1]
        h_pt = np.concatenate([[0], np.cumsum([len(s[2]) for s in sweeps])]).astype(np.int64)
        h_box = (np.concatenate([[0], np.cumsum([len(s[0].id) for s in sweeps])]) + lead).astype(np.int64)      # ``lead`` plan rows of other sweeps first
        rows, nb = int(h_pt[-1]), int(h_box[-1])
        cat = lambda parts, tail, dt: np.ascontiguousarray(np.concatenate([np.asarray(p, dt).reshape((-1,) + tail) for p in parts]))      # noqa: E731
        pad = lambda a: np.concatenate([np.zeros((lead,) + a.shape[1:], a.dtype), a])      # noqa: E731
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)      # noqa: E731
        pc0, label = up(cat([s[2] for s in sweeps], (pitch,), f32)), up(cat([s[4] for s in sweeps], (), np.int32))
        shove = np.zeros(1 if skew else 0, f32)                     # one float in front: a start 4 bytes off a 16-byte boundary
        flow = up(np.concatenate([shove, cat([s[3] for s in sweeps], (3,), f32).reshape(-1), np.zeros(4, f32)]))
        E = up(cat([s[5] for s in sweeps], (12,), f32))
        sid, srow = up(pad(cat([s[0].sorted_id for s in sweeps], (), np.int32))), up(pad(cat([s[0].sorted_row for s in sweeps], (), np.int32)))
        state = up(pad(cat([s[1].state for s in sweeps], (), np.int32)))
        shift, disp = up(pad(cat([s[1].shift for s in sweeps], (3,), f32))), up(pad(cat([s[1].disp for s in sweeps], (3,), f32)))
        d_pt, d_box = up(h_pt), up(h_box)
        g = Guarded(gpu, {"out": (3 * rows, torch.float32), "counts": (2 * ns, torch.int32)})
        prm = TrackFlowParams(mode=mode).c_struct()
        assert g.at("out") % 16 == 0 and flow.data_ptr() % 16 == 0   # (the wide path needs both; the skewed flow alone takes the narrow one)
        a = dict(ns=ns, h_pt=h_pt.ctypes.data, d_pt=P(d_pt), pc0=P(pc0), pitch=pitch, flow=flow.data_ptr() + (4 if skew else 0), label=P(label), E=P(E),
                 h_box=h_box.ctypes.data, d_box=P(d_box), total=nb, sid=P(sid), srow=P(srow), state=P(state), shift=P(shift), disp=P(disp),
                 prm=ctypes.addressof(prm), out=g.at("out"), counts=g.at("counts"))
        a.update({k: v(a[k]) if callable(v) else v for k, v in over.items()})      # (a callable: the admitted address, moved)
        with torch.cuda.device(gpu):
            self.status = lib.himo_trackflow_apply(*[a[k] for k in ("ns", "h_pt", "d_pt", "pc0", "pitch", "flow", "label", "E", "h_box", "d_box", "total",
                                                                    "sid", "srow", "state", "shift", "disp", "prm", "out", "counts")], _lib.stream_handle())
        torch.cuda.synchronize()
        out, self.intact = g.read()
        self.out, self.counts = out["out"].reshape(-1, 3), out["counts"].reshape(-1, 2)
        self.untouched = bool((bits(self.out) == bits(np.array([FILL_F], f32))[0]).all() and (self.counts == FILL_I).all())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pitch", [3, 4, 5])
def test_points_of_seven_sweeps_in_one_launch(gpu, pitch, mode):
    sweeps, wants = point_case(pitch)
    want_out, want_counts = wants[mode]
    if pitch == 4:                                                  # the cases do what they are for
        assert (want_counts[[0, 3]] == 0).all() and (want_counts[[2, 4, 5, 6]] > 0).all() and want_counts[1].sum() <= 1
        changed = (bits(want_out) != bits(np.concatenate([s[3] for s in sweeps]))).any(axis=1)
        assert 100 < changed.sum() < 1475 and not changed[~np.isfinite(want_out).all(axis=1)].any()
    raw = RawApply(gpu, sweeps, mode=mode)
    assert raw.status == 0 and raw.intact
    same_bits(raw.out, want_out, "out")
    assert raw.counts.tolist() == want_counts.tolist()
    skewed = RawApply(gpu, sweeps, mode=mode, skew=True, lead=37)   # the narrow path, and plan rows that do not start at 0
    assert skewed.status == 0 and skewed.intact
    same_bits(skewed.out, want_out, "out, skewed")
    assert skewed.counts.tolist() == want_counts.tolist()


def test_static_boxes_get_the_ego_motion_flow_in_both_modes(gpu):
    import torch
    from himo_amd.seflow.ssl_label import _moved
    sweeps, wants = point_case(4)
    for k in (5, 6):
        s, pl, pc0, flow, label, E = sweeps[k]
        d_pc0 = torch.from_numpy(pc0).to(gpu)
        moved = _moved(d_pc0, np.concatenate([E, [0, 0, 0, 1]]).reshape(4, 4))      # himo_rigid_transform
        ego = (moved - d_pc0[:, :3]).cpu().numpy()
        pos = np.clip(np.searchsorted(s.sorted_id, label), 0, len(s.sorted_id) - 1)
        static = (label > 0) & (s.sorted_id[pos] == label) & (pl.state[s.sorted_row[pos]] == ref.STATIC) & np.isfinite(flow).all(axis=1)
        assert static.sum() >= 5
        lo = sum(SIZES[:k])
        for mode in (0, 1):
            assert bits(wants[mode][0][lo:lo + len(pc0)][static]).tobytes() == bits(ego[static]).tobytes()
    one = RawApply(gpu, [sweeps[5]], mode=1)                        # a sweep alone equals its rows of the launch
    assert one.status == 0 and one.intact and bits(one.out).tobytes() == bits(wants[1][0][sum(SIZES[:5]):sum(SIZES[:6])]).tobytes()


def test_points_a_second_run_gives_the_same_bytes_and_nothing_to_do(gpu):
    sweeps, _ = point_case(3)
    one, two = RawApply(gpu, sweeps, mode=1), RawApply(gpu, sweeps, mode=1)
    assert bits(one.out).tobytes() == bits(two.out).tobytes() and one.counts.tolist() == two.counts.tolist()
    empty = RawApply(gpu, [sweeps[0], sweeps[0]])                   # sweeps without a point: the counts are written, nothing else
    assert empty.status == 0 and empty.intact and empty.counts.tolist() == [[0, 0], [0, 0]]
    none = RawApply(gpu, sweeps[:2], ns=0)
    assert none.status == 0 and none.intact and none.untouched


def test_point_refusals_leave_the_outputs_untouched(gpu):
    from himo_amd import _lib
    from himo_amd.track_flow import TrackFlowParams
    sweeps, _ = point_case(4)
    sweeps = sweeps[2:6]
    h_pt = np.concatenate([[0], np.cumsum([len(s[2]) for s in sweeps])]).astype(np.int64)
    h_box = np.concatenate([[0], np.cumsum([len(s[0].id) for s in sweeps])]).astype(np.int64)
    late, falling, below, beyond, falling_b, over = h_pt.copy(), h_pt.copy(), h_box.copy(), h_box.copy(), h_box.copy(), h_box.copy()
    late[0], falling[2], below[0], beyond[-1], falling_b[2], over[1:] = 1, 0, -1, h_box[-1] + 1, 0, h_box[1:] + 513

    def params(**kw):
        c = TrackFlowParams().c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    bad = [params(mode=2), params(half=9), params(min_len=0), params(sensor_dt=math.nan), params(motion_min=-1.0), params(reserved=3)]
    refused = [dict(ns=-1), dict(pitch=2), dict(pitch=0), dict(total=-1), dict(prm=None), dict(h_pt=None), dict(h_box=None), dict(h_pt=late.ctypes.data),
               dict(h_pt=falling.ctypes.data), dict(h_box=below.ctypes.data), dict(h_box=beyond.ctypes.data), dict(h_box=falling_b.ctypes.data),
               dict(d_pt=None), dict(d_box=None), dict(E=None), dict(counts=None), dict(pc0=None), dict(flow=None), dict(label=None), dict(out=None),
               dict(sid=None), dict(srow=None), dict(state=None), dict(shift=None), dict(disp=None)] + [dict(prm=ctypes.addressof(b)) for b in bad]
    for kw in refused:
        r = RawApply(gpu, sweeps, **kw)
        assert r.status == _lib.ERR_INVALID_ARGUMENT and r.intact and r.untouched, kw
    r = RawApply(gpu, sweeps, h_box=over.ctypes.data, total=int(over[-1]))
    assert r.status == _lib.ERR_UNSUPPORTED and r.intact and r.untouched      # a sweep above the cap
    for key, off in (("flow", 2), ("out", 2), ("label", 2), ("pc0", 1), ("sid", 2), ("srow", 1), ("state", 2), ("shift", 2), ("disp", 3), ("counts", 2),
                     ("E", 2), ("d_pt", 4), ("d_box", 4)):
        r = RawApply(gpu, sweeps, **{key: lambda p, off=off: p + off})      # misaligned
        assert r.status == _lib.ERR_INVALID_ARGUMENT and r.intact and r.untouched, key
    ok = RawApply(gpu, sweeps)
    assert ok.status == 0 and ok.intact and not ok.untouched


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------
def test_the_engine_equals_the_raw_calls(gpu):
    import torch
    from himo_amd.track_flow import TrackFlow
    scenes, cases, wants = plan_case()
    eng = TrackFlow(gpu, **cases[1])
    res = eng.plan(scenes)
    assert len(res) == 4 and res.sweeps(0) == 11 and res.sweeps(1) == 0
    for k, want in zip(PLAN_NAMES, wants[1]):
        same_bits(getattr(res, k), want, k)
    lo, hi = res.rows(2, 1)
    assert hi - lo == 512 and bits(res.sweep(2, 1)[4]).tobytes() == bits(wants[1][4][lo:hi]).tobytes()
    empty = eng.plan([])
    assert len(empty) == 0 and empty.state.shape == (0,) and empty.u.shape == (0, 3)
    # points for sweeps that are no neighbours in the plan, in an order of their own, on another stream: three runs of plan rows
    rng = np.random.default_rng(83)
    picks = [(0, 7), (0, 8), (2, 2), (0, 2)]
    data = []
    for n, k in picks:
        s = scenes[n][k]
        N = int(rng.integers(100, 400))
        pc0, flow = rng.uniform(-50, 50, (N, 4)).astype(f32), rng.normal(0, 1, (N, 3)).astype(f32)
        label = rng.choice(np.concatenate([s.sorted_id, [0, -1]]), N).astype(np.int64)
        E = ref.ego_transform(ref.ego_pose(k), ref.ego_pose(k + 1))
        pl = ref.Plan(*(a[slice(*res.rows(n, k))] for a in wants[1]))
        data.append((pc0, flow, label, E, ref.apply_sweep(pc0, flow, label, E, s, pl, 0)))
    s1 = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s1):
        got = eng.apply(res, picks, [d[0] for d in data], [torch.from_numpy(d[1]).to(gpu) for d in data], [d[2] for d in data], [d[3] for d in data])
    s1.synchronize()
    for j, d in enumerate(data):
        same_bits(got.sweep(j).cpu().numpy(), d[4][0], f"sweep {j}")
        assert got.counts[j].tolist() == [d[4][1], d[4][2]] and d[4][1] > 0
    none = eng.apply(res, [], [], [], [], [])
    assert none.flow.shape == (0, 3) and none.counts.shape == (0, 2)
    with pytest.raises(ValueError, match="row-aligned"):
        eng.apply(res, picks[:1], [data[0][0]], [data[0][1][:-1]], [data[0][2]], [data[0][3]])
    with pytest.raises(ValueError, match="one integer per point"):
        eng.apply(res, picks[:1], [data[0][0]], [data[0][1]], [data[0][2].astype(f32)], [data[0][3]])


# ---- the program, end to end -------------------------------------------------------------------------------------------------------------------
VEHICLES = ((10.0, 12.0, 0.3, 5.0), (-18.0, 20.0, 2.0, 12.0), (25.0, -22.0, -1.2, 20.0))      # x, y, heading, speed [m/s]


def drive(root, n_scenes=2, n_sweeps=12, sigma=0.05, dt=0.1):
    """a small npz dataset: per scene three well-separated vehicles of 200 points at 5, 12 and 20 m/s and 300 static points seen from an ego
    that drives and turns slowly; the stored flow ``res`` is the truth plus one common offset of sigma per cluster and sweep.  Returns
    {(scene, timestamp): (truth float32 [N, 3], vehicle rows bool [N])}"""
    import boxfit_ref
    from himo_amd.dataset import NpzDataset
    frames, truth = [], {}
    for sc in range(n_scenes):
        rng = np.random.default_rng(200 + sc)
        static = np.concatenate([rng.uniform(-45, 45, (300, 2)), rng.uniform(-1, 2, (300, 1))], axis=1)
        for k in range(n_sweeps):
            pose0, pose1 = ref.ego_pose(k, speed=3.0, turn=0.01), ref.ego_pose(k + 1, speed=3.0, turn=0.01)
            world, nxt, ids, offs = [static], [static], [np.zeros(300, np.int32)], [np.zeros((300, 3))]
            for j, (x, y, yaw, speed) in enumerate(VEHICLES):
                v = speed * np.array([math.cos(yaw), math.sin(yaw), 0.0])
                centre = np.array([x, y]) + v[:2] * dt * k
                xy = boxfit_ref.lshape(rng, 200, yaw, 4.5, 1.9, 0.02, tuple(centre))
                pts = np.concatenate([xy, rng.uniform(-0.5, 1.5, (200, 1))], axis=1)
                world.append(pts), nxt.append(pts + v * dt), ids.append(np.full(200, 11 + j, np.int32))
                offs.append(np.tile(rng.normal(0.0, sigma, (1, 3)), (200, 1)))
            world, nxt, ids, offs = np.concatenate(world), np.concatenate(nxt), np.concatenate(ids), np.concatenate(offs)
            into = lambda pose, p: (p - pose[:3, 3]) @ pose[:3, :3]      # noqa: E731  (inv(pose) p for a rigid pose)
            p0, p1 = into(pose0, world), into(pose1, nxt)
            order = rng.permutation(len(p0))
            flow = (p1 - p0).astype(f32)[order]
            n = len(order)
            f = {"scene_id": f"s{sc}", "timestamp": 1000 + k, "pc0": p0.astype(f32)[order], "pose0": pose0, "pose1": pose1, "lidar_dt": np.zeros(n, f32),
                 "gm0": np.zeros(n, bool), "flow": flow, "flow_is_valid": np.ones(n, np.uint8), "flow_category_indices": np.zeros(n, np.uint8),
                 "ids": ids[order], "res": (flow + offs[order]).astype(f32)}
            frames.append(f)
            truth[(f["scene_id"], f["timestamp"])] = (flow, ids[order] > 0)
    NpzDataset.write(root, frames)
    return truth


def test_program_end_to_end_on_an_npz_container(gpu, tmp_path, monkeypatch, capsys):
    from himo_amd import box_fit, eval_flow, track, track_flow
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "drive"
    truth = drive(root)
    box_fit.main(str(root), "res", "ids")
    track.main(str(root), "res")
    capsys.readouterr()
    out = tmp_path / "track_flow.json"
    numbers = track_flow.main(str(root), "res", "ids", json_path=str(out), batch=1, sweeps_per_launch=5)
    assert json.loads(out.read_text()) == numbers and list(numbers) == ["res"]
    printed = capsys.readouterr().out
    assert "track flow, v1; parity unpinned" in printed and "res -> res_track" in printed
    r = numbers["res"]
    assert r["confirmed_tracks"] == 6 and r["boxes_moving"] == 72 and r["boxes_static"] == 0 and r["boxes_left_alone"] == 0
    assert r["points"] == 24 * 900 and r["points_rewritten"] == r["points_moving"] == 24 * 600 and 0.01 < r["mean_shift"] < 0.2

    def load(keys):
        got = {}
        for (sc, ts) in truth:
            with np.load(root / sc / f"{ts}.npz") as z:
                got[(sc, ts)] = {k: z[k] for k in keys}
        return got
    stored = load(("res", "res_track", "ids", "pc0", "pose0", "pose1", "boxes_res", "tracks_res"))
    before, after = [], []
    for key, (flow, vehicle) in truth.items():
        f = stored[key]
        assert f["res_track"].dtype == np.float32 and f["res_track"].shape == flow.shape
        assert bits(f["res_track"][~vehicle]).tobytes() == bits(f["res"][~vehicle]).tobytes()      # unlabelled rows keep their bytes
        before.append(np.linalg.norm(f["res"][vehicle].astype(np.float64) - flow[vehicle], axis=1))
        after.append(np.linalg.norm(f["res_track"][vehicle].astype(np.float64) - flow[vehicle], axis=1))
    before, after = float(np.concatenate(before).mean()), float(np.concatenate(after).mean())
    with capsys.disabled():
        print(f"\nmean end-point error of the vehicles' rows: {before:.4f} m under res, {after:.4f} m under res_track, ratio {after / before:.3f}")
    assert after < 0.7 * before
    # the stored flow is the restatement's, from the stored boxes and tracks
    for sc in ("s0", "s1"):
        keys = sorted(k for k in truth if k[0] == sc)
        sweeps = [ref.prepare(stored[k]["boxes_res"], stored[k]["tracks_res"], stored[k]["pose0"], stored[keys[0]]["pose0"]) for k in keys]
        for k, s, pl in zip(keys, sweeps, ref.plan_scene(sweeps)):
            f = stored[k]
            want, _, _ = ref.apply_sweep(f["pc0"], f["res"], f["ids"], ref.ego_transform(f["pose0"], f["pose1"]), s, pl, 0)
            same_bits(f["res_track"], want, k)
    # the evaluator reads the key
    m = eval_flow.main(str(root), res_names="res,res_track", data_name="av2")
    res = m.results()
    assert set(res) == {"res", "res_track"} and res["res_track"]["counted"] == res["res"]["counted"] > 0
    assert "res_track in av2" in capsys.readouterr().out
    # a second run is refused and leaves the files alone; --overwrite replaces, here in the other mode
    with pytest.raises(FileExistsError, match="res_track.*--overwrite"):
        track_flow.main(str(root), "res", "ids")
    track_flow._cli(["--data_dir", str(root), "--res_names", "res", "--label_key", "ids", "--overwrite", "--mode", "replace", "--half", "1"])
    again = load(("res_track",))
    for sc in ("s0", "s1"):
        keys = sorted(k for k in truth if k[0] == sc)
        sweeps = [ref.prepare(stored[k]["boxes_res"], stored[k]["tracks_res"], stored[k]["pose0"], stored[keys[0]]["pose0"]) for k in keys]
        for k, s, pl in zip(keys, sweeps, ref.plan_scene(sweeps, half=1)):
            f = stored[k]
            want, _, _ = ref.apply_sweep(f["pc0"], f["res"], f["ids"], ref.ego_transform(f["pose0"], f["pose1"]), s, pl, 1)
            same_bits(again[k]["res_track"], want, k)


def test_program_on_h5_scene_files(gpu, tmp_path, monkeypatch):
    import warnings
    from himo_amd import box_fit, synthetic, track, track_flow
    from himo_amd.dataset import HDF5Dataset, h5_reader
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    root = tmp_path / "scenes"
    root.mkdir()
    synthetic.write_h5_scenes(root, [synthetic.make_scene(s, 4, n_points=3000, n_instances=4, scene_id=f"sc{s}") for s in (1, 2)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # (the last sweep of a scene has no successor)
        box_fit.main(str(root), "flow", "flow_instance_id")
        track.main(str(root), "flow")
        numbers = track_flow.main(str(root), "flow", "flow_instance_id", min_len=2)
        with pytest.raises(FileExistsError, match="--overwrite"):
            track_flow.main(str(root), "flow", "flow_instance_id")
        ds = HDF5Dataset(root, vis_name="", fields=("pose0",))
    scenes = {}
    for scene_id, ts in ds.index:
        with h5_reader().File(root / f"{scene_id}.h5", "r") as h:
            g = h[str(ts)]
            f = {k: np.asarray(g[k][:]) for k in ("boxes_flow", "tracks_flow", "flow", "flow_track", "flow_instance_id")}
            f["pose0"] = np.asarray(g["pose"][:])
            scenes.setdefault(scene_id, []).append((f, ts))
    ds.close()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ds = HDF5Dataset(root, vis_name="", fields=("pose0", "pose1", "pc0"))
        frames = {tuple(map(str, ds.index[i])): ds[i] for i in range(len(ds))}
        ds.close()
    rewritten = 0
    for scene_id, items in scenes.items():
        sweeps = [ref.prepare(f["boxes_flow"], f["tracks_flow"], f["pose0"], items[0][0]["pose0"]) for f, _ in items]
        for (f, ts), s, pl in zip(items, sweeps, ref.plan_scene(sweeps, min_len=2)):
            fr = frames[(scene_id, str(ts))]
            want, nm, ns = ref.apply_sweep(fr["pc0"], f["flow"], f["flow_instance_id"], ref.ego_transform(fr["pose0"], fr["pose1"]), s, pl, 0)
            same_bits(f["flow_track"], want, (scene_id, ts))
            rewritten += nm + ns
    assert numbers["flow"]["points_rewritten"] == rewritten and [len(v) for v in scenes.values()] == [3, 3]
