"""An exact restatement of the instance evaluator (csrc/evalmetrics.hip: himo_eval_instances) and of the exact nearest-neighbour
search (csrc/nn.hip: himo_nn_search, himo_sqrt_inplace).  CPU only, numpy.

Both files are compiled with -ffp-contract=off and write every fused multiply-add out, so the order of every operation is the
source's and this oracle restates it; tests/test_eval_conformance_gpu.py demands equal bits of every float64 the stage returns.
The shared arithmetic (fma64, pose_flow, lu_ego, frame_max) is compdis_oracle's.

  select       eval_mask != 0 and (class_lut[category] & 3) != 0; the label of a point is (frame, class_lut & 3, id mod 2^32)
  segments     the distinct labels in (frame, group, id) order, the rows of each in index order (the counting sort of rank_frames_kernel)
  payload      payload_kernel's five modes, operation by operation
  seg_nn2      the minimum over a segment of (dx*dx + dy*dy) + dz*dz in float64 (a candidate that is not < +inf never wins)
  fixed_sum    seg_reduce_kernel's sum: thread t adds rows t, t + 256, ... from 0.0, then the tree 128, 64, ... 1
  records      the himo_instance_record array of a case, sorted by (frame, group, instance)
  nn_search    himo_nn_search: float64 the value and the lowest row that attains it; float32 the exact value (in float64 from the
               float32 inputs) for the bound 6 * 2^-24 (check_nn_f32)
  CASES, NN_CASES   the matrices; every case names the paths it promises to reach and ``promise`` / ``nn_promise`` prove each one
               with the kernels' own integer arithmetic
  WRONG, NN_WRONG   the restatement with one line changed: tests/test_eval_oracle.py shows each failing the checks on a named case
"""
from __future__ import annotations

import numpy as np

import compdis_oracle as co

F32, F64 = np.float32, np.float64
MODE_FLOW, MODE_COMPDIS, MODE_RAW, MODE_SCORE, MODE_DIRECT = range(5)          # include/himo_amd.h HIMO_EVAL_*
MODE_NAMES = ("flow", "compdis", "raw", "score", "direct")
FLAG_POSE_IS_EGO, DIRECT_EST_IS_DIS = 0x8, 0x100
SEL_BLOCK, LANE_PTS = 1024, 4                                                  # evalmetrics.hip:29-30
RANK_THREADS, RANK_SLOTS, RANK_ADMIT = 1024, 2048, 1536                        # :175-176, :219
RANK_MULT = 0x9E3779B97F4A7C15                                                 # :213
RED_THREADS, RED_GRID = 256, 1024                                              # :357, :502
SCAN_CHUNK = 1024                                                              # :114
NN_THREADS, NN_TILE = 256, 1024                                                # nn.hip:26-27
U24 = 2.0 ** -24
RECORD_DTYPE = np.dtype([("frame", "<i4"), ("group", "<i4"), ("instance", "<i8"), ("num_pts", "<i8"),
                         ("vel", "<f8"), ("dis", "<f8"), ("mpe", "<f8"), ("cham", "<f8")])
INT_FIELDS, F64_FIELDS = ("frame", "group", "instance", "num_pts"), ("vel", "dis", "mpe", "cham")

WRONG = ("no_group", "no_frame", "dis3", "one_sided", "sqrt_after_mean", "vel_no_dt")
NN_WRONG = ("ties_highest", "range_end_plus_one")


# ---- selection and grouping ------------------------------------------------------------------------------------------------------
def rank_slot(lab):
    """the initial slot of a label in rank_frames_kernel's table: the top 11 bits of the 64-bit product"""
    return (np.asarray(lab, np.uint64) * np.uint64(RANK_MULT)) >> np.uint64(53)


def labels_of(frame, group, id32):
    return (np.asarray(frame, np.uint64) << np.uint64(34)) | (np.asarray(group, np.uint64) << np.uint64(32)) | np.asarray(id32, np.uint64)


def select(d):
    """rows (ascending), frame, group and id mod 2^32 of the selected points (evalmetrics.hip:73-75, :158-159)"""
    lutv = (np.asarray(d.lut, np.uint8) & 3)[d.cat]
    rows = np.nonzero((d.mask != 0) & (lutv != 0))[0]
    frame = (np.searchsorted(d.offsets, rows, side="right") - 1).astype(np.int64)
    return rows, frame, lutv[rows].astype(np.int64), d.inst[rows].astype(np.int64) & 0xFFFFFFFF


def segments(d, wrong=None):
    """[(frame, group, id32, positions into the selected rows, ascending)] in (frame, group, id) order"""
    rows, frame, group, id32 = select(d)
    kf = np.zeros_like(frame) if wrong == "no_frame" else frame
    kg = np.zeros_like(group) if wrong == "no_group" else group
    order = np.lexsort((id32, kg, kf))                                            # stable: index order inside a label
    if len(order) == 0:
        return rows, []
    key = np.stack([kf[order], kg[order], id32[order]], 1)
    cut = np.nonzero(np.any(key[1:] != key[:-1], axis=1))[0] + 1
    out = []
    for pos in np.split(order, cut):
        out.append((int(frame[pos[0]]), int(group[pos[0]]), int(id32[pos[0]]), pos))
    return rows, out


# ---- the per-point chain ---------------------------------------------------------------------------------------------------------
def norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])     # evalmetrics.hip:282


_EGO = {}


def transforms(d, frames):
    """{frame: ([3, 4] float64 transform, float32 maximum of lidar_dt)} for the frames named: the given rows under POSE_IS_EGO,
    compute_ego's own order otherwise (compdis_oracle.lu_ego), the maximum as frame_prep_kernel forms it"""
    out = {}
    for f in frames:
        f = int(f)
        if d.c["pose_is_ego"]:
            ego = np.asarray(d.given[f], F64)[:3]
        else:
            k = (d.pose0[f].tobytes(), d.pose1[f].tobytes())
            if k not in _EGO:
                _EGO[k] = co.lu_ego(d.pose0[f], d.pose1[f])
            ego = _EGO[k]
        out[f] = (ego, co.frame_max(d.dt[int(d.offsets[f]):int(d.offsets[f + 1])]))
    return out


def payload(d, rows, frame, wrong=None):
    """payload_kernel (evalmetrics.hip:284-354) on the selected rows: refined GT and estimate [M, 3], speed, range, error [M], float64"""
    c = d.c
    mode, n = c["mode"], len(rows)
    sdt = F64(c["sensor_dt"])
    with np.errstate(all="ignore"):
        if mode == MODE_SCORE:                                                    # :290-305, float32 arithmetic on the zip payloads
            p = d.pc[rows, :3] if c["has_pc"] else np.zeros((n, 3), F32)
            gd, ed = d.gt[rows], d.est[rows]
            g, e = (p + gd).astype(F64), (p + ed).astype(F64)
            df = gd - ed
            d2 = np.zeros(n, F32)
            for k in range(3):
                d2 = d2 + df[:, k] * df[:, k]
            err = np.sqrt(d2).astype(F64)
            vel = d.dt[rows].astype(F64) if c["has_dt"] else np.zeros(n, F64)
            return g, e, vel, np.zeros(n, F64), err
        pcr = d.pc[rows]
        p32 = pcr[:, :3]
        p = p32.astype(F64)
        if mode == MODE_DIRECT:                                                   # :306-324
            gtf = np.asarray(d.gt, F64)[rows]
            dt0 = d.dt[rows]
            pf = None
        else:                                                                     # :326-349
            pf, dt0 = np.empty((n, 3), F64), np.empty(n, F32)
            xf = transforms(d, np.unique(frame))
            for f, (ego, fmax) in xf.items():
                m = frame == f
                pf[m] = co.pose_flow(ego, p32[m], False)                          # :335  k-ordered FMA dot, (dot + t) - p
                dt0[m] = F32(fmax) - d.dt[rows[m]]                                # :330  float32
            gtf = d.gt[rows].astype(F64) - pf                                     # :336
        d0 = dt0.astype(F64)
        g = p + gtf / sdt * d0[:, None]                                           # :316, :337  divide THEN multiply
        if mode == MODE_COMPDIS or (mode == MODE_DIRECT and c["est_is_dis"]):
            e = (p32 + d.est[rows]).astype(F64)                                   # :317, :339  float32 + float32
        else:
            if mode == MODE_RAW:
                ef = np.zeros((n, 3), F64)
            elif mode == MODE_DIRECT:
                ef = np.asarray(d.est, F64)[rows]
            else:
                ef = d.est[rows].astype(F64) - pf                                 # :341
            e = p + ef / sdt * d0[:, None]                                        # :318, :342
        vel = norm3(gtf)
        s = np.zeros(n, F32)
        for k in range(3 if wrong == "dis3" else c["stride"]):                    # :346-347: ALL columns, in column order, float32
            s = s + pcr[:, k] * pcr[:, k]
        dis = np.sqrt(s).astype(F64)
        err = norm3(g - e)
    return g, e, vel, dis, err


# ---- segment NN and the means ------------------------------------------------------------------------------------------------------
def _pair_d2(q, r):
    dx, dy, dz = q[:, None, 0] - r[None, :, 0], q[:, None, 1] - r[None, :, 1], q[:, None, 2] - r[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz                                          # nn.hip:55-58


def seg_nn2(q, r):
    """per row of q the minimum squared distance over r, float64; ``d < best`` from +inf: a NaN or +inf candidate never wins"""
    out = np.empty(len(q), F64)
    step = max(1, (1 << 22) // max(len(r), 1))
    with np.errstate(all="ignore"):
        for a in range(0, len(q), step):
            d2 = _pair_d2(q[a:a + step], r)
            out[a:a + step] = np.where(d2 < np.inf, d2, np.inf).min(axis=1) if len(r) else np.inf
    return out


def fixed_sum(v):
    """seg_reduce_kernel:363-377: 256 running sums over rows t, t + 256, ... from 0.0 (adding the 0.0 of a row that does not exist
    changes no bit: a running sum that starts at +0.0 is never -0.0), then red[t] += red[t + off] for off = 128 ... 1"""
    v = np.asarray(v, F64)
    k = -(-len(v) // RED_THREADS)
    pad = np.zeros(max(k, 1) * RED_THREADS, F64)
    pad[:len(v)] = v
    acc = np.zeros(RED_THREADS, F64)
    with np.errstate(all="ignore"):
        for row in pad.reshape(-1, RED_THREADS):
            acc = acc + row
        off = RED_THREADS // 2
        while off:
            acc[:off] = acc[:off] + acc[off:2 * off]
            off >>= 1
    return acc[0]


def records(d, wrong=None):
    """the records of a case, sorted by (frame, group, instance)"""
    rows, segs = segments(d, wrong)
    out = np.zeros(len(segs), RECORD_DTYPE)
    if not segs:
        return out
    _, frame, _, _ = select(d)
    g, e, vel, dis, err = payload(d, rows, frame, wrong)
    sdt = F64(d.c["sensor_dt"])
    with np.errstate(all="ignore"):
        for i, (f, grp, ident, pos) in enumerate(segs):
            n = F64(len(pos))
            d12, d21 = seg_nn2(g[pos], e[pos]), seg_nn2(e[pos], g[pos])             # :498, :500
            if wrong == "sqrt_after_mean":
                a, b = np.sqrt(fixed_sum(d12) / n), np.sqrt(fixed_sum(d21) / n)
            else:
                a, b = fixed_sum(np.sqrt(d12)) / n, fixed_sum(np.sqrt(d21)) / n   # :366
            v = fixed_sum(vel[pos]) / n
            out[i] = (f, grp, ident, len(pos), v if wrong == "vel_no_dt" else v / sdt, fixed_sum(dis[pos]) / n, fixed_sum(err[pos]) / n,
                      a if wrong == "one_sided" else (a + b) / F64(2.0))          # :381-384
    return np.sort(out, order=["frame", "group", "instance"])


# ---- the checks the GPU module applies (proved on the restatement's own output in tests/test_eval_oracle.py) ---------------------
def _bits(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def same_f64(a, b):
    """equal bits; a NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


def sort_records(r):
    return np.sort(np.asarray(r, RECORD_DTYPE), order=["frame", "group", "instance"])


def check_records(got, want, case=""):
    """``got`` in any order: the integer fields equal, the four doubles equal in bits.  Returns the number of doubles compared."""
    got, want = sort_records(got), sort_records(want)
    assert len(got) == len(want), f"{case}: {len(got)} records, the restatement has {len(want)}"
    for k in INT_FIELDS:
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, f"{case}: {k} differs in {bad.size} records; first {got[bad[0]]} for {want[bad[0]]}"
    for k in F64_FIELDS:
        if not same_f64(got[k], want[k]):
            bad = np.nonzero((_bits(got[k]) != _bits(want[k])) & ~(np.isnan(got[k]) & np.isnan(want[k])))[0]
            i = int(bad[0])
            raise AssertionError(f"{case}: {k} differs in bits in {bad.size} of {len(want)} records; first (frame {want['frame'][i]}, group "
                                 f"{want['group'][i]}, instance {want['instance'][i]}, {want['num_pts'][i]} points): {got[k][i]!r} "
                                 f"({float(got[k][i]).hex()}) for {want[k][i]!r} ({float(want[k][i]).hex()})")
    return 4 * len(want)


def check_overflow(slots, counts, want, n_selected, max_records, case=""):
    """a call whose record buffer holds ``max_records``: counts = {M, K} whatever the room; the slots written are a duplicate-free
    subset of the expected records, every field complete"""
    K = len(want)
    assert [int(v) for v in counts] == [n_selected, K], f"{case}: counts {list(counts)} for {[n_selected, K]}"
    slots = np.asarray(slots, RECORD_DTYPE)
    assert len(slots) == min(K, max_records), f"{case}: {len(slots)} slots for {min(K, max_records)}"
    key = lambda r: list(zip(r["frame"].tolist(), r["group"].tolist(), r["instance"].tolist()))
    where = {k: i for i, k in enumerate(key(want))}
    ks = key(slots)
    assert len(set(ks)) == len(ks), f"{case}: a record appears twice"
    assert all(k in where for k in ks), f"{case}: a record that is not expected: {[k for k in ks if k not in where][:3]}"
    return check_records(slots, want[[where[k] for k in ks]], case)


# ---- himo_nn_search --------------------------------------------------------------------------------------------------------------
def nn_launch(nq):
    """launch_nn (nn.hip:143-165): the launch shape and its queries per block"""
    b = (nq + NN_THREADS - 1) // NN_THREADS
    if b >= 2048:
        return "QPT2", 2 * NN_THREADS
    if b >= 256:
        return "QPT1", NN_THREADS
    if b >= 64:
        return "SPLIT4", NN_THREADS // 4
    return "SPLIT16", NN_THREADS // 16


NN_SHAPES = ("QPT2", "QPT1", "SPLIT4", "SPLIT16")


def nn_search(q, r, q_off, r_off, f64, wrong=None):
    """(squared distance [nq], row [nq] int32).  float64: the kernel's value and the lowest row that attains it.  float32: the exact
    value, formed in float64 from the float32 inputs, and the lowest row that attains THAT (the kernel's row may differ where two
    candidates lie within the bound of each other: check_nn_f32).  An empty range, or one whose candidates are all NaN: +inf, -1."""
    T = F64 if f64 else F32
    q, r = np.ascontiguousarray(q, T).reshape(-1, 3).astype(F64), np.ascontiguousarray(r, T).reshape(-1, 3).astype(F64)
    dist, idx = np.full(len(q), np.inf, F64), np.full(len(q), -1, np.int32)
    with np.errstate(all="ignore"):
        for s in range(len(q_off) - 1):
            qa, qb, ra, rb = int(q_off[s]), int(q_off[s + 1]), int(r_off[s]), int(r_off[s + 1])
            if wrong == "range_end_plus_one":
                rb = min(rb + 1, len(r))
            if qb <= qa or rb <= ra:
                continue
            step = max(1, (1 << 22) // (rb - ra))
            for a in range(qa, qb, step):
                b = min(a + step, qb)
                d2 = _pair_d2(q[a:b], r[ra:rb])
                d2 = np.where(d2 < np.inf, d2, np.inf)
                best = d2.min(axis=1)
                if wrong == "ties_highest":
                    arg = d2.shape[1] - 1 - np.argmin(d2[:, ::-1], axis=1)
                else:
                    arg = np.argmin(d2, axis=1)                                   # the first minimal entry: the lowest row
                hit = best < np.inf
                dist[a:b] = best
                idx[a:b] = np.where(hit, arg + ra, -1)
    return dist, idx


def exact_d2(q, r, rows):
    """the exact squared distance of query i to reference rows[i] (float64 from the inputs' own values)"""
    q, r = np.asarray(q).reshape(-1, 3).astype(F64), np.asarray(r).reshape(-1, 3).astype(F64)
    with np.errstate(all="ignore"):
        dv = q - r[rows]
        return (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]


def check_nn_f64(got_d, got_i, want_d, want_i, case=""):
    assert same_f64(got_d, want_d), f"{case}: {int((_bits(got_d) != _bits(want_d)).sum())} float64 distances differ in bits"
    if got_i is not None:
        bad = np.nonzero(np.asarray(got_i) != want_i)[0]
        assert bad.size == 0, f"{case}: {bad.size} rows differ; first query {bad[0]}: {got_i[bad[0]]} for {want_i[bad[0]]}"
    return len(want_d)


def check_nn_f32(got_d, got_i, q, r, want_d, want_i, q_off, r_off, case=""):
    """|got - exact| <= 6 * 2^-24 * exact: 2 * 2^-24 for squaring a rounded difference, one rounding for the product and one for each
    of the two fused multiply-adds, on a sum of non-negative terms; the returned row lies in the query's range and its exact distance
    within the same factor of the exact minimum.  Where the range is empty: +inf and -1, as the restatement."""
    got_d = np.asarray(got_d, F32).astype(F64)
    empty = want_i < 0
    assert bool(np.array_equal(np.isinf(got_d) & (got_d > 0), empty)), f"{case}: +inf at other queries than the empty ranges"
    ok = ~empty
    err = np.abs(got_d[ok] - want_d[ok])
    bad = err > 6 * U24 * want_d[ok]
    assert not bad.any(), f"{case}: {int(bad.sum())} float32 distances beyond 6 * 2^-24 of the exact minimum; worst {float((err / np.maximum(want_d[ok], 1e-300)).max()) / U24:.3g} * 2^-24"
    if got_i is not None:
        got_i = np.asarray(got_i)
        assert bool((got_i[empty] == -1).all()), f"{case}: a row for an empty range"
        seg = np.searchsorted(np.asarray(q_off), np.nonzero(ok)[0], side="right") - 1
        lo, hi = np.asarray(r_off)[seg], np.asarray(r_off)[seg + 1]
        assert bool(((got_i[ok] >= lo) & (got_i[ok] < hi)).all()), f"{case}: a row outside the query's range"
        ex = exact_d2(np.asarray(q, F32).reshape(-1, 3)[ok], r, got_i[ok])
        bad = np.abs(ex - want_d[ok]) > 6 * U24 * want_d[ok]
        assert not bad.any(), f"{case}: {int(bad.sum())} returned rows are not within 6 * 2^-24 of the nearest"
    return int(ok.sum())


# ---- the evaluator's matrix ---------------------------------------------------------------------------------------------------------
# class_lut of the cases: category -> byte.  5 -> 1 (CAR), 7 -> 2 (OTHER_VEHICLES), 9 -> 3, 11 -> 4 (& 3 == 0: not evaluated),
# 13 -> 5 (group 1), 15 -> 6 (group 2), 17 -> 255 (group 3); every other category 0.
LUT = np.zeros(256, np.uint8)
CAT_OF_BYTE = {1: 5, 2: 7, 3: 9, 4: 11, 5: 13, 6: 15, 255: 17}
for _b, _c in CAT_OF_BYTE.items():
    LUT[_c] = _b
DEAD_CATS = np.array([0, 1, 2, 3, 11, 20, 254], np.uint8)                          # (11 holds the byte 4)


def frame_spec(labels, unselected=0, shuffle=True):
    """a frame: ``labels`` = [(lut byte, instance id, number of points)], ``unselected`` more points that are not selected"""
    return dict(labels=[(int(b), int(i), int(n)) for b, i, n in labels], unselected=int(unselected), shuffle=shuffle)


def _rand_frame(rng, size, p_sel, n_inst, ids=None):
    n_sel = int(round(size * p_sel))
    if n_sel == 0 or n_inst == 0:
        return frame_spec([], size)
    n_inst = min(n_inst, n_sel)
    cuts = np.sort(rng.choice(np.arange(1, n_sel), n_inst - 1, replace=False)) if n_inst > 1 else np.array([], np.int64)
    counts = np.diff(np.concatenate([[0], cuts, [n_sel]]))
    ids = rng.choice(1 << 20, n_inst, replace=False) if ids is None else ids
    return frame_spec([(1 + (k % 2), ids[k], counts[k]) for k in range(n_inst)], size - n_sel)


def _exact_labels(rng, n_labels, n_points, byte=1):
    """``n_points`` selected points over exactly ``n_labels`` distinct ids (half under each group when byte is None)"""
    ids = rng.choice(1 << 31, n_labels, replace=False)
    extra = np.bincount(rng.integers(0, n_labels, n_points - n_labels), minlength=n_labels)
    return frame_spec([(byte if byte else 1 + (k % 2), ids[k], 1 + extra[k]) for k in range(n_labels)])


def _slot_ids(frame, group, slot, count, start=1):
    """the first ``count`` ids >= start whose label (frame, group, id) has ``slot`` as its initial slot"""
    ids = np.arange(start, start + (1 << 20), dtype=np.uint64)
    hit = ids[rank_slot(labels_of(frame, group, ids)) == np.uint64(slot)]
    assert len(hit) >= count
    return [int(v) for v in hit[:count]]


def _case(frames, promises=(), **kw):
    c = dict(frames=frames, promises=tuple(promises), mode=MODE_FLOW, stride=4, pose="small", pose_is_ego=False, est_is_dis=False,
             has_pc=True, has_dt=True, sensor_dt=0.1, both_ego_modes=False, reference=True, seed=0)
    c.update(kw)
    return c


def _make_cases():
    rng = np.random.default_rng(20261020)
    C = {}
    R = lambda size, p=0.4, k=6, ids=None: _rand_frame(rng, size, p, k, ids)
    # blocks and frames
    C["blocks_1022_5_1021_1027"] = _case([R(1022), R(5, 0.8, 2), R(1021), R(1027)], ("uniform", "straddling", "lane_in_two_frames"), pose="mixed")
    C["empties_0_3_0_1_0"] = _case([frame_spec([]), frame_spec([(1, 7, 2), (2, 7, 1)]), frame_spec([]), frame_spec([(1, 9, 1)]), frame_spec([])],
                                   ("empty_frames", "straddling", "lane_in_two_frames"), pose="mixed")
    C["unselected_frame_between"] = _case([R(40), frame_spec([], 50), R(30)], ("unselected_frame_between", "straddling"))
    C["total1023"] = _case([R(501), R(522)], ("total:1023", "boundary_not_mult4"))
    C["total1024"] = _case([R(501), R(523)], ("total:1024", "boundary_not_mult4"))
    C["total1025"] = _case([R(501), R(524)], ("total:1025", "boundary_not_mult4", "uniform"))
    sizes = [int(v) for v in rng.integers(0, 3, 1025)]
    sizes[-1], sizes[-2], sizes[3] = 2, 1, 0
    C["frames1025"] = _case([R(s, 0.7, 2) for s in sizes], ("frame_scan_carry", "empty_frames", "lane_in_two_frames"), pose="mixed")
    C["points_1024x1024_plus_5"] = _case([R(400000, 0.0003, 9), frame_spec([]), R(648576, 0.0002, 7), R(5, 0.6, 2)],
                                         ("block_scan_carry", "empty_frames", "uniform", "straddling"), pose="mixed", reference=False)
    # ranking
    C["selected_1_1023_1024_1025_2049"] = _case([frame_spec([(1, 3, 1)]), _exact_labels(rng, 2, 40, None), _exact_labels(rng, 5, 1023, None),
                                                 _exact_labels(rng, 7, 1024, None), _exact_labels(rng, 6, 1025, None), _exact_labels(rng, 9, 2049, None)],
                                                ("selected:1", "selected:1023", "selected:1024", "selected:1025", "selected:2049", "labels:1", "labels:2",
                                                 "scattered_tiles"), pose="mixed")
    C["labels_1536_1537_2100"] = _case([_exact_labels(rng, 1536, 2000, None), _exact_labels(rng, 1537, 2000, None), _exact_labels(rng, 2100, 2300, None)],
                                       ("labels:1536", "labels:1537", "labels:2100", "table_path", "allpairs_path", "records_gt_1024"), reference=False)
    big = 1 << 32
    C["ids_and_groups"] = _case([frame_spec([(1, 0, 3), (2, 0, 4), (1, 1, 2), (1, 1 << 31, 5), (2, big - 1, 3), (1, big + 5, 2), (1, 5, 3), (2, -1, 2),
                                             (1, 77, 12), (2, 77, 11)], 9),
                                 frame_spec([(1, 77, 13), (2, 0, 1), (1, big - 1, 2), (2, 1 << 31, 2)], 5)],
                                ("same_id_both_groups", "same_id_two_frames", "edge_ids", "id_mod_2_32"), reference=False)
    h8 = _slot_ids(0, 1, RANK_SLOTS - 1, 8)
    s8 = _slot_ids(1, 2, 1000, 8)
    C["shared_slot_and_wrap"] = _case([frame_spec([(1, i, 2 + k) for k, i in enumerate(h8)] + [(2, 4242, 3), (1, 4243, 1)], 4),
                                       frame_spec([(2, i, 1 + k) for k, i in enumerate(s8)] + [(1, 99, 2)], 3)],
                                      ("shared_slot:8", "chain_wraps"))
    # segments
    C["segment_lengths"] = _case([frame_spec([(1 + (k % 2), 100 + k, n) for k, n in enumerate((1, 2, 255, 256, 257, 1023, 1024, 1025, 2049))], 40)],
                                 tuple(f"seg_len:{n}" for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049)) + ("scattered_tiles",))
    C["records1025"] = _case([_exact_labels(rng, 513, 1026, None), _exact_labels(rng, 512, 1024, None)], ("records:1025", "table_path"), reference=False)
    # modes and strides
    M = lambda: [R(300, 0.6, 6), R(7, 0.9, 2), R(260, 0.5, 5)]
    for mode in range(5):
        for stride in (3, 4):
            C[f"mode_{MODE_NAMES[mode]}_stride{stride}"] = _case(M(), (), mode=mode, stride=stride, pose="mixed")
        if mode != MODE_SCORE:
            C[f"mode_{MODE_NAMES[mode]}_stride6"] = _case(M(), ("extra_columns",), mode=mode, stride=6, sensor_dt=0.2)
    for stride in (3, 4):
        C[f"direct_est_is_dis_stride{stride}"] = _case(M(), (), mode=MODE_DIRECT, stride=stride, est_is_dis=True)
    C["score_pc0_null"] = _case(M(), (), mode=MODE_SCORE, has_pc=False)
    C["score_lidar_dt_null"] = _case(M(), (), mode=MODE_SCORE, has_dt=False, stride=3)
    C["score_both_null"] = _case(M(), (), mode=MODE_SCORE, has_pc=False, has_dt=False)
    for kind in ("identity", "yaw90", "tie45", "far"):
        C[f"pose_{kind}"] = _case([R(2, 1.0, 1), R(270, 0.6, 4)], (), pose=kind, both_ego_modes=True, mode=(MODE_COMPDIS if kind == "tie45" else MODE_FLOW))
    C["lut_bytes_3_and_above"] = _case([frame_spec([(3, 8, 12), (1, 8, 11), (5, 8, 4), (6, 8, 3), (2, 8, 2), (255, 8, 5), (4, 8, 20)], 6)],
                                       ("lut_byte_3", "lut_byte_above_3"), reference=False)
    # the evaluator's own searches (explicit per-query ranges, float64) through the wider launch shapes: M > 16128 and M > 65280
    L = lambda n, first: frame_spec([(1 + (k % 2), first + k, 100) for k in range(n)], 300)
    C["selected_17000"] = _case([L(170, 10)], ("eval_launch:SPLIT4", "scattered_tiles"))
    C["selected_66000"] = _case([L(400, 10), L(260, 5)], ("eval_launch:QPT1", "scattered_tiles"), mode=MODE_DIRECT, stride=3)
    for i, k in enumerate(C):
        C[k]["seed"] = 3000 + i
    return C


CASES = _make_cases()
CASE_NAMES = tuple(CASES)


class Data:
    pass


def make_data(c, offsets, pc, gt, est, dt, cat, inst, mask, lut, pose0=None, pose1=None):
    """a case's operands as the entry point receives them"""
    d = Data()
    d.c, d.offsets = c, np.asarray(offsets, np.int64)
    d.sizes = [int(v) for v in np.diff(d.offsets)]
    d.F, d.T = len(d.sizes), int(d.offsets[-1])
    d.pc, d.gt, d.est, d.dt = pc, gt, est, dt
    d.cat, d.inst, d.mask, d.lut = np.asarray(cat, np.uint8), np.asarray(inst, np.int64), np.asarray(mask, np.uint8), np.asarray(lut, np.uint8)
    d.pose0, d.pose1 = pose0, pose1
    d.given = None
    if pose0 is not None and pose1 is not None:
        d.given = co.numpy_egos(d)
    return d


_BUILT = {}


def build(name, pose_is_ego=None):
    """the operands of a case, from its seed"""
    key = (name, pose_is_ego)
    if key in _BUILT:
        return _BUILT[key]
    c = dict(CASES[name])
    if pose_is_ego is not None:
        c["pose_is_ego"] = pose_is_ego
    rng = np.random.default_rng(c["seed"])
    cats, insts, masks, sizes = [], [], [], []
    for fs in c["frames"]:
        cat_f, inst_f, mask_f = [], [], []
        for byte, ident, n in fs["labels"]:
            cat_f.append(np.full(n, CAT_OF_BYTE[byte], np.uint8))
            inst_f.append(np.full(n, ident, np.int64))
            mask_f.append(rng.choice(np.array([1, 1, 2, 255], np.uint8), n) if LUT[CAT_OF_BYTE[byte]] & 3 else np.ones(n, np.uint8))
        u = fs["unselected"]
        if u:
            kill = rng.integers(0, 3, u)                           # 0: the mask is 0;  1: a category outside the table;  2: both
            live = np.array([5, 7], np.uint8)
            cat_f.append(np.where(kill == 0, rng.choice(live, u), rng.choice(DEAD_CATS, u)).astype(np.uint8))
            inst_f.append(rng.integers(0, 50, u).astype(np.int64))
            mask_f.append(np.where(kill == 1, 1, 0).astype(np.uint8))
        n = sum(len(a) for a in cat_f)
        sizes.append(n)
        if n:
            order = rng.permutation(n) if fs["shuffle"] else np.arange(n)
            cats.append(np.concatenate(cat_f)[order]); insts.append(np.concatenate(inst_f)[order]); masks.append(np.concatenate(mask_f)[order])
    T = sum(sizes)
    cat = np.concatenate(cats) if cats else np.zeros(0, np.uint8)
    inst = np.concatenate(insts) if insts else np.zeros(0, np.int64)
    mask = np.concatenate(masks) if masks else np.zeros(0, np.uint8)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    F, stride, mode = len(sizes), c["stride"], c["mode"]
    pc = np.zeros((T, stride), F32)
    # an instance is a cluster the size of a vehicle, its points closer to each other than the estimate's error is large: the nearest
    # neighbour of a refined point is then often NOT its own counterpart, and the two halves of the Chamfer distance differ
    ids = np.searchsorted(offsets, np.arange(T), side="right") - 1
    _, inv = np.unique(ids * 1000003 + cat.astype(np.int64) * 7919 + inst, return_inverse=True)
    centre = rng.uniform(-40.0, 40.0, (int(inv.max()) + 1 if T else 0, 3)) * np.array([1.0, 1.0, 0.02])
    pc[:, :3] = centre[inv] + rng.uniform(-1.0, 1.0, (T, 3)) * np.array([2.2, 1.0, 0.7])
    if stride > 3:
        pc[:, 3:] = rng.uniform(-5.0, 5.0, (T, stride - 3))
    dt = rng.uniform(0.0, 0.1, T).astype(F32)
    kinds = co.POSE_KINDS if c["pose"] == "mixed" else (c["pose"],)
    pairs = {k: co.pose_pair(k) for k in kinds}
    pose_kinds = [kinds[f % len(kinds)] for f in range(F)]
    pose0 = np.stack([pairs[k][0] for k in pose_kinds])
    pose1 = np.stack([pairs[k][1] for k in pose_kinds])
    move = rng.uniform(-1.5, 1.5, (T, 3))
    if mode == MODE_SCORE:
        gt = (move * 0.3).astype(F32)
        est = (move * 0.3 + rng.normal(0, 0.3, (T, 3))).astype(F32)
        dt = rng.uniform(0.0, 1.0, T).astype(F32)                                  # gt_flow_norm
    elif mode == MODE_DIRECT:
        gt = move.astype(F64)
        est = (move * 0.05 + rng.normal(0, 0.3, (T, 3))).astype(F32) if c["est_is_dis"] else (move + rng.normal(0, 0.8, (T, 3))).astype(F64)
    else:
        ego_flow = np.zeros((T, 3))
        for f in range(F):
            m = ids == f
            if m.any():
                ego = np.linalg.inv(pose1[f]) @ pose0[f]
                ego_flow[m] = pc[m, :3].astype(F64) @ ego[:3, :3].T + ego[:3, 3] - pc[m, :3]
        gt = (ego_flow + move).astype(F32)
        est = (move * 0.05 + rng.normal(0, 0.3, (T, 3))).astype(F32) if mode == MODE_COMPDIS else (ego_flow + move + rng.normal(0, 0.8, (T, 3))).astype(F32)
    d = make_data(c, offsets, pc, gt, est, dt, cat, inst, mask, LUT, pose0, pose1)
    d.name, d.pose_kinds = name, pose_kinds
    _BUILT[key] = d
    return d


# ---- the promises of the cases, proved with integer arithmetic -----------------------------------------------------------------------
def block_paths(offsets, total):
    """select_count_kernel / select_compact_kernel (:78-82, :132-135): which blocks lie inside one frame"""
    o, met = [int(v) for v in offsets], set()
    for bstart in range(0, total, SEL_BLOCK):
        bend = min(bstart + SEL_BLOCK, total)
        f0 = co.segment_of(o, bstart)
        met.add("uniform" if o[f0 + 1] >= bend else "straddling")
    return met


def table_occupancy(labs):
    """the slots the distinct labels of a frame end in (linear probing; the SET of occupied slots does not depend on the order)"""
    used = set()
    wrapped = False
    for lab in labs:
        h = int(rank_slot(np.uint64(lab)))
        while h in used:
            h += 1
            if h == RANK_SLOTS:
                h, wrapped = 0, True
        used.add(h)
    return used, wrapped


def promise(d, what):
    o, T = [int(v) for v in d.offsets], d.T
    rows, frame, group, id32 = select(d)
    per_frame = np.bincount(frame, minlength=d.F) if len(rows) else np.zeros(d.F, np.int64)
    labs = labels_of(frame, group, id32)
    distinct = {f: np.unique(labs[frame == f]) for f in np.unique(frame)}
    if what in ("uniform", "straddling"):
        return what in block_paths(o, T)
    if what == "lane_in_two_frames":                               # two selected points of one thread's four lie in different frames
        lane = rows // LANE_PTS
        both = np.nonzero(lane[1:] == lane[:-1])[0]
        return bool((frame[both + 1] != frame[both]).any())
    if what == "empty_frames":
        return 0 in d.sizes and T > 0 and len(rows) > 0
    if what == "unselected_frame_between":
        return any(d.sizes[f] > 0 and per_frame[f] == 0 and per_frame[:f].sum() > 0 and per_frame[f + 1:].sum() > 0 for f in range(d.F))
    if what.startswith("total:"):
        return T == int(what[6:])
    if what == "boundary_not_mult4":
        return any(0 < v < T and v % LANE_PTS for v in o[1:-1])
    if what == "frame_scan_carry":                                 # select_scan_kernel's second pass runs a second chunk, with a carry in it
        return d.F > SCAN_CHUNK and per_frame[:SCAN_CHUNK].sum() > 0 and per_frame[SCAN_CHUNK:].sum() > 0
    if what == "block_scan_carry":
        nblk = (T + SEL_BLOCK - 1) // SEL_BLOCK
        blk = rows // SEL_BLOCK
        return nblk > SCAN_CHUNK and bool((blk >= SCAN_CHUNK).any()) and bool((blk < SCAN_CHUNK).any()) and len(rows) <= 600
    if what.startswith("selected:"):
        return int(what[9:]) in per_frame.tolist()
    if what.startswith("labels:"):
        return int(what[7:]) in [len(v) for v in distinct.values()]
    if what == "table_path":
        return any(len(v) <= RANK_ADMIT for v in distinct.values())
    if what == "allpairs_path":
        return any(len(v) > RANK_ADMIT for v in distinct.values())
    if what == "records_gt_1024":
        return sum(len(v) for v in distinct.values()) > RED_GRID
    if what.startswith("records:"):
        return sum(len(v) for v in distinct.values()) == int(what[8:])
    if what == "scattered_tiles":                                  # a label with points in three tiles of its frame's selected points
        for f in distinct:
            m = np.nonzero(frame == f)[0]
            tile = np.arange(len(m)) // RANK_THREADS
            for lab in distinct[f]:
                if len(np.unique(tile[labs[m] == lab])) >= 3:
                    return True
        return False
    if what == "same_id_both_groups":
        return any(((group[frame == f] == 1) & (id32[frame == f] == 77)).any() and ((group[frame == f] == 2) & (id32[frame == f] == 77)).any() for f in distinct)
    if what == "same_id_two_frames":
        return len({int(f) for f in frame[(id32 == 77) & (group == 1)]}) >= 2
    if what == "edge_ids":
        return {0, 1, 1 << 31, (1 << 32) - 1} <= set(id32.tolist())
    if what == "id_mod_2_32":                                      # two ids that differ as int64 and agree in their low 32 bits, in one frame and group
        raw = d.inst[rows]
        k = {}
        for f, g, i, r in zip(frame.tolist(), group.tolist(), id32.tolist(), raw.tolist()):
            k.setdefault((f, g, i), set()).add(r)
        return any(len(v) > 1 for v in k.values())
    if what.startswith("shared_slot:"):
        n = int(what[12:])
        return any(np.bincount(rank_slot(v).astype(np.int64), minlength=RANK_SLOTS).max() >= n for v in distinct.values())
    if what == "chain_wraps":
        return any(table_occupancy(v.tolist())[1] for v in distinct.values() if len(v) <= RANK_ADMIT)
    if what.startswith("eval_launch:"):                            # nn_search_ranges(M, M, ...) at evalmetrics.hip:498-500
        return nn_launch(len(rows))[0] == what[12:]
    if what.startswith("seg_len:"):
        return int(what[8:]) in [len(p) for _, _, _, p in segments(d)[1]]
    if what == "extra_columns":
        return d.c["stride"] > 4 and bool((d.pc[rows, 3:] != 0).any())
    if what == "lut_byte_3":
        return bool((d.lut[d.cat[rows]] == 3).any())
    if what == "lut_byte_above_3":
        b = d.lut[d.cat[d.mask != 0]]
        return bool(((b > 3) & (b & 3 != 0)).any()) and bool(((b > 3) & (b & 3 == 0)).any())
    raise KeyError(what)


# ---- the search's matrix ------------------------------------------------------------------------------------------------------------
def _nn(nq, nr, promises, q_sizes=None, r_sizes=None, kind="random"):
    q_sizes, r_sizes = list(q_sizes or [nq]), list(r_sizes or [nr])
    assert sum(q_sizes) == nq and sum(r_sizes) == nr and len(q_sizes) == len(r_sizes)
    return dict(nq=nq, nr=nr, q_off=np.concatenate([[0], np.cumsum(q_sizes)]).astype(np.int64),
                r_off=np.concatenate([[0], np.cumsum(r_sizes)]).astype(np.int64), promises=tuple(promises), kind=kind)


def _make_nn_cases():
    C = {}
    for nq in (1, 15, 16, 17):
        for nr in (1, 15, 16, 17, 1023, 1024, 1025, 2049):
            C[f"q{nq}_r{nr}"] = _nn(nq, nr, ("launch:SPLIT16",) + (("tile_crossing",) if nr > NN_TILE else ()))
    for nq, shape in ((16128, "SPLIT16"), (16129, "SPLIT4"), (65280, "SPLIT4"), (65281, "QPT1")):
        C[f"q{nq}_r17"] = _nn(nq, 17, (f"launch:{shape}",))
        C[f"q{nq}_r1025"] = _nn(nq, 1025, (f"launch:{shape}", "tile_crossing"))
    for nq, shape in ((524032, "QPT1"), (524033, "QPT2")):
        C[f"q{nq}_r17"] = _nn(nq, 17, (f"launch:{shape}",) + (("last_block_partial",) if shape == "QPT2" else ()))
        # 1025 references: 700 queries search the first 1008 of them, the others the last 17; the block that holds query 700 holds both
        C[f"q{nq}_r1025_two_ranges"] = _nn(nq, 1025, (f"launch:{shape}", "tile_crossing", "segments_in_block"), [700, nq - 700], [1008, 17])
    C["segments_in_a_block"] = _nn(40, 90, ("launch:SPLIT16", "segments_in_block"), [3, 5, 1, 9, 22], [20, 1, 40, 9, 20])
    C["empty_reference_range"] = _nn(30, 50, ("launch:SPLIT16", "empty_r"), [10, 8, 12], [30, 0, 20])
    C["empty_query_range"] = _nn(30, 50, ("launch:SPLIT16", "empty_q"), [10, 0, 20], [20, 10, 20])
    C["ranges_far_apart"] = _nn(12, 3020, ("launch:SPLIT16", "far_ranges", "empty_q", "tile_crossing"), [5, 0, 7], [9, 2991, 20])
    C["no_references"] = _nn(20, 0, ("launch:SPLIT16", "empty_r"))
    for nq in (17, 20000, 70000):
        C[f"ties_q{nq}"] = _nn(nq, 2049, (f"launch:{nn_launch(nq)[0]}", "ties"), kind="ties")
    C["nan_query_and_reference"] = _nn(40, 300, ("launch:SPLIT16", "nan"), kind="nan")
    return C


NN_CASES = _make_nn_cases()
NN_CASE_NAMES = tuple(NN_CASES)
TIE_ROWS = ((1023, 1024), (5, 22, 39), (40, 2048))                                 # rows that hold the same point; the first is the lowest
TIE_POINTS = ((0, 0, 0), (100, 0, 0), (0, 100, 0))
NAN_QUERY, NAN_REFERENCE = 7, 11


def nn_build(name, f64):
    """(q [nq, 3], r [nr, 3]) of the search's dtype"""
    c = NN_CASES[name]
    rng = np.random.default_rng(7000 + NN_CASE_NAMES.index(name))
    T = F64 if f64 else F32
    nq, nr = c["nq"], c["nr"]
    if c["kind"] == "ties":
        # integer lattice: every difference, product and sum is exact in float32, so both dtypes return the same bits and the
        # candidates that hold the same point tie exactly
        r = rng.integers(200, 1000, (nr, 3)).astype(T)
        for rows, pt in zip(TIE_ROWS, TIE_POINTS):
            r[list(rows)] = np.array(pt, T)
        which = np.arange(nq) % 3
        q = (np.array(TIE_POINTS, np.int64)[which] + rng.integers(-3, 4, (nq, 3))).astype(T)
        return q, r
    if f64:
        q, r = rng.normal(size=(nq, 3)) * 5, rng.normal(size=(nr, 3)) * 5
    else:
        q, r = rng.uniform(-50, 50, (nq, 3)).astype(F32), rng.uniform(-50, 50, (nr, 3)).astype(F32)
    if c["kind"] == "nan":
        q[NAN_QUERY, 1] = np.nan
        r[NAN_REFERENCE, 2] = np.nan
        q[3] = r[NAN_REFERENCE]                                   # the query that would match it
        q[3, 2] = 0.0
    return np.ascontiguousarray(q, T), np.ascontiguousarray(r, T)


def nn_promise(name, what):
    c = NN_CASES[name]
    nq, q_off, r_off = c["nq"], c["q_off"], c["r_off"]
    shape, qpb = nn_launch(nq)

    def unions():                                                # per block: the segments of its queries and the union of their ranges
        seg = np.searchsorted(q_off, np.arange(nq), side="right") - 1
        nonempty = r_off[seg + 1] > r_off[seg]
        for b in range(0, nq, qpb):
            s = seg[b:b + qpb][nonempty[b:b + qpb]]
            if len(s):
                yield np.unique(s), int(r_off[s].min()), int(r_off[s + 1].max())
    if what.startswith("launch:"):
        return shape == what[7:]
    if what == "last_block_partial":
        return nq % qpb != 0
    if what == "tile_crossing":
        return any(hi - lo > NN_TILE for _, lo, hi in unions())
    if what == "segments_in_block":
        return any(len(s) > 1 for s, _, _ in unions())
    if what == "far_ranges":                                     # the union of a block holds a tile no query of the block reads
        return any(len(s) > 1 and hi - lo > sum(int(r_off[k + 1] - r_off[k]) for k in s) + NN_TILE for s, lo, hi in unions())
    if what == "empty_r":
        return bool(((np.diff(r_off) == 0) & (np.diff(q_off) > 0)).any())
    if what == "empty_q":
        return bool(((np.diff(q_off) == 0) & (np.diff(r_off) > 0)).any())
    if what == "ties":                                           # equal candidates in different lanes of a SPLIT group, and on both sides of the tile boundary
        split = {"SPLIT16": 16, "SPLIT4": 4}.get(shape, 1)
        lanes_differ = split == 1 or len({r % split for r in TIE_ROWS[1]}) == len(TIE_ROWS[1])
        return lanes_differ and TIE_ROWS[0] == (NN_TILE - 1, NN_TILE) and TIE_ROWS[2][1] // NN_TILE == 2 and len(q_off) == 2
    if what == "nan":
        q, r = nn_build(name, True)
        return bool(np.isnan(q[NAN_QUERY]).any()) and bool(np.isnan(r[NAN_REFERENCE]).any()) and int(np.isnan(q).any(1).sum()) == 1
    raise KeyError(what)
