"""The restatement of "box evaluation, v1" (the rule is the module docstring of himo_amd/eval_box.py): rules A-G in plain Python
float64, in the rule's operation order, one operation a line where the order matters.  The kernels (himo_amd/csrc/boxeval.hip) are
compared with it bit for bit (tests/test_box_eval_gpu.py); it is itself checked against exact rational arithmetic and against exact
expectations (tests/test_box_eval_cpu.py).  Rule D is the plain sequential greedy: sort the candidates, walk them once.

How good the intersection area is (tests/test_box_eval_cpu.py::test_intersection_area_against_exact_rational_arithmetic): ``clip`` on
``fractions.Fraction`` over the same float64 corners is the exact area of the intersection of the two quadrilaterals.  Over 4000 seeded
pairs (centres within 3 m of each other, l in 0.3..6, w in 0.3..3, any yaw; 2356 of them intersect) the greatest absolute difference
measured is 2.95e-15 m^2 with the pairs about the origin and 1.11e-14 m^2 with the same pairs shifted to (45, -45) m (3.8 x).  Rule B1
takes the translation out: over the pairs that rule B6 does not clamp the two figures are 2.94e-15 and 2.33e-15 m^2.  The larger figure at
45 m belongs to boxes that lie inside their partner: there the corners are rounded to 7e-15 m, the quadrilateral they name differs from
``l * w`` by about 1e-14 m^2, and rule B6 clamps the clipped area to ``l * w``.  The test asserts ``AREA_BOUND`` = 16 x the maximum measured
about the origin = 4.72e-14 m^2 on both sets -- the headroom for other draws on the same operation count -- and that the shifted set is
no more than 4 x worse than the unshifted one, over all pairs and over the unclamped ones.  ``clip(A, B)`` and ``clip(B, A)`` differ by
3.6e-15 m^2 at the most on the same pairs.
"""
import math
from fractions import Fraction

import numpy as np

MAX_BOXES = 1024
TAUS = (0.3, 0.5, 0.7)
AREA_MEASURED = 2.95e-15           # m^2: the greatest |restatement - exact| over the case set about the origin (see above)
AREA_BOUND = 16 * AREA_MEASURED


# ---- rule A ---------------------------------------------------------------------------------------------------------------------------------
def rect(row):
    """one box row (float32 in the stored layout; whatever it is, widened to float64) -> the twelve floats of its rect (twelve NaN: INVALID)"""
    x, y, z, l, w, h, yaw = (float(v) for v in row[:7])
    if not all(math.isfinite(v) for v in (x, y, z, l, w, h, yaw)) or l < 0 or w < 0 or h < 0:
        return [math.nan] * 12
    c, s = math.cos(yaw), math.sin(yaw)
    hl, hw = l * 0.5, w * 0.5
    out = []
    for dx, dy in ((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw)):
        out += [x + (dx * c - dy * s), y + (dx * s + dy * c)]
    out += [z - h * 0.5, z + h * 0.5, l * w, 0.0]
    return out if all(math.isfinite(v) for v in out) else [math.nan] * 12


def rects(rows):
    rows = np.asarray(rows)
    return np.array([rect(r) for r in rows], dtype=np.float64).reshape(-1, 12)


def valid(r):
    return all(math.isfinite(float(v)) for v in r) and r[10] >= 0 and r[9] >= r[8]


# ---- rule B ---------------------------------------------------------------------------------------------------------------------------------
def clip(P, Q, half=0.5):
    """rules B3-B6 without the clamp: the subject polygon P (four (x, y)) clipped by the edges of Q in order, then the fan area.
    Works on floats (the rule) and on Fractions (the exact area: ``half=Fraction(1, 2)``)."""
    V = list(P)
    for e in range(4):
        px, py = Q[e]
        qx, qy = Q[(e + 1) % 4]
        ex = qx - px
        ey = qy - py
        d = []
        for vx, vy in V:
            a = vy - py
            b = vx - px
            d.append(ex * a - ey * b)
        out, n, most = [], len(V), 5 + e
        for m in range(n):
            sx, sy = V[m]
            tx, ty = V[(m + 1) % n]
            ds, de = d[m], d[(m + 1) % n]
            ins, ine = ds >= 0, de >= 0
            if ins and len(out) < most:
                out.append((sx, sy))
            if ins != ine and len(out) < most:
                t = ds / (ds - de)
                out.append((sx + t * (tx - sx), sy + t * (ty - sy)))
        V = out
    if len(V) < 3:
        return half * 0
    x0, y0 = V[0]
    acc = half * 0
    for m in range(1, len(V) - 1):
        acc = acc + ((V[m][0] - x0) * (V[m + 1][1] - y0) - (V[m + 1][0] - x0) * (V[m][1] - y0))
    return half * acc


def relative(ra, rb):
    """rule B1: (P, Q), the corners of A and of B relative to A's corner 0"""
    ox, oy = float(ra[0]), float(ra[1])
    P = [(float(ra[2 * k]) - ox, float(ra[2 * k + 1]) - oy) for k in range(4)]
    Q = [(float(rb[2 * k]) - ox, float(rb[2 * k + 1]) - oy) for k in range(4)]
    return P, Q


def disjoint(P, Q):
    """rule B2"""
    axl, axh = min(p[0] for p in P), max(p[0] for p in P)
    ayl, ayh = min(p[1] for p in P), max(p[1] for p in P)
    bxl, bxh = min(p[0] for p in Q), max(p[0] for p in Q)
    byl, byh = min(p[1] for p in Q), max(p[1] for p in Q)
    return axh < bxl or bxh < axl or ayh < byl or byh < ayl


def inter_area(ra, rb):
    """rule B on two rects: the clamped intersection area (0 for an INVALID rect)"""
    if not (valid(ra) and valid(rb)):
        return 0.0
    P, Q = relative(ra, rb)
    if disjoint(P, Q):
        return 0.0
    inter = clip(P, Q)
    lim = float(ra[10]) if ra[10] < rb[10] else float(rb[10])
    if not inter >= 0.0:
        inter = 0.0
    if inter > lim:
        inter = lim
    return inter


def exact_area(ra, rb):
    """the exact area of the intersection of the two quadrilaterals the rects' float64 corners name"""
    P = [(Fraction(float(ra[2 * k])), Fraction(float(ra[2 * k + 1]))) for k in range(4)]
    Q = [(Fraction(float(rb[2 * k])), Fraction(float(rb[2 * k + 1]))) for k in range(4)]
    return clip(P, Q, Fraction(1, 2))


# ---- rule C ---------------------------------------------------------------------------------------------------------------------------------
def pair_iou(ra, rb):
    """(iou, iou3) of two rects"""
    if not (valid(ra) and valid(rb)):
        return 0.0, 0.0
    inter = inter_area(ra, rb)
    aa, ab = float(ra[10]), float(rb[10])
    union = (aa + ab) - inter
    iou = inter / union if union > 0.0 else 0.0
    top = float(ra[9]) if ra[9] < rb[9] else float(rb[9])
    bot = float(ra[8]) if ra[8] > rb[8] else float(rb[8])
    dz = top - bot
    hz = dz if dz > 0.0 else 0.0
    inter3 = inter * hz
    den = (aa * (float(ra[9]) - float(ra[8])) + ab * (float(rb[9]) - float(rb[8]))) - inter3
    iou3 = inter3 / den if den > 0.0 else 0.0
    return iou, iou3


def iou_matrix(RA, RB):
    """(iou, iou3) float64 [Fa, Fb] each.  Rule B2 is evaluated for the whole matrix at once with numpy (the same subtractions and
    comparisons, element by element); only the pairs it lets through are clipped, one at a time."""
    RA, RB = np.asarray(RA, dtype=np.float64).reshape(-1, 12), np.asarray(RB, dtype=np.float64).reshape(-1, 12)
    Fa, Fb = len(RA), len(RB)
    iou, iou3 = np.zeros((Fa, Fb)), np.zeros((Fa, Fb))
    if not (Fa and Fb):
        return iou, iou3
    with np.errstate(all="ignore"):
        ok = np.array([valid(r) for r in RA])[:, None] & np.array([valid(r) for r in RB])[None, :]
        ax = RA[:, 0:8:2] - RA[:, 0:1]                                          # [Fa, 4]
        ay = RA[:, 1:8:2] - RA[:, 1:2]
        bx = RB[None, :, 0:8:2] - RA[:, None, 0:1]                              # [Fa, Fb, 4]
        by = RB[None, :, 1:8:2] - RA[:, None, 1:2]
        apart = (ax.max(1)[:, None] < bx.min(2)) | (bx.max(2) < ax.min(1)[:, None]) | (ay.max(1)[:, None] < by.min(2)) | (by.max(2) < ay.min(1)[:, None])
    for i, j in zip(*np.nonzero(ok & ~apart)):
        iou[i, j], iou3[i, j] = pair_iou(RA[i], RB[j])
    return iou, iou3


# ---- rule D ---------------------------------------------------------------------------------------------------------------------------------
def greedy(iou, min_iou=0.1):
    """the sequential greedy on a matrix of BEV IoUs: (match_a int32 [Fa], match_b int32 [Fb])"""
    iou = np.asarray(iou, dtype=np.float64)
    Fa, Fb = iou.shape
    cand = [(-float(iou[i, j]), int(i), int(j)) for i, j in zip(*np.nonzero(iou >= min_iou))]
    cand.sort()
    ma, mb = np.full(Fa, -1, np.int32), np.full(Fb, -1, np.int32)
    for _, i, j in cand:
        if ma[i] < 0 and mb[j] < 0:
            ma[i], mb[j] = j, i
    return ma, mb


def match_rects(RA, RB, min_iou=0.1):
    """one sweep: (match_a, match_b, iou_a float64 [Fa, 2])"""
    RA, RB = np.asarray(RA).reshape(-1, 12), np.asarray(RB).reshape(-1, 12)
    if len(RA) > MAX_BOXES or len(RB) > MAX_BOXES:
        raise ValueError("a sweep above the cap")
    iou, iou3 = iou_matrix(RA, RB)
    ma, mb = greedy(iou, min_iou)
    iou_a = np.zeros((len(RA), 2))
    for i in np.flatnonzero(ma >= 0):
        iou_a[i] = iou[i, ma[i]], iou3[i, ma[i]]
    return ma, mb, iou_a


def match(rows_a, rows_b, min_iou=0.1):
    return match_rects(rects(rows_a), rects(rows_b), min_iou)


def iou_pairs(rows_a, rows_b, pairs):
    """rule G's numbers: float64 [n, 2]; an index outside its table gives zeros"""
    RA, RB = rects(rows_a), rects(rows_b)
    out = np.zeros((len(pairs), 2))
    for n, (i, j) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)):
        if 0 <= i < len(RA) and 0 <= j < len(RB):
            out[n] = pair_iou(RA[i], RB[j])
    return out


# ---- rules F and G --------------------------------------------------------------------------------------------------------------------------
def speed_bucket(v, motion_min=0.05, sensor_dt=0.1):
    if v < motion_min / sensor_dt:
        return "static"
    if v < 10.0:
        return "0-10"
    if v < 20.0:
        return "10-20"
    return "20-30" if v < 30.0 else "30+"


def range_bucket(r):
    if r < 10.0:
        return "0-10"
    if r < 20.0:
        return "10-20"
    return "20-30" if r < 30.0 else "30+"


BUCKETS = ["all"] + ["speed " + b for b in ("static", "0-10", "10-20", "20-30", "30+")] + ["range " + b for b in ("0-10", "10-20", "20-30", "30+")]


def score(sweeps, pair_by="iou", motion_min=0.05, sensor_dt=0.1):
    """Rule F (and G) for one result name in one pass over ``sweeps`` = [(rows_gt, rows_pred, match_gt, iou_gt)]: the dictionary
    ``eval_box.summary`` gives for that name."""
    pred = 0
    rec = {k: {"gt": 0, "iou": [], "iou3": [], "dl": [], "dw": [], "centre": [], "yaw": []} for k in BUCKETS}
    for rows_gt, rows_pred, match_gt, iou_gt in sweeps:
        pred += len(rows_pred)
        for i, g in enumerate(np.asarray(rows_gt, dtype=np.float64)):
            keys = ("all", "speed " + speed_bucket(math.hypot(g[7], g[8]), motion_min, sensor_dt), "range " + range_bucket(math.hypot(g[0], g[1])))
            for k in keys:
                rec[k]["gt"] += 1
            if match_gt[i] < 0:
                continue
            p = np.asarray(rows_pred, dtype=np.float64)[match_gt[i]]
            fold = abs(math.degrees(g[6] - p[6])) % 90.0
            for k in keys:
                r = rec[k]
                r["iou"].append(float(iou_gt[i][0]))
                r["iou3"].append(float(iou_gt[i][1]))
                r["dl"].append(abs(g[3] - p[3]))
                r["dw"].append(abs(g[4] - p[4]))
                r["centre"].append(math.hypot(g[0] - p[0], g[1] - p[1]))
                r["yaw"].append(min(fold, 90.0 - fold))
    mean = lambda v: sum(v) / len(v) if v else None                # noqa: E731
    div = lambda a, b: a / b if b else None                         # noqa: E731
    out = {"pred": pred, "buckets": {}}
    for k in BUCKETS:
        r = rec[k]
        b = {"gt": r["gt"], "pairs": len(r["iou"]), "mean_iou": mean(r["iou"]), "mean_iou3": mean(r["iou3"]), "mean_dl": mean(r["dl"]),
             "mean_dw": mean(r["dw"]), "mean_centre": mean(r["centre"]), "mean_yaw_deg": mean(r["yaw"])}
        if pair_by == "iou":
            b["at"] = {}
            for tau in TAUS:
                tp = sum(1 for v in r["iou"] if v >= tau)
                fn = r["gt"] - tp
                at = {"tp": tp, "fn": fn, "recall": div(tp, tp + fn)}
                if k == "all":
                    fp = pred - tp
                    p_, r_ = div(tp, tp + fp), at["recall"]
                    at.update(fp=fp, precision=p_, f1=None if p_ is None or r_ is None or p_ + r_ == 0 else 2 * p_ * r_ / (p_ + r_))
                b["at"][f"{tau:g}"] = at
        out["buckets"][k] = b
    return out


# ---- shared case builders -------------------------------------------------------------------------------------------------------------------
def box_rows(centres, sizes, yaws, z=0.5, h=1.6, vel=None, ids=None):
    """float32 [F, 12] rows in ``box_fit``'s layout"""
    centres, sizes, yaws = np.asarray(centres, dtype=np.float64).reshape(-1, 2), np.asarray(sizes, dtype=np.float64).reshape(-1, 2), np.asarray(yaws, dtype=np.float64).reshape(-1)
    F = len(centres)
    rows = np.zeros((F, 12), dtype=np.float32)
    rows[:, 0:2], rows[:, 2], rows[:, 3:5], rows[:, 5], rows[:, 6] = centres, z, sizes, h, yaws
    if vel is not None:
        rows[:, 7:9] = np.asarray(vel).reshape(F, 2)
    rows[:, 10] = np.arange(1, F + 1) if ids is None else ids
    rows[:, 11] = 50
    return rows


def jittered_sweep(rng, F, extra=0.2, spacing=8.0):
    """F boxes on a jittered grid and their jittered copies (centre +-0.3 m, yaw +-5 degrees, a third of them stretched by up to 3 m along
    the heading), plus ``extra`` x F boxes on each side that overlap nothing: (rows_a, rows_b), each in random order"""
    side = max(1, int(math.ceil(math.sqrt(F))))
    k = np.arange(F)
    centres = np.stack([(k % side - side / 2) * spacing, (k // side - side / 2) * spacing], axis=1) + rng.uniform(-1.0, 1.0, (F, 2))
    sizes = np.stack([rng.uniform(3.5, 5.5, F), rng.uniform(1.6, 2.2, F)], axis=1)
    yaws = rng.uniform(-math.pi, math.pi, F)
    vel = rng.uniform(-1, 1, (F, 2)) * rng.choice([0.0, 5.0, 15.0, 25.0, 40.0], (F, 1))
    a = box_rows(centres, sizes, yaws, vel=vel)
    stretch = np.where(rng.uniform(0, 1, F) < 1 / 3, rng.uniform(0, 3.0, F), 0.0)
    yb = yaws + np.radians(rng.uniform(-5, 5, F))
    cb = centres + rng.uniform(-0.3, 0.3, (F, 2)) + 0.5 * stretch[:, None] * np.stack([np.cos(yaws), np.sin(yaws)], axis=1)
    b = box_rows(cb, sizes + np.stack([stretch, np.zeros(F)], axis=1), yb, vel=vel)
    n_extra = int(round(extra * F))
    far = lambda off: box_rows(np.stack([(np.arange(n_extra) - n_extra / 2) * spacing, np.full(n_extra, off)], axis=1) + rng.uniform(-1, 1, (n_extra, 2)),      # noqa: E731
                               np.tile([4.0, 1.8], (n_extra, 1)), rng.uniform(-math.pi, math.pi, n_extra), ids=np.arange(n_extra) + 100000 + int(off))
    lim = (side / 2 + 2) * spacing
    a, b = np.concatenate([a, far(lim)]), np.concatenate([b, far(-lim - spacing)])
    return a[rng.permutation(len(a))], b[rng.permutation(len(b))]


def chain(n=140, yaw=0.37, through=(30.0, -20.0), size=(4.0, 2.0)):
    """n boxes of ``size`` along a line at ``yaw`` through ``through``, alternating between A and B; consecutive overlaps are 1.9 - 0.01 k
    metres: (rows_a, rows_b).  A(i) overlaps B(i) more than B(i) overlaps A(i + 1), and so on down the line."""
    pos, s = [], 0.0
    for k in range(n):
        pos.append(s)
        s += size[0] - (1.9 - 0.01 * k)
    pos = np.asarray(pos) - pos[n // 2]
    centres = np.asarray(through)[None, :] + pos[:, None] * np.array([math.cos(yaw), math.sin(yaw)])[None, :]
    rows = box_rows(centres, np.tile(size, (n, 1)), np.full(n, yaw))
    return rows[0::2].copy(), rows[1::2].copy()
