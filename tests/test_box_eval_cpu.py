"""Box evaluation without a GPU: the restatement (tests/boxeval_ref.py) against exact rational arithmetic and exact expectations, the
sequential greedy of rule D against rounds of locally dominant pairs, the host glue of rules F and G, the binding's declarations and
the program's refusals.  The kernels themselves: tests/test_box_eval_gpu.py."""
import ctypes
import functools
import math
import re
from fractions import Fraction

import numpy as np
import pytest

import boxeval_ref as ref
from conftest import REPO


def one(cx, cy, l, w, yaw, z=0.5, h=1.6):
    """the rect of one box given in float64 (a float32 row cannot hold pi / 2)"""
    return ref.rects(np.array([[cx, cy, z, l, w, h, yaw]], dtype=np.float64))[0]


# ---- the restatement's area against exact rational arithmetic --------------------------------------------------------------------------------
def case_set(shift):
    """4000 seeded pairs: centres within +-3 m of each other, l in 0.3..6, w in 0.3..3, any yaw; the whole set moved by ``shift``"""
    rng = np.random.default_rng(2024)
    n = 4000
    ca = rng.uniform(-1.5, 1.5, (n, 2))
    cb = ca + rng.uniform(-3, 3, (n, 2))
    sa = np.stack([rng.uniform(0.3, 6, n), rng.uniform(0.3, 3, n)], 1)
    sb = np.stack([rng.uniform(0.3, 6, n), rng.uniform(0.3, 3, n)], 1)
    ya, yb = rng.uniform(-math.pi, math.pi, n), rng.uniform(-math.pi, math.pi, n)
    shift = np.asarray(shift, dtype=np.float64)
    return ref.rects(ref.box_rows(ca + shift, sa, ya)), ref.rects(ref.box_rows(cb + shift, sb, yb))


@functools.lru_cache(maxsize=None)
def area_errors(shift):
    """(greatest |restatement - exact|, the same over the pairs rule B6 does not clamp, greatest |clip(A, B) - clip(B, A)|, pairs that
    intersect) over the case set"""
    RA, RB = case_set(shift)
    worst, unclamped, order, hit = 0.0, 0.0, 0.0, 0
    for a, b in zip(RA, RB):
        got = ref.inter_area(a, b)
        err = float(abs(Fraction(got) - ref.exact_area(a, b)))
        worst = max(worst, err)
        if got != min(a[10], b[10]):
            unclamped = max(unclamped, err)
        order = max(order, abs(got - ref.inter_area(b, a)))
        hit += got > 0
    return worst, unclamped, order, hit


def test_intersection_area_against_exact_rational_arithmetic():
    here, free, order, hit = area_errors((0.0, 0.0))
    there, free_there, order_there, hit_there = area_errors((45.0, -45.0))
    print(f"max |area - exact|: {here:.3g} m^2 about the origin, {there:.3g} m^2 at (45, -45) (unclamped pairs: {free:.3g}, {free_there:.3g}); "
          f"bound {ref.AREA_BOUND:.3g}; "
          f"max |clip(A, B) - clip(B, A)|: {order:.3g}, {order_there:.3g}; {hit} and {hit_there} of 4000 pairs intersect")
    assert hit > 2000 and hit_there > 2000                         # the set is about intersecting pairs
    assert ref.AREA_BOUND == 16 * ref.AREA_MEASURED and here <= ref.AREA_MEASURED * 1.001      # the docstring's figure is this run's
    assert here <= ref.AREA_BOUND and there <= ref.AREA_BOUND
    assert there <= 4 * here and free_there <= 4 * free              # rule B1 does its job
    assert order <= ref.AREA_BOUND and order_there <= ref.AREA_BOUND


# ---- exact expectations ------------------------------------------------------------------------------------------------------------------------
def test_exact_expectations():
    big = one(0, 0, 4, 2, 0.0)
    assert ref.pair_iou(big, big)[0] == 1.0 and ref.pair_iou(big, big)[1] == 1.0
    assert ref.pair_iou(big, one(4, 0, 4, 2, 0.0)) == (0.0, 0.0)                            # a shared edge
    assert ref.pair_iou(big, one(4, 2, 4, 2, 0.0)) == (0.0, 0.0)                            # touching at a corner
    assert ref.pair_iou(big, one(0.5, 0.25, 1, 0.5, 0.0))[0] == 0.0625                      # inside
    assert ref.pair_iou(one(0.5, 0.25, 1, 0.5, 0.0), big)[0] == 0.0625
    assert abs(ref.pair_iou(big, one(0, 0, 2, 4, math.pi / 2))[0] - 1.0) <= 1e-15           # the same rectangle, named the other way
    assert ref.pair_iou(big, one(2, 0, 4, 2, 0.0))[0] == 1.0 / 3.0                          # a half-length shift
    assert ref.pair_iou(big, one(0, 0, 4, 0, 0.0)) == (0.0, 0.0)                            # zero width
    assert ref.pair_iou(one(0, 0, 0, 0, 0.0), one(0, 0, 0, 0, 0.0)) == (0.0, 0.0)
    # z: half the height shared -> inter3 = 8 * 0.8, den = 2 * 8 * 1.6 - 6.4; disjoint in z -> iou3 0 while iou is 1
    assert ref.pair_iou(big, one(0, 0, 4, 2, 0.0, z=1.3))[1] == pytest.approx(6.4 / 19.2, rel=1e-15)
    assert ref.pair_iou(big, one(0, 0, 4, 2, 0.0, z=5.0)) == (1.0, 0.0)


def test_invalid_rects_give_zero_and_stay_unmatched():
    good = ref.box_rows([[0, 0], [10, 0]], [[4, 2], [4, 2]], [0.1, 0.2])
    bad = good.copy()
    bad[0, 3] = -1.0                                                # l < 0
    bad = np.concatenate([bad, good[:1], good[:1], good[:1]])
    bad[2, 0], bad[3, 5], bad[4, 6] = np.nan, -0.5, np.inf          # x not finite, h < 0, yaw not finite
    R = ref.rects(bad)
    assert np.isnan(R[[0, 2, 3, 4]]).all() and np.isfinite(R[1]).all()
    ma, mb, iou_a = ref.match(good, bad)
    assert ma.tolist() == [-1, 1] and mb.tolist() == [-1, 1, -1, -1, -1] and iou_a[0].tolist() == [0.0, 0.0] and iou_a[1, 0] == 1.0
    assert ref.pair_iou(R[0], R[1]) == (0.0, 0.0) and ref.pair_iou(R[1], R[2]) == (0.0, 0.0)


def test_rects_corner_order_and_z_range():
    from himo_amd import eval_box
    rows = ref.box_rows([[1, 2], [-3, 4], [45, -45]], [[4, 2], [0, 0], [5.5, 2.5]], [0.0, 1.0, -2.5], z=0.25, h=1.5)
    R = eval_box.rects(rows)
    assert R.dtype == np.float64 and R.shape == (3, 12)
    assert R.tobytes() == ref.rects(rows).tobytes()                 # the binding's rule A is the restatement's, bit for bit
    assert R[0].tolist() == [3.0, 3.0, -1.0, 3.0, -1.0, 1.0, 3.0, 1.0, -0.5, 1.0, 8.0, 0.0]      # from (+l/2, +w/2), counter-clockwise
    assert R[1, :8].tolist() == [-3.0, 4.0] * 4 and R[1, 10] == 0.0
    x, y = R[2, 0:8:2], R[2, 1:8:2]
    assert 0.5 * sum(x[k] * y[(k + 1) % 4] - x[(k + 1) % 4] * y[k] for k in range(4)) == pytest.approx(5.5 * 2.5, rel=1e-13)      # > 0: ccw
    bad = rows.copy()
    bad[1, 4] = -0.0                                                # -0 is not < 0
    bad[2, 4] = -1e-3
    assert np.isfinite(eval_box.rects(bad)[1]).all() and np.isnan(eval_box.rects(bad)[2]).all()
    assert eval_box.rects(np.zeros((0, 12), np.float32)).shape == (0, 12)
    with pytest.raises(ValueError):
        eval_box.rects(np.zeros((3, 6), np.float32))


# ---- rule D -------------------------------------------------------------------------------------------------------------------------------------
def locally_dominant(iou, min_iou):
    """rounds of locally dominant pairs -- the kernel's form of rule D, restated here to be held against the sequential greedy:
    (match_a, match_b, rounds that kept a pair)"""
    iou = np.asarray(iou, dtype=np.float64)
    Fa, Fb = iou.shape
    ma, mb, rounds = np.full(Fa, -1, np.int32), np.full(Fb, -1, np.int32), 0
    for _ in range(min(Fa, Fb) + 1):
        free = np.where((ma[:, None] < 0) & (mb[None, :] < 0) & (iou >= min_iou), iou, -1.0)
        keep = []
        for i in range(Fa):
            if free[i].max(initial=-1.0) < 0:
                continue
            j = int(np.argmax(free[i]))                             # the greatest, then the lowest j
            if int(np.argmax(free[:, j])) == i:                     # ... and the greatest of its column, then the lowest i
                keep.append((i, j))
        if not keep:
            break
        rounds += 1
        for i, j in keep:
            ma[i], mb[j] = j, i
    return ma, mb, rounds


def test_duplicates_match_in_order():
    for k in (1, 2, 8):
        rows = ref.box_rows(np.tile([[3.0, -2.0]], (k, 1)), np.tile([[4.0, 2.0]], (k, 1)), np.full(k, 0.3))
        ma, mb, iou_a = ref.match(rows, rows)
        assert ma.tolist() == list(range(k)) and mb.tolist() == list(range(k)) and (iou_a[:, 0] == iou_a[0, 0]).all() and iou_a[0, 0] > 0.999999


def test_greedy_equals_rounds_of_locally_dominant_pairs_under_ties():
    rng = np.random.default_rng(5)
    for n in range(200):
        Fa, Fb = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        iou = rng.choice([0.0, 0.05, 0.1, 0.3, 0.3, 0.5, 0.7, 1.0], (Fa, Fb))      # a handful of values: ties everywhere
        for min_iou in (0.1, 0.5):
            ma, mb = ref.greedy(iou, min_iou)
            la, lb, _ = locally_dominant(iou, min_iou)
            assert ma.tolist() == la.tolist() and mb.tolist() == lb.tolist(), (n, iou)
            kept = np.flatnonzero(ma >= 0)
            assert (iou[kept, ma[kept]] >= min_iou).all() and sorted(ma[kept].tolist()) == sorted(set(ma[kept].tolist()))
    # the matching at a threshold is the subset of the matching at min_iou
    iou = rng.choice([0.0, 0.2, 0.4, 0.6, 0.8], (12, 9))
    low, _ = ref.greedy(iou, 0.1)
    high, _ = ref.greedy(iou, 0.5)
    assert high.tolist() == [j if j >= 0 and iou[i, j] >= 0.5 else -1 for i, j in enumerate(low.tolist())]


def test_the_chain_needs_many_rounds():
    rows_a, rows_b = ref.chain()
    assert len(rows_a) == len(rows_b) == 70
    iou, _ = ref.iou_matrix(ref.rects(rows_a), ref.rects(rows_b))
    ma, mb = ref.greedy(iou, 0.05)
    assert ma.tolist() == list(range(70)) and mb.tolist() == list(range(70))
    la, lb, rounds = locally_dominant(iou, 0.05)
    assert la.tolist() == ma.tolist() and lb.tolist() == mb.tolist()
    print(f"the chain: {rounds} rounds of locally dominant pairs")
    assert 65 <= rounds <= 71


# ---- rules F and G --------------------------------------------------------------------------------------------------------------------------------
def test_bucket_edges():
    from himo_amd import eval_box
    edge = 0.05 / 0.1
    for v, want in ((0.0, "static"), (np.nextafter(edge, 0), "static"), (edge, "0-10"), (np.nextafter(10.0, 0), "0-10"), (10.0, "10-20"),
                    (np.nextafter(20.0, 0), "10-20"), (20.0, "20-30"), (np.nextafter(30.0, 0), "20-30"), (30.0, "30+"), (1e9, "30+")):
        assert eval_box.speed_bucket(float(v)) == ref.speed_bucket(float(v)) == want, v
    assert eval_box.speed_bucket(0.9, motion_min=0.1) == "static" and eval_box.speed_bucket(1.0, motion_min=0.1) == "0-10"
    for r, want in ((0.0, "0-10"), (10.0, "10-20"), (np.nextafter(10.0, 0), "0-10"), (20.0, "20-30"), (30.0, "30+"), (29.999, "20-30")):
        assert eval_box.range_bucket(float(r)) == ref.range_bucket(float(r)) == want, r
    assert eval_box.bucket_keys() == ref.BUCKETS


def glue_case(seed):
    rng = np.random.default_rng(seed)
    sweeps = []
    for _ in range(3):
        a, b = ref.jittered_sweep(rng, 30)
        ma, mb, iou_a = ref.match(a, b)
        sweeps.append((a, b, ma, iou_a))
    return sweeps


def same_numbers(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (a.keys(), b.keys())
        for k in a:
            same_numbers(a[k], b[k])
    elif a is None or b is None or isinstance(a, int):
        assert a == b and type(a) is type(b)
    else:
        assert a == pytest.approx(b, rel=1e-12, abs=1e-15)


def test_host_glue_is_the_restatements_and_ranks_merge():
    from himo_amd import eval_box
    sweeps = glue_case(7)
    sums = {"x": eval_box.new_sums()}
    for s in sweeps:
        eval_box.tally(sums["x"], *s)
    got = eval_box.summary(sums)["x"]
    want = ref.score(sweeps)
    same_numbers(got, want)
    a = got["buckets"]["all"]
    assert a["gt"] == 3 * 36 and got["pred"] == 3 * 36 and 60 <= a["pairs"] <= 90 and a["at"]["0.3"]["tp"] >= a["at"]["0.5"]["tp"] >= a["at"]["0.7"]["tp"] > 0
    # FP in "all" only; the buckets partition the ground truth twice
    assert a["at"]["0.5"]["fp"] == got["pred"] - a["at"]["0.5"]["tp"]
    assert all("fp" not in b["at"]["0.5"] for k, b in got["buckets"].items() if k != "all")
    for kind in ("speed", "range"):
        assert sum(b["gt"] for k, b in got["buckets"].items() if k.startswith(kind)) == a["gt"]
        assert sum(b["at"]["0.5"]["tp"] for k, b in got["buckets"].items() if k.startswith(kind)) == a["at"]["0.5"]["tp"]
    # two ranks' sums merged equal one pass
    parts = [{"x": eval_box.new_sums()}, {"x": eval_box.new_sums()}]
    for n, s in enumerate(sweeps):
        eval_box.tally(parts[n % 2]["x"], *s)
    from himo_amd import distenv
    same_numbers(eval_box.summary(distenv.add_sums(*parts))["x"], got)
    # rule G: given pairs, no TP / FP / FN
    labelled = eval_box.summary(sums, "label")["x"]
    assert "at" not in labelled["buckets"]["all"] and labelled["buckets"]["all"]["mean_iou"] == a["mean_iou"]
    same_numbers(labelled, ref.score(sweeps, "label"))


def test_zero_denominators_come_out_as_none():
    from himo_amd import eval_box
    empty = eval_box.summary({"x": eval_box.new_sums()})["x"]["buckets"]["all"]
    assert empty["mean_iou"] is None and empty["mean_dl"] is None
    assert empty["at"]["0.5"] == {"tp": 0, "fn": 0, "recall": None, "fp": 0, "precision": None, "f1": None}
    # ground truth without a prediction: recall 0, precision None, F1 None; predictions without ground truth: the other way round
    rows = ref.box_rows([[0, 0]], [[4, 2]], [0.0])
    none = np.zeros((0, 12), np.float32)
    s = {"x": eval_box.new_sums()}
    eval_box.tally(s["x"], rows, none, np.array([-1]), np.zeros((1, 2)))
    at = eval_box.summary(s)["x"]["buckets"]["all"]["at"]["0.5"]
    assert at == {"tp": 0, "fn": 1, "recall": 0.0, "fp": 0, "precision": None, "f1": None}
    s = {"x": eval_box.new_sums()}
    eval_box.tally(s["x"], none, rows, np.zeros(0, np.int32), np.zeros((0, 2)))
    at = eval_box.summary(s)["x"]["buckets"]["all"]["at"]["0.5"]
    assert at == {"tp": 0, "fn": 0, "recall": None, "fp": 1, "precision": 0.0, "f1": None}
    same_numbers(eval_box.summary(s)["x"], ref.score([(none, rows, np.zeros(0, np.int32), np.zeros((0, 2)))]))


def test_label_pairs():
    from himo_amd import eval_box
    a = ref.box_rows(np.zeros((4, 2)), np.ones((4, 2)), np.zeros(4), ids=[7, 3, 9, 5])
    b = ref.box_rows(np.zeros((3, 2)), np.ones((3, 2)), np.zeros(3), ids=[9, 4, 3])
    ia, ib = eval_box.label_pairs(a, b)
    assert ia.tolist() == [1, 2] and ib.tolist() == [2, 0]


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------------
def test_binding_mirrors_the_header():
    from himo_amd import _lib, eval_box
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_boxeval_params") == ctypes.sizeof(eval_box._CParams) == 16
    header = (REPO / "include" / "himo_amd.h").read_text()
    assert re.search(r"#define HIMO_BOXEVAL_MAX_BOXES (\d+)", header).group(1) == str(eval_box.MAX_BOXES) == str(ref.MAX_BOXES) == "1024"
    assert re.search(r"#define HIMO_BOXEVAL_TILE (\d+)", header).group(1) == str(eval_box.TILE)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, args in (("himo_boxeval_workspace_bytes", 3), ("himo_boxeval_match", 14), ("himo_box_iou_pairs", 8)):
        m = re.search(name + r"\s*\(([^)]*)\)", text)
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == args, name
    # the workspace query needs no GPU: the dense candidate store, and 0 for what it refuses
    off = lambda *v: np.asarray(v, dtype=np.int64)                  # noqa: E731
    q = lambda S, a, b: int(lib.himo_boxeval_workspace_bytes(S, a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None))      # noqa: E731
    assert q(2, off(0, 300, 301), off(0, 10, 129)) == 301 * 119 * 8 + (-(301 * 119 * 8) % 256)
    assert q(1, off(0, 1024), off(0, 1024)) == 1024 * 1024 * 8 and q(1, off(0, 0), off(0, 0)) == 256 and q(0, None, None) == 256
    assert q(1, off(0, 1025), off(0, 3)) == 0 and q(1, off(0, 3), off(0, 1025)) == 0 and q(-1, off(0), off(0)) == 0
    assert q(2, off(0, 5, 4), off(0, 1, 2)) == 0 and q(1, off(1, 5), off(0, 1)) == 0 and q(1, None, off(0, 1)) == 0
    for v in (0.0, -0.1, 1.5, math.nan, math.inf, True, "0.1"):
        with pytest.raises(ValueError):
            eval_box.check_min_iou(v)
    assert eval_box.check_min_iou(1) == 1.0 and eval_box.check_min_iou(np.float32(0.5)) == 0.5


def test_documents_name_the_stage():
    from himo_amd import eval_box
    for doc, needle in (("README.md", "box evaluation, v1; parity unpinned: the reference has no such stage"), ("DESIGN.md", "box evaluation, v1"),
                        ("INTEGRATION.md", "himo_boxeval_match"), ("profiles/README.md", "box_eval.txt")):
        assert needle in (REPO / doc).read_text(), doc
    assert "PARITY UNPINNED" in eval_box.__doc__ and "profiles/box_eval.txt" in eval_box.__doc__ and (REPO / "profiles" / "box_eval.txt").exists()
    assert "parity unpinned" in eval_box._parser().format_help() and "profiles/box_eval.txt" in eval_box._parser().format_help()
    assert "FLAGS_boxeval := -ffp-contract=off" in (REPO / "himo_amd" / "csrc" / "Makefile").read_text()


# ---- the program's refusals, before any GPU use ------------------------------------------------------------------------------------------------------
def _container(root, boxes):
    """an npz directory of two sweeps holding the arrays of ``boxes`` = {key: [array of sweep 0, array of sweep 1]}"""
    from himo_amd.dataset import NpzDataset
    frames = []
    for k in range(2):
        f = {"scene_id": "s0", "timestamp": 1000 + k, "pc0": np.zeros((4, 3), np.float32), "pose0": np.eye(4), "pose1": np.eye(4)}
        f.update({key: v[k] for key, v in boxes.items()})
        frames.append(f)
    NpzDataset.write(root, frames)


def test_program_refusals(tmp_path, monkeypatch):
    from himo_amd import eval_box

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was asked for before the refusal")
    monkeypatch.setattr(eval_box, "BoxEvaluator", no_gpu)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    rows = ref.box_rows([[0, 0], [9, 9]], [[4, 2], [4, 2]], [0.0, 1.0])
    root = tmp_path / "d"
    _container(root, {"boxes_flow": [rows, rows], "boxes_raw": [rows, rows[:1]], "boxes_wide": [rows, np.zeros((2, 13), np.float32)],
                      "boxes_f64": [rows.astype(np.float64), rows], "boxes_part": [rows, rows], "boxes_big": [rows, np.zeros((1025, 12), np.float32)]})
    with np.load(root / "s0" / "1001.npz") as z:                     # ... and one name that the second sweep lacks
        kept = {k: z[k] for k in z.files if k != "boxes_part"}
    np.savez(root / "s0" / "1001.npz", **kept)
    with pytest.raises(ValueError, match="different names"):
        eval_box.main(str(root), "flow", "raw,raw")
    with pytest.raises(ValueError, match="different names"):
        eval_box.main(str(root), "flow", "")
    with pytest.raises(ValueError, match="--gt flow is among"):
        eval_box.main(str(root), "flow", "raw,flow")
    with pytest.raises(ValueError, match="--gt flow is among"):
        eval_box._cli(["--data_dir", str(root), "--gt", "flow", "--res_names", "flow"])
    with pytest.raises(KeyError, match="boxes_nope.*himo_amd.box_fit"):
        eval_box.main(str(root), "flow", "raw,nope")
    with pytest.raises(KeyError, match="boxes_nope.*himo_amd.box_fit"):
        eval_box.main(str(root), "nope", "raw")
    with pytest.raises(KeyError, match="boxes_part: s0/1001"):
        eval_box.main(str(root), "flow", "part")
    with pytest.raises(ValueError, match=r"boxes_wide.*\(2, 13\).*float32 \[F\]\[12\]"):
        eval_box.main(str(root), "flow", "wide")
    with pytest.raises(ValueError, match="boxes_f64.*float64"):
        eval_box.main(str(root), "flow", "f64")
    with pytest.raises(ValueError, match="boxes_big.*1025 boxes.*1024"):
        eval_box.main(str(root), "flow", "big")
    for kw in (dict(pair_by="score"), dict(min_iou=0.0), dict(min_iou=1.5), dict(batch=0), dict(motion_min=math.nan)):
        with pytest.raises(ValueError):
            eval_box.main(str(root), "flow", "raw", **kw)
    with pytest.raises(SystemExit):
        eval_box._cli(["--data_dir", str(root), "--gt", "flow", "--res_names", "raw", "--pair_by", "score"])
