"""The viewer's line overlay without a GPU: the restatement of "line overlay, v1" (tests/renderlines_ref.py) against pixels worked by
hand on an 8 x 6 image, ``box_segments`` and ``trail_segments`` against hand values, the program's new arguments and refusals."""
import numpy as np
import pytest

import render_ref as pref
import renderlines_ref as ref
from himo_amd import view
from test_view_cpu import ortho_cam, pinhole_cam

W, H = 8, 6
Z5, Z3 = 8388608, 4194304                                        # zq of depth 5 and of depth 3 between near 1 and far 9
BELOW_2_20 = float(np.nextafter(np.float32(1048576.0), np.float32(0.0)))
NAN = float("nan")

# the hand-worked cases, shared with tests/test_view_boxes_gpu.py: (name, segments, half_px)
LINE_HAND_CASES = [
    ("horizontal", [[1.5, 2.5, 5, 5.5, 2.5, 5], [5.5, 2.5, 5, 1.5, 2.5, 5]], 0),
    ("vertical", [[3.5, 0.5, 5, 3.5, 4.5, 5], [3.5, 4.5, 5, 3.5, 0.5, 5]], 0),
    ("diagonal", [[1.5, 1.5, 5, 4.5, 4.5, 5], [4.5, 4.5, 5, 1.5, 1.5, 5]], 0),
    ("shallow", [[0.5, 1.5, 5, 6.5, 3.5, 5], [6.5, 3.5, 5, 0.5, 1.5, 5]], 0),
    ("half-way", [[1.5, 1.5, 5, 3.5, 2.5, 5], [3.5, 2.5, 5, 1.5, 1.5, 5], [1.5, 2.5, 5, 3.5, 1.5, 5]], 0),
    ("zero length", [[2.5, 3.5, 5, 2.5, 3.5, 5]], 0),
    ("crossing near", [[1.5, 1.5, -1, 5.5, 1.5, 3], [5.5, 1.5, 3, 1.5, 1.5, -1]], 0),
    ("both ends behind", [[1.5, 1.5, -1, 5.5, 1.5, 0.5]], 1),
    ("both ends beyond far", [[1.5, 1.5, 9.5, 5.5, 1.5, 30]], 1),
    ("crossing far", [[1.5, 4.5, 5, 5.5, 4.5, 13]], 0),
    ("crossing near and far", [[0.5, 0.5, -7, 6.5, 0.5, 17]], 0),
    ("nan and inf ends", [[NAN, 2.5, 5, 5.5, 2.5, 5], [1.5, 2.5, 5, 5.5, NAN, 5], [1.5, 2.5, float("inf"), 5.5, 2.5, 5],
                          [1.5, 2.5, 5, float("-inf"), 2.5, 5]], 1),
    ("2^20 is dropped", [[1048576.0, 2.5, 5, 3.5, 2.5, 5], [3.5, 2.5, 5, -1048576.0, 2.5, 5], [3.5, 1048576.0, 5, 3.5, 2.5, 5]], 0),
    ("just below 2^20 is drawn", [[3.5, 2.5, 5, BELOW_2_20, 2.5, 5], [-BELOW_2_20, 4.5, 5, 2.5, 4.5, 5]], 0),
    ("equal depth", [[1.5, 2.5, 5, 5.5, 2.5, 5], [1.5, 2.5, 5, 5.5, 2.5, 5], [3.5, 0.5, 5, 3.5, 4.5, 5]], 0),
    ("nearer wins", [[1.5, 2.5, 5, 5.5, 2.5, 5], [3.5, 0.5, 3, 3.5, 4.5, 3]], 0),
    ("half_px 1", [[2.5, 3.5, 5, 4.5, 3.5, 5]], 1),
    ("half_px 2", [[2.5, 3.5, 5, 4.5, 3.5, 5]], 2),
    ("half_px 3 off the corner", [[-2.5, -1.5, 5, -2.5, -1.5, 5]], 3),
]
CASE = {name: (segs, half_px) for name, segs, half_px in LINE_HAND_CASES}


def cam8(ortho=True):
    return ortho_cam(W, H) if ortho else pinhole_cam(W, H)


def drawn(buf):
    return {(int(x), int(y)): (int(buf[y, x] >> np.uint64(32)), int(buf[y, x] & np.uint64(0xFFFFFFFF)))
            for y, x in zip(*np.nonzero(buf != ref.EMPTY))}


def one(segs, cam=None, **kw):
    buf = ref.clear(W, H)
    ref.lines(buf, np.asarray(segs, np.float32).reshape(-1, 6), cam if cam is not None else cam8(), **kw)
    return drawn(buf)


def test_horizontal_vertical_diagonal_and_shallow_segments_walked_both_ways():
    for k in (0, 1):
        assert one(CASE["horizontal"][0][k]) == {(x, 2): (Z5, 0) for x in range(1, 6)}
        assert one(CASE["vertical"][0][k]) == {(3, y): (Z5, 0) for y in range(0, 5)}
        assert one(CASE["diagonal"][0][k]) == {(d, d): (Z5, 0) for d in range(1, 5)}
        # dx = 6, dy = 2: y_k = 1 + floor((4 k + 6) / 12) = 1 1 2 2 2 3 3; backwards y_k = 3 + floor((6 - 4 k) / 12) = 3 3 2 2 2 1 1
        assert one(CASE["shallow"][0][k]) == {(x, y): (Z5, 0) for x, y in zip(range(7), (1, 1, 2, 2, 2, 3, 3))}


def test_a_half_way_pixel_rounds_up_whichever_way_the_segment_runs():
    """(1, 1) -> (3, 2): at k = 1 the line stands at y = 1.5, which rounds UP to 2: floor((2 * 1 * 1 + 2) / 4) = 1.  Walked from the
    other end the same point is 2 + floor((2 * 1 * -1 + 2) / 4) = 2 + 0: the same pixel.  The rule's walk is a function of the point
    (x_k = floor(X0 + k dx / steps + 1/2)), so swapping the ends changes nothing; it is the MIRROR IMAGE of the segment, (1, 2) -> (3, 1),
    whose half-way pixel (2, 2) is not the mirror image (2, 1) of the first one's."""
    a_to_b, b_to_a, mirrored = (one(s) for s in CASE["half-way"][0])
    assert a_to_b == b_to_a == {(1, 1): (Z5, 0), (2, 2): (Z5, 0), (3, 2): (Z5, 0)}
    assert mirrored == {(1, 2): (Z5, 0), (2, 2): (Z5, 0), (3, 1): (Z5, 0)}
    assert ref.walk_py(1, 1, 0, 3, 2, 0) == [(1, 1, 0), (2, 2, 0), (3, 2, 0)] and ref.walk_py(3, 2, 0, 1, 1, 0) == [(3, 2, 0), (2, 2, 0), (1, 1, 0)]
    # depth along the walk: floor division from either end gives the same depth at the same pixel
    assert [z for _, _, z in ref.walk_py(0, 0, 10, 3, 0, 0)] == [10, 6, 3, 0] and [z for _, _, z in ref.walk_py(3, 0, 0, 0, 0, 10)] == [0, 3, 6, 10]


def test_the_array_walk_is_the_python_int_walk():
    rng = np.random.default_rng(3)
    for _ in range(300):
        e = [int(v) for v in rng.integers(-40, 40, 6)]
        e[2], e[5] = int(rng.integers(0, 1 << 24)), int(rng.integers(0, 1 << 24))
        x, y, zq = ref.walk(*e)
        assert list(zip(x.tolist(), y.tolist(), zq.tolist())) == ref.walk_py(*e)
        back = ref.walk_py(e[3], e[4], e[5], e[0], e[1], e[2])
        assert back[::-1] == ref.walk_py(*e)                          # swapping the ends changes no pixel and no depth
    e = (-1048575, 1048575, 0, 1048575, -1048575, (1 << 24) - 1)      # the longest segment the rule admits: int64 holds every product
    x, y, zq = ref.walk(*e)
    assert len(x) == 2097151 and (x[0], y[0], zq[0]) == e[:3] and (x[-1], y[-1], zq[-1]) == e[3:]
    k = 1234567
    assert (int(x[k]), int(y[k]), int(zq[k])) == (e[0] + (2 * k * 2097150 + 2097150) // 4194300, e[1] + (-2 * k * 2097150 + 2097150) // 4194300,
                                                  (k * e[5]) // 2097150)


def test_zero_length_is_one_pixel():
    assert one(CASE["zero length"][0]) == {(2, 3): (Z5, 0)}
    assert one(CASE["zero length"][0], cam8(False)) == {(5, 4): (Z5, 0)}         # u = 2 * (2.5 / 5) + 4 = 5, v = 2 * (3.5 / 5) + 3 = 4.4


def test_depth_clip_by_hand():
    # za = -1 < near = 1: t = (1 - -1) / (3 - -1) = 0.5, xa' = 1.5 + 0.5 * 4 = 3.5, za' = 1 -> zq 0; b stays: zq (3 - 1) / 8 * 2^24
    want = {(3, 1): (0, 0), (4, 1): (Z3 // 2, 0), (5, 1): (Z3, 0)}
    assert one(CASE["crossing near"][0][0]) == want and one(CASE["crossing near"][0][1]) == want
    assert one(CASE["both ends behind"][0], half_px=1) == {} and one(CASE["both ends beyond far"][0], half_px=1) == {}
    # zb = 13 > far = 9: t = (9 - 13) / (5 - 13) = 0.5, xb' = 5.5 + 0.5 * -4 = 3.5, zb' = 9 -> zq 2^24, clamped to 2^24 - 1
    assert one(CASE["crossing far"][0]) == {(1, 4): (Z5, 0), (2, 4): (Z5 + (2 ** 24 - 1 - Z5) // 2, 0), (3, 4): (2 ** 24 - 1, 0)}
    # both ends clipped, each from the ORIGINAL pair: a: t = 8 / 24, xa' = 0.5 + 6 / 3 = 2.5; b: t = (9 - 17) / (-7 - 17) = 1 / 3,
    # xb' = 6.5 - 2 = 4.5
    got = one(CASE["crossing near and far"][0])
    assert set(got) == {(2, 0), (3, 0), (4, 0)} and got[(2, 0)] == (0, 0) and got[(4, 0)] == (2 ** 24 - 1, 0) and got[(3, 0)] == ((2 ** 24 - 1) // 2, 0)


def test_non_finite_ends_and_the_2_20_limit():
    assert one(CASE["nan and inf ends"][0], half_px=1) == {} and one(CASE["nan and inf ends"][0], cam8(False), half_px=1) == {}
    assert one(CASE["2^20 is dropped"][0]) == {}
    got = one(CASE["just below 2^20 is drawn"][0])
    assert got == {**{(x, 2): (Z5, 0) for x in range(3, 8)}, **{(x, 4): (Z5, 1) for x in range(0, 3)}}
    buf = ref.clear(W, H)
    assert ref.lines(buf, np.asarray(CASE["2^20 is dropped"][0], np.float32), cam8()) == 0
    assert ref.lines(buf, np.asarray(CASE["just below 2^20 is drawn"][0], np.float32), cam8()) == 2


def test_equal_depth_goes_to_the_lowest_index_and_a_nearer_segment_wins():
    got = one(CASE["equal depth"][0])
    assert got == {**{(x, 2): (Z5, 0) for x in range(1, 6)}, **{(3, y): (Z5, 2) for y in (0, 1, 3, 4)}}
    got = one(CASE["equal depth"][0], index_base=7)
    assert got[(3, 2)] == (Z5, 7) and got[(3, 0)] == (Z5, 9)
    got = one(CASE["nearer wins"][0])
    assert got[(3, 2)] == (Z3, 1) and got[(2, 2)] == (Z5, 0)
    # the split over calls does not matter
    a, b = ref.clear(W, H), ref.clear(W, H)
    segs = np.asarray(CASE["equal depth"][0] + CASE["nearer wins"][0], np.float32)
    ref.lines(a, segs, cam8())
    ref.lines(b, segs[3:], cam8(), index_base=3)
    ref.lines(b, segs[:3], cam8())
    assert np.array_equal(a, b)


def test_line_widths_counted_by_hand():
    # three pixels (2..4, 3) under the plus of half_px 1: row 3 spans 1..5, rows 2 and 4 span 2..4: 5 + 3 + 3
    got = one(CASE["half_px 1"][0], half_px=1)
    assert len(got) == 11 and set(got) == {(x, 3) for x in range(1, 6)} | {(x, y) for x in range(2, 5) for y in (2, 4)}
    # the 13-pixel disc of half_px 2: row 3 spans 0..6, rows 2 and 4 span 1..5, rows 1 and 5 span 2..4: 7 + 2 * 5 + 2 * 3
    got = one(CASE["half_px 2"][0], half_px=2)
    assert len(got) == 23 and sum(1 for x, y in got if y == 3) == 7 and sum(1 for x, y in got if y in (1, 5)) == 6
    assert len(one(CASE["zero length"][0], half_px=1)) == 5 and len(one(CASE["zero length"][0], half_px=2)) == 13
    # pixel (-3, -2) under the disc of half_px 3 (dx^2 + dy^2 <= 9): only (dx, dy) = (3, ...) has dy = 0: nothing reaches row 0
    assert one(CASE["half_px 3 off the corner"][0], half_px=3) == {}
    assert set(one([[-2.5, 0.5, 5, -2.5, 0.5, 5]], half_px=3)) == {(0, 0)}                   # pixel (-3, 0): (dx, dy) = (3, 0) alone reaches column 0


def test_composite_by_hand():
    key = lambda zq, idx: np.uint64(zq << 32 | idx)                  # noqa: E731
    lines = np.array([[key(5, 0), key(9, 1), key(7, 2), key(7, 0), ref.EMPTY, key(3, 9)]], np.uint64)
    vis = np.array([[key(9, 0), key(5, 0), key(7, 0), ref.EMPTY, key(1, 0), ref.EMPTY]], np.uint64)
    rgb = np.full((1, 6, 3), 10, np.uint8)
    colors = np.array([0x010203, 0x040506, 0x070809], np.uint32)
    on_top = ref.composite(rgb, lines, None, colors, neutral=0x0C0B0A)
    assert on_top[0].tolist() == [[3, 2, 1], [6, 5, 4], [9, 8, 7], [3, 2, 1], [10, 10, 10], [10, 11, 12]]
    tested = ref.composite(rgb, lines, vis, colors, neutral=0x0C0B0A)
    # nearer line; farther line hidden; equal depth: the line; an empty point word never hides; no line; idx >= n_colors: neutral
    assert tested[0].tolist() == [[3, 2, 1], [10, 10, 10], [9, 8, 7], [3, 2, 1], [10, 10, 10], [10, 11, 12]]
    assert (rgb == 10).all()                                         # the input is not written
    assert ref.composite(rgb, lines, vis, np.zeros(0, np.uint32), neutral=0x0C0B0A)[0, 0].tolist() == [10, 11, 12]


# ---- box_segments ------------------------------------------------------------------------------------------------------------------
def box(x=10.0, y=20.0, z=1.0, l=4.0, w=2.0, h=2.0, yaw=0.0, vx=0.0, vy=0.0):     # noqa: E741
    return [x, y, z, l, w, h, yaw, vx, vy, 0.0, 3.0, 50.0]


def test_box_corners_by_hand():
    q = view.box_corners(box())
    assert q.tolist() == [[12, 21, 0], [8, 21, 0], [8, 19, 0], [12, 19, 0], [12, 21, 2], [8, 21, 2], [8, 19, 2], [12, 19, 2]]
    q = view.box_corners(box(yaw=np.pi / 2))                         # the front now points along +y
    assert np.abs(q[:4] - [[9, 22, 0], [9, 18, 0], [11, 18, 0], [11, 22, 0]]).max() < 1e-12 and (q[4:, 2] == 2).all()


def test_box_segments_order_counts_and_arrow():
    segs, owner = view.box_segments([box()], 0.1, 0.05, 0.5)
    assert segs.dtype == np.float32 and segs.shape == (view.SEGMENTS_STATIC, 6) == (13, 6) and owner.tolist() == [0] * 13
    assert segs[0].tolist() == [12, 21, 0, 8, 21, 0] and segs[3].tolist() == [12, 19, 0, 12, 21, 0]          # the bottom ring closes
    assert segs[4].tolist() == [12, 21, 2, 8, 21, 2] and segs[8].tolist() == [12, 21, 0, 12, 21, 2] and segs[11].tolist() == [12, 19, 0, 12, 19, 2]
    assert segs[12].tolist() == [10, 20, 2, 12, 20, 2]                                                        # the heading mark
    edges = {tuple(sorted([tuple(s[:3]), tuple(s[3:])])) for s in segs[:12].tolist()}
    assert len(edges) == 12 and all(sum(a != b for a, b in zip(*e)) == 1 for e in edges)                     # 12 different axis-parallel edges
    # moving: 3 m/s along +x, 0.5 s of travel: d = (1.5, 0), tip (11.5, 20), n = (0, 1.5): strokes to (11.5 - 0.375, 20 +- 0.1875)
    segs, owner = view.box_segments([box(), box(vx=3.0)], 0.1, 0.05, 0.5)
    assert len(segs) == 13 + view.SEGMENTS_MOVING == 29 and owner.tolist() == [0] * 13 + [1] * 16
    assert segs[26].tolist() == [10, 20, 2, 11.5, 20, 2] and segs[27].tolist() == [11.5, 20, 2, 11.125, 20.1875, 2]
    assert segs[28].tolist() == [11.5, 20, 2, 11.125, 19.8125, 2]
    # hypot(vx, vy) * sensor_dt >= motion_min decides (in numbers that are exact in binary): 0.5 m/s over 0.125 s is exactly the 0.0625 m,
    # 0.4375 m/s is static; arrow_s = 0 draws no arrow
    assert len(view.box_segments([box(vy=-0.5)], 0.125, 0.0625, 0.5)[0]) == 16 and len(view.box_segments([box(vx=0.4375)], 0.125, 0.0625, 0.5)[0]) == 13
    assert len(view.box_segments([box(vx=3.0)], 0.1, 0.05, 0.0)[0]) == 13 and len(view.box_segments([box(vx=3.0)], 0.1, 40.0, 0.5)[0]) == 13


def test_box_segments_skips_invalid_rows():
    rows = [box(), box(x=NAN), box(l=-1.0), box(vx=float("inf")), box(h=0.0, vy=-2.0), [NAN] * 12]
    segs, owner = view.box_segments(rows, 0.1, 0.05, 0.5)
    assert owner.tolist() == [0] * 13 + [4] * 16 and np.isfinite(segs).all()
    assert view.box_valid(rows).tolist() == [True, False, False, False, True, False]
    segs, owner = view.box_segments(np.zeros((0, 12), np.float32))
    assert segs.shape == (0, 6) and segs.dtype == np.float32 and owner.shape == (0,)


# ---- trail_segments ----------------------------------------------------------------------------------------------------------------
def pose(x):
    p = np.eye(4)
    p[0, 3] = x
    return p


def track_rows(*rows):
    return np.array([[i, 1, x, y, 0, 0] if i >= 0 else [-1, 0, 0, 0, 0, 0] for i, x, y in rows], np.float64)


@pytest.fixture()
def trail_scene():
    """three sweeps of scene a, the sensor 10 m further along +x in each, then one sweep of scene b; id 1 is missing from sweep 1"""
    from himo_amd.dataset import ListDataset
    two = np.array([box(3, 1, 0), box(7, 5, 0)], np.float32)
    frames = [dict(scene_id="a", timestamp=0, pose0=pose(0.0), boxes_flow=two, tracks_flow=track_rows((0, 1, 1), (1, 5, 5))),
              dict(scene_id="a", timestamp=1, pose0=pose(10.0), boxes_flow=two[:1], tracks_flow=track_rows((0, 2, 1))),
              dict(scene_id="a", timestamp=2, pose0=pose(20.0), boxes_flow=two, tracks_flow=track_rows((0, 3, 1), (1, 7, 5))),
              dict(scene_id="b", timestamp=3, pose0=pose(30.0), boxes_flow=two, tracks_flow=track_rows((0, 4, 1), (1, 8, 5)))]
    return ListDataset(frames)


def test_trails_in_the_current_frame_with_a_gap_and_no_scene_crossing(trail_scene):
    segs, owner = view.trail_segments(trail_scene, 2, "flow", 2)
    # id 0: (1, 1) of sweep 0 is 20 m behind, (2, 1) of sweep 1 10 m behind; the top face of a box at z = 0 with h = 2 is at 1
    assert segs.dtype == np.float32 and segs.tolist() == [[-19, 1, 1, -8, 1, 1], [-8, 1, 1, 3, 1, 1]] and owner.tolist() == [0, 0]
    # id 1 is in sweeps 0 and 2, not in 1: a gap, and so no segment at all
    segs, owner = view.trail_segments(trail_scene, 2, "flow", 1)
    assert segs.tolist() == [[-8, 1, 1, 3, 1, 1]] and owner.tolist() == [0]
    assert view.trail_segments(trail_scene, 2, "flow", 0)[0].shape == (0, 6)
    assert view.trail_segments(trail_scene, 2, "flow", 50)[0].shape == (2, 6)                # the scene starts at sweep 0
    # sweep 3 opens scene b: the same ids in scene a are other objects
    assert view.trail_segments(trail_scene, 3, "flow", 2)[0].shape == (0, 6)
    # an untracked box (id -1) and an invalid box have no trail
    trail_scene.frames[2]["tracks_flow"] = track_rows((-1, 0, 0), (1, 7, 5))
    trail_scene.frames[1]["tracks_flow"] = track_rows((1, 6, 5))
    segs, owner = view.trail_segments(trail_scene, 2, "flow", 2, boxes=trail_scene.frames[2]["boxes_flow"])
    assert segs.tolist() == [[-15, 5, 1, -4, 5, 1], [-4, 5, 1, 7, 5, 1]] and owner.tolist() == [1, 1]


def test_trails_need_tracks_and_refuse_stale_ones(trail_scene, capsys):
    with pytest.raises(KeyError, match="tracks_other"):
        view.trail_segments(trail_scene, 2, "other", 2)
    assert "[Warning]: No tracks_other in a at 2, check the data." in capsys.readouterr().out
    trail_scene.frames[2]["tracks_flow"] = track_rows((0, 3, 1))                              # one row for two boxes
    with pytest.raises(ValueError, match="stale"):
        view.trail_segments(trail_scene, 2, "flow", 2)
    with pytest.raises(ValueError):
        view.trail_segments(trail_scene, 1, "flow", -1)


# ---- the program's arguments -------------------------------------------------------------------------------------------------------
def test_cli_arguments_of_the_overlay():
    a = view._parser().parse_args("--data_dir D --index 1 --out_dir O".split())
    assert (a.boxes, a.boxes_gt, a.box_color_by, a.trail, a.arrow_s, a.line_px, a.box_depth) == (False, None, "fixed", 0, 0.5, 0, False)
    a = view._parser().parse_args("--data_dir D --index 1 --out_dir O --boxes --boxes_gt flow --box_color_by track --trail 10 --arrow_s 1.5 "
                                  "--line_px 2 --box_depth".split())
    assert (a.boxes, a.boxes_gt, a.box_color_by, a.trail, a.arrow_s, a.line_px, a.box_depth) == (True, "flow", "track", 10, 1.5, 2, True)
    assert view.overlay_keys(["raw", "flow"]) == [] and view.overlay_keys(["raw", "flow"], boxes=True) == ["boxes_raw", "boxes_flow"]
    assert view.overlay_keys(["raw"], True, "flow", "track") == ["boxes_raw", "tracks_raw", "boxes_flow"]
    assert view.overlay_keys(["flow"], True, "flow", "moving", trail=3) == ["boxes_flow", "tracks_flow"]
    assert view.overlay_keys(["flow"], False, "gt") == ["boxes_gt"]
    view.check_line_options("moving", 3, 3, 0.0)
    for kw in (dict(box_color_by="id"), dict(trail=-1), dict(trail=1.5), dict(line_px=4), dict(line_px=-1), dict(arrow_s=-1.0), dict(arrow_s=NAN)):
        with pytest.raises(ValueError):
            view.check_line_options(**kw)


def test_the_program_refuses_before_it_opens_anything(tmp_path):
    base = f"--data_dir {tmp_path / 'none'} --index 0 --res_names raw --out_dir {tmp_path / 'out'}"
    with pytest.raises(ValueError, match="line_px"):
        view._cli(f"{base} --boxes --line_px 4".split())
    with pytest.raises(ValueError, match="box_color_by"):
        view._cli(f"{base} --boxes --box_color_by speed".split())
    with pytest.raises(ValueError, match="--boxes"):
        view._cli(f"{base} --trail 2".split())
    assert not (tmp_path / "out").exists()


def test_stale_tracks_are_refused_for_colouring():
    rows = np.array([box(), box(x=30.0)], np.float32)
    data = dict(scene_id="a", timestamp=0, boxes_flow=rows, tracks_flow=track_rows((0, 10, 20)))
    with pytest.raises(ValueError, match="stale"):
        view._panel_lines(data, ["flow"], None, None, "track", None, 0.1, 0.05, 0.5)
    data["tracks_flow"] = track_rows((7, 10, 20), (-1, 0, 0))
    segs, cols, count = view._panel_lines(data, ["flow"], None, "flow", "track", None, 0.1, 0.05, 0.5)
    pal = view.palette()
    assert count == 4 and len(segs) == 52 and cols.tolist() == [pal[1]] * 13 + [view.NEUTRAL] * 13 + [view.WHITE] * 26
    data["boxes_flow"] = np.array([box(), box(vx=5.0)], np.float32)
    segs, cols, count = view._panel_lines(data, ["flow"], None, None, "moving", None, 0.1, 0.05, 0.5)
    assert cols.tolist() == [pal[2]] * 13 + [pal[1]] * 16
    segs, cols, count = view._panel_lines(data, ["flow"], [0x123456], None, "moving", None, 0.1, 0.05, 0.5)
    assert set(cols.tolist()) == {0x123456}


def test_the_restatement_reuses_the_point_splats_camera_disc_and_clear():
    assert ref.camera is pref.camera and ref.disc is pref.disc and ref.clear is pref.clear
