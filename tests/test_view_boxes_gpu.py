"""The viewer's line overlay on the GPU: ``himo_render_lines`` / ``himo_render_composite`` against the restatement of their written
rule (tests/renderlines_ref.py; "line overlay, v1" is this build's own rule: parity unpinned, the reference has no such stage) -- the
lines buffer bit for bit over the segment counts at which waves and blocks fill, three image sizes, both projections and every
``half_px``, with ends off-screen, behind the camera and non-finite; the hand-worked cases of tests/test_view_boxes_cpu.py; a segment
whose ends lie 10^5 pixels off-screen; a contended pixel; depth ties; split calls in both orders; the composite bit for bit over
buffers a real splat made; the refusals; ``Renderer.lines`` / ``composite``; ``render_frame(boxes=True)`` against the restatement
chained by hand; then the program end to end.  Every output has guard words on both sides."""
import ctypes
import json

import numpy as np
import pytest

import render_ref as pref
import renderlines_ref as ref
from test_view_boxes_cpu import LINE_HAND_CASES, box, track_rows
from test_view_cpu import decode_png, ortho_cam, pinhole_cam
from test_view_gpu import FILL8, FILL64, GUARD, Buffer, cloud, to_ctypes

pytestmark = pytest.mark.gpu


class LineBuffer(Buffer):
    """a guarded lines buffer on the device, cleared by the library"""

    def lines(self, segs, cam, half_px=0, index_base=0, n=None):
        """one raw call -> its status"""
        import torch
        from himo_amd import _lib
        segs = np.ascontiguousarray(np.asarray(segs, np.float32).reshape(-1, 6))
        self.keep = torch.from_numpy(segs).to(self.t.device)
        c = cam if isinstance(cam, ctypes.Structure) else to_ctypes(cam)
        return self.lib.himo_render_lines(len(segs) if n is None else n, self.keep.data_ptr(), ctypes.addressof(c), half_px, index_base, self.ptr,
                                          _lib.stream_handle())


def assert_lines_equal_the_restatement(segs, cam, calls=None, half_px=0):
    """``calls``: [(lo, hi)] slices issued in that order with index_base = lo (default: one call)"""
    segs = np.asarray(segs, np.float32).reshape(-1, 6)
    buf = LineBuffer(cam["width"], cam["height"])
    want = ref.clear(cam["width"], cam["height"])
    ref.lines(want, segs, cam, half_px=half_px)
    for lo, hi in calls if calls is not None else [(0, len(segs))]:
        assert buf.lines(segs[lo:hi], cam, half_px=half_px, index_base=lo) == 0
    got, clean = buf.read()
    assert clean
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} words differ"
    return want


def unproject(cam, u, v, z):
    if cam["ortho"]:
        return (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
    return (u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z


def segments(seed, n, cam, depths=None):
    """segments whose ends' images cover the screen and a margin of its own size round it (most cross an edge, a fifth lie outside
    altogether), depths on both sides of near (1) and far (9) and of the camera plane, some ends on whole pixels, a few rows NaN / Inf"""
    rng = np.random.default_rng(seed)
    w, h = cam["width"], cam["height"]
    out = np.zeros((n, 6), np.float64)
    for e in (0, 3):
        u, v = rng.uniform(-w - 4.0, 2.0 * w + 4.0, n), rng.uniform(-h - 4.0, 2.0 * h + 4.0, n)
        z = rng.uniform(-2.0, 12.0, n) if depths is None else rng.choice(np.asarray(depths, np.float64), n)
        u[::5], v[::7] = np.floor(u[::5]), np.floor(v[::7])
        out[:, e], out[:, e + 1] = unproject(cam, u, v, z)
        out[:, e + 2] = z
    out = out.astype(np.float32)
    if n > 30:
        out[3, 0], out[9, 4], out[17, 2], out[19, 3], out[23] = np.nan, np.inf, -np.inf, -3.0e38, (0, 0, -3.0e38, 1, 1, 3.0e38)
        out[27] = out[26]                                            # a duplicate: an equal-depth tie along a whole segment
        out[29, 3:] = out[29, :3]                                    # zero length
    return out


SIZES = [(1, 1), (7, 5), (64, 48)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_segment_counts_images_projections_and_widths(gpu, n, size):
    w, h = size
    for make in (ortho_cam, pinhole_cam):
        cam = make(w, h)
        segs = segments(1000 * n + 10 * w + (make is pinhole_cam), n, cam)
        for half_px in (0, 1, 2, 3):
            want = assert_lines_equal_the_restatement(segs, cam, half_px=half_px)
            assert n < 63 or (want != ref.EMPTY).any()


@pytest.mark.parametrize("case", LINE_HAND_CASES, ids=lambda c: c[0])
def test_hand_worked_cases(gpu, case):
    _, segs, half_px = case
    segs = np.asarray(segs, np.float32)
    for cam in (ortho_cam(8, 6), pinhole_cam(8, 6), pinhole_cam(8, 6, near=-1.0)):
        assert_lines_equal_the_restatement(segs, cam, half_px=half_px)
        for k in range(len(segs)):                                   # each segment alone: no other key can hide a difference
            assert_lines_equal_the_restatement(segs[k:k + 1], cam, half_px=half_px)
            assert_lines_equal_the_restatement(segs[k:k + 1, [3, 4, 5, 0, 1, 2]], cam, half_px=half_px)


def test_a_segment_from_far_off_screen_to_far_off_screen(gpu):
    """both ends about 10^5 pixels outside a 64 x 48 image, on opposite sides: a walk of 2 * 10^5 steps of which some 60 are on screen"""
    for make in (ortho_cam, pinhole_cam):
        cam = make(64, 48)
        segs = []
        for (u0, v0, u1, v1) in ((-100000.5, -74990.2, 100050.5, 75040.7), (100031.0, 20.5, -99990.0, 27.25), (30.5, -100000.0, 33.5, 100000.0),
                                 (-99000.0, 100000.0, 99040.0, -99950.0), (-1048575.0, -786400.0, 1048575.0, 786470.0),
                                 (-100000.0, 70.0, 100000.0, 60.0), (70.0, -100000.0, 64.0, 100000.0)):
            (x0, y0), (x1, y1) = unproject(cam, u0, v0, 3.0), unproject(cam, u1, v1, 7.0)
            segs.append([x0, y0, 3.0, x1, y1, 7.0])
        segs = np.asarray(segs, np.float32)
        for half_px in (0, 3):
            want = assert_lines_equal_the_restatement(segs, cam, half_px=half_px)
            hit = (want & np.uint64(0xFFFFFFFF))[want != ref.EMPTY]
            assert set(hit.tolist()) >= {0, 1, 2, 3, 4} and 5 not in hit         # the first five cross the image, a miss is a miss
        for k in range(len(segs)):
            assert_lines_equal_the_restatement(segs[k:k + 1], cam, half_px=1)


def test_a_thousand_segments_through_one_pixel(gpu):
    rng = np.random.default_rng(2)
    n = 1000
    th, r0, r1 = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.0, 40.0, n), rng.uniform(0.0, 40.0, n)
    jx, jy = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n)
    segs = np.stack([32.5 + jx + r0 * np.cos(th), 24.5 + jy + r0 * np.sin(th), rng.uniform(1.0, 9.0, n),
                     32.5 + jx - r1 * np.cos(th), 24.5 + jy - r1 * np.sin(th), rng.uniform(1.0, 9.0, n)], axis=1).astype(np.float32)
    for half_px in (0, 3):
        want = assert_lines_equal_the_restatement(segs, ortho_cam(64, 48), half_px=half_px)
        assert want[24, 32] != ref.EMPTY
    want = assert_lines_equal_the_restatement(segs, ortho_cam(1, 1), half_px=3)
    assert want.shape == (1, 1)


def test_depth_ties_go_to_the_lowest_index(gpu):
    for make in (ortho_cam, pinhole_cam):
        cam = make(64, 48)
        segs = segments(77, 1000, cam, depths=np.arange(1, 10))      # nine depths: crossing segments often meet at one zq
        want = assert_lines_equal_the_restatement(segs, cam, half_px=1)
        rev = LineBuffer(64, 48)                                     # the same segments in reverse order, each under its own index
        assert rev.lines(segs[::-1].copy(), cam, half_px=1) == 0
        got, clean = rev.read()
        hit = want != ref.EMPTY
        assert clean and np.array_equal(got == ref.EMPTY, ~hit)
        assert np.array_equal(got[hit] >> np.uint64(32), want[hit] >> np.uint64(32))


def test_segments_split_over_two_calls_in_both_orders(gpu):
    for make in (ortho_cam, pinhole_cam):
        cam = make(64, 48)
        segs = segments(5, 600, cam)
        one = assert_lines_equal_the_restatement(segs, cam, half_px=1)
        for calls in ([(0, 234), (234, 600)], [(234, 600), (0, 234)], [(599, 600), (4, 599), (0, 4)]):
            assert np.array_equal(assert_lines_equal_the_restatement(segs, cam, calls=calls, half_px=1), one)
    buf = LineBuffer(8, 6)                                           # index_base reaches the last index a key can hold
    assert buf.lines([[3.5, 2.5, 5, 3.5, 2.5, 5]], ortho_cam(8, 6), index_base=0xFFFFFFFF) == 0
    got, clean = buf.read()
    assert clean and got[2, 3] == np.uint64(8388608 << 32 | 0xFFFFFFFF) and int((got != ref.EMPTY).sum()) == 1


# ---- composite ---------------------------------------------------------------------------------------------------------------------
def device_composite(d_lines_ptr, d_vis_ptr, w, h, rgb, colors, neutral=0x808080, n_colors=None, null_out=False, null_colors=False, call_size=None):
    """one raw call on a guarded copy of ``rgb`` ([h][w][3]; ``call_size``: the width and height the call is given instead) ->
    (status, uint8 [h][w][3], guards untouched?)"""
    import torch
    from himo_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    call_w, call_h = call_size if call_size is not None else (w, h)
    out = torch.full((GUARD + 3 * w * h + GUARD,), FILL8, dtype=torch.uint8, device=dev)
    out[GUARD:GUARD + 3 * w * h] = torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(np.asarray(colors, np.uint32)).view(np.int32)).to(dev)
    st = lib.himo_render_composite(d_lines_ptr, d_vis_ptr, call_w, call_h, None if null_colors or col.numel() == 0 else col.data_ptr(),
                                   len(colors) if n_colors is None else n_colors, neutral, None if null_out else out.data_ptr() + GUARD,
                                   _lib.stream_handle())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    clean = bool((o[:GUARD] == FILL8).all() and (o[GUARD + 3 * w * h:] == FILL8).all())
    return st, o[GUARD:GUARD + 3 * w * h].reshape(h, w, 3).copy(), clean


@pytest.fixture(scope="module")
def drawn_scene(gpu):
    """a 64 x 48 pinhole view: points splatted and segments drawn BY THE DEVICE, read back once, and the resolved image of the points"""
    cam = pinhole_cam(64, 48)
    pts, _, _ = cloud(41, 1500, cam)
    segs = segments(42, 300, cam)
    points, lines = Buffer(64, 48), LineBuffer(64, 48)
    assert points.splat(pts, cam, radius=2) == 0 and lines.lines(segs, cam, half_px=1) == 0
    vis, clean_p = points.read()
    buf, clean_l = lines.read()
    want_vis, want_buf = pref.clear(64, 48), ref.clear(64, 48)
    pref.splat(want_vis, pts, cam, radius=2)
    ref.lines(want_buf, segs, cam, half_px=1)
    assert clean_p and clean_l and np.array_equal(vis, want_vis) and np.array_equal(buf, want_buf)
    both = (vis != ref.EMPTY) & (buf != ref.EMPTY)
    assert (both & ((vis >> np.uint64(32)) < (buf >> np.uint64(32)))).sum() > 20 and (both & ((vis >> np.uint64(32)) > (buf >> np.uint64(32)))).sum() > 20
    rgb = pref.resolve(vis, 0, np.arange(1500, dtype=np.uint32) * np.uint32(2654435761) & np.uint32(0xFFFFFF))
    return points, lines, vis, buf, rgb


def test_composite_is_bit_equal_with_and_without_the_depth_test(gpu, drawn_scene):
    points, lines, vis, buf, rgb = drawn_scene
    colors = (np.arange(300, dtype=np.uint32) * np.uint32(40503) + np.uint32(77)) & np.uint32(0xFFFFFF)
    for with_vis in (False, True):
        for cols in (colors, colors[:100], colors[:0]):                  # indices past the colours take neutral; none at all: all neutral
            st, got, clean = device_composite(lines.ptr, points.ptr if with_vis else None, 64, 48, rgb, cols, neutral=0x0A0B0C)
            want = ref.composite(rgb, buf, vis if with_vis else None, cols, neutral=0x0A0B0C)
            assert st == 0 and clean and np.array_equal(got, want), (with_vis, len(cols))
            assert np.array_equal(got[buf == ref.EMPTY], rgb[buf == ref.EMPTY])
    hidden = ref.composite(rgb, buf, vis, colors)
    on_top = ref.composite(rgb, buf, None, colors)
    assert (hidden != on_top).any() and (on_top != rgb).any()
    # an equal depth shows the line, an empty point word never hides one: the hand-made words of the CPU test, on the device
    import torch
    key = lambda zq, idx: (zq << 32 | idx) - (1 << 64 if zq >> 31 else 0)        # noqa: E731
    words_l = np.array([key(5, 0), key(9, 1), key(7, 2), key(7, 0), -1, key(3, 9)], np.int64)
    words_v = np.array([key(9, 0), key(5, 0), key(7, 0), -1, key(1, 0), -1], np.int64)
    d_l, d_v = torch.from_numpy(words_l).to(gpu), torch.from_numpy(words_v).to(gpu)
    flat = np.full((1, 6, 3), 10, np.uint8)
    three = np.array([0x010203, 0x040506, 0x070809], np.uint32)
    st, got, clean = device_composite(d_l.data_ptr(), d_v.data_ptr(), 6, 1, flat, three, neutral=0x0C0B0A)
    assert st == 0 and clean and got[0].tolist() == [[3, 2, 1], [10, 10, 10], [9, 8, 7], [3, 2, 1], [10, 10, 10], [10, 11, 12]]
    st, got, clean = device_composite(d_l.data_ptr(), None, 6, 1, flat, three, neutral=0x0C0B0A)
    assert st == 0 and clean and got[0].tolist() == [[3, 2, 1], [6, 5, 4], [9, 8, 7], [3, 2, 1], [10, 10, 10], [10, 11, 12]]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu, drawn_scene):
    import torch
    from himo_amd import _lib
    lib, bad, unsupported = _lib.load(), _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    cam, W, H = ortho_cam(8, 6), 8, 6
    segs = segments(8, 100, cam)

    def untouched(buf):
        got, clean = buf.read()
        return clean and (got == np.uint64(FILL64)).all()

    for kw in (dict(half_px=-1), dict(half_px=4), dict(n=-1)):
        buf = LineBuffer(W, H, clear=False)
        assert buf.lines(segs, cam, **kw) == bad and untouched(buf), kw
    for field, value, status in (("width", 0, bad), ("width", -8, bad), ("height", 0, bad), ("height", -1, bad), ("znear", float("nan"), bad),
                                 ("zfar", float("inf"), bad), ("zfar", 1.0, bad), ("zfar", 0.5, bad), ("inv_range", 0.0, bad),
                                 ("inv_range", float("nan"), bad), ("width", 16385, unsupported), ("height", 16385, unsupported)):
        c = to_ctypes(cam)
        setattr(c, field, value)
        buf = LineBuffer(W, H, clear=False)
        assert buf.lines(segs, c, half_px=1) == status and untouched(buf), (field, value)
    buf = LineBuffer(W, H, clear=False)
    c = to_ctypes(cam)
    stream = _lib.stream_handle()
    d_seg = torch.from_numpy(segs).to(gpu)
    assert lib.himo_render_lines(100, None, ctypes.addressof(c), 1, 0, buf.ptr, stream) == bad
    assert lib.himo_render_lines(100, d_seg.data_ptr(), None, 1, 0, buf.ptr, stream) == bad
    assert lib.himo_render_lines(100, d_seg.data_ptr(), ctypes.addressof(c), 1, 0, None, stream) == bad
    assert lib.himo_render_lines(100, d_seg.data_ptr(), ctypes.addressof(c), 1, 0, buf.ptr + 4, stream) == bad
    assert lib.himo_render_lines(99, d_seg.data_ptr() + 2, ctypes.addressof(c), 1, 0, buf.ptr, stream) == bad
    assert lib.himo_render_lines(2, d_seg.data_ptr(), ctypes.addressof(c), 1, 0xFFFFFFFF, buf.ptr, stream) == unsupported
    assert lib.himo_render_lines(2 ** 31, d_seg.data_ptr(), ctypes.addressof(c), 1, 0, buf.ptr, stream) == unsupported
    assert lib.himo_render_lines(0, None, ctypes.addressof(c), 1, 0, buf.ptr, stream) == 0          # n == 0: a no-op
    assert untouched(buf)

    points, lines, vis, line_words, rgb = drawn_scene
    colors = np.arange(300, dtype=np.uint32)

    def refused(status=bad, lines_ptr=lines.ptr, vis_ptr=None, **kw):
        st, got, clean = device_composite(lines_ptr, vis_ptr, 64, 48, np.full((48, 64, 3), FILL8, np.uint8), colors, **kw)
        return st == status and clean and (got == FILL8).all()

    assert refused(lines_ptr=None) and refused(lines_ptr=lines.ptr + 4) and refused(vis_ptr=points.ptr + 4) and refused(null_out=True)
    assert refused(call_size=(0, 48)) and refused(call_size=(64, -48)) and refused(n_colors=-1) and refused(null_colors=True)
    assert refused(unsupported, call_size=(16385, 1)) and refused(unsupported, call_size=(1, 16385))
    assert np.array_equal(lines.read()[0], line_words) and np.array_equal(points.read()[0], vis)     # and the inputs are inputs


# ---- Renderer and render_frame -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boxed_frame():
    """a small synthetic sweep with hand-placed boxes for `raw` and `flow` and tracks for `flow`"""
    from himo_amd.synthetic import make_scene
    frame = dict(make_scene(23, 1, n_points=3000, scene_id="vb0")[0])
    frame["boxes_flow"] = np.array([box(5, 4, -1, 4.5, 1.9, 1.6, 0.3, 6.0, 2.0), box(-12, 9, -1, 10, 2.5, 3.2, -2.0), box(np.nan, 0, 0),
                                    box(20, -15, 0, 4, 2, 2, 1.2, -0.2, 0.1)], np.float32)
    frame["boxes_raw"] = np.array([box(5.3, 4.1, -1, 5.5, 2.1, 1.6, 0.35), box(-12, 9, -1, 10, 2.5, 3.2, -2.0)], np.float32)
    frame["tracks_flow"] = track_rows((8, 5, 4), (-1, 0, 0), (-1, 0, 0), (3, 20, -15))
    frame["tracks_raw"] = track_rows((5, 5.3, 4.1), (-1, 0, 0))
    return frame


def test_renderer_lines_and_composite(gpu, boxed_frame):
    from himo_amd.view import Camera, Renderer, box_segments
    cam = Camera.look_at((-30.0, -25.0, 20.0), (0.0, 0.0, 0.0), width=64, height=48, far=150.0)
    c = pref.from_ctypes(cam)
    r = Renderer(64, 48, gpu)
    assert r.line_buffer() is None
    rgba = np.arange(len(boxed_frame["pc0"]), dtype=np.uint32) * np.uint32(2654435761)
    with pytest.raises(ValueError):
        r.composite(np.zeros(3, np.uint32))                             # nothing resolved yet
    r.splat(boxed_frame["pc0"], radius=1, camera=cam)
    assert r.line_buffer() is None                                      # a renderer that draws no lines allocates none
    segs, owner = box_segments(boxed_frame["boxes_flow"])
    r.lines(segs[:20], half_px=1, camera=cam)
    r.lines(segs[20:], half_px=1, index_base=20, camera=cam)
    want = ref.clear(64, 48)
    ref.lines(want, segs, c, half_px=1)
    assert np.array_equal(r.line_buffer().cpu().numpy().view(np.uint64), want) and (want != ref.EMPTY).sum() > 20
    vis = pref.clear(64, 48)
    pref.splat(vis, boxed_frame["pc0"][:, :3], c, radius=1)
    assert np.array_equal(r.visibility().cpu().numpy().view(np.uint64), vis)                  # the point buffer is untouched
    base = pref.resolve(vis, 0, rgba)
    colors = np.array([0xFF0000, 0x00FF00, 0, 0x0000FF], np.uint32)[owner]
    for depth_test in (False, True):
        r.resolve(colors=rgba)
        image = r.composite(colors, depth_test=depth_test, neutral=0x123456)
        assert image.shape == (48, 64, 3) and np.array_equal(image.cpu().numpy(), ref.composite(base, want, vis if depth_test else None, colors, 0x123456))
    r.resolve(colors=rgba)
    assert np.array_equal(r.composite(colors[:5]).cpu().numpy(), ref.composite(base, want, None, colors[:5]))
    with pytest.raises(ValueError):
        r.lines(segs[:, :5], camera=cam)
    with pytest.raises(ValueError):
        r.lines(segs, camera=Camera.bev(width=32, height=48))
    with pytest.raises(ValueError):
        r.lines(segs, half_px=4, camera=cam)
    with pytest.raises(ValueError):
        r.lines(segs)
    assert np.array_equal(r.line_buffer().cpu().numpy().view(np.uint64), want)                # the refused calls drew nothing
    r.clear_lines()
    assert (r.line_buffer().cpu().numpy() == -1).all() and np.array_equal(r.visibility().cpu().numpy().view(np.uint64), vis)
    r.lines(segs, camera=cam)
    r.clear()                                                           # the panel: both buffers
    assert (r.line_buffer().cpu().numpy() == -1).all() and (r.visibility().cpu().numpy() == -1).all()


def test_render_frame_with_boxes_against_the_restatement_chained_by_hand(gpu, boxed_frame):
    from himo_amd import compdis, view
    from test_view_gpu import frame_skip
    frame = boxed_frame
    cam = view.Camera.bev((0.0, 0.0), 40.0, 64, 48, z_range=(-5.0, 10.0))
    c = pref.from_ctypes(cam)
    skip, pal = frame_skip(frame), view.palette()
    plain, plain_info = view.render_frame(frame, ["raw", "flow"], "lidar", cam)
    assert set(plain_info) == {"panels", "points", "pixels"}
    for box_depth in (False, True):
        image, info, buffers, line_buffers = view.render_frame(frame, ["raw", "flow"], "lidar", cam, return_buffers=True, boxes=True, boxes_gt="flow",
                                                               box_color_by="track", line_px=1, box_depth=box_depth, arrow_s=1.0)
        image = image.cpu().numpy()
        gt_segs, _ = view.box_segments(frame["boxes_flow"], 0.1, 0.05, 1.0)
        assert info["boxes"] == [2 + 3, 3 + 3] and info["points"] == plain_info["points"] and info["pixels"] == plain_info["pixels"]
        for k, name in enumerate(("raw", "flow")):
            vis = pref.clear(64, 48)
            moved = frame["pc0"][:, :3] if name == "raw" else frame["pc0"][:, :3] + compdis.comp_dis_frame(frame, name)
            pref.splat(vis, moved, c, radius=1, skip=skip)
            own, owner = view.box_segments(frame[f"boxes_{name}"], 0.1, 0.05, 1.0)
            ids = np.array({"raw": [5, -1], "flow": [8, -1, -1, 3]}[name])
            per_box = np.where(ids >= 0, pal[ids % 6], view.NEUTRAL).astype(np.uint32)
            colors = np.concatenate([per_box[owner], np.full(len(gt_segs), 0xFFFFFF, np.uint32)])
            want = ref.clear(64, 48)
            ref.lines(want, np.concatenate([own, gt_segs]), c, half_px=1)
            assert np.array_equal(buffers[k].cpu().numpy().view(np.uint64), vis) and np.array_equal(line_buffers[k].cpu().numpy().view(np.uint64), want)
            assert info["segments"][k] == len(own) + len(gt_segs) and info["line_pixels"][k] == int((want != ref.EMPTY).sum()) > 50
            x0 = k * (64 + view.SEPARATOR_PX)
            base = pref.resolve(vis, 2, frame["lidar_id"].astype(np.int32), palette=pal)
            assert np.array_equal(image[:, x0:x0 + 64], ref.composite(base, want, vis if box_depth else None, colors))
            assert np.array_equal(plain.cpu().numpy()[:, x0:x0 + 64], base)             # and without the flags the panel is what it was
        with pytest.raises(ValueError, match="stale"):                   # one track row for the two boxes of raw
            view.render_frame({**frame, "tracks_raw": track_rows((0, 1, 1))}, ["raw"], "lidar", cam, boxes=True, box_color_by="track")
    # the overlay panel: every name's boxes in that name's cloud colour
    image, info, buffers, line_buffers = view.render_frame(frame, ["raw", "flow"], "overlay", cam, return_buffers=True, boxes=True)
    a, _ = view.box_segments(frame["boxes_raw"])
    b, _ = view.box_segments(frame["boxes_flow"])
    want = ref.clear(64, 48)
    ref.lines(want, np.concatenate([a, b]), c)
    assert np.array_equal(line_buffers[0].cpu().numpy().view(np.uint64), want) and info["boxes"] == [5] and info["segments"] == [len(a) + len(b)]
    got = image.cpu().numpy()[want != ref.EMPTY]
    low = (want & np.uint64(0xFFFFFFFF))[want != ref.EMPTY]
    assert (got[low < len(a)] == 255).all() and (got[low >= len(a)] == (0x1b, 0x9e, 0x77)).all()
    with pytest.raises(KeyError, match="boxes_nope"):
        view.render_frame(frame, ["raw"], "lidar", cam, boxes_gt="nope")
    with pytest.raises(KeyError, match="tracks_raw"):
        view.render_frame({k: v for k, v in frame.items() if k != "tracks_raw"}, ["raw"], "lidar", cam, boxes=True, box_color_by="track")


# ---- the program -------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end_with_boxes_tracks_and_trails(gpu, tmp_path, capsys):
    from himo_amd import view
    from himo_amd.dataset import NpzDataset
    from himo_amd.synthetic import make_scene
    root = tmp_path / "scenes"
    frames = []
    for s in range(2):                                                   # two scenes of 4 sweeps, 3 boxes each, the ego frame moving on
        for k, f in enumerate(make_scene(80 + s, 4, n_points=400, scene_id=f"vb{s}")):
            f = dict(f)
            rows = [box(6 + 1.5 * k, 5, -1, 4.5, 1.9, 1.6, 0.1, 15.0, 1.0), box(-8, -6 - 0.5 * k, -1, 4.5, 1.9, 1.6, -1.5, 0.0, -5.0),
                    box(15, -12, -0.5, 10, 2.5, 3.2, 2.0)]
            f["boxes_flow"] = np.array(rows, np.float32)
            f["boxes_raw"] = np.array(rows[:2], np.float32) + np.float32([0.4, 0.2, 0, 1.5, 0.2, 0, 0.05, 0, 0, 0, 0, 0])
            ids = [(0, rows[0][0], rows[0][1]), (1, rows[1][0], rows[1][1]), ((2, rows[2][0], rows[2][1]) if k != 2 else (-1, 0, 0))]
            f["tracks_flow"], f["tracks_raw"] = track_rows(*ids), track_rows(*ids[:2])
            frames.append(f)
    NpzDataset.write(root, frames)
    out = tmp_path / "out"
    flags = "--boxes --boxes_gt flow --box_color_by track --trail 2"
    base = f"--data_dir {root} --indices 2:6 --res_names raw,flow --color_by lidar --camera auto --size 96x64"
    listing = view._cli(f"{base} --out_dir {out} {flags}".split())
    assert json.loads((out / "view.json").read_text()) == listing and len(listing) == 4
    pal = view.palette()
    line_colours = {(int(c) & 0xFF, int(c) >> 8 & 0xFF, int(c) >> 16 & 0xFF) for c in pal[:3]} | {(255, 255, 255), (0x80, 0x80, 0x80)}
    for entry, scene_sweep in zip(listing, (2, 3, 0, 1)):
        assert entry["boxes"] == [2 + 3, 3 + 3] and entry["panels"] == ["raw", "flow"]
        # 16 segments for each of the two moving boxes, 13 for the still one; trails: one segment per earlier sweep of the id's scene
        # (ids 0 and 1 are in every sweep; id 2 is missing from sweep 2, which leaves its trail a gap in sweeps 2 and 3)
        trail_raw = 2 * min(scene_sweep, 2)
        trail_flow = trail_raw + (1 if scene_sweep == 1 else 0)
        assert entry["segments"] == [32 + trail_raw + 45, 45 + trail_flow + 45], (scene_sweep, entry["segments"])
        assert min(entry["line_pixels"]) > 10 and len(entry["points"]) == 2
        image = decode_png((out / entry["file"]).read_bytes())
        assert image.shape == (64, 2 * 96 + view.SEPARATOR_PX, 3)
        seen = {tuple(px) for px in image.reshape(-1, 3).tolist()}
        assert (255, 255, 255) in seen and len(seen & line_colours) >= 3
    # the same command without the flags: none of the new keys, and the points as they were
    plain = view._cli(f"{base} --out_dir {tmp_path / 'plain'}".split())
    assert all(set(e) == {"file", "scene_id", "timestamp", "color_by", "camera", "panels", "points", "pixels"} for e in plain)
    assert [e["points"] for e in plain] == [e["points"] for e in listing] and [e["pixels"] for e in plain] == [e["pixels"] for e in listing]
    without = decode_png((tmp_path / "plain" / plain[0]["file"]).read_bytes())
    assert (255, 255, 255) not in {tuple(px) for px in without.reshape(-1, 3).tolist()}
    # what the scene does not hold is the error that names it; tracks that do not fit the boxes are stale
    capsys.readouterr()
    with pytest.raises(KeyError, match="boxes_seflowpp"):
        view._cli(f"{base} --out_dir {tmp_path / 'no'} --boxes_gt seflowpp".split())
    assert "[Warning]: No boxes_seflowpp in vb0 at" in capsys.readouterr().out
    for f in frames:
        del f["tracks_raw"]
    NpzDataset.write(root, frames)
    with pytest.raises(KeyError, match="tracks_raw"):
        view._cli(f"{base} --out_dir {tmp_path / 'no'} --boxes --trail 2".split())
    for f in frames:
        f["tracks_raw"] = track_rows((0, 1, 1))
    NpzDataset.write(root, frames)
    with pytest.raises(ValueError, match="stale"):
        view._cli(f"{base} --out_dir {tmp_path / 'no'} --boxes --box_color_by track".split())
