"""The headless viewer on the GPU: ``himo_render_clear`` / ``himo_render_splat`` / ``himo_render_resolve`` against the numpy
restatement of their written rule (tests/render_ref.py; "point splat, v1" is this build's own rule and no other viewer's pixels are
claimed) -- the visibility buffer bit for bit over the point counts at which waves and blocks fill, three image sizes, four radii,
both pitches, offset, skip, both projections, the hand-worked edge cases of tests/test_view_cpu.py, a contended pixel, depth ties
and split calls in both orders; the image bit for bit in all three colour modes and within one level under eye-dome lighting; the
refusals; ``Renderer`` / ``render_frame`` on a synthetic frame; then the program end to end.  Every output has guard words on both
sides."""
import ctypes
import json

import numpy as np
import pytest

import render_ref as ref
from test_view_cpu import HAND_CASES, decode_png, ortho_cam, pinhole_cam

pytestmark = pytest.mark.gpu

GUARD, FILL64, FILL8 = 256, 0x5A5A5A5A5A5A5A5A, 0xA5
POISON = np.float32(1.0e30)                                        # the fourth column of pitch-4 rows: never read


def to_ctypes(cam):
    from himo_amd.view import Camera
    c = Camera.make(cam["m"], cam["ortho"], float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), cam["znear"], cam["zfar"],
                    cam["width"], cam["height"])
    assert np.float32(c.inv_range) == cam["inv_range"]
    return c


class Buffer:
    """a guarded visibility buffer on the device, cleared by the library"""

    def __init__(self, width, height, clear=True):
        import torch
        from himo_amd import _lib
        self.lib, self.w, self.h = _lib.load(), width, height
        self.t = torch.full((GUARD + width * height + GUARD,), FILL64, dtype=torch.int64, device=torch.device("cuda", 0))
        self.ptr = self.t.data_ptr() + 8 * GUARD
        if clear:
            assert self.lib.himo_render_clear(self.ptr, width, height, _lib.stream_handle()) == 0

    def splat(self, pts, cam, radius=0, index_base=0, offset=None, skip=None, pitch=3, call_pitch=None, n=None):
        """one raw call -> its status"""
        import torch
        from himo_amd import _lib
        dev = self.t.device
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        rows = np.concatenate([pts, np.full((len(pts), pitch - 3), POISON, np.float32)], axis=1)
        self.keep = [torch.from_numpy(np.ascontiguousarray(rows)).to(dev),
                     None if offset is None else torch.from_numpy(np.ascontiguousarray(offset, dtype=np.float32)).to(dev),
                     None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, dtype=np.uint8)).to(dev)]
        c = cam if isinstance(cam, ctypes.Structure) else to_ctypes(cam)
        return self.lib.himo_render_splat(len(pts) if n is None else n, self.keep[0].data_ptr(), pitch if call_pitch is None else call_pitch,
                                          _lib.ptr(self.keep[1]), _lib.ptr(self.keep[2]), ctypes.addressof(c), radius, index_base, self.ptr,
                                          _lib.stream_handle())

    def read(self):
        """-> (uint64 [h][w], guards untouched?)"""
        import torch
        torch.cuda.synchronize()
        a = self.t.cpu().numpy().view(np.uint64)
        clean = bool((a[:GUARD] == FILL64).all() and (a[GUARD + self.w * self.h:] == FILL64).all())
        return a[GUARD:GUARD + self.w * self.h].reshape(self.h, self.w).copy(), clean


def assert_splat_equals_the_restatement(pts, cam, calls=None, **kw):
    """``calls``: [(lo, hi)] slices issued in that order with index_base = lo (default: one call)"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    buf = Buffer(cam["width"], cam["height"])
    want = ref.clear(cam["width"], cam["height"])
    ref_kw = {k: v for k, v in kw.items() if k in ("radius", "offset", "skip")}
    ref.splat(want, pts, cam, **ref_kw)
    for lo, hi in calls if calls is not None else [(0, len(pts))]:
        part = {k: (v[lo:hi] if k in ("offset", "skip") and v is not None else v) for k, v in kw.items()}
        assert buf.splat(pts[lo:hi], cam, index_base=lo, **part) == 0
    got, clean = buf.read()
    assert clean
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} words differ"
    return want


def cloud(seed, n, cam, spread=1.0, depths=None):
    """points whose images cover the screen and a margin wider than the largest radius, depths on both sides of near and far, some
    on whole pixels, a few NaN / Inf; and an offset and a skip array for them"""
    rng = np.random.default_rng(seed)
    w, h = cam["width"], cam["height"]
    u, v = rng.uniform(-12.0, w + 12.0, n), rng.uniform(-12.0, h + 12.0, n)
    z = rng.uniform(0.5, 10.0, n) if depths is None else np.asarray(depths, np.float64)
    u[::5], v[::7] = np.floor(u[::5]), np.floor(v[::7])
    if cam["ortho"]:
        x, y = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"]
    else:
        x, y = (u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z
    pts = np.stack([x, y, z], axis=1).astype(np.float32)
    if n > 20:
        pts[3], pts[9, 1], pts[17, 2], pts[19, 0] = (np.nan, 1.0, 5.0), np.inf, -np.inf, -3.0e38
    offset = rng.normal(0.0, 0.4 * spread, (n, 3)).astype(np.float32)
    if n > 20:
        offset[11] = (np.nan, 0.0, 0.0)
    skip = (rng.random(n) < 0.25).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)        # any non-zero byte skips
    return pts, offset, skip


SIZES = [(1, 1), (7, 5), (64, 48)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_point_counts_images_radii_pitches_offset_skip_and_projections(gpu, n, size):
    w, h = size
    combo = 0
    for radius in (0, 1, 3, 8):
        for make in (ortho_cam, pinhole_cam):
            cam = make(w, h)
            pts, offset, skip = cloud(1000 * n + 10 * w + radius, n, cam)
            # every pairing of (offset, skip) at every radius and projection over the two pitches in turn
            for with_offset, with_skip in ((False, False), (True, True), (True, False), (False, True)):
                want = assert_splat_equals_the_restatement(pts, cam, radius=radius, pitch=3 + combo % 2, offset=offset if with_offset else None,
                                                           skip=skip if with_skip else None)
                combo += 1
                assert n < 257 or w == 1 or (want != ref.EMPTY).any()


@pytest.mark.parametrize("case", HAND_CASES, ids=lambda c: c[0])
def test_hand_worked_edge_cases(gpu, case):
    _, pts, radius = case
    pts = np.asarray(pts, np.float32)
    for cam in (ortho_cam(), pinhole_cam(), pinhole_cam(near=-1.0)):
        assert_splat_equals_the_restatement(pts, cam, radius=radius)
        for k in range(len(pts)):                                    # each point alone: no other point's key can hide a difference
            assert_splat_equals_the_restatement(pts[k:k + 1], cam, radius=radius)
    assert_splat_equals_the_restatement(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]], np.float32), pinhole_cam(near=-1.0), radius=1)
    for r in (0, 1, 2, 3):
        want = assert_splat_equals_the_restatement(np.array([[7.5, 7.5, 5.0]], np.float32), ortho_cam(15, 15), radius=r)
        assert int((want != ref.EMPTY).sum()) == (1, 5, 13, 29)[r]


def test_five_thousand_points_in_one_pixel(gpu):
    rng = np.random.default_rng(2)
    n = 5000
    pts = np.stack([rng.uniform(3.0, 4.0, n), rng.uniform(2.0, 3.0, n), rng.uniform(1.0, 9.0, n)], axis=1).astype(np.float32)
    for radius in (0, 8):
        want = assert_splat_equals_the_restatement(pts, ortho_cam(), radius=radius, pitch=4)
        assert int(want[2, 3] & np.uint64(0xFFFFFFFF)) == int(np.argmin(pts[:, 2]))
    want = assert_splat_equals_the_restatement(pts, ortho_cam(1, 1), radius=8)                   # everything reaches the only pixel
    assert want.shape == (1, 1) and want[0, 0] != ref.EMPTY


def test_depth_ties_go_to_the_lowest_index(gpu):
    rng = np.random.default_rng(4)
    n = 5000
    for make in (ortho_cam, pinhole_cam):
        cam = make(64, 48)
        pts, _, _ = cloud(77, n, cam, depths=rng.integers(1, 10, n))    # nine depths: most pixels see several points of one zq
        want = assert_splat_equals_the_restatement(pts, cam, radius=3)
        assert len(np.unique(want[want != ref.EMPTY] >> np.uint64(32))) <= 9
        rev = Buffer(64, 48)                                             # the same points in reverse order, each under its own index
        assert rev.splat(pts[::-1].copy(), cam, radius=3) == 0
        got, clean = rev.read()
        hit = want != ref.EMPTY
        assert clean and np.array_equal(got == ref.EMPTY, ~hit)
        assert np.array_equal(got[hit] >> np.uint64(32), want[hit] >> np.uint64(32))


def test_a_cloud_split_over_two_calls_in_both_orders(gpu):
    for make in (ortho_cam, pinhole_cam):
        cam = make(64, 48)
        pts, offset, skip = cloud(5, 3000, cam)
        one = assert_splat_equals_the_restatement(pts, cam, radius=2, offset=offset, skip=skip)
        for calls in ([(0, 1234), (1234, 3000)], [(1234, 3000), (0, 1234)], [(2999, 3000), (64, 2999), (0, 64)]):
            assert np.array_equal(assert_splat_equals_the_restatement(pts, cam, calls=calls, radius=2, offset=offset, skip=skip, pitch=4), one)
    # index_base reaches the last index a key can hold
    buf = Buffer(7, 5)
    assert buf.splat([[3.5, 2.5, 5.0]], ortho_cam(), index_base=0xFFFFFFFF) == 0
    got, clean = buf.read()
    assert clean and got[2, 3] == np.uint64(8388608 << 32 | 0xFFFFFFFF) and int((got != ref.EMPTY).sum()) == 1


# ---- resolve -----------------------------------------------------------------------------------------------------------------------
def device_resolve(vis, mode, attr, lut=None, palette=None, lo=0.0, hi=1.0, background=0, neutral=0x808080, edl=0.0, edl_px=1, n_attr=None,
                   raw=None, width=None, height=None, null_out=False):
    """one raw call on a guarded image -> (status, uint8 [h][w][3], guards untouched?)"""
    import torch
    from himo_amd import _lib
    from himo_amd.view import Shade
    lib, dev = _lib.load(), torch.device("cuda", 0)
    h, w = vis.shape

    def up(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a).astype(dt))
        return torch.from_numpy(a.view(np.int32) if dt == np.uint32 else a).to(dev)
    d_vis = up(vis.view(np.int64), np.int64)
    d_attr = up(attr, (np.uint32, np.float32, np.int32)[mode]) if attr is not None else None
    d_lut, d_pal = up(lut, np.uint32), up(palette, np.uint32)
    sh = Shade(mode=mode, palette_n=0 if palette is None else len(palette), background=background, neutral=neutral, edl_strength=edl, edl_px=edl_px)
    sh.lut, sh.palette = _lib.ptr(d_lut), _lib.ptr(d_pal)
    setattr(sh, ("rgba", "scalar", "ids")[mode], _lib.ptr(d_attr))
    sh.n_attr = (0 if attr is None else len(attr)) if n_attr is None else n_attr
    sh.lo, sh.scale = np.float32(lo), np.float32(256.0) / (np.float32(hi) - np.float32(lo))
    for k, v in (raw or {}).items():
        setattr(sh, k, v)
    out = torch.full((GUARD + 3 * w * h + GUARD,), FILL8, dtype=torch.uint8, device=dev)
    st = lib.himo_render_resolve(d_vis.data_ptr(), w if width is None else width, h if height is None else height, ctypes.addressof(sh),
                                 None if null_out else out.data_ptr() + GUARD, _lib.stream_handle())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    clean = bool((o[:GUARD] == FILL8).all() and (o[GUARD + 3 * w * h:] == FILL8).all())
    return st, o[GUARD:GUARD + 3 * w * h].reshape(h, w, 3).copy(), clean


@pytest.fixture(scope="module")
def scene_buffers():
    """restatement buffers shared by the resolve tests: a half-empty 64 x 48 pinhole view, a full 7 x 5 one, an empty 1 x 1 one"""
    out = []
    for (w, h), n, radius in (((64, 48), 700, 1), ((7, 5), 300, 2), ((1, 1), 0, 0)):
        cam = pinhole_cam(w, h)
        pts, _, _ = cloud(31 + w, n, cam)
        vis = ref.clear(w, h)
        ref.splat(vis, pts, cam, radius=radius)
        out.append((vis, max(n, 1)))
    assert (out[0][0] == ref.EMPTY).any() and (out[0][0] != ref.EMPTY).any() and (out[2][0] == ref.EMPTY).all()
    return out


def attributes(mode, n, seed=0):
    rng = np.random.default_rng(seed)
    if mode == 0:
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if mode == 1:
        s = rng.uniform(-0.5, 1.5, n).astype(np.float32)              # bins at both clamps ...
        s[::11], s[1::13], s[2::17], s[3::19] = np.nan, np.inf, -np.inf, 1.0
        s[4::23], s[5::29] = 0.0, np.nextafter(np.float32(1.0), np.float32(0.0))
        return s
    ids = rng.integers(-3, 40, n).astype(np.int32)                    # ... negative ids and id % P wrap-around
    ids[::7], ids[1::9] = 2 ** 31 - 1, -2 ** 31
    return ids


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resolve_without_edl_is_bit_equal(gpu, scene_buffers, mode):
    from himo_amd.view import palette, sequential_lut
    for vis, n in scene_buffers:
        attr = attributes(mode, n, seed=mode)
        kw = dict(lut=sequential_lut(), palette=palette() if n % 2 else np.arange(1, 8, dtype=np.uint32) * 0x030507, lo=0.0, hi=1.0,
                  background=0x0A141E, neutral=0x112233)
        st, got, clean = device_resolve(vis, mode, attr, **kw)
        want = ref.resolve(vis, mode, attr, **kw)
        assert st == 0 and clean and np.array_equal(got, want)
        assert (got[vis == ref.EMPTY] == (0x1E, 0x14, 0x0A)).all()
        if (vis != ref.EMPTY).any():
            # attributes that end before the highest index: the pixels past them are neutral, nothing is read there
            short = int((vis[vis != ref.EMPTY] & np.uint64(0xFFFFFFFF)).max()) // 2 + 1
            st, got, clean = device_resolve(vis, mode, attr[:short], **kw)
            assert st == 0 and clean and np.array_equal(got, ref.resolve(vis, mode, attr[:short], **kw))
    if mode == 1:                                                      # another range: lo != 0, a scale that is no power of two
        vis, n = scene_buffers[0]
        attr = attributes(1, n, seed=9) * np.float32(7.0) - np.float32(2.0)
        kw = dict(lut=sequential_lut(), lo=-1.3, hi=4.9)
        st, got, clean = device_resolve(vis, 1, attr, **kw)
        assert st == 0 and clean and np.array_equal(got, ref.resolve(vis, 1, attr, **kw))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resolve_with_edl_is_within_one_level(gpu, scene_buffers, mode):
    from himo_amd.view import palette, sequential_lut
    for vis, n in scene_buffers:
        attr = attributes(mode, n, seed=3 + mode)
        for edl, px in ((0.7, 1), (4.0, 2), (1.0, 100)):
            kw = dict(lut=sequential_lut(), palette=palette(), background=0x0A141E, neutral=0xFFFFFF, edl=edl, edl_px=px)
            st, got, clean = device_resolve(vis, mode, attr, **kw)
            want = ref.resolve(vis, mode, attr, **kw)
            worst = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max())
            print(f"edl={edl} px={px} mode={mode} {vis.shape}: worst channel difference {worst}, {int((got != want).sum())} of {got.size} differ")
            assert st == 0 and clean and worst <= 1
            assert np.array_equal(got[vis == ref.EMPTY], want[vis == ref.EMPTY]) and (got[vis == ref.EMPTY] == (0x1E, 0x14, 0x0A)).all()
            if px == 100:                                              # every neighbour is outside the image: no shading at all
                assert np.array_equal(got, ref.resolve(vis, mode, attr, **dict(kw, edl=0.0)))
    plain = ref.resolve(scene_buffers[0][0], 0, np.full(scene_buffers[0][1], 0xFFFFFF, np.uint32))
    lit = ref.resolve(scene_buffers[0][0], 0, np.full(scene_buffers[0][1], 0xFFFFFF, np.uint32), edl=1.0)
    assert (lit <= plain).all() and (lit < plain).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu):
    import torch
    from himo_amd import _lib
    from himo_amd.view import Camera, Shade, sequential_lut
    lib = _lib.load()
    assert lib.himo_abi_sizeof(b"himo_camera") == ctypes.sizeof(Camera) == 88
    assert lib.himo_abi_sizeof(b"himo_shade") == ctypes.sizeof(Shade) == 80
    bad = _lib.ERR_INVALID_ARGUMENT
    cam, W, H = ortho_cam(), 7, 5
    pts, offset, skip = cloud(8, 300, cam)

    def untouched(buf):
        got, clean = buf.read()
        return clean and (got == np.uint64(FILL64)).all()

    for kw in (dict(radius=-1), dict(radius=9), dict(call_pitch=2), dict(call_pitch=0), dict(call_pitch=-3), dict(n=-1)):
        buf = Buffer(W, H, clear=False)
        assert buf.splat(pts, cam, **{"radius": 1, **kw}) == bad and untouched(buf), kw
    for field, value in (("width", 0), ("width", -7), ("height", 0), ("height", -1), ("znear", float("nan")), ("zfar", float("inf")),
                         ("zfar", 1.0), ("inv_range", 0.0), ("inv_range", float("nan")), ("inv_range", -1.0)):
        c = to_ctypes(cam)
        setattr(c, field, value)
        buf = Buffer(W, H, clear=False)
        assert buf.splat(pts, c, radius=1) == bad and untouched(buf), (field, value)
    buf = Buffer(W, H, clear=False)
    c = to_ctypes(cam)
    stream = _lib.stream_handle()
    d_pts = torch.from_numpy(pts).to(gpu)
    assert lib.himo_render_splat(300, None, 3, None, None, ctypes.addressof(c), 1, 0, buf.ptr, stream) == bad
    assert lib.himo_render_splat(300, d_pts.data_ptr(), 3, None, None, None, 1, 0, buf.ptr, stream) == bad
    assert lib.himo_render_splat(300, d_pts.data_ptr(), 3, None, None, ctypes.addressof(c), 1, 0, None, stream) == bad
    assert lib.himo_render_splat(300, d_pts.data_ptr(), 3, None, None, ctypes.addressof(c), 1, 0, buf.ptr + 4, stream) == bad
    assert lib.himo_render_splat(300, d_pts.data_ptr() + 2, 3, None, None, ctypes.addressof(c), 1, 0, buf.ptr, stream) == bad
    assert lib.himo_render_splat(2, d_pts.data_ptr(), 3, None, None, ctypes.addressof(c), 1, 0xFFFFFFFF, buf.ptr, stream) == _lib.ERR_UNSUPPORTED
    assert lib.himo_render_splat(0, None, 3, None, None, ctypes.addressof(c), 1, 0, buf.ptr, stream) == 0          # n == 0: a no-op
    for w, h in ((0, 5), (7, 0), (-1, 5), (7, -5)):
        assert lib.himo_render_clear(buf.ptr, w, h, stream) == bad
    assert lib.himo_render_clear(None, 7, 5, stream) == bad and lib.himo_render_clear(buf.ptr + 4, 7, 5, stream) == bad
    assert lib.himo_render_clear(buf.ptr, 16385, 1, stream) == _lib.ERR_UNSUPPORTED
    assert untouched(buf)

    vis = ref.clear(W, H)
    ref.splat(vis, pts, cam, radius=1)
    lut, pal = sequential_lut(), np.array([1, 2, 3], np.uint32)

    def refused(mode, attr, **kw):
        st, got, clean = device_resolve(vis, mode, attr, **kw)
        return st == bad and clean and (got == FILL8).all()

    ids, scal, rgba = attributes(2, 300), attributes(1, 300), attributes(0, 300)
    assert refused(2, ids, palette=pal, raw=dict(palette_n=0)) and refused(2, ids, palette=pal, raw=dict(palette_n=-6))
    assert refused(2, ids, palette=None, raw=dict(palette_n=3)) and refused(2, None, palette=pal, n_attr=300)
    assert refused(1, scal, lut=None) and refused(1, None, lut=lut, n_attr=300) and refused(0, None, n_attr=300)
    assert refused(1, scal, lut=lut, raw=dict(scale=float("inf"))) and refused(1, scal, lut=lut, raw=dict(lo=float("nan")))
    assert refused(0, rgba, raw=dict(mode=3)) and refused(0, rgba, raw=dict(mode=-1)) and refused(0, rgba, n_attr=-1)
    assert refused(0, rgba, edl=-1.0) and refused(0, rgba, edl=float("nan")) and refused(0, rgba, edl=1.0, edl_px=0)
    assert refused(0, rgba, width=0) and refused(0, rgba, height=-5) and refused(0, rgba, null_out=True)
    d_vis = torch.from_numpy(vis.view(np.int64)).to(gpu)
    out = torch.zeros(3 * W * H, dtype=torch.uint8, device=gpu)
    assert lib.himo_render_resolve(d_vis.data_ptr(), W, H, None, out.data_ptr(), stream) == bad
    assert lib.himo_render_resolve(None, W, H, ctypes.addressof(Shade()), out.data_ptr(), stream) == bad
    torch.cuda.synchronize()
    assert not out.any().item()
    # an attribute-less call is fine when nothing can index it: n_attr = 0 paints every hit neutral
    st, got, clean = device_resolve(vis, 0, None, n_attr=0, neutral=0x010203)
    assert st == 0 and clean and np.array_equal(got, ref.resolve(vis, 0, np.zeros(0, np.uint32), neutral=0x010203))


# ---- Renderer and render_frame -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic_frame():
    from himo_amd.synthetic import make_scene
    frame = dict(make_scene(21, 1, n_points=4000, scene_id="view0")[0])
    rng = np.random.default_rng(6)
    frame["seflowpp_best"] = (frame["flow"] + rng.normal(0.0, 0.05, frame["flow"].shape) * (frame["flow_instance_id"][:, None] > 0)).astype(np.float32)
    frame["my_label"] = (frame["flow_instance_id"] % 5).astype(np.int32)
    return frame


def frame_skip(frame, keep_ground=False):
    lo, hi = np.float32([-9.5, -3 / 2, 0]), np.float32([5, 2.760004 / 2, 5])
    p = frame["pc0"][:, :3]
    inside_ego = ((p > lo) & (p < hi)).all(axis=1)
    return (inside_ego | (np.zeros_like(inside_ego) if keep_ground else frame["gm0"])).astype(np.uint8)


def test_renderer_class(gpu, synthetic_frame):
    from himo_amd.view import Camera, Renderer, palette, sequential_lut
    pts = synthetic_frame["pc0"]
    cam = Camera.look_at((-40.0, -30.0, 25.0), (0.0, 0.0, 0.0), width=64, height=48, far=150.0)
    r = Renderer(64, 48, gpu, max_points=10_000)
    assert (r.visibility().cpu().numpy() == -1).all()
    r.splat(pts, radius=2, camera=cam)
    want = ref.clear(64, 48)
    ref.splat(want, pts[:, :3], ref.from_ctypes(cam), radius=2)
    assert np.array_equal(r.visibility().cpu().numpy().view(np.uint64), want) and (want != ref.EMPTY).sum() > 200
    ids = synthetic_frame["lidar_id"].astype(np.int32)
    assert np.array_equal(r.resolve(ids=(ids,)).cpu().numpy(), ref.resolve(want, 2, ids, palette=palette()))
    assert np.array_equal(r.resolve(ids=(ids, [5, 6]), background=0x332211, neutral=7).cpu().numpy(),
                          ref.resolve(want, 2, ids, palette=[5, 6], background=0x332211, neutral=7))
    dt = synthetic_frame["lidar_dt"]
    assert np.array_equal(r.resolve(scalar=(dt, 0.02, 0.09)).cpu().numpy(), ref.resolve(want, 1, dt, lo=0.02, hi=0.09, lut=sequential_lut()))
    rgba = np.arange(len(pts), dtype=np.uint32) * np.uint32(2654435761)
    image = r.resolve(colors=rgba)
    assert image.shape == (48, 64, 3) and np.array_equal(image.cpu().numpy(), ref.resolve(want, 0, rgba))
    lit = r.resolve(colors=rgba, edl=1.5, edl_px=2).cpu().numpy()
    assert np.abs(lit.astype(np.int32) - ref.resolve(want, 0, rgba, edl=1.5, edl_px=2).astype(np.int32)).max() <= 1
    with pytest.raises(ValueError):
        r.resolve(colors=rgba[:100])                                  # fewer attributes than point indices in the buffer
    with pytest.raises(ValueError):
        r.resolve(colors=rgba, ids=(ids,))
    with pytest.raises(ValueError):
        r.splat(pts, camera=Camera.bev(width=32, height=48))          # another image size
    with pytest.raises(ValueError):
        r.splat(pts, camera=cam, index_base=9_000)                    # past max_points
    with pytest.raises(ValueError):
        r.splat(pts, camera=cam, radius=9)
    with pytest.raises(ValueError):
        r.splat(pts, skip=np.zeros(5, np.uint8), camera=cam)
    assert np.array_equal(r.visibility().cpu().numpy().view(np.uint64), want)          # the refused calls drew nothing
    r.clear()
    assert (r.visibility().cpu().numpy() == -1).all()


def test_render_frame_fuses_the_offset_and_overlays_through_index_base(gpu, synthetic_frame):
    from himo_amd import compdis, view
    frame = synthetic_frame
    n = len(frame["pc0"])
    cam = view.Camera.bev((0.0, 0.0), 51.2, 64, 48, z_range=(-5.0, 10.0))
    c = ref.from_ctypes(cam)
    skip = frame_skip(frame)
    image, info, buffers = view.render_frame(frame, ["raw", "seflowpp_best", "flow"], "lidar", cam, point_px=1, return_buffers=True)
    assert info["panels"] == ["raw", "seflowpp_best", "flow"] and info["points"] == [int((skip == 0).sum())] * 3
    assert tuple(image.shape) == (48, 3 * 64 + 2 * view.SEPARATOR_PX, 3)
    image = image.cpu().numpy()
    pal = view.palette()
    for k, name in enumerate(info["panels"]):
        want = ref.clear(64, 48)
        moved = frame["pc0"][:, :3] if name == "raw" else frame["pc0"][:, :3] + compdis.comp_dis_frame(frame, name)      # added on the host
        ref.splat(want, moved, c, radius=1, skip=skip)
        assert np.array_equal(buffers[k].cpu().numpy().view(np.uint64), want), name
        assert info["pixels"][k] == int((want != ref.EMPTY).sum()) > 100
        x0 = k * (64 + view.SEPARATOR_PX)
        assert np.array_equal(image[:, x0:x0 + 64], ref.resolve(want, 2, frame["lidar_id"].astype(np.int32), palette=pal))
    assert (image[:, 64:66] == (0x40, 0x40, 0x40)).all() and not np.array_equal(image[:, :64], image[:, 132:196])
    # the overlay: every cloud in one buffer, cloud k under index_base = k * n
    image, info, buffers = view.render_frame(frame, ["raw", "flow"], "overlay", cam, point_px=1, return_buffers=True)
    want = ref.clear(64, 48)
    ref.splat(want, frame["pc0"][:, :3], c, radius=1, skip=skip)
    ref.splat(want, frame["pc0"][:, :3], c, radius=1, skip=skip, offset=compdis.comp_dis_frame(frame, "flow"), index_base=n)
    assert info["panels"] == ["raw+flow"] and tuple(image.shape) == (48, 64, 3) and info["points"] == [2 * int((skip == 0).sum())]
    assert np.array_equal(buffers[0].cpu().numpy().view(np.uint64), want)
    colours = np.concatenate([np.full(n, 0xFFFFFF, np.uint32), np.full(n, pal[0], np.uint32)])
    assert np.array_equal(image.cpu().numpy(), ref.resolve(want, 0, colours))
    low = (want & np.uint64(0xFFFFFFFF))[want != ref.EMPTY]
    assert (low < n).any() and (low >= n).any()
    # the other colourings, against the restatement fed the same attributes
    r = view.Renderer(64, 48, gpu)
    for color_by, keep_ground in (("dt0", False), ("speed", False), ("ground", True), ("label:my_label", False)):
        image, info, buffers = view.render_frame(frame, ["flow"], color_by, cam, r, point_px=0, return_buffers=True)
        want = ref.clear(64, 48)
        ref.splat(want, frame["pc0"][:, :3], c, radius=0, skip=frame_skip(frame, keep_ground), offset=compdis.comp_dis_frame(frame, "flow"))
        assert np.array_equal(buffers[0].cpu().numpy().view(np.uint64), want), color_by
        got = image.cpu().numpy()
        if color_by == "ground":
            assert np.array_equal(got, ref.resolve(want, 2, frame["gm0"].astype(np.int32), palette=pal))
        elif color_by == "label:my_label":
            assert np.array_equal(got, ref.resolve(want, 2, frame["my_label"] - 1, palette=pal))
        elif color_by == "dt0":
            dt0 = (frame["lidar_dt"].max() - frame["lidar_dt"]).astype(np.float32)
            assert np.array_equal(got, ref.resolve(want, 1, dt0, lo=0.0, hi=0.1, lut=view.sequential_lut()))
        else:
            assert len(np.unique(got.reshape(-1, 3), axis=0)) > 3            # moving instances and the still world differ
    # --instance: only those instances are drawn, and the fitted camera frames them
    chosen = [int(i) for i in np.unique(frame["flow_instance_id"][(frame["flow_instance_id"] > 0) & (skip == 0)])[:2]]
    fitted = view.auto_camera(frame, 64, 48, instances=chosen)
    image, info, buffers = view.render_frame(frame, ["raw"], "label:flow_instance_id", fitted, r, instances=chosen, return_buffers=True)
    member = np.isin(frame["flow_instance_id"], chosen) & (skip == 0)
    assert info["points"] == [int(member.sum())] and info["pixels"][0] > 0
    low = buffers[0].cpu().numpy().view(np.uint64)
    assert member[(low[low != ref.EMPTY] & np.uint64(0xFFFFFFFF)).astype(np.int64)].all()
    want = ref.clear(64, 48)
    assert ref.splat(want, frame["pc0"][member, :3], ref.from_ctypes(fitted), radius=1) == int(member.sum())        # all inside the view


# ---- the program -------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(gpu, tmp_path, capsys):
    from himo_amd import view
    from himo_amd.synthetic import make_scene, write_h5_scenes
    root = tmp_path / "scenes"
    root.mkdir()
    scenes = [make_scene(60 + s, 3, n_points=3000, scene_id=f"vw{s}") for s in range(2)]       # 2 usable sweeps each
    write_h5_scenes(root, scenes)
    out = tmp_path / "out"
    listing = view._cli(f"--data_dir {root} --indices 0:2 --res_names raw,flow --color_by lidar --size 64x48 --out_dir {out}".split())
    assert "2 images" in capsys.readouterr().out
    on_disk = json.loads((out / "view.json").read_text())
    assert on_disk == listing and len(listing) == 2
    for entry, frame in zip(listing, scenes[0][:2]):
        assert entry["file"] == f"vw0_{frame['timestamp']}.png" and entry["panels"] == ["raw", "flow"] and entry["scene_id"] == "vw0"
        assert entry["camera"]["ortho"] and entry["camera"]["width"] == 64 and len(entry["points"]) == len(entry["pixels"]) == 2
        assert entry["points"][0] == entry["points"][1] > 1000 and min(entry["pixels"]) > 100
        image = decode_png((out / entry["file"]).read_bytes())
        assert image.shape == (48, 2 * 64 + view.SEPARATOR_PX, 3)
        left, right = image[:, :64], image[:, 66:]
        assert left.any() and right.any() and (image[:, 64:66] == (0x40, 0x40, 0x40)).all()
        assert int((left.reshape(-1, 3) != 0).any(axis=1).sum()) == entry["pixels"][0]
        assert not np.array_equal(left, right)                          # the scene has moving instances: compensation moves them
    # --scene counts within that scene; a camera path of three keyframes with --sample_step 2 writes five numbered frames
    keys = [{"front": [0.3 * k, -1.0, 0.8], "lookat": [5.0 * k, 0.0, 0.0], "up": [0, 0, 1], "zoom": 0.8 + 0.1 * k} for k in range(3)]
    (tmp_path / "path.json").write_text(json.dumps(keys))
    path_out = tmp_path / "path"
    listing = view._cli(f"--data_dir {root} --scene vw1 --index 1 --res_names flow --color_by label:flow_instance_id --camera {tmp_path / 'path.json'} "
                        f"--sample_step 2 --size 64x48 --point_px 2 --edl 1.0 --out_dir {path_out}".split())
    assert [e["file"] for e in listing] == [f"{k:05d}.png" for k in range(5)] and sorted(p.name for p in path_out.glob("*.png")) == [e["file"] for e in listing]
    assert all(e["scene_id"] == "vw1" and e["timestamp"] == scenes[1][1]["timestamp"] and not e["camera"]["ortho"] for e in listing)
    frames = [decode_png((path_out / e["file"]).read_bytes()) for e in listing]
    assert all(f.shape == (48, 64, 3) and f.any() for f in frames) and not np.array_equal(frames[0], frames[4])
    # one keyframe is a fixed camera; --camera auto fits the view
    (tmp_path / "one.json").write_text(json.dumps(keys[0]))
    listing = view._cli(f"--data_dir {root} --index 0 --res_names raw --camera {tmp_path / 'one.json'} --size 32x32 --out_dir {tmp_path / 'one'}".split())
    assert [e["file"] for e in listing] == [f"vw0_{scenes[0][0]['timestamp']}.png"]
    listing = view._cli(f"--data_dir {root} --index 0 --res_names raw,flow --color_by overlay --camera auto --size 32x32 --out_dir {tmp_path / 'auto'}".split())
    assert listing[0]["panels"] == ["raw+flow"] and decode_png((tmp_path / "auto" / listing[0]["file"]).read_bytes()).shape == (32, 32, 3)
    # what the scene does not hold is an error that names it
    capsys.readouterr()
    with pytest.raises(KeyError, match="seflowpp_best"):
        view._cli(f"--data_dir {root} --index 0 --res_names raw,seflowpp_best --size 32x32 --out_dir {tmp_path / 'no'}".split())
    assert "[Warning]: No seflowpp_best in vw0 at" in capsys.readouterr().out
    with pytest.raises(KeyError, match="ray_label"):
        view._cli(f"--data_dir {root} --index 0 --res_names raw --color_by label:ray_label --size 32x32 --out_dir {tmp_path / 'no'}".split())
    with pytest.raises(IndexError):
        view._cli(f"--data_dir {root} --index 99 --res_names raw --size 32x32 --out_dir {tmp_path / 'no'}".split())
    with pytest.raises(ValueError):
        view._cli(f"--data_dir {root} --indices 0:2 --res_names raw --camera {tmp_path / 'path.json'} --size 32x32 --out_dir {tmp_path / 'no'}".split())
