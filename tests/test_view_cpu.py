"""The headless viewer without a GPU: the numpy restatement of "point splat, v1" (tests/render_ref.py) on hand-worked cases of a
7 x 5 image, the camera constructors, ``spline_path`` against scipy's clamped cubic spline, ``write_png`` through a decoder written
here, the program's argument parsing and its error for a key the scene does not hold."""
import struct
import zlib

import numpy as np
import pytest

import render_ref as ref
from himo_amd.view import Camera

W, H = 7, 5
IDENT = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]


def ortho_cam(width=W, height=H, near=1.0, far=9.0):
    """u = x, v = y, depth = z: a point's coordinates ARE its screen position.  Built as the product builds a camera (the ctypes
    mirror and its float32 ``inv_range``), read back as the restatement's dict."""
    cam = ref.from_ctypes(Camera.make(IDENT, True, 1.0, 1.0, 0.0, 0.0, near, far, width, height))
    assert cam == {**ref.camera(IDENT, True, 1.0, 1.0, 0.0, 0.0, near, far, width, height), "m": cam["m"]} and np.array_equal(cam["m"], np.float32(IDENT))
    return cam


def pinhole_cam(width=W, height=H, near=1.0, far=9.0, f=2.0):
    cam = ref.from_ctypes(Camera.make(IDENT, False, f, f, width / 2.0, height / 2.0, near, far, width, height))
    assert cam["inv_range"] == ref.camera(IDENT, False, f, f, width / 2.0, height / 2.0, near, far, width, height)["inv_range"]
    return cam


def drawn(vis):
    return {(int(x), int(y)): (int(vis[y, x] >> np.uint64(32)), int(vis[y, x] & np.uint64(0xFFFFFFFF)))
            for y, x in zip(*np.nonzero(vis != ref.EMPTY))}


def one(points, cam=None, **kw):
    vis = ref.clear(W, H)
    ref.splat(vis, np.asarray(points, np.float32).reshape(-1, 3), cam if cam is not None else ortho_cam(), **kw)
    return drawn(vis)


# the hand-worked cases, shared with tests/test_view_gpu.py: (name, points, radius)
HAND_CASES = [
    ("pixel corner", [[3.0, 2.0, 5.0]], 0),
    ("just inside the corner's left neighbour", [[np.nextafter(np.float32(3.0), np.float32(0.0)), 2.0, 5.0]], 0),
    ("at near and at far", [[1.0, 1.0, 1.0], [2.0, 1.0, 9.0]], 0),
    ("beyond near and far", [[1.0, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0))], [2.0, 1.0, np.nextafter(np.float32(9.0), np.float32(10.0))]], 0),
    ("behind the camera", [[3.0, 2.0, -5.0]], 1),
    ("nan and inf", [[np.nan, 2.0, 5.0], [3.0, np.inf, 5.0], [3.0, 2.0, np.nan], [-np.inf, 2.0, 5.0], [3.0, 2.0, np.inf]], 1),
    ("off-screen by less than the radius", [[-1.5, 2.5, 5.0], [8.5, 5.9, 5.0]], 2),
    ("off-screen by the radius + 1", [[-3.0, 2.5, 5.0], [np.nextafter(np.float32(-3.0), np.float32(-4.0)), 2.5, 5.0], [10.0, 2.5, 5.0]], 2),
    ("equal zq", [[3.5, 2.5, 5.0], [3.25, 2.75, 5.0], [3.75, 2.25, 5.0]], 1),
    ("nearer wins", [[3.5, 2.5, 5.0], [3.5, 2.5, 4.0]], 0),
]


def test_a_point_on_a_pixel_corner_belongs_to_the_pixel_it_starts():
    assert one(HAND_CASES[0][1]) == {(3, 2): (8388608, 0)}                    # (5 - 1) / 8 * 2^24
    assert one(HAND_CASES[1][1]) == {(2, 2): (8388608, 0)}


def test_near_and_far_are_inside_the_next_float_is_not():
    assert one(HAND_CASES[2][1]) == {(1, 1): (0, 0), (2, 1): (2 ** 24 - 1, 1)}  # zq = 2^24 at far, clamped
    assert one(HAND_CASES[3][1]) == {}


def test_behind_the_camera_and_non_finite_points_draw_nothing():
    assert one(HAND_CASES[4][1], radius=1) == {} and one(HAND_CASES[4][1], pinhole_cam(), radius=1) == {}
    assert one(HAND_CASES[5][1], radius=1) == {} and one(HAND_CASES[5][1], pinhole_cam(), radius=1) == {}
    # a pinhole with near <= 0 meets zc == 0: the quotient is not finite, the point is dropped
    assert one([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]], pinhole_cam(near=-1.0)) == {}


def test_a_footprint_off_screen_is_clipped():
    got = one(HAND_CASES[6][1][:1], radius=2)                                # pixel (-2, 2): only dx = +2 reaches column 0
    assert set(got) == {(0, 2)}
    got = one(HAND_CASES[6][1][1:], radius=2)                                # pixel (8, 5): dx^2 + dy^2 <= 4 reaches (6, 5)? no row 5
    assert got == {}                                                         # (7 + 0 columns; row 5 is outside: (7, 4) and (8, 3) too)
    got = one([[7.5, 4.5, 5.0]], radius=2)                                   # pixel (7, 4): (6, 4), (6, 3), (5, 4) lie inside
    assert set(got) == {(6, 4), (6, 3), (5, 4)}
    # at -(radius + 1) exactly the point is still taken (and reaches nothing); one float below it is dropped: same picture
    assert one(HAND_CASES[7][1], radius=2) == {}
    vis = ref.clear(W, H)
    assert ref.splat(vis, np.asarray(HAND_CASES[7][1], np.float32), ortho_cam(), radius=2) == 1


def test_equal_depth_goes_to_the_lowest_index_and_a_nearer_point_wins():
    got = one(HAND_CASES[8][1], radius=1)
    assert len(got) == 5 and all(v == (8388608, 0) for v in got.values())
    got = one(HAND_CASES[8][1], radius=1, index_base=7)
    assert all(v == (8388608, 7) for v in got.values())
    got = one(HAND_CASES[8][1][::-1], radius=1, skip=[0, 0, 1])
    assert all(v[1] == 0 for v in got.values())
    assert one(HAND_CASES[9][1]) == {(3, 2): (3 * 2 ** 21, 1)}


@pytest.mark.parametrize("radius,count", [(0, 1), (1, 5), (2, 13), (3, 29)])
def test_disc_footprints_counted_by_hand(radius, count):
    assert len(ref.disc(radius)) == count
    vis = ref.clear(15, 15)
    ref.splat(vis, np.array([[7.5, 7.5, 5.0]], np.float32), ortho_cam(15, 15), radius=radius)
    assert int((vis != ref.EMPTY).sum()) == count
    ys, xs = np.nonzero(vis != ref.EMPTY)
    assert ((xs - 7) ** 2 + (ys - 7) ** 2 <= radius * radius).all()


def test_offset_is_added_first_and_the_split_over_calls_does_not_matter():
    rng = np.random.default_rng(1)
    pts = rng.uniform((-1, -1, 0), (8, 6, 10), (400, 3)).astype(np.float32)
    off = rng.normal(0, 0.3, (400, 3)).astype(np.float32)
    a, b, c = ref.clear(W, H), ref.clear(W, H), ref.clear(W, H)
    ref.splat(a, pts, ortho_cam(), radius=1, offset=off)
    ref.splat(b, (pts + off).astype(np.float32), ortho_cam(), radius=1)
    ref.splat(c, pts[250:], ortho_cam(), radius=1, offset=off[250:], index_base=250)
    ref.splat(c, pts[:250], ortho_cam(), radius=1, offset=off[:250])
    assert np.array_equal(a, b) and np.array_equal(a, c) and (a != ref.EMPTY).all()


def test_resolve_modes_by_hand():
    vis = ref.clear(3, 1)
    vis[0, 0], vis[0, 1] = np.uint64(5 << 32 | 0), np.uint64(9 << 32 | 1)
    lut = np.arange(256, dtype=np.uint32)
    got = ref.resolve(vis, 1, np.array([-3.0, np.nan], np.float32), background=0x010203, neutral=0x0A0B0C, lo=0.0, hi=1.0, lut=lut)
    assert got.tolist() == [[[0, 0, 0], [12, 11, 10], [3, 2, 1]]]
    got = ref.resolve(vis, 1, np.array([0.5, 77.0], np.float32), lo=0.0, hi=1.0, lut=lut)
    assert got[0, :2, 0].tolist() == [128, 255]
    got = ref.resolve(vis, 2, np.array([7, -1], np.int32), palette=[1, 2, 3], neutral=9)
    assert got[0, :2, 0].tolist() == [2, 9]
    got = ref.resolve(vis, 0, np.array([0xFFFFFF], np.uint32), neutral=9)                  # index 1 has no attribute behind it
    assert got[0, :2].tolist() == [[255, 255, 255], [9, 0, 0]]
    # eye-dome lighting darkens a pixel that lies BEHIND a neighbour (zq 9 beside zq 5: 255 * 2^-(log2(10 / 6) / 4) = 224.4), never the
    # nearer one, never for an empty neighbour or one outside the image, and never an empty pixel
    flat = ref.resolve(vis, 0, np.array([0xFFFFFF, 0xFFFFFF], np.uint32), edl=1.0)
    assert flat[0, 0].tolist() == [255, 255, 255] and flat[0, 1].tolist() == [224, 224, 224] and flat[0, 2].tolist() == [0, 0, 0]
    vis[0, 1] = np.uint64((2 ** 24 - 1) << 32 | 1)
    lit = ref.resolve(vis, 0, np.array([0xFFFFFF, 0xFFFFFF], np.uint32), edl=1.0)
    want = np.floor(255 * 2.0 ** (-(24 - np.log2(6.0)) / 4) + 0.5)                        # against the nearer pixel on its left only
    assert lit[0, 0, 0] == 255 and abs(int(lit[0, 1, 0]) - int(want)) <= 1


# ---- cameras -----------------------------------------------------------------------------------------------------------------------
def project(cam, p, radius=0):
    assert isinstance(cam, Camera)
    c = ref.from_ctypes(cam)
    vis = ref.clear(c["width"], c["height"])
    ref.splat(vis, np.asarray(p, np.float32).reshape(1, 3), c, radius=radius)
    ys, xs = np.nonzero(vis != ref.EMPTY)
    return [(int(x), int(y)) for x, y in zip(xs, ys)]


def test_look_at_is_a_rotation_and_looks_at_its_target():
    rng = np.random.default_rng(5)
    for _ in range(20):
        eye, target = rng.uniform(-30, 30, 3), rng.uniform(-30, 30, 3)
        cam = Camera.look_at(eye, target, up=(0.1, -0.2, 1.0), fov_y_deg=50, width=65, height=49, near=0.1, far=200.0)
        m = np.array(list(cam.m), np.float64).reshape(3, 4)
        assert np.abs(m[:, :3] @ m[:, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(m[:, :3]) - 1.0) < 1e-6
        assert np.abs(m[:, :3] @ eye + m[:, 3]).max() < 1e-4                    # the eye is the origin
        assert project(cam, target) == [(32, 24)]                                # the target sits in the middle pixel
        assert project(cam, 2 * eye - target) == []                              # and what lies behind is not drawn
    cam = Camera.look_at((-10, 0, 0), (0, 0, 0), up=(0, 0, 1), width=65, height=49)
    (x0, y0), (x1, y1), (x2, y2) = project(cam, (0, 0, 0))[0], project(cam, (0, 0, 2))[0], project(cam, (0, 2, 0))[0]
    assert y1 < y0 and x1 == x0 and x2 < x0 and y2 == y0                         # up is up; looking along +x, +y is to the left
    assert cam.inv_range == np.float32(1.0) / (np.float32(200.0) - np.float32(0.1))
    with pytest.raises(ValueError):
        Camera.look_at((0, 0, 0), (0, 0, 5), up=(0, 0, 1))
    with pytest.raises(ValueError):
        Camera.look_at((0, 0, 0), (0, 0, 0))


def test_bev_maps_its_centre_to_the_image_centre_and_y_up():
    for w, h in ((7, 5), (64, 48), (1, 1)):
        cam = Camera.bev((12.5, -3.0), 10.0, w, h, z_range=(-2.0, 6.0))
        assert cam.ortho == 1 and project(cam, (12.5, -3.0, 0.0)) == [(w // 2, h // 2)]
        assert project(cam, (12.5, -3.0, 6.5)) == [] and project(cam, (12.5, -3.0, -2.5)) == []
    cam = Camera.bev((12.5, -3.0), 10.0, 64, 48, z_range=(-2.0, 6.0))
    (cx, cy), (ux, uy), (rx, ry) = project(cam, (12.5, -3.0, 0))[0], project(cam, (12.5, 2.0, 0))[0], project(cam, (17.5, -3.0, 0))[0]
    assert uy < cy and ux == cx                                                  # +y is up
    assert rx > cx and ry == cy                                                  # +x is right
    assert project(cam, (12.5, 6.9, 0)) != [] and project(cam, (12.5, 7.1, 0)) == []       # 10 m reach the nearer edge
    vis = ref.clear(64, 48)                                                      # seen from above, the higher point is the nearer one
    ref.splat(vis, np.array([[12.5, -3.0, 1.0], [12.5, -3.0, 5.0]], np.float32), ref.from_ctypes(cam))
    assert int(vis[24, 32] & np.uint64(0xFFFFFFFF)) == 1


def test_from_view_places_the_eye_zoom_scene_radii_along_front():
    cam = Camera.from_view((0, 0, 2), (1, 2, 3), (0, 1, 0), zoom=0.5, scene_radius=40.0, width=33, height=33)
    m = np.array(list(cam.m), np.float64).reshape(3, 4)
    eye = -m[:, :3].T @ m[:, 3]
    assert np.allclose(eye, (1, 2, 23), atol=1e-5) and project(cam, (1, 2, 3)) == [(16, 16)]
    assert cam.zfar == np.float32(20.0 + 80.0)
    with pytest.raises(ValueError):
        Camera.from_view((0, 0, 1), (0, 0, 0), (0, 1, 0), zoom=0.0)


# ---- the camera path ---------------------------------------------------------------------------------------------------------------
def test_spline_path_equals_scipys_clamped_cubic_spline():
    scipy_interpolate = pytest.importorskip("scipy.interpolate")
    from himo_amd.view import KEYFRAME_KEYS, spline_path
    rng = np.random.default_rng(11)
    for n, step in ((2, 5), (3, 2), (4, 10), (9, 7)):
        keys = [{"front": rng.uniform(-1, 1, 3).tolist(), "lookat": rng.uniform(-1, 1, 3).tolist(), "up": rng.uniform(-1, 1, 3).tolist(),
                 "zoom": float(rng.uniform(0.1, 1.0))} for _ in range(n)]
        got = spline_path(keys, step)
        assert len(got) == n * step - (step - 1)
        t = np.linspace(0, n - 1, len(got))
        for name in KEYFRAME_KEYS:
            want = scipy_interpolate.CubicSpline(np.arange(n), np.array([k[name] for k in keys]), bc_type="clamped")(t)
            assert np.abs(np.array([g[name] for g in got]) - want).max() <= 1e-9, (n, step, name)
        assert got[0] == {k: keys[0][k] for k in KEYFRAME_KEYS} and np.allclose(got[-1]["front"], keys[-1]["front"], atol=1e-12)


def test_spline_path_counts_and_refusals():
    from himo_amd.view import spline_path
    key = {"front": [0, 0, 1], "lookat": [0, 0, 0], "up": [0, 1, 0], "zoom": 0.7}
    assert len(spline_path([key], 4)) == 1 and len(spline_path([key, key, key], 2)) == 5 and len(spline_path([key, key], 1)) == 2
    assert all(k["zoom"] == pytest.approx(0.7) for k in spline_path([key, key, key], 3))
    with pytest.raises(ValueError):
        spline_path([], 3)
    with pytest.raises(ValueError):
        spline_path([key], 0)
    with pytest.raises(KeyError):
        spline_path([{"front": [0, 0, 1]}], 2)


def test_the_product_imports_neither_scipy_nor_pil():
    from conftest import REPO
    src = (REPO / "himo_amd" / "view.py").read_text()
    assert "import scipy" not in src and "from scipy" not in src and "import PIL" not in src and "from PIL" not in src
    assert "open3d" not in [line.split()[1] for line in src.splitlines() if line.startswith(("import ", "from "))]


# ---- PNG ---------------------------------------------------------------------------------------------------------------------------
def decode_png(data: bytes) -> np.ndarray:
    """the files ``write_png`` promises: 8-bit RGB, not interlaced, filter 0 on every row, one IDAT; every CRC is checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        (length,) = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + length]
        (crc,) = struct.unpack(">I", data[at + 8 + length:at + 12 + length])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        at += 12 + length
    assert at == len(data) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3).copy()


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (300, 200)])
def test_write_png_round_trip(tmp_path, w, h):
    from himo_amd.view import write_png
    rgb = np.random.default_rng(w * h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb[0, 0] = (0, 255, 10)
    write_png(tmp_path / "a.png", rgb)
    assert np.array_equal(decode_png((tmp_path / "a.png").read_bytes()), rgb)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(tmp_path / "a.png") as im:
            assert im.mode == "RGB" and im.size == (w, h) and np.array_equal(np.asarray(im), rgb)
    import torch
    write_png(tmp_path / "b.png", torch.from_numpy(rgb))
    assert (tmp_path / "b.png").read_bytes() == (tmp_path / "a.png").read_bytes()
    for bad in (rgb[..., :2], rgb.astype(np.int32), rgb[0], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_png(tmp_path / "c.png", bad)


# ---- colour tables -----------------------------------------------------------------------------------------------------------------
def test_built_in_colour_tables():
    from himo_amd.view import PALETTE_HEX, palette, sequential_lut
    pal = palette()
    assert pal.dtype == np.uint32 and len(pal) == 6 == len(PALETTE_HEX) and pal[0] == 0x1b | 0x9e << 8 | 0x77 << 16
    lut = sequential_lut()
    assert lut.dtype == np.uint32 and lut.shape == (256,) and len(set(lut.tolist())) > 200 and (lut >> 24 == 0).all()
    rgb = np.stack([lut & 0xFF, (lut >> 8) & 0xFF, (lut >> 16) & 0xFF], axis=1).astype(np.float64)
    light = rgb @ (0.30, 0.59, 0.11)
    assert (np.diff(light) > -1.0).all() and light[0] < 60 and light[-1] > 220           # sequential: lightness rises (to rounding)


# ---- the program's arguments -------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    from himo_amd import view
    a = view._parser().parse_args("--data_dir D --index 270 --res_names raw,seflowpp_best,flow --color_by lidar --out_dir O".split())
    assert (a.data_dir, a.index, a.indices, a.out_dir, a.camera, a.size, a.point_px, a.edl) == ("D", 270, None, "O", "bev", "1024x768", 1, 0.0)
    assert a.sample_step == 10 and a.scene is None and not a.keep_ground and a.instance is None
    a = view._parser().parse_args("--data_dir D --out_dir O --indices 3:9 --camera k.json --sample_step 4 --size 64x48 --point_px 3 "
                                  "--edl 0.8 --scene s --color_by label:ray_label --keep_ground --instance 8,9".split())
    assert (a.indices, a.camera, a.sample_step, a.size, a.point_px, a.edl, a.scene, a.instance) == ("3:9", "k.json", 4, "64x48", 3, 0.8, "s", "8,9")
    with pytest.raises(SystemExit):
        view._parser().parse_args(["--index", "1"])
    assert view.parse_size("64x48") == (64, 48) and view.parse_indices(None, "3:9") == [3, 4, 5, 6, 7, 8] and view.parse_indices(4, None) == [4]
    for bad in ("64", "0x5", "axb", "3x4x5"):
        with pytest.raises(ValueError):
            view.parse_size(bad)
    for index, indices in ((None, None), (1, "1:2"), (None, "5:5"), (None, "x"), (None, "-1:3")):
        with pytest.raises(ValueError):
            view.parse_indices(index, indices)
    assert view.parse_color_by("label:ray_label") == ("label", "ray_label") and view.parse_color_by("speed") == ("speed", None)
    for bad in ("colour", "label:", "Lidar"):
        with pytest.raises(ValueError):
            view.parse_color_by(bad)
    assert view.required_keys(["raw", "flow"], "lidar") == ["pc0", "pose0", "pose1", "lidar_dt", "gm0", "flow", "lidar_id"]
    assert view.required_keys(["raw"], "label:ray_label", [8])[-2:] == ["ray_label", "flow_instance_id"]


def test_camera_files(tmp_path):
    import json
    from himo_amd.view import load_keyframes
    key = {"front": [0, 0, 1], "lookat": [0, 0, 0], "up": [0, 1, 0], "zoom": 0.7}
    for name, doc, count in (("one.json", key, 1), ("list.json", [key, key, key], 3), ("traj.json", {"trajectory": [key, key]}, 2)):
        (tmp_path / name).write_text(json.dumps(doc))
        assert len(load_keyframes(tmp_path / name)) == count
    (tmp_path / "bad.json").write_text(json.dumps([{"front": [0, 0, 1]}]))
    with pytest.raises(KeyError, match="lookat"):
        load_keyframes(tmp_path / "bad.json")
    (tmp_path / "none.json").write_text("[]")
    with pytest.raises(ValueError):
        load_keyframes(tmp_path / "none.json")


def test_a_key_the_scene_does_not_hold_is_an_error_that_names_it(capsys):
    from himo_amd import view
    from himo_amd.synthetic import make_scene
    frame = make_scene(3, 1, n_points=200, scene_id="v0")[0]
    for names, color_by, key in ((["raw", "nope_flow"], "lidar", "nope_flow"), (["raw"], "label:ray_label", "ray_label")):
        with pytest.raises(KeyError, match=key):
            view.render_frame(frame, names, color_by, view.Camera.bev(width=8, height=8))
        assert f"[Warning]: No {key} in v0 at {frame['timestamp']}, check the data." in capsys.readouterr().out
    with pytest.raises(ValueError):
        view.render_frame(frame, ["raw"], "colour", view.Camera.bev(width=8, height=8))
