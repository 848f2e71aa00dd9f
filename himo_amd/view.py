"""The headless viewer: a sweep as it was recorded beside the same sweep compensated by a stored flow, as PNG panels.

    python -m himo_amd.view --data_dir D --index 270 --res_names raw,seflowpp_best,flow --color_by lidar --out_dir O

The reference shows its clouds in open3d windows (``tools/view_instance.py``, ``tools/animation_video.py``, ``visualize.py``); this
program renders on the GPU and writes plain PNG files: no window system, no open3d, no PIL.  The renderer follows the build's own
written rule, below, and is checked bit for bit against a numpy restatement of it (``tests/render_ref.py``), never against another
viewer: NO CLAIM IS MADE ABOUT open3d's PIXELS.  Its timing is unmeasured.

The rule -- "point splat, v1" (normative)
==========================================
All float arithmetic is float32 and every operation rounds on its own (``himo_amd/csrc/render.hip`` is built with
``-ffp-contract=off``, without fast-math, with the correctly rounded division).

The visibility buffer is one uint64 per pixel, ``[height][width]``; an empty pixel is ``~0``, a hit ``(zq << 32) | point index``.
The camera (``Camera``, mirrored as ``himo_camera``) holds a 3x4 world -> camera matrix ``M`` (the camera looks along +z; x is
right, y is down in the image), ``ortho``, ``fx, fy, cx, cy``, ``znear``, ``zfar``, ``inv_range = 1 / (zfar - znear)`` computed in
float32 on the host, and ``width, height``.

A. Position.  ``p = pts[i] + offset[i]`` per component when an offset is given (``refine_pts`` fused in: a compensated cloud is
   never materialised).  A point whose skip byte is non-zero is not drawn.
B. Camera coordinates.  ``xc = ((M00 x + M01 y) + M02 z) + M03``, left to right; ``yc``, ``zc`` likewise.  Dropped when any of the
   three is not finite, ``zc < znear`` or ``zc > zfar``.
C. Screen.  Perspective ``u = fx (xc / zc) + cx``, ``v = fy (yc / zc) + cy``; orthographic ``u = fx xc + cx``, ``v = fy yc + cy``.
   Dropped when ``u`` or ``v`` is not finite or outside ``[-(radius + 1), extent + radius + 1)``, tested in float.  The pixel is
   ``(floor u, floor v)``.
D. Depth.  ``zq = min(2^24 - 1, floor(((zc - znear) * inv_range) * 16777216))``.
E. Write.  For every integer ``(dx, dy)`` with ``dx^2 + dy^2 <= radius^2`` (``radius`` 0..8: 1, 5, 13, 29 ... pixels) whose pixel
   lies inside the image: the 64-bit minimum of the pixel's word and ``(zq << 32) | (index_base + i)``.  So the nearest point
   wins, the lowest index among equal ``zq``; the buffer is a pure function of the set of (point, index), whatever the launch
   order and the split over calls; calls with different ``index_base`` accumulate several clouds into one image.
F. Colour.  An empty pixel takes ``background``.  A hit takes, by the key's low 32 bits ``idx`` (which is why overlaid clouds
   concatenate their attributes; an ``idx`` past the attribute array takes ``neutral``): mode 0 the uint32 ``r | g << 8 | b << 16``
   at ``idx``; mode 1 ``lut[clamp(floor((s - lo) * scale), 0, 255)]`` of the float32 scalar ``s`` (256 entries,
   ``scale = (float)256 / (hi - lo)``), ``neutral`` for a non-finite ``s``; mode 2 ``palette[id % P]`` of the int32 ``id``,
   ``neutral`` for a negative one.
G. Eye-dome lighting, when ``edl > 0`` (depth made readable in a flat-coloured cloud).  ``L = log2(1 + zq)``; an empty neighbour
   counts as ``L = 24``, one outside the image as the centre's own ``L``; ``resp`` = (the sum over the neighbours at
   ``(-e, 0), (+e, 0), (0, -e), (0, +e)``, in that order, of ``max(0, L_c - L_nb)``) / 4; ``shade = exp2(-edl * resp)``; every
   channel becomes ``floor(c * shade + 0.5)``.  (``log2`` / ``exp2`` differ from numpy's by a few ulp: a channel may differ from
   the restatement by one level here, nowhere else.)

The rule -- "line overlay, v1" (normative)
===========================================
Oriented boxes (``boxes_<name>``, with their velocities) and track trails (``tracks_<name>``) are drawn as line segments over the
panels.  PARITY UNPINNED: the reference has no such stage; the rule is this build's own and is checked bit for bit against
``tests/renderlines_ref.py``.  All float arithmetic is float32 and every operation rounds on its own
(``himo_amd/csrc/renderlines.hip`` is built with ``-ffp-contract=off``, without fast-math); everything after rule C is integer
arithmetic.

The overlay has ITS OWN buffer, ``lines``: one uint64 per pixel, ``[height][width]``; ``~0`` is empty, otherwise the word is
``(zq << 32) | segment index``.  ``himo_render_clear`` clears it.  The point buffer and ``himo_render_resolve`` are untouched by it.
A segment is a float32 row ``[6]`` = ``x0, y0, z0, x1, y1, z1`` in the frame the camera matrix reads; its ends are ``a`` and ``b``.

A. Camera coordinates.  Both ends by rule B of the point splat: the same expression in the same order.  The segment is dropped when
   any of the six values is not finite.
B. Depth clip.  Dropped when both ``zc < znear`` or both ``zc > zfar``.  Otherwise each end is replaced on its own, both replacements
   computed from the ORIGINAL pair, so that their order cannot matter.  End ``a`` with ``za < znear``: ``t = (znear - za) / (zb - za)``,
   ``xa' = xa + t * (xb - xa)``, ``ya' = ya + t * (yb - ya)``, ``za' = znear``; with ``za > zfar`` the same with ``zfar`` in place of
   ``znear``; otherwise unchanged.  End ``b`` symmetrically: ``t = (znear - zb) / (za - zb)``, ``xb' = xb + t * (xa - xb)``, ...
C. Screen.  Each end is projected by rule C of the point splat.  Dropped when any of ``u0, v0, u1, v1`` is not finite or has
   ``|.| >= 2^20`` (a documented limit of v1: it keeps everything below in exact integers).  The end pixels are ``X = floor(u)``,
   ``Y = floor(v)`` as int32; ``zq0`` and ``zq1`` by rule D of the point splat from the clipped ``zc``.
D. Pixels.  ``dx = X1 - X0``, ``dy = Y1 - Y0``, ``steps = max(|dx|, |dy|)``.  For ``k = 0 .. steps``, in int64 with FLOOR division:
   ``x_k = X0 + floordiv(2 k dx + steps, 2 steps)``, ``y_k`` likewise, ``zq_k = zq0 + floordiv(k (zq1 - zq0), steps)``; for
   ``steps = 0`` the one pixel ``(X0, Y0)`` with ``zq0``.  So ``k = 0`` is exactly end ``a`` and ``k = steps`` exactly end ``b``.  A half-way
   case rounds UP (towards +x, +y), whichever way the segment runs: ``x_k = floor(X0 + k dx / steps + 1/2)`` exactly, a function of the
   point alone, and ``floordiv((steps - k)(zq0 - zq1), steps) = floordiv(k (zq1 - zq0), steps) - (zq1 - zq0)``; so the walk from ``b`` to
   ``a`` visits the pixels and depths of the walk from ``a`` to ``b`` in reverse, and swapping the ends of a segment changes no bit (what
   is NOT symmetric is a reflection of the segment: the mirror image of a half-way pixel rounds the other way).  Depth is linear along
   the SCREEN segment; under a pinhole camera that is an approximation: THE OVERLAY MAKES NO CLAIM OF
   PERSPECTIVE-CORRECT DEPTH.
E. Write.  For every ``k`` and every ``(ddx, ddy)`` with ``ddx^2 + ddy^2 <= half_px^2`` (``half_px`` 0..3) whose pixel
   ``(x_k + ddx, y_k + ddy)`` lies inside the image: the 64-bit minimum of the word and ``(zq_k << 32) | (index_base + i)``.  The nearest
   segment wins, the lowest index among equal ``zq``; the buffer is a pure function of the set of (segment, index), whatever the launch
   order and the split over calls.
F. Composite, per pixel, onto an RGB image that ``himo_render_resolve`` has written.  An empty ``lines`` word leaves the three bytes
   alone.  With the depth test on, a non-empty point word whose ``zq`` is LESS than the line's leaves them alone too; on equal ``zq`` the
   line wins; an empty point word never hides a line.  Otherwise the pixel takes ``colors[idx]`` (uint32 ``r | g << 8 | b << 16``), or
   ``neutral`` when ``idx >= n_colors``.  Lines are not eye-dome shaded.

What is drawn (host code, float64, cast to float32 at the end): ``box_segments`` -- per box its 12 edges, a heading mark and, for a
MOVING box, a velocity arrow; ``trail_segments`` -- per tracked box the polyline of its id's stored positions over the last sweeps.
Not part of v1: perspective-correct line depth, anti-aliasing or alpha, text labels, filled faces or meshes, a 2-D clip of segments
beyond the 2^20 bound, trails from coasting tracks (``track`` v1 does not store them).  Nothing has been tried on field data.

Cameras.  ``Camera.bev``: orthographic, looking down, world x to the right and world y UP in the image.  ``Camera.look_at``: a
pinhole with a vertical field of view.  ``Camera.from_view`` takes the four quantities of the reference's camera keyframes
(``front``, ``lookat``, ``up``, ``zoom``; tools/animation_video.py:36) and maps them onto ``look_at``: the eye sits at
``lookat + zoom * scene_radius * front / |front|`` -- ``zoom`` is defined HERE as the eye's distance in scene radii; open3d's own
convention is not claimed.  ``spline_path`` is the clamped cubic spline through keyframes that ``interpolate_trajectory``
(tools/animation_video.py:32) describes, in numpy.

Not built: text in the image, video encoding, meshes, an interactive window, per-instance scores in the panel
(``himo_amd.eval`` prints those).  Many sweeps in one frame are a stage of their own: ``python -m himo_amd.accumulate`` writes them as
scene files, which ``--data_dir O --res_names raw`` then shows.
"""
from __future__ import annotations

import ctypes
import json
import struct
import zlib
from pathlib import Path

import numpy as np

EMPTY = -1                                   # the empty word ~0 as the int64 that torch holds the buffer in
SEPARATOR_PX = 2
WHITE, NEUTRAL, BACKGROUND, SEPARATOR = 0xFFFFFF, 0x808080, 0x000000, 0x404040
# the six-colour categorical palette of tools/view_instance.py:22
PALETTE_HEX = ("#1b9e77", "#d95f02", "#7570b3", "#e7298a", "#66a61e", "#e6ab02")
COLOR_BY = ("lidar", "dt0", "speed", "ground", "overlay")          # and "label:<key>"
DEFAULT_RANGE = {"dt0": (0.0, 0.1), "speed": (0.0, 20.0)}           # [s], [m/s]


def pack_rgb(r: int, g: int, b: int) -> int:
    return int(r) | int(g) << 8 | int(b) << 16


def palette() -> np.ndarray:
    """uint32[6]: ``PALETTE_HEX`` packed as rule F reads colours"""
    return np.array([pack_rgb(int(h[1:3], 16), int(h[3:5], 16), int(h[5:7], 16)) for h in PALETTE_HEX], dtype=np.uint32)


def sequential_lut() -> np.ndarray:
    """uint32[256]: a sequential colour table of monotonically rising lightness, by formula (the cubehelix scheme of Green 2011:
    a helix round the grey diagonal of the RGB cube; start 0.5, -1.5 rotations, hue 1, lightness 0.15 .. 0.95)"""
    lam = np.linspace(0.15, 0.95, 256)
    phi = 2.0 * np.pi * (0.5 / 3.0 + 1.0 - 1.5 * (np.arange(256) / 255.0))
    amp = 1.0 * lam * (1.0 - lam) / 2.0
    rgb = np.stack([lam + amp * (-0.14861 * np.cos(phi) + 1.78277 * np.sin(phi)),
                    lam + amp * (-0.29227 * np.cos(phi) - 0.90649 * np.sin(phi)),
                    lam + amp * (1.97294 * np.cos(phi))], axis=1)
    q = np.floor(np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint32)
    return (q[:, 0] | q[:, 1] << 8 | q[:, 2] << 16).astype(np.uint32)


# --------------------------------------------------------------------------------------------------------------------------
# cameras
# --------------------------------------------------------------------------------------------------------------------------
def _unit(v, what):
    v = np.asarray(v, dtype=np.float64).reshape(3)
    n = float(np.linalg.norm(v))
    if not np.isfinite(n) or n < 1e-12:
        raise ValueError(f"camera: {what} has no direction: {v.tolist()}")
    return v / n


class Camera(ctypes.Structure):
    """mirror of ``himo_camera`` (include/himo_amd.h)"""
    _fields_ = [("m", ctypes.c_float * 12), ("ortho", ctypes.c_int32), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("znear", ctypes.c_float), ("zfar", ctypes.c_float), ("inv_range", ctypes.c_float),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32)]

    @classmethod
    def make(cls, matrix, ortho, fx, fy, cx, cy, znear, zfar, width, height) -> "Camera":
        m = np.asarray(matrix, dtype=np.float32).reshape(12)
        znear, zfar = np.float32(znear), np.float32(zfar)
        if not (np.isfinite(znear) and np.isfinite(zfar) and zfar > znear):
            raise ValueError(f"camera: the depth range [{znear}, {zfar}] is empty")
        if int(width) < 1 or int(height) < 1:
            raise ValueError(f"camera: an image of {width} x {height}")
        inv_range = np.float32(1.0) / (zfar - znear)                  # float32, as the rule says
        return cls((ctypes.c_float * 12)(*m.tolist()), int(bool(ortho)), fx, fy, cx, cy, znear, zfar, inv_range, int(width), int(height))

    @classmethod
    def bev(cls, center_xy=(0.0, 0.0), half_extent_m: float = 51.2, width: int = 1024, height: int = 1024, z_range=(-5.0, 15.0)) -> "Camera":
        """orthographic, looking down from ``z_range[1]``: world x to the right, world y up; ``half_extent_m`` metres from the centre
        reach the nearer image edge"""
        zlo, zhi = float(z_range[0]), float(z_range[1])
        if not float(half_extent_m) > 0.0:
            raise ValueError(f"camera: half_extent_m={half_extent_m}")
        s = min(int(width), int(height)) / 2.0 / float(half_extent_m)
        cx0, cy0 = float(center_xy[0]), float(center_xy[1])
        m = [[1.0, 0.0, 0.0, -cx0], [0.0, -1.0, 0.0, cy0], [0.0, 0.0, -1.0, zhi]]
        return cls.make(m, True, s, s, width / 2.0, height / 2.0, 0.0, zhi - zlo, width, height)

    @classmethod
    def look_at(cls, eye, target, up=(0.0, 0.0, 1.0), fov_y_deg: float = 60.0, width: int = 1024, height: int = 768, near: float = 0.1,
                far: float = 200.0) -> "Camera":
        """a pinhole at ``eye`` looking at ``target``; ``fov_y_deg`` spans the image height"""
        eye = np.asarray(eye, dtype=np.float64).reshape(3)
        f = _unit(np.asarray(target, dtype=np.float64).reshape(3) - eye, "target - eye")
        r = _unit(np.cross(f, _unit(up, "up")), "front x up (up is parallel to the viewing direction)")
        d = np.cross(f, r)
        rot = np.stack([r, d, f])
        m = np.concatenate([rot, (-rot @ eye)[:, None]], axis=1)
        if not 0.0 < float(fov_y_deg) < 180.0:
            raise ValueError(f"camera: fov_y_deg={fov_y_deg}")
        focal = height / 2.0 / np.tan(np.deg2rad(float(fov_y_deg)) / 2.0)
        return cls.make(m, False, focal, focal, width / 2.0, height / 2.0, near, far, width, height)

    @classmethod
    def from_view(cls, front, lookat, up, zoom: float, scene_radius: float = 50.0, fov_y_deg: float = 60.0, width: int = 1024,
                  height: int = 768) -> "Camera":
        """a keyframe of the reference's camera files: the eye at ``lookat + zoom * scene_radius * front / |front|`` (``zoom`` = the
        eye's distance in scene radii: this module's definition), looking at ``lookat``"""
        dist = float(zoom) * float(scene_radius)
        if not dist > 0.0:
            raise ValueError(f"camera: zoom * scene_radius = {dist}")
        lookat = np.asarray(lookat, dtype=np.float64).reshape(3)
        eye = lookat + dist * _unit(front, "front")
        return cls.look_at(eye, lookat, up, fov_y_deg, width, height, near=max(0.05, dist * 1e-3), far=dist + 2.0 * float(scene_radius))

    def as_dict(self) -> dict:
        return {"matrix": [float(v) for v in self.m], "ortho": bool(self.ortho), "fx": float(self.fx), "fy": float(self.fy), "cx": float(self.cx),
                "cy": float(self.cy), "near": float(self.znear), "far": float(self.zfar), "width": int(self.width), "height": int(self.height)}


class Shade(ctypes.Structure):
    """mirror of ``himo_shade`` (include/himo_amd.h)"""
    _fields_ = [("mode", ctypes.c_int32), ("palette_n", ctypes.c_int32), ("rgba", ctypes.c_void_p), ("scalar", ctypes.c_void_p),
                ("ids", ctypes.c_void_p), ("lut", ctypes.c_void_p), ("palette", ctypes.c_void_p), ("n_attr", ctypes.c_int64),
                ("lo", ctypes.c_float), ("scale", ctypes.c_float), ("background", ctypes.c_uint32), ("neutral", ctypes.c_uint32),
                ("edl_strength", ctypes.c_float), ("edl_px", ctypes.c_int32)]


KEYFRAME_KEYS = ("front", "lookat", "up", "zoom")


def spline_path(keyframes, sample_step: int = 10) -> list:
    """The clamped cubic spline (zero first derivative at both ends, knots 0, 1, 2, ...) through the keyframes' ``front`` /
    ``lookat`` / ``up`` / ``zoom``, sampled ``sample_step`` times per interval: ``len * step - (step - 1)`` keyframes."""
    keyframes, step = list(keyframes), int(sample_step)
    if not keyframes or step < 1:
        raise ValueError(f"spline_path: {len(keyframes)} keyframes, sample_step={sample_step}")
    n = len(keyframes)
    y = np.array([np.concatenate([np.asarray(k[name], dtype=np.float64).reshape(-1) for name in KEYFRAME_KEYS]) for k in keyframes])
    if y.shape[1] != 10:
        raise ValueError("spline_path: a keyframe holds front[3], lookat[3], up[3] and zoom")
    count = n * step - (step - 1)
    if n == 1:
        out = np.repeat(y, count, axis=0)
    else:
        # the slopes s of the C2 piecewise cubic: s[0] = s[n-1] = 0, s[i-1] + 4 s[i] + s[i+1] = 3 (y[i+1] - y[i-1])
        a = np.zeros((n, n))
        rhs = np.zeros_like(y)
        a[0, 0] = a[n - 1, n - 1] = 1.0
        for i in range(1, n - 1):
            a[i, i - 1], a[i, i], a[i, i + 1] = 1.0, 4.0, 1.0
            rhs[i] = 3.0 * (y[i + 1] - y[i - 1])
        s = np.linalg.solve(a, rhs)
        t = np.linspace(0.0, n - 1.0, count)
        k = np.minimum(np.floor(t).astype(np.int64), n - 2)
        x = (t - k)[:, None]
        h00, h10 = (1.0 + 2.0 * x) * (1.0 - x) ** 2, x * (1.0 - x) ** 2
        h01, h11 = x * x * (3.0 - 2.0 * x), x * x * (x - 1.0)
        out = h00 * y[k] + h10 * s[k] + h01 * y[k + 1] + h11 * s[k + 1]
    return [{"front": row[0:3].tolist(), "lookat": row[3:6].tolist(), "up": row[6:9].tolist(), "zoom": float(row[9])} for row in out]


# --------------------------------------------------------------------------------------------------------------------------
# the renderer
# --------------------------------------------------------------------------------------------------------------------------
class Renderer:
    """Owns the visibility buffer and the output image of one ``width`` x ``height`` panel on ``device``.  Every call is a launch on
    the current stream; nothing waits.  ``max_points``: the highest point index + 1 a buffer may hold (``index_base + n``)."""

    def __init__(self, width: int, height: int, device=None, max_points: int = 1 << 24):
        import torch
        from . import _lib
        if int(width) < 1 or int(height) < 1:
            raise ValueError(f"Renderer: an image of {width} x {height}")
        self.lib = _lib.load()
        for name, mirror in (("himo_camera", Camera), ("himo_shade", Shade)):
            if self.lib.himo_abi_sizeof(name.encode()) != ctypes.sizeof(mirror):
                raise ImportError(f"{name}: the library's struct has {self.lib.himo_abi_sizeof(name.encode())} bytes, the mirror {ctypes.sizeof(mirror)}")
        self.width, self.height, self.max_points = int(width), int(height), int(max_points)
        self.device = device if device is not None else _lib.require_gpu()
        self._vis = torch.empty((self.height, self.width), dtype=torch.int64, device=self.device)
        self._rgb = torch.empty((self.height, self.width, 3), dtype=torch.uint8, device=self.device)
        self._lut = torch.from_numpy(sequential_lut().view(np.int32)).to(self.device)
        self._palette = torch.from_numpy(palette().view(np.int32)).to(self.device)
        self._top = 0
        self._lines = None                                        # the overlay's buffer: allocated by the first clear_lines() / lines()
        self._resolved = False
        self.clear()

    def clear(self) -> None:
        """empties the panel: the point buffer and, when one was allocated, the lines buffer (a renderer that never draws lines
        launches one clear)"""
        from . import _lib
        _lib.check(self.lib.himo_render_clear(self._vis.data_ptr(), self.width, self.height, _lib.stream_handle()), "himo_render_clear")
        self._top = 0
        if self._lines is not None:
            self.clear_lines()

    def clear_lines(self) -> None:
        """empties the lines buffer of "line overlay, v1" (allocated here on first use); the point buffer stays"""
        import torch
        from . import _lib
        if self._lines is None:
            self._lines = torch.empty((self.height, self.width), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.himo_render_clear(self._lines.data_ptr(), self.width, self.height, _lib.stream_handle()), "himo_render_clear")

    def lines(self, segments, half_px: int = 0, index_base: int = 0, camera: Camera | None = None) -> None:
        """Add segments to the lines buffer (rules A-E of "line overlay, v1"): ``segments`` (n, 6) float32 rows ``x0, y0, z0, x1, y1,
        z1`` (array or tensor), ``half_px`` 0..3 the disc radius round every pixel of the walk, ``index_base`` the index of the first
        segment in the buffer's keys (``composite`` reads ``colors`` by it)."""
        import torch
        from . import _lib
        if camera is None:
            raise ValueError("lines: a camera is required")
        if (int(camera.width), int(camera.height)) != (self.width, self.height):
            raise ValueError(f"lines: the camera renders {camera.width} x {camera.height}, the buffer is {self.width} x {self.height}")
        seg = self._on_device(segments, torch.float32, None, "segments")
        if seg.dim() != 2 or seg.shape[1] != 6:
            raise ValueError(f"segments are rows of x0, y0, z0, x1, y1, z1, not {tuple(seg.shape)}")
        n = int(seg.shape[0])
        if not 0 <= int(index_base) <= int(index_base) + n <= 1 << 32:
            raise ValueError(f"lines: segments {index_base}..{int(index_base) + n} do not fit the 32 index bits of a key")
        if self._lines is None:
            self.clear_lines()
        _lib.check(self.lib.himo_render_lines(n, _lib.ptr(seg), ctypes.addressof(camera), int(half_px), int(index_base), self._lines.data_ptr(),
                                              _lib.stream_handle()), "himo_render_lines")

    def composite(self, colors, depth_test: bool = False, neutral: int = NEUTRAL):
        """Rule F of "line overlay, v1": the lines buffer over the image the last ``resolve`` returned, which is written in place and
        returned.  ``colors``: uint32 ``r | g << 8 | b << 16`` per segment index (an index past it takes ``neutral``); ``depth_test``:
        a nearer point hides a line (the default draws lines on top)."""
        import torch
        from . import _lib
        if not self._resolved:
            raise ValueError("composite: nothing was resolved yet: lines are drawn over the image resolve() made")
        if self._lines is None:
            self.clear_lines()
        t = colors if isinstance(colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint32).view(np.int32))
        col = self._on_device(t, torch.int32, None, "colors")
        if col.dim() != 1:
            raise ValueError(f"colors are one uint32 per segment index, not {tuple(col.shape)}")
        _lib.check(self.lib.himo_render_composite(self._lines.data_ptr(), self._vis.data_ptr() if depth_test else None, self.width, self.height,
                                                  _lib.ptr(col) if col.numel() else None, int(col.numel()), int(neutral), self._rgb.data_ptr(),
                                                  _lib.stream_handle()), "himo_render_composite")
        return self._rgb

    def line_buffer(self):
        """the raw lines buffer, (H, W) int64 on the device holding the uint64 words (``EMPTY`` = -1), as ``visibility()`` is for
        the points; None before the first ``clear_lines()`` / ``lines()``"""
        return self._lines

    def _on_device(self, a, dtype, shape, what):
        import torch
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype == torch.bool and dtype == torch.uint8:
            t = t.to(torch.uint8)
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} is {tuple(shape)}, not {tuple(t.shape)}")
        return t

    def splat(self, points, offset=None, skip=None, radius: int = 1, index_base: int = 0, camera: Camera | None = None) -> None:
        """Add a cloud: ``points`` (n, >= 3) float32 rows (array or tensor), ``offset`` (n, 3) added on the device, ``skip`` (n,)
        non-zero = not drawn, ``radius`` 0..8 pixels, ``index_base`` the index of its first point in the buffer's keys."""
        import torch
        from . import _lib
        if camera is None:
            raise ValueError("splat: a camera is required")
        if (int(camera.width), int(camera.height)) != (self.width, self.height):
            raise ValueError(f"splat: the camera renders {camera.width} x {camera.height}, the buffer is {self.width} x {self.height}")
        pts = self._on_device(points, torch.float32, None, "points")
        if pts.dim() != 2 or pts.shape[1] < 3:
            raise ValueError(f"points are rows of x, y, z[, ...], not {tuple(pts.shape)}")
        n = int(pts.shape[0])
        if not 0 <= int(index_base) <= int(index_base) + n <= self.max_points:
            raise ValueError(f"splat: points {index_base}..{int(index_base) + n} in a renderer of max_points={self.max_points}")
        off = None if offset is None else self._on_device(offset, torch.float32, (n, 3), "offset")
        sk = None if skip is None else self._on_device(skip, torch.uint8, (n,), "skip")
        _lib.check(self.lib.himo_render_splat(n, _lib.ptr(pts), int(pts.shape[1]), _lib.ptr(off), _lib.ptr(sk), ctypes.addressof(camera),
                                              int(radius), int(index_base), self._vis.data_ptr(), _lib.stream_handle()), "himo_render_splat")
        self._top = max(self._top, int(index_base) + n)

    def resolve(self, colors=None, scalar=None, ids=None, edl: float = 0.0, edl_px: int = 1, background: int = BACKGROUND,
                neutral: int = NEUTRAL):
        """The (H, W, 3) uint8 device image of the buffer (the renderer's own tensor: the next ``resolve`` overwrites it).  Exactly one
        of ``colors`` (uint32 ``r | g << 8 | b << 16`` per point), ``scalar=(values, lo, hi[, lut])`` and ``ids=(ids[, palette])``;
        the arrays are indexed by point index, so they cover every index splatted since ``clear()``."""
        import torch
        from . import _lib
        if sum(x is not None for x in (colors, scalar, ids)) != 1:
            raise ValueError("resolve: exactly one of colors=, scalar=, ids=")
        sh = Shade(background=int(background), neutral=int(neutral), edl_strength=float(edl), edl_px=int(edl_px))
        keep = []
        if colors is not None:
            t = colors if isinstance(colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint32).view(np.int32))
            attr = self._on_device(t, torch.int32, None, "colors")
            sh.mode, sh.rgba = 0, attr.data_ptr()
        elif scalar is not None:
            values, lo, hi = scalar[:3]
            lut = self._lut if len(scalar) < 4 or scalar[3] is None else self._on_device(np.asarray(scalar[3], dtype=np.uint32).view(np.int32), torch.int32, (256,), "lut")
            attr = self._on_device(values, torch.float32, None, "scalar")
            lo, hi = np.float32(lo), np.float32(hi)
            if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
                raise ValueError(f"resolve: the scalar range [{lo}, {hi}] is empty")
            sh.mode, sh.scalar, sh.lut, sh.lo, sh.scale = 1, attr.data_ptr(), lut.data_ptr(), lo, np.float32(256.0) / (hi - lo)
            keep.append(lut)
        else:
            ids = ids if isinstance(ids, (tuple, list)) else (ids,)
            pal = self._palette if len(ids) < 2 or ids[1] is None else self._on_device(np.asarray(ids[1], dtype=np.uint32).view(np.int32), torch.int32, None, "palette")
            attr = self._on_device(ids[0], torch.int32, None, "ids")
            sh.mode, sh.ids, sh.palette, sh.palette_n = 2, attr.data_ptr(), pal.data_ptr(), int(pal.numel())
            keep.append(pal)
        if attr.dim() != 1 or attr.numel() < self._top:
            raise ValueError(f"resolve: {attr.numel()} attributes for the {self._top} point indices in the buffer")
        sh.n_attr = int(attr.numel())
        _lib.check(self.lib.himo_render_resolve(self._vis.data_ptr(), self.width, self.height, ctypes.addressof(sh), self._rgb.data_ptr(),
                                                _lib.stream_handle()), "himo_render_resolve")
        self._resolved = True
        return self._rgb

    def visibility(self):
        """the raw buffer, (H, W) int64 on the device holding the uint64 words (``EMPTY`` = -1; ``.cpu().numpy().view(np.uint64)``):
        the low 32 bits of a hit answer "which point is under this pixel\""""
        return self._vis


# --------------------------------------------------------------------------------------------------------------------------
# one frame -> panels
# --------------------------------------------------------------------------------------------------------------------------
def parse_color_by(color_by: str):
    """-> (kind, key): ("label", "<key>") for ``label:<key>``, else (kind, None)"""
    if color_by.startswith("label:") and len(color_by) > 6:
        return "label", color_by[6:]
    if color_by not in COLOR_BY:
        raise ValueError(f"--color_by {color_by!r}: one of {', '.join(COLOR_BY)} or label:<key>")
    return color_by, None


def required_keys(res_names, color_by: str, instances=None) -> list:
    """the frame keys ``render_frame`` reads for these options (what the program asks the loader for, and checks)"""
    kind, key = parse_color_by(color_by)
    keys = ["pc0", "pose0", "pose1", "lidar_dt", "gm0"] + [n for n in res_names if n != "raw"]
    keys += {"lidar": ["lidar_id"], "label": [key]}.get(kind, [])
    keys += ["flow_instance_id"] if instances else []
    return list(dict.fromkeys(keys))


def _need(data: dict, key: str):
    if key not in data:
        print(f"[Warning]: No {key} in {data.get('scene_id')} at {data.get('timestamp')}, check the data.")
        raise KeyError(key)
    return data[key]


def frame_skip(data: dict, keep_ground: bool = False, instances=None):
    """uint8 device tensor: the points of the sweep that are not drawn -- ground (``gm0``; kept with ``keep_ground``), the ego
    vehicle's own returns (``utils.ego_pts_mask``) and, with ``instances``, everything outside those ``flow_instance_id``s"""
    import torch
    from . import _lib, utils
    dev = _lib.require_gpu()
    pc0 = torch.from_numpy(np.ascontiguousarray(_need(data, "pc0"), dtype=np.float32)).to(dev)
    skip = ~utils.ego_pts_mask(pc0)
    if not keep_ground:
        skip |= torch.from_numpy(np.ascontiguousarray(_need(data, "gm0")).astype(bool)).to(dev)
    if instances:
        inst = torch.from_numpy(np.ascontiguousarray(_need(data, "flow_instance_id")).astype(np.int64)).to(dev)
        skip |= ~torch.isin(inst, torch.tensor([int(i) for i in instances], dtype=torch.int64, device=dev))
    return pc0, skip.to(torch.uint8)


def auto_camera(data: dict, width: int, height: int, keep_ground: bool = False, instances=None) -> Camera:
    """a bird's-eye camera fitted to the bounding box of the points that will be drawn (10 % margin, at least 2 m)"""
    pc0, skip = frame_skip(data, keep_ground, instances)
    pts = pc0[skip == 0, :3]
    pts = pts[pts.isfinite().all(dim=1)]
    if pts.shape[0] == 0:
        return Camera.bev(width=width, height=height)
    lo, hi = pts.amin(dim=0).cpu().numpy().astype(np.float64), pts.amax(dim=0).cpu().numpy().astype(np.float64)
    half = max(2.0, 1.1 * max((hi[0] - lo[0]) / 2.0 * min(width, height) / width, (hi[1] - lo[1]) / 2.0 * min(width, height) / height))
    return Camera.bev(((lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0), half, width, height, z_range=(lo[2] - 1.0, hi[2] + 1.0))


def scene_radius(data: dict, keep_ground: bool = False, instances=None) -> float:
    """half the diagonal of the drawn points' bounding box (what ``Camera.from_view`` scales ``zoom`` by)"""
    pc0, skip = frame_skip(data, keep_ground, instances)
    pts = pc0[skip == 0, :3]
    pts = pts[pts.isfinite().all(dim=1)]
    if pts.shape[0] == 0:
        return 50.0
    return max(1.0, float((pts.amax(dim=0) - pts.amin(dim=0)).norm().item()) / 2.0)


def _speed(data: dict, res_name: str, sensor_dt: float) -> np.ndarray:
    """|flow - pose_flow| / sensor_dt of a panel's result [m/s]; ``raw`` compensates nothing: 0"""
    pc = np.asarray(data["pc0"], dtype=np.float64)[:, :3]
    if res_name == "raw":
        return np.zeros(pc.shape[0], dtype=np.float32)
    ego = np.linalg.inv(np.asarray(data["pose1"], dtype=np.float64)) @ np.asarray(data["pose0"], dtype=np.float64)
    pose_flow = pc @ ego[:3, :3].T + ego[:3, 3] - pc
    return (np.linalg.norm(np.asarray(_need(data, res_name), dtype=np.float64) - pose_flow, axis=1) / float(sensor_dt)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------------
# boxes and trails -> segments (host, float64; what "line overlay, v1" draws)
# --------------------------------------------------------------------------------------------------------------------------
BOX_COLOR_BY = ("fixed", "track", "moving")
# the ring of a box face in (sx, sy): front-left, rear-left, rear-right, front-right (counter-clockwise seen from above; +x of the
# box is its front)
BOX_RING = ((1, 1), (-1, 1), (-1, -1), (1, -1))
SEGMENTS_STATIC, SEGMENTS_MOVING = 13, 16
ARROW_HEAD_BACK, ARROW_HEAD_SIDE = 0.25, 0.125


def box_corners(row) -> np.ndarray:
    """float64 [8][3]: the corners of one ``box_fit`` row (``x, y, z, l, w, h, yaw``; z is the box CENTRE), the bottom ring in the
    order of ``BOX_RING`` and then the top ring.  With ``c, s = cos yaw, sin yaw`` the corner ``(sx, sy, sz)`` is ``X = x + sx (l / 2) c
    - sy (w / 2) s``, ``Y = y + sx (l / 2) s + sy (w / 2) c``, ``Z = z + sz (h / 2)``."""
    x, y, z, l, w, h, yaw = (float(v) for v in np.asarray(row, dtype=np.float64)[:7])
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[x + sx * (l / 2) * c - sy * (w / 2) * s, y + sx * (l / 2) * s + sy * (w / 2) * c, z + sz * (h / 2)]
                     for sz in (-1, 1) for sx, sy in BOX_RING], dtype=np.float64)


def box_valid(rows) -> np.ndarray:
    """bool [F]: every value of the row finite and no negative extent (the rows ``track`` takes as valid)"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 12)
    return np.isfinite(rows).all(axis=1) & (rows[:, 3:6] >= 0).all(axis=1)


def box_moving(rows, sensor_dt: float, motion_min: float) -> np.ndarray:
    """bool [F]: ``hypot(vx, vy) * sensor_dt >= motion_min``, the MOVING test of ``box_fit`` on the stored velocity"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 12)
    with np.errstate(all="ignore"):
        return np.hypot(rows[:, 7], rows[:, 8]) * float(sensor_dt) >= float(motion_min)


def box_segments(rows, sensor_dt: float = 0.1, motion_min: float = 0.05, arrow_s: float = 0.5):
    """``box_fit``'s ``[F][12]`` rows -> (segments float32 [S][6], box_of_segment int64 [S]).  A row with a value that is not finite
    or with a negative extent is skipped.  Per box, in this order (corners as ``box_corners`` numbers them, 0..3 the bottom ring, 4..7
    the top ring):

      0..3    the bottom ring 0-1, 1-2, 2-3, 3-0
      4..7    the top ring 4-5, 5-6, 6-7, 7-4
      8..11   the uprights 0-4, 1-5, 2-6, 3-7
      12      the heading mark: from the centre of the top face ``T = (x, y, z + h / 2)`` to the midpoint of its front edge
              ``(x + (l / 2) c, y + (l / 2) s, z + h / 2)``
      13..15  only for a MOVING box (``box_moving``) and ``arrow_s > 0``: the velocity arrow on the top face.  With ``d = (vx, vy) *
              arrow_s`` (the way the box travels in ``arrow_s`` seconds), the tip ``P = T + d`` and the left normal ``n = (-d_y, d_x)``:
              the shaft ``T -> P``, then the two head strokes ``P -> P - 0.25 d + 0.125 n`` and ``P -> P - 0.25 d - 0.125 n``

    so a static box gives 13 segments and a moving one 16.  Everything in float64, cast to float32 at the end."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 12)
    valid, moving = box_valid(rows), box_moving(rows, sensor_dt, motion_min)
    segs, owner = [], []
    for f in np.flatnonzero(valid):
        row = rows[f]
        q = box_corners(row)
        pairs = [(q[a], q[(a + 1) % 4]) for a in range(4)] + [(q[4 + a], q[4 + (a + 1) % 4]) for a in range(4)] + [(q[a], q[4 + a]) for a in range(4)]
        top = np.array([row[0], row[1], row[2] + row[5] / 2])
        pairs.append((top, (q[4] + q[7]) / 2))
        if moving[f] and float(arrow_s) > 0:
            d = np.array([row[7], row[8], 0.0]) * float(arrow_s)
            n = np.array([-d[1], d[0], 0.0])
            tip = top + d
            pairs += [(top, tip), (tip, tip - ARROW_HEAD_BACK * d + ARROW_HEAD_SIDE * n), (tip, tip - ARROW_HEAD_BACK * d - ARROW_HEAD_SIDE * n)]
        segs += [np.concatenate(p) for p in pairs]
        owner += [int(f)] * len(pairs)
    return np.asarray(segs, dtype=np.float64).reshape(-1, 6).astype(np.float32), np.asarray(owner, dtype=np.int64)


def _stored(ds, i, keys) -> dict:
    """the arrays ``keys`` of item ``i`` that exist (and its ``scene_id``), read without the sweep itself where the dataset can"""
    if hasattr(ds, "index"):
        from .stored import arrays
        return {**arrays(ds, i, keys), "scene_id": ds.index[i][0], "timestamp": ds.index[i][1]}
    d = ds[i]
    return {**{k: np.asarray(d[k]) for k in keys if k in d}, "scene_id": d.get("scene_id"), "timestamp": d.get("timestamp")}


def trail_segments(dataset, item: int, name: str, trail: int, boxes=None):
    """The trails of sweep ``item`` (its position in ``dataset``) -> (segments float32 [S][6], box_of_segment int64 [S]).  For every
    box row f of the sweep whose stored ``tracks_<name>`` row has id >= 0: the polyline through that id's stored ``(x, y)`` in the
    sweeps ``item - trail .. item`` of the same scene, each earlier point moved into THIS sweep's sensor frame by ``inv(pose0_item) @
    pose0_j`` (float64; the point's z is taken as 0 in sweep j's frame, and only x and y of the result are used) and placed at the
    height of the box's top face, ``z + h / 2`` (``boxes``: the sweep's ``boxes_<name>`` rows; read from the dataset when None).  Two
    consecutive sweeps that both hold the id give one segment, older end first; a sweep without the id leaves a gap; a neighbour of
    another scene ends the walk.  Reads only ``tracks_<name>`` and ``pose0`` of the neighbour sweeps.  A ``tracks_<name>`` whose row
    count differs from the boxes' is refused as stale."""
    from .box_fit import boxes_key
    from .track import tracks_key
    bk, tk, trail = boxes_key(name), tracks_key(name), int(trail)
    if trail < 0:
        raise ValueError(f"trail={trail}: the number of earlier sweeps, >= 0")
    wanted = [tk, "pose0"] + ([bk] if boxes is None else [])
    here = _stored(dataset, item, wanted)
    for k in wanted:
        _need(here, k)
    rows = np.asarray(here[bk] if boxes is None else boxes, dtype=np.float64).reshape(-1, 12)
    tracks = _check_tracks(np.asarray(here[tk]), rows, tk, bk)
    inv_here = np.linalg.inv(np.asarray(here["pose0"], dtype=np.float64))
    history = [(tracks, np.eye(4))]                                # newest first
    for j in range(item - 1, item - trail - 1, -1):
        if j < 0:
            break
        then = _stored(dataset, j, [tk, "pose0"])
        if then["scene_id"] != here["scene_id"] or tk not in then or "pose0" not in then:
            break
        history.append((np.asarray(then[tk], dtype=np.float64).reshape(-1, 6), inv_here @ np.asarray(then["pose0"], dtype=np.float64)))
    segs, owner = [], []
    valid = box_valid(rows)
    for f in np.flatnonzero(valid & (tracks[:, 0] >= 0)):
        top = rows[f, 2] + rows[f, 5] / 2
        points = []
        for trk, move in reversed(history):                       # oldest first
            hit = np.flatnonzero(trk[:, 0] == tracks[f, 0])
            if len(hit) == 0:
                points.append(None)
                continue
            p = move @ np.array([trk[hit[0], 2], trk[hit[0], 3], 0.0, 1.0])
            points.append(np.array([p[0], p[1], top]))
        for a, b in zip(points[:-1], points[1:]):
            if a is not None and b is not None:
                segs.append(np.concatenate([a, b]))
                owner.append(int(f))
    return np.asarray(segs, dtype=np.float64).reshape(-1, 6).astype(np.float32), np.asarray(owner, dtype=np.int64)


def _check_tracks(tracks, rows, tk: str, bk: str) -> np.ndarray:
    tracks = np.asarray(tracks)
    if tracks.ndim != 2 or tracks.shape[1] != 6:
        raise ValueError(f"{tk}: holds {tracks.dtype} {tracks.shape}, not [F][6] track rows")
    if len(tracks) != len(rows):
        raise ValueError(f"{tk}: holds {len(tracks)} rows for the {len(rows)} boxes of {bk}: stale tracks (run `python -m himo_amd.track "
                         f"--overwrite` after box_fit)")
    return tracks.astype(np.float64)


def check_line_options(box_color_by: str = "fixed", trail: int = 0, line_px: int = 0, arrow_s: float = 0.5) -> None:
    if box_color_by not in BOX_COLOR_BY:
        raise ValueError(f"--box_color_by {box_color_by!r}: one of {', '.join(BOX_COLOR_BY)}")
    if isinstance(trail, bool) or int(trail) != trail or int(trail) < 0:
        raise ValueError(f"--trail {trail!r}: the number of earlier sweeps, >= 0")
    if isinstance(line_px, bool) or int(line_px) != line_px or not 0 <= int(line_px) <= 3:
        raise ValueError(f"--line_px {line_px!r}: 0..3")
    if not (np.isfinite(arrow_s) and arrow_s >= 0):
        raise ValueError(f"--arrow_s {arrow_s!r}: finite and >= 0")


def overlay_keys(res_names, boxes: bool = False, boxes_gt=None, box_color_by: str = "fixed", trail: int = 0) -> list:
    """the frame keys the line overlay of ``render_frame`` reads for these options, beside ``required_keys``"""
    from .box_fit import boxes_key
    from .track import tracks_key
    keys = []
    if boxes:
        keys += [boxes_key(n) for n in res_names]
        if box_color_by == "track" or int(trail) > 0:
            keys += [tracks_key(n) for n in res_names]
    if boxes_gt:
        keys.append(boxes_key(boxes_gt))
    return list(dict.fromkeys(keys))


def _panel_lines(data: dict, names, clouds, gt, box_color_by, trails, sensor_dt, motion_min, arrow_s):
    """the segments of one panel -> (segments float32 [S][6], colours uint32 [S], boxes drawn).  ``names``: the result names whose
    boxes the panel draws; ``clouds``: None, or one colour per name (the overlay panel); ``gt``: a name drawn in white, or None."""
    from .box_fit import boxes_key
    from .track import tracks_key
    pal = palette()
    segs, cols, count = [], [], 0
    for k, name in enumerate(names):
        rows = np.asarray(_need(data, boxes_key(name)), dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != 12:
            raise ValueError(f"{boxes_key(name)}: holds {rows.shape}, not [F][12] box rows")
        per_box = np.full(len(rows), pal[1], dtype=np.uint32)
        if clouds is not None:
            per_box[:] = clouds[k]
        elif box_color_by == "track":
            ids = _check_tracks(_need(data, tracks_key(name)), rows, tracks_key(name), boxes_key(name))[:, 0].astype(np.int64)
            per_box = np.where(ids >= 0, pal[ids % len(pal)], np.uint32(NEUTRAL)).astype(np.uint32)
        elif box_color_by == "moving":
            per_box = np.where(box_moving(rows, sensor_dt, motion_min), pal[1], pal[2]).astype(np.uint32)
        s, owner = box_segments(rows, sensor_dt, motion_min, arrow_s)
        segs.append(s)
        cols.append(per_box[owner])
        count += int(box_valid(rows).sum())
        if trails is not None and name in trails:
            s, owner = trails[name]
            segs.append(np.asarray(s, dtype=np.float32).reshape(-1, 6))
            cols.append(per_box[np.asarray(owner, dtype=np.int64)])
    if gt:
        rows = np.asarray(_need(data, boxes_key(gt)), dtype=np.float64)
        s, owner = box_segments(rows, sensor_dt, motion_min, arrow_s)
        segs.append(s)
        cols.append(np.full(len(owner), WHITE, dtype=np.uint32))
        count += int(box_valid(rows).sum())
    if not segs:
        return np.zeros((0, 6), np.float32), np.zeros(0, np.uint32), 0
    return np.concatenate(segs).astype(np.float32), np.concatenate(cols).astype(np.uint32), count


def render_frame(data: dict, res_names, color_by: str = "lidar", camera: Camera | None = None, renderer: Renderer | None = None,
                 point_px: int = 1, edl: float = 0.0, keep_ground: bool = False, instances=None, sensor_dt: float = 0.1,
                 value_range=None, background: int = BACKGROUND, return_buffers: bool = False, *, boxes: bool = False, boxes_gt=None,
                 box_color_by: str = "fixed", trails=None, arrow_s: float = 0.5, line_px: int = 0, box_depth: bool = False,
                 motion_min: float = 0.05):
    """One panel per result name of ``res_names``, joined left to right with a ``SEPARATOR_PX`` separator: ``raw`` draws ``pc0`` as it
    stands, any other name ``pc0 + comp_dis`` (``compdis.comp_dis_frame(data, name)``; the offset goes to the splat, it is not added
    on the host).  ``color_by``: see the module docstring of the program below; ``overlay`` draws ONE panel.  ``point_px`` is the
    disc radius of rule E.  Returns (image: (H, W_total, 3) uint8 device tensor, info: {"panels", "points", "pixels"}); with
    ``return_buffers`` also the list of the panels' visibility buffers (clones).

    The line overlay ("line overlay, v1"), all off by default: ``boxes`` draws on each panel ``boxes_<its own name>`` (``raw``:
    ``boxes_raw``; the ``overlay`` panel draws every name's boxes in that name's cloud colour, whatever ``box_color_by`` says);
    ``boxes_gt`` a name whose boxes are drawn in white on every panel; ``box_color_by``: ``fixed`` one palette colour, ``track``
    ``palette[id % 6]`` of ``tracks_<name>`` (neutral for id -1; a row count that differs from the boxes' is refused as stale),
    ``moving`` one colour for MOVING boxes and another for the rest; ``trails``: {name: ``trail_segments(...)``} drawn in their boxes'
    colours; ``arrow_s`` the seconds of travel a velocity arrow shows; ``line_px`` the ``half_px`` of rule E; ``box_depth`` tests the
    lines against the points (default: lines on top).  With any of them ``info`` gains "boxes", "segments" and "line_pixels" per panel
    and ``return_buffers`` a second list, the panels' lines buffers."""
    import torch
    from . import compdis, utils
    res_names = list(res_names)
    if not res_names:
        raise ValueError("render_frame: no result names")
    kind, key = parse_color_by(color_by)
    keep_ground = keep_ground or kind == "ground"
    with_lines = bool(boxes or boxes_gt)
    if trails and not boxes:
        raise ValueError("render_frame: trails belong to the boxes of boxes=True")
    if with_lines:
        check_line_options(box_color_by, 0, line_px, arrow_s)
    for k in required_keys(res_names, color_by, instances) + (overlay_keys(res_names, boxes, boxes_gt, box_color_by) if with_lines else []):
        _need(data, k)
    if camera is None:
        camera = auto_camera(data, 1024, 1024, keep_ground, instances)
    r = renderer if renderer is not None else Renderer(int(camera.width), int(camera.height))
    dev = r.device
    pc0, skip = frame_skip(data, keep_ground, instances)
    n = int(pc0.shape[0])
    drawn = n - int(skip.sum().item())
    offsets = {name: torch.from_numpy(compdis.comp_dis_frame(data, name, sensor_dt=sensor_dt)).to(dev) for name in res_names if name != "raw"}
    panels, images, points, pixels, buffers = [], [], [], [], []
    line_info, line_buffers = {"boxes": [], "segments": [], "line_pixels": []}, []

    def finish(name, image, count, drawn_names=None, clouds=None):
        if with_lines:                                            # rule F, over the image just resolved
            segs, cols, n_boxes = _panel_lines(data, drawn_names if boxes else [], clouds, boxes_gt, box_color_by, trails if boxes else None,
                                               sensor_dt, motion_min, arrow_s)
            r.clear_lines()
            r.lines(segs, line_px, 0, camera)
            image = r.composite(cols, depth_test=box_depth)
            line_info["boxes"].append(n_boxes)
            line_info["segments"].append(int(len(segs)))
            line_info["line_pixels"].append(int((r.line_buffer() != EMPTY).sum().item()))
            if return_buffers:
                line_buffers.append(r.line_buffer().clone())
        panels.append(name)
        images.append(image.clone())
        points.append(count)
        pixels.append(int((r.visibility() != EMPTY).sum().item()))
        if return_buffers:
            buffers.append(r.visibility().clone())

    if kind == "overlay":
        r.clear()
        pal, colors, results, clouds = palette(), [], 0, []
        for k, name in enumerate(res_names):
            r.splat(pc0, offsets.get(name), skip, point_px, k * n, camera)
            clouds.append(WHITE if name == "raw" else pal[results % len(pal)])
            colors.append(np.full(n, clouds[-1], dtype=np.uint32))
            results += name != "raw"
        finish("+".join(res_names), r.resolve(colors=np.concatenate(colors), edl=edl, background=background), drawn * len(res_names),
               res_names, clouds)
    else:
        shared = None
        if kind == "lidar":
            shared = dict(ids=(np.asarray(data["lidar_id"]).astype(np.int32),))
        elif kind == "ground":
            shared = dict(ids=(np.asarray(data["gm0"]).astype(np.int32),))
        elif kind == "label":
            shared = dict(ids=(np.asarray(data[key]).astype(np.int64).astype(np.int32) - 1,))          # 0 -> -1: neutral
        elif kind == "dt0":
            lo, hi = value_range if value_range is not None else DEFAULT_RANGE["dt0"]
            shared = dict(scalar=(utils.dt0_from_lidar_dt(torch.from_numpy(np.ascontiguousarray(data["lidar_dt"], dtype=np.float32)).to(dev)), lo, hi))
        for name in res_names:
            r.clear()
            r.splat(pc0, offsets.get(name), skip, point_px, 0, camera)
            how = shared
            if kind == "speed":
                lo, hi = value_range if value_range is not None else DEFAULT_RANGE["speed"]
                how = dict(scalar=(_speed(data, name, sensor_dt), lo, hi))
            finish(name, r.resolve(edl=edl, background=background, **how), drawn, [name])
    sep = torch.tensor([SEPARATOR & 0xFF, (SEPARATOR >> 8) & 0xFF, (SEPARATOR >> 16) & 0xFF], dtype=torch.uint8, device=dev)
    parts = []
    for k, image in enumerate(images):
        if k:
            parts.append(sep.expand(image.shape[0], SEPARATOR_PX, 3))
        parts.append(image)
    info = {"panels": panels, "points": points, "pixels": pixels, **(line_info if with_lines else {})}
    out = (torch.cat(parts, dim=1).contiguous(), info)
    if return_buffers:
        out += (buffers, line_buffers) if with_lines else (buffers,)
    return out


# --------------------------------------------------------------------------------------------------------------------------
# PNG
# --------------------------------------------------------------------------------------------------------------------------
def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def write_png(path, rgb) -> None:
    """``rgb`` (H, W, 3) uint8 (array or tensor) as an 8-bit RGB, non-interlaced PNG: filter type 0 on every row, one IDAT chunk"""
    a = rgb.cpu().numpy() if hasattr(rgb, "cpu") else np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: an image is (H, W, 3) uint8, not {a.shape} {a.dtype}")
    h, w = int(a.shape[0]), int(a.shape[1])
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)               # a filter byte of 0 before every row
    rows[:, 1:] = a.reshape(h, 3 * w)
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(data)


# --------------------------------------------------------------------------------------------------------------------------
# the program
# --------------------------------------------------------------------------------------------------------------------------
def load_keyframes(path) -> list:
    """a camera file: one keyframe ``{"front", "lookat", "up", "zoom"}``, a list of them, or ``{"trajectory": [...]}``"""
    with open(path) as f:
        doc = json.load(f)
    if isinstance(doc, dict) and "trajectory" in doc:
        doc = doc["trajectory"]
    frames = [doc] if isinstance(doc, dict) else list(doc)
    for k in frames:
        missing = [name for name in KEYFRAME_KEYS if name not in k]
        if missing:
            raise KeyError(f"{path}: a keyframe lacks {missing}")
    if not frames:
        raise ValueError(f"{path}: no keyframes")
    return frames


def parse_size(text: str) -> tuple:
    try:
        w, h = (int(v) for v in str(text).lower().split("x"))
    except ValueError:
        raise ValueError(f"--size {text!r}: WxH, e.g. 1024x768") from None
    if w < 1 or h < 1:
        raise ValueError(f"--size {text!r}: WxH, e.g. 1024x768")
    return w, h


def parse_indices(index, indices) -> list:
    if (index is None) == (indices is None):
        raise ValueError("one of --index i and --indices a:b")
    if index is not None:
        return [int(index)]
    try:
        a, b = (int(v) for v in str(indices).split(":"))
    except ValueError:
        raise ValueError(f"--indices {indices!r}: a:b, the sweeps a .. b - 1") from None
    if not 0 <= a < b:
        raise ValueError(f"--indices {indices!r}: a:b, the sweeps a .. b - 1")
    return list(range(a, b))


def main(data_dir: str, out_dir: str, res_names="raw,seflowpp_best", index=None, indices=None, scene: str | None = None,
         color_by: str = "lidar", camera: str = "bev", sample_step: int = 10, size: str = "1024x768", point_px: int = 1, edl: float = 0.0,
         keep_ground: bool = False, instance=None, dataset=None, *, boxes: bool = False, boxes_gt: str | None = None,
         box_color_by: str = "fixed", trail: int = 0, arrow_s: float = 0.5, line_px: int = 0, box_depth: bool = False) -> list:
    """The program: the sweeps ``index`` / ``indices`` of the dataset's index (of ``scene``'s sweeps with ``scene``) as
    ``<out_dir>/<scene>_<timestamp>.png``, from a fixed camera; or, with a camera file of several keyframes, ONE sweep as the numbered
    frames ``00000.png ...`` along ``spline_path(keyframes, sample_step)``.  ``<out_dir>/view.json`` lists every image with its panel
    names, its camera and, per panel, the points drawn and the non-empty pixels.  Returns that list.

    ``boxes`` / ``boxes_gt`` / ``box_color_by`` / ``arrow_s`` / ``line_px`` / ``box_depth``: the line overlay of ``render_frame``;
    ``trail`` K > 0 adds to every tracked box the trail of its id over the K sweeps before it (``trail_segments``; needs ``boxes`` and
    the stored ``tracks_<name>``).  With ``boxes`` or ``boxes_gt`` every entry of ``view.json`` gains "boxes", "segments" and
    "line_pixels" per panel; without them it gains nothing."""
    from . import _lib
    from .dataset import open_dataset
    from .eval_seg import parse_res_names
    names = parse_res_names(res_names)
    kind, _ = parse_color_by(color_by)
    width, height = parse_size(size)
    todo = parse_indices(index, indices)
    instances = [int(v) for v in str(instance).split(",")] if instance not in (None, "") else None
    keep_ground = keep_ground or kind == "ground"
    check_line_options(box_color_by, trail, line_px, arrow_s)
    if int(trail) > 0 and not boxes:
        raise ValueError("--trail draws the trails of the boxes of --boxes: give --boxes")
    keys = required_keys(names, color_by, instances) + overlay_keys(names, boxes, boxes_gt, box_color_by, trail)
    keyframes = None if camera in ("bev", "auto") else load_keyframes(camera)
    if keyframes is not None and len(keyframes) > 1 and len(todo) != 1:
        raise ValueError("a camera path of several keyframes renders one sweep: give --index")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    if dataset is None:
        dataset = open_dataset(data_dir, vis_name=[n for n in names if n != "raw"], fields=tuple(keys))
    where = list(range(len(dataset)))
    if scene is not None:
        where = [i for i, entry in enumerate(getattr(dataset, "index", [])) if entry[0] == scene]
        if not where:
            raise KeyError(f"{scene}: no such scene in {data_dir}")
    renderer = Renderer(width, height, _lib.require_gpu())
    listing = []

    def one(data, cam, file_name, trails=None):
        image, info = render_frame(data, names, color_by, cam, renderer, point_px=point_px, edl=edl, keep_ground=keep_ground, instances=instances,
                                   boxes=boxes, boxes_gt=boxes_gt, box_color_by=box_color_by, trails=trails, arrow_s=arrow_s, line_px=line_px,
                                   box_depth=box_depth)
        write_png(out_dir / file_name, image)
        listing.append({"file": file_name, "scene_id": str(data.get("scene_id")), "timestamp": int(data.get("timestamp", 0)),
                        "color_by": color_by, "camera": cam.as_dict(), **info})

    try:
        for i in todo:
            if not 0 <= i < len(where):
                raise IndexError(f"sweep {i} of {len(where)}")
            data = dataset[where[i]]
            for k in keys:
                _need(data, k)
            trails = None
            if int(trail) > 0:
                from .box_fit import boxes_key
                trails = {n: trail_segments(dataset, where[i], n, int(trail), boxes=data[boxes_key(n)]) for n in names}
            if keyframes is None:
                cam = Camera.bev(width=width, height=height) if camera == "bev" else auto_camera(data, width, height, keep_ground, instances)
                one(data, cam, f"{data['scene_id']}_{data['timestamp']}.png", trails)
                continue
            radius = scene_radius(data, keep_ground, instances)
            path = spline_path(keyframes, sample_step) if len(keyframes) > 1 else keyframes
            for k, kf in enumerate(path):
                cam = Camera.from_view(kf["front"], kf["lookat"], kf["up"], kf["zoom"], radius, width=width, height=height)
                one(data, cam, f"{k:05d}.png" if len(keyframes) > 1 else f"{data['scene_id']}_{data['timestamp']}.png", trails)
    finally:
        close = getattr(dataset, "close", None)
        if close is not None:
            close()
    with open(out_dir / "view.json", "w") as f:
        json.dump(listing, f, indent=1)
    print(f"{len(listing)} image{'s' if len(listing) != 1 else ''} of {len(listing[0]['panels']) if listing else 0} panel(s) -> {out_dir}")
    return listing


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="render sweeps, raw and compensated, as PNG panels on the GPU (point splat, v1: this build's own "
                                             "rule, no claim about open3d's pixels; timing unmeasured; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files and index_total.pkl")
    ap.add_argument("--scene", default=None, help="count --index / --indices within this scene's sweeps")
    ap.add_argument("--index", type=int, default=None, help="the sweep to draw")
    ap.add_argument("--indices", default=None, help="a:b -- the sweeps a .. b - 1, one image each from a fixed camera")
    ap.add_argument("--res_names", default="raw,seflowpp_best", help="one panel each: raw = the sweep as recorded, any other name = compensated by that flow")
    ap.add_argument("--color_by", default="lidar", help=f"{' | '.join(COLOR_BY)} | label:<key> (any int dataset of the sweep, 0 = neutral)")
    ap.add_argument("--camera", default="bev", help="bev | auto | FILE.json (one keyframe {front, lookat, up, zoom}, or a list of them)")
    ap.add_argument("--sample_step", type=int, default=10, help="samples per interval of a keyframe list (frames 00000.png ...)")
    ap.add_argument("--size", default="1024x768", help="WxH of one panel")
    ap.add_argument("--point_px", type=int, default=1, help="disc radius of a point in pixels (0..8)")
    ap.add_argument("--edl", type=float, default=0.0, help="eye-dome lighting strength (0 = off)")
    ap.add_argument("--keep_ground", action="store_true", help="draw the ground points too")
    ap.add_argument("--instance", default=None, help="8,9 -- draw only these flow_instance_ids (--camera auto fits them)")
    ap.add_argument("--out_dir", required=True)
    # the line overlay ("line overlay, v1": this build's own rule; parity unpinned, the reference has no such stage; timing: profiles/view_boxes.txt)
    ap.add_argument("--boxes", action="store_true", help="draw boxes_<name> on the panel of <name> (raw: boxes_raw; --color_by overlay: every name's, in its cloud colour)")
    ap.add_argument("--boxes_gt", default=None, help="NAME -- also draw boxes_<NAME> in white on every panel")
    ap.add_argument("--box_color_by", default="fixed", help=f"{' | '.join(BOX_COLOR_BY)} (track: by tracks_<name> id; moving: MOVING boxes apart from the rest)")
    ap.add_argument("--trail", type=int, default=0, help="K -- the trail of every tracked box over the K sweeps before it (needs --boxes and tracks_<name>)")
    ap.add_argument("--arrow_s", type=float, default=0.5, help="a velocity arrow shows this many seconds of travel (0 = none)")
    ap.add_argument("--line_px", type=int, default=0, help="half-width of a line in pixels (0..3)")
    ap.add_argument("--box_depth", action="store_true", help="nearer points hide lines (default: lines on top)")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    return main(a.data_dir, a.out_dir, a.res_names, a.index, a.indices, a.scene, a.color_by, a.camera, a.sample_step, a.size, a.point_px,
                a.edl, a.keep_ground, a.instance, boxes=a.boxes, boxes_gt=a.boxes_gt, box_color_by=a.box_color_by, trail=a.trail,
                arrow_s=a.arrow_s, line_px=a.line_px, box_depth=a.box_depth)


if __name__ == "__main__":
    _cli()
