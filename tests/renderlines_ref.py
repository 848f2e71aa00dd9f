"""numpy / Python restatement of the viewer's line overlay, "line overlay, v1" (the module docstring of himo_amd/view.py is the rule;
himo_amd/csrc/renderlines.hip the device side).  Rules A-C run per segment on float32 SCALARS, one operation per statement; from
the end pixels on everything is an integer: Python ints for the ends, and for the walk either Python ints (``walk_py``, the rule
read aloud) or the same expressions on int64 arrays (``walk``: every magnitude stays below 2^46, so int64 is exact; numpy's ``//`` is
the floor division).  The two walks are compared in tests/test_view_boxes_cpu.py.  It is the only checker of the overlay: the rule is
this build's own and no other viewer's pixels are claimed."""
import numpy as np

from render_ref import EMPTY, F, _bytes, camera, clear, disc  # noqa: F401  (camera, clear and disc are the point splat's own)

LIMIT = F(1048576.0)                                               # 2^20


def _cam_coords(m, p):
    out = []
    for r in range(3):
        a = F(m[r, 0] * p[0])
        b = F(m[r, 1] * p[1])
        a = F(a + b)
        b = F(m[r, 2] * p[2])
        a = F(a + b)
        a = F(a + m[r, 3])
        out.append(a)
    return out


def _clip_end(e, o, znear, zfar):
    """rule B for the end ``e`` against the other ORIGINAL end ``o``"""
    x, y, z = e
    if not (z < znear or z > zfar):
        return e
    plane = znear if z < znear else zfar
    t = F(plane - z)
    d = F(o[2] - z)
    t = F(t / d)
    dx = F(o[0] - x)
    dx = F(t * dx)
    dy = F(o[1] - y)
    dy = F(t * dy)
    return [F(x + dx), F(y + dy), plane]


def _project(cam, e):
    if cam["ortho"]:
        u = F(cam["fx"] * e[0])
        v = F(cam["fy"] * e[1])
    else:
        u = F(e[0] / e[2])
        u = F(cam["fx"] * u)
        v = F(e[1] / e[2])
        v = F(cam["fy"] * v)
    return F(u + cam["cx"]), F(v + cam["cy"])


def _depth(cam, zc):
    t = F(zc - cam["znear"])
    t = F(t * cam["inv_range"])
    t = F(t * F(16777216.0))
    return int(min(np.floor(t), F(16777215.0)))


def ends(seg, cam):
    """rules A-C for one segment: -> None when it is dropped, else the Python ints (X0, Y0, zq0, X1, Y1, zq1)"""
    seg = np.asarray(seg, F).reshape(6)
    with np.errstate(all="ignore"):
        a, b = _cam_coords(cam["m"], seg[0:3]), _cam_coords(cam["m"], seg[3:6])
        if not all(np.isfinite(v) for v in a + b):
            return None
        znear, zfar = cam["znear"], cam["zfar"]
        if (a[2] < znear and b[2] < znear) or (a[2] > zfar and b[2] > zfar):
            return None
        ca, cb = _clip_end(a, b, znear, zfar), _clip_end(b, a, znear, zfar)
        u0, v0 = _project(cam, ca)
        u1, v1 = _project(cam, cb)
        if not all(np.isfinite(v) for v in (u0, v0, u1, v1)) or any(abs(v) >= LIMIT for v in (u0, v0, u1, v1)):
            return None
        return (int(np.floor(u0)), int(np.floor(v0)), _depth(cam, ca[2]), int(np.floor(u1)), int(np.floor(v1)), _depth(cam, cb[2]))


def walk_py(X0, Y0, zq0, X1, Y1, zq1):
    """rule D in Python ints: -> [(x_k, y_k, zq_k)] for k = 0 .. steps"""
    dx, dy = X1 - X0, Y1 - Y0
    steps = max(abs(dx), abs(dy))
    if steps == 0:
        return [(X0, Y0, zq0)]
    return [(X0 + (2 * k * dx + steps) // (2 * steps), Y0 + (2 * k * dy + steps) // (2 * steps), zq0 + (k * (zq1 - zq0)) // steps)
            for k in range(steps + 1)]


def walk(X0, Y0, zq0, X1, Y1, zq1):
    """rule D on int64 arrays: -> (x, y, zq), each [steps + 1]"""
    dx, dy = X1 - X0, Y1 - Y0
    steps = max(abs(dx), abs(dy))
    if steps == 0:
        return np.array([X0], np.int64), np.array([Y0], np.int64), np.array([zq0], np.int64)
    k = np.arange(steps + 1, dtype=np.int64)
    return (X0 + (2 * k * dx + steps) // (2 * steps), Y0 + (2 * k * dy + steps) // (2 * steps), zq0 + (k * (zq1 - zq0)) // steps)


def lines(buf, segs, cam, half_px=0, index_base=0):
    """add the segments to ``buf`` (uint64 [height][width], in place; rules A-E).  -> the number of segments that passed every
    rejection"""
    assert 0 <= half_px <= 3
    segs = np.asarray(segs, F).reshape(-1, 6)
    w, h = cam["width"], cam["height"]
    flat = buf.reshape(-1)
    kept = 0
    for i, seg in enumerate(segs):
        e = ends(seg, cam)
        if e is None:
            continue
        kept += 1
        x, y, zq = walk(*e)
        near = (x >= -half_px) & (x < w + half_px) & (y >= -half_px) & (y < h + half_px)           # only to spare work: rule E tests every pixel
        x, y, zq = x[near], y[near], zq[near]
        key = (zq.astype(np.uint64) << np.uint64(32)) | np.uint64(index_base + i)
        for ddx, ddy in disc(half_px):
            qx, qy = x + ddx, y + ddy
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            np.minimum.at(flat, qy[inside] * w + qx[inside], key[inside])
    return kept


def composite(rgb, buf, vis, colors, neutral=0x808080):
    """rule F: -> a copy of ``rgb`` (uint8 [height][width][3]) with the overlay on it; ``vis`` None = no depth test"""
    colors = np.asarray(colors, np.uint32).reshape(-1)
    out = np.array(rgb, np.uint8, copy=True)
    show = buf != EMPTY
    if vis is not None:
        show &= ~((vis != EMPTY) & ((vis >> np.uint64(32)) < (buf >> np.uint64(32))))
    idx = (buf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    colour = np.full(buf.shape, np.uint32(neutral), dtype=np.uint32)
    have = show & (idx < len(colors))
    colour[have] = colors[idx[have]]
    out[show] = _bytes(colour)[show]
    return out
