"""numpy restatement of the viewer's renderer, "point splat, v1" (the module docstring of himo_amd/view.py is the rule;
himo_amd/csrc/render.hip the device side).  float32 throughout, one operation per statement, ``np.floor`` and ``np.minimum.at`` on
the uint64 keys.  It is the only checker of the renderer: the rule is this build's own and no other viewer's pixels are claimed."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera(m, ortho, fx, fy, cx, cy, znear, zfar, width, height):
    """the fields of ``himo_camera`` as a dict; ``inv_range`` is the float32 quotient the host computes"""
    znear, zfar = F(znear), F(zfar)
    with np.errstate(all="ignore"):
        inv_range = F(1.0) / (zfar - znear)
    return dict(m=np.asarray(m, F).reshape(3, 4), ortho=bool(ortho), fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy), znear=znear, zfar=zfar,
                inv_range=F(inv_range), width=int(width), height=int(height))


def from_ctypes(cam):
    """the same dict from a ``himo_amd.view.Camera``"""
    return dict(m=np.array(list(cam.m), F).reshape(3, 4), ortho=bool(cam.ortho), fx=F(cam.fx), fy=F(cam.fy), cx=F(cam.cx), cy=F(cam.cy),
                znear=F(cam.znear), zfar=F(cam.zfar), inv_range=F(cam.inv_range), width=int(cam.width), height=int(cam.height))


def clear(width, height):
    return np.full((height, width), EMPTY, dtype=np.uint64)


def disc(radius):
    """the integer offsets (dx, dy) with dx^2 + dy^2 <= radius^2"""
    return [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dx * dx + dy * dy <= radius * radius]


def splat(vis, pts, cam, radius=0, index_base=0, offset=None, skip=None):
    """add the points to ``vis`` (uint64 [height][width], in place).  -> the number of points that passed every rejection"""
    assert 0 <= radius <= 8
    pts = np.asarray(pts, F)
    n = pts.shape[0]
    if n == 0:
        return 0
    with np.errstate(all="ignore"):
        x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
        if offset is not None:
            offset = np.asarray(offset, F).reshape(n, 3)
            x = x + offset[:, 0]
            y = y + offset[:, 1]
            z = z + offset[:, 2]
        m = cam["m"]
        cc = []
        for r in range(3):
            a = m[r, 0] * x
            b = m[r, 1] * y
            a = a + b
            b = m[r, 2] * z
            a = a + b
            a = a + m[r, 3]
            cc.append(a.astype(F))
        xc, yc, zc = cc
        keep = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & ~(zc < cam["znear"]) & ~(zc > cam["zfar"])
        if skip is not None:
            keep &= np.asarray(skip).reshape(n) == 0
        if cam["ortho"]:
            u = cam["fx"] * xc
            v = cam["fy"] * yc
        else:
            u = xc / zc
            u = cam["fx"] * u
            v = yc / zc
            v = cam["fy"] * v
        u = (u + cam["cx"]).astype(F)
        v = (v + cam["cy"]).astype(F)
        lo = F(-(radius + 1))
        keep &= np.isfinite(u) & np.isfinite(v)
        keep &= ~(u < lo) & (u < F(cam["width"] + radius + 1)) & ~(v < lo) & (v < F(cam["height"] + radius + 1))
        t = zc - cam["znear"]
        t = t * cam["inv_range"]
        t = t * F(16777216.0)
        t = np.minimum(np.floor(t), F(16777215.0))
    idx = np.flatnonzero(keep)
    px = np.floor(u[idx]).astype(np.int64)
    py = np.floor(v[idx]).astype(np.int64)
    zq = t[idx].astype(np.uint64)
    key = (zq << np.uint64(32)) | (np.uint64(index_base) + idx.astype(np.uint64))
    flat = vis.reshape(-1)
    for dx, dy in disc(radius):
        qx, qy = px + dx, py + dy
        inside = (qx >= 0) & (qx < cam["width"]) & (qy >= 0) & (qy < cam["height"])
        np.minimum.at(flat, qy[inside] * cam["width"] + qx[inside], key[inside])
    return int(idx.size)


def _bytes(c):
    c = np.asarray(c, np.uint32)
    return np.stack([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF], axis=-1).astype(np.uint8)


def _depth_log(vis):
    with np.errstate(all="ignore"):
        zq1 = ((vis >> np.uint64(32)) + np.uint64(1)).astype(F)
        return np.where(vis == EMPTY, F(24.0), np.log2(zq1).astype(F)).astype(F)


def resolve(vis, mode, attr, background=0, neutral=0x808080, lo=0.0, hi=1.0, lut=None, palette=None, edl=0.0, edl_px=1, scale=None):
    """uint8 [height][width][3] of the buffer.  ``attr``: mode 0 uint32 rgba, mode 1 float32 scalars, mode 2 int32 ids."""
    h, w = vis.shape
    hit = vis != EMPTY
    idx = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    colour = np.full((h, w), np.uint32(neutral), dtype=np.uint32)
    attr = np.asarray(attr)
    have = hit & (idx < attr.shape[0])
    at = idx[have]
    if mode == 0:
        colour[have] = attr.astype(np.uint32)[at]
    elif mode == 1:
        lut = np.asarray(lut, np.uint32)
        assert lut.shape == (256,)
        s = attr.astype(F)[at]
        if scale is None:
            scale = F(F(256.0) / (F(hi) - F(lo)))
        with np.errstate(all="ignore"):
            t = s - F(lo)
            t = t * F(scale)
            b = np.clip(np.floor(t), F(0.0), F(255.0))
        fin = np.isfinite(s)
        c = np.full(at.shape, np.uint32(neutral), dtype=np.uint32)
        c[fin] = lut[b[fin].astype(np.int64)]
        colour[have] = c
    else:
        palette = np.asarray(palette, np.uint32)
        ids = attr.astype(np.int64)[at]
        c = np.full(at.shape, np.uint32(neutral), dtype=np.uint32)
        c[ids >= 0] = palette[ids[ids >= 0] % len(palette)]
        colour[have] = c
    colour[~hit] = np.uint32(background)
    rgb = _bytes(colour)
    if edl > 0:
        e = int(edl_px)
        L = _depth_log(vis)
        total = np.zeros((h, w), F)
        for dy, dx in ((0, -e), (0, e), (-e, 0), (e, 0)):
            nb = L.copy()                                         # a neighbour outside the image counts as the centre's own L
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
            nb[np.ix_(oky, okx)] = L[np.ix_(ys[oky], xs[okx])]
            d = (L - nb).astype(F)
            total = (total + np.maximum(F(0.0), d)).astype(F)
        resp = (total / F(4.0)).astype(F)
        shade = np.exp2((F(-edl) * resp).astype(F)).astype(F)
        lit = np.floor((rgb.astype(F) * shade[..., None]).astype(F) + F(0.5)).astype(np.uint8)
        rgb = np.where(hit[..., None], lit, rgb)
    return rgb
