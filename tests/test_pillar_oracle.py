"""The checker of the pillar stage checked: oracle/pillar_oracle.py must accept an emulated CORRECT kernel (float32, fma chain,
another summation order) on every case of the matrix and reject each emulated WRONG kernel on at least one.  CPU only."""
import numpy as np
import pytest

import pillar_oracle as po

F32, F64 = np.float32, np.float64
EPS, MOM = 1e-3, 0.1


def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def emu_forward(pts, T, grid, p, bugs=()):
    if "fma_transform" in bugs:
        xyz = (np.asarray(pts, F64) @ np.asarray(T, F64)[:3, :3].T + np.asarray(T, F64)[:3, 3][None]).astype(F32)
    else:
        xyz = po.transform(pts, T)
    with np.errstate(all="ignore"):
        f = np.floor((xyz - grid.vmin[None]) / grid.voxel[None]).astype(F32)
        lim = np.array([grid.W, grid.H, 1], F32)[None]
        okk = np.all((f >= 0) & ((f <= lim) if "le_upper" in bugs else (f < lim)), axis=1)
    ix, iy = np.where(okk, f[:, 0], 0).astype(np.int64), np.where(okk, f[:, 1], 0).astype(np.int64)
    pid = np.where(okk, iy * grid.W + ix, -1).astype(np.int32)
    if "centre_half" in bugs:
        cc = np.stack([grid.vmin[0] + (ix.astype(F32) + F32(0.5)) * grid.voxel[0], grid.vmin[1] + (iy.astype(F32) + F32(0.5)) * grid.voxel[1],
                       np.full(ix.shape, grid.vmin[2] + F32(0.5) * grid.voxel[2], F32)], 1).astype(F32)
    else:
        cc = po.cell_centres(grid, ix, iy)
    with np.errstate(all="ignore"):
        off = np.where(okk[:, None], xyz - cc, F32(0)).astype(F32)
    start, order = po.cell_lists(pid, grid.cells)
    cnt = np.diff(start)
    cellp = pid[order].astype(np.int64)
    rank = np.arange(order.size) - start[cellp]
    rev = order[start[cellp] + cnt[cellp] - 1 - rank] if order.size else order        # another (legitimate) summation order
    if "scatter_order" in bugs:
        order = np.where(cnt[cellp] > 32, rev, order)
    x = xyz[order]
    cp = cnt[cellp].astype(F32)[:, None]
    div = np.where((cp == 33) & ("mean_div32" in bugs), F32(32), cp)
    m = (po.ordered_sum32(xyz, start, rev)[cellp] / div).astype(F32) if order.size else x
    m = np.where(cp == 1, x, m)
    feats = np.concatenate([x, (x - m).astype(F32), off[order]], 1).astype(F32)
    v = (feats[:, :1] * p["w"][0][None]).astype(F32)
    for q in range(1, 9):
        v = fma32(feats[:, q:q + 1], p["w"][q][None], v)
    out = dict(xyz_t=xyz, pid=pid, offsets=off, start=start, order=order, feats=feats, v=v, cell=cellp, cp=cp, cnt=cnt, rank=rank)
    out["image"] = emu_image(out, grid, p["scale"], p["shift"], bugs)
    return out


def emu_image(o, grid, scale, shift, bugs=()):
    y = ((o["v"] * scale[None]).astype(F32) + shift[None]).astype(F32)
    r = np.maximum(y, F32(0))
    if "drop_last_chunk" in bugs:
        r = np.where(((o["cp"] == 33) & (o["rank"][:, None] >= 32)), F32(0), r)
    n = o["order"].size
    pos = o["start"][o["cell"]] + o["cnt"][o["cell"]] - 1 - o["rank"] if n else np.arange(0)
    return (po.ordered_sum32(r, o["start"], pos) / np.maximum(o["cnt"], 1).astype(F32)[:, None]).astype(F32)


def emu_stats(members, p, rm, rv, bugs=()):
    """one group -> scale, shift, mean, invstd (float32), new running mean / var"""
    mem = members[:1] if "per_sweep_stats" in bugs else members
    v = np.concatenate([o["v"] for o in mem]).astype(F64)
    n = v.shape[0]
    g, b = p["gamma"], p["beta"]
    if n == 0:
        sc = (g / np.sqrt((rv if rv is not None else F32(1)) + F32(EPS), dtype=F32)).astype(F32)
        z = np.zeros(32, F32)
        return sc, (b - (rm if rm is not None else z) * sc).astype(F32), z, z, rm, rv
    mean = v.sum(0) / n
    var = np.maximum((v * v).sum(0) / n - mean * mean, 0.0)
    norm = var * n / (n - 1) if ("unbiased_norm" in bugs and n > 1) else var
    inv = (1.0 / np.sqrt(norm + float(F32(EPS)))).astype(F32)
    sc = (g * inv).astype(F32)
    sh = (b - (mean.astype(F32) * sc).astype(F32)).astype(F32)
    if rm is not None:
        mo = float(F32(MOM))
        unb = var * n / (n - 1) if n > 1 else var
        rm, rv = ((1 - mo) * rm.astype(F64) + mo * mean).astype(F32), ((1 - mo) * rv.astype(F64) + mo * unb).astype(F32)
    return sc, sh, mean.astype(F32), inv, rm, rv


def _dw32(feats, dy):
    """sum over the points of f_k dy in float32: partial sums of 32 points, then their sum"""
    out = np.zeros((9, 32), F32)
    for k in range(9):
        t = (feats[:, k:k + 1] * dy).astype(F32)
        parts = np.add.reduceat(t, np.arange(0, t.shape[0], 32), axis=0, dtype=F32) if t.shape[0] else np.zeros((1, 32), F32)
        out[k] = parts.sum(0, dtype=F32)
    return out


def emu_backward(outs, dimgs, sc, sh, mean=None, inv=None, n_groups=1, bugs=()):
    sc, sh = sc.reshape(-1, 32), sh.reshape(-1, 32)
    dW = np.zeros((9, 32), F32)
    q = []
    for i, (o, d) in enumerate(zip(outs, dimgs)):
        g_ = i % n_groups
        y = ((o["v"] * sc[g_][None]).astype(F32) + sh[g_][None]).astype(F32)
        on = (o["v"] > 0) if "mask_v" in bugs else (y > 0)
        gi = (d[o["cell"]] / o["cp"]).astype(F32)
        q.append(dict(o=o, g=np.where(on, gi, F32(0)).astype(F32), grp=g_))
    if mean is None:
        s = np.ones((1, 32), F32) if "dw_no_scale" in bugs else sc[0][None]
        return dict(dW=_dw32(q[0]["o"]["feats"], (q[0]["g"] * s).astype(F32)))
    mean, inv = mean.reshape(-1, 32), inv.reshape(-1, 32)
    dg, db = np.zeros(32, F32), np.zeros(32, F32)
    for g_ in range(n_groups):
        mem = [e for e in q if e["grp"] == g_]
        for e in mem:
            e["xh"] = ((e["o"]["v"] - mean[g_][None]) * inv[g_][None]).astype(F32)
        a0 = sum(e["g"].astype(F64).sum(0) for e in mem)
        a1 = sum((e["g"].astype(F64) * e["xh"]).sum(0) for e in mem)
        n = sum(e["g"].shape[0] for e in mem)
        dg, db = (dg + a1.astype(F32)).astype(F32), (db + a0.astype(F32)).astype(F32)
        if n == 0:
            continue
        if "meang_one_sweep" in bugs and mem[0]["g"].shape[0]:
            e = mem[0]
            k2, k3 = (e["g"].astype(F64).sum(0) / e["g"].shape[0]).astype(F32), ((e["g"].astype(F64) * e["xh"]).sum(0) / e["g"].shape[0]).astype(F32)
        else:
            k2, k3 = (a0 / n).astype(F32), (a1 / n).astype(F32)
        s = np.ones((1, 32), F32) if "dw_no_scale" in bugs else sc[g_][None]
        for e in mem:
            dy = (s * ((e["g"] - k2[None]).astype(F32) - (e["xh"] * k3[None]).astype(F32)).astype(F32)).astype(F32)
            dW = (dW + _dw32(e["o"]["feats"], dy)).astype(F32)
    return dict(dW=dW, dgamma=dg, dbeta=db)


def emu_incremental(images, nonempty, bugs=()):
    """the persistent image after every pass: non-empty cells written, cells that emptied zeroed, the rest left alone"""
    img = np.full(images[0].shape, np.nan, F32)
    was = np.ones(nonempty[0].shape, bool)                     # after himo_pillar_occupancy_reset: every cell dirty
    out = []
    for k, (im, ne) in enumerate(zip(images, nonempty)):
        clear = ~ne & was
        if "stale_next_block" in bugs and k:                    # from the second pass on: the first cell of every later 64-block
            clear[64::64] = False
        img[ne], img[clear] = im[ne], 0
        was = ne
        out.append(img.copy())
    return out


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
NAMES = list(po.SCENES)
_CACHE = {}


def case(name, seed=0):
    """seed: the gradient / running-statistics draw (the scenes and parameters stay)"""
    if (name, seed) not in _CACHE:
        grid, T, pts = po.build_scene(name)
        rng = np.random.default_rng(31 * NAMES.index(name) + 1000 * seed)
        _CACHE[(name, seed)] = dict(grid=grid, T=T, pts=pts, ptsB=po.build_scene(name, seed=1)[2], p=po.params(NAMES.index(name)),
                                    dimg=rng.standard_normal((2, grid.cells, 32)).astype(F32),
                                    dhx=rng.standard_normal((pts.shape[0], 128)).astype(F32),
                                    rm=rng.uniform(-0.1, 0.1, 32).astype(F32), rv=rng.uniform(0.5, 1.5, 32).astype(F32))
    return _CACHE[(name, seed)]


def run_all(name, bugs=(), seed=0):
    """every check of the oracle on one case, the kernel played by the emulation -> [(family, worst, rms ratio)]"""
    c = case(name, seed)
    grid, p = c["grid"], c["p"]
    res = []
    a = emu_forward(c["pts"], c["T"], grid, p, bugs)
    b = emu_forward(c["ptsB"], c["T"], grid, p, bugs)
    res.append(("image",) + po.check_forward(a, c["pts"], c["T"], grid, p, name))
    # incremental images: A, B, an empty sweep, A, A
    e = emu_forward(c["pts"][:0], c["T"], grid, p, bugs)
    seq = [a, b, e, a, a]
    for k, (im, o) in enumerate(zip(emu_incremental([o["image"] for o in seq], [o["cnt"] > 0 for o in seq], bugs), seq)):
        po.exact(f"incremental pass {k}", im, o["image"], name)
    # scatter
    b0, dec = po.scatter_ref(a["start"], a["order"], c["dhx"], 0, 2, 3)
    if "g1_to_g0" in bugs:
        b0[:, 0], b0[:, 2] = b0[:, 2].copy(), 0
    if "scatter_order" in bugs:
        dec = po.ordered_sum32(c["dhx"][:, 64:128], a["start"], a["order"])
    w0, w1 = po.scatter_ref(*po.cell_lists(a["pid"], grid.cells), c["dhx"], 0, 2, 3)
    po.exact("d_b0", b0, w0, name)
    po.exact("d_dec", dec, w1, name)
    # frozen backward
    sw = [(a["xyz_t"], a["pid"], c["dimg"][0])]
    ref = po.backward_ref(sw, grid, p["w"], p["scale"], p["shift"])
    assert ref["undecided"] <= po.UNDECIDED_CAP * max(ref["pairs"], 1), (name, ref["undecided"], ref["pairs"])
    got = emu_backward([a], c["dimg"][:1], p["scale"], p["shift"], bugs=bugs)
    res.append(("dW frozen",) + po.verify("dW", got["dW"], *ref["dW"], case=name))
    # BatchNorm training path: one group of two sweeps, then each sweep its own group
    for n_groups in (1, 2):
        groups = [[a, b]] if n_groups == 1 else [[a], [b]]
        st = [emu_stats(m, p, c["rm"], c["rv"], bugs) for m in groups]
        for g_, (m, s) in enumerate(zip(groups, st)):
            want = po.bn_stats_ref([(o["xyz_t"], o["pid"]) for o in m], grid, p["w"], p["gamma"], p["beta"], EPS, MOM, c["rm"], c["rv"])
            for key, val in zip(("scale", "shift", "mean", "invstd", "running_mean", "running_var"), s):
                res.append((f"stats {key}",) + po.verify(key, val, *want[key], case=f"{name} groups={n_groups}"))
        sc, sh, mu, iv = (np.stack([s[k] for s in st]) for k in range(4))
        sw = [(a["xyz_t"], a["pid"], c["dimg"][0]), (b["xyz_t"], b["pid"], c["dimg"][1])]
        ref = po.backward_ref(sw, grid, p["w"], sc, sh, mu, iv, n_groups)
        assert ref["undecided"] <= po.UNDECIDED_CAP * max(ref["pairs"], 1), (name, ref["undecided"], ref["pairs"])
        got = emu_backward([a, b], c["dimg"], sc, sh, mu, iv, n_groups, bugs)
        for key in ("dW", "dgamma", "dbeta"):
            res.append((f"bn {key}",) + po.verify(key, got[key], *ref[key], case=f"{name} groups={n_groups}",
                                                  limit=po.R_BN_DW if key == "dW" else None))
    return res


@pytest.mark.parametrize("name", NAMES)
def test_correct_twin_accepted_and_cap_met(name):
    for fam, worst, rr in run_all(name):
        assert worst <= 1.0 and rr <= (po.R_BN_DW if fam == "bn dW" else po.R["f32"]), (name, fam, worst, rr)


def test_bn_dw_limit_rests_on_the_correct_twin():
    """R_BN_DW (oracle docstring): over scenes 1x1 .. 41x25 and four gradient draws each, the emulated CORRECT kernel exceeds
    R["f32"] on the dW of the batch-statistics backward somewhere, never exceeds 3.6 = R_BN_DW / 2, and keeps R["f32"] elsewhere"""
    top = 0.0
    for name in NAMES[:7]:
        for seed in range(4):
            for fam, worst, rr in run_all(name, (), seed):
                assert worst <= 1.0, (name, seed, fam, worst)
                if fam == "bn dW":
                    top = max(top, rr)
                else:
                    assert rr <= po.R["f32"], (name, seed, fam, rr)
    assert po.R["f32"] < top <= 3.6 == po.R_BN_DW / 2, top


# emulated wrong kernel -> the checks (names as the oracle reports them) of which one must be the first to fail
BUGS = {"fma_transform": ("xyz_t",), "le_upper": ("pid",), "centre_half": ("offsets",), "scatter_order": ("ascending point order",),
        "drop_last_chunk": ("image",), "mean_div32": ("image",), "stale_next_block": ("incremental pass 1", "incremental pass 2"),
        "mask_v": ("dW", "dgamma", "dbeta"), "unbiased_norm": ("scale", "invstd"), "per_sweep_stats": ("scale", "shift", "mean", "invstd"),
        "meang_one_sweep": ("dW",), "dw_no_scale": ("dW",), "g1_to_g0": ("d_b0",)}


@pytest.mark.parametrize("bug", list(BUGS))
def test_wrong_kernel_rejected(bug):
    rejected = []
    for name in ("7x5", "65x1", "64x1", "41x25"):
        try:
            run_all(name, (bug,))
        except AssertionError as e:
            assert any(f"{name} {k}" in str(e) or f" {k} [" in str(e) or f" {k}:" in str(e) for k in BUGS[bug]), f"{bug} on {name}: rejected by another check: {e}"
            rejected.append(name)
    assert rejected, f"{bug}: accepted on every case"


def test_boundary_rows_mean_what_they_say():
    """on the dyadic grids the float32 transform lands on the faces, and the emulation keeps / drops as intended"""
    full = 0
    for name, (grid, _, _, kind, _, faces) in po.SCENES.items():
        if not faces:
            continue
        T = po.rigid(kind)
        rows, kept, hit = po.boundary_rows(grid, T)
        pid, off = po.cells_of(po.transform(rows, T), grid)
        assert np.array_equal((pid >= 0)[hit], kept[hit]), name
        assert not off[pid < 0].any()
        full += bool(hit.all())
    assert full >= 1


def test_split_words_layout():
    x = np.arange(64, dtype=F32).reshape(2, 32) * F32(1.0009765625) + F32(0.3)
    w = po.split_words(x).view(np.uint16).reshape(2, 2, 2, 16)
    h = w[:, :, 0].view(np.float16).astype(F32).reshape(2, 32)
    l = w[:, :, 1].view(np.float16).astype(F32).reshape(2, 32)
    assert np.array_equal(h, x.astype(np.float16).astype(F32))
    assert np.array_equal(l, (x - h).astype(np.float16).astype(F32))
