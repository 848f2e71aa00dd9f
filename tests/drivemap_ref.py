"""The checker of the whole-drive free-space map: a numpy restatement of "free-space drive map, v1" (the module docstring of
``himo_amd/drivemap.py`` is the text), built on the restatement of "free-space ray map, v1" (tests/raymap_ref.py), whose rules A-C it
uses as they are.  Rule D' is stated sweep by sweep, without the device's word: every sweep carves a FRESH v1 map with slot = ``src``;
``free_k`` = any FREE bit, ``hit_k`` = any HIT bit; ``free_n += free_k & ~hit_k``, ``hit_n += hit_k``.  Then rules E' and S, with the
emit order and the centre arithmetic.  Nothing under ``himo_amd/`` imports it; it imports nothing from there either."""
import numpy as np

import raymap_ref as rr

DEFAULTS = dict(x0=-51.2, y0=-51.2, z0=-3.0, voxel=0.2, nx=512, ny=512, nz=30, guard=2, min_votes=2, min_hits=2)
MAX_SWEEP = 65534

f32 = np.float32


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def v1_rule(**kw):
    """the keywords tests/raymap_ref.py takes, of this rule's"""
    p = params(**kw)
    return {k: p[k] for k in rr.DEFAULTS}


class DriveMap:
    """``free_n`` / ``hit_n`` (uint16 [nz, ny, nx]) of the sweeps carved so far.  The rays of one sweep may come in several calls, in
    any order and more than once; sweep numbers do not decrease."""

    def __init__(self, **kw):
        self.rule = params(**kw)
        self.v1 = v1_rule(**kw)
        shape = (int(self.rule["nz"]), int(self.rule["ny"]), int(self.rule["nx"]))
        self.free_n, self.hit_n = np.zeros(shape, np.uint16), np.zeros(shape, np.uint16)
        self.sweep, self.cur = None, None

    def _of_current(self):
        """(free_k & ~hit_k, hit_k) of the sweep being carved"""
        if self.cur is None:
            return None
        free_k, hit_k = (self.cur & np.uint32(0xFFFF)) != 0, (self.cur >> np.uint32(16)) != 0
        return free_k & ~hit_k, hit_k

    def carve(self, pts, src, origins, sweep):
        """the rays origins[src[i]] -> pts[i] of sweep ``sweep``; a src byte in 16..254: ValueError, nothing marked"""
        sweep = int(sweep)
        if not 0 <= sweep <= MAX_SWEEP:
            raise ValueError(f"sweep {sweep}: 0..{MAX_SWEEP}")
        if self.sweep is not None and sweep < self.sweep:
            raise ValueError(f"sweep {sweep} after sweep {self.sweep}")
        if sweep != self.sweep:
            done = self._of_current()
            if done is not None:
                self.free_n += done[0]
                self.hit_n += done[1]
            self.sweep, self.cur = sweep, rr.new_map(**self.v1)
        return rr.carve(self.cur, pts, src, origins, **self.v1)

    def counts(self):
        """(free_n, hit_n) with the sweep being carved counted in; carving may go on afterwards"""
        now = self._of_current()
        if now is None:
            return self.free_n.copy(), self.hit_n.copy()
        return self.free_n + now[0], self.hit_n + now[1]

    def query(self, pts, skip=None):
        """rule E': (dynamic bool [N], fv uint16 [N], hv uint16 [N])"""
        free_n, hit_n = self.counts()
        pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
        u, usable = rr.quantise(pts, **self.v1)
        v = u >> 8
        live = usable & rr.in_grid(v, **self.v1)
        if skip is not None:
            live &= np.asarray(skip).reshape(-1) == 0
        fv, hv = np.zeros(len(pts), np.uint16), np.zeros(len(pts), np.uint16)
        fv[live] = free_n[v[live, 2], v[live, 1], v[live, 0]]
        hv[live] = hit_n[v[live, 2], v[live, 1], v[live, 0]]
        return live & (fv >= int(self.rule["min_votes"])) & (fv > hv), fv, hv

    def static(self):
        """rule S: bool [nz, ny, nx]"""
        free_n, hit_n = self.counts()
        return (hit_n >= int(self.rule["min_hits"])) & ~((free_n >= int(self.rule["min_votes"])) & (free_n > hit_n))

    def emit(self):
        """rule S: (rows float32 [M, 4], hits int32 [M], free int32 [M]) in ascending linear voxel index (vz*ny + vy)*nx + vx"""
        free_n, hit_n = self.counts()
        idx = np.nonzero(self.static().reshape(-1))[0]                    # ascending
        nx, ny = int(self.rule["nx"]), int(self.rule["ny"])
        vx, vy, vz = idx % nx, (idx // nx) % ny, idx // (nx * ny)
        voxel = f32(self.rule["voxel"])
        rows = np.zeros((len(idx), 4), np.float32)
        for col, (v, m) in enumerate(((vx, "x0"), (vy, "y0"), (vz, "z0"))):
            half = (v.astype(np.float32) + f32(0.5)).astype(np.float32)    # every operation rounds on its own
            rows[:, col] = ((half * voxel).astype(np.float32) + f32(self.rule[m])).astype(np.float32)
        return rows, hit_n.reshape(-1)[idx].astype(np.int32), free_n.reshape(-1)[idx].astype(np.int32)


def counts_of_words(words):
    """(free_n, hit_n) of the device's map words (uint64): bits 31..16 and 15..0"""
    w = np.asarray(words, dtype=np.uint64)
    return ((w >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16), (w & np.uint64(0xFFFF)).astype(np.uint16)


def relative_poses(poses):
    """rule G': T_k = inv(pose_0) @ pose_k in float64, rounded to float32"""
    inv0 = np.linalg.inv(np.asarray(poses[0], np.float64))
    return [(inv0 @ np.asarray(p, np.float64)).astype(np.float32) for p in poses]
