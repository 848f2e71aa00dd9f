"""Ego-motion de-skew: every row of every sweep moved along the ego vehicle's own motion from its capture time to the sweep's reference
time, on the GPU (``python -m himo_amd.deskew``).  Every program of this package assumes sweeps in which the ego motion during the
roughly 0.1 s of capture has been taken out already (the reference's data arrives "w. ego-motion comp."); this one makes that state for
drives that lack it, from a stored pose key -- ``pose``, or ``pose_odom`` of ``python -m himo_amd.odometry``.  The chain for a raw drive:
``extract -> odometry -> deskew -> ground_seg -> raymap -> fit / save -> save_zip``.

PARITY UNPINNED.  The reference has no such stage.  This one follows the build's own written rule, below, and is checked against a
numpy restatement of it (``tests/deskew_ref.py``), never against the reference.  It is opt-in: nothing calls it unless asked, and no
existing output changes.  Nothing has been tried on field data.

The rule -- "ego de-skew, v1" (normative)
=========================================
Inputs per sweep: ``pts`` float32 [n][pitch] (pitch 3 or 4), ``lidar_dt`` float32 [n] in seconds, a twist ``xi = (v, w)`` float64 in
the sweep's own frame per ``span`` seconds, ``span`` > 0, a reference mode.

Reference time ``t_ref`` (float32): ``max`` (the default; the convention of ``utils.dt0_from_lidar_dt``, save_zip.py:120) the greatest
finite ``lidar_dt`` of the sweep; ``min`` the least; ``zero`` 0.  A sweep without a finite ``lidar_dt`` gets ``t_ref = 0`` and all its
rows pass through.

Per row, in float64: ``s = ((double)t_ref - (double)dt) / span`` and ``g = -s`` (``g = +s`` with ``inverse``, the re-skew that the
round trip needs).  The move is ``p' = Exp(g xi) p``.  With ``ww = (wx*wx + wy*wy) + wz*wz``:

* ``ww < 1e-16``: the first-order form ``d = g (w x p) + g v``, each component as ``g*c + g*v`` with ``c = w x p``.
* otherwise ``theta = sqrt(ww)``, ``n = w / theta``, ``A = n x v``, ``B = n x A``, ``phi = g theta``, and
  ``d = (((sin(phi) (n x p) + (1 - cos(phi)) (n x (n x p))) + g v) + ((1 - cos(phi)) / theta) A) + ((phi - sin(phi)) / theta) B``
  component by component in that order, where ``sin(phi) = (2 sh) ch`` and ``1 - cos(phi) = (2 sh) sh`` with ``sh = sin(phi / 2)``,
  ``ch = cos(phi / 2)`` (the half angle keeps ``1 - cos`` from cancelling at small ``phi``).

Every cross product is ``a1*b2 - a2*b1`` per component; every operation rounds on its own (``himo_amd/csrc/deskew.hip`` is built with
``-ffp-contract=off``).  ``p' = p + d`` is rounded ONCE to float32.  The device uses ``sin`` / ``cos`` in float64, one pair per moved
row: this is the one place where the project's "no transcendental on the device" habit is relaxed.  Only the scalar ``phi / 2`` needs
them -- no decision hangs on their last bit -- and the comparison with the restatement is by tolerance (one float32 ulp), not by bytes.

Rows that keep their bytes, all columns, and are counted as passed through: a row with ``s == 0``; a row with a non-finite coordinate
or a non-finite ``lidar_dt``; every row of a sweep whose twist is all zeros.  Column 3 (intensity) is copied (0 where a pitch-3 input
is written at pitch 4).  The row count and the row order never change, so every per-point key stays row-aligned.

Per sweep: ``counts`` int32 [2] (rows moved, rows passed through) and ``max_disp`` float32, the greatest ``|d|`` of the moved rows --
``sqrt((dx*dx + dy*dy) + dz*dz)`` in float64, rounded once -- combined with an integer atomic max on the bits of a non-negative float.
There are no floating-point atomics: the same inputs give the same bytes on every run.

The twist from poses (host, float64 numpy, the closed-form SE(3) logarithm; ``twists_from_poses``): ``rel_k = inv(P_{k-1}) P_k``.
``backward`` (default): sweep ``k`` takes ``Log(rel_k)``, sweep 0 takes ``Log(rel_1)`` -- ``P_k`` is taken to be the pose at ``t_ref``,
so ``rel_k`` is the motion DURING sweep ``k``.  ``forward``: ``Log(rel_{k+1})``, the last sweep ``Log(rel_{K-1})``.  ``central``: the
mean of the two 6-vectors (and of their spans); at either end of a scene the one that exists.  ``Log``: ``r = vee(R - R^T) / 2``,
``theta = atan2(|r|, (tr R - 1) / 2)``, ``w = r theta / |r|`` (``w = r`` below 1e-8 rad), ``v = t - (w x t) / 2 + c (w x (w x t))``
with ``c = (1 - (theta / 2) / tan(theta / 2)) / theta^2`` (1/12 below 1e-8 rad).  The span: ``fixed`` (default) ``sensor_dt`` = 0.1 s;
``stamps`` the timestamp difference, in ns, of the pose pair used.  Refused with a clear error: a rotation angle >= pi / 2 per sweep,
a non-finite pose, a span not > 0.  A one-sweep scene has a zero twist: its rows are unchanged, and it is listed in the table.

Not part of v1: a twist that changes inside a sweep, IMU input, per-sensor extrinsics / ``SensorsCenter``, de-skew inside
``odometry``'s loop, the npz container, an in-line switch of ``save``.

The program: ``python -m himo_amd.deskew --data_dir D --out_dir O [--pose_key pose] [--twist backward|forward|central]
[--ref max|min|zero] [--span fixed|stamps] [--sensor_dt 0.1] [--batch SWEEPS] [--inverse] [--json PATH] [--overwrite]``.  It takes
``.h5`` scene directories (the npz container is refused), walks whole scenes (``sweeps.sharded_scenes``), ``--batch`` sweeps per call,
and writes ``O/<scene>.h5`` through ``h5lite.write_file``: ``lidar`` replaced by the de-skewed rows (same shape and dtype), every other
dataset of the group carried over unchanged, a new ``<timestamp>/deskew`` float64 [8] = ``v``, ``w``, ``span``, ``t_ref``, and the
index file as ``accumulate`` writes it.  Refused: ``O`` equal to ``D``; a scene file in ``O`` without ``--overwrite``; input sweeps that
hold a ``deskew`` key already (compensating twice) unless ``--inverse``, which in turn requires the key, uses its stored twist and
``t_ref`` and drops the key; a missing ``--pose_key`` (the ``KeyError`` of ``dataset.py``).  It prints, per scene and over all: sweeps,
rows moved / passed through, the mean of the sweeps' ``max_disp``, the greatest ``max_disp``, and the mean speed and yaw rate of the
twists used.  Under ``torchrun`` the scenes are dealt to the ranks as elsewhere.  There is no CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

REFS = ("max", "min", "zero")
TWISTS = ("backward", "forward", "central")
SPANS = ("fixed", "stamps")
KEY = "deskew"
LOG_SMALL = 1e-8


@dataclass(frozen=True)
class DeskewParams:
    """the parameters of "ego de-skew, v1"; refuses what the rule does not admit before anything is launched"""
    ref: str = "max"
    twist: str = "backward"
    span: str = "fixed"
    sensor_dt: float = 0.1
    batch: int = 16

    def __post_init__(self):
        for name, allowed in (("ref", REFS), ("twist", TWISTS), ("span", SPANS)):
            if getattr(self, name) not in allowed:
                raise ValueError(f"DeskewParams.{name}={getattr(self, name)!r}: one of {', '.join(allowed)}")
        v = self.sensor_dt
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
            raise ValueError(f"DeskewParams.sensor_dt={v!r}: a finite, positive number of seconds")
        b = self.batch
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1 or b > 4096:
            raise ValueError(f"DeskewParams.batch={b!r}: 1..4096 sweeps per call")

    @property
    def ref_mode(self) -> int:
        return REFS.index(self.ref)


# --------------------------------------------------------------------------------------------------------------------------
# the twist from poses (host)
# --------------------------------------------------------------------------------------------------------------------------
def se3_log(T) -> np.ndarray:
    """the twist (v, w) float64 [6] with Exp(v, w) = T: the rule's closed form"""
    T = np.asarray(T, np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("a pose that is not a finite [4, 4] matrix")
    R, t = T[:3, :3], T[:3, 3]
    r = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    norm = math.sqrt(float(r @ r))
    theta = math.atan2(norm, 0.5 * (float(R[0, 0] + R[1, 1] + R[2, 2]) - 1.0))
    if theta >= math.pi / 2:
        raise ValueError(f"a rotation of {theta:.4f} rad between two sweeps: the rule admits less than pi / 2")
    if theta < LOG_SMALL:
        w, c = r, 1.0 / 12.0
    else:
        w = r * (theta / norm)
        c = (1.0 - (0.5 * theta) / math.tan(0.5 * theta)) / (theta * theta)
    wt = np.cross(w, t)
    return np.concatenate([t - 0.5 * wt + c * np.cross(w, wt), w])


def twists_from_poses(poses, mode: str = "backward", span=0.1, sensor_dt: float = 0.1) -> np.ndarray:
    """The rule's twist of every sweep of ONE scene: float64 [K, 8] = v, w, span, 0.  ``poses`` [K, 4, 4] in index order; ``span`` a
    number of seconds (``fixed``) or the K timestamps in ns (``stamps``: the difference of the pose pair used).  A one-sweep scene: a
    zero twist with the span ``span`` (``sensor_dt`` where stamps were given)."""
    if mode not in TWISTS:
        raise ValueError(f"twist mode {mode!r}: one of {', '.join(TWISTS)}")
    poses = np.asarray(poses, np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"poses of shape [K, 4, 4], not {poses.shape}")
    if not np.isfinite(poses).all():
        raise ValueError("a non-finite pose")
    K = len(poses)
    stamps = None
    if np.ndim(span) != 0:
        stamps = [int(x) for x in np.asarray(span).reshape(-1)]
        if len(stamps) != K:
            raise ValueError(f"{len(stamps)} timestamps for {K} poses")
    out = np.zeros((K, 8))
    if K == 0:
        return out
    if K == 1:
        out[0, 6] = float(sensor_dt if stamps is not None else span)
    else:
        rel = [None] + [se3_log(np.linalg.inv(poses[k - 1]) @ poses[k]) for k in range(1, K)]
        sp = [None] + [float(span) if stamps is None else (stamps[k] - stamps[k - 1]) * 1e-9 for k in range(1, K)]
        for k in range(K):
            use = {"backward": [max(k, 1)], "forward": [min(k + 1, K - 1)], "central": [j for j in (k, k + 1) if 1 <= j < K]}[mode]
            out[k, :6] = sum(rel[j] for j in use) / len(use)
            out[k, 6] = sum(sp[j] for j in use) / len(use)
    check_twists(out)
    return out


def check_twists(twists) -> np.ndarray:
    tw = np.ascontiguousarray(np.asarray(twists, np.float64))
    if tw.ndim != 2 or tw.shape[1] != 8:
        raise ValueError(f"twists of shape [B, 8] (v, w, span, spare), not {tw.shape}")
    if not np.isfinite(tw[:, :7]).all():
        raise ValueError("a twist or span that is not finite")
    if not (tw[:, 6] > 0).all():
        raise ValueError("a span that is not > 0 (timestamps that do not increase?)")
    return tw


# --------------------------------------------------------------------------------------------------------------------------
# the device
# --------------------------------------------------------------------------------------------------------------------------
class EgoDeskew:
    """``EgoDeskew(device, params).sweeps(pts_list, dt_list, twists, inverse=False)`` -> (the moved sweeps as device tensors, counts int32
    [B, 2], max_disp float32 [B]); ``.t_ref`` holds the reference times float32 [B] of the last call.  There is no CPU path."""

    def __init__(self, device=None, params: DeskewParams | None = None):
        from . import _lib
        self.params = params if params is not None else DeskewParams()
        self.lib = _lib.load()
        self.device = device if device is not None else _lib.require_gpu()
        self.t_ref = None

    def sweeps(self, pts_list, dt_list, twists, inverse: bool = False, t_ref=None, out_pitch: int | None = None):
        """One call for a ragged batch: ``pts_list`` [n_b, 3 or 4] float32 arrays or device tensors of one pitch, ``dt_list`` [n_b]
        ``lidar_dt``, ``twists`` float64 [B, 8].  ``t_ref``: None = the rule's reference time from ``lidar_dt`` on the device
        (``himo_deskew_tref``), else float32 [B] given (``--inverse`` uses the stored ones).  ``out_pitch``: None = the input's."""
        import torch
        from . import _lib
        from .sweeps import sweep_offsets
        B = len(pts_list)
        if len(dt_list) != B:
            raise ValueError(f"{B} sweeps and {len(dt_list)} lidar_dt arrays")
        tw = check_twists(np.zeros((0, 8)) if B == 0 and np.size(twists) == 0 else twists)
        if len(tw) != B:
            raise ValueError(f"{B} sweeps and {len(tw)} twists")
        dev, P = self.device, _lib.ptr
        with torch.cuda.device(dev):
            def rows(a, dtype=torch.float32):
                t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
                return t.to(device=dev, dtype=dtype)
            pts = [rows(p) for p in pts_list]
            dts = [rows(d).reshape(-1) for d in dt_list]
            pitches = {int(p.shape[1]) if p.dim() == 2 else -1 for p in pts}
            if B and (len(pitches) != 1 or not pitches <= {3, 4}):
                raise ValueError(f"sweeps of ONE pitch, 3 or 4 float32 columns, not {[tuple(p.shape) for p in pts]}")
            pitch = pitches.pop() if B else 3
            out_pitch = pitch if out_pitch is None else int(out_pitch)
            if out_pitch not in (3, 4):
                raise ValueError(f"out_pitch={out_pitch}: 3 or 4")
            counts_host = [int(p.shape[0]) for p in pts]
            for n, d in zip(counts_host, dts):
                if int(d.shape[0]) != n:
                    raise ValueError(f"a sweep of {n} rows with {int(d.shape[0])} lidar_dt values")
            h_off = sweep_offsets(counts_host)
            n = int(h_off[-1])
            cat = torch.cat(pts, 0).contiguous() if B else torch.zeros((0, pitch), dtype=torch.float32, device=dev)
            dt = torch.cat(dts, 0).contiguous() if B else torch.zeros(0, dtype=torch.float32, device=dev)
            d_off = torch.from_numpy(h_off).to(dev)
            d_tw = torch.from_numpy(tw).to(dev)
            out = torch.empty((n, out_pitch), dtype=torch.float32, device=dev)
            counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
            disp = torch.zeros(B, dtype=torch.float32, device=dev)
            s = _lib.stream_handle()
            if t_ref is None:
                tref = torch.zeros(B, dtype=torch.float32, device=dev)
                _lib.check(self.lib.himo_deskew_tref(B, n, h_off.ctypes.data, P(d_off), P(dt) if n else None, self.params.ref_mode,
                                                     P(tref) if B else None, s), "himo_deskew_tref")
            else:
                given = np.ascontiguousarray(np.asarray(t_ref, np.float32).reshape(-1))
                if len(given) != B or not np.isfinite(given).all():
                    raise ValueError(f"t_ref: {B} finite float32 values")
                tref = torch.from_numpy(given).to(dev)
            _lib.check(self.lib.himo_deskew_rows(B, n, h_off.ctypes.data, P(d_off), P(cat) if n else None, pitch, P(dt) if n else None,
                                                 tw.ctypes.data if B else None, P(d_tw) if B else None, P(tref) if B else None,
                                                 1 if inverse else 0, P(out) if n else None, out_pitch, P(counts) if B else None,
                                                 P(disp) if B else None, s), "himo_deskew_rows")
            self.t_ref = tref.cpu().numpy()
            return list(torch.split(out, counts_host, 0)) if B else [], counts.cpu().numpy(), disp.cpu().numpy()


# --------------------------------------------------------------------------------------------------------------------------
# the tables
# --------------------------------------------------------------------------------------------------------------------------
def new_sums() -> dict:
    return {"scenes": 0, "sweeps": 0, "moved": 0, "passed": 0, "disp_sum": 0.0, "disp_max": 0.0, "speed_sum": 0.0, "yaw_sum": 0.0}


def fold_sums(a: dict, b: dict) -> dict:
    return {k: max(a[k], b[k]) if k.endswith("_max") else a[k] + b[k] for k in a}


def numbers_of(s: dict) -> dict:
    from .stored import ratio
    return {"scenes": s["scenes"], "sweeps": s["sweeps"], "rows_moved": s["moved"], "rows_passed": s["passed"],
            "mean_max_disp_m": ratio(s["disp_sum"], s["sweeps"]), "max_disp_m": s["disp_max"] if s["sweeps"] else None,
            "mean_speed_mps": ratio(s["speed_sum"], s["sweeps"]), "mean_yaw_rate_dps": ratio(s["yaw_sum"], s["sweeps"])}


def _line(name: str, n: dict) -> str:
    from .stored import fmt
    return (f"  {name}: {n['sweeps']} sweeps, {n['rows_moved']} rows moved, {n['rows_passed']} passed through, max_disp mean "
            f"{fmt(n['mean_max_disp_m'], '.4f')} greatest {fmt(n['max_disp_m'], '.4f')} m, mean speed {fmt(n['mean_speed_mps'], '.2f')} m/s, mean yaw "
            f"rate {fmt(n['mean_yaw_rate_dps'], '.2f')} deg/s")


# --------------------------------------------------------------------------------------------------------------------------
# the program
# --------------------------------------------------------------------------------------------------------------------------
def _is_npz_container(root: Path) -> bool:
    return any(root.glob("*/*.npz")) and not any(root.glob("*.h5"))


def main(data_dir: str, out_dir: str, pose_key: str = "pose", twist: str = "backward", ref: str = "max", span: str = "fixed",
         sensor_dt: float = 0.1, batch: int = 16, inverse: bool = False, json_path: str | None = None, overwrite: bool = False) -> dict:
    """The program (module docstring).  Returns what ``--json`` writes: {"scenes": {scene: numbers}, "all": numbers} over every rank."""
    from . import distenv, h5lite
    from .accumulate import _write_index
    from .dataset import HDF5Dataset, _open_h5
    from .sweeps import sharded_scenes
    prm = DeskewParams(ref=ref, twist=twist, span=span, sensor_dt=sensor_dt, batch=batch)
    root, out_root = Path(data_dir), Path(out_dir)
    if out_root.resolve() == root.resolve():
        raise ValueError(f"--out_dir {out_dir}: the de-skewed scene files are written beside the input, never over it (--out_dir equals --data_dir)")
    if _is_npz_container(root):
        raise ValueError(f"{data_dir}: the npz container is not taken by this program (ego de-skew, v1 reads and writes <scene>.h5 files)")
    if not sorted(root.glob("*.h5")):
        raise FileNotFoundError(f"{data_dir}: no <scene>.h5 files")
    per_scene = {}
    with distenv.process_group() as (rank, world):
        ds = HDF5Dataset(root, vis_name="", fields=("pose0",), need_next=False, pose_key="pose" if inverse else pose_key)
        mine = sharded_scenes(ds)

        def loop():
            # the refusals, before anything touches the GPU or a file is written
            have = [sc for sc, _ in mine if (out_root / f"{sc}.h5").exists()]
            if have and not overwrite:
                raise FileExistsError(f"{out_dir}: {len(have)} scene files exist already, {have[0]}.h5 among them (--overwrite replaces them)")
            for sc, items in mine:
                with _open_h5(ds.scene_path(sc)) as h:
                    for i in items:
                        ts = ds.index[i][1]
                        g = h[ts]
                        if KEY in g and not inverse:
                            raise ValueError(f"{sc}/{ts} already holds '{KEY}': its sweeps are de-skewed, and compensating twice is refused "
                                             "(--inverse takes the compensation out again)")
                        if KEY not in g and inverse:
                            raise KeyError(f"{KEY}: {sc}/{ts} holds no such key: --inverse re-skews what this program de-skewed, by the stored twist")
                        if "lidar" not in g:
                            raise KeyError(f"lidar: {sc}/{ts} holds no sweep")
                        if not inverse:
                            ds.read(i)                                   # a missing --pose_key: the KeyError dataset.py words
            if not mine:
                return
            eng = EgoDeskew(params=prm)
            out_root.mkdir(parents=True, exist_ok=True)
            for sc, items in mine:
                stamps = [ds.index[i][1] for i in items]
                with _open_h5(ds.scene_path(sc)) as h:
                    groups = [{k: np.asarray(h[ts][k][()]) for k in h[ts].keys()} for ts in stamps]
                if inverse:
                    stored = np.stack([np.asarray(g[KEY], np.float64).reshape(8) for g in groups])
                    tw = np.concatenate([stored[:, :7], np.zeros((len(groups), 1))], axis=1)
                    given = stored[:, 7].astype(np.float32)
                else:
                    poses = np.stack([np.asarray(ds.read(i)["pose0"], np.float64) for i in items])
                    try:
                        tw = twists_from_poses(poses, prm.twist, [int(t) for t in stamps] if prm.span == "stamps" else float(prm.sensor_dt),
                                               float(prm.sensor_dt))
                    except ValueError as e:
                        raise ValueError(f"{sc}: {e}") from None
                    given = None
                sums = new_sums()
                sums["scenes"] = 1
                for lo in range(0, len(groups), prm.batch):
                    part = groups[lo:lo + prm.batch]
                    lidar = [np.asarray(g["lidar"]) for g in part]
                    for g, a, ts in zip(part, lidar, stamps[lo:]):
                        if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] not in (3, 4):
                            raise ValueError(f"{sc}/{ts}: lidar of shape {a.shape} {a.dtype}, not float32 rows of 3 or 4 columns")
                    dts = [np.asarray(g["lidar_dt"], np.float32) if "lidar_dt" in g else np.zeros(len(a), np.float32) for g, a in zip(part, lidar)]
                    by_pitch = {}
                    for j, a in enumerate(lidar):
                        by_pitch.setdefault(a.shape[1], []).append(j)
                    for pitch, js in by_pitch.items():                       # (one pitch per call; a scene has one)
                        moved, counts, disp = eng.sweeps([lidar[j] for j in js], [dts[j] for j in js], tw[[lo + j for j in js]], inverse=inverse,
                                                         t_ref=None if given is None else given[[lo + j for j in js]])
                        for j, m, c, d, tr in zip(js, moved, counts, disp, eng.t_ref):
                            g = part[j]
                            g["lidar"] = m.cpu().numpy()
                            if inverse:
                                del g[KEY]
                            else:
                                g[KEY] = np.concatenate([tw[lo + j, :7], [float(tr)]])
                            sums["sweeps"] += 1
                            sums["moved"] += int(c[0])
                            sums["passed"] += int(c[1])
                            sums["disp_sum"] += float(d)
                            sums["disp_max"] = max(sums["disp_max"], float(d))
                            sums["speed_sum"] += float(np.linalg.norm(tw[lo + j, :3]) / tw[lo + j, 6])
                            sums["yaw_sum"] += math.degrees(float(np.linalg.norm(tw[lo + j, 3:6]) / tw[lo + j, 6]))
                h5lite.write_file(out_root / f"{sc}.h5", {ts: g for ts, g in zip(stamps, groups)})
                per_scene[sc] = sums

        distenv.run_shard(loop, "its scene files", closing=(ds,))
        every = distenv.gathered(per_scene, lambda a, b: {**a, **b})
        if rank == 0 and every:
            _write_index(out_root, [[s, t] for s, t in ds.index if s in every])
        total = new_sums()
        for sc in sorted(every):
            total = fold_sums(total, every[sc])
        numbers = {"scenes": {sc: numbers_of(every[sc]) for sc in sorted(every)}, "all": numbers_of(total)}
        how = "inverse by the stored twists" if inverse else (f"pose key '{pose_key}', twist {prm.twist}, ref {prm.ref}, span {prm.span}"
                                                              + (f" {prm.sensor_dt:g} s" if prm.span == "fixed" else ""))
        head = f"deskew (ego de-skew, v1; parity unpinned), {how}, into {out_dir}:"
        lines = [head] + [_line(sc, numbers["scenes"][sc]) for sc in sorted(every)] + [_line("all", numbers["all"])]
        distenv.report(rank, "\n".join(lines), numbers, json_path)
    return numbers


def _parser():
    import argparse
    d = DeskewParams()
    ap = argparse.ArgumentParser(description="move every row of every sweep along the ego motion from its capture time to the sweep's reference "
                                             "time and write new scene files (ego de-skew, v1; parity unpinned: the reference has no such "
                                             "stage; nothing has been tried on field data; MI355X path)")
    ap.add_argument("--data_dir", required=True, help="directory of <scene>.h5 files and index_total.pkl")
    ap.add_argument("--out_dir", required=True, help="directory the de-skewed <scene>.h5 files and their index_total.pkl are written to")
    ap.add_argument("--pose_key", default="pose", help="the stored pose the twists are taken from (pose_odom: python -m himo_amd.odometry)")
    ap.add_argument("--twist", default=d.twist, choices=TWISTS, help="which pose pair gives a sweep its twist")
    ap.add_argument("--ref", default=d.ref, choices=REFS, help="the reference time of a sweep: its greatest / least finite lidar_dt, or 0")
    ap.add_argument("--span", default=d.span, choices=SPANS, help="fixed: --sensor_dt; stamps: the timestamp difference of the pose pair")
    ap.add_argument("--sensor_dt", type=float, default=d.sensor_dt, help="seconds a twist spans with --span fixed")
    ap.add_argument("--batch", type=int, default=d.batch, metavar="SWEEPS", help="sweeps per device call")
    ap.add_argument("--inverse", action="store_true", help="re-skew sweeps this program de-skewed, by their stored twist; drops the key")
    ap.add_argument("--json", default=None, metavar="PATH", help="write the table's numbers to PATH")
    ap.add_argument("--overwrite", action="store_true", help="replace scene files that exist in --out_dir instead of refusing")
    return ap


def _cli(argv=None):
    a = _parser().parse_args(argv)
    return main(a.data_dir, a.out_dir, a.pose_key, a.twist, a.ref, a.span, a.sensor_dt, a.batch, a.inverse, a.json, a.overwrite)


if __name__ == "__main__":
    _cli()
