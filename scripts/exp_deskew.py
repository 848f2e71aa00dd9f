"""Timing of ego de-skew (himo_amd/deskew.py, csrc/deskew.hip): ``himo_deskew_tref`` + ``himo_deskew_rows`` on one 120 000-row synthetic
sweep (``make_scene``) and on a batch of 32 such sweeps in one call, beside ``himo_rigid_transform`` -- the package's streaming move,
about 32 B a row against about 36 B here -- over the same rows in the same process, the two taking turns.  Device events around every
call, the median (min, max) of 60 calls after 10 warm-ups; the two kernels also by the library's event scopes in a run of their own;
the ratio and the achieved bytes per second.  The first sweep is first compared with ``tests/deskew_ref.py``.  Sets no bar.

    python scripts/exp_deskew.py [OUT]          # OUT: the file the lines are also written to (profiles/deskew.txt)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from himo_amd import _lib                                                   # noqa: E402
from himo_amd.deskew import EgoDeskew, twists_from_poses                     # noqa: E402
import himo_amd.seflow.ssl_label                                             # noqa: E402,F401  (registers himo_rigid_transform)
from himo_amd.sweeps import sweep_offsets                                    # noqa: E402
from himo_amd.synthetic import make_scene                                    # noqa: E402
import deskew_ref as ref                                                     # noqa: E402

REPS, WARM = 60, 10
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def timed_turns(fns):
    """every callable of ``fns`` in turn within a repetition: per callable the median (min, max) ms of REPS calls after WARM warm-ups"""
    for _ in range(WARM):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for _ in fns]
    for i in range(REPS):
        for k, fn in enumerate(fns):
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    res = []
    for k in range(len(fns)):
        ms = sorted(a.elapsed_time(b) for a, b in ev[k])
        res.append((ms[len(ms) // 2], ms[0], ms[-1]))
    return res


def leg(name, eng, dev, frames, tw, pitch):
    lib, P, s = eng.lib, _lib.ptr, _lib.stream_handle
    B = len(frames)
    pts = [np.ascontiguousarray(f["pc0"][:, :pitch]) for f in frames]
    h_off = sweep_offsets([len(p) for p in pts])
    n = int(h_off[-1])
    cat = torch.from_numpy(np.concatenate(pts)).to(dev)
    dt = torch.from_numpy(np.concatenate([f["lidar_dt"] for f in frames])).to(dev)
    d_off, d_tw = torch.from_numpy(h_off).to(dev), torch.from_numpy(tw).to(dev)
    moved = torch.empty((n, pitch), dtype=torch.float32, device=dev)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    disp, tref = torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
    T32 = torch.from_numpy(np.eye(4, dtype=np.float32)).to(dev)
    T32[0, 3] = 0.5

    def f_tref():
        _lib.check(lib.himo_deskew_tref(B, n, h_off.ctypes.data, P(d_off), P(dt), 0, P(tref), s()), "tref")

    def f_rows():
        _lib.check(lib.himo_deskew_rows(B, n, h_off.ctypes.data, P(d_off), P(cat), pitch, P(dt), tw.ctypes.data, P(d_tw), P(tref), 0, P(moved), pitch,
                                        P(counts), P(disp), s()), "rows")

    def f_both():
        f_tref()
        f_rows()

    def f_rigid():
        _lib.check(lib.himo_rigid_transform(n, P(cat), pitch, P(T32), P(moved), pitch, s()), "rigid")

    t_both, t_rigid, t_tref, t_rows = timed_turns([f_both, f_rigid, f_tref, f_rows])
    fmt = lambda t: "%.4f ms (min %.4f max %.4f)" % t          # noqa: E731
    here, there = n * (4 * pitch + 4 + 4 * pitch), n * (8 * pitch)
    say(f"[{name}, pitch {pitch}] {B} sweep(s), {n} rows")
    say(f"[{name}, pitch {pitch}]   himo_deskew_tref + himo_deskew_rows  {fmt(t_both)}   {here / 1e6:.2f} MB -> {here / (t_both[0] * 1e-3) / 1e12:.3f} TB/s")
    say(f"[{name}, pitch {pitch}]     himo_deskew_tref alone             {fmt(t_tref)}")
    say(f"[{name}, pitch {pitch}]     himo_deskew_rows alone (+ clear)   {fmt(t_rows)}   -> {here / (t_rows[0] * 1e-3) / 1e12:.3f} TB/s")
    say(f"[{name}, pitch {pitch}]   himo_rigid_transform                 {fmt(t_rigid)}   {there / 1e6:.2f} MB -> {there / (t_rigid[0] * 1e-3) / 1e12:.3f} TB/s")
    say(f"[{name}, pitch {pitch}]   ratio both / rigid {t_both[0] / t_rigid[0]:.2f}, rows / rigid {t_rows[0] / t_rigid[0]:.2f} (bytes {here / there:.2f}); "
        "HBM: 8.0 TB/s peak")
    _lib.prof_start("deskew_")
    for _ in range(20):
        f_both()
    torch.cuda.synchronize()
    for kname, v in sorted(_lib.prof_stop().items()):
        say(f"[{name}, pitch {pitch}]     {kname}: {v['avg_ms'] * 1e3:.1f} us avg (min {v['min_ms'] * 1e3:.1f}) over {v['count']}")


def main():
    dev = _lib.require_gpu()
    eng = EgoDeskew(dev)
    frames = make_scene(5, 4, n_points=120_000, n_instances=30)
    tw = twists_from_poses(np.stack([f["pose0"] for f in frames]), "backward", 0.1)
    # the first sweep against the restatement
    got, counts, disp = eng.sweeps([frames[0]["pc0"]], [frames[0]["lidar_dt"]], tw[:1])
    want, wc, wd, wt = ref.deskew(frames[0]["pc0"], frames[0]["lidar_dt"], tw[0])
    g = got[0].cpu().numpy()
    diff = int((g.view(np.uint32) != want.view(np.uint32)).sum())
    ulp = np.abs(g.astype(np.float64) - want) <= np.maximum(np.spacing(np.abs(g)), np.spacing(np.abs(want)))
    say(f"120k-row sweep against tests/deskew_ref.py: {diff} of {g.size} values not bit-identical, all within 1 float32 ulp {bool(ulp.all())}; counts "
        f"{counts[0].tolist()} (restatement {wc.tolist()}), max_disp {disp[0]:.6f} m (restatement {wd:.6f}), t_ref equal {eng.t_ref[0] == wt}")
    for pitch in (4, 3):
        leg("one sweep", eng, dev, frames[:1], tw[:1], pitch)
        batch = [frames[k % len(frames)] for k in range(32)]
        leg("batch of 32", eng, dev, batch, np.ascontiguousarray(tw[[k % len(frames) for k in range(32)]]), pitch)


if __name__ == "__main__":
    main()
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text("\n".join(out) + "\n")
