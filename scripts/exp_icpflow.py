"""Time of the ICP-Flow baseline (himo_amd/icpflow.py, csrc/icpflow.hip) per stage on a synthetic 120 000-point sweep pair of the
"rings" cloud: clusters (ego transform, DBSCAN, sort, the pair's one host wait), vote, iterations (apply + search + step, iters + 1
passes), apply (the flow), each bracketed by HIP events on the launch stream; beside it, for context only, the FastNSF fit of the same
pair -- the baseline a user would otherwise wait for.  Prints what is measured; promises and gates nothing.

    python scripts/exp_icpflow.py [--points 120000] [--warmup 5] [--pairs 30] [--nsf_iters 100] [--out profiles/extract_icpflow.txt]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--nsf_iters", type=int, default=100)
    ap.add_argument("--nsf_pairs", type=int, default=3)
    ap.add_argument("--out", default="profiles/extract_icpflow.txt")
    a = ap.parse_args()
    if a.warmup < 5 or a.pairs < 30:
        raise SystemExit("at least 5 warm-ups and 30 timed pairs")

    import torch
    from himo_amd import _lib
    from himo_amd.fastnsf import FastNSF
    from himo_amd.icpflow import IcpFlow
    from himo_amd.synthetic import make_scene
    dev = _lib.require_gpu()
    frames = make_scene(11, 2, n_points=a.points, scene_id="exp", cloud="rings")
    f0, f1 = frames[0], frames[1]
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
    pair = (up(f0["pc0"], torch.float32), up(f1["pc0"], torch.float32), up(f0["gm0"], torch.bool), up(f1["gm0"], torch.bool), f0["pose0"], f1["pose0"])
    icp = IcpFlow(dev)
    for _ in range(a.warmup):
        icp.fit(*pair)
    torch.cuda.synchronize()
    stages, whole = {}, []
    for _ in range(a.pairs):
        icp.stage_events = []
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        icp.fit(*pair)
        t1.record()
        t1.synchronize()
        whole.append(t0.elapsed_time(t1))
        for name, s, e in icp.stage_events:
            stages.setdefault(name, []).append(s.elapsed_time(e))
    icp.stage_events = None
    st = icp.last_status
    _lib.prof_start("icp_")
    for _ in range(5):
        icp.fit(*pair)
    kernels = _lib.prof_stop()
    nsf = FastNSF(device=dev, iters=a.nsf_iters)
    nsf.fit(pair[0], pair[1], pair[4], pair[5])
    torch.cuda.synchronize()
    nsf_ms = []
    for _ in range(a.nsf_pairs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        nsf.fit(pair[0], pair[1], pair[4], pair[5])
        t1.record()
        t1.synchronize()
        nsf_ms.append(t0.elapsed_time(t1))
    med = lambda v: float(np.median(v))
    total = med(whole)
    lines = [f"icpflow: one pair of {a.points}-point rings sweeps, {a.warmup} warm-ups, {a.pairs} timed pairs, HIP events ({torch.cuda.get_device_name(dev)})",
             f"  clusters {len(st)} (accepted {int((st[:, 0] == 0).sum())}, failed {int((st[:, 0] == 1).sum())}, rejected {int((st[:, 0] == 2).sum())}), "
             f"iters {icp.params.iters}, vote half {icp.params.half} x bin {icp.params.bin} m",
             f"  whole fit: median {total:.3f} ms, min {min(whole):.3f} ms, max {max(whole):.3f} ms -> {1e3 / total:.1f} pairs/s"]
    for name in ("clusters", "vote", "iterations", "apply"):
        if name in stages:
            lines.append(f"  {name:<10s}: median {med(stages[name]):.3f} ms ({100 * med(stages[name]) / total:.1f} % of the fit), min {min(stages[name]):.3f} ms")
    if "vote" in stages and stages["vote"] and med(stages["vote"]) > 0.5 * total:
        lines.append(f"  the vote dominates: {med(stages['vote']) / max(total - med(stages['vote']), 1e-9):.1f} x everything else")
    for name, k in sorted(kernels.items()):
        lines.append(f"  {name}: avg {k['avg_ms'] * 1e3:.1f} us, min {k['min_ms'] * 1e3:.1f} us over {k['count']} launches")
    lines.append(f"  for context only -- FastNSF fit of the same pair, {a.nsf_iters} iterations, one at a time: median {med(nsf_ms):.1f} ms over {a.nsf_pairs} fits "
                 f"({med(nsf_ms) / total:.1f} x the icpflow fit)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
