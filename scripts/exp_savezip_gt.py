"""save_zip_gt.run_dataset: serial loop (columns decoded, host encoder) vs the overlapped feeder -> kernel -> drain form (the device
writes each sweep's record-batch body; head + pinned view + tail go to the file), sweeps/s and Feather bytes/s on 120k-point sweeps
held in host memory, and the stages of the overlapped form on their own: the feeder (pack into pinned memory + copy to the device)
and the drain (copy back + write one Feather file per sweep).  Compare the bytes/s with scripts/exp_savezip.py's sweeps/s x 12
bytes per point run in the same sitting (a ground-truth file holds 34 bytes per point).

    python scripts/exp_savezip_gt.py [N]                       every step, each as a child process under its own time limit
    python scripts/exp_savezip_gt.py STEP [N]                  one of: serial, overlapped, feeder, drain (for ``timeout -k 10 S ...``)"""
import subprocess, sys, tempfile, time
from pathlib import Path

STEPS = {"serial": 240, "overlapped": 240, "feeder": 120, "drain": 180}       # step -> its time limit in seconds
args = sys.argv[1:]
if not args or args[0] not in STEPS:
    for step, limit in STEPS.items():
        r = subprocess.run([sys.executable, __file__, step] + args[:1], timeout=limit + 30)
        if r.returncode != 0:                                                # nothing more is started on the device after a failure
            sys.exit(f"step {step!r} ended with status {r.returncode}")
    sys.exit(0)
STEP = args[0]
N = int(args[1]) if len(args) > 1 else 192

import torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from himo_amd import feather, save_zip_gt
from himo_amd.compdis import FrameBatch
from himo_amd.dataset import ListDataset
from himo_amd.feeder import BatchFeeder, ResultDrain
from himo_amd.synthetic import make_frame

POINTS = 120_000
base = [make_frame(i, n_points=POINTS) for i in range(48)]
frames = [dict(base[i % 48], timestamp=base[i % 48]["timestamp"] + 1000 * i) for i in range(N)]
ds = ListDataset(frames)
names, dtypes = feather.gt_schema()
head, tail, body_len, _ = feather.framing(names, dtypes, POINTS)
file_bytes = len(head) + body_len + len(tail)
dev = torch.device("cuda:0")

if STEP in ("serial", "overlapped"):
    print(f"{POINTS} points per sweep, {file_bytes} bytes per Feather file ({body_len / POINTS:.1f} bytes per point)", flush=True)
    for rep in range(3):
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            n = save_zip_gt.run_dataset(ds, "av2", Path(d), batch_frames=16, overlap=STEP == "overlapped")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print(f"overlap={STEP == 'overlapped'}: {n / dt:.1f} sweeps/s ({dt * 1e3 / n:.2f} ms per sweep), {n * file_bytes / dt / 1e9:.3f} GB/s of Feather", flush=True)

if STEP == "feeder":
    def build(fr, upload):
        return fr, FrameBatch.from_frames(fr, "flow", device=dev, with_masks=True, upload=upload, with_labels=True, host_ego=True)
    for rep in range(2):
        t0 = time.perf_counter()
        n = 0
        for fr, b in BatchFeeder((frames[lo:lo + 16] for lo in range(0, N, 16)), build, device=dev):
            n += len(fr)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"feeder alone (pack + pinned + copy to the device): {n / dt:.1f} sweeps/s", flush=True)

if STEP == "drain":
    body = torch.zeros(body_len, dtype=torch.uint8, device=dev)
    for threads in (1, 4, 8):
        with tempfile.TemporaryDirectory() as d:
            def sink(key, arr, d=d):
                with open(Path(d) / f"{key}.feather", "wb") as fh:
                    fh.write(head); fh.write(memoryview(arr)); fh.write(tail)
            drain = ResultDrain(sink, device=dev, threads=threads, copy=False)
            t0 = time.perf_counter()
            for i in range(N):
                drain.put(str(i), body)
            drain.close()
            dt = time.perf_counter() - t0
        print(f"drain alone, {threads} writer thread(s) (copy back + file): {N / dt:.1f} sweeps/s, {N * file_bytes / dt / 1e9:.3f} GB/s of Feather", flush=True)
