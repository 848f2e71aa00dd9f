"""GPU experiment: the fused head alone at the flagship step's shape -- 16 samples of 120k points in one launch (f16x2, folded weights,
gru_head_kernel<2, 9, false>), HIP events around every launch: mean and min-max per launch in us.

    python scripts/exp_head_diet.py [uniform|rings] [launches]

One process per library: HIMO_AMD_LIB selects a build of libhimo_amd.so (a variant compiled with -DHIMO_HEAD_PACKED_SLAB=0 /
-DHIMO_HEAD_GATE_FMA=0 / -DHIMO_HEAD_GATE_PK=0, or another commit's), so each switch's share shows (profiles/head_instruction_diet.txt).
"""
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np, torch
from himo_amd import _lib
from himo_amd.seflow import spec
from himo_amd.seflow.model import SeFlowNet
from himo_amd.synthetic import make_frame

cloud = sys.argv[1] if len(sys.argv) > 1 else "uniform"
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 30
B, N = 16, 120_000
dev = torch.device("cuda", 0)
net = SeFlowNet(spec.init_params(0), device=dev, max_points=N, precision="f16x2", max_batch=B)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
samples = []
for k in range(B):
    f = [make_frame(3 * k + i, n_points=N, cloud=cloud) for i in range(3)]
    samples.append((up(f[0]["pc0"]), up(f[1]["pc0"]), up(f[2]["pc0"]), f[0]["pose0"], f[1]["pose0"], f[1]["pose1"]))
outs = [torch.empty((N, 3), dtype=torch.float32, device=dev) for _ in range(B)]
net.forward_batch(samples, outs)                       # fills the images and the decoder map the head gathers from
torch.cuda.synchronize()
pc0s = [s[1] for s in samples]
for _ in range(5):
    net.head_batch(pc0s, outs)
torch.cuda.synchronize()
_lib.prof_start(only="gru_head")
for _ in range(launches):
    net.head_batch(pc0s, outs)
torch.cuda.synchronize()
p = _lib.prof_stop()["gru_head_kernel"]
assert int(net.nonfinite.item()) == 0 and bool(torch.isfinite(outs[0]).all())
print(f"{os.environ.get('HIMO_AMD_LIB', 'libhimo_amd.so'):40s} {cloud:8s} {p['count']} launches of {B} x {N}: "
      f"mean {p['avg_ms'] * 1e3:.1f} us (min {p['min_ms'] * 1e3:.1f} - max {p['max_ms'] * 1e3:.1f})  checksum {float(outs[0].double().abs().sum()):.6f}")
