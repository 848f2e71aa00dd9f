"""``SeFlowNet.sparse_dec4``: dec4 formed only at the cells that hold a point of pc0 (the row mask the pillar stage writes) gives the
flows of the dense network bit for bit, and DEC agrees bitwise wherever the occupancy bit is set -- through ``forward_batch`` and
through ``HiMoPipeline.run`` on consecutive, different batches (so cells left over from the earlier batch are in DEC)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (5000, 64, 1)


def make_batch(gpu, seed):
    """three samples of 5000 / 64 / 1 points per sweep; some points out of range; the 64-point sample sits in ONE cell"""
    from himo_amd.pipeline import Sample
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(COUNTS):
        sweeps = []
        for _ in range(3):
            p = np.empty((n, 3), dtype=np.float32)
            p[:, :2] = rng.uniform(-50.0, 50.0, size=(n, 2))
            p[:, 2] = rng.uniform(-2.5, 2.5, size=n)
            if n == 64:
                p[:, :2] = np.float32(3.02 + seed) + rng.uniform(0.0, 0.05, size=(n, 2))       # one 0.2 m cell
            if n >= 5000:
                p[::17, 0] = 80.0                        # beyond the grid: pid = -1
                p[5::29, 2] = 9.0
            sweeps.append(torch.from_numpy(p).to(gpu))
        pose = lambda dx: np.array([[1, 0, 0, dx], [0, 1, 0, 0.02 * dx], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
        dt = torch.from_numpy(rng.uniform(0.0, 0.1, size=n).astype(np.float32)).to(gpu)
        out.append(Sample(sweeps[0], sweeps[1], sweeps[2], pose(0.0), pose(0.3 + 0.1 * k), pose(0.6 + 0.1 * k), dt))
    return out


def as_tuples(samples):
    return [(s.pch1, s.pc0, s.pc1, s.pose_h1, s.pose0, s.pose1) for s in samples]


@pytest.fixture(scope="module")
def params():
    from himo_amd.seflow import spec
    return spec.init_params(0)


@pytest.fixture(scope="module")
def net(gpu, params):
    from himo_amd.seflow.model import SeFlowNet
    return SeFlowNet(params, device=gpu, max_points=6000, precision="f16x2", autotune=False, max_batch=3)


def occupancy_bits(net, k):
    """host copy of sample k's occupancy words as a bool array over the cells"""
    words = net.occ0[k].cpu().numpy().view(np.uint8)
    return np.unpackbits(words, bitorder="little").astype(bool)[:net.H * net.W]


def test_forward_batch_off_then_on(net, gpu):
    samples = make_batch(gpu, 1)
    flows = lambda: [torch.full((n, 3), float("nan"), device=gpu) for n in COUNTS]
    assert net.sparse_dec4 is False
    off = flows()
    net.forward_batch(as_tuples(samples), off)
    torch.cuda.synchronize()
    dec_off = net.DEC.clone()
    net.DEC.view(torch.int32).fill_(0x7FC0BEEF)                       # what the masked launch must leave alone
    net.sparse_dec4 = True
    on = flows()
    net.forward_batch(as_tuples(samples), on)
    torch.cuda.synchronize()
    try:
        for k, n in enumerate(COUNTS):
            assert torch.equal(on[k], off[k]), k
            assert bool(torch.isfinite(on[k]).all())
            pid = net._pt[k]["pid"][net.HEAD_SLOT][:n].cpu().numpy()
            want = np.zeros(net.H * net.W, dtype=bool)
            want[pid[pid >= 0]] = True
            got = occupancy_bits(net, k)
            assert np.array_equal(got, want), (k, int(got.sum()), int(want.sum()))
            occ = torch.from_numpy(got).to(gpu)
            a, b = net.DEC[k].view(torch.int32), dec_off[k].view(torch.int32)
            assert torch.equal(a[occ], b[occ]), k
            assert bool((a[~occ] == 0x7FC0BEEF).all()), k              # nothing else was written
        assert int(occupancy_bits(net, 1).sum()) == 1 and int(occupancy_bits(net, 2).sum()) <= 1
        assert (net._pt[0]["pid"][net.HEAD_SLOT][:COUNTS[0]] < 0).any()
    finally:
        net.sparse_dec4 = False


def test_pipeline_two_batches_in_a_row(net, gpu):
    from himo_amd.pipeline import HiMoPipeline
    b1, b2 = make_batch(gpu, 2), make_batch(gpu, 3)
    pipe = HiMoPipeline(net, device=gpu)
    assert net.sparse_dec4 is True                                    # f16x2, split activations, fused head
    try:
        net.sparse_dec4 = False
        want = []
        for b in (b1, b2):
            r = pipe.run(b, copy=True)
            want.append((r["flow"], r["comp_dis"]))
        net.sparse_dec4 = True
        for b, (flow, cd) in zip((b1, b2), want):                     # DEC still holds the other batch's cells each time
            r = pipe.run(b, copy=True)
            torch.cuda.synchronize()
            assert torch.equal(r["flow"], flow) and torch.equal(r["comp_dis"], cd)
        pipe.sync_check()
        net.split_acts = False                                        # float32 activations: the masked kernel does not apply
        assert net.sparse_dec4 is False
    finally:
        net.split_acts = True
        net.sparse_dec4 = False


def test_auto_fallback_runs_dense(gpu, params):
    from himo_amd.pipeline import HiMoPipeline
    from himo_amd.seflow.model import SeFlowNet
    batch = make_batch(gpu, 4)
    pipe = HiMoPipeline(None, device=gpu, max_points=6000, max_batch=3, precision="auto", params=params)
    assert pipe.net.precision == "f16x2" and pipe.net.sparse_dec4 is True
    pipe._fall_back()
    assert pipe.net.precision == "bf16x3" and pipe.net.sparse_dec4 is False
    pipe.net.autotune = False                                         # (every tile variant gives the same bits; tuning only takes time)
    got = pipe.run(batch, copy=True)["flow"]
    ref = SeFlowNet(params, device=gpu, max_points=6000, precision="bf16x3", autotune=False, max_batch=3)
    outs = [torch.empty((n, 3), device=gpu) for n in COUNTS]
    ref.forward_batch(as_tuples(batch), outs)
    torch.cuda.synchronize()
    assert torch.equal(got, torch.cat(outs))
