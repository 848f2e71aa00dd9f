"""GPU tests of stage "NSFP, v1" (himo_amd/nsfp.py, csrc/nsfp.hip; PARITY UNPINNED, own specification): the objective step against the
layer-kernel path's search + Chamfer kernels and a float64 brute force, one iteration against autograd and against
FastNSF(objective="nn"), a short trajectory, the stop rule on the device, reproducibility, overlap, and the program."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TRUNC = 2.0


def _scene(seed, n0, n1):
    rng = np.random.default_rng(seed)
    pc1 = rng.uniform([-40, -40, -2], [40, 40, 2], (n1, 3)).astype(np.float32)
    k = min(n0, n1)
    pc0 = np.empty((n0, 3), np.float32)
    pc0[:k] = pc1[:k] - np.array([0.6, 0.2, 0.0], np.float32) + rng.normal(0, 0.02, (k, 3)).astype(np.float32)
    if n0 > k:
        pc0[k:] = rng.uniform([-40, -40, -2], [40, 40, 2], (n0 - k, 3)).astype(np.float32)
    return pc0, pc1


# ---- 1. the objective step alone ---------------------------------------------------------------------------------------------------
def _grid():
    from himo_amd.ssl_loss import GRID_CELL, GRID_H, GRID_W, GRID_X0, GRID_Y0
    return GRID_X0, GRID_Y0, GRID_CELL, GRID_W, GRID_H


def _objective(gpu, moved, pc1, calls=1):
    """himo_nsfp_prepare + ``calls`` x himo_nsfp_objective with x0 = moved, out = 0 (moved = x0 + 0 exactly)"""
    from himo_amd import _lib
    lib = _lib.load()
    n0, n1 = len(moved), len(pc1)
    n_pad, parts = int(lib.himo_nsf_padded_rows(n0)), int(lib.himo_nsfp_partials(n0, n1))
    x0 = torch.zeros((max(n_pad, 1), 4), dtype=torch.float32, device=gpu)
    x0[:n0, :3] = torch.from_numpy(moved).to(gpu)
    out = torch.zeros_like(x0)
    dout = torch.full_like(x0, 7.0)                             # every row must be written: padding rows as zeros
    p1 = torch.from_numpy(np.ascontiguousarray(pc1)).to(gpu)
    ws = torch.empty(int(lib.himo_nsfp_workspace_bytes(n0, n1, *_grid()[3:])), dtype=torch.uint8, device=gpu)
    mv = torch.full((max(n0, 1), 3), 9.0, dtype=torch.float32, device=gpu)
    d_a, i_a = torch.full((max(n0, 1),), -1.0, device=gpu), torch.full((max(n0, 1),), -7, dtype=torch.int32, device=gpu)
    d_b, i_b = torch.full((max(n1, 1),), -1.0, device=gpu), torch.full((max(n1, 1),), -7, dtype=torch.int32, device=gpu)
    lp = torch.full((max(parts, 1),), 5.0, dtype=torch.float64, device=gpu)
    cp = torch.full((max(parts, 1),), 5, dtype=torch.int32, device=gpu)
    s = _lib.stream_handle()
    p1_ptr = p1.data_ptr() if n1 else None
    _lib.check(lib.himo_nsfp_prepare(n0, n1, p1_ptr, *_grid(), ws.data_ptr(), ws.numel(), s), "prepare")
    runs = []
    for _ in range(calls):
        _lib.check(lib.himo_nsfp_objective(n0, n1, x0.data_ptr(), out.data_ptr(), p1_ptr, *_grid(), TRUNC, mv.data_ptr(), d_a.data_ptr(),
                                           i_a.data_ptr(), d_b.data_ptr(), i_b.data_ptr(), dout.data_ptr(), lp.data_ptr(), cp.data_ptr(),
                                           ws.data_ptr(), ws.numel(), s), "objective")
        torch.cuda.synchronize()
        runs.append(dict(n_pad=n_pad, parts=parts, moved=mv.cpu().numpy(), d_a=d_a.cpu().numpy()[:n0], i_a=i_a.cpu().numpy()[:n0],
                         d_b=d_b.cpu().numpy()[:n1], i_b=i_b.cpu().numpy()[:n1], dout=dout.cpu().numpy(), lp=lp.cpu().numpy(), cp=cp.cpu().numpy()))
    return runs


def _layer_kernel_path(gpu, moved, pc1):
    """the two himo_nn_grid searches + himo_chamfer_trunc of FastNSF(objective="nn") on the same points"""
    from himo_amd import _lib
    from himo_amd.ssl_loss import nn_grid
    import himo_amd.fastnsf  # noqa: F401  (signatures)
    lib = _lib.load()
    n0, n1 = len(moved), len(pc1)
    m, p = torch.from_numpy(moved).to(gpu), torch.from_numpy(np.ascontiguousarray(pc1)).to(gpu)
    d_a, i_a = nn_grid(m, p)
    d_b, i_b = nn_grid(p, m)
    loss = torch.zeros(1, dtype=torch.float64, device=gpu)
    g = torch.empty((n0, 3), dtype=torch.float32, device=gpu)
    ws = torch.empty(int(lib.himo_chamfer_trunc_workspace_bytes(n0, n1)), dtype=torch.uint8, device=gpu)
    _lib.check(lib.himo_chamfer_trunc(n0, n1, m.data_ptr(), p.data_ptr(), d_a.data_ptr(), i_a.data_ptr(), d_b.data_ptr(), i_b.data_ptr(), TRUNC,
                                      loss.data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle()), "chamfer")
    return d_a.cpu().numpy(), i_a.cpu().numpy(), d_b.cpu().numpy(), i_b.cpu().numpy(), float(loss.item()), g.cpu().numpy()


def _brute_force(moved, pc1):
    """float64: (loss, d L / d moved, a, ia, b, ib, pairwise squared distances); ties keep the lowest row (argmin's rule)"""
    m, p = moved.astype(np.float64), pc1.astype(np.float64)
    d = ((m[:, None, :] - p[None, :, :]) ** 2).sum(2)
    ia, ib = d.argmin(1), d.argmin(0)
    a, b = d[np.arange(len(m)), ia], d[ib, np.arange(len(p))]
    ka, kb = a <= TRUNC * TRUNC, b <= TRUNC * TRUNC
    loss = a[ka].sum() / len(m) + b[kb].sum() / len(p)
    g = np.zeros_like(m)
    g[ka] += 2.0 / len(m) * (m[ka] - p[ia[ka]])
    np.add.at(g, ib[kb], 2.0 / len(p) * (m[ib[kb]] - p[kb]))
    return loss, g, a, ia, b, ib, d


def _case(name):
    rng = np.random.default_rng({"lattice": 1, "random": 2, "border": 3, "fanin": 4}[name])
    if name == "lattice":
        # moved rows on half-integer x between two pc1 lattice points (exact ties in float32), and every pc1 row twice
        gx, gy = np.meshgrid(np.arange(-6, 6), np.arange(-5, 5), indexing="ij")
        lat = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1).astype(np.float32)                    # 120 points
        pc1 = np.concatenate([lat, lat, lat[:17]])                                                           # 257 rows, all duplicated
        moved = np.concatenate([lat + np.float32([0.5, 0, 0]), lat + np.float32([0, 0.5, 0.25]), lat[:60] + np.float32([0.5, 0.5, 0])])
        return moved.astype(np.float32), pc1[rng.permutation(len(pc1))].astype(np.float32)                   # (300, 257)
    if name == "random":
        return (rng.uniform([-10, -10, -2], [10, 10, 2], (300, 3)).astype(np.float32),
                rng.uniform([-10, -10, -2], [10, 10, 2], (257, 3)).astype(np.float32))
    if name == "border":
        # beyond the grid's +-52 m (border cells) and sparse: most pairs are farther apart than tau, some are close
        pc1 = rng.uniform([-75, -75, -2], [75, 75, 2], (1400, 3)).astype(np.float32)
        moved = rng.uniform([-75, -75, -2], [75, 75, 2], (1500, 3)).astype(np.float32)
        moved[:500] = pc1[:500] + rng.normal(0, 0.3, (500, 3)).astype(np.float32)
        return moved, pc1
    if name == "fanin":
        # 2000 pc1 rows whose nearest moved row is ONE row (row 123, at the origin); every other moved row is far away
        moved = rng.uniform([20, -30, -2], [45, 30, 2], (300, 3)).astype(np.float32)
        moved[123] = 0.0
        pc1 = np.concatenate([rng.uniform(-1.0, 1.0, (2000, 3)), rng.uniform([20, -30, -2], [45, 30, 2], (57, 3))]).astype(np.float32)
        return moved, pc1
    raise KeyError(name)


@pytest.mark.parametrize("name", ["lattice", "random", "border", "fanin"])
def test_objective_step_equals_the_layer_kernel_path_and_brute_force(gpu, name):
    moved, pc1 = _case(name)
    n0, n1 = len(moved), len(pc1)
    first, second = _objective(gpu, moved, pc1, calls=2)
    r = first
    assert np.array_equal(r["moved"], moved)
    d_a, i_a, d_b, i_b, ref_loss, ref_g = _layer_kernel_path(gpu, moved, pc1)
    # the searches: the same exact rule on the same grid -> the same bits
    assert np.array_equal(r["i_a"], i_a) and np.array_equal(r["i_b"], i_b)
    assert np.array_equal(r["d_a"].view(np.uint32), d_a.view(np.uint32)) and np.array_equal(r["d_b"].view(np.uint32), d_b.view(np.uint32))
    # what himo_nsf_update makes of the lists: loss = sum / sum of counts, gradient = d_dout / sum of counts
    assert r["cp"][:r["parts"]].sum() == n0
    loss = r["lp"][:r["parts"]].sum() / n0
    g = r["dout"][:n0, :3].astype(np.float64) / np.float32(n0)
    print(f"{name}: loss {loss!r} vs layer kernels {ref_loss!r}; max |g - ref| / max |ref| = {np.abs(g - ref_g).max() / np.abs(ref_g).max():.3g}")
    assert loss == pytest.approx(ref_loss, rel=1e-9)
    assert np.abs(g - ref_g).max() <= 1e-6 * np.abs(ref_g).max()
    assert np.all(r["dout"][n0:] == 0) and np.all(r["dout"][:, 3] == 0) and r["n_pad"] > n0
    # a second step on the same workspace (the fixed-point sums are left clear): the same bits
    for k in ("d_a", "i_a", "d_b", "i_b", "dout", "lp", "cp"):
        assert np.array_equal(first[k], second[k]), k
    # float64 brute force
    bl, bg, a, ia, b, ib, d = _brute_force(moved, pc1)
    if name == "lattice":                                       # exact arithmetic: ties resolved to the lowest row, like argmin
        assert np.array_equal(r["i_a"], ia) and np.array_equal(r["i_b"], ib)
        assert np.array_equal(r["d_a"].astype(np.float64), a) and np.array_equal(r["d_b"].astype(np.float64), b)
        assert (np.sort(d, 1)[:, 0] == np.sort(d, 1)[:, 1]).all()         # every moved row had a tie to break
    else:                                                       # float32 distances: the chosen row is a nearest one to rounding
        assert np.all(d[np.arange(n0), r["i_a"]] <= a * (1 + 1e-6) + 1e-9) and np.all(d[r["i_b"], np.arange(n1)] <= b * (1 + 1e-6) + 1e-9)
        assert np.allclose(r["d_a"], a, rtol=1e-6, atol=1e-9) and np.allclose(r["d_b"], b, rtol=1e-6, atol=1e-9)
    # float32 differences and squares of coordinates below 2^7: each term to a few 2^-24 relative
    assert loss == pytest.approx(bl, rel=1e-6)
    assert np.abs(g - bg).max() <= 1e-6 * np.abs(bg).max()
    if name == "border":
        assert (a > TRUNC * TRUNC).sum() > 100 and (a <= TRUNC * TRUNC).sum() > 100 and np.abs(moved[:, :2]).max() > 60
    if name == "fanin":
        assert (r["i_b"][:2000] == 123).all()


def test_objective_step_with_an_empty_target_or_an_empty_source(gpu):
    from himo_amd import _lib
    lib = _lib.load()
    moved, _ = _case("random")
    r = _objective(gpu, moved, np.zeros((0, 3), np.float32))[0]
    assert r["parts"] == r["n_pad"] // 64
    assert r["lp"][:r["parts"]].sum() == 0.0 and r["cp"][:r["parts"]].sum() == len(moved)
    assert np.all(r["dout"] == 0) and np.all(np.isinf(r["d_a"])) and np.all(r["i_a"] == -1)
    # n0 == 0: nothing is launched, nothing is written
    r = _objective(gpu, np.zeros((0, 3), np.float32), _case("random")[1])[0]
    assert np.all(r["dout"] == 7.0) and np.all(r["lp"] == 5.0)
    # a misaligned buffer is refused
    x = torch.zeros(4 * 256 + 4, dtype=torch.float32, device=gpu)
    ws = torch.empty(int(lib.himo_nsfp_workspace_bytes(10, 0, 104, 104)), dtype=torch.uint8, device=gpu)
    ok = x.data_ptr()
    args = lambda x0: (10, 0, x0, ok, None, *_grid(), TRUNC, ok, ok, ok, None, None, ok, ok, ok, ws.data_ptr(), ws.numel(), _lib.stream_handle())
    assert lib.himo_nsfp_objective(*args(ok + 4)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.himo_nsfp_keep_best(10, ok + 4, ok, ok, ok, 1, 3, 0.0, _lib.stream_handle()) == _lib.ERR_INVALID_ARGUMENT


# ---- 2. one iteration, lr = 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(6000, 5500), (300, 257)])
def test_one_iteration_matches_autograd_and_the_layer_kernels(gpu, n0, n1):
    import fastnsf_oracle as fo
    from himo_amd.fastnsf import FastNSF, init_mlp
    from himo_amd.nsfp import NSFP
    pc0, pc1 = _scene(1, n0, n1)
    layers = init_mlp(3)
    eng = NSFP(device=gpu, iters=1, lr=0.0, seed=3)
    eng.fit(pc0, pc1, layers=layers)
    assert [t for t, _ in eng.loss_history] == [1] and (eng.best_iter, eng.stopped_at) == (1, 0)
    loss = eng.loss_history[0][1]
    ref_loss, ref_grads, _ = fo.loss_and_grads(layers, pc0, pc1)
    old = FastNSF(device=gpu, iters=1, lr=0.0, seed=3, objective="nn")
    old.fit(pc0, pc1, layers=layers)
    print(f"loss {loss!r}: autograd {ref_loss!r}, layer kernels {old.loss_history[0][1]!r}")
    assert loss == pytest.approx(ref_loss, rel=1e-4)
    assert loss == pytest.approx(old.loss_history[0][1], rel=1e-6)
    for k, (gw, gb) in enumerate(ref_grads):
        cin, cout = gw.shape
        got_w, got_b = eng.gW[k].cpu().numpy()[:cin, :cout], eng.gb[k].cpu().numpy()[:cout]
        old_w, old_b = old.gW[k].cpu().numpy()[:cin, :cout], old.gb[k].cpu().numpy()[:cout]
        print(f"layer {k}: dW {np.abs(got_w - gw).max() / max(np.abs(gw).max(), 1e-8):.3g} db {np.abs(got_b - gb).max() / max(np.abs(gb).max(), 1e-8):.3g} (autograd); "
              f"dW {np.abs(got_w - old_w).max() / max(np.abs(old_w).max(), 1e-12):.3g} db {np.abs(got_b - old_b).max() / max(np.abs(old_b).max(), 1e-12):.3g} (layer kernels)")
        assert np.abs(got_w - gw).max() <= 1e-3 * max(np.abs(gw).max(), 1e-8), k
        assert np.abs(got_b - gb).max() <= 1e-3 * max(np.abs(gb).max(), 1e-8), k
        assert np.abs(got_w - old_w).max() <= 2e-4 * max(np.abs(old_w).max(), 1e-12), k      # (k = 8: the last layer's own path)
        assert np.abs(got_b - old_b).max() <= 2e-4 * max(np.abs(old_b).max(), 1e-12), k


# ---- 3. trajectory -----------------------------------------------------------------------------------------------------------------
def test_fit_follows_the_cpu_restatement(gpu):
    import fastnsf_oracle as fo
    from himo_amd.fastnsf import init_mlp
    from himo_amd.nsfp import NSFP
    pc0, pc1 = _scene(2, 8000, 8000)
    layers = init_mlp(5)
    iters = 25
    eng = NSFP(device=gpu, iters=iters, lr=1e-3, keep_best=False, patience=0)
    eng.fit(pc0, pc1, layers=layers)
    hist, _ = fo.fit(layers, pc0, pc1, iters)
    got = [v for _, v in eng.loss_history]
    assert len(got) == iters
    print("losses", got[:10], "restatement", hist[:10], "last", got[-1], hist[-1])
    for a, b in zip(got[:10], hist[:10]):
        assert a == pytest.approx(b, rel=2e-3)
    assert got[-1] < 0.5 * got[0]


# ---- 4. the stop rule on the device ------------------------------------------------------------------------------------------------
def test_stop_rule_on_the_device(gpu):
    from himo_amd.nsfp import NSFP, stop_rule
    pc0, pc1 = _scene(3, 3000, 2900)
    # (a) nothing after the first loss can improve by 1e9: best_iter 1, three stale iterations later the rule stops
    flows = []
    for check_every in (1, 7, 25):
        eng = NSFP(device=gpu, iters=60, min_delta=1e9, patience=3, check_every=check_every)
        flows.append(eng.fit(pc0, pc1).clone())
        losses = [v for _, v in eng.loss_history]
        assert [t for t, _ in eng.loss_history] == list(range(1, len(losses) + 1))
        assert (eng.best_iter, eng.stopped_at) == (1, 4) and eng.stopped_at < 60
        assert (eng.best_iter, eng.stopped_at) == stop_rule(losses, 3, 1e9)
        if check_every == 1:
            assert len(losses) < 60                             # the host stopped queueing
    assert torch.equal(flows[0], flows[1]) and torch.equal(flows[0], flows[2])
    first = NSFP(device=gpu, iters=0, keep_best=False).fit(pc0, pc1)          # best_iter - 1 = 0 updates: the initial field
    assert torch.equal(flows[0], first)
    # (b) patience = iters: never stops (iteration 1 always improves), the best iterate is kept
    flows = []
    for check_every in (1, 7, 25):
        eng = NSFP(device=gpu, iters=40, min_delta=0.0, patience=40, check_every=check_every)
        flows.append(eng.fit(pc0, pc1).clone())
        losses = [v for _, v in eng.loss_history]
        assert len(losses) == 40 and eng.stopped_at == 0 and eng.best_iter >= 1
        assert (eng.best_iter, eng.stopped_at) == stop_rule(losses, 40, 0.0)
        assert losses[eng.best_iter - 1] == min(losses)
    assert torch.equal(flows[0], flows[1]) and torch.equal(flows[0], flows[2])
    last = NSFP(device=gpu, iters=eng.best_iter - 1, min_delta=0.0, patience=40, keep_best=False).fit(pc0, pc1)
    assert torch.equal(flows[0], last)


# ---- 5. reproducibility and overlap --------------------------------------------------------------------------------------------------
def test_fit_is_bit_reproducible(gpu):
    from himo_amd.nsfp import NSFP
    pc0, pc1 = _scene(4, 5000, 5300)
    runs = []
    for _ in range(2):
        eng = NSFP(device=gpu, iters=20)
        flow = eng.fit(pc0, pc1)
        assert flow.shape == (5000, 3) and torch.isfinite(flow).all()
        runs.append((flow.clone(), list(eng.loss_history), eng.best_iter))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]
    assert runs[0][1][-1][1] < runs[0][1][0][1]


def test_two_fits_in_flight_return_the_single_engine_bits(gpu):
    from himo_amd.fastnsf import OverlappedFastNSF
    from himo_amd.nsfp import NSFP
    from himo_amd.synthetic import make_frame
    pairs = []
    for i in range(5):
        f = make_frame(830 + i, n_points=8_000 - 577 * i)
        p0 = torch.from_numpy(f["pc0"][:, :3].copy()).to(gpu)
        p1 = torch.from_numpy((f["pc0"][:, :3] + f["flow"]).astype(np.float32)).to(gpu)
        pairs.append((p0, p1, f["pose0"], f["pose1"]))
    one = NSFP(device=gpu, iters=12, seed=3, check_every=5)
    ref = []
    for p in pairs:
        flow = one.fit(*p)
        ref.append((flow.clone(), list(one.loss_history), one.best_iter))
    two = OverlappedFastNSF(device=gpu, engines=2, engine=NSFP, iters=12, seed=3, check_every=5)
    got = []
    for k, flow in enumerate(two.fits(iter(pairs))):
        eng = two.engines[k % 2]
        got.append((flow.clone(), list(eng.loss_history), eng.best_iter))
    assert len(got) == len(ref)
    for (fa, la, ba), (fb, lb, bb) in zip(ref, got):
        assert torch.equal(fa, fb) and la == lb and ba == bb and len(la) == 12


# ---- 6. the program ------------------------------------------------------------------------------------------------------------------
def test_save_program_writes_nsfp_and_still_writes_fastnsf(gpu, tmp_path):
    from himo_amd import save
    from himo_amd.dataset import NpzDataset
    from himo_amd.fastnsf import FastNSF
    from himo_amd.nsfp import NSFP
    from himo_amd.synthetic import make_frame
    frames = [make_frame(860 + i, n_points=6_000 - 500 * i, scene_id="s0" if i < 3 else "s1") for i in range(5)]
    NpzDataset.write(tmp_path, frames)
    assert save.main(dataset_path=str(tmp_path), model="fastnsf", objective="nn", iters=8) == 3      # the last sweep of each scene has no successor
    assert save.main(dataset_path=str(tmp_path), model="fastnsf", objective="dt", iters=8) == 3
    for key, one in (("nsfp", NSFP(device=gpu, iters=8)), ("fastnsf", FastNSF(device=gpu, iters=8))):
        ds = NpzDataset(tmp_path, vis_name=key)
        seen = 0
        for i in range(len(ds)):
            f = ds[i]
            if key not in f:
                continue
            seen += 1
            assert f[key].shape == (len(f["pc0"]), 3) and f[key].dtype == np.float32
            want = one.fit(f["pc0"][:, :3], ds[i + 1]["pc0"][:, :3], f["pose0"], f["pose1"]).cpu().numpy()
            assert np.array_equal(f[key], want), key
        assert seen == 3, key
    with pytest.raises(ValueError):
        save.main(dataset_path=str(tmp_path), model="fastnsf", objective="chamfer")
