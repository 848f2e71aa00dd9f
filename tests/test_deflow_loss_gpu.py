"""himo_deflow_loss (csrc/deflowloss.hip, "DeFlow loss, v1") against the float64 statement of its rule (tests/deflowloss_ref.py).

Bounds, none taken from the kernel's output:
  counts    equal exactly -- the same double operations in the same order give the same bands, so the band test needs no margin
  terms     relative n * 2^-53 + 2^-52 -- reordering a sum of n non-negative doubles against the exactly rounded sum, plus one division
  gradient  1 float32 ulp of the reference's float32 value on every element (bit equality is expected where the device's double sqrt
            and division are correctly rounded; every case prints how many elements differ at all)
Row counts: 0, 1, one row short of a block, a block, a block and a row, and 65 537 = 257 blocks, one more block than the 256 threads
of the single-block fold, so that one of its lanes adds two partials."""
import functools

import numpy as np
import pytest
import torch

from deflowloss_ref import TERMS, deflow_loss_ref, make_case

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 257, 65_537)
VARIANTS = {
    "all": dict(n_exact=3, n_bad_gt=3),
    "no_pid": dict(with_pid=False, n_bad_gt=2),
    "no_valid": dict(with_valid=False, n_exact=2),
    "bare": dict(with_pid=False, with_valid=False),
    "band0": dict(bands=(0,)),
    "band1": dict(bands=(1,)),
    "band2": dict(bands=(2,)),
    "dropped": dict(all_dropped=True),
    "nan_est": dict(nan_est_row=200, n_bad_gt=2),
}
PITCHES = ((3, 3), (3, 4), (4, 3), (4, 4))                    # (pc0, est) row pitch in floats


@functools.lru_cache(maxsize=None)
def _case(n, variant):
    """the seeded case and its reference, made once and shared (callers do not write into them)"""
    case = make_case(n, seed=11 + sorted(VARIANTS).index(variant), **VARIANTS[variant])
    ref = deflow_loss_ref(case["pc0"], case["moved"], case["est"], case["gt"], case["pid"], case["valid"], case["sensor_dt"])
    return case, ref


@pytest.fixture(scope="module")
def engine(gpu):
    from himo_amd.deflow_loss import DeFlowLoss
    return DeFlowLoss(device=gpu)


def _ordered(x):
    """float32 -> int64 keys whose differences count representable values between two floats (+0 and -0 share key 0)"""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _padded(a, cols, fill):
    out = np.full((a.shape[0], cols), fill, np.float32)
    out[:, :3] = a[:, :3]
    return out


def _run(engine, gpu, case, pitches=(3, 3)):
    up = lambda a: None if a is None else torch.from_numpy(a).to(gpu)
    terms, total, grad = engine(up(_padded(case["pc0"], pitches[0], 0.5)), up(case["moved"]), up(_padded(case["est"], pitches[1], -7.0)),
                                up(case["gt"]), pid=up(case["pid"]), valid=up(case["valid"]), sensor_dt=case["sensor_dt"])
    return torch.stack([terms[k] for k in TERMS]).clone(), total.clone(), grad, engine.counts.clone()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("n", SIZES)
def test_loss_counts_and_gradient_match_the_float64_rule(gpu, engine, n, variant):
    case, ref = _case(n, variant)
    if variant in ("all", "no_pid", "no_valid", "bare", "nan_est") and n >= 255:
        assert (ref["counts"] > 0).all()                                       # all three bands occupied
    if variant == "all" and n >= 255:
        assert ((ref["e"] == 0) & ref["counted"]).any() and not np.isfinite(case["gt"]).all() and not ref["counted"].all()
    nan_row = VARIANTS[variant]["nan_est_row"] % n if (variant == "nan_est" and n) else None
    bound = n * 2.0 ** -53 + 2.0 ** -52
    first = None
    for pitches in PITCHES:
        terms, total, grad, counts = (t.cpu().numpy() for t in _run(engine, gpu, case, pitches))
        assert counts.dtype == np.int64 and np.array_equal(counts, ref["counts"]), (pitches, counts, ref["counts"])
        for k in range(3):
            if np.isnan(ref["terms"][k]):
                assert np.isnan(terms[k])
            else:
                assert abs(terms[k] - ref["terms"][k]) <= bound * abs(ref["terms"][k]), (pitches, k, terms[k], ref["terms"][k])
            if ref["counts"][k] == 0:
                assert terms[k] == 0.0                                          # an empty band contributes exactly 0
        if np.isnan(ref["total"]):
            assert nan_row is not None and np.isnan(total)
        else:
            assert abs(total - ref["total"]) <= bound * abs(ref["total"]), (pitches, total, ref["total"])
        assert grad.shape == (n, 3) and grad.dtype == np.float32
        finite = np.isfinite(ref["grad"]).all(axis=1)
        if nan_row is None:
            assert finite.all()
        else:                                                                   # only that row's gradient is non-finite
            assert ref["counted"][nan_row] and not finite[nan_row] and finite.sum() == n - 1
            assert not np.isfinite(grad[nan_row]).any()
        assert np.isfinite(grad[finite]).all()
        diff = np.abs(_ordered(grad[finite]) - _ordered(ref["grad"][finite]))
        if first is None:
            print(f"deflow loss n={n} {variant}: {int((diff != 0).sum())} of {diff.size} gradient elements differ from the float64 rule "
                  f"(largest {int(diff.max(initial=0))} ulp)")
        assert diff.max(initial=0) <= 1, (pitches, int(diff.max()), int((diff > 1).sum()))
        assert (grad[~ref["counted"]] == 0).all()                               # uncounted rows: exactly 0
        assert (grad[ref["counted"] & (ref["e"] == 0)] == 0).all()              # est == g: exactly 0, no NaN
        if first is None:
            first = (terms, total, grad)
        else:                                                                   # the row pitch changes no bit
            assert np.array_equal(first[0].view(np.int64), terms.view(np.int64)) and np.array_equal(first[2].view(np.int32), grad.view(np.int32))


@pytest.mark.parametrize("n", (257, 65_537))
def test_two_calls_give_the_same_bits(gpu, engine, n):
    for variant in ("all", "nan_est"):
        case, _ = _case(n, variant)
        a, b = _run(engine, gpu, case, (4, 4)), _run(engine, gpu, case, (4, 4))
        assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[3], b[3])


def test_views_of_wider_rows_go_in_without_a_copy_and_a_fresh_engine_agrees(gpu, engine):
    """the trainer's call: the head's [n][4] rows and a [:, :3] view of them, pc0 rows with an intensity column"""
    from himo_amd.deflow_loss import DeFlowLoss
    case, ref = _case(257, "all")
    up = lambda a: torch.from_numpy(a).to(gpu)
    est4, pc04 = up(_padded(case["est"], 4, 3.0)), up(_padded(case["pc0"], 5, 9.0))
    args = (up(case["moved"]), )
    kw = dict(pid=up(case["pid"]), valid=up(case["valid"]).bool())
    t0, tot0, g0 = engine(pc04, *args, est4, up(case["gt"]), **kw)
    t1, tot1, g1 = DeFlowLoss(device=gpu)(pc04[:, :3], *args, est4[:, :3], up(case["gt"]), **kw)
    assert torch.equal(tot0, tot1) and torch.equal(g0, g1) and all(torch.equal(t0[k], t1[k]) for k in TERMS)
    assert tot0.dtype == torch.float64 and tot0.dim() == 0 and set(t0) == set(TERMS)
    assert abs(float(tot0) - ref["total"]) <= (257 * 2.0 ** -53 + 2.0 ** -52) * ref["total"]


def test_refusals_and_the_empty_call(gpu):
    """argument checks happen before anything is launched: a short workspace is the library's workspace status, a pitch below 3 and a
    non-positive sensor_dt are invalid arguments; n == 0 writes zeros over whatever the outputs held"""
    from himo_amd import _lib
    import himo_amd.deflow_loss  # noqa: F401  (registers the entry points)
    lib = _lib.load()
    n = 300
    need = int(lib.himo_deflow_loss_workspace_bytes(n))
    assert need >= n and int(lib.himo_deflow_loss_workspace_bytes(0)) > 0
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=gpu)
    p, m, gt, est, grad = f(n, 3), f(n, 3), f(n, 3), f(n, 3), f(n, 3)
    loss = torch.full((4,), 5.0, dtype=torch.float64, device=gpu)
    counts = torch.full((3,), 9, dtype=torch.int64, device=gpu)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    s = _lib.stream_handle()
    call = lambda n_, pitch, dt, ws_bytes: lib.himo_deflow_loss(n_, p.data_ptr(), pitch, m.data_ptr(), gt.data_ptr(), est.data_ptr(), 3, None, None,
                                                                  dt, loss.data_ptr(), counts.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws_bytes, s)
    assert call(n, 3, 0.1, need - 1) == _lib.ERR_WORKSPACE
    assert call(n, 2, 0.1, need) == _lib.ERR_INVALID_ARGUMENT
    assert call(n, 3, 0.0, need) == _lib.ERR_INVALID_ARGUMENT
    assert call(-1, 3, 0.1, need) == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (loss == 5.0).all() and (counts == 9).all()                          # refused calls touch nothing
    assert call(0, 3, 0.1, 0) == _lib.OK
    torch.cuda.synchronize()
    assert (loss == 0).all() and (counts == 0).all()
    assert call(n, 3, 0.1, need) == _lib.OK                                     # all-zero rows: band 0, est == g everywhere
    torch.cuda.synchronize()
    assert counts.tolist() == [n, 0, 0] and (loss == 0).all() and (grad == 0).all()
