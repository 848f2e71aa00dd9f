"""The two CPU references of DBSCAN against each other: oracle/dbscan_oracle.dbscan (cKDTree + sklearn) and the brute-force
restatement oracle/dbscan_exact.dbscan_exact share no code and must give the same labels on random blobs and on every hand-built
input of the GPU conformance suite (tests/test_dbscan_conformance_gpu.py); and the generators of that suite's hazardous inputs
must find what they are for."""
import warnings

import numpy as np
import pytest

import dbscan_exact as de
import dbscan_oracle as do

HAZARD_EPS = (0.5, 0.4, 0.3, 1.0)
# pairs that pass the distance test two cells apart, found by an earlier sweep of the float neighbours of every cell boundary of the
# production grid (x0 = -52, cell = eps): the exhaustive generator must find at least as many
HAZARD_FLOOR = {0.5: 4, 0.25: 4, 1.0: 4, 0.4: 192, 0.3: 220, 0.35: 152, 0.6: 88, 0.7: 84, 0.8: 78}
CONTRACTION = ((0.5, "in_out"), (0.4, "out_in"))
CONTRACTION_FLOOR = 32


def _both(pts, eps, min_pts, skip=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # sklearn: "precomputed sparse input was not sorted by row values"
        a = do.dbscan(pts, eps, min_pts, skip)
    b = de.dbscan_exact(pts, eps, min_pts, skip)
    assert np.array_equal(a, b), (np.flatnonzero(a != b)[:10], a[a != b][:10], b[a != b][:10])
    return b


@pytest.mark.parametrize("seed,n,eps,min_pts", [(1, 2000, 0.5, 8), (2, 3001, 0.3, 4), (3, 777, 1.0, 12), (4, 4097, 0.4, 2), (5, 500, 0.5, 1)])
def test_references_agree_on_blobs(seed, n, eps, min_pts):
    pts = de.blobs(seed, n)
    skip = (np.random.default_rng(seed).uniform(size=n) < 0.1).astype(np.uint8) * (seed % 2 + 1)
    pts[::97, seed % 3] = np.nan
    pts[5::131, (seed + 1) % 3] = np.inf
    got = _both(pts, eps, min_pts, skip)
    assert got.max() > 0 and (got[skip != 0] == 0).all() and (got[~np.isfinite(pts).all(1)] == 0).all()


def test_references_agree_on_hand_built_inputs():
    for name, pts, eps, min_pts, skip, want in de.hand_built():
        got = _both(pts, eps, min_pts, skip)
        if want is not None:
            assert np.array_equal(got, want), (name, got, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_references_agree_on_isolated_pairs(n):
    pts = de.isolated_pairs(n, n)
    got = _both(pts, 0.5, 2)
    n_single = n % 2 + 2 * min(3, n // 16)
    assert got.max() == (n - n_single) // 2 and (got == 0).sum() == n_single


def test_cell_hazard_pairs():
    """every pair passes the float32 distance test, sits two cells apart under floor((x - x0) * (1 / cell)), and both references
    make one cluster of it; the clouds the GPU suite builds from them (pairs at min_pts 2, triples around one core point at 3)"""
    counts = {}
    for eps, floor in HAZARD_FLOOR.items():
        pr = de.cell_hazard_pairs(eps)
        counts[eps] = len(pr)
        assert len(pr) >= floor, (eps, len(pr))
        d = pr[:, 1] - pr[:, 0]
        assert np.all(d * d <= np.float32(eps) * np.float32(eps))
        assert np.all(de.naive_cell(pr[:, 1], -52.0, eps) - de.naive_cell(pr[:, 0], -52.0, eps) == 2)
        assert np.all(de.naive_cell(pr[:, 0], -52.0, eps) >= 0) and np.all(de.naive_cell(pr[:, 1], -52.0, eps) < np.ceil(104 / eps))
        two = np.zeros((2, 3), np.float32)
        two[:, 0] = pr[len(pr) // 2]
        assert np.array_equal(_both(two, eps, 2), [1, 1])
    print("\ncell-hazard pairs per eps (x0 = -52, cell = eps): " + ", ".join(f"{e}: {c}" for e, c in counts.items()))
    assert tuple(pr.tolist() for pr in de.cell_hazard_pairs(0.5)[:1]) == ([-20.000001907348633, -19.500001907348633],)
    for eps in HAZARD_EPS:
        found = len(de.cell_hazard_pairs(eps))                  # every generated pair is placed: along x and along y
        pairs = de.hazard_cloud(eps, min_pts=2)
        got = _both(pairs, eps, 2)
        assert len(pairs) == 4 * found and got.min() == 1 and got.max() == 2 * found and np.all(np.bincount(got)[1:] == 2)
        triples = de.hazard_cloud(eps, min_pts=3)
        got = _both(triples, eps, 3)
        assert len(triples) == 6 * found and got.min() == 1 and got.max() == 2 * found and np.all(np.bincount(got)[1:] == 3)


def test_contraction_pairs():
    """at least 32 pairs per direction at seed 0; each is decided one way by the unfused float32 sum and the other way by every
    contracted form (checked again here in float64, where the float32 products are exact), and the references follow the unfused sum"""
    counts = {}
    for eps, direction in CONTRACTION:
        p, q = de.contraction_pairs(eps, direction)
        counts[(eps, direction)] = len(p)
        assert len(p) >= CONTRACTION_FLOOR, (eps, direction, len(p))
        d = q - p
        e2 = np.float32(eps) * np.float32(eps)
        unfused = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= e2
        assert np.all(unfused == (direction == "in_out"))
        r = lambda v: v.astype(np.float32).astype(np.float64)
        for v in de._sums(*(d.astype(np.float64).T ** 2), r)[1:]:
            assert np.all((v <= float(e2)) != unfused)
        cloud = np.concatenate([p, q])
        got = _both(cloud, eps, 2)
        want = np.tile(np.arange(1, len(p) + 1), 2) if direction == "in_out" else np.zeros(2 * len(p))
        assert np.array_equal(got, want)
    print("\ncontraction-sensitive pairs: " + ", ".join(f"eps {e} {d}: {c}" for (e, d), c in counts.items()))


def test_brute_force_at_the_largest_case():
    """the GPU suite's largest brute-force case (n = 8193): about a second on an idle machine; the time is printed, and only a bound
    generous enough for a loaded machine (a minute) is asserted"""
    import time
    pts = de.isolated_pairs(8193, 8193)
    t0 = time.perf_counter()
    got = de.dbscan_exact(pts, 0.5, 2)
    took = time.perf_counter() - t0
    print(f"\ndbscan_exact, n = 8193: {took:.2f} s")
    assert got.max() == 4093 and took < 60.0
