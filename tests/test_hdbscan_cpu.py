"""HDBSCAN, v1 without a GPU: the library's host phase (``himo_hdbscan_tree``: dendrogram, condensed tree, stabilities, selection,
labels -- plain C++, driven through ctypes) against tests/hdbscan_ref.py, and the reference itself against sklearn."""
import ctypes

import numpy as np
import pytest

import hdbscan_ref as ref

SEEDS = list(range(24))
PARAMS = [(10, 10), (15, 5), (8, 4), (20, 1)]


def blobs(seed):
    """the issue's generator: 2-6 Gaussian blobs of 12-79 points and up to 39 uniform points, flattened in z, shuffled"""
    rng = np.random.default_rng(seed); nb = rng.integers(2, 7)
    pts = [rng.normal(rng.uniform(-20, 20, 3) * [1, 1, .1], rng.uniform(.2, .8), (rng.integers(12, 80), 3)) for _ in range(nb)]
    pts.append(rng.uniform(-25, 25, (rng.integers(0, 40), 3)) * [1, 1, .1])
    x = np.concatenate(pts).astype(np.float32); x = x[rng.permutation(len(x))]
    m, k = PARAMS[seed % 4]
    return x, m, k


def lattice():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def duplicates():
    rng = np.random.default_rng(5)
    return np.concatenate([np.tile(np.float32([[3.0, -2.0, 0.5]]), (50, 1)), rng.normal([-4.0, 4.0, 0.0], 0.3, (30, 3)).astype(np.float32)])


@pytest.fixture(scope="module")
def lib():
    from himo_amd import _lib
    import himo_amd.seflow.ssl_label  # noqa: F401  (registers the entry points)
    return _lib.load()


def tree(lib, n, index, edges, m, k):
    """himo_hdbscan_tree on host arrays -> (status, labels, count)"""
    index = np.ascontiguousarray(index, dtype=np.int32)
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 3).astype(np.uint32))
    labels = np.full(n, -7, dtype=np.int32)
    count = ctypes.c_int32(-7)
    st = lib.himo_hdbscan_tree(n, len(index), index.ctypes.data, len(edges), edges.ctypes.data, m, k, labels.ctypes.data, ctypes.addressof(count))
    return st, labels, count.value


def check_against_ref(lib, x, m, k, skip=None):
    r = ref.hdbscan(x, m, k, skip)
    rng = np.random.default_rng(len(x))
    edges = r["edges"][rng.permutation(len(r["edges"]))]               # the device emits them in no particular order
    st, labels, count = tree(lib, len(x), r["index"], edges, m, k)
    assert st == 0
    assert np.array_equal(labels, r["labels"]) and count == r["count"]
    return r


@pytest.mark.parametrize("seed", SEEDS)
def test_tree_phase_equals_the_reference_on_blobs(lib, seed):
    x, m, k = blobs(seed)
    r = check_against_ref(lib, x, m, k)
    assert r["count"] >= 1


def test_tree_phase_on_a_lattice_where_every_weight_ties(lib):
    r = check_against_ref(lib, lattice(), 10, 4)
    assert len(np.unique(r["edges"][:, 0])) == 1


def test_tree_phase_on_duplicates(lib):
    r = check_against_ref(lib, duplicates(), 10, 5)
    assert r["count"] == 2 and (r["edges"][:, 0] == 0).sum() == 49


def test_tree_phase_small_and_empty_inputs(lib):
    two = np.float32([[0, 0, 0], [1, 0, 0]])
    assert check_against_ref(lib, two, 2, 1)["count"] == 0
    x = blobs(3)[0]
    few = np.ones(len(x), dtype=bool); few[:7] = False
    assert check_against_ref(lib, x, 5, 8, skip=few)["count"] == 0             # |P| = 7 < k = 8
    assert check_against_ref(lib, x, 5, 8, skip=np.ones(len(x), dtype=bool))["count"] == 0
    assert check_against_ref(lib, x, len(x) + 1, 4)["count"] == 0              # m larger than |P|
    nan = x.copy(); nan[::3, 1] = np.nan
    r = check_against_ref(lib, nan, 8, 4)
    assert (r["labels"][::3] == 0).all() and r["count"] >= 1


def test_tree_phase_refuses_what_is_not_a_spanning_tree(lib):
    from himo_amd import _lib
    x, m, k = blobs(1)
    r = ref.hdbscan(x, m, k)
    n, idx, e = len(x), r["index"], r["edges"]
    assert tree(lib, n, idx, e, m, k)[0] == 0
    bad = _lib.ERR_INVALID_ARGUMENT
    assert tree(lib, n, idx, e[:-1], m, k)[0] == bad                            # too short
    cyc = e.copy(); cyc[-1] = cyc[0]
    assert tree(lib, n, idx, cyc, m, k)[0] == bad                               # an edge twice: a cycle
    a, b, c = idx[:3]
    tri = e.copy(); tri[:3, 1:] = [[a, b], [b, c], [a, c]]
    assert tree(lib, n, idx, tri, m, k)[0] == bad                               # a triangle
    out = e.copy(); out[0, 2] = n
    assert tree(lib, n, idx, out, m, k)[0] == bad                               # out of range
    swapped = e.copy(); swapped[0, 1:] = swapped[0, :0:-1]
    assert tree(lib, n, idx, swapped, m, k)[0] == bad                           # lo >= hi
    skip = np.zeros(n, dtype=bool); skip[5] = True
    r2 = ref.hdbscan(x, m, k, skip)
    stranger = r2["edges"].copy(); v = int(stranger[0, 1]); stranger[0, 1:] = [min(5, v), max(5, v)]
    assert tree(lib, n, r2["index"], stranger, m, k)[0] == bad                  # an end that takes no part
    nanw = e.copy(); nanw[0, 0] = 0x7fc00000
    assert tree(lib, n, idx, nanw, m, k)[0] == bad                              # a weight that is no non-negative float
    assert tree(lib, n, idx[::-1], e, m, k)[0] == bad                           # indices not ascending
    assert tree(lib, n, idx, e, 1, k)[0] == bad and tree(lib, n, idx, e, m, 33)[0] == bad
    assert tree(lib, n, idx[:3], e[:2], m, 8)[0] == bad                         # |P| < k wants no edges


def ari(a, b):
    """adjusted Rand index of two labelings (noise = one more class)"""
    from math import comb
    _, ai = np.unique(a, return_inverse=True)
    _, bi = np.unique(b, return_inverse=True)
    t = np.zeros((ai.max() + 1, bi.max() + 1), dtype=np.int64)
    np.add.at(t, (ai, bi), 1)
    s = sum(comb(int(v), 2) for v in t.ravel())
    sa, sb = sum(comb(int(v), 2) for v in t.sum(1)), sum(comb(int(v), 2) for v in t.sum(0))
    exp = sa * sb / comb(len(a), 2)
    return (s - exp) / (0.5 * (sa + sb) - exp)


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist())) and ((a == 0) == (b == 0)).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_against_sklearn(seed):
    """tests/hdbscan_ref.py against sklearn.cluster.HDBSCAN(algorithm="brute") on the same points as float64.  k = 1 (no weight ties):
    an identical partition and noise set.  k > 1: an equal cluster count and ARI >= 0.98 -- sklearn orders tied merges by its Prim walk,
    this rule by (w, lo, hi).

    ARI measured per seed (sklearn 1.7.2), cluster counts equal on all 24: 1.0000 (identical partition and noise set) on seeds 0, 3-7,
    9-21 and 23, every k = 1 seed among them; seed 1 (m 15, k 5) 0.9869, seed 2 (m 8, k 4) 0.9952, seed 8 (m 10, k 10) 0.9861,
    seed 22 (m 8, k 4) 0.9964."""
    sk = pytest.importorskip("sklearn.cluster")
    x, m, k = blobs(seed)
    want = sk.HDBSCAN(min_cluster_size=m, min_samples=k, algorithm="brute", allow_single_cluster=False).fit(x.astype(np.float64)).labels_ + 1
    got = ref.hdbscan(x, m, k)["labels"]
    score = ari(got, want)
    print(f"seed {seed} (m {m}, k {k}): clusters {got.max()} / {want.max()}, ARI {score:.4f}")
    assert got.max() == want.max()
    if k == 1:
        assert same_partition(got, want)
    else:
        assert score >= 0.98
