"""The case table of the self-supervised loss stage (csrc/sslloss.hip, csrc/nngrid.hip), shared by tests/test_sslloss_oracle.py (CPU:
the reference and this table checked) and tests/test_sslloss_conformance_gpu.py (the kernels against the reference).

A case is ``(name, pc0, pc1, flow, label0, label1, n_labels)`` from a fixed seed; ``case(name)`` builds it, ``reference(name)`` is its
``sslloss_oracle.ssl_loss_f64`` (computed once per process, never modified).  Two families:

* lattice -- coordinates and flows are multiples of 1/8 within +-32 m: every difference, square and three-term sum is exact in float32
  with or without FMA, so a deliberate tie is an exact tie in the kernel too and the lowest-row / lowest-index rules need no guard.
* random  -- generic float32 values; the seeds are chosen so that the reference reports no ambiguous correspondence and no ambiguous
  anchor at a relative gap of AMBIGUOUS (tests/test_sslloss_oracle.py asserts it: a seed that fails is replaced, not excused).

Sizes sit at the boundaries the kernels are built around: the 256-thread blocks of the point kernels, the 64-lane scans of
dyn_write_kernel, the 64-query blocks of nng_query_kernel, and the second 1024-count chunk of dyn_scan_kernel (above 262 144 points).
"""
import functools

import numpy as np

import sslloss_oracle as so

U = 2.0 ** -24                       # float32 unit roundoff
AMBIGUOUS = 16 * U                   # relative gap below which float32 could order two distances differently
TERM_REL = 8 * U                     # per term: <= 3 float32 roundings per summand + the rounding of 1/n, no cancellation among summands
GRAD_REL = 16 * U                    # per gradient component, of the sum of |contributions|: ~5 roundings per contribution, <= 4 additions, doubled
SCAT_UNIT = 2.0 ** -40               # one unit of the fixed-point scatter, per scattered contribution
GRID = (-52.0, -52.0, 1.0, 104, 104)  # himo_amd.ssl_loss.GRID_*: the grid the loss is called with

F32 = np.float32
SMALL_SIZES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (255, 257), (256, 256), (257, 255), (513, 1000)]
CARRY_SIZES = [(262_444, 500), (500, 262_444)]
ALL_TERMS = frozenset(so.TERMS)

_TABLE = {}                          # name -> (family, builder, terms the case claims to exercise)


def _register(name, family, claims):
    def deco(fn):
        _TABLE[name] = (family, fn, frozenset(claims))
        return fn
    return deco


def _cloud(rng, n, family, extent, centre=(0.0, 0.0)):
    if family == "lattice":
        e = int(extent * 8)
        xy = rng.integers(-e, e + 1, (n, 2)) / 8.0 + np.asarray(centre)
        z = rng.integers(-16, 17, (n, 1)) / 8.0
    else:
        xy = rng.uniform(-extent, extent, (n, 2)) + np.asarray(centre)
        z = rng.uniform(-2.0, 2.0, (n, 1))
    return np.concatenate([xy, z], 1).astype(F32)


def _small(rng, n, family, scale=0.5):
    if family == "lattice":
        return (rng.integers(-8, 9, (n, 3)) / 8.0).astype(F32)
    return rng.normal(0.0, scale, (n, 3)).astype(F32)


def _scene(seed, family, n0, n1, extent=None):
    """two clouds of the same region; the first rows of pc1 sit near where the first rows of pc0 move to"""
    rng = np.random.default_rng(seed)
    extent = extent or min(30.0, max(2.0, 0.5 * np.sqrt(max(n0, n1))))
    pc0, pc1, flow = _cloud(rng, n0, family, extent), _cloud(rng, n1, family, extent), _small(rng, n0, family)
    k = min(n0, n1) // 2
    pc1[:k] = pc0[:k] + flow[:k] + _small(rng, k, family, 0.1) * (0.25 if family == "lattice" else 1.0)
    if family == "lattice":
        pc1 = np.round(pc1 * 8) / 8
    lab0 = rng.choice(np.array([-1, 0, 0, 1, 2, 3], np.int32), n0)
    lab1 = rng.choice(np.array([-1, 0, 1, 1, 5], np.int32), n1)
    return pc0, pc1.astype(F32), flow, lab0, lab1, rng


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
RESEEDED = {"size_256x256_random": 126}          # seed 106 gave an ambiguous correspondence: replaced, as the table's rule says
                                                 # (likewise the second carry case: 211 .. 213 were ambiguous or lacked a cluster)


def _size_case(family, n0, n1, seed):
    def build():
        pc0, pc1, flow, lab0, lab1, _ = _scene(seed, family, n0, n1)
        if n0 == 1:
            lab0[:] = 1
        if n1 == 1:
            lab1[:] = 1
        return pc0, pc1, flow, lab0, lab1, 4
    return build


for _k, (_n0, _n1) in enumerate(SMALL_SIZES):
    for _fam in ("lattice", "random"):
        # (1, 300): the single pc0 point is dynamic, so nothing is static; the other sizes exercise everything
        _claims = ALL_TERMS - {"static_flow_loss"} if _n0 == 1 else ALL_TERMS
        _name = f"size_{_n0}x{_n1}_{_fam}"
        _TABLE[_name] = (_fam, _size_case(_fam, _n0, _n1, RESEEDED.get(_name, 100 + _k)), _claims)


def _carry_case(n0, n1, seed):
    """dynamic points thinly over the large side and among its last 300 rows: their positions depend on the running total that
    dyn_scan_kernel carries into its second chunk of 1024 block counts"""
    def build():
        rng = np.random.default_rng(seed)
        pc0, pc1, flow = _cloud(rng, n0, "random", 50.0), _cloud(rng, n1, "random", 50.0), _small(rng, n0, "random")
        lab0 = np.where(rng.random(n0) < 0.1, rng.integers(1, 4, n0), 0).astype(np.int32)
        lab1 = np.where(rng.random(n1) < 0.1, 1, 0).astype(np.int32)
        big = lab0 if n0 > n1 else lab1
        big[-300::7] = 2                                    # 43 dynamic rows among the last 300
        big[-1] = 1
        return pc0, pc1, flow, lab0, lab1, 4
    return build


CARRY = []
for (_n0, _n1), _seed in zip(CARRY_SIZES, (201, 215)):
    _TABLE[f"carry_{_n0}x{_n1}_random"] = ("random", _carry_case(_n0, _n1, _seed), ALL_TERMS)
    CARRY.append(f"carry_{_n0}x{_n1}_random")


# ---- labels ---------------------------------------------------------------------------------------------------------------------
@_register("all_static", "random", {"chamfer_dis", "static_flow_loss"})
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(301, "random", 400, 380)
    return pc0, pc1, flow, np.zeros_like(lab0), np.zeros_like(lab1), 1


@_register("one_cluster", "random", ALL_TERMS - {"static_flow_loss"})
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(302, "random", 400, 380)
    return pc0, pc1, flow, np.ones_like(lab0), np.ones_like(lab1), 2


@_register("all_minus_one", "random", {"chamfer_dis"})
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(303, "random", 300, 333)
    return pc0, pc1, flow, np.full_like(lab0, -1), np.full_like(lab1, -1), 4


@_register("sparse_ids", "lattice", ALL_TERMS)
def _():
    pc0, pc1, flow, lab0, lab1, rng = _scene(304, "lattice", 500, 450)
    return pc0, pc1, flow, rng.choice(np.array([0, 1, 7, 1000], np.int32), 500), rng.choice(np.array([0, 1000], np.int32), 450), 1001


@_register("labels_above_n_labels", "random", ALL_TERMS)
def _():
    pc0, pc1, flow, lab0, lab1, rng = _scene(305, "random", 500, 450)
    return pc0, pc1, flow, rng.choice(np.array([0, 1, 2, 5, 9], np.int32), 500), rng.choice(np.array([0, 1, 9], np.int32), 450), 3


# ---- dynamic subsets ----------------------------------------------------------------------------------------------------------------
@_register("dynamic_rows_at_block_edges", "lattice", ALL_TERMS)
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(306, "lattice", 300, 320)
    lab0[:] = 0
    lab0[[0, 63, 64, 255, 256, 299]] = 1
    return pc0, pc1, flow, lab0, np.abs(lab1), 2


@_register("dynamic_in_pc0_only", "random", {"chamfer_dis", "static_flow_loss"})
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(307, "random", 350, 300)
    return pc0, pc1, flow, lab0, np.minimum(lab1, 0), 4


@_register("dynamic_in_pc1_only", "random", {"chamfer_dis", "static_flow_loss"})
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(308, "random", 350, 300)
    return pc0, pc1, flow, np.minimum(lab0, 0), lab1, 4


@_register("one_dynamic_point_each", "random", {"chamfer_dis", "static_flow_loss", "dynamic_chamfer_dis"})
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(309, "random", 300, 310)
    lab0, lab1 = np.minimum(lab0, 0), np.minimum(lab1, 0)
    lab0[77], lab1[201] = 2, 3
    return pc0, pc1, flow, lab0, lab1, 4


# ---- clusters and anchors ------------------------------------------------------------------------------------------------------------
@_register("cluster_without_dynamic_neighbour", "random", ALL_TERMS)
def _():
    """cluster 2 lives where every pc1 point is static (x < 0), cluster 1 where every pc1 point is dynamic: 2 is skipped, 1 anchored"""
    pc0, pc1, flow, lab0, lab1, _ = _scene(310, "random", 400, 420, extent=10.0)
    lab0 = np.where(pc0[:, 0] < -3, 2, np.where(pc0[:, 0] > 3, 1, 0)).astype(np.int32)
    return pc0, pc1, flow, lab0, (pc1[:, 0] > 0).astype(np.int32), 3


def _paired(seed, n, flow_is_target=False):
    """lattice: pc0 on distinct nodes of a 3 m mesh, pc1 row i = pc0 row i + an offset of at most 1 m, so the raw neighbour of row i is
    row i.  Cluster 1: rows 10 and 200 both sit 1 m from their neighbours (in different directions), every other member closer: an
    anchor tie that row 10 must win.  Cluster 2: every member coincides with its neighbour: an anchor at raw distance exactly 0."""
    rng = np.random.default_rng(seed)
    nodes = rng.permutation(21 * 21)[:n]
    pc0 = np.stack([(nodes % 21 - 10) * 3.0, (nodes // 21 - 10) * 3.0, rng.integers(-8, 9, n) / 8.0], 1).astype(F32)
    lab0 = rng.choice(np.array([0, 1, 1, 2], np.int32), n)
    lab0[[10, 200]] = 1
    near = np.array([[0.5, 0.5, 0], [-0.5, 0.5, 0], [0.5, 0, 0], [0, -0.5, 0.25], [0.25, 0, 0]], F32)
    off = near[rng.integers(0, len(near), n)]
    off[10], off[200] = (1.0, 0, 0), (0, 1.0, 0)
    off[lab0 == 2] = 0
    flow = _small(rng, n, "lattice")
    if flow_is_target:
        flow[lab0 == 1] = off[10]
    return pc0, (pc0 + off).astype(F32), flow, lab0, np.ones(n, np.int32), 3


@_register("anchor_tie_and_anchor_at_zero", "lattice", ALL_TERMS)
def _():
    return _paired(311, 320)


@_register("flow_equals_cluster_target", "lattice", ALL_TERMS)
def _():
    """cluster 1's residual is exactly zero at every member: zero sub-gradient, finite; cluster 2 keeps the term positive"""
    return _paired(312, 320, flow_is_target=True)


# ---- duplicates and fan-in -----------------------------------------------------------------------------------------------------------
@_register("every_pc1_point_twice", "random", ALL_TERMS)
def _():
    """the second copy of every pc1 point is static, the first keeps its label: which copy a raw search returns decides the anchors"""
    pc0, pc1, flow, lab0, lab1, _ = _scene(313, "random", 300, 280)
    return pc0, np.concatenate([pc1, pc1]), flow, lab0, np.concatenate([np.abs(lab1), np.zeros_like(lab1)]), 4


@_register("identical_pc0_pairs", "random", ALL_TERMS)
def _():
    """rows i and i + 150 of pc0 are the same point with the same flow and label: every pc1 -> moved gradient lands on row i"""
    pc0, pc1, flow, lab0, lab1, _ = _scene(314, "random", 150, 330)
    return np.concatenate([pc0, pc0]), pc1, np.concatenate([flow, flow]), np.concatenate([lab0, lab0]), lab1, 4


@_register("fan_in", "random", ALL_TERMS)
def _():
    """pc0 row 5 inside a blob of 1000 dynamic pc1 points, every other pc0 point 40 m away: 2000 scattered contributions on one row"""
    rng = np.random.default_rng(315)
    pc0 = _cloud(rng, 300, "random", 6.0, centre=(-40.0, 0.0))
    pc0[5] = (20.0, 10.0, 0.25)
    pc1 = (np.array([20.0, 10.0, 0.0]) + rng.normal(0, 0.7, (1000, 3))).astype(F32)
    flow = _small(rng, 300, "random")
    lab0 = rng.choice(np.array([0, 1, 2], np.int32), 300)
    lab0[5] = 1
    return pc0, pc1, flow, lab0, np.ones(1000, np.int32), 3


# ---- grid edge and zeros ---------------------------------------------------------------------------------------------------------------
@_register("across_the_grid_edge", "random", ALL_TERMS)
def _():
    """points out to +-70 m on a +-52 m grid; a third of the flows are 20 m long and carry `moved` over the border cells"""
    pc0, pc1, flow, lab0, lab1, rng = _scene(316, "random", 500, 480, extent=70.0)
    far = rng.random(500) < 0.33
    flow[far, 0] += 20.0 * np.sign(pc0[far, 0]) * np.where(np.abs(pc0[far, 0]) < 52, 1.0, -1.0)     # out of the grid, or back into it
    flow[far & (lab0 > 0), 1] -= 20.0 * np.sign(pc0[far & (lab0 > 0), 1])
    return pc0, pc1, flow, lab0, lab1, 4


@_register("zero_flow", "random", ALL_TERMS - {"static_flow_loss"})
def _():
    pc0, pc1, flow, lab0, lab1, _ = _scene(317, "random", 420, 400)
    return pc0, pc1, np.zeros_like(flow), lab0, lab1, 4


NAMES = list(_TABLE)
SMALL = [n for n in NAMES if n not in CARRY]
TWICE = ["fan_in", "size_513x1000_lattice", "size_513x1000_random"]      # cases run twice for bit-reproducibility


def family(name):
    return _TABLE[name][0]


def claims(name):
    return _TABLE[name][2]


@functools.lru_cache(maxsize=None)
def case(name):
    pc0, pc1, flow, lab0, lab1, n_labels = _TABLE[name][1]()
    arrs = [np.ascontiguousarray(pc0, F32), np.ascontiguousarray(pc1, F32), np.ascontiguousarray(flow, F32),
            np.ascontiguousarray(lab0, np.int32), np.ascontiguousarray(lab1, np.int32)]
    for a in arrs:
        a.setflags(write=False)
    return (name, *arrs, int(n_labels))


@functools.lru_cache(maxsize=None)
def reference(name):
    return so.ssl_loss_f64(*case(name)[1:])


def compare(ref, loss5, grad):
    """The conformance check of one result against ``ref``: -> dict with ``term`` (worst |got - ref| / (TERM_REL * ref) over the
    terms the reference has > 0), ``zeros`` (every term the reference has at 0 is exactly 0), ``total`` (loss5[4] is the sum of the
    four terms as the kernel adds them), ``grad`` (worst |got - ref| / (GRAD_REL * abs_sum + n_scat * SCAT_UNIT) over EVERY point and
    component; an error where the bound is 0 counts as inf), ``finite``."""
    loss5, grad = np.asarray(loss5, np.float64), np.asarray(grad, np.float64)
    want = np.array([ref.terms[k] for k in so.TERMS])
    pos = want > 0
    term = float((np.abs(loss5[:4] - want)[pos] / (TERM_REL * want[pos])).max()) if pos.any() else 0.0
    err = np.abs(grad - ref.grad)
    bound = GRAD_REL * ref.abs_sum + (ref.n_scat * SCAT_UNIT)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return {"term": term, "zeros": bool((loss5[:4][~pos] == 0).all()),
            "total": bool(loss5[4] == ((loss5[0] + loss5[1]) + loss5[2]) + loss5[3]),
            "grad": float(ratio.max()) if ratio.size else 0.0,
            "finite": bool(np.isfinite(loss5).all() and np.isfinite(grad).all())}


def passes(c):
    return c["finite"] and c["zeros"] and c["total"] and c["term"] <= 1.0 and c["grad"] <= 1.0
