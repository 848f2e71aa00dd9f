"""Conformance of the self-supervised loss stage (csrc/sslloss.hip, searching through csrc/nngrid.hip) through its exported entry
points, called directly: himo_ssl_loss, himo_ssl_loss_ex, himo_ssl_loss_presized, himo_ssl_dyn_sizes, himo_nn_grid and the two
workspace queries.

Every case of tests/sslloss_cases.py is compared with the float64 reference oracle/sslloss_oracle.py: ssl_loss_f64 (checked on the CPU
by tests/test_sslloss_oracle.py) at EVERY point: each term within 8 * 2^-24 relative (a term the reference has at 0 exactly 0), the
total the sum of the four, and each gradient component within 16 * 2^-24 * A + c * 2^-40, A the reference's sum of |contributions| to
that component and c its number of scattered contributions.  The lattice cases make every tie exact, so "ties: lowest row" and
"anchor ties: lowest index" are tested without a guard band; the random cases have no correspondence or anchor closer than
16 * 2^-24 relative to its runner-up.  Every operand, output and workspace lives in a NaN-filled guarded buffer (oracle/guarded.py),
the workspace has exactly the size the library's query returns, after every call the inputs are bit-unchanged and nothing outside an
output or the workspace is written.  The three entry points return identical bits on every small case; refusals (read in
sslloss.hip: they return before any launch) leave gradient, loss and workspace unwritten.

Worst error / bound measured on the MI355X (printed by the module's summary):
    lattice  terms 0.109  gradient 0.139  (13 cases)
    random   terms 0.102  gradient 0.527  (24 cases; the gradient figure is one_cluster's, every other case is at 0.21 or below)
"""
import numpy as np
import pytest
import torch

import sslloss_cases as sc
import sslloss_oracle as so
from guarded import Guarded

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = 1, 3
STATS = {}        # family -> [worst term ratio, worst gradient ratio, cases]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nsslloss conformance: per family, the largest error / bound over the table")
    for fam, (t, g, n) in sorted(STATS.items()):
        print(f"  {fam:8s} terms {t:.3g}  gradient {g:.3g}  {n} cases")


@pytest.fixture(scope="module")
def lib(gpu):
    from himo_amd import _lib, ssl_loss                      # noqa: F401  (registers the signatures)
    return _lib.load()


def _s():
    from himo_amd import _lib
    return _lib.stream_handle()


def gwords(gpu, values=None, n=None):
    """a guarded operand of 32-bit words: float32 / int32 values, or ``n`` NaN-filled words"""
    g = Guarded(torch.arange(values.size if values is not None else n, dtype=torch.int64), gpu)
    if values is not None:
        g.put(torch.from_numpy(np.array(values).reshape(-1)))
    return g


class Run:
    """one case in guarded buffers"""

    def __init__(self, lib, gpu, name, grid=sc.GRID):
        _, pc0, pc1, flow, lab0, lab1, self.n_labels = sc.case(name)
        self.lib, self.gpu, self.grid, self.n0, self.n1 = lib, gpu, grid, len(pc0), len(pc1)
        self.host = [pc0, pc1, flow, lab0, lab1]
        self.inputs = [gwords(gpu, a) for a in self.host]                      # the labels go through the int32 path of put()
        self.grad, self.loss = gwords(gpu, n=3 * self.n0), gwords(gpu, n=10)
        self.ws_bytes = int(lib.himo_ssl_loss_workspace_bytes(self.n0, self.n1, self.n_labels, grid[3], grid[4]))
        assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
        self.ws = gwords(gpu, n=self.ws_bytes // 4)
        self.extra = []

    def head(self, n_labels=None, grid=None):
        return (self.n0, self.n1, *(g.ptr for g in self.inputs), self.n_labels if n_labels is None else n_labels, *(grid or self.grid))

    def tail(self, ws_ptr=None, ws_bytes=None):
        return (self.loss.ptr, self.grad.ptr, self.ws.ptr if ws_ptr is None else ws_ptr, self.ws_bytes if ws_bytes is None else ws_bytes, _s())

    def fresh(self, workspace=True):
        self.grad.reset(), self.loss.reset()
        if workspace:
            self.ws.reset()

    def result(self, status):
        """after a call that must have succeeded: guards intact, inputs unchanged, no NaN -> (loss [5] float64, grad [n0, 3] float32)"""
        torch.cuda.synchronize()
        assert status == 0
        for g in (*self.inputs, self.grad, self.loss, self.ws, *self.extra):
            assert g.untouched_outside()
        for g, a in zip(self.inputs, self.host):
            assert np.array_equal(g.words().numpy(), a.reshape(-1).view(np.int32))
        loss = self.loss.words().numpy().view(np.float64).copy()
        grad = self.grad.get().numpy().reshape(self.n0, 3).copy()
        assert np.isfinite(loss).all() and np.isfinite(grad).all()
        return loss, grad

    def plain(self):
        return self.result(self.lib.himo_ssl_loss(*self.head(), *self.tail()))

    def raw_pair(self):
        """himo_nn_grid(pc0 -> pc1) on the same grid, into guarded buffers of their own"""
        lib, g = self.lib, self.grid
        d2, idx = gwords(self.gpu, n=self.n0), gwords(self.gpu, n=self.n0)
        nb = int(lib.himo_nn_grid_workspace_bytes(max(self.n0, self.n1), g[3], g[4]))
        ws = gwords(self.gpu, n=nb // 4)
        st = lib.himo_nn_grid(self.n0, self.inputs[0].ptr, self.n1, self.inputs[1].ptr, *g, d2.ptr, idx.ptr, ws.ptr, nb, _s())
        torch.cuda.synchronize()
        assert st == 0
        self.extra += [d2, idx, ws]
        return d2, idx

    def sizes(self):
        counts = gwords(self.gpu, n=2)
        st = self.lib.himo_ssl_dyn_sizes(self.n0, self.inputs[3].ptr, self.n1, self.inputs[4].ptr, counts.ptr, _s())
        torch.cuda.synchronize()
        assert st == 0 and counts.untouched_outside()
        self.extra.append(counts)
        return [int(v) for v in counts.words()]


def _check(name, loss, grad):
    ref = sc.reference(name)
    c = sc.compare(ref, loss, grad)
    print(f"\n  {name}: terms err/bound {c['term']:.3g}, gradient err/bound {c['grad']:.3g}, zeros {c['zeros']}, total {c['total']}")
    s = STATS.setdefault(sc.family(name), [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], c["term"]), max(s[1], c["grad"]), s[2] + 1
    assert c["zeros"], "a term the reference has at 0 is not exactly 0"
    assert c["total"], "the total is not the sum of the four terms"
    assert c["term"] <= 1.0, dict(zip(so.TERMS, zip(loss, ref.terms.values())))
    if c["grad"] > 1.0:
        err = np.abs(grad - ref.grad)
        bound = sc.GRAD_REL * ref.abs_sum + (ref.n_scat * sc.SCAT_UNIT)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        i, k = np.unravel_index(r.argmax(), r.shape)
        pytest.fail(f"{name}: gradient row {i} component {k}: got {grad[i, k]!r}, reference {ref.grad[i, k]!r}, "
                    f"|contributions| {ref.abs_sum[i, k]!r}, scattered {ref.n_scat[i]}; {int((r > 1).sum())} components over the bound")


@pytest.mark.parametrize("name", sc.SMALL)
def test_small_case_through_the_three_entry_points(lib, gpu, name):
    """every point of the case against the float64 reference, and himo_ssl_loss == himo_ssl_loss_ex with himo_nn_grid's raw pair ==
    himo_ssl_loss_presized with himo_ssl_dyn_sizes' counts, bit for bit; the cases of sc.TWICE once more on the used workspace"""
    run = Run(lib, gpu, name)
    loss, grad = run.plain()
    _check(name, loss, grad)
    d2, idx = run.raw_pair()
    run.fresh()
    loss_ex, grad_ex = run.result(lib.himo_ssl_loss_ex(*run.head(), d2.ptr, idx.ptr, *run.tail()))
    nd = run.sizes()
    assert tuple(nd) == sc.reference(name).n_dyn
    run.fresh()
    loss_ps, grad_ps = run.result(lib.himo_ssl_loss_presized(*run.head(), d2.ptr, idx.ptr, nd[0], nd[1], *run.tail()))
    run.fresh()
    loss_p0, grad_p0 = run.result(lib.himo_ssl_loss_presized(*run.head(), None, None, nd[0], nd[1], *run.tail()))
    for other_loss, other_grad in ((loss_ex, grad_ex), (loss_ps, grad_ps), (loss_p0, grad_p0)):
        assert np.array_equal(other_loss.view(np.int64), loss.view(np.int64))
        assert np.array_equal(other_grad.view(np.int32), grad.view(np.int32))
    if name in sc.TWICE:
        run.fresh(workspace=False)                           # the second call meets the first one's workspace
        loss2, grad2 = run.plain()
        assert np.array_equal(loss2.view(np.int64), loss.view(np.int64)) and np.array_equal(grad2.view(np.int32), grad.view(np.int32))


@pytest.mark.parametrize("name", sc.CARRY)
def test_carry_case(lib, gpu, name):
    """more than 1024 block counts on one side: dyn_scan_kernel's second chunk, the running total carried into it (one call each)"""
    run = Run(lib, gpu, name)
    loss, grad = run.plain()
    _check(name, loss, grad)


NN_SIZES = (1, 63, 64, 65, 513)


def _nn_variant(variant, nq, nr, rng):
    """lattice clouds (multiples of 1/8): distances are exact in float32, ties are exact ties"""
    grid = sc.GRID
    if variant == "one_cell":                                # 64 distinct BEV positions: duplicates and ties everywhere
        mk = lambda n: np.concatenate([rng.integers(0, 8, (n, 2)) / 8.0 + 3.0, rng.integers(-64, 65, (n, 1)) / 8.0], 1)
    else:
        mk = lambda n: np.concatenate([rng.integers(-256, 257, (n, 2)) / 8.0, rng.integers(-16, 17, (n, 1)) / 8.0], 1)
    q, r = mk(nq).astype(np.float32), mk(nr).astype(np.float32)
    if variant == "outside_the_grid":                        # every point beyond the grid's corner: all binned into border cells
        grid = (40.0, 40.0, 1.0, 8, 8)
    elif variant == "grid_1x1":
        grid = (-52.0, -52.0, 104.0, 1, 1)
    elif variant == "references_twice":
        r = np.concatenate([r, r])
    return q, r, grid


@pytest.mark.parametrize("variant", ["one_cell", "outside_the_grid", "grid_1x1", "references_twice"])
def test_nn_grid_alone_is_the_lowest_row_search(lib, gpu, variant):
    """rows equal to the float64 exhaustive search with the lowest row winning ties, distances bit-equal"""
    rng = np.random.default_rng(len(variant))
    for nq in NN_SIZES:
        for nr in NN_SIZES:
            q, r, grid = _nn_variant(variant, nq, nr, rng)
            want_d, want_i, _ = so.search_f64(q, r)
            gq, gr, d2, idx = gwords(gpu, q), gwords(gpu, r), gwords(gpu, n=nq), gwords(gpu, n=nq)
            nb = int(lib.himo_nn_grid_workspace_bytes(max(len(q), len(r)), grid[3], grid[4]))
            ws = gwords(gpu, n=nb // 4)
            st = lib.himo_nn_grid(len(q), gq.ptr, len(r), gr.ptr, *grid, d2.ptr, idx.ptr, ws.ptr, nb, _s())
            torch.cuda.synchronize()
            assert st == 0, (nq, nr)
            assert all(g.untouched_outside() for g in (gq, gr, d2, idx, ws)), (nq, nr)
            assert np.array_equal(gq.get().numpy(), q.reshape(-1)) and np.array_equal(gr.get().numpy(), r.reshape(-1))
            assert np.array_equal(idx.words().numpy(), want_i.astype(np.int32)), (nq, nr)
            assert (want_d.astype(np.float32) == want_d).all()
            assert np.array_equal(d2.words().numpy(), want_d.astype(np.float32).view(np.int32)), (nq, nr)
            if variant == "references_twice":
                assert (want_i < nr).all()


def test_refusals_write_nothing(lib, gpu):
    """each refused call returns its status before any launch: gradient, loss and workspace keep every word"""
    run = Run(lib, gpu, "size_63x65_lattice")
    d2, idx = run.raw_pair()
    words = run.ws_bytes // 4
    shifted = gwords(gpu, n=words + 1)
    big_bytes = int(lib.himo_ssl_loss_workspace_bytes(run.n0, run.n1, run.n_labels, 1025, 1024))
    big = gwords(gpu, n=big_bytes // 4)
    g = sc.GRID
    calls = {
        "n_labels = 0": (INVALID, lambda: lib.himo_ssl_loss(*run.head(n_labels=0), *run.tail())),
        "grid_cell = 0": (INVALID, lambda: lib.himo_ssl_loss(*run.head(grid=(g[0], g[1], 0.0, g[3], g[4])), *run.tail())),
        "grid_w * grid_h > 2^20": (INVALID, lambda: lib.himo_ssl_loss(*run.head(grid=(g[0], g[1], g[2], 1025, 1024)),
                                                                      *run.tail(ws_ptr=big.ptr, ws_bytes=big_bytes))),
        "workspace one byte short": (WORKSPACE, lambda: lib.himo_ssl_loss(*run.head(), *run.tail(ws_bytes=run.ws_bytes - 1))),
        "workspace pointer off by 4 bytes": (WORKSPACE, lambda: lib.himo_ssl_loss(*run.head(), *run.tail(ws_ptr=shifted.ptr + 4))),
        "distances without indices": (INVALID, lambda: lib.himo_ssl_loss_ex(*run.head(), d2.ptr, None, *run.tail())),
        "n_dyn0 = n0 + 1": (INVALID, lambda: lib.himo_ssl_loss_presized(*run.head(), d2.ptr, idx.ptr, run.n0 + 1, 0, *run.tail())),
    }
    for what, (status, call) in calls.items():
        run.fresh()
        got = call()
        torch.cuda.synchronize()
        assert got == status and got != 0, what
        assert run.grad.untouched() and run.loss.untouched() and run.ws.untouched(), what
        assert shifted.untouched() and big.untouched(), what
    run.fresh()
    loss, grad = run.plain()                                 # and the same buffers still serve a good call
    assert sc.passes(sc.compare(sc.reference("size_63x65_lattice"), loss, grad))
