"""Stage "NSFP, v1": the Neural Scene Flow Prior baseline (result key ``nsfp``) -- a per-pair coordinate MLP fitted at run time on the
truncated Chamfer distance, with early stopping, returning its best iterate.

PARITY UNPINNED.  The reference only names the key (``nsfp`` among the compared flow producers, tools/view_instance.py:155-156;
README.md:119); its implementation is in the absent OpenSceneFlow submodule.  This docstring is the normative text of this build.

  * field, initialisation, ego pre-transform: exactly FastNSF's (``fastnsf.init_mlp``: 3 -> 128 (x8 hidden layers, ReLU) -> 3;
    p' = R p + t with inv(pose1) @ pose0 by ``himo_rigid_transform``).  Output: (N,3) float32 flow INCLUDING ego motion, row-aligned
    with pc0.
  * objective   L = (1/n0) sum_i [a_i <= tau^2] a_i + (1/n1) sum_j [b_j <= tau^2] b_j, with moved_i = p'_i + f(p'_i), a_i the squared
                distance from moved_i to its nearest pc1 point, b_j the squared distance from pc1_j to its nearest moved point, tau = 2 m.
                Correspondences are exact and constant within an iteration; ties keep the lowest row (``himo_nn_grid``'s rule, on its
                grid ``ssl_loss.GRID_*``).  n1 == 0: L = 0 with a zero gradient.  The function oracle/fastnsf_oracle.py
                ``loss_and_grads`` states.
  * optimiser   Adam(``lr``, betas (0.9, 0.999), eps 1e-8), as FastNSF.
  * defaults    lr 8e-3, iters 5000 (a cap), patience 100, min_delta 1e-4: a RECOLLECTION of the published method's settings, not a
                surveyed fact -- nothing in the reference tree states them.
  * stop and keep-best rule -- a pure function of the loss sequence L_1 .. L_T, L_t being the loss of the parameters BEFORE update t;
    every comparison in float64 (``stop_rule`` below states it on the host, csrc/nsfp.hip runs it on the device):
        state: best = +inf, best_iter = 0, stale = 0, stopped_at = 0
        at iteration t, while stopped_at == 0:
            if L_t < best - min_delta:  best = L_t, best_iter = t, stale = 0, and iteration t's MLP output is remembered
            else:                       stale += 1, and if patience > 0 and stale >= patience: stopped_at = t
        a NaN loss never improves; after stopping nothing changes; patience <= 0 never stops, the best iterate is still kept.
    The returned flow is (p' + out_best) - p.  If no iteration improved (every loss NaN or +inf) out_best is zero: the flow is the ego
    motion alone.  ``keep_best=False`` returns the LAST iterate through a closing forward pass, as FastNSF does (with patience > 0 the
    last iterate is that of the last iteration queued, see ``check_every``).  ``iters=0`` returns the initial field.
  * not built: the backward-flow / cycle-consistency network of the published method, and any multi-frame variant.

An iteration is six entry points and no host read (csrc/nsffused.hip, csrc/nsfp.hip): himo_nsf_forward_keep (the fused forward pass,
which also keeps H_7), himo_nsfp_objective (moved points, their binning, BOTH searches in one launch, d loss / d out, loss and count
sums; pc1 was binned once, by himo_nsfp_prepare), himo_nsf_last_grad (the last layer's gradients, which FastNSF's forward kernel
computes itself only together with ITS objective: H_7 is spilled rather than recomputed from H_6 -- 32 KiB per tile into a slot of the
spill that was allocated and unused, against a 128 x 128 product per tile), himo_nsf_backward and himo_nsf_update unchanged, and
himo_nsfp_keep_best (the rule above on device scalars).  Every ``check_every`` iterations the host asks for ``stopped_at`` with an
asynchronous copy and looks at the PREVIOUS answer, so it never waits for the iteration it has just queued; iterations queued beyond
the stop are wasted work and by the rule cannot alter the result.  The whole fit is bit-reproducible.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from .fastnsf import N_HIDDEN, TRUNC, _MlpParams, init_mlp
from .ssl_loss import GRID_CELL, GRID_H, GRID_W, GRID_X0, GRID_Y0

_GRID = (GRID_X0, GRID_Y0, GRID_CELL, GRID_W, GRID_H)


def stop_rule(losses, patience: int, min_delta: float):
    """-> (best_iter, stopped_at) of the loss sequence L_1 .. L_T (1-based iterations; 0 = none / never): the rule of the module docstring."""
    best, best_iter, stale, stopped_at = math.inf, 0, 0, 0
    for t, loss in enumerate(losses, 1):
        if stopped_at:
            break
        if float(loss) < best - float(min_delta):
            best, best_iter, stale = float(loss), t, 0
        else:
            stale += 1
            if patience > 0 and stale >= patience:
                stopped_at = t
    return best_iter, stopped_at


class NSFP(_MlpParams):
    def __init__(self, device=None, lr: float = 8e-3, iters: int = 5000, seed: int = 0, trunc: float = TRUNC, patience: int = 100,
                 min_delta: float = 1e-4, check_every: int = 25, keep_best: bool = True):
        self.mixed = True
        self.lib = _lib.load()
        self.device = device if device is not None else _lib.require_gpu()
        self.lr, self.iters, self.seed, self.trunc = lr, iters, seed, trunc
        self.patience, self.min_delta, self.check_every, self.keep_best = int(patience), float(min_delta), max(1, int(check_every)), bool(keep_best)
        self.loss_history, self.best_iter, self.stopped_at = [], 0, 0
        self._defer_finish, self._finish, self._flags = False, None, None

    def fit(self, pc0, pc1, pose0=None, pose1=None, layers=None) -> torch.Tensor:
        """-> (N0,3) float32 device tensor: flow of every pc0 row including ego motion.  Afterwards ``loss_history`` [(t, L_t)] holds
        every executed iteration, ``best_iter`` / ``stopped_at`` the rule's outcome."""
        lib, dev, s = self.lib, self.device, _lib.stream_handle
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(dev, torch.float32)
        p0_raw, p1 = up(pc0)[:, :3].contiguous(), up(pc1)[:, :3].contiguous()
        n, n1 = p0_raw.shape[0], p1.shape[0]
        self.loss_history, self.best_iter, self.stopped_at, self._finish = [], 0, 0, None
        if n == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=dev)
        T = np.eye(4) if pose0 is None else np.linalg.inv(np.asarray(pose1, np.float64)) @ np.asarray(pose0, np.float64)
        T32 = torch.from_numpy(np.ascontiguousarray(T, dtype=np.float32)).to(dev)
        n_pad = int(lib.himo_nsf_padded_rows(n))
        blocks, parts = int(lib.himo_nsf_backward_blocks(n)), int(lib.himo_nsfp_partials(n, n1))
        padded = lambda: torch.zeros((n_pad, 4), dtype=torch.float32, device=dev)[:n]          # (views of the padded buffers)
        self.X0, self.OUT, self.dOUT, self.BEST = padded(), padded(), padded(), padded()       # X0 = [x', y', z', 0]; padding rows zero
        _lib.check(lib.himo_rigid_transform(n, p0_raw.data_ptr(), 3, T32.data_ptr(), self.X0.data_ptr(), 4, s()), "rigid")
        self._load(init_mlp(self.seed) if layers is None else layers)
        L = len(self.W)                                         # 1 + (N_HIDDEN - 1) + 1 layers
        total = self.flat_p.numel()
        stride = (total + 63) // 64 * 64
        spill = torch.empty(int(lib.himo_nsf_spill_bytes(n, N_HIDDEN)), dtype=torch.uint8, device=dev)
        partial = torch.empty((blocks, stride), dtype=torch.float32, device=dev)
        loss_partial = torch.zeros(parts, dtype=torch.float64, device=dev)
        count_partial = torch.zeros(parts, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.himo_nsfp_workspace_bytes(n, n1, GRID_W, GRID_H)), dtype=torch.uint8, device=dev)
        moved = torch.empty((n, 3), dtype=torch.float32, device=dev)
        self._d_a, self._i_a = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        self._d_b, self._i_b = torch.empty(max(n1, 1), dtype=torch.float32, device=dev)[:n1], torch.empty(max(n1, 1), dtype=torch.int32, device=dev)[:n1]
        state = torch.zeros(8, dtype=torch.float64, device=dev)
        state[0] = math.inf
        loss_hist = torch.zeros(max(self.iters, 1), dtype=torch.float64, device=dev)       # one slot per iteration: read back ONCE, after the fit
        P = ctypes.c_void_p * N_HIDDEN
        hid = lambda bufs: P(*([None] + [bufs[k].data_ptr() for k in range(1, L - 1)]))
        wf, wb, bias = hid(self.pk_fwd), hid(self.pk_bwd), hid(self.b)
        I = ctypes.c_int * L
        off_w, off_b = I(*self.off_w), I(*self.off_b)
        p1_ptr = p1.data_ptr() if n1 else None
        _lib.check(lib.himo_nsfp_prepare(n, n1, p1_ptr, *_GRID, ws.data_ptr(), ws.numel(), s()), "himo_nsfp_prepare")      # pc1 is binned ONCE

        def forward():
            _lib.check(lib.himo_nsf_forward_keep(n, self.X0.data_ptr(), N_HIDDEN, self.W[0].data_ptr(), self.b[0].data_ptr(), wf, bias,
                                                 self.W[L - 1].data_ptr(), self.b[L - 1].data_ptr(), spill.data_ptr(), self.OUT.data_ptr(), s()),
                       "himo_nsf_forward_keep")

        polls = -(-self.iters // self.check_every) + 1
        if self.patience > 0 and (self._flags is None or self._flags.numel() < polls):
            self._flags = _lib.pinned_empty(polls, torch.float64)
        asked, done = None, 0                                   # (event, slot) of the last ``stopped_at`` asked for
        for it in range(1, self.iters + 1):
            forward()
            _lib.check(lib.himo_nsfp_objective(n, n1, self.X0.data_ptr(), self.OUT.data_ptr(), p1_ptr, *_GRID, self.trunc, moved.data_ptr(),
                                               self._d_a.data_ptr(), self._i_a.data_ptr(), self._d_b.data_ptr() if n1 else None,
                                               self._i_b.data_ptr() if n1 else None, self.dOUT.data_ptr(), loss_partial.data_ptr(),
                                               count_partial.data_ptr(), ws.data_ptr(), ws.numel(), s()), "himo_nsfp_objective")
            _lib.check(lib.himo_nsf_last_grad(n, N_HIDDEN, self.dOUT.data_ptr(), spill.data_ptr(), s()), "himo_nsf_last_grad")
            _lib.check(lib.himo_nsf_backward(n, self.X0.data_ptr(), self.dOUT.data_ptr(), N_HIDDEN, wb, self.W[L - 1].data_ptr(), spill.data_ptr(),
                                             off_w, off_b, stride, partial.data_ptr(), s()), "himo_nsf_backward")
            _lib.check(lib.himo_nsf_update(total, blocks, stride, partial.data_ptr(), parts, loss_partial.data_ptr(), count_partial.data_ptr(),
                                           self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(), self.flat_v.data_ptr(),
                                           self.lr, 0.9, 0.999, 1e-8, it, N_HIDDEN, off_w, wf, wb, loss_hist.data_ptr() + 8 * (it - 1), count.data_ptr(), s()),
                       "himo_nsf_update")
            _lib.check(lib.himo_nsfp_keep_best(n, self.OUT.data_ptr(), self.BEST.data_ptr(), loss_hist.data_ptr() + 8 * (it - 1), state.data_ptr(),
                                               it, self.patience, self.min_delta, s()), "himo_nsfp_keep_best")
            done = it
            if self.patience > 0 and it % self.check_every == 0 and it < self.iters:
                # has the rule stopped?  The answer asked for one window ago has long arrived: the host does not wait for this iteration
                if asked is not None:
                    asked[0].synchronize()
                    if self._flags[asked[1]].item() != 0.0:
                        break
                k = it // self.check_every
                self._flags[k:k + 1].copy_(state[(it & 1) * 4 + 3:(it & 1) * 4 + 4], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                asked = (ev, k)
        self._moved = moved                                     # (tests read the last iteration's objective)
        if not (self.keep_best and done):
            forward()                                           # the last iterate (or the initial field)
        out = self.BEST if (self.keep_best and done) else self.OUT
        flow = torch.empty((n, 3), dtype=torch.float32, device=dev)
        final = torch.empty((n, 3), dtype=torch.float32, device=dev)
        # flow incl. ego motion = (p' + f(p')) - p
        _lib.check(lib.himo_rows_add(n, 3, self.X0.data_ptr(), 4, out.data_ptr(), 4, 1.0, final.data_ptr(), 3, 0, s()), "rows_add")
        _lib.check(lib.himo_rows_add(n, 3, final.data_ptr(), 3, p0_raw.data_ptr(), 3, -1.0, flow.data_ptr(), 3, 0, s()), "rows_add")

        def finish():
            # the loss trajectory and the rule's outcome, read once the whole fit is queued
            if done:
                hist = loss_hist[:done].cpu().numpy()
                self.loss_history = [(it, float(hist[it - 1])) for it in range(1, done + 1)]
                st = state[(done & 1) * 4:(done & 1) * 4 + 4].cpu().numpy()
                self.best_iter, self.stopped_at = int(st[1]), int(st[3])
        self._finish = finish
        if not self._defer_finish:
            self.wait()
        return flow

    def fit_async(self, pc0, pc1, pose0=None, pose1=None, layers=None) -> torch.Tensor:
        """``fit`` without its closing host reads: the flow tensor is valid in stream order, ``wait()`` reads ``loss_history``,
        ``best_iter`` and ``stopped_at``.  With ``patience <= 0`` every launch of the fit is queued at once; with early stopping the host
        follows the fit one ``check_every`` window behind, so a second engine overlaps only the fit's last windows.
        Two fits in flight: ``fastnsf.OverlappedFastNSF(engine=NSFP, ...)``."""
        self._defer_finish = True
        try:
            return self.fit(pc0, pc1, pose0, pose1, layers)
        finally:
            self._defer_finish = False

    def wait(self):
        """completes a ``fit_async`` (blocks on the fit's stream)"""
        f, self._finish = self._finish, None
        if f is not None:
            f()

