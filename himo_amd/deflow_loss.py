"""Host side of the supervised loss on ground-truth flow: "DeFlow loss, v1" (``loss_fn=deflowLoss``, the launcher's other option
value at assets/slurm/ssl-train-av2.sh:34) -- end-point error averaged inside three speed bands, the bands summed, and its
gradient with respect to the estimated flow.

PARITY UNPINNED -- the reference's ``deflowLoss`` is in the absent OpenSceneFlow submodule.  The rule is this build's own, written
after the published DeFlow formulation; it is stated in include/himo_amd.h and csrc/deflowloss.hip, and in float64 in
tests/deflowloss_ref.py.  No claim is made about the reference's numbers.  Timing unmeasured.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

_lib.register({
    "himo_deflow_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "himo_deflow_loss": (ctypes.c_int, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
})

TERMS = ("slow", "medium", "fast")               # speed below 0.4 dt | up to 1.0 dt | above, of the ground-truth residual
BAND_EDGES = (0.4, 1.0)                          # in units of sensor_dt (metres per sweep interval)


def _rows(t, dev, what):
    """a float32 device view of (n, >= 3) rows with unit column stride (row pitch = stride(0): a [n][4] buffer or its [:, :3]
    go in as they are); anything else is copied into packed rows"""
    t = torch.as_tensor(t).to(device=dev, dtype=torch.float32)
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"{what}: expected (n, >= 3) rows, got {tuple(t.shape)}")
    if t.shape[0] <= 1 or t.stride(1) != 1 or t.stride(0) < 3:
        t = t.contiguous()
    return t


class DeFlowLoss:
    """``loss(pc0, moved, flow_est, gt_flow, pid=None, valid=None, sensor_dt=0.1)`` -> ({"slow", "medium", "fast"} 0-d float64
    device tensors, total, d total / d flow_est (n, 3) float32).  All arrays have n rows aligned with ``pc0``: the raw pc0 rows,
    the same points in pc1's frame as the network saw them (``moved``), the network's residual flow (the first three columns of
    the head's rows), the dataset's ``flow`` (ego motion included), optionally the pillar stage's cell ids (``pid`` < 0: dropped
    row) and ``flow_is_valid``.  The per-band row counts of the last call are in ``self.counts`` (int64 device tensor).  Nothing
    here waits for the device."""

    def __init__(self, device=None):
        self.lib = _lib.load()
        self.device = device if device is not None else _lib.require_gpu()
        self._ws = None
        self.counts = None

    def __call__(self, pc0, moved, flow_est, gt_flow, pid=None, valid=None, sensor_dt: float = 0.1):
        dev = self.device
        p, m, f, gt = _rows(pc0, dev, "pc0"), _rows(moved, dev, "moved"), _rows(flow_est, dev, "flow_est"), _rows(gt_flow, dev, "gt_flow")
        m, gt = m[:, :3].contiguous(), gt[:, :3].contiguous()
        n = p.shape[0]
        if m.shape[0] != n or f.shape[0] != n or gt.shape[0] != n:
            raise ValueError("shape mismatch between pc0, moved, flow_est and gt_flow")
        if pid is not None:
            pid = torch.as_tensor(pid).to(device=dev, dtype=torch.int32).contiguous()
            if pid.shape != (n,):
                raise ValueError("pid does not match pc0")
        if valid is not None:
            valid = torch.as_tensor(valid).to(device=dev, dtype=torch.uint8).contiguous()
            if valid.shape != (n,):
                raise ValueError("valid does not match pc0")
        need = int(self.lib.himo_deflow_loss_workspace_bytes(n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
        loss = torch.empty(4, dtype=torch.float64, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        grad = torch.empty((n, 3), dtype=torch.float32, device=dev)
        _lib.check(self.lib.himo_deflow_loss(n, _lib.ptr(p), p.stride(0) if n > 1 else p.shape[1], _lib.ptr(m), _lib.ptr(gt), _lib.ptr(f),
                                             f.stride(0) if n > 1 else f.shape[1], _lib.ptr(pid), _lib.ptr(valid), float(sensor_dt),
                                             _lib.ptr(loss), _lib.ptr(counts), _lib.ptr(grad), _lib.ptr(self._ws), self._ws.numel(),
                                             _lib.stream_handle()), "himo_deflow_loss")
        self.counts = counts
        return {name: loss[k] for k, name in enumerate(TERMS)}, loss[3], grad
