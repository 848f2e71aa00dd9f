"""Drop-in for the reference's ``downstream/eval_seg.py``: the segmentation mIoU table (downstream/README.md, Table IV) of
``seg_raw`` / ``seg_<res_name>`` against ``flow_category_indices`` over three classes (ignore, car, other vehicle).

Same public names as the reference:
    CATEGORY_TO_INDEX, INDEX_TO_CATEGORY, CAR, OTHER_VEHICLES                      eval_seg.py:24-28, :82-93
    iouEval(n_classes=3, ignore=[])  .addBatch(x, y) .getStats() .getIoU() .reset() .num_classes()     eval_seg.py:94-153
    main(data_dir, res_names)                                                      eval_seg.py:234-286

What runs where: the class remap of eval_seg.py:255-257 / :261-263 and the confusion matrices of ``iouEval.addBatch``
(eval_seg.py:113-134) run in one HIP kernel per packed batch of sweeps (csrc/segiou.hip, ``himo_seg_confusion``), for every
result name and for both choices of eval_seg.py:250 at once: ``conf[r][0]`` counts all points ("All", the reference as
shipped), ``conf[r][1]`` the points with ``seg_valid`` set ("Mask only", the reference with line 250 removed).  The matrices
are integers, so they equal the reference's element for element; the nine-number IoU arithmetic of eval_seg.py:136-153 stays on
the host in float64, in the reference's own order.  ``SegMetrics`` is the batched form ``main`` is built on; with
``torch.distributed`` initialised the sweeps are sharded across ranks (frame i -> rank i % world) and the matrices summed by one
all-reduce.
"""
from __future__ import annotations

import ctypes
import time

import numpy as np

from . import _lib
from .eval import ANNOTATION_CATEGORIES, BUCKETED_METACATAGORIES
from .eval import CATEGORY_TO_INDEX as _AV2_CATEGORY_TO_INDEX
from .sweeps import MissingKey, SweepPacker, fed, raise_missing, sharded_batches, timed

# the package's AV2 table (eval.py; the reference builds the same dict from av2's AnnotationCategories, eval_seg.py:24-27)
CATEGORY_TO_INDEX = dict(_AV2_CATEGORY_TO_INDEX)
INDEX_TO_CATEGORY = {v: k for k, v in CATEGORY_TO_INDEX.items()}
CAR = list(BUCKETED_METACATAGORIES["CAR"])
OTHER_VEHICLES = list(BUCKETED_METACATAGORIES["OTHER_VEHICLES"])
assert len(CATEGORY_TO_INDEX) == len(ANNOTATION_CATEGORIES) + 1

CLASS_STRINGS = {0: "ignore", 1: "car", 2: "other_vehicle"}       # eval_seg.py:278
MODES = ("All", "Mask only")
MAX_RESULTS = 8                                                   # HIMO_SEG_MAX_RESULTS


def class_lut() -> np.ndarray:
    """uint8[256]: category index -> 0 (ignore) | 1 (car) | 2 (other vehicle), the ONE table that stands for the reference's three
    in-place assignments (eval_seg.py:255-257).  They collapse to a table only while no value a step writes is caught by a later
    step: 0 must be in neither list, the lists must be disjoint, and 1 (what step 2 writes) must not be in OTHER_VEHICLES, or
    step 3 would turn every car into class 2.  Checked here, so a changed category table fails instead of counting wrongly."""
    car = [CATEGORY_TO_INDEX[c] for c in CAR]
    other = [CATEGORY_TO_INDEX[c] for c in OTHER_VEHICLES]
    if 0 in car + other or set(car) & set(other) or 1 in other:
        raise ValueError("the three remap steps of eval_seg.py:255-257 do not collapse to one table for this category table")
    lut = np.zeros(256, dtype=np.uint8)
    lut[car] = 1
    lut[other] = 2
    return lut


def identity_lut() -> np.ndarray:
    """labels that are classes already (``iouEval.addBatch``): 0, 1, 2 stay, every other byte value counts as class 0"""
    lut = np.zeros(256, dtype=np.uint8)
    lut[:3] = (0, 1, 2)
    return lut


def parse_res_names(value) -> list:
    """``--res_names``: ``seg_raw,seg_flow`` or the reference's list spelling ``"['seg_raw','seg_flow']"`` (what ``fire`` parses);
    a list / tuple passes through."""
    if isinstance(value, (list, tuple)):
        names = [str(v) for v in value]
    else:
        text = str(value).strip()
        if text[:1] in "[(" and text[-1:] in "])":
            text = text[1:-1]
        names = [part.strip().strip("'\"").strip() for part in text.split(",")]
        names = [n for n in names if n]
    if not names:
        raise ValueError(f"no result name in {value!r}")
    return names


def as_labels_u8(a) -> np.ndarray:
    """flat uint8 labels of a host array: uint8 and bool as they are, any other dtype cast with values outside 0..255 -> 0"""
    a = np.asarray(a).reshape(-1)
    if a.dtype == np.uint8:
        return a
    if a.dtype == np.bool_:
        return a.view(np.uint8)
    return np.where((a >= 0) & (a <= 255), a, 0).astype(np.uint8)


def seg_confusion(conf, gt, preds, valid=None, lut: np.ndarray | None = None) -> None:
    """``conf`` (device int64 [R][2][3][3]) += the confusion matrices of the device uint8 arrays ``preds`` (R of them) against
    ``gt``, over all points and over those where ``valid`` (device uint8 or None) is set: one launch on the current stream."""
    lut = class_lut() if lut is None else np.ascontiguousarray(lut, dtype=np.uint8)
    n = int(gt.numel())
    r = len(preds)
    if not 1 <= r <= MAX_RESULTS:
        raise ValueError(f"{r} result arrays: himo_seg_confusion takes 1..{MAX_RESULTS}")
    if tuple(conf.shape) != (r, 2, 3, 3) or not conf.is_contiguous():
        raise ValueError(f"conf must be a contiguous int64 [{r}][2][3][3] tensor")
    for t in list(preds) + ([valid] if valid is not None else []):
        if int(t.numel()) != n:
            raise ValueError("prediction / seg_valid arrays must have as many points as the ground truth")
    ptrs = (ctypes.c_void_p * r)(*[_lib.ptr(p) if n else None for p in preds])
    _lib.check(_lib.load().himo_seg_confusion(n, _lib.ptr(gt) if n else None, ptrs, r, _lib.ptr(valid) if (valid is not None and n) else None,
                                              lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _lib.ptr(conf), _lib.stream_handle()),
               "himo_seg_confusion")


def iou_from_conf(conf_matrix, ignore, include):
    """eval_seg.py:136-153 on one matrix: (tp, fp, fn), (mean IoU over ``include``, per-class IoU), float64 in the reference's order"""
    conf = np.asarray(conf_matrix).astype(np.float64)
    conf[:, ignore] = 0
    tp = np.diag(conf)
    fp = conf.sum(axis=1) - tp
    fn = conf.sum(axis=0) - tp
    union = tp + fp + fn + 1e-15
    iou = tp / union
    iou_mean = (tp[include] / union[include]).mean()
    return (tp, fp, fn), (iou_mean, iou)


class iouEval:  # noqa: N801  (the reference's name)
    """eval_seg.py:94-153 with the matrix accumulated on the device.  ``x`` / ``y`` are class labels (0, 1, 2): host arrays of any
    integer dtype (cast on the host; values outside 0..255 count as class 0, as do byte values above 2) or device uint8 tensors.
    ``conf_matrix`` is the host int64 view of the counts so far (reading it synchronises; assigning replaces the counts).
    The kernel counts three classes, so ``n_classes`` must be 3."""

    def __init__(self, n_classes=3, ignore=None):
        if n_classes != 3:
            raise ValueError("iouEval on the device path counts exactly 3 classes (ignore, car, other vehicle)")
        self.n_classes = n_classes
        self.ignore = np.array([] if ignore is None else ignore, dtype=np.int64)
        self.include = np.array([n for n in range(self.n_classes) if n not in self.ignore], dtype=np.int64)
        self._dev = None
        self.reset()

    def num_classes(self):
        return self.n_classes

    def reset(self):
        self._host = np.zeros((self.n_classes, self.n_classes), dtype=np.int64)
        if self._dev is not None:
            self._dev.zero_()

    @property
    def conf_matrix(self) -> np.ndarray:
        if self._dev is not None:
            self._host = self._host + self._dev[0, 0].cpu().numpy()
            self._dev.zero_()
        return self._host

    @conf_matrix.setter
    def conf_matrix(self, value):
        self._host = np.array(value, dtype=np.int64).reshape(self.n_classes, self.n_classes)
        if self._dev is not None:
            self._dev.zero_()

    def addBatch(self, x, y):  # noqa: N802  x=preds, y=targets
        import torch
        dev = _lib.require_gpu()

        def on_device(a):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.dtype != torch.uint8:
                    a = torch.where((a >= 0) & (a <= 255), a, torch.zeros_like(a)).to(torch.uint8)
                return a.reshape(-1).contiguous()
            if isinstance(a, torch.Tensor):
                a = a.numpy()
            return torch.from_numpy(np.ascontiguousarray(as_labels_u8(a))).to(dev)
        xd, yd = on_device(x), on_device(y)
        if xd.numel() != yd.numel():
            raise ValueError("predictions and targets differ in size")
        if self._dev is None:
            self._dev = torch.zeros((1, 2, 3, 3), dtype=torch.int64, device=dev)
        seg_confusion(self._dev, yd, [xd], None, identity_lut())

    def getStats(self):  # noqa: N802
        return iou_from_conf(self.conf_matrix, self.ignore, self.include)[0]

    def getIoU(self):  # noqa: N802
        return iou_from_conf(self.conf_matrix, self.ignore, self.include)[1]


class SegBatch:
    """A packed batch of sweeps on the device: ``gt``, ``valid`` and ``preds[r]`` are uint8 [T], packed alike."""

    def __init__(self, gt, valid, preds, sweeps: int):
        self.gt, self.valid, self.preds, self.sweeps = gt, valid, preds, sweeps

    @property
    def total_points(self) -> int:
        return int(self.gt.numel())

    def tensors(self) -> list:
        return [self.gt, self.valid] + list(self.preds)

    @classmethod
    def from_frames(cls, frames, res_names, device=None, upload=None) -> "SegBatch":
        """``frames``: dicts with ``flow_category_indices``, ``seg_valid`` and every name of ``res_names`` (a missing key is the
        reference's KeyError, eval_seg.py:248 / :260).  ``upload(parts, dtype)``: the feeder's staging (``feeder.BatchFeeder``);
        None: one plain copy per array."""
        p = SweepPacker(frames, upload, device, count_key="flow_category_indices")
        gt, valid, *preds = [p.cat(key, np.uint8, labels=True) for key in ("flow_category_indices", "seg_valid") + tuple(res_names)]
        return cls(gt, valid, preds, len(p.frames))


class SegMetrics:
    """The batched evaluator: one device accumulator ``conf[R][2][3][3]`` for ``res_names``, fed whole batches of sweeps."""

    def __init__(self, res_names, device=None):
        self.res_names = parse_res_names(res_names)
        if len(self.res_names) > MAX_RESULTS:
            raise ValueError(f"{len(self.res_names)} result names: at most {MAX_RESULTS} are evaluated in one pass")
        self.device = device
        self.lut = class_lut()
        self.host = np.zeros((len(self.res_names), 2, 3, 3), dtype=np.int64)      # what has been folded off the device (or set)
        self._dev = None
        self.frame_cnt = 0
        self.points = 0

    def add_batch(self, batch: SegBatch) -> None:
        import torch
        if self._dev is None:
            self.device = self.device if self.device is not None else _lib.require_gpu()
            self._dev = torch.zeros(self.host.shape, dtype=torch.int64, device=self.device)
        seg_confusion(self._dev, batch.gt, batch.preds, batch.valid, self.lut)
        self.frame_cnt += batch.sweeps
        self.points += batch.total_points

    def add(self, frames) -> None:
        """the sweeps of ``frames`` (host dicts) as one packed batch, one launch"""
        frames = list(frames)
        if frames:
            self.add_batch(SegBatch.from_frames(frames, self.res_names, device=self.device))

    @property
    def conf(self) -> np.ndarray:
        """host int64 [R][2][3][3] (synchronises)"""
        if self._dev is not None:
            self.host = self.host + self._dev.cpu().numpy()
            self._dev.zero_()
        return self.host

    def reset(self) -> None:
        self.host = np.zeros_like(self.host)
        if self._dev is not None:
            self._dev.zero_()
        self.frame_cnt = self.points = 0

    def gather(self) -> None:
        """Sum the matrices over the ranks of the process group: ONE all-reduce of 18 R integers (on the host over gloo, on the
        device over RCCL).  Integer sums: every rank ends with exactly the single-process matrices."""
        import torch
        import torch.distributed as dist
        conf = self.conf
        if not (dist.is_available() and dist.is_initialized()):
            return
        t = torch.from_numpy(np.concatenate([conf.reshape(-1), [self.frame_cnt, self.points]]).astype(np.int64))
        if dist.get_backend() == "nccl":
            t = t.to(torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        flat = t.cpu().numpy()
        self.host = flat[:-2].reshape(conf.shape).copy()
        self.frame_cnt, self.points = int(flat[-2]), int(flat[-1])

    def evaluator(self, name: str, mode=0) -> iouEval:
        """the reference's per-name evaluator (eval_seg.py:239) holding this name's matrix of ``mode`` (0 / "All", 1 / "Mask only")"""
        ev = iouEval(n_classes=3, ignore=[])
        ev.conf_matrix = self.conf[self.res_names.index(name), _mode_index(mode)]
        return ev

    def table(self, mode=0) -> str:
        """the reference's result block (eval_seg.py:272-286) for ``mode``, as the text its ``print`` calls put on stdout"""
        out = ["\n  ========================== RESULTS ==========================  "]
        for name in self.res_names:
            _, class_jaccard = self.evaluator(name, mode).getIoU()
            m_jaccard = class_jaccard[1:].mean()
            out.append("{name} 100 frames val:\nIoU avg {m_jaccard:.3f}".format(name=name, m_jaccard=m_jaccard * 100))
            for i, jacc in enumerate(class_jaccard):
                if i == 0:                                            # eval_seg.py:277: class 0 is not listed
                    continue
                out.append("IoU class {i:} [{class_str:}] = {jacc:.3f}".format(i=i, class_str=CLASS_STRINGS[i], jacc=jacc * 100))
            out.append("-" * 20)
        return "\n".join(out) + "\n"


def _mode_index(mode) -> int:
    if mode in (0, 1):
        return int(mode)
    return {m.lower(): k for k, m in enumerate(MODES)}[str(mode).lower()]


def sweep_warnings(frame: dict, res_names) -> list:
    """the lines the reference's loader prints for the keys a sweep lacks (eval_seg.py:219-223), in its order"""
    return [f"[Warning]: No {key} in {frame['scene_id']} at {frame['timestamp']}, check the data."
            for key in ["seg_valid", "flow_category_indices"] + list(res_names) if key not in frame]


def run_dataset(dataset, metrics: SegMetrics, batch_frames: int = 32, overlap: bool = True) -> int:
    """Shared body of ``main``: sweep i of ``dataset`` on rank i % world, ``batch_frames`` sweeps per launch.  A sweep without
    ``flow_category_indices`` is skipped with the reference's warnings (eval_seg.py:245-247); one that lacks ``seg_valid`` or a
    result name raises ``KeyError`` naming it, where the reference fails (eval_seg.py:248, :260).  With ``overlap`` the batches
    are read, packed and copied two ahead by ``feeder.BatchFeeder``; the warnings travel with their batch and are printed by the
    calling thread, in sweep order.  Returns the sweeps this rank evaluated."""
    names = metrics.res_names

    def batches():
        for keys in sharded_batches(dataset, batch_frames):
            frames, lines = [], []
            for i in keys:
                f = dataset[i]
                lines += sweep_warnings(f, names)
                if "flow_category_indices" not in f:
                    lines.append(f"[Warning]: No flow_category_indices in {f['scene_id']} at {f['timestamp']}, check the data.")
                    continue
                for key in ["seg_valid"] + names:
                    if key not in f:
                        raise MissingKey(key, lines)
                frames.append(f)
            yield frames, lines

    if overlap and metrics.device is None:
        metrics.device = _lib.require_gpu()

    def build(item, upload):
        frames, lines = item
        return (SegBatch.from_frames(frames, names, device=metrics.device, upload=upload) if frames else None), lines
    done = 0
    try:
        for batch, lines in fed(batches(), build, device=metrics.device, overlap=overlap):
            for line in lines:
                print(line)
            if batch is not None:
                metrics.add_batch(batch)
                done += batch.sweeps
    except MissingKey as e:
        raise_missing(e)
    return done


def main(data_dir: str = "/home/kin/data/av2/h5py/sensor/himo", res_names: list = ["seg_raw", "seg_flow"],  # noqa: B006
         mask_only: bool = False, both: bool = False, batch_frames: int = 32, dataset=None):
    """eval_seg.py:234-286.  ``mask_only``: the "Mask only" table (the reference with its line 250 removed) instead of "All";
    ``both``: "All", then "Mask only".  The evaluation list is ``index_eval.pkl`` (the reference hard-codes ``val=True``).  Under
    ``torchrun`` sweep i is counted by rank i % world on its own GPU and rank 0 prints.  Returns the ``SegMetrics``."""
    from . import distenv
    from .dataset import SEG_FIELDS, open_dataset

    names = parse_res_names(res_names)

    def loop():
        t0 = time.perf_counter()
        data = dataset if dataset is not None else open_dataset(data_dir, vis_name=names, eval=True, fields=SEG_FIELDS + tuple(names), need_next=False)
        done = run_dataset(data, metrics, batch_frames=batch_frames)
        metrics.conf                                             # (wait for the device: the loop's time includes its kernels)
        metrics.loop = {"seconds": time.perf_counter() - t0, "sweeps": done}
    with distenv.process_group() as (rank, world):
        metrics = SegMetrics(names)
        distenv.run_shard(loop, "its sweeps, but no table was printed")
        metrics.gather()
        if rank == 0:
            for mode in ((0, 1) if both else ((1,) if mask_only else (0,))):
                print(metrics.table(mode), end="")
    return metrics


def _cli(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="segmentation mIoU of seg_<name> against flow_category_indices (MI355X path)")
    ap.add_argument("--data_dir", default="/home/kin/data/av2/h5py/sensor/himo")
    ap.add_argument("--res_names", default="seg_raw,seg_flow", help="seg_raw,seg_flow  or  \"['seg_raw','seg_flow']\"")
    ap.add_argument("--mask_only", action="store_true", help="count only the points with seg_valid set")
    ap.add_argument("--both", action="store_true", help="print the table over all points, then the one over seg_valid")
    ap.add_argument("--batch_frames", type=int, default=32)
    a = ap.parse_args(argv)
    return main(a.data_dir, parse_res_names(a.res_names), mask_only=a.mask_only, both=a.both, batch_frames=a.batch_frames)


if __name__ == "__main__":
    timed(_cli)
