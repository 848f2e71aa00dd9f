"""The training loop around ``SeFlowTrainer`` -- this build's counterpart of the reference's training job
(``python train.py model=deflowpp ... loss_fn=seflowppLoss batch_size=8 epochs=12 save_top_model=3 optimizer.lr=6e-5
+optimizer.scheduler.name=StepLR +...step_size=3 +...gamma=0.5``, assets/slurm/ssl-train-av2.sh:31-34, on 4 GPUs :3).

PARITY UNPINNED: ``OpenSceneFlow/train.py`` is absent, so only the launcher's numbers are mirrored: epochs over the
dataset, ``batch_size`` samples per optimiser step (spread over the ranks: a rank's share goes through the network in ONE
pass, the ranks' gradient sums and sample counts are added -- bucket by bucket under the backward pass, ``train.BucketedAllReduce``
-- and the sum is divided by the global count: every sample of a batch weighs the same however it splits over the ranks),
``num_workers`` threads preparing samples ahead of the step (``feeder.TrainFeeder``), Adam at ``lr`` with StepLR(step_size, gamma) per epoch, the
``save_top`` best checkpoints kept by the epoch's validation (or mean training) loss, and resuming from a checkpoint.
Conventions of this build: BatchNorm runs in TRAINING mode by default (``batchnorm="batch"``: batch statistics, trainable
gamma / beta, running statistics with momentum 0.1 -- the launcher passes no checkpoint, so the reference's job trains from
scratch; statistics are per forward call = over a rank's share of the step's batch, as torch.nn.BatchNorm takes them in a
per-process batch, un-synchronised across ranks like DDP's default, and rank 0's running statistics go into the checkpoints); ``batchnorm="frozen"`` is the fine-tuning convention (running statistics
and affine folded into constants); validation always uses the running statistics; the labels (0 static, > 0 dynamic
cluster id) are GENERATED from the sweep pair on the GPU by default (``ssl_label="seflow_auto"``, the launcher's
``+ssl_label=seflow_auto``: seflow/ssl_label.py -- nearest-neighbour dynamic candidates + DBSCAN; the reference's generator
and its label files are absent: unpinned); ``ssl_label=<frame key>`` (e.g. ``flow_instance_id``) reads them from the frames.

``loss_fn="deflowLoss"`` (the launcher's other option value, ssl-train-av2.sh:34) trains SUPERVISED on the ground-truth ``flow`` every
labelled frame carries ("DeFlow loss, v1", himo_amd/deflow_loss.py; parity unpinned, no claim about the reference's numbers): no
labels are generated or read, validation uses the same loss, and the samples are built on the launch thread inside the step loop
(``make_supervised_sample``, the shape of ``num_workers=0``) -- ``feeder.TrainFeeder`` does not prefetch supervised samples (timing
unmeasured).

``val_metric="three_way"`` / ``"mean_dynamic"`` ranks the checkpoints by FLOW ERROR instead of the validation loss (which for the
self-supervised loss is only a proxy for it): after a validated epoch every validation triplet of the rank goes through ONE
``forward(training=False)`` pass and ONE ``eval_flow.flow_metrics`` launch in residual mode, straight on the head's residual rows
and the sample's device arrays ("flow metrics, v1" with rules 3b and 9, himo_amd/eval_flow.py; parity unpinned) -- no labels are
read or generated, nothing waits for the device per sample -- and ``FlowMetrics.gather()`` adds the ranks' integers.  The
validation frames must carry ``flow``, ``flow_category_indices`` and ``gm0`` (Scania: ``flow_is_valid`` too).  ``val_every=k``
(the launcher's ``val_every=3``, ssl-train-av2.sh:32; default 1) validates epoch e iff ``(e + 1) % k == 0`` or e is the last.
"""
from __future__ import annotations

import math
import time
from pathlib import Path

import numpy as np
import torch

from .checkpoint import TopK
from .train import SeFlowTrainer


def triplets(dataset):
    """(history, current, next) frame indices of every frame that has a successor in its scene (the history frame is the
    previous sweep of the scene, else the frame itself -- ``num_frames=3``, ssl-train-av2.sh:32).  A dataset whose frames
    carry their successor themselves (``HDF5Dataset``: ``pc1`` / ``pose1`` come from the next timestamp, and successor-less
    sweeps are not in its index at all) yields ``next = None`` for EVERY entry -- the last usable sweep of a scene included."""
    index = getattr(dataset, "index", None)
    scene = (lambda i: index[i][0]) if index is not None else (lambda i: dataset[i].get("scene_id"))
    n = len(dataset)
    carries_next = n > 0 and "pc1" in dataset[0]
    out = []
    for i in range(n):
        ih = i - 1 if i > 0 and scene(i - 1) == scene(i) else i
        if carries_next:
            out.append((ih, i, None))
        elif i + 1 < n and scene(i + 1) == scene(i):
            out.append((ih, i, i + 1))
    return out


AUTO_LABELS = ("seflow_auto", "seflowpp_auto")                  # the launchers' option values (ssl-train-av2.sh:32, ssl-train-scania.sh:32)


# the frame keys the training loop reads (``HDF5Dataset(fields=...)``): the sweep pair, their poses and -- for generated labels --
# their ground masks; a run on stored labels adds its label key (and ``<key>_next``) with ``train_fields``
TRAIN_FIELDS = ("pc0", "pose0", "pose1", "pc1", "gm0", "gm1")


def train_fields(label_key: str = "seflow_auto") -> tuple:
    return TRAIN_FIELDS if label_key in AUTO_LABELS else TRAIN_FIELDS + (label_key, label_key + "_next")


LOSS_FNS = ("seflowppLoss", "deflowLoss")                     # the launcher's option values (ssl-train-av2.sh:34)

# ... and what a supervised run reads: the sweep pair, their poses, the ground-truth flow and (where the file has it) its validity
SUPERVISED_FIELDS = ("pc0", "pose0", "pose1", "pc1", "flow", "flow_is_valid")


def loss_fields(loss_fn: str = "seflowppLoss", label_key: str = "seflow_auto") -> tuple:
    """the frame keys a run with ``loss_fn`` reads (``label_key`` only matters to the self-supervised loss)"""
    if loss_fn not in LOSS_FNS:
        raise ValueError(f"loss_fn={loss_fn!r}: one of {LOSS_FNS}")
    return SUPERVISED_FIELDS if loss_fn == "deflowLoss" else train_fields(label_key)


def _frame(dataset, i, fields=None):
    """``dataset[i]``, restricted to ``fields`` where the dataset can restrict a read (``HDF5Dataset.read``)"""
    read = getattr(dataset, "read", None)
    return read(i, fields) if (read is not None and fields is not None) else dataset[i]


def host_sample(dataset, trip, label_key: str = "flow_instance_id") -> dict:
    """The HOST half of a training sample: {"pch1", "pc0", "pc1" (float32 arrays, possibly views of a file mapping), "pose_h1",
    "pose0", "pose1" (float64 4x4), and either "gm0" / "gm1" (``label_key`` in ``AUTO_LABELS``: the labels are generated from the
    pair and its ground masks) or "lab0" / "lab1" (the frame key that holds them)}.  Same errors as the reference's loader would
    raise at the same point: a missing key is a KeyError naming it."""
    ih, i0, i1 = trip
    f0 = dataset[i0]
    fh = _frame(dataset, ih, ("pc0", "pose0")) if ih != i0 else f0
    auto = label_key in AUTO_LABELS
    if i1 is None:                                            # the frame carries its successor (HDF5Dataset)
        pc1, lab1, gm1 = f0["pc1"], f0.get(label_key + "_next"), f0.get("gm1")
        if lab1 is None and not auto:
            raise KeyError(f"{label_key}_next: the frame carries pc1 but not its labels")
    else:
        f1 = dataset[i1]
        pc1, lab1, gm1 = f1["pc0"], f1.get(label_key), f1.get("gm0")
        if lab1 is None and not auto:
            raise KeyError(f"{label_key}: the next frame does not hold the labels ssl_label={label_key!r} names "
                           f"(ssl_label='seflow_auto' generates them from the sweeps and their ground masks gm0 / gm1; "
                           f"`python -m himo_amd.ground_seg` writes them)")
    if not auto and f0.get(label_key) is None:
        raise KeyError(f"{label_key}: the frame does not hold the labels ssl_label={label_key!r} names "
                       f"(ssl_label='seflow_auto' generates them from the sweeps and their ground masks gm0 / gm1; "
                       f"`python -m himo_amd.ground_seg` writes them)")
    out = {"pch1": fh["pc0"], "pc0": f0["pc0"], "pc1": pc1, "pose_h1": np.asarray(fh["pose0"], np.float64),
           "pose0": np.asarray(f0["pose0"], np.float64), "pose1": np.asarray(f0["pose1"], np.float64)}
    if auto:
        if f0.get("gm0") is None or gm1 is None:
            raise KeyError("gm0 / gm1: ssl_label=seflow_auto needs the ground masks of both sweeps "
                           "(`python -m himo_amd.ground_seg` writes them)")
        out["gm0"], out["gm1"] = f0["gm0"], gm1
    else:
        out["lab0"], out["lab1"] = f0[label_key], lab1
    return out


def make_sample(dataset, trip, device, label_key: str = "flow_instance_id"):
    """(pch1, pc0, pc1, pose_h1, pose0, pose1, label0, label1, n_labels) on ``device`` for one triplet, built HERE and NOW on the
    calling thread and the current stream (tests, one-off calls; the training loop takes the same tuples from
    ``feeder.TrainFeeder``, which prepares them ahead of the step).  ``label_key`` in ``AUTO_LABELS``: the labels are generated
    from the pair (needs the sweeps' ground masks ``gm0``; a frame that carries its successor also carries ``gm1``); any other
    value names the frame key that holds them."""
    h = host_sample(dataset, trip, label_key)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    lab = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(device)
    p0, p1 = up(h["pc0"]), up(h["pc1"])
    if "gm0" in h:
        from .ssl_label import auto_labels
        l0, l1, top = auto_labels(p0, p1, h["gm0"], h["gm1"], h["pose0"], h["pose1"], return_top=True)
        n_labels = int(top.item()) + 1
    else:
        l0, l1 = lab(h["lab0"]), lab(h["lab1"])
        n_labels = int(max(int(np.max(h["lab0"], initial=0)), int(np.max(h["lab1"], initial=0)))) + 1
    return (up(h["pch1"]), p0, p1, h["pose_h1"], h["pose0"], h["pose1"], l0, l1, n_labels)


def make_supervised_sample(dataset, trip, device):
    """(pch1, pc0, pc1, pose_h1, pose0, pose1, gt_flow, valid_or_None) on ``device`` for one triplet -- the sample of
    ``SeFlowTrainer(loss="deflow")`` -- built here and now on the calling thread and the current stream.  ``flow`` (n0, 3) is the
    frame's ground truth with ego motion; ``flow_is_valid`` is optional.  A frame without ``flow`` is a KeyError naming it."""
    ih, i0, i1 = trip
    f0 = dataset[i0]
    fh = _frame(dataset, ih, ("pc0", "pose0")) if ih != i0 else f0
    if f0.get("flow") is None:
        raise KeyError("flow: loss_fn=deflowLoss trains on the ground-truth flow, which this frame does not hold")
    pc1 = f0["pc1"] if i1 is None else dataset[i1]["pc0"]
    if np.shape(f0["flow"]) != (np.shape(f0["pc0"])[0], 3):
        raise ValueError(f"flow has shape {np.shape(f0['flow'])} for {np.shape(f0['pc0'])[0]} points")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    valid = f0.get("flow_is_valid")
    if valid is not None:
        valid = torch.from_numpy(np.ascontiguousarray(valid).astype(np.uint8)).to(device)
    return (up(fh["pc0"]), up(f0["pc0"]), up(pc1), np.asarray(fh["pose0"], np.float64), np.asarray(f0["pose0"], np.float64),
            np.asarray(f0["pose1"], np.float64), up(f0["flow"]), valid)


VAL_METRICS = ("loss", "three_way", "mean_dynamic")

# what a validation pass by flow error reads (``flow_is_valid`` where the file has it; Scania requires it)
VAL_FLOW_FIELDS = ("pc0", "pose0", "pose1", "pc1", "flow", "flow_category_indices", "gm0", "flow_is_valid")


def validates(epoch: int, epochs: int, val_every: int = 1) -> bool:
    """whether the 0-based ``epoch`` of a run of ``epochs`` validates: every ``val_every``-th one and the last"""
    if val_every < 1:
        raise ValueError(f"val_every={val_every}: at least 1")
    return (epoch + 1) % val_every == 0 or epoch == epochs - 1


def validation_epochs(epochs: int, val_every: int = 1, start_epoch: int = 0) -> list:
    """the 0-based epochs of a run that validate (and are offered to ``TopK``)"""
    return [e for e in range(start_epoch, epochs) if validates(e, epochs, val_every)]


def make_validation_sample(dataset, trip, device, scania: bool = False):
    """((pch1, pc0, pc1, pose_h1, pose0, pose1), gt_flow, category, ground, valid_or_None) on ``device`` for one triplet: the
    forward pass's sample and the ground-truth arrays "flow metrics, v1" reads (float32 [n0][3], uint8 [n0] each).  A frame
    without one of them is a KeyError naming it."""
    ih, i0, i1 = trip
    f0 = dataset[i0]
    fh = _frame(dataset, ih, ("pc0", "pose0")) if ih != i0 else f0
    for key in ("flow", "flow_category_indices", "gm0") + (("flow_is_valid",) if scania else ()):
        if f0.get(key) is None:
            raise KeyError(f"{key}: validation by flow error reads it, and this validation frame does not hold it")
    pc1 = f0["pc1"] if i1 is None else dataset[i1]["pc0"]
    n0 = np.shape(f0["pc0"])[0]
    if np.shape(f0["flow"]) != (n0, 3):
        raise ValueError(f"flow has shape {np.shape(f0['flow'])} for {n0} points")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)

    def byte(key):
        a = np.ascontiguousarray(f0[key]).reshape(-1)
        if a.shape[0] != n0:
            raise ValueError(f"{key} has {a.shape[0]} entries for {n0} points")
        return torch.from_numpy(a.astype(np.uint8)).to(device)
    valid = byte("flow_is_valid") if f0.get("flow_is_valid") is not None else None
    fwd = (up(fh["pc0"]), up(f0["pc0"]), up(pc1), np.asarray(fh["pose0"], np.float64), np.asarray(f0["pose0"], np.float64),
           np.asarray(f0["pose1"], np.float64))
    return fwd, up(f0["flow"]), byte("flow_category_indices"), byte("gm0"), valid


def validate_flow(tr, val_dataset, val_trips, rank: int = 0, world: int = 1, data_name: str = "av2") -> dict:
    """One validation pass by flow error: triplet j of ``val_trips`` on rank j % world (keyed by j), one inference pass and one
    residual-mode ``flow_metrics`` launch each, then ``gather()`` (EVERY rank calls this).  Returns ``results()["val"]``."""
    from ..eval_flow import FlowBatch, FlowMetrics
    metrics = FlowMetrics(["val"], data_name, device=tr.device, accuracy=True, residual=True)
    for j in range(rank, len(val_trips), world):
        fwd, gt, category, ground, valid = make_validation_sample(val_dataset, val_trips[j], tr.device, scania=data_name == "scania")
        tr.forward(*fwd, training=False)
        pc0, res = tr.flow_rows(0)
        metrics.add_batch(FlowBatch.from_device(pc0, gt, [res], category, ground, fwd[4], fwd[5], valid=valid, keys=[j]))
    metrics.gather()
    return metrics.results()["val"]


def fit(dataset, params: dict | None = None, out_dir=None, epochs: int = 12, batch_size: int = 8, lr: float = 6e-5,
        step_size: int = 3, gamma: float = 0.5, save_top: int = 3, val_dataset=None, resume=None, precision: str = "mixed",
        max_points: int = 140_000, device=None, seed: int = 0, max_steps: int | None = None, log=print,
        trainer: SeFlowTrainer | None = None, batchnorm: str = "batch", ssl_label: str = "seflow_auto",
        num_workers: int = 1, prefetch: int = 2, label_lanes: int = 1,
        cache_labels: bool = True, loss_fn: str = "seflowppLoss", val_metric: str = "loss", val_every: int = 1,
        val_data_name: str = "av2") -> dict:
    """Train for ``epochs`` passes over ``dataset``; returns {"trainer", "history", "best"}.

    ``num_workers`` > 0 (default; the launcher's ``num_workers=16``, ssl-train-av2.sh:32): the samples of an epoch come from
    ``feeder.TrainFeeder`` -- read on that many threads, staged, copied and labelled a step's samples + ``prefetch`` ahead of the
    optimiser step.  0: every sample is built inside the step loop on the launch thread (``make_sample``) -- same parameter bits, slower.
    ``cache_labels``: labels generated for a pair (``ssl_label=seflow_auto``) are kept on the host and uploaded again in the later
    epochs instead of being generated again (the reference's job reads labels an offline pass wrote once); same bits.
    ``loss_fn``: "seflowppLoss" (default) or "deflowLoss" = supervised on the frames' ``flow`` (module docstring): ``ssl_label``, the
    feeder options and the label cache are not used, every sample is built inside the step loop (``make_supervised_sample``).

    ``val_metric``: what ``save_top`` ranks by -- "loss" (default: the validation loss, or the mean training loss without a validation
    set) or a flow error of the validation set, "three_way" / "mean_dynamic" (module docstring; ``val_data_name`` "av2" | "scania"
    selects the evaluation mask; works with either ``loss_fn``).  The history entries of such a run gain "val_flow" (the whole results
    dict, accuracy included), "val_figure" and "val_seconds"; a non-finite figure is logged and never kept.  ``val_every``: with a
    validation set only every k-th epoch and the last validate, and only those are offered to ``save_top``; ignored without one.
    Checkpoints written under another metric than the loss carry ``val_metric`` in their extras, and ``resume`` under a different
    metric than the checkpoint's is refused (``TopK`` would rank metres against loss units).

    Ranks (torch.distributed, initialised by the caller / ``distenv.process_group``): step s of an epoch takes the global
    samples [s * batch_size, (s + 1) * batch_size) of that epoch's seeded shuffle; rank r takes every world-th of them.
    ``max_steps`` bounds the optimiser steps of the whole run (tests)."""
    import torch.distributed as dist
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
    if loss_fn not in LOSS_FNS:
        raise ValueError(f"loss_fn={loss_fn!r}: one of {LOSS_FNS}")
    if val_metric not in VAL_METRICS:
        raise ValueError(f"val_metric={val_metric!r}: one of {VAL_METRICS}")
    if val_every < 1:
        raise ValueError(f"val_every={val_every}: at least 1")
    by_flow = val_metric != "loss"
    if by_flow and val_dataset is None:
        raise ValueError(f"val_metric={val_metric!r} needs a validation set (val_dataset) whose frames carry flow, flow_category_indices and gm0")
    if by_flow and val_data_name not in ("av2", "scania"):
        raise ValueError(f"val_data_name {val_data_name!r}: 'av2' or 'scania'")
    if resume is not None:
        from .checkpoint import val_metric_of
        had = val_metric_of(resume)
        if had != val_metric:
            raise ValueError(f"the checkpoint {resume} was ranked by val_metric={had!r}; resuming under val_metric={val_metric!r} would rank "
                             f"its figures against another unit")
    supervised = loss_fn == "deflowLoss"
    if supervised and log is not None and rank == 0:
        log(f"loss_fn=deflowLoss: supervised on the frames' ground-truth flow; ssl_label={ssl_label!r} is ignored")
    # a rank's share of a step's samples goes through the network in ONE pass (BatchNorm statistics over them: torch's semantics
    # for a per-process batch), up to 8 at a time
    per_rank = min(8, max(1, math.ceil(batch_size / world)))
    tr = trainer if trainer is not None else SeFlowTrainer(params, device=device, max_points=max_points, seed=seed, precision=precision,
                                                           batchnorm=batchnorm, batch=per_rank,
                                                           **({"loss": "deflow"} if supervised else {}))
    if supervised != (getattr(tr, "loss_kind", "seflow") == "deflow"):
        raise ValueError(f"loss_fn={loss_fn!r} does not match the loss the trainer was built with")
    dev = tr.device
    start_epoch = 0
    if resume is not None:
        extra = tr.load_checkpoint(resume)
        start_epoch = int(extra.get("epoch", -1)) + 1
    top = TopK(out_dir, k=save_top, resume=resume is not None) if (out_dir is not None and rank == 0) else None
    trips = triplets(dataset)
    if not trips:
        raise ValueError("the dataset has no frame with a successor in its scene")
    val_trips = triplets(val_dataset) if val_dataset is not None else []
    if by_flow and not val_trips:
        raise ValueError("the validation set has no frame with a successor in its scene")
    ckpt_extra = {"val_metric": val_metric} if by_flow else {}
    steps_per_epoch = math.ceil(len(trips) / batch_size)
    history, steps_done = [], 0
    feed_stats = []
    label_caches = {}                                        # per dataset: (i0, i1) -> (label0, label1, n_labels), filled by the first epoch

    def samples_of(ds, groups):
        """one iterator of device samples per group of triplets, in order; the groups' samples are prepared ahead across group
        boundaries (``TrainFeeder``), or built on the spot (``num_workers=0``)"""
        if not groups:
            return
        if supervised:                                       # (no prefetching of supervised samples: module docstring)
            for grp in groups:
                yield (make_supervised_sample(ds, t, dev) for t in grp)
            return
        if num_workers <= 0:
            for grp in groups:
                yield (make_sample(ds, t, dev, ssl_label) for t in grp)
            return
        import itertools
        from ..feeder import TrainFeeder
        # (a step takes its whole share of the batch at once: the NEXT step's samples, and ``prefetch`` more, are prepared under this one)
        feed = TrainFeeder(ds, [t for grp in groups for t in grp], device=dev, label_key=ssl_label, depth=prefetch + max(len(g) for g in groups),
                           workers=num_workers,
                           label_lanes=label_lanes,
                           label_cache=label_caches.setdefault(id(ds), {}) if (cache_labels and ssl_label in AUTO_LABELS) else None)
        try:
            it = iter(feed)
            for grp in groups:
                yield itertools.islice(it, len(grp))
        finally:
            feed.close()
            feed_stats.append(dict(feed.stage_seconds))

    for epoch in range(start_epoch, epochs):
        lr_e = SeFlowTrainer.step_lr(epoch, lr, step_size, gamma)
        order = np.random.default_rng(seed * 1_000_003 + epoch).permutation(len(trips))      # same shuffle on every rank
        n_steps = steps_per_epoch if max_steps is None else max(0, min(steps_per_epoch, max_steps - steps_done))
        # rank r's samples of every step of the epoch (a partial last batch may leave a rank none: it still joins the all-reduce,
        # with zeros)
        mine = [[trips[j] for j in order[s * batch_size:(s + 1) * batch_size][rank::world]] for s in range(n_steps)]
        losses = []
        del feed_stats[:]
        t_epoch = time.perf_counter()
        # the exchange runs under the backward pass when EVERY rank's share of the step fits one pass -- decided from what all ranks
        # know (the step's global sample count and the world size), so that all of them enter the same sequence of collectives
        step_sizes = [len(order[s * batch_size:(s + 1) * batch_size]) for s in range(n_steps)]
        for smp, n_global in zip(samples_of(dataset, mine), step_sizes):
            losses.append(tr.train_batch(smp, lr=lr_e, bucketed=math.ceil(n_global / world) <= tr.B, global_count=n_global))
            steps_done += 1
        train_feed = dict(feed_stats[0]) if feed_stats else None
        train_loss = float(torch.stack(losses).mean().item()) if losses else float("nan")      # (waits for the epoch's last step)
        t_epoch = time.perf_counter() - t_epoch
        tr.sync_running_stats()                              # validation and the checkpoint use rank 0's running statistics
        val_loss = None
        validated = bool(val_trips) and validates(epoch, epochs, val_every)
        if validated and by_flow:
            t_val = time.perf_counter()
            val_flow = validate_flow(tr, val_dataset, val_trips, rank, world, val_data_name)      # (gather() waits for the pass)
            t_val = time.perf_counter() - t_val
        elif validated:
            vals = [tr.loss_only(*smp) for grp in samples_of(val_dataset, [val_trips[rank::world]]) for smp in grp]
            v = torch.stack(vals).sum() if vals else torch.zeros((), dtype=torch.float64, device=dev)
            cnt = torch.tensor([float(len(vals))], dtype=torch.float64, device=dev)
            tot = torch.stack([v.reshape(()), cnt.reshape(())])
            if world > 1:
                dist.all_reduce(tot)
            val_loss = float((tot[0] / tot[1].clamp(min=1.0)).item())
        entry = {"epoch": epoch, "lr": lr_e, "train_loss": train_loss, "val_loss": val_loss, "steps": len(losses),
                 "samples": sum(len(g) for g in mine), "feeder": train_feed, "train_seconds": t_epoch}      # (feeder: host seconds per stage on its own threads)
        line = f"  val loss {val_loss:.6f}" if val_loss is not None else ""
        if validated and by_flow:
            figure = float(val_flow[val_metric])
            entry.update({"val_flow": val_flow, "val_figure": figure, "val_seconds": t_val})
            line = (f"  val three-way {val_flow['three_way']:.6f}  FD {val_flow['FD']:.6f}  FS {val_flow['FS']:.6f}  BS {val_flow['BS']:.6f}"
                    f"  mean_dynamic {val_flow['mean_dynamic']:.6f}  acc_strict ALL {val_flow['acc_strict']['ALL']:.6f}  ({t_val:.2f} s)")
            if not math.isfinite(figure):
                line += f"  [{val_metric} is not finite: nothing of its kind in the validation set; this epoch is not kept]"
        history.append(entry)
        if log is not None and rank == 0:
            log(f"epoch {epoch}: lr {lr_e:.3g}  train loss {train_loss:.6f}" + line)
        if top is not None and losses and (validated or not val_trips):
            if by_flow:
                figure = entry["val_figure"]
            else:
                figure = val_loss if val_loss is not None else train_loss
            top.offer(figure, epoch, tr.export_params(), adam_m=tr.flat_m.cpu().numpy(), adam_v=tr.flat_v.cpu().numpy(), step=tr.step_count,
                      **ckpt_extra)
        if max_steps is not None and steps_done >= max_steps:
            break
    return {"trainer": tr, "history": history, "best": top.best() if top is not None else None}


def _parser():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset_path", required=True)
    ap.add_argument("--val_path", default="")
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--resume", default="")
    ap.add_argument("--out_dir", default="checkpoints")
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--lr", type=float, default=6e-5)
    ap.add_argument("--save_top_model", type=int, default=3)
    ap.add_argument("--batchnorm", default="batch", choices=["batch", "frozen"],
                    help="batch: BatchNorm in training mode (from-scratch training, the reference job); frozen: fine-tuning convention")
    ap.add_argument("--ssl_label", default="seflow_auto",
                    help="seflow_auto (the launcher's +ssl_label=seflow_auto): labels generated on the GPU; or the frame key that holds them")
    ap.add_argument("--loss_fn", default="seflowppLoss", choices=list(LOSS_FNS),
                    help="seflowppLoss: the self-supervised terms; deflowLoss: supervised on the scenes' ground-truth flow (--ssl_label is ignored)")
    ap.add_argument("--num_workers", type=int, default=1,
                    help="reader threads that prepare samples ahead of the step (the launcher's num_workers=16; one thread reads ~3.7 k samples/s from "
                         "warm .h5 files and more of them only contend with the launch thread for the interpreter lock); 0: inside the step loop")
    ap.add_argument("--precision", default="mixed", choices=["mixed", "bf16x3", "f32"])
    ap.add_argument("--max_points", type=int, default=140_000, help="points per sweep the trainer's buffers are sized for")
    ap.add_argument("--val_metric", default="loss", choices=list(VAL_METRICS),
                    help="what --save_top_model ranks by: the validation loss, or a flow error of the validation set (flow metrics, v1; needs "
                         "--val_path scenes with flow, flow_category_indices and gm0)")
    ap.add_argument("--val_every", type=int, default=1, help="validate every N-th epoch and the last (the launcher's val_every=3)")
    ap.add_argument("--data_name", default="auto", choices=["auto", "av2", "scania"],
                    help="the evaluation mask of a flow --val_metric; auto: sniffed from --val_path")
    return ap


def main(argv=None):
    """``python -m himo_amd.seflow.fit --dataset_path <dir> [--checkpoint init.npz] [--out_dir ckpt] [--loss_fn deflowLoss]
    [--val_path <dir> --val_metric three_way --val_every 3]``; under torchrun one rank per GPU (RCCL)."""
    from .. import distenv
    from ..dataset import open_dataset
    from .checkpoint import load_params
    a = _parser().parse_args(argv)
    by_flow = a.val_metric != "loss"
    if by_flow and not a.val_path:
        raise ValueError(f"--val_metric {a.val_metric} needs --val_path")
    data_name = a.data_name
    if data_name == "auto":
        from ..eval_flow import data_name_of
        data_name = data_name_of(a.val_path) if by_flow else "av2"
    with distenv.process_group():
        opts = {"fields": loss_fields(a.loss_fn, a.ssl_label), "zero_copy": True}      # (h5 scene files; the npz container ignores them)
        ds = open_dataset(Path(a.dataset_path), **opts)
        if by_flow:                                          # the union of what the loss and the metric read
            opts = dict(opts, fields=opts["fields"] + tuple(k for k in VAL_FLOW_FIELDS if k not in opts["fields"]))
        val = open_dataset(Path(a.val_path), **opts) if a.val_path else None
        params = load_params(a.checkpoint) if a.checkpoint else None
        return fit(ds, params, out_dir=a.out_dir, epochs=a.epochs, batch_size=a.batch_size, lr=a.lr, save_top=a.save_top_model,
                   val_dataset=val, resume=a.resume or None, batchnorm=a.batchnorm, ssl_label=a.ssl_label, num_workers=a.num_workers,
                   precision=a.precision, loss_fn=a.loss_fn, max_points=a.max_points, val_metric=a.val_metric, val_every=a.val_every,
                   val_data_name=data_name)


if __name__ == "__main__":
    main()
