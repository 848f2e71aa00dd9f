"""Validation by flow error inside the training loop: ``fit(val_metric="three_way" | "mean_dynamic", val_every=k)`` and the program
``python -m himo_amd.seflow.fit --val_metric ... --val_every ...``.  Small sweeps (max_points <= 6 000): these tests pin the
plumbing -- the epoch's figure is the flow error of the trainer's own inference output under "flow metrics, v1" in residual mode
(recomputed by hand through tests/flowaccuracy_ref.py), the schedule, the checkpoints' extras -- not a trained network's accuracy."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))

import flowaccuracy_ref as acc  # noqa: E402
import flowmetrics_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _by_hand(tr, val, gpu):
    """the validation figures of the trainer as it stands: one inference pass per validation triplet, RES to the host, the
    restatement in residual mode -> (means of rules 7 and 8, counted points, accuracy table [4][3])"""
    from himo_amd.seflow.fit import make_validation_sample, triplets
    frames = []
    for trip in triplets(val):
        fwd = make_validation_sample(val, trip, gpu)[0]
        res = tr.forward(*fwd, training=False)
        n0 = tr.n_pts_b[0][1]
        assert res.shape == (n0, 4) and res.stride(0) == 4
        dropped = tr.net._pt[0]["pid"][1][:n0] < 0
        # rows of points the pillar stage dropped: the fused head leaves zeros there, so they enter as a zero residual
        assert (res[dropped] == 0).all() and (res[:, 3] == 0).all()
        print(f"validation pass: {int(dropped.sum())} of {n0} rows dropped by the pillar stage, all zero")
        frames.append(dict(val[trip[1]], res=res[:, :3].cpu().numpy()))
    buckets, threeway, rejected, table = acc.flow_accuracy_ref(frames, ["res"], "av2", residual=True)
    assert rejected[0] == 0
    means = ref.means_ref(buckets[0], threeway[:, 0])
    counted = int(buckets[0, 0, :, 0].sum() + threeway[:, 0, :2, 0].sum())
    return means, counted, table[0]


@pytest.mark.parametrize("loss_fn", ["seflowppLoss", "deflowLoss"])
def test_fit_ranks_its_checkpoints_by_the_flow_error_of_its_own_output(gpu, tmp_path, loss_fn):
    from himo_amd.dataset import ListDataset
    from himo_amd.seflow import spec
    from himo_amd.seflow.checkpoint import load_params
    from himo_amd.seflow.fit import fit
    from himo_amd.synthetic import make_scene
    frames = make_scene(47, 5, n_points=5_000, scene_id="valfit")
    for f in frames:                                             # make_scene alone leaves FS empty: every 4th background row becomes a car
        cat = np.array(f["flow_category_indices"])
        cat[np.flatnonzero(cat == 0)[::4]] = 19
        f["flow_category_indices"] = cat
    val = ListDataset(frames[:3])
    logs = []
    out = fit(ListDataset(frames), spec.init_params(27), out_dir=tmp_path, epochs=2, batch_size=2, lr=2e-4, save_top=1, max_points=6_000,
              device=gpu, log=logs.append, loss_fn=loss_fn, ssl_label="flow_instance_id", val_dataset=val, val_metric="three_way")
    hist = out["history"]
    assert len(hist) == 2
    for e in hist:
        assert e["val_figure"] == e["val_flow"]["three_way"] and np.isfinite(e["val_seconds"]) and e["val_seconds"] > 0
        assert e["val_loss"] is None and set(e["val_flow"]["acc_strict"]) == {"ALL", "FD", "FS", "BS"}
    lines = [line for line in logs if line.startswith("epoch ")]
    assert len(lines) == 2 and all("three-way" in line and "mean_dynamic" in line and "acc_strict ALL" in line for line in lines)
    print("\n".join(lines))
    # the last epoch's figures, by hand
    means, counted, table = _by_hand(out["trainer"], val, gpu)
    got = hist[-1]["val_flow"]
    assert got["counted"] == counted and got["rejected"] == 0
    for key in ("three_way", "FD", "FS", "BS"):
        print(f"{key}: fit {got[key]!r}, by hand {means[key]!r}, difference {abs(got[key] - means[key]):.3g}")
        assert (np.isnan(got[key]) and np.isnan(means[key])) or abs(got[key] - means[key]) <= 2.0 ** -23
    assert all(np.isfinite(e["val_figure"]) for e in hist)       # FD, FS and BS are all populated
    strict, relaxed = acc.accuracy_means(table)
    print("acc_strict", got["acc_strict"], "by hand", strict)
    # the kept checkpoint: the smallest figure, and it names its metric
    kept = sorted(tmp_path.glob("*.npz"))
    assert len(kept) == 1
    _, extra = load_params(kept[0], with_extra=True)
    assert float(extra["val"]) == min(e["val_figure"] for e in hist) and str(extra["val_metric"]) == "three_way"
    if loss_fn != "seflowppLoss":
        return
    # val_every=2 over 3 epochs: epochs 1 and 2 validate, two checkpoints at most are offered
    out2 = fit(ListDataset(frames), trainer=out["trainer"], out_dir=tmp_path / "every2", epochs=3, batch_size=2, lr=2e-4, save_top=3, device=gpu,
               log=None, ssl_label="flow_instance_id", val_dataset=val, val_metric="mean_dynamic", val_every=2)
    h2 = out2["history"]
    assert ["val_flow" in e for e in h2] == [False, True, True] and "val_figure" not in h2[0] and "val_seconds" not in h2[0]
    assert all(e["val_figure"] == e["val_flow"]["mean_dynamic"] for e in h2[1:])
    kept2 = sorted((tmp_path / "every2").glob("*.npz"))
    assert len(kept2) <= 2 and all("epoch00" not in p.name for p in kept2)
    assert len(kept2) == sum(np.isfinite(e["val_figure"]) for e in h2[1:])
    # a validation set without flow is a KeyError naming it
    no_flow = ListDataset([{k: v for k, v in f.items() if k != "flow"} for f in frames[:3]])
    with pytest.raises(KeyError, match="flow"):
        fit(ListDataset(frames), trainer=out["trainer"], epochs=1, batch_size=2, max_steps=1, device=gpu, log=None, ssl_label="flow_instance_id",
            val_dataset=no_flow, val_metric="three_way")


def test_fit_program_validates_by_flow_error_over_h5_scene_files(gpu, tmp_path):
    """``python -m himo_amd.seflow.fit --val_path V --val_metric mean_dynamic --val_every 2 --epochs 2`` as a PROGRAM over two tiny
    ``.h5`` scenes: the validation set opened with the union of the loss's fields and the metric's, one validation line (after
    the last epoch), one checkpoint whose extras name the metric."""
    import os, subprocess
    from himo_amd.seflow.checkpoint import load_params
    from himo_amd.synthetic import make_scene, write_h5_scenes
    data = tmp_path / "scenes_av2"                               # (--data_name auto sniffs the name from the path)
    data.mkdir()
    write_h5_scenes(data, [make_scene(85 + sc, 3, n_points=3_000, scene_id=f"h5val{sc}") for sc in range(2)])     # 2 usable sweeps each
    env = dict(os.environ, PYTHONPATH=str(REPO))
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, "-m", "himo_amd.seflow.fit", "--dataset_path", str(data), "--val_path", str(data), "--out_dir", str(tmp_path / "ckpt"),
           "--epochs", "2", "--batch_size", "2", "--save_top_model", "1", "--max_points", "4000", "--val_metric", "mean_dynamic", "--val_every", "2"]
    out = subprocess.run(cmd, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    print(out.stdout)
    assert out.stdout.count("epoch ") == 2 and out.stdout.count("three-way") == 1
    kept = sorted((tmp_path / "ckpt").glob("*.npz"))
    assert len(kept) == 1 and "epoch01" in kept[0].name
    params, extra = load_params(kept[0], with_extra=True)
    assert str(extra["val_metric"]) == "mean_dynamic" and np.isfinite(float(extra["val"])) and np.isfinite(params["enc1.0.weight"]).all()
