"""Validation by flow error in the training loop, the parts that need no GPU: the schedule of ``val_every`` as a pure function,
the arguments ``fit`` refuses before it builds a trainer, the program's flags, and the ``val_metric`` extra of the checkpoints."""
import numpy as np
import pytest


def _dataset(n=3):
    from himo_amd.dataset import ListDataset
    from himo_amd.synthetic import make_scene
    return ListDataset(make_scene(3, n, n_points=200, scene_id="valcpu", n_instances=2))


def test_validation_schedule_is_every_kth_epoch_and_the_last():
    from himo_amd.seflow.fit import validates, validation_epochs
    assert validation_epochs(12, 3) == [2, 5, 8, 11]             # the launcher's val_every=3 over its 12 epochs
    assert validation_epochs(3, 2) == [1, 2]                     # ... and the last epoch whatever k
    assert validation_epochs(4, 1) == [0, 1, 2, 3]               # the default: every epoch, as before
    assert validation_epochs(5, 7) == [4]
    assert validation_epochs(12, 3, start_epoch=6) == [8, 11]    # a resumed run keeps the schedule of the whole run
    assert validates(2, 12, 3) and not validates(3, 12, 3) and validates(11, 12, 5)
    for k in (0, -1):
        with pytest.raises(ValueError, match="val_every"):
            validation_epochs(3, k)


def test_fit_refuses_bad_validation_arguments_before_it_builds_a_trainer():
    from himo_amd.seflow.fit import VAL_METRICS, fit
    assert VAL_METRICS == ("loss", "three_way", "mean_dynamic")
    ds = _dataset()
    with pytest.raises(ValueError, match="bogus"):
        fit(ds, epochs=1, val_metric="bogus", log=None)
    with pytest.raises(ValueError, match="val_every"):
        fit(ds, epochs=1, val_every=0, log=None)
    for metric in ("three_way", "mean_dynamic"):
        with pytest.raises(ValueError, match="validation set"):
            fit(ds, epochs=1, val_metric=metric, log=None)       # a flow metric without a validation set
    with pytest.raises(ValueError, match="val_data_name"):
        fit(ds, epochs=1, val_metric="three_way", val_dataset=ds, val_data_name="kitti", log=None)


def test_parser_has_the_validation_flags():
    from himo_amd.seflow.fit import _parser
    a = _parser().parse_args(["--dataset_path", "d"])
    assert (a.val_metric, a.val_every, a.data_name) == ("loss", 1, "auto")           # nothing changes unasked
    a = _parser().parse_args(["--dataset_path", "d", "--val_path", "v", "--val_metric", "mean_dynamic", "--val_every", "3", "--data_name", "scania"])
    assert (a.val_metric, a.val_every, a.data_name, a.val_path) == ("mean_dynamic", 3, "scania", "v")
    for bad in (["--val_metric", "epe"], ["--data_name", "kitti"], ["--val_every", "often"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(["--dataset_path", "d"] + bad)


def test_program_refuses_a_flow_metric_without_a_validation_path():
    from himo_amd.seflow.fit import main
    with pytest.raises(ValueError, match="val_path"):
        main(["--dataset_path", "d", "--val_metric", "three_way"])


def test_validation_fields_are_the_union_with_the_losses():
    from himo_amd.seflow.fit import VAL_FLOW_FIELDS, loss_fields
    for key in ("flow", "flow_category_indices", "gm0", "flow_is_valid", "pc0", "pc1", "pose0", "pose1"):
        assert key in VAL_FLOW_FIELDS
    assert "flow_category_indices" not in loss_fields("seflowppLoss") and "flow_category_indices" not in loss_fields("deflowLoss")


def test_checkpoints_name_their_metric_and_resume_under_another_is_refused(tmp_path):
    from himo_amd.seflow import spec
    from himo_amd.seflow.checkpoint import TopK, load_params, save_params, val_metric_of
    from himo_amd.seflow.fit import fit
    params = spec.init_params(5)
    plain = save_params(tmp_path / "plain.npz", params, epoch=0, val=0.5)
    assert val_metric_of(plain) == "loss"                        # an absent extra means the loss
    top = TopK(tmp_path / "kept", k=1)
    path = top.offer(0.25, 1, params, val_metric="three_way")
    _, extra = load_params(path, with_extra=True)
    assert str(extra["val_metric"]) == "three_way" and float(extra["val"]) == 0.25 and val_metric_of(path) == "three_way"
    assert top.offer(float("nan"), 2, params, val_metric="three_way") is None        # a non-finite figure is never kept
    ds = _dataset()
    with pytest.raises(ValueError, match="three_way"):
        fit(ds, epochs=3, resume=path, log=None)                                     # metres against loss units
    with pytest.raises(ValueError, match="mean_dynamic"):
        fit(ds, epochs=3, resume=path, val_metric="mean_dynamic", val_dataset=ds, log=None)
    with pytest.raises(ValueError, match="loss"):
        fit(ds, epochs=3, resume=plain, val_metric="three_way", val_dataset=ds, log=None)
    assert np.isfinite(load_params(path)["enc1.0.weight"]).all()
