"""The shared packer and fed loop on the device (himo_amd/sweeps.py): a batch staged by the real ``feeder.BatchFeeder`` holds the
very bits of the same batch packed with ``host_upload``, for every batch class of the dataset programs; and the fed loop leaves no
feeder thread behind when its source fails."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (1, 64, 65)


def _frames(counts=COUNTS):
    from himo_amd.synthetic import make_frame
    frames = [make_frame(40 + k, n_points=n, scene_id="s") for k, n in enumerate(counts)]
    rng = np.random.default_rng(9)
    for f in frames:
        n = len(f["pc0"])
        f["seg_valid"] = rng.random(n) > 0.3
        f["seg_raw"] = rng.integers(0, 3, n).astype(np.uint8)
        f["seg_flow"] = rng.integers(-2, 300, n).astype(np.int64)           # cast on the host: outside 0..255 -> 0
    return frames


def _label_sweeps(frames, boxes=(2, 0, 3)):
    rng = np.random.default_rng(5)
    return [(f["pc0"], np.linalg.inv(f["pose1"]) @ f["pose0"],
             (rng.normal(size=(m, 8)), rng.normal(size=(m, 3)).astype(np.float32), rng.integers(0, 30, m).astype(np.uint8),
              rng.integers(0, 2, m).astype(np.uint8))) for f, m in zip(frames, boxes)]


def _tensors(obj) -> dict:
    out = {}
    for name, v in vars(obj).items():
        for k, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(t, torch.Tensor):
                out[f"{name}[{k}]"] = t
    return out


def _cases(gpu):
    from himo_amd.compdis import FrameBatch
    from himo_amd.eval_flow import FlowBatch
    from himo_amd.eval_seg import SegBatch
    from himo_amd.extract_sca import GroundBatch, LabelBatch
    frames = _frames()
    sweeps = _label_sweeps(frames)
    return {
        "FrameBatch": (lambda up: FrameBatch.from_frames(frames, "seflowpp_best", device=gpu, with_masks=True, upload=up, with_labels=True)),
        "FrameBatch host_ego": (lambda up: FrameBatch.from_frames(frames, "flow", device=gpu, upload=up, with_labels=True, host_ego=True)),
        "FlowBatch": (lambda up: FlowBatch.from_frames(frames, ["seflowpp_best", "raw"], device=gpu, upload=up, keys=[7, 8, 9])),
        "SegBatch": (lambda up: SegBatch.from_frames(_frames(COUNTS + (0,)), ["seg_raw", "seg_flow"], device=gpu, upload=up)),
        "LabelBatch": (lambda up: LabelBatch(sweeps, 0, device=gpu, upload=up)),
        "GroundBatch": (lambda up: GroundBatch([f["pc0"] for f in frames], None, device=gpu, upload=up)),
    }


@pytest.mark.parametrize("name", ["FrameBatch", "FrameBatch host_ego", "FlowBatch", "SegBatch", "LabelBatch", "GroundBatch"])
def test_a_fed_batch_holds_the_bits_of_the_host_uploaded_one(gpu, name):
    from himo_amd.feeder import BatchFeeder
    from himo_amd.sweeps import host_upload
    pack = _cases(gpu)[name]
    calls = []

    def counting(parts, dtype):
        calls.append(len(parts))
        return host_upload(gpu)(parts, dtype)
    want = pack(counting)
    fed = list(BatchFeeder(iter([None]), lambda item, upload: pack(upload), device=gpu))
    torch.cuda.synchronize()
    assert len(fed) == 1 and type(fed[0]) is type(want)
    a, b = _tensors(want), _tensors(fed[0])
    assert list(a) == list(b) and len({id(t) for t in a.values()}) == len(calls) > 0      # one upload call per device tensor
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and b[key].device == a[key].device, key
        assert torch.equal(a[key], b[key]), key
    for key, v in vars(want).items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, vars(fed[0])[key]), key


def test_fed_with_overlap_delivers_what_came_before_a_failing_source_and_leaves_no_thread(gpu):
    from himo_amd.compdis import FrameBatch
    from himo_amd.sweeps import fed
    frames = _frames()

    def source():
        yield frames[:2]
        yield frames[2:]
        raise OSError("batch 2 cannot be read")
    got = []
    with pytest.raises(OSError, match="batch 2 cannot be read"):
        for batch in fed(source(), lambda item, upload: FrameBatch.from_frames(item, "raw", device=gpu, upload=upload), device=gpu, overlap=True):
            got.append(batch.offsets_host.tolist())
    assert got == [[0, 1, 65], [0, 65]]
    assert not [t for t in threading.enumerate() if t.name == "himo-batch-feeder" and t.is_alive()]
    feed = fed(iter([frames]), lambda item, upload: FrameBatch.from_frames(item, "raw", device=gpu, upload=upload), device=gpu, overlap=True)
    assert next(feed).n_frames == 3
    feed.close()                                                          # a consumer that gives up early
    assert not [t for t in threading.enumerate() if t.name == "himo-batch-feeder" and t.is_alive()]
    torch.cuda.synchronize()
