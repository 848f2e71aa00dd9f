"""The host scaffolding the dataset programs share (himo_amd/sweeps.py): packing, sharding, the fed loop, the missing-key
protocol, the drain ladder and the Feather file sink.  No GPU: ``upload`` is a numpy concatenation that returns CPU tensors."""
import threading

import numpy as np
import pytest
import torch

from himo_amd import distenv, sweeps
from himo_amd.eval_seg import as_labels_u8


def cpu_upload(parts, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(p) for p in parts], axis=0).astype(dtype)))


def _frames(counts=(5, 0, 7)):
    rng = np.random.default_rng(3)
    out = []
    for k, n in enumerate(counts):
        out.append({"scene_id": f"scene{k}", "timestamp": 1000 + k, "pc0": rng.normal(size=(n, 4)).astype(np.float32),
                    "flow": rng.normal(size=(n, 3)).astype(np.float64), "lidar_dt": rng.random(n).astype(np.float32),
                    "labels": rng.integers(-3, 300, n).astype(np.int64), "pose0": rng.normal(size=(4, 4)).astype(np.float32)})
    return out


def test_packer_lays_three_sweeps_end_to_end():
    frames = _frames()
    p = sweeps.SweepPacker(iter(frames), cpu_upload)
    assert p.offsets_host.dtype == np.int64 and p.offsets_host.tolist() == [0, 5, 5, 12]
    assert p.offsets.dtype == torch.int64 and p.offsets.tolist() == [0, 5, 5, 12]
    assert sweeps.sweep_offsets([5, 0, 7]).tolist() == [0, 5, 5, 12] and sweeps.sweep_offsets([]).tolist() == [0]
    for key, dtype, width in (("pc0", np.float32, 4), ("flow", np.float32, 3), ("lidar_dt", np.float32, None), ("labels", np.int32, None)):
        got = p.cat(key, dtype, width)
        assert np.array_equal(got.numpy(), np.concatenate([f[key] for f in frames]).astype(dtype)) and got.numpy().dtype == dtype
    got = p.cat("labels", np.uint8, labels=True)
    assert np.array_equal(got.numpy(), np.concatenate([as_labels_u8(f["labels"]) for f in frames]))
    poses = p.stack("pose0", np.float64)
    assert poses.dtype == torch.float64 and np.array_equal(poses.numpy(), np.stack([f["pose0"] for f in frames]).astype(np.float64))


def test_packer_names_scene_timestamp_and_key_of_a_misshapen_array():
    frames = _frames()
    frames[2]["lidar_dt"] = frames[2]["lidar_dt"][:-1]                # a wrong row count
    frames[0]["flow"] = np.zeros((5, 2), np.float32)                  # a wrong width
    p = sweeps.SweepPacker(frames, cpu_upload)
    with pytest.raises(ValueError, match=r"scene2 at 1002: lidar_dt has shape \(6,\) for a sweep of 7 points"):
        p.cat("lidar_dt", np.float32)
    with pytest.raises(ValueError, match=r"scene0 at 1000: flow has shape \(5, 2\) for a sweep of 5 points"):
        p.cat("flow", np.float32, 3)
    with pytest.raises(KeyError, match="no_such_key"):
        p.cat("no_such_key", np.float32)
    with pytest.raises(KeyError, match="no_such_key"):
        sweeps.SweepPacker(frames, cpu_upload, count_key="no_such_key")
    with pytest.raises(ValueError, match="^empty batch$"):
        sweeps.SweepPacker([], cpu_upload)


def test_sharded_batches_deal_item_i_to_rank_i_mod_world(monkeypatch):
    items = list("abcdefg")
    monkeypatch.setattr(distenv, "rank_world", lambda: (0, 2))
    assert sweeps.sharded_batches(items, 3) == [[0, 2, 4], [6]]
    monkeypatch.setattr(distenv, "rank_world", lambda: (1, 2))
    assert sweeps.sharded_batches(items, 3) == [[1, 3, 5]]
    monkeypatch.undo()
    assert distenv.rank_world() == (0, 1)                             # no process group here
    assert sweeps.sharded_batches(items, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert list(sweeps.sharded_batches([], 3)) == []


def test_fed_without_overlap_builds_in_order_on_the_calling_thread():
    seen = []

    def build(item, upload):
        assert upload is None and threading.current_thread() is threading.main_thread()
        seen.append(item)
        return item * 10
    assert list(sweeps.fed(iter(range(3)), build, overlap=False)) == [0, 10, 20] and seen == [0, 1, 2]

    def source():
        yield 0
        yield 1
        raise OSError("item 2 cannot be read")
    got = []
    with pytest.raises(OSError, match="item 2 cannot be read"):
        for obj in sweeps.fed(source(), build, overlap=False):
            got.append(obj)
    assert got == [0, 10]


def test_missing_key_prints_its_lines_then_raises_a_bare_key_error(capsys):
    def source():
        yield "batch 0", ["line a"]
        raise sweeps.MissingKey("seg_valid", ["line b", "line c"])
    with pytest.raises(KeyError) as caught:
        try:
            for _, lines in sweeps.fed(source(), lambda item, upload: item, overlap=False):
                for line in lines:
                    print(line)
        except sweeps.MissingKey as e:
            sweeps.raise_missing(e)
    assert caught.value.args == ("seg_valid",) and caught.value.__cause__ is None and caught.value.__suppress_context__
    assert capsys.readouterr().out == "line a\nline b\nline c\n"


class _Closes:
    def __init__(self, log, name, error=None):
        self.log, self.name, self.error = log, name, error

    def close(self):
        self.log.append(self.name)
        if self.error is not None:
            raise self.error


def test_draining_closes_the_feed_then_the_drain_and_keeps_the_first_error():
    log = []
    with pytest.raises(RuntimeError, match="consumer"):
        with sweeps.draining(_Closes(log, "feed"), _Closes(log, "drain", OSError("disk full"))):
            raise RuntimeError("consumer")
    assert log == ["feed", "drain"]                                    # the drain's own error is dropped
    log.clear()
    with pytest.raises(OSError, match="disk full"):
        with sweeps.draining(_Closes(log, "feed"), _Closes(log, "drain", OSError("disk full"))):
            pass
    assert log == ["drain"]                                            # a loop that ended: the drain's error surfaces
    log.clear()
    with sweeps.draining(_Closes(log, "feed"), None):                  # the serial loop has no drain
        pass
    with pytest.raises(KeyboardInterrupt):
        with sweeps.draining(_Closes(log, "feed"), None):
            raise KeyboardInterrupt
    assert log == ["feed"]


def test_feather_sink_from_four_threads(tmp_path):
    sink = sweeps.FeatherSink(tmp_path / "out")
    jobs = [(f"scene{s}", str(100 + t), [bytes([s, t]) * 3, memoryview(np.full(5, 7 * s + t, np.uint8)), b"tail"]) for s in range(2) for t in range(3)]
    errors = []

    def work(mine):
        try:
            for scene, stamp, buffers in mine:
                sink.write(scene, stamp, buffers)
        except BaseException as e:
            errors.append(e)
    threads = [threading.Thread(target=work, args=(jobs[k::4],)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    files = sorted(p.relative_to(tmp_path / "out").as_posix() for p in (tmp_path / "out").rglob("*.feather"))
    assert files == sorted(f"{scene}/{stamp}.feather" for scene, stamp, _ in jobs) and len(files) == 6
    for scene, stamp, buffers in jobs:
        assert (tmp_path / "out" / scene / f"{stamp}.feather").read_bytes() == b"".join(bytes(b) for b in buffers)
