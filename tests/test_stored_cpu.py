"""The layer the box / track programs share (``himo_amd.stored``, the scene sharding of ``himo_amd.sweeps``, ``distenv.run_shard`` with
``closing=``, ``distenv.add_sums`` / ``gathered``): host logic only, no GPU.  The refusal texts are the programs' own, copied from
where they were written out before this layer existed."""
import copy
import json
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = Path(__file__).resolve().parents[1]


# ---- sharding ----------------------------------------------------------------------------------------------------------------------------
class _Index:
    """3 scenes of 4, 1 and 3 sweeps, interleaved: index order is not scene order"""

    def __init__(self):
        self.index = [[s, str(100 + n)] for n, s in enumerate(["a", "b", "a", "c", "a", "c", "c", "a"])]

    def __len__(self):
        return len(self.index)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_sharding_partitions_the_index_by_whole_scenes(world, monkeypatch):
    from himo_amd import distenv, sweeps
    ds = _Index()
    assert sweeps.scene_items(ds) == {"a": [0, 2, 4, 7], "b": [1], "c": [3, 5, 6]}
    scenes, whole, single = [], [], []
    for rank in range(world):
        monkeypatch.setattr(distenv, "rank_world", lambda rank=rank: (rank, world))
        mine = sweeps.sharded_scenes(ds)
        items = sweeps.sharded_items(ds, whole_scenes=True)
        assert items == sorted(i for _, part in mine for i in part)           # the same share, in index order
        assert all(part == sorted(part) for _, part in mine)
        assert {ds.index[i][0] for i in items} == {s for s, _ in mine}
        assert sweeps.sharded_items(ds, whole_scenes=False) == list(range(rank, len(ds), world))
        scenes.append([s for s, _ in mine])
        whole.append(items)
        single.append(sweeps.sharded_items(ds, whole_scenes=False))
    assert sorted(s for part in scenes for s in part) == ["a", "b", "c"]      # no scene on two ranks, none left out
    assert sorted(i for part in whole for i in part) == list(range(len(ds)))
    assert sorted(i for part in single for i in part) == list(range(len(ds)))
    assert scenes[0][0] == "a" and (world < 4 or whole[3] == [])              # scene n goes to rank n % world; world 4 leaves a rank empty


# ---- scene files -------------------------------------------------------------------------------------------------------------------------
def _hdf5_or_skip():
    from himo_amd.save import h5_writer
    mod, how = h5_writer()
    if mod is None:
        pytest.skip(how)
    return mod, how


def _write_scenes(root):
    from himo_amd import h5lite
    trees = {}
    for sc in ("s0", "s1"):
        rng = np.random.default_rng(len(trees))
        trees[sc] = {ts: {"lidar": rng.normal(size=(5, 4)).astype(np.float32), "foreign": rng.integers(0, 9, 7).astype(np.uint16)}
                     for ts in ("10", "20")}
        h5lite.write_file(Path(root) / f"{sc}.h5", trees[sc])
    return trees


class _FakeScenes:
    """what ``KeySink`` asks of a scene-file dataset, with the calls written down"""

    def __init__(self, root, log):
        self.root, self.log = Path(root), log

    def forget(self, scene):
        self.log.append(("forget", scene))

    def scene_path(self, scene):
        return self.root / f"{scene}.h5"


def test_put_keys_and_keysink_on_scene_files(tmp_path, monkeypatch):
    from himo_amd import h5lite, save, stored
    mod, how = _hdf5_or_skip()
    trees = _write_scenes(tmp_path)
    log = []

    class Recorder:
        @staticmethod
        def File(path, mode):
            log.append(("open", Path(path).stem, mode))
            return mod.File(path, mode)

    monkeypatch.setattr(save, "h5_writer", lambda: (Recorder, how))
    ids = np.array([3, -1, 7], dtype=np.int32)
    none = np.zeros((0, 6), dtype=np.float64)
    flags = np.array([True, False, True, True])
    sink = stored.KeySink(_FakeScenes(tmp_path, log), tmp_path)
    for sc in ("s0", "s1"):
        for ts in ("10", 20):                                                 # a time stamp may come as an int
            sink.put(sc, ts, "ids", ids)
            sink.put(sc, ts, "rows", none)
            sink.put(sc, ts, "flags", flags)
        assert ("open", sc, "a") not in log                                   # held back until the scene is done
    sink.close()
    sink.close()                                                              # (nothing left: no further open)
    assert log == [("forget", "s0"), ("open", "s0", "a"), ("forget", "s1"), ("open", "s1", "a")]
    # the same key again, with another shape: replaced
    again = np.arange(10, dtype=np.int32).reshape(5, 2)
    with mod.File(tmp_path / "s0.h5", "a") as h:
        stored.put_keys(h, "10", {"ids": again})
    for sc, tree in trees.items():
        with h5lite.File(tmp_path / f"{sc}.h5") as f:
            for ts, group in tree.items():
                g = f[ts]
                assert sorted(g.keys()) == sorted(list(group) + ["ids", "rows", "flags"])
                want = again if (sc, ts) == ("s0", "10") else ids
                assert g["ids"].dtype == np.int32 and g["ids"].shape == want.shape and np.array_equal(g["ids"][:], want)
                assert g["rows"].dtype == np.float64 and g["rows"].shape == (0, 6)
                assert g["flags"].dtype == np.dtype(bool) and np.array_equal(g["flags"][:], flags)
                for name, a in group.items():                                 # the foreign datasets are untouched
                    b = g[name][:]
                    assert b.dtype == a.dtype and b.tobytes() == np.ascontiguousarray(a).tobytes(), (sc, ts, name)


def test_h5_module_refuses_in_the_programs_words(tmp_path, monkeypatch):
    from himo_amd import save, stored
    monkeypatch.setattr(save, "h5_writer", lambda: (None, "no HDF5 library"))
    want = ("writing 'boxes_x' into the scene files of D needs an HDF5 library (h5py, or libhdf5 for himo_amd.h5c; HIMO_LIBHDF5 names one): "
            "no HDF5 library")
    with pytest.raises(RuntimeError) as e:
        stored.h5_module("writing 'boxes_x' into the scene files of D")
    assert str(e.value) == want
    with pytest.raises(RuntimeError) as e:
        stored.KeySink(_FakeScenes(tmp_path, []), tmp_path, "writing 'boxes_x' into the scene files of D")
    assert str(e.value) == want
    assert list(tmp_path.iterdir()) == []


# ---- the npz container -------------------------------------------------------------------------------------------------------------------
def test_put_npz_keeps_dtypes_and_the_other_arrays(tmp_path):
    from himo_amd import save, stored
    from himo_amd.dataset import NpzDataset
    pc0 = np.arange(12, dtype=np.float32).reshape(4, 3)
    frame = {"scene_id": "s", "timestamp": 5, "pc0": pc0, "lidar_id": np.arange(4, dtype=np.uint8)}
    NpzDataset.write(tmp_path, [frame])
    put = {"ids": np.array([1, 2, 3, 4], dtype=np.int32), "rows": np.zeros((0, 6), dtype=np.float64), "flags": np.array([True, False])}
    stored.put_npz(tmp_path, "s", 5, put)
    save.NpzResultSink(tmp_path, "flow64")(0, frame, np.ones((4, 3), dtype=np.float64))
    sink = stored.KeySink(NpzDataset(tmp_path), tmp_path)                      # the npz container: written at once, nothing to close
    sink.put("s", 5, "late", np.array([9], dtype=np.int64))
    with np.load(tmp_path / "s" / "5.npz") as z:
        assert sorted(z.files) == sorted(["pc0", "lidar_id", "flow64", "late"] + list(put))
        for k, a in put.items():
            assert z[k].dtype == a.dtype and z[k].shape == a.shape and np.array_equal(z[k], a)
        assert z["pc0"].dtype == np.float32 and z["pc0"].tobytes() == pc0.tobytes() and z["lidar_id"].dtype == np.uint8
        assert z["flow64"].dtype == np.float32 and np.array_equal(z["flow64"], np.ones((4, 3), np.float32))      # the flow sink stores float32
        assert z["late"].dtype == np.int64
    assert not list(tmp_path.rglob("*.writing.npz"))
    ds = NpzDataset(tmp_path)
    assert stored.present(ds, 0, ["ids", "nope", "pc0"]) == {"ids", "pc0"}
    got = stored.arrays(ds, 0, ["ids", "nope"])
    assert list(got) == ["ids"] and got["ids"].dtype == np.int32


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_validators_raise_the_programs_texts():
    from himo_amd import stored
    says = lambda text: pytest.raises(ValueError, match="^" + __import__("re").escape(text) + "$")      # noqa: E731
    with says("res_names='a,,a': one or more different names"):
        stored.result_names("a,,a", raw_ok=False)
    with says("res_names=[]: one or more different names ('raw' = the points as recorded)"):
        stored.result_names([], raw_ok=True)
    assert stored.result_names("raw,,flow", raw_ok=True) == ["raw", "flow"] and stored.result_names(("a", "b"), raw_ok=False) == ["a", "b"]
    with says("boxes_x: s/1 holds float64 (2, 12), not float32 [F][12] box rows"):
        stored.check_box_rows(np.zeros((2, 12)), "boxes_x", "s/1", 4)
    with says("boxes_x: s/1 holds 3 boxes: at most 2 per sweep"):
        stored.check_box_rows(np.zeros((3, 12), np.float32), "boxes_x", "s/1", 2)
    stored.check_box_rows(np.zeros((0, 12), np.float32), "boxes_x", "s/1", 2)
    b = np.zeros((2, 12), np.float32)
    with says("tracks_x: s/1 holds float32 (2, 6), not float64 [F][6] track rows"):
        stored.check_track_rows(np.zeros((2, 6), np.float32), b, "tracks_x", "boxes_x", "s/1", "python -m himo_amd.track --res_names x --overwrite")
    with says("tracks_x: s/1 holds 1 rows for the 2 boxes of boxes_x: stale tracks (run `python -m himo_amd.track --res_names x --overwrite` "
              "after box_fit)"):
        stored.check_track_rows(np.zeros((1, 6)), b, "tracks_x", "boxes_x", "s/1", "python -m himo_amd.track --res_names x --overwrite")
    with says("ray_label: s/1 holds float32 (5,), not one integer per point of its 5 points"):
        stored.check_point_labels(np.zeros(5, np.float32), "ray_label", "s/1", rows=5)
    with says("ray_label: s/1 holds int32 (5, 1), not one integer per point"):
        stored.check_point_labels(np.zeros((5, 1), np.int32), "ray_label", "s/1")
    with says("ray_label: s/1 holds uint32 (4,), not one integer per point of its 5 points"):
        stored.check_point_labels(np.zeros(4, np.uint32), "ray_label", "s/1", rows=5)
    stored.check_point_labels(np.zeros(4, np.uint32), "ray_label", "s/1")
    with says("pose0: s/1 holds no [4, 4] pose"):
        stored.check_pose({"pose0": np.eye(3)}, "s/1")
    with says("pose0: s/1 holds no [4, 4] pose"):
        stored.check_pose({}, "s/1")
    with says("batch=0: at least 1 sweep per launch"):
        stored.at_least_one("batch", 0, " sweep per launch")
    with says("min_hits=True: at least 1"):
        stored.at_least_one("min_hits", True)
    with says("sweeps_per_launch=2.0: at least 1"):
        stored.at_least_one("sweeps_per_launch", 2.0)
    with says("motion_min=-0.5: finite and >= 0"):
        stored.check_motion_min(-0.5)
    with says("motion_min=nan: finite and >= 0"):
        stored.check_motion_min(float("nan"))
    stored.check_motion_min(0.0)
    assert (stored.fmt(None), stored.fmt(0.25), stored.fmt(0.25, ".1f"), stored.ratio(1, 0), stored.ratio(1, 4)) == ("-", "0.250", "0.2", None, 0.25)


# ---- the ranks' sums ---------------------------------------------------------------------------------------------------------------------
def _doubled(v):
    return {k: _doubled(x) for k, x in v.items()} if isinstance(v, dict) else [2 * x for x in v] if isinstance(v, list) else None if v is None else 2 * v


def test_add_sums_over_the_programs_structures():
    from himo_amd import eval_box, eval_xsensor, track
    from himo_amd.distenv import add_sums
    box = {"x": eval_box.new_sums()}
    b = box["x"]["buckets"]["all"]
    box["x"]["pred"], b["gt"], b["sum_iou"], b["tp"], b["shape"]["sum_dl"] = 5, 4, 1.5, [3, 2, 1], 0.25
    assert add_sums(box, copy.deepcopy(box)) == _doubled(box) and add_sums(box, box)["x"]["buckets"]["all"]["tp"] == [6, 4, 2]
    for against in (None, {"x": eval_xsensor.new_against(True)}):
        xs = {"totals": {"x": eval_xsensor.new_totals(True)}, "against": against}
        xs["totals"]["x"]["states"] = [4, 3, 2, 1]
        xs["totals"]["x"]["buckets"]["all"].update(clusters=2, sum_X=0.5)
        if against:
            against["x"]["all"].update(pairs=3, sum_X_against=1.25)
        two = add_sums(xs, copy.deepcopy(xs))
        assert two == _doubled(xs) and two["totals"]["x"]["states"] == [8, 6, 4, 2] and (two["against"] is None) == (against is None)
    # folding in the other order gives the same, and the parts are left as they were
    one = {"x": eval_box.new_sums()}
    one["x"]["pred"], one["x"]["buckets"]["all"]["tp"] = 7, [1, 1, 0]
    kept = copy.deepcopy((box, one))
    assert add_sums(box, one) == add_sums(one, box) and (box, one) == kept
    assert add_sums(add_sums(box, one), box) == add_sums(box, add_sums(one, box))
    with pytest.raises(ValueError, match="different shapes"):
        add_sums({"tp": [1, 2]}, {"tp": [1, 2, 3]})
    # track: ``lengths`` is the one list that is joined, and only at track's own call
    t1, t2 = {"x": track.new_sums()}, {"x": track.new_sums()}
    t1["x"].update(ids=3, lengths=[4], jitter_sum=5.0)
    t1["x"]["mot"]["all"]["tp"] = 2
    t2["x"].update(ids=2, lengths=[3, 9])
    two = track.add_sums(t1, t2)
    assert two["x"]["ids"] == 5 and two["x"]["lengths"] == [4, 3, 9] and two["x"]["mot"]["all"]["tp"] == 2 and two["x"]["jitter_sum"] == 5.0
    assert track.add_sums(t2, t1)["x"]["lengths"] == [3, 9, 4] and sorted(two["x"]) == sorted(t1["x"])
    assert track.summary(track.add_sums(t1, t1), False)["x"]["confirmed"] == 2


# ---- the shell ---------------------------------------------------------------------------------------------------------------------------
class _Closes:
    def __init__(self, log, name, fails=False):
        self.log, self.name, self.fails = log, name, fails

    def close(self):
        self.log.append(self.name)
        if self.fails:
            raise OSError(f"close of {self.name}")


def test_run_shard_closes_everything_and_keeps_the_first_error():
    from himo_amd import distenv

    def bad():
        raise KeyError("the loop")

    log = []
    with pytest.raises(KeyError, match="the loop"):
        distenv.run_shard(bad, "its share", closing=(_Closes(log, "a", fails=True), object(), None, _Closes(log, "b")))
    assert log == ["a", "b"]
    log.clear()
    with pytest.raises(OSError, match="close of a"):
        distenv.run_shard(lambda: None, "its share", closing=lambda: [_Closes(log, "a", fails=True), object(), _Closes(log, "b", fails=True)])
    assert log == ["a", "b"]
    log.clear()
    distenv.run_shard(lambda: log.append("loop"), "its share", closing=[_Closes(log, "a")])
    assert log == ["loop", "a"]
    distenv.run_shard(lambda: None)


def test_report_prints_and_writes_on_rank_0_only(tmp_path, capsys):
    from himo_amd import distenv
    distenv.report(1, "table", {"a": 1}, tmp_path / "no.json")
    assert capsys.readouterr().out == "" and not (tmp_path / "no.json").exists()
    distenv.report(0, "table", {"a": None}, tmp_path / "yes.json")
    assert capsys.readouterr().out == "table\n" and (tmp_path / "yes.json").read_text() == '{\n "a": null\n}\n'
    distenv.report(0, "table", {"a": 1}, None)


# ---- two ranks over gloo -----------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, str(REPO))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _worker(rank, world, port, out_dir):
    _init(rank, world, port)
    from himo_amd import distenv
    closed = []
    total = distenv.gathered({"x": {"n": rank + 1, "tp": [rank, 10], "none": None, "s": 0.5 * (rank + 1)}})

    def loop():
        if rank == 1:
            raise KeyError("rank 1's sweep")

    try:
        distenv.run_shard(loop, "its share of the test", closing=(_Closes(closed, "ds"),))
        raised = None
    except Exception as e:                                             # noqa: BLE001
        raised = [type(e).__name__, str(e)]
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps({"total": total, "raised": raised, "closed": closed}))
    dist.destroy_process_group()


def test_two_ranks_gather_the_same_total_and_meet_after_a_failure(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(2)]
    assert got[0]["total"] == got[1]["total"] == {"x": {"n": 3, "tp": [1, 20], "none": None, "s": 1.5}}
    assert got[1]["raised"] == ["KeyError", "\"rank 1's sweep\""]
    assert got[0]["raised"] == ["RuntimeError", "another rank failed; this rank finished its share of the test"]
    assert got[0]["closed"] == got[1]["closed"] == ["ds"]
