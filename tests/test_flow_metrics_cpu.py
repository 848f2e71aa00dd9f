"""The scene-flow evaluator without a GPU: the numpy restatement of "flow metrics, v1" (tests/flowmetrics_ref.py) on a sweep worked
by hand, the bucket rule at its edges, the class table, and the host bookkeeping of himo_amd/eval_flow.py (means, table, JSON,
the gather over ranks) on host-set integer tables."""
import json
import math
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))

import flowmetrics_ref as ref  # noqa: E402

Q = 2 ** 24


def hand_sweep():
    """11 points, identity poses (the pose flow is exactly zero, so g = gt), Scania rules (flow_is_valid counts; ego box
    -9.5..5 x -1.5..1.38 x 0..5).  Every value is a small binary fraction, so the integers below are exact."""
    nan = float("nan")
    #        x    y   z  ground valid cat   gt x      est x  est y  est z
    rows = [(10,   0, 1, 0, 1, 19, 0.5,     0.5,   0.25, 0),       # 0 FD: CAR, speed 0.5 -> bucket 12, epe 0.25
            (0,   10, 1, 0, 1, 17, 0,       0,     0,    0.125),   # 1 FS: PEDESTRIAN, still, epe 0.125
            (-20,  5, 1, 0, 1, 0,  0.03125, 0.03125, 0,  0),       # 2 BS: background, speed 1/32 < 0.05, epe 0
            (20,   5, 1, 0, 1, 0,  1,       1,     0,    0.5),     # 3 background DYNAMIC: buckets only; 25 w > 1 -> bucket 24
            (5,   10, 1, 0, 1, 1,  0,       0.5,   0,    0),       # 4 class 5 (ANIMAL): FS, in no bucket, epe 0.5
            (30,  30, 1, 0, 1, 19, 0,       9,     9,    9),       # 5 out of range (42 m)
            (10,  10, 1, 1, 1, 19, 0,       9,     9,    9),       # 6 ground
            (0,    0, 1, 0, 1, 19, 0,       9,     9,    9),       # 7 inside the ego box
            (10, -10, 1, 0, 0, 19, 0,       9,     9,    9),       # 8 flow_is_valid = 0
            (-10, -10, 1, 0, 1, 19, 0,      nan,   0,    0),       # 9 rejected: NaN estimate (raw: CAR, still, epe 0)
            (-10, 10, 1, 0, 1, 19, 0,       2000,  0,    0)]       # 10 rejected: 2000 m      (raw: CAR, still, epe 0)
    a = np.array(rows, dtype=np.float64)
    return {"scene_id": "hand", "timestamp": 0, "pc0": a[:, :3].astype(np.float32), "gm0": a[:, 3].astype(bool),
            "flow_is_valid": a[:, 4].astype(np.uint8), "flow_category_indices": a[:, 5].astype(np.uint8),
            "flow": np.stack([a[:, 6], 0 * a[:, 6], 0 * a[:, 6]], axis=1).astype(np.float32), "est": a[:, 7:10].astype(np.float32),
            "pose0": np.eye(4), "pose1": np.eye(4)}


def test_restatement_on_the_hand_worked_sweep():
    buckets, threeway, rejected = ref.flow_metrics_ref([hand_sweep()], ["est", "raw"], "scania")
    want = np.zeros((2, 5, 51, 3), dtype=np.int64)
    want[0, 1, 12] = (1, Q // 4, Q // 2)            # point 0
    want[0, 3, 0] = (1, Q // 8, 0)                  # point 1
    want[0, 0, 0] = (1, 0, Q // 32)                 # point 2
    want[0, 0, 24] = (1, Q // 2, Q)                 # point 3
    want[1, 1, 12] = (1, Q // 2, Q // 2)            # raw: epe = speed
    want[1, 3, 0] = (1, 0, 0)
    want[1, 0, 0] = (1, Q // 32, Q // 32)
    want[1, 0, 24] = (1, Q, Q)
    want[1, 1, 0] = (2, 0, 0)                       # points 9 and 10 count for raw
    assert np.array_equal(buckets, want)
    assert threeway.tolist() == [[[[1, Q // 4], [2, Q // 8 + Q // 2], [1, 0]],            # est: FD p0, FS p1 + p4, BS p2
                                  [[1, Q // 2], [4, 0], [1, Q // 32]]]]                   # raw: FS p1 p4 p9 p10
    assert rejected.tolist() == [2, 0]
    m = ref.means_ref(buckets[0], threeway[:, 0])
    assert (m["FD"], m["FS"], m["BS"], m["three_way"]) == (0.25, 0.3125, 0.0, 0.1875)
    assert m["static"][0] == 0.0 and math.isnan(m["static"][1]) and m["static"][3] == 0.125 and math.isnan(m["static"][4])
    assert m["dynamic"][0] == 0.5 and m["dynamic"][1] == 0.5 and math.isnan(m["dynamic"][2])
    assert m["mean_static"] == 0.0625 and m["mean_dynamic"] == 0.5
    # the same sweep under the AV2 rules: flow_is_valid is not read (point 8 counts), the ego box is 3 x 3 x 4 m (point 7 stays out)
    b2, t2, r2 = ref.flow_metrics_ref([hand_sweep()], ["raw"], "av2")
    assert b2[0, 1, 0].tolist() == [3, 0, 0] and t2[0, 0, 1].tolist() == [5, 0] and r2.tolist() == [0]


def test_bucket_rule_at_below_and_beyond_its_edges():
    w = 0.4 * 0.1
    for k in range(1, 51):
        edge = k * w
        assert ref.bucket_of(edge) == k and ref.bucket_of(np.nextafter(edge, 0.0)) == k - 1 and ref.bucket_of(np.nextafter(edge, 9.0)) == k
    assert ref.bucket_of(0.0) == 0 and ref.bucket_of(np.nextafter(w, 0.0)) == 0
    assert 50 * w > 2.0 and ref.bucket_of(2.0) == 49            # the edges are k * w in double: the 50th lies one ulp above 2.0
    assert ref.bucket_of(np.nextafter(2.0, 9.0)) == 50 and ref.bucket_of(2.5) == 50 and ref.bucket_of(1000.0) == 50
    assert ref.bucket_of([0.039, 0.041, 1.0, 1.99]).tolist() == [0, 1, 24, 49]


def test_class_table_for_all_256_bytes():
    from himo_amd import eval_flow
    from himo_amd.eval import BUCKETED_METACATAGORIES, CATEGORY_TO_INDEX
    lut = eval_flow.class_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256,) and np.array_equal(lut, ref.class_table())
    for cid, name in enumerate(("BACKGROUND", "CAR", "OTHER_VEHICLES", "PEDESTRIAN", "WHEELED_VRU")):
        assert sorted(np.flatnonzero(lut == cid)) == sorted(CATEGORY_TO_INDEX[c] for c in BUCKETED_METACATAGORIES[name])
    assert np.all(lut[31:] == 5) and int((lut == 5).sum()) == 256 - 1 - 1 - 9 - 4 - 6
    assert eval_flow.CLASS_NAMES == ("BACKGROUND", "CAR", "OTHER_VEHICLES", "PEDESTRIAN", "WHEELED_VRU")


def _host_tables():
    """two results, three sweeps (dataset indices 4, 0, 2 -- given out of order); sweep 2 has no FD points"""
    buckets = np.zeros((2, 5, 51, 3), dtype=np.int64)
    buckets[0, 0, 0] = (4, Q, 0)                    # BACKGROUND static 0.25
    buckets[0, 1, 0] = (2, Q, 0)                    # CAR static 0.5
    buckets[0, 1, 3] = (2, Q, 4 * Q)                # CAR dynamic: buckets 3 and 10 -> mean(0.25, 0.75) = 0.5
    buckets[0, 1, 10] = (1, 3 * Q, 4 * Q)
    buckets[0, 3, 7] = (3, Q, 8 * Q)                # PEDESTRIAN dynamic 0.125, no static points
    threeway = {4: [[[1, Q], [1, 0], [2, Q]], [[0, 0], [0, 0], [0, 0]]],
                0: [[[2, Q], [0, 0], [1, Q]], [[0, 0], [0, 0], [0, 0]]],
                2: [[[0, 0], [4, Q], [4, Q]], [[0, 0], [0, 0], [0, 0]]]}
    return buckets, threeway


def test_results_table_and_json_from_host_set_tables(tmp_path):
    from himo_amd import eval_flow
    buckets, threeway = _host_tables()
    m = eval_flow.FlowMetrics.from_counts("a,b", "av2", buckets, threeway, rejected=[7, 0])
    assert list(m.threeway) == [0, 2, 4] and m.frame_cnt == 3                      # dataset order
    res = m.results()
    a, b = res["a"], res["b"]
    assert a["FD"] == (0.5 + 1.0) / 2                                             # sweeps 0 and 4; sweep 2 has no FD point
    assert a["FS"] == (0.25 + 0.0) / 2 and a["BS"] == (1.0 + 0.25 + 0.5) / 3
    assert a["three_way"] == float(np.mean([a["FD"], a["FS"], a["BS"]]))
    assert a["static"]["BACKGROUND"] == 0.25 and a["static"]["CAR"] == 0.5 and math.isnan(a["static"]["PEDESTRIAN"])
    assert a["dynamic"]["CAR"] == 0.5 and a["dynamic"]["PEDESTRIAN"] == 0.125 and math.isnan(a["dynamic"]["BACKGROUND"])
    assert a["mean_static"] == 0.375 and a["mean_dynamic"] == 0.3125
    assert a["counted"] == 4 + (1 + 2) + (1 + 4) and a["rejected"] == 7
    want = ref.means_ref(buckets[0], [np.array(threeway[k])[0] for k in (0, 2, 4)])
    for key in ("FD", "FS", "BS", "three_way", "mean_static", "mean_dynamic"):
        assert a[key] == pytest.approx(want[key], rel=1e-14)
    # a result with nothing counted: nan everywhere, "-" in the table
    assert all(math.isnan(b[k]) for k in ("FD", "FS", "BS", "three_way", "mean_static", "mean_dynamic")) and b["counted"] == 0
    text = m.table()
    block_a, block_b = text.split("Flow metrics (v1) for ")[1:]
    assert block_a.startswith("a in av2: 3 sweeps, 12 points, 7 rejected")
    rows = {ln.split()[0]: ln.split()[1:] for ln in block_a.splitlines()[2:4]}
    assert rows["static"] == ["0.250000", "0.500000", "-", "-", "-", "0.375000"]
    assert rows["dynamic"] == ["-", "0.500000", "-", "0.125000", "-", "0.312500"]
    assert "three-way 0.486111  FD 0.750000  FS 0.125000  BS 0.583333" in block_a
    assert "three-way -  FD -  FS -  BS -" in block_b and block_b.splitlines()[2].split() == ["static"] + ["-"] * 6
    # the JSON merge keeps what the file held for other names and round-trips nan
    path = tmp_path / "flow.json"
    path.write_text(json.dumps({"other": {"three_way": 1.5}, "a": "stale"}))
    eval_flow.merge_json(str(path), res)
    back = json.loads(path.read_text())
    assert back["other"] == {"three_way": 1.5} and set(back) == {"other", "a", "b"}
    assert back["a"]["FD"] == a["FD"] and back["a"]["dynamic"]["CAR"] == 0.5 and math.isnan(back["b"]["three_way"])
    assert math.isnan(back["a"]["static"]["PEDESTRIAN"]) and back["a"]["rejected"] == 7
    # assignable views and reset()
    m.buckets = 2 * buckets
    assert m.results()["a"]["static"]["CAR"] == 0.5 and m.results()["a"]["counted"] == 8 + 8
    m.reset()
    assert m.buckets.sum() == 0 and m.threeway == {} and m.rejected.sum() == 0 and m.frame_cnt == 0


def test_evaluator_refuses_what_it_cannot_count():
    from himo_amd import eval_flow
    with pytest.raises(ValueError):
        eval_flow.FlowMetrics([f"r{k}" for k in range(9)], "av2")
    with pytest.raises(ValueError):
        eval_flow.FlowMetrics("a", "kitti")
    assert eval_flow.data_name_of("/data/av2/h5") == "av2" and eval_flow.data_name_of("/data/Scania/val") == "scania"
    with pytest.raises(ValueError):
        eval_flow.data_name_of("av2")                                             # (a match at position 0 does not count)
    assert eval_flow.parse_res_names("['seflowpp_best','raw']") == ["seflowpp_best", "raw"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sweep_words(i, n_results):
    rng = np.random.default_rng(500 + i)
    return rng.integers(0, 1 << 40, (n_results, 3, 2)), rng.integers(0, 1 << 40, (n_results, 5, 51, 3)), rng.integers(0, 9, n_results)


def _worker_gather(rank, world, port, n_sweeps, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, str(REPO))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from himo_amd.eval_flow import FlowMetrics
    m = FlowMetrics("a,b", "av2")
    buckets, rejected, threeway = m.buckets.copy(), m.rejected.copy(), {}
    for i in range(rank, n_sweeps, world):                        # sweep i -> rank i % world
        tw, b, rj = _sweep_words(i, 2)
        threeway[i], buckets, rejected = tw, buckets + b, rejected + rj
    m.buckets, m.threeway, m.rejected, m.frame_cnt = buckets, threeway, rejected, len(threeway)
    m.gather()
    np.savez(Path(out_dir) / f"rank{rank}.npz", buckets=m.buckets, rejected=m.rejected, keys=np.array(list(m.threeway)),
             threeway=np.stack(list(m.threeway.values())), frames=m.frame_cnt)
    dist.destroy_process_group()


def test_gather_gives_every_rank_the_single_process_integers_in_dataset_order(tmp_path):
    n_sweeps, world = 7, 2
    mp.spawn(_worker_gather, args=(world, _free_port(), n_sweeps, str(tmp_path)), nprocs=world, join=True)
    words = [_sweep_words(i, 2) for i in range(n_sweeps)]
    for rank in range(world):
        with np.load(tmp_path / f"rank{rank}.npz") as z:
            assert z["keys"].tolist() == list(range(n_sweeps)) and int(z["frames"]) == n_sweeps
            assert np.array_equal(z["threeway"], np.stack([w[0] for w in words]))
            assert np.array_equal(z["buckets"], sum(w[1] for w in words)) and np.array_equal(z["rejected"], sum(w[2] for w in words))
