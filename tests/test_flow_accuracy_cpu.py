"""Rules 3b (residual estimates) and 9 (accuracy table) of "flow metrics, v1" without a GPU: the numpy restatement
(tests/flowaccuracy_ref.py) on the fixture whose table a throw-away prototype gave, and the host bookkeeping of
himo_amd/eval_flow.py (the means, the table's lines, the gather over ranks) on host-set integer tables."""
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

import flowaccuracy_ref as acc  # noqa: E402
import flowmetrics_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def frames():
    return acc.fixture()


def test_restatement_reproduces_the_prototypes_table_in_both_modes(frames):
    b, t, rj, a = acc.flow_accuracy_ref(frames, ["a", "raw"], "av2")
    assert a[0].tolist() == acc.FIXTURE_TABLE
    c, s, r = a[0, :, 0], a[0, :, 1], a[0, :, 2]
    assert (0 < s).all() and (s < r).all() and (r < c).all()                      # every group populated, strict < relaxed < count
    assert c[0] - c[1:].sum() == 15                                               # ALL also holds the dynamic background points
    assert np.array_equal(a[1, :, 0], c) and not rj.any()                         # raw counts the same points
    # rules 1-8 are untouched by the additions
    wb, wt, wr = ref.flow_metrics_ref(frames, ["a", "raw"], "av2")
    assert np.array_equal(b, wb) and np.array_equal(t, wt) and np.array_equal(rj, wr)
    # residual mode: the same table, the margins the issue records, an all-zero residual is raw
    b2, t2, rj2, a2 = acc.flow_accuracy_ref(frames, ["res", "raw"], "av2", residual=True)
    assert a2[0].tolist() == acc.FIXTURE_TABLE and np.array_equal(a2[1], a[1]) and not rj2.any()
    assert np.array_equal(b2[..., 0], b[..., 0]) and np.array_equal(t2[..., 0], t[..., 0])
    assert acc.threshold_margin(frames, "res", residual=True) >= 4.9e-5
    assert min(np.abs(ref.speeds(f) - 0.05).min() for f in frames) >= 1.1e-4
    zero = [dict(f, zero=np.zeros_like(f["res"])) for f in frames]
    bz, tz, rz, az = acc.flow_accuracy_ref(zero, ["zero", "raw"], "av2", residual=True)
    assert np.array_equal(bz[0], bz[1]) and np.array_equal(tz[:, 0], tz[:, 1]) and np.array_equal(az[0], az[1])


def test_rejected_rows_are_in_no_group(frames):
    bad = [dict(f, a=f["a"].copy()) for f in frames]
    for f in bad:
        f["a"][0::9, 0], f["a"][1::9, 1], f["a"][2::9, 2] = np.nan, np.inf, 2000.0
    _, _, rj, a = acc.flow_accuracy_ref(bad, ["a", "raw"], "av2")
    assert rj[0] > 0 and rj[1] == 0
    assert a[0, 0, 0] + rj[0] == a[1, 0, 0] == acc.FIXTURE_TABLE[0][0]


def test_from_counts_gives_the_means_and_nan_for_an_empty_group():
    from himo_amd.eval_flow import BUCKETS, CLASSES, GROUPS, FlowMetrics
    assert GROUPS == acc.GROUPS
    table = np.zeros((2, 4, 3), dtype=np.int64)
    table[0] = acc.FIXTURE_TABLE
    table[1] = [[8, 2, 4], [8, 2, 4], [0, 0, 0], [0, 0, 0]]
    buckets = np.zeros((2, CLASSES, BUCKETS, 3), dtype=np.int64)
    m = FlowMetrics.from_counts("a,b", "av2", buckets, {}, accuracy=table)
    assert m.accuracy.dtype == np.int64 and np.array_equal(m.accuracy, table)
    res = m.results()
    for r, name in enumerate(("a", "b")):
        strict, relaxed = acc.accuracy_means(table[r])
        for g in acc.GROUPS:
            for got, want in ((res[name]["acc_strict"][g], strict[g]), (res[name]["acc_relaxed"][g], relaxed[g])):
                assert (math.isnan(got) and math.isnan(want)) or got == want
    assert res["a"]["acc_strict"]["ALL"] == 363 / 524 and res["a"]["acc_relaxed"]["BS"] == 138 / 140
    assert res["b"]["acc_strict"]["FD"] == 0.25 and math.isnan(res["b"]["acc_strict"]["FS"]) and math.isnan(res["b"]["acc_relaxed"]["BS"])
    lines = m.table().splitlines()
    assert sum(line.startswith("accuracy strict ") for line in lines) == 2 and sum(line.startswith("accuracy relaxed") for line in lines) == 2
    assert f"ALL {363 / 524:.6f}" in m.table() and "FS -" in m.table()
    m.accuracy = np.zeros_like(table)                              # the setter replaces the counts
    assert m.accuracy.sum() == 0
    # accuracy off: today's keys and today's lines
    plain = FlowMetrics.from_counts("a,b", "av2", buckets, {})
    assert "acc_strict" not in plain.results()["a"] and "acc_relaxed" not in plain.results()["a"]
    assert set(res["a"]) - set(plain.results()["a"]) == {"acc_strict", "acc_relaxed"}
    assert "accuracy" not in plain.table()
    with pytest.raises(ValueError):
        FlowMetrics.from_counts("a,b", "av2", buckets, {}, accuracy=np.zeros((3, 4, 3), dtype=np.int64))


def test_cli_has_the_accuracy_flag():
    import inspect
    from himo_amd import eval_flow
    assert inspect.signature(eval_flow.main).parameters["accuracy"].default is False
    assert inspect.signature(eval_flow.flow_metrics).parameters["residual"].default is False
    assert inspect.signature(eval_flow.flow_metrics).parameters["accuracy"].default is None


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sweep_words(i, n_results):
    rng = np.random.default_rng(900 + i)
    return (rng.integers(0, 1 << 40, (n_results, 3, 2)), rng.integers(0, 1 << 40, (n_results, 5, 51, 3)), rng.integers(0, 9, n_results),
            rng.integers(0, 1 << 40, (n_results, 4, 3)))


def _worker_gather(rank, world, port, n_sweeps, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, str(REPO))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from himo_amd.eval_flow import FlowMetrics
    m = FlowMetrics("a,b", "av2", accuracy=True)
    buckets, rejected, table, threeway = m.buckets.copy(), m.rejected.copy(), m.accuracy.copy(), {}
    for i in range(rank, n_sweeps, world):                        # sweep i -> rank i % world
        tw, b, rj, a = _sweep_words(i, 2)
        threeway[i], buckets, rejected, table = tw, buckets + b, rejected + rj, table + a
    m.buckets, m.threeway, m.rejected, m.accuracy, m.frame_cnt = buckets, threeway, rejected, table, len(threeway)
    calls, all_reduce = [], dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (calls.append(int(t.numel())), all_reduce(t, *a, **k))[1]
    m.gather()
    dist.all_reduce = all_reduce
    np.savez(Path(out_dir) / f"rank{rank}.npz", buckets=m.buckets, rejected=m.rejected, accuracy=m.accuracy, keys=np.array(list(m.threeway)),
             threeway=np.stack(list(m.threeway.values())), frames=m.frame_cnt, calls=np.array(calls))
    dist.destroy_process_group()


def test_gather_carries_the_accuracy_table_in_the_same_all_reduce(tmp_path):
    n_sweeps, world = 5, 2
    mp.spawn(_worker_gather, args=(world, _free_port(), n_sweeps, str(tmp_path)), nprocs=world, join=True)
    words = [_sweep_words(i, 2) for i in range(n_sweeps)]
    for rank in range(world):
        with np.load(tmp_path / f"rank{rank}.npz") as z:
            assert z["keys"].tolist() == list(range(n_sweeps)) and int(z["frames"]) == n_sweeps
            assert np.array_equal(z["threeway"], np.stack([w[0] for w in words]))
            assert np.array_equal(z["buckets"], sum(w[1] for w in words)) and np.array_equal(z["rejected"], sum(w[2] for w in words))
            assert np.array_equal(z["accuracy"], sum(w[3] for w in words))
            assert z["calls"].tolist() == [2 * 5 * 51 * 3 + 2 + 2 * 4 * 3 + 1]      # ONE all-reduce: buckets, rejected, accuracy, sweeps
