"""The scene-flow evaluator on the device (csrc/flowmetrics.hip, himo_amd/eval_flow.py) against the numpy float64 restatement of
"flow metrics, v1" (tests/flowmetrics_ref.py).

What is compared, and how tightly.  Every seeded speed, as the restatement computes it, stays >= 1e-4 m from every bucket edge
and from the dynamic threshold (asserted), so class, bucket and kind cannot differ and every count, three-way count and
``rejected`` must be EQUAL.  Every sum of q(epe) / q(speed) may differ by at most one unit (2^-24 m) per counted point of its
bin: each double operation of the kernel is within one ulp of numpy's (the transform's LU and fused dot products differ from
numpy's in the last bit), which moves a point's quantised value by at most one unit.  The sums of a STORED result's q(epe)
involve no transform -- identical inputs, correctly rounded operations in the same order -- and are printed as exact or not."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))

import flowmetrics_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

H5 = REPO / "tests" / "golden" / "h5"
W, THR = 0.4 * 0.1, 0.5 * 0.1
EDGES = np.array([k * W for k in range(1, 51)] + [THR])
CATEGORY_OF_CLASS = np.array([0, 19, 6, 17, 3, 1], dtype=np.uint8)      # NONE, REGULAR_VEHICLE, BOX_TRUCK, PEDESTRIAN, BICYCLE, ANIMAL


def rigid(rng, angle, shift):
    ax, ay, az = rng.uniform(-angle, angle, 3)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    t = np.eye(4)
    t[:3, :3] = rz @ ry @ rx
    t[:3, 3] = rng.uniform(-shift, shift, 3)
    return t


def speed_in_bucket(rng, b):
    """a speed at least 2e-3 m inside bucket ``b`` (the last one is open-ended) and off the dynamic threshold"""
    lo = b * W + 2e-3
    hi = np.where(b < 50, (b + 1) * W - 2e-3, 3.0)
    s = lo + rng.random(b.shape) * (hi - lo)
    s[np.abs(s - THR) < 2e-3] = THR + 4e-3
    return s


def make_sweep(rng, n, k, names, bad=None, bins=None, all_counted=False, invalid=0.0):
    xyz = rng.uniform(-52, 52, (n, 3))
    xyz[:, 2] = rng.uniform(-3, 3, n)
    near = rng.random(n) < 0.05
    xyz[near] = rng.uniform(-2.5, 2.5, (int(near.sum()), 3))                  # some inside the ego box
    gm0 = rng.random(n) < 0.2
    if all_counted:
        rad, th = rng.uniform(6, 30, n), rng.uniform(0, 2 * np.pi, n)
        xyz = np.stack([rad * np.cos(th), rad * np.sin(th), rng.uniform(-1, 1, n)], axis=1)
        gm0[:] = False
    pc0 = np.concatenate([xyz, rng.random((n, 1))], axis=1).astype(np.float32)
    if bins is None:
        cls = rng.choice(6, n, p=[0.5, 0.15, 0.1, 0.1, 0.1, 0.05])
        bucket = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 51, n))
    else:
        cls, bucket = bins
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True) if n else 1.0
    motion = speed_in_bucket(rng, bucket)[:, None] * direction
    pose0, pose1 = rigid(rng, 0.02, 1.5), rigid(rng, 0.02, 1.5)
    ego = np.linalg.inv(pose1) @ pose0
    p = pc0[:, :3].astype(np.float64)
    flow = ((p @ ego[:3, :3].T + ego[:3, 3] - p) + motion).astype(np.float32)
    f = {"scene_id": "seeded", "timestamp": k, "pc0": pc0, "gm0": gm0, "pose0": pose0, "pose1": pose1, "flow": flow,
         "flow_category_indices": CATEGORY_OF_CLASS[cls], "flow_is_valid": (rng.random(n) >= invalid).astype(np.uint8)}
    for name in names:
        if name == "raw":
            continue
        est = (flow + rng.normal(0, 0.1, (n, 3))).astype(np.float32)
        if name == bad:
            rows = np.flatnonzero(rng.random(n) < 0.06)
            est[rows[0::3], 0], est[rows[1::3], 1], est[rows[2::3], 2] = np.nan, np.inf, 2000.0
        f[name] = est
    return f


def make_frames(seed, sizes, names, **kw):
    rng = np.random.default_rng(seed)
    return [make_sweep(rng, n, k, names, **kw) for k, n in enumerate(sizes)]


def assert_clear_of_edges(frames, margin, pose_is_ego=False):
    for f in frames:
        s = ref.speeds(f, pose_is_ego)
        if s.size:
            assert np.abs(s[:, None] - EDGES).min() >= margin


def assert_tables(metrics, frames, names, data_name, pose_is_ego=False, times=1, keys=None):
    """the evaluator's integers against the restatement's (``times``: how often the frames were added)"""
    wb, wt, wr = ref.flow_metrics_ref(frames, names, data_name, pose_is_ego=pose_is_ego)
    b, rj, tw = metrics.buckets, metrics.rejected, metrics.threeway
    assert list(tw) == (list(range(len(frames))) if keys is None else list(keys))
    t = np.stack(list(tw.values())) if tw else np.zeros((0, len(names), 3, 2), np.int64)
    assert b.dtype == t.dtype == rj.dtype == np.int64
    assert np.array_equal(b[..., 0], times * wb[..., 0]) and np.array_equal(t[..., 0], times * wt[..., 0]) and np.array_equal(rj, times * wr)
    for got, want, count in ((b[..., 1], wb[..., 1], wb[..., 0]), (b[..., 2], wb[..., 2], wb[..., 0]), (t[..., 1], wt[..., 1], wt[..., 0])):
        assert np.all(np.abs(got - times * want) <= times * count)
    stored = [r for r, name in enumerate(names) if name != "raw"]
    exact = np.array_equal(b[stored][..., 1], times * wb[stored][..., 1]) and np.array_equal(t[:, stored][..., 1], times * wt[:, stored][..., 1])
    worst = max(int(np.abs(b[..., 1:] - times * wb[..., 1:]).max()), int(np.abs(t[..., 1] - times * wt[..., 1]).max()) if t.size else 0)
    print(f"flow metrics vs restatement: {int(wb[..., 0].sum())} bucketed point-results, stored sum q(epe) exact: {exact}, "
          f"largest difference of any sum: {worst} units")
    return wb, wt, wr


SIZES = {"0": [0], "1": [1], "63": [63], "64": [64], "65": [65], "1023": [1023], "1024": [1024], "1025": [1025],
         "ragged": [5, 0, 16, 33, 1, 4097, 250]}


@pytest.mark.parametrize("case", list(SIZES))
def test_sweep_sizes_against_the_restatement(gpu, case):
    """an empty sweep, sweeps smaller than a wave, around the wave and block sizes, one spanning blocks; two calls accumulate
    and reset() zeroes"""
    from himo_amd.eval_flow import FlowMetrics
    names = ["flow_a", "raw"]
    frames = make_frames(11 + sum(SIZES[case]), SIZES[case], names, bad="flow_a")
    assert_clear_of_edges(frames, 1e-4)
    m = FlowMetrics(names, "av2")
    m.add(frames)
    wb, _, _ = assert_tables(m, frames, names, "av2")
    assert m.frame_cnt == len(frames)
    if sum(SIZES[case]) >= 1023:
        assert wb[..., 0].sum() > 0 and (wb[0, :, 0, 0] > 0).all() and (wb[0, :, 1:, 0].sum(axis=1) > 0).all()     # (every class, both regimes)
    m.add(frames, keys=range(len(frames)))                     # a second call accumulates
    assert_tables(m, frames, names, "av2", times=2)
    m.reset()
    assert m.buckets.sum() == 0 and m.rejected.sum() == 0 and m.threeway == {} and m.frame_cnt == 0
    m.add(frames[:1])
    assert_tables(m, frames[:1], names, "av2")


def test_two_large_sweeps_take_the_capped_grid(gpu):
    """more points than blocks x threads: every block walks a run of several steps; the second sweep starts unaligned"""
    from himo_amd.eval_flow import FlowMetrics
    names = ["flow_a", "raw"]
    frames = make_frames(5, [120_000, 119_993], names, bad="flow_a")
    assert_clear_of_edges(frames, 1e-4)
    m = FlowMetrics(names, "av2")
    m.add(frames)
    _, _, wr = assert_tables(m, frames, names, "av2")
    assert wr[0] > 1000 and wr[1] == 0


@pytest.mark.parametrize("n_results", [1, 2, 8])
def test_result_counts_with_raw_and_a_result_of_bad_rows(gpu, n_results):
    from himo_amd.eval_flow import FlowMetrics
    names = (["flow_0", "raw"] + [f"flow_{k}" for k in range(2, 8)])[:n_results]
    frames = make_frames(70 + n_results, [700, 0, 300], names, bad="flow_0")
    assert_clear_of_edges(frames, 1e-4)
    m = FlowMetrics(names, "av2")
    m.add(frames)
    _, _, wr = assert_tables(m, frames, names, "av2")
    assert wr[0] > 0 and not wr[1:].any()                       # NaN / inf / 2000 m rows of counted points are rejected, for that result only


def test_one_bin_for_every_point_takes_the_aggregated_path(gpu):
    from himo_amd.eval_flow import FlowMetrics
    n = 4097
    frames = make_frames(3, [n], ["flow_a"], bins=(np.zeros(n, np.int64), np.zeros(n, np.int64)), all_counted=True)
    assert_clear_of_edges(frames, 1e-4)
    m = FlowMetrics(["flow_a"], "av2")
    m.add(frames)
    wb, wt, _ = assert_tables(m, frames, ["flow_a"], "av2")
    assert wb[0, 0, 0, 0] == n and wb[..., 0].sum() == n and wt[0, 0, 2, 0] == n


def test_255_bins_in_turn_take_the_per_lane_path(gpu):
    """point i falls into bin i % 255, so every wave holds 64 different bins: four aggregated rounds, then lane by lane"""
    from himo_amd.eval_flow import FlowMetrics
    n = 4096
    bins = np.arange(n) % 255
    frames = make_frames(4, [n], ["flow_a", "raw"], bins=(bins // 51, bins % 51), all_counted=True)
    assert_clear_of_edges(frames, 1e-4)
    m = FlowMetrics(["flow_a", "raw"], "av2")
    m.add(frames)
    wb, _, _ = assert_tables(m, frames, ["flow_a", "raw"], "av2")
    assert (wb[1, :, :, 0] >= n // 255).all()                   # all 255 bins are occupied


@pytest.mark.parametrize("invalid", [0.0, 0.3])
def test_scania_rules_read_flow_is_valid_and_the_long_ego_box(gpu, invalid):
    from himo_amd.eval_flow import FlowMetrics
    names = ["flow_a", "raw"]
    frames = make_frames(21, [900, 333], names, invalid=invalid)
    assert_clear_of_edges(frames, 1e-4)
    m = FlowMetrics(names, "scania")
    m.add(frames)
    wb, _, _ = assert_tables(m, frames, names, "scania")
    assert wb[..., 0].sum() > 0
    assert any((ref.counted_mask(f, "scania") != ref.counted_mask(f, "av2")).any() for f in frames)      # (the two rules differ on these points)
    if invalid:
        assert any((ref.counted_mask(f, "scania") < ref.counted_mask(dict(f, flow_is_valid=np.ones_like(f["flow_is_valid"])), "scania")).any()
                   for f in frames)                              # (invalid points the other rules would count)
        with pytest.raises(KeyError, match="flow_is_valid"):
            FlowMetrics(names, "scania").add([{k: v for k, v in f.items() if k != "flow_is_valid"} for f in frames])


def test_pose_is_ego_takes_the_callers_transform(gpu):
    from himo_amd.eval_flow import FlowBatch, FlowMetrics
    names = ["flow_a", "raw"]
    frames = make_frames(31, [500, 77], names)
    held = [dict(f, pose0=np.linalg.inv(f["pose1"]) @ f["pose0"], pose1=np.eye(4)) for f in frames]
    assert_clear_of_edges(held, 1e-4, pose_is_ego=True)
    batch = FlowBatch.from_frames(held, names)
    batch.pose_is_ego = True
    m = FlowMetrics(names, "av2")
    m.add_batch(batch)
    assert_tables(m, held, names, "av2", pose_is_ego=True)


def _device_tables(gpu, n_frames, n_results):
    import torch
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=gpu)      # noqa: E731
    return z(n_results, 5, 51, 3), z(n_frames, n_results, 3, 2), z(n_results)


def test_thin_launch_on_a_row_view_and_its_invalid_arguments(gpu):
    import torch
    from himo_amd.eval_flow import FlowBatch, class_lut, flow_metrics
    names = ["flow_a", "raw"]
    frames = make_frames(41, [300, 211], names)
    assert_clear_of_edges(frames, 1e-4)
    b = FlowBatch.from_frames(frames, names)
    wide = torch.zeros((b.total_points, 6), dtype=torch.float32, device=gpu)
    wide[:, :4] = b.pc0
    view = wide[:, :4]                                            # an [N, 4] view of rows six floats apart
    assert not view.is_contiguous()
    buckets, threeway, rejected = _device_tables(gpu, 2, 2)
    flow_metrics(buckets, threeway, rejected, b.offsets, b.pose0, b.pose1, view, b.gt, b.ests, b.category, b.ground)
    wb, wt, wr = ref.flow_metrics_ref(frames, names, "av2")
    got_b, got_t = buckets.cpu().numpy(), threeway.cpu().numpy()
    assert np.array_equal(got_b[..., 0], wb[..., 0]) and np.array_equal(got_t[..., 0], wt[..., 0]) and np.array_equal(rejected.cpu().numpy(), wr)
    assert np.all(np.abs(got_b[..., 1:] - wb[..., 1:]) <= wb[..., :1]) and np.all(np.abs(got_t[..., 1] - wt[..., 1]) <= wt[..., 0])

    def launch(ests=b.ests, lut=None, tables=None):
        bk, tw, rj = tables if tables is not None else _device_tables(gpu, 2, len(ests))
        flow_metrics(bk, tw, rj, b.offsets, b.pose0, b.pose1, b.pc0, b.gt, ests, b.category, b.ground, lut=lut)
        return bk
    with pytest.raises(ValueError):
        launch(ests=[b.ests[0]] * 9)                              # nine results
    with pytest.raises(ValueError):
        launch(ests=[b.ests[0][:-1], None])                       # a short result
    six = class_lut()
    six[200] = 6
    with pytest.raises(ValueError):
        launch(lut=six)                                           # a table value of 6
    with pytest.raises(ValueError):
        launch(tables=_device_tables(gpu, 2, 1))                  # tables of another result count
    assert int(launch().sum()) > 0                                # (the same call with valid arguments counts)


class _Listed:
    """a dataset of frame dicts held in memory"""

    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i]


def test_batch_size_and_overlap_cannot_change_a_digit(gpu, capsys):
    from himo_amd.eval_flow import FlowMetrics, run_dataset
    names = ["flow_a", "raw"]
    frames = make_frames(51, [400, 0, 129, 64, 1000], names, bad="flow_a")
    frames.insert(2, {k: v for k, v in frames[0].items() if k != "flow"})          # a sweep without ground truth is skipped
    frames[2]["timestamp"] = 99
    kept = [0, 1, 3, 4, 5]
    assert_clear_of_edges([frames[i] for i in kept], 1e-4)
    tables = []
    for batch_frames, overlap in ((1, True), (2, True), (32, True), (1, False), (2, False), (32, False)):
        m = FlowMetrics(names, "av2")
        assert run_dataset(_Listed(frames), m, batch_frames=batch_frames, overlap=overlap) == len(kept)
        assert capsys.readouterr().out == "[Warning]: No flow in seeded at 99, check the data.\n"
        tables.append((m.buckets, np.stack(list(m.threeway.values())), m.rejected))
        if len(tables) == 1:
            assert_tables(m, [frames[i] for i in kept], names, "av2", keys=kept)
            capsys.readouterr()
        assert list(m.threeway) == kept and m.frame_cnt == len(kept)
        assert all(np.array_equal(x, y) for x, y in zip(tables[0], tables[-1]))


@pytest.mark.parametrize("overlap", [True, False])
def test_missing_result_name_is_a_key_error(gpu, overlap, capsys):
    from himo_amd.eval_flow import FlowMetrics, main, run_dataset
    frames = make_frames(61, [100, 50], ["flow_a"])
    with pytest.raises(KeyError, match="flow_nowhere"):
        if overlap:
            main(str(H5), res_names="seflowpp_best,flow_nowhere", data_name="av2")
        else:
            run_dataset(_Listed(frames), FlowMetrics(["flow_a", "flow_nowhere"], "av2"), overlap=False)
    assert "[Warning]: No flow_nowhere in " in capsys.readouterr().out


def test_main_over_the_golden_scenes(gpu, capsys, tmp_path):
    from himo_amd import eval_flow
    from himo_amd.dataset import FLOW_EVAL_FIELDS, open_dataset
    names = ["seflowpp_best", "raw"]
    ds = open_dataset(H5, vis_name=["seflowpp_best"], eval=True, fields=FLOW_EVAL_FIELDS + ("seflowpp_best",))
    frames = [ds[i] for i in range(len(ds))]
    assert len(frames) > 1 and all("flow" in f and "flow_category_indices" in f for f in frames)
    assert_clear_of_edges(frames, 1e-9)                           # (checked on the CPU first: no fixture speed sits on an edge)
    path = tmp_path / "flow.json"
    path.write_text(json.dumps({"kept": 1}))
    m = eval_flow.main(str(H5), res_names="seflowpp_best,raw", data_name="av2", json_path=str(path))
    out = capsys.readouterr().out
    wb, _, _ = assert_tables(m, frames, names, "av2")
    assert wb[..., 0].sum() > 0 and m.frame_cnt == len(frames)
    res = m.results()
    assert out == m.table()
    fmt = lambda v: "-" if v != v else f"{v:.6f}"                 # noqa: E731
    for name, block in zip(names, out.split("Flow metrics (v1) for ")[1:]):
        lines = block.splitlines()
        assert lines[0].startswith(f"{name} in av2: {len(frames)} sweeps, {res[name]['counted']} points, {res[name]['rejected']} rejected")
        for row, line in (("static", lines[2]), ("dynamic", lines[3])):
            assert line.split() == [row] + [fmt(res[name][row][c]) for c in eval_flow.CLASS_NAMES] + [fmt(res[name]["mean_" + row])]
        assert lines[4].split() == ["three-way", fmt(res[name]["three_way"]), "FD", fmt(res[name]["FD"]), "FS", fmt(res[name]["FS"]),
                                    "BS", fmt(res[name]["BS"])]
    back = json.loads(path.read_text())
    assert back["kept"] == 1 and set(back) == {"kept", *names}
    same = lambda x, y: (x != x and y != y) or x == y             # noqa: E731  (nan round-trips as nan)
    for name in names:
        for key, v in res[name].items():
            if isinstance(v, dict):
                assert all(same(back[name][key][c], v[c]) for c in v)
            else:
                assert same(back[name][key], v)
    # the float64 means are the restatement's on the evaluator's own integers (sums of at most 50 terms: 1e-13 relative)
    tw = np.stack(list(m.threeway.values()))
    for r, name in enumerate(names):
        want = ref.means_ref(m.buckets[r], tw[:, r])
        for key in ("FD", "FS", "BS", "three_way", "mean_static", "mean_dynamic"):
            assert same(res[name][key], want[key]) or res[name][key] == pytest.approx(want[key], rel=1e-13)
        for c, cname in enumerate(eval_flow.CLASS_NAMES):
            for row in ("static", "dynamic"):
                assert same(res[name][row][cname], want[row][c]) or res[name][row][cname] == pytest.approx(want[row][c], rel=1e-13)
