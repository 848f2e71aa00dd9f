"""The Scania extractor on the GPU (dataprocess/extract_sca.py): ``himo_box_label_batch`` bit for bit against the h5 files the
reference wrote and against the float64 checker (tests/boxlabel_ref.py) over the sizes at which the kernel changes path, the
face / overlap cases, the refusals, and the program end to end on the committed raw tree.  Reads committed fixtures only."""
import json
import pickle
from pathlib import Path

import numpy as np
import pytest

import boxlabel_ref
from conftest import GOLDEN, REPO
from test_extract_sca_cpu import BOX, FACE_POINTS, FACE_WANT, labelled_frames

pytestmark = pytest.mark.gpu

SCA = GOLDEN / "sca"
RAW = SCA / "raw"
BYTE_GUARD, BYTE_FILL = 4096, 0xA5


def _h5():
    from himo_amd.dataset import h5_reader
    return h5_reader()


class Outputs:
    """the four output columns inside guarded buffers (``off``: floats / words / bytes of misalignment)"""

    def __init__(self, total, dev, off=0):
        import torch
        from guarded import Guarded
        self.total = total
        self.flow = Guarded(torch.arange(total * 3, dtype=torch.int64), dev, off=off)
        self.inst = Guarded(torch.arange(total, dtype=torch.int64), dev, off=off)
        self.bytes = [torch.full((2 * BYTE_GUARD + total + 16,), BYTE_FILL, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.boff = BYTE_GUARD + off

    def ptrs(self):
        return self.flow.ptr, self.bytes[0].data_ptr() + self.boff, self.bytes[1].data_ptr() + self.boff, self.inst.ptr

    def get(self):
        T = self.total
        flow = self.flow.get().numpy().reshape(T, 3) if T else np.zeros((0, 3), np.float32)
        inst = self.inst.words().numpy().view(np.uint32) if T else np.zeros(0, np.uint32)
        valid, cat = (b[self.boff:self.boff + T].cpu().numpy() for b in self.bytes)
        return flow, valid, cat, inst

    def guards_untouched(self):
        ok = self.flow.untouched_outside() and self.inst.untouched_outside() if self.total else self.flow.untouched() and self.inst.untouched()
        for b in self.bytes:
            h = b.cpu().numpy()
            ok = ok and bool((h[:self.boff] == BYTE_FILL).all()) and bool((h[self.boff + self.total:] == BYTE_FILL).all())
        return ok

    def untouched(self):
        return self.flow.untouched() and self.inst.untouched() and all(bool((b == BYTE_FILL).all()) for b in self.bytes)


def launch(sweeps, background, dev, off=0, h_offsets=None, h_box_offsets=None, null=None):
    """``sweeps``: [(pc [N,4] f32, ego [4,4] f64, (geom, obj_flow, cls, finite))] -> (status, Outputs, offsets)"""
    import torch
    from himo_amd import _lib
    from himo_amd.extract_sca import LabelBatch
    lib = _lib.load()
    b = LabelBatch(sweeps, background, device=dev)
    out = Outputs(b.total_points, dev, off)
    ho = b.offsets_host if h_offsets is None else np.asarray(h_offsets, dtype=np.int64)
    hb = b.box_offsets_host if h_box_offsets is None else np.asarray(h_box_offsets, dtype=np.int32)
    p_flow, p_valid, p_cat, p_inst = out.ptrs()
    args = [b.n, b.total_points, ho.ctypes.data, _lib.ptr(b.offsets), _lib.ptr(b.ego), _lib.ptr(b.pc), int(b.box_offsets_host[-1]),
            hb.ctypes.data, _lib.ptr(b.box_offsets), _lib.ptr(b.geom), _lib.ptr(b.obj_flow), _lib.ptr(b.box_class), _lib.ptr(b.vel_finite),
            background, p_flow, p_valid, p_cat, p_inst, _lib.stream_handle()]
    if null is not None:
        args[null] = None
    st = lib.himo_box_label_batch(*args)
    torch.cuda.synchronize()
    return st, out, b.offsets_host


def assert_matches(sweeps, background, dev, want, off=0):
    st, out, o = launch(sweeps, background, dev, off)
    assert st == 0
    flow, valid, cat, inst = out.get()
    for k, w in enumerate(want):
        lo, hi = int(o[k]), int(o[k + 1])
        assert flow[lo:hi].tobytes() == np.asarray(w[0], np.float32).tobytes(), f"flow of sweep {k} ({hi - lo} points)"
        assert np.array_equal(valid[lo:hi], np.asarray(w[1]).astype(np.uint8)), f"flow_is_valid of sweep {k}"
        assert np.array_equal(cat[lo:hi], w[2]), f"category of sweep {k}"
        assert np.array_equal(inst[lo:hi], w[3]), f"instance of sweep {k}"
    assert out.guards_untouched()


# ---- golden ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_sweeps():
    """[(sweep for the kernel, the reference's four datasets)] of every labelled golden frame"""
    from himo_amd import extract_sca as ex
    mapping = ex.load_name_mapping(SCA / "name_mapping.json")
    with open(RAW / "metadata.pkl", "rb") as fh:
        metadata = pickle.load(fh)
    out = []
    for scene, group, annos in labelled_frames(metadata):
        seq = json.loads((RAW / scene / f"sequence_{scene.split('_')[1]}.json").read_text())
        pose0, _ = ex.get_pose_and_timestamp(seq, int(group) - 1)
        pose1, _ = ex.get_pose_and_timestamp(seq, int(group))
        with _h5().File(SCA / "h5" / f"{scene}.h5", "r") as f:
            g = f[group]
            pc = np.asarray(g["lidar"])
            want = (np.asarray(g["flow"]), np.asarray(g["flow_is_valid"]), np.asarray(g["flow_category_indices"]),
                    np.asarray(g["flow_instance_id"]))
            ego = np.linalg.inv(pose1) @ pose0
            assert np.array_equal(ego.astype(np.float32), np.asarray(g["ego_motion"]))
        out.append(((pc, ego, ex.box_table(annos, mapping, 0.2)), want))
    return out


def test_kernel_is_bit_equal_to_the_reference_h5(gpu, golden_sweeps):
    assert len(golden_sweeps) == 5
    assert any((w[3] > 0).any() and not w[1].all() for _, w in golden_sweeps)          # boxes hit, an infinite velocity among them
    assert_matches([s for s, _ in golden_sweeps], 0, gpu, [w for _, w in golden_sweeps])
    for s, w in golden_sweeps:
        assert_matches([s], 0, gpu, [w])


# ---- seeded inputs against the checker ------------------------------------------------------------------------------------------
def seeded_sweep(seed, n, m):
    rng = np.random.default_rng(seed)
    boxes = np.stack([rng.uniform(-20, 20, m), rng.uniform(-20, 20, m), rng.uniform(-1, 1, m), rng.uniform(1, 8, m), rng.uniform(0.5, 3, m),
                      rng.uniform(1, 3, m), rng.uniform(-np.pi, np.pi, m)], axis=1).reshape(m, 7)
    pts = np.stack([rng.uniform(-25, 25, n), rng.uniform(-25, 25, n), rng.uniform(-2, 5, n), rng.uniform(0, 255, n)], axis=1)
    if m and n:
        near = rng.random(n) < 0.5
        b = rng.integers(0, m, n)
        pts[near, :3] = (boxes[b, :3] + rng.uniform(-0.7, 0.7, (n, 3)) * boxes[b, 3:6] + [0, 0, 0.5] * boxes[b, 5:6])[near]
    yaw = rng.uniform(-0.2, 0.2)
    ego = np.eye(4)
    ego[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    ego[:3, 3] = rng.uniform(-2, 2, 3)
    finite = (rng.random(m) > 0.2).astype(np.uint8)
    obj_flow = (rng.uniform(-1.5, 1.5, (m, 3)) * finite[:, None]).astype(np.float32)
    cls = rng.integers(1, 31, m).astype(np.uint8)
    return pts.astype(np.float32), ego, (boxlabel_ref.box_constants(boxes), obj_flow, cls, finite)


def checker(sweeps, background):
    return [boxlabel_ref.label_sweep(pc, ego, *t, background) for pc, ego, t in sweeps]


POINTS = [0, 1, 63, 64, 65, 4097]
BOXES = [0, 1, 2, 33, 500]
BATCHES = {
    "one": [(4097, 33)],
    "three_empty_between": [(65, 2), (0, 1), (4097, 500)],
    "thirty_two_mixed": [(POINTS[k % 6], BOXES[(k // 2) % 5]) for k in range(31)] + [(1025, 0)],
    "large": [(120_000, 33), (1, 2), (120_000, 500)],
}


# (off = 1: every output one element past its alignment, which takes the element-wise path; the small sizes cover it)
@pytest.mark.parametrize("name,off", [(n, o) for n in BATCHES for o in (0, 1) if not (n == "large" and o)])
def test_kernel_is_bit_equal_to_the_checker(gpu, name, off):
    sweeps = [seeded_sweep(1000 * len(name) + k, n, m) for k, (n, m) in enumerate(BATCHES[name])]
    want = checker(sweeps, 7)
    assert any((w[3] > 0).any() for w in want)
    assert_matches(sweeps, 7, gpu, want, off)


def test_every_size_is_covered():
    cases = [c for b in BATCHES.values() for c in b]
    assert {n for n, _ in cases} >= set(POINTS) | {120_000} and {m for _, m in cases} >= set(BOXES)
    assert len(BATCHES["thirty_two_mixed"]) == 32


def test_a_sweep_without_boxes_is_background_valid_pure_pose_flow(gpu):
    sweeps = [seeded_sweep(5, 300, 4), seeded_sweep(6, 2500, 0), seeded_sweep(7, 300, 4)]
    st, out, o = launch(sweeps, 9, gpu)
    assert st == 0
    flow, valid, cat, inst = out.get()
    lo, hi = int(o[1]), int(o[2])
    pc, ego, _ = sweeps[1]
    pose_flow = (pc[:, :3] @ ego[:3, :3].T + ego[:3, -1] - pc[:, :3]).astype(np.float32)
    assert flow[lo:hi].tobytes() == pose_flow.tobytes()
    assert valid[lo:hi].all() and (cat[lo:hi] == 9).all() and not inst[lo:hi].any()
    assert (inst[:lo] > 0).any() and (inst[hi:] > 0).any()


def _hand_sweep(points, boxes):
    m = len(boxes)
    pc = np.concatenate([points, np.zeros((len(points), 1))], axis=1).astype(np.float32)
    return pc, np.eye(4), (boxlabel_ref.box_constants(boxes), np.zeros((m, 3), np.float32), np.arange(1, m + 1, dtype=np.uint8),
                           np.ones(m, np.uint8))


def test_faces_and_overlaps_on_the_device(gpu):
    pts = FACE_POINTS[:7]                                         # the exactly representable ones
    st, out, _ = launch([_hand_sweep(pts, BOX)], 0, gpu)
    assert st == 0
    assert out.get()[3].astype(np.int64).tolist() == (FACE_WANT[:7] + 1).tolist()
    boxes = np.array([[10.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0], [2.0, -1.0, 0.5, 1.0, 1.0, 1.0, 0.0], [2.0, -1.0, 0.5, 4.0, 2.0, 1.0, 0.0],
                      [2.0, -1.0, 0.5, 4.0, 2.0, 1.0, 0.5]])
    pts = np.array([[2.0, -1.0, 1.0], [3.5, -1.0, 1.0], [10.5, 0.5, 1.0], [50.0, 0.0, 1.0], [2.0, -1.0, 3.0]])
    for bx, want in ((boxes, [2, 3, 1, 0, 0]), (boxes[::-1].copy(), [1, 1, 4, 0, 0])):
        st, out, _ = launch([_hand_sweep(pts, bx)], 0, gpu)
        flow, valid, cat, inst = out.get()
        assert st == 0 and inst.tolist() == want and cat.tolist() == want and valid.all() and not flow.any()


def test_refusals_leave_the_outputs_untouched(gpu):
    from himo_amd import _lib
    sweeps = [seeded_sweep(20 + k, n, m) for k, (n, m) in enumerate([(100, 3), (50, 2), (70, 4)])]
    bad = [dict(h_offsets=[0, 100, 90, 220]), dict(h_offsets=[-5, 100, 150, 220]), dict(h_offsets=[0, 100, 150, 221]),
           dict(h_box_offsets=[0, 3, 2, 9]), dict(h_box_offsets=[0, 3, 5, 8]), dict(h_box_offsets=[1, 3, 5, 9]),
           dict(null=3), dict(null=4), dict(null=5), dict(null=9), dict(null=14), dict(null=17)]
    for kw in bad:
        st, out, _ = launch(sweeps, 0, gpu, **kw)
        assert st == _lib.ERR_INVALID_ARGUMENT, kw
        assert out.untouched(), kw
    st, out, _ = launch(sweeps, 0, gpu)
    assert st == 0 and not out.untouched()


# ---- the program -----------------------------------------------------------------------------------------------------------------
def _tree(directory):
    out = {}
    for path in sorted(Path(directory).glob("*.h5")):
        with _h5().File(path, "r") as f:
            for g in sorted(f.keys()):
                for name in sorted(f[g].keys()):
                    a = np.asarray(f[g][name])
                    out[(path.name, g, name)] = (a.dtype.str, a.shape, a.tobytes())
    return out


def test_program_end_to_end(gpu, tmp_path, capsys):
    from himo_amd import extract_sca as ex
    kw = dict(origin_data=str(RAW), metadata_pkl=str(RAW / "metadata.pkl"), output_dir=str(tmp_path / "out"), nproc=2, batch_sweeps=3,
              lidar_ext_dir=str(SCA / "lidar_ext"), name_mapping=str(SCA / "name_mapping.json"))
    ex.main(**kw)
    want, got = _tree(SCA / "h5"), _tree(tmp_path / "out")
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key][:2] == want[key][:2], key
        assert got[key][2] == want[key][2], key
    assert ("batch_12.h5", "0003", "flow") not in got and ("batch_11.h5", "0004", "flow") not in got
    index = (tmp_path / "out" / "index_total.pkl").read_bytes()
    assert len(pickle.loads(index)) == 8

    capsys.readouterr()
    ex.main(**kw)                                                  # a second run skips finished scenes
    assert capsys.readouterr().out.count("already exist, skip") == 2
    assert _tree(tmp_path / "out") == got

    (tmp_path / "out" / "index_total.pkl").unlink()
    ex.main(output_dir=str(tmp_path / "out"), create_index_only=True)
    assert (tmp_path / "out" / "index_total.pkl").read_bytes() == index


def test_process_one_writes_the_same_scene(gpu, tmp_path):
    from himo_amd import extract_sca as ex
    with open(RAW / "metadata.pkl", "rb") as fh:
        meta = [m for m in pickle.load(fh) if m["sample_idx"] == "batch_12"]
    ex.process_one(str(RAW), tmp_path, "batch_12", meta, lidar_ext_dir=str(SCA / "lidar_ext"), name_mapping=str(SCA / "name_mapping.json"))
    want = {k: v for k, v in _tree(SCA / "h5").items() if k[0] == "batch_12.h5"}
    assert _tree(tmp_path) == want
