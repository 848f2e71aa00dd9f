"""The kernels' fixed-order reductions, scans and segment search have ONE definition, himo_amd/csrc/blockops.h ("The fixed
summation orders and the segment search"): every translation unit that sums, scans or searches includes it, the per-stage copies it
replaced are gone from csrc/, and the loops themselves are written nowhere else.  Source text only: no GPU, no build."""
import re

from conftest import REPO

CSRC = REPO / "himo_amd" / "csrc"
# the units that call the header's sums, scans or search ...
UNITS = ("groundseg", "icpflow", "nn", "dtloss", "fastnsf", "sslloss", "rigidrefine", "nsfp", "flowmetrics", "deflowloss", "evalmetrics",
         "segiou", "dbscan", "hdbscan", "nngrid", "pillar")
# ... and the ones that reach it through compdis_math.h (flowmetrics and evalmetrics are in both lists: they also sum and scan)
THROUGH_COMPDIS_MATH = ("boxlabel", "compdis", "compdis_gt", "evalmetrics", "flowmetrics")
REMOVED = ("find_frame", "gs_find_frame", "icp_find_cluster", "find_segment", "dt_block_sum", "block_sum1", "block_sum4", "icp_block_sum",
           "rr_sum", "rr_max", "nsfp_wave_sum", "icp_clampi", "hd_takes_part")
HELPERS = ("clampi", "segment_of", "wave_sum", "wave_sum2", "shfl_xor_u64", "wave_max_u64", "wave_inclusive_scan", "tiles_before_and_all", "block_sum",
           "group_sum", "group_max_u64", "block_inclusive_scan")


def sources():
    return {p.name: p.read_text() for p in sorted(CSRC.iterdir()) if p.suffix in (".hip", ".h")}


def includes(text, header):
    return re.search(r'^#include "%s"$' % re.escape(header), text, re.M) is not None


def test_every_unit_includes_the_header():
    src = sources()
    assert includes(src["compdis_math.h"], "blockops.h") and includes(src["nngrid.h"], "blockops.h")
    for unit in UNITS:
        text = src[unit + ".hip"]
        assert includes(text, "blockops.h") or (includes(text, "compdis_math.h") and unit in THROUGH_COMPDIS_MATH) \
            or (unit == "nngrid" and includes(text, "nngrid.h")), unit
        assert any(re.search(r"\b%s\b" % h, text) for h in HELPERS), unit
    for unit in THROUGH_COMPDIS_MATH:
        text = src[unit + ".hip"]
        assert includes(text, "compdis_math.h") and "segment_of(" in text, unit


def test_the_header_defines_each_helper_once():
    text = (CSRC / "blockops.h").read_text()
    assert "namespace himo" in text and "__global__" not in text                 # device helpers only, as unionfind.h and rigid_math.h
    for h in HELPERS:
        found = re.findall(r"__device__ inline [\w ]+?\b%s\(" % h, text)
        assert len(found) == (2 if h == "block_sum" else 1), (h, found)          # block_sum: K values, and the K = 1 form
    for name, other in sources().items():
        if name != "blockops.h":
            for h in HELPERS:
                assert not re.search(r"__device__ inline [\w ]+?\b%s\(" % h, other), (name, h)


def test_the_removed_copies_are_gone():
    for name, text in sources().items():
        for old in REMOVED:
            assert not re.search(r"\b%s\b" % old, text), (name, old)


def test_the_loops_are_written_in_the_header_only():
    # the wave butterfly and the wave scan: a shuffle inside a loop over `off` / `w`.  Left where they are, by decision: the single-step
    # folds of mlpfused.hip and nsffused.hip (no loop), the SPLIT-lane argmin of nn.hip, the neighbour compare of accumulate.hip's run
    # sums, compdis.hip's wave_max(float), the root minimum of dbscan.hip and the per-cell minimum key of groundseg.hip (through
    # shfl_xor_u64) -- none of them a sum, a 64-bit maximum or a scan
    sum_loop = re.compile(r"for \(int (off|w) = 32;[^\n]*\n?[^\n]*\+=? *__shfl_xor")
    scan_loop = re.compile(r"__shfl_up\(\w+, off, 64\)")
    tree = re.compile(r"\[threadIdx\.x\] \+= \w+(\[\w+\])?\[threadIdx\.x \+ \w+\]|= sh\[threadIdx\.x\] \+ sh\[threadIdx\.x \+ s\]")
    hillis = re.compile(r"part\[threadIdx\.x - off\]")
    search = re.compile(r"while \(hi - lo > 1\)")
    for name, text in sources().items():
        for what, rx in (("butterfly sum", sum_loop), ("wave scan", scan_loop), ("float64 tree", tree), ("Hillis-Steele scan", hillis),
                         ("segment search", search)):
            hits = len(rx.findall(text))
            if name == "blockops.h":
                assert hits >= 1, what
            elif what == "float64 tree":
                # the five units whose float64 trees moved; dtloss.hip keeps its two INTEGER count trees.  (The trees of
                # evalmetrics.hip's seg_reduce_kernel -- inside a loop over records -- and of nsffused.hip have another shape and stay)
                if name in ("fastnsf.hip", "sslloss.hip", "icpflow.hip", "rigidrefine.hip", "dtloss.hip"):
                    assert hits == (2 if name == "dtloss.hip" else 0), name
            else:
                assert hits == 0, (name, what)


def test_the_shared_neighbours():
    src = sources()
    # one cell formula on the BEV search grid, one takes-part rule for the clusterings
    assert "nng_cell_x(" in src["nngrid.h"] and "nng_cell_y(" in src["nngrid.h"]
    for unit in ("nngrid.hip", "icpflow.hip"):
        assert "nng_cell_x(" in src[unit] and "inv_cell)" not in src[unit], unit
    assert "db_takes_part(" in src["unionfind.h"]
    for unit in ("dbscan.hip", "hdbscan.hip"):
        assert "db_takes_part(" in src[unit] and "x == x" not in src[unit], unit
    # the two cross-wave orders that are part of their stages' rules stay at the call sites
    assert "((s_w[0] + s_w[1]) + (s_w[2] + s_w[3]))" in src["nsfp.hip"]
    assert "((s_v[k][0] + s_v[k][1]) + s_v[k][2]) + s_v[k][3]" in src["deflowloss.hip"]
    design = (REPO / "DESIGN.md").read_text()
    assert "csrc/blockops.h" in design and "segment_of" in design and "not to be unified" in design
