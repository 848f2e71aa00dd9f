"""Instruction mix of the fused GRU head per GRU iteration and wave, counted from the gfx950 ISA (no GPU needed).

    python scripts/count_head_isa.py [--trips 3,3] [-D HIMO_HEAD_PACKED_SLAB=0 ...] [--kernel FMT,SLABS,SAVE]

Compiles himo_amd/csrc/gruhead.hip for gfx950 to assembly (device side only), takes the kernel instantiation asked for
(default gru_head_kernel<2, 9, false>, the inference kernel of the flagship step) and counts the instructions of its `it` loop:
the depth-1 loop that holds the matrix instructions, found from the loop annotations the compiler leaves on every basic
block.  The slab loops inside it (depth 2) are not fully unrolled; their blocks are counted `--trips` times each, in the
order the loops appear (trip count = slabs in the loop / its `#pragma unroll` factor in gemm192).  The count is static: a
block that only some trips run (the weight prefetch, skipped on the last trip) counts in every trip.

Classes: matrix (v_mfma*), transcendental (v_exp / v_rcp / v_log / v_rsq / v_sqrt / v_sin / v_cos, quarter rate), packed
float32 (v_pk_*_f32, two elements per instruction; counted inside "other VALU" too), other VALU (every other v_*), LDS
stores (ds_write* / ds_store*), LDS loads (ds_read* / ds_load*), global loads, scratch accesses (register spills).
Also prints the kernel's register counts and scratch size from its metadata, and the additive cycle model of
profiles/head_instruction_diet.txt redone with the counts.
"""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
TRANS = re.compile(r"^v_(exp|rcp|log|rsq|sqrt|sin|cos)_")
CLASSES = ("matrix", "transcendental", "other VALU", "  of which packed f32", "LDS stores", "LDS loads", "global loads", "scratch", "barriers")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return ["matrix"]
    if TRANS.match(op):
        return ["transcendental"]
    if op.startswith("v_"):
        return ["other VALU", "  of which packed f32"] if re.match(r"^v_pk_\w+_f32", op) else ["other VALU"]
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return ["LDS stores"]
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return ["LDS loads"]
    if op.startswith("global_load") or op.startswith("buffer_load") or op.startswith("flat_load"):
        return ["global loads"]
    if op.startswith("scratch_"):
        return ["scratch"]
    if op == "s_barrier":
        return ["barriers"]
    return []


def kernel_lines(asm, symbol):
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel") or lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def blocks_of(lines):
    """[(label, loop header or None, depth, parent header or None, {class: count}, [opcodes])]"""
    out, cur = [], dict(label="entry", header=None, depth=0, parent=None, ops=[])
    for i, l in enumerate(lines):
        m = re.match(r"^\.L(BB\d+_\d+):\s*(;.*)?$", l)
        if m:
            out.append(cur)
            note = (m.group(2) or "") + " " + (lines[i + 1] if i + 1 < len(lines) and lines[i + 1].lstrip().startswith(";") else "")
            cur = dict(label=m.group(1), header=None, depth=0, parent=None, ops=[])
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            p = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", note)
            t = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", note)
            if t:
                cur["header"], cur["depth"] = m.group(1), int(t.group(1))
                if p:
                    cur["parent"] = p.group(1)
            elif h:
                cur["header"], cur["depth"] = h.group(1), int(h.group(2))
            continue
        s = l.strip()
        if not s or s.startswith(";") or s.startswith("."):
            continue
        cur["ops"].append(s.split()[0])
    out.append(cur)
    return out


def count(ops):
    c = dict.fromkeys(CLASSES, 0)
    for op in ops:
        for k in classify(op):
            c[k] += 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trips", default="3,3", help="trip counts of the slab loops inside the it loop, in order of appearance")
    ap.add_argument("--kernel", default="2,9,0", help="FMT,SLABS,SAVE of the instantiation")
    ap.add_argument("-D", action="append", default=[], help="preprocessor definitions passed to the compiler")
    ap.add_argument("--asm", help="count this assembly file instead of compiling")
    ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
    ap.add_argument("--hist", action="store_true", help="also print the opcode histogram of the it loop (trips applied)")
    a = ap.parse_args()
    fmt, slabs, save = (int(v) for v in a.kernel.split(","))
    symbol = f"_ZN4himo15gru_head_kernelILi{fmt}ELi{slabs}ELb{save}EEEvNS_11GruHeadArgsENS_12GruHeadBatchENS_11GruHeadSaveE"
    if a.asm:
        asm = Path(a.asm).read_text()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = Path(d) / "gruhead.s"
            cmd = [a.hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", *(f"-D{v}" for v in a.D),
                   str(REPO / "himo_amd" / "csrc" / "gruhead.hip"), "-o", str(out)]
            subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
            asm = out.read_text()
    blocks = blocks_of(kernel_lines(asm, symbol))
    # loop tree: header -> parent header
    parent = {b["header"]: b["parent"] for b in blocks if b["header"] and b["label"] == b["header"]}
    member = lambda b, h: b["header"] == h
    inner_of = lambda h: [k for k, p in parent.items() if p == h]
    mfma_in = lambda h: sum(count(b["ops"])["matrix"] for b in blocks if member(b, h) or b["header"] in inner_of(h))
    tops = [h for h, p in parent.items() if p is None]
    it = max(tops, key=mfma_in)
    inner = inner_of(it)                                  # in order of appearance (dict order = block order)
    trips = [int(v) for v in a.trips.split(",")]
    if len(trips) != len(inner):
        sys.exit(f"the it loop holds {len(inner)} inner loops, --trips names {len(trips)}")
    total = dict.fromkeys(CLASSES, 0)
    print(f"kernel gru_head_kernel<{fmt}, {slabs}, {'true' if save else 'false'}>  defines: {' '.join(a.D) or '(none)'}")
    body = count([op for b in blocks if member(b, it) for op in b["ops"]])
    print(f"  it loop {it}: blocks outside the slab loops, once per iteration")
    for k in CLASSES:
        total[k] += body[k]
    for h, t in zip(inner, trips):
        c = count([op for b in blocks if member(b, h) for op in b["ops"]])
        print(f"  slab loop {h}: {c['matrix']} matrix / {c['other VALU']} VALU / {c['LDS loads']} LDS loads / {c['global loads']} global loads per trip, x {t} trips")
        for k in CLASSES:
            total[k] += c[k] * t
    if a.hist:
        hist = {}
        for b in blocks:
            w = 1 if member(b, it) else trips[inner.index(b["header"])] if b["header"] in inner else 0
            for op in b["ops"]:
                if w:
                    hist[op] = hist.get(op, 0) + w
        for op, n in sorted(hist.items(), key=lambda kv: -kv[1]):
            print(f"      {n:5d} {op}")
    print("  per GRU iteration and wave:")
    for k in CLASSES:
        print(f"    {k:24s} {total[k]:6d}")
    meta = next(c for c in re.split(r"\n  - (?=\.)", asm[asm.index("amdhsa.kernels:"):]) if re.search(rf"\.name:\s+{symbol}\n", c))
    for key in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        m = re.search(rf"\n\s*\.{key}:\s*(\d+)", "\n" + meta)
        if m:
            print(f"    {key:28s} {m.group(1)}")
    # the additive model: a 32x32x16 matrix instruction holds the pipe 8 passes x 4 cycles = 32 cycles (16 at K = 8 ... not used here);
    # a VALU instruction issues in 4 cycles for 64 lanes, a transcendental in 16; three waves share a SIMD
    mx, va = total["matrix"] * 32, (total["other VALU"]) * 4 + total["transcendental"] * 16
    print(f"    model: matrix {mx} cycles, vector {va} cycles per wave; x 3 waves per SIMD: {3 * mx} + {3 * va} = {3 * (mx + va)}")


if __name__ == "__main__":
    main()
