#!/usr/bin/env python3
"""Per-phase instruction budget of the featurise kernel (K1) from its gfx950 ISA.

    python tools/k1_isa_budget.py [--kernel plain|bf16|bf16x3] [--csrc DIR] > profiles/r09_k1_isa_budget_bf16x3.txt

Compiles csrc/featurize.hip with -DCOUGH_K1_MARKERS -save-temps (the markers are ISA comments between two scheduling
barriers: no instruction is added, but the scheduler cannot move instructions across a phase boundary, so the counts
are attributable -- the production build differs from this one in instruction ORDER, and in contracting the window products
into the first butterflies' FMAs across the marker between them), cuts the chosen instantiation's
instruction stream (up to the end of the function, not to the first s_endpgm: that one is the NaN clip's early return) at the
markers and counts wave-instructions per phase and class.

Dynamic counts = static counts x trips.  The P1 loop runs 26 four-frame groups over 4 waves = 6.5 iterations per wave.  Which
instructions are inside it is taken from the compiler's own block annotations ("in Loop: Header=..."), not from the position of
the markers: the loop's latch is laid out IN FRONT of its header (and of the LOOP marker), and everything behind the loop runs
once.  Everything the compiler left as a loop outside P1 is reported with its static size and back-edge so that the trip count
can be read from the source.  Sections between SKIP / ENDSKIP markers (branches that the shipped configuration never takes: PCEN,
the rescaled second P1 pass) are left out, markers inside them included.  Per clip = per wave x 4 waves.

The last lines give, per four-frame group of the P1 loop, the instructions that compute nothing: zero-moves feeding a DPP move,
register copies, s_nop, and the max instructions of the clip's peak.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shipped-geometry instantiations <PRE_EMPH = false, STEM, FULL = false, TALL = false, PCS = false, GEO = false>: all six
# template arguments, or the FULL instantiations of the same stem (defined first) match
KERNELS = {"plain": "featurize_kernelILb0ELi0ELb0ELb0ELb0ELb0EE", "bf16": "featurize_kernelILb0ELi1ELb0ELb0ELb0ELb0EE",
           "bf16x3": "featurize_kernelILb0ELi2ELb0ELb0ELb0ELb0EE"}
LATCH = "P1 loop blocks laid out in front of the header (latch)"
PEAK_PHASES = ("P1 peak + window multiply", "P1 peak + window multiply + next group's loads", LATCH)

# trip counts per wave of loops the compiler keeps rolled, by phase (from the source): (static back-edge count order)
ROLLED_TRIPS = {
    "P2 floor + mel rows store": 3232 / 256.0,          # i2 < 64*101/2 step 256
    "P2 DCT 13x64": 64 / 8.0,                            # #pragma unroll 8 over the 64 mel bands
    "P2 feature image (stem) + MFCC / delta rows": None,  # several loops: reported individually
    "K2 stem MFMA + pool + store": 8.0,                  # 16 tiles, two per iteration
}


def classify(op: str) -> str:
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith(("ds_", "s_barrier")):
        return "lds" if op.startswith("ds_") else "salu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    return "other"


def block_loops(text, start, end):
    """For every line of the kernel, the loop headers its basic block names in the compiler's annotations (a header names itself)."""
    loops, cur = {}, frozenset()
    for ln in range(start, end):
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", text[ln])
        if m:
            head, k = text[ln], ln + 1     # a block's annotations continue on the comment lines that follow its label
            while k < end and text[k].lstrip().startswith(";") and not re.match(r"^; (%bb\.|K1MARK)", text[k]):
                head += " " + text[k]
                k += 1
            names = set(re.findall(r"(?:Header=|Parent Loop )(BB\d+_\d+)", head))
            if "Loop Header" in head and m.group(1):
                names.add(m.group(1))
            cur = frozenset(names)
        loops[ln] = cur
    return loops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="bf16x3", choices=list(KERNELS))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "cough_detector_amd", "csrc"),
                    help="directory of featurize.hip (a copy of csrc/ of another revision, beside its include/)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "--offload-arch=gfx950", "-fno-slp-vectorize", "-DCOUGH_K1_MARKERS", "-c", "-save-temps",
               os.path.join(args.csrc, "featurize.hip"), "-o", os.devnull]
        subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(os.path.join(tmp, "featurize-hip-amdgcn-amd-amdhsa-gfx950.s")).read().splitlines()
    start = next(i for i, l in enumerate(text) if l.startswith("_ZN5cough") and KERNELS[args.kernel] in l.split(":")[0] and ": ; @" in l)
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    loops_of = block_loops(text, start, end)

    def markers():
        """(line, kind, body) of the markers that count: those inside a SKIP section are ignored."""
        skip = False
        for ln in range(start + 1, end):
            l = text[ln].strip()
            if not l.startswith("; K1MARK"):
                continue
            body = l[len("; K1MARK"):].strip()
            kind = body.split()[0]
            if skip and kind != "ENDSKIP":
                continue
            skip = kind == "SKIP" or (skip and kind != "ENDSKIP")
            yield ln, kind, body

    marks = {ln: (kind, body) for ln, kind, body in markers()}
    # the P1 loop: the first loop header behind the LOOP marker
    loop_ln = next(ln for ln, (kind, _) in sorted(marks.items()) if kind == "LOOP")
    loop_mult = float(marks[loop_ln][1].split()[1])
    p1 = next(m.group(1) for ln in range(loop_ln, end)
              for m in [re.match(r"^\.L(BB\d+_\d+):", text[ln])] if m and m.group(1) in loops_of[ln])

    phases, order = {}, []
    cur, cur_in_p1, skip, weight = "entry", False, False, 1.0
    rolled = {}   # loop header outside P1 -> [phase of its first instruction, VALU in its blocks]
    waste = {"zero-move feeding a DPP move": 0.0, "register copy (v_mov_b32 v, v)": 0.0, "s_nop": 0.0, "max of the peak": 0.0,
             "DPP move": 0.0}
    prev_zero = None
    for ln in range(start + 1, end):
        l = text[ln].strip()
        if l.startswith("; K1MARK"):
            if ln not in marks:
                continue
            kind, body = marks[ln]
            if kind == "PHASE":
                cur, cur_in_p1 = body[6:].strip(), p1 in loops_of[ln]
            elif kind in ("SKIP", "ENDSKIP"):
                skip = kind == "SKIP"
            elif kind == "WEIGHT":
                weight = float(body.split()[1])
            elif kind == "ENDWEIGHT":
                weight = 1.0
            continue
        if not l or l.startswith((";", ".")) and not l.startswith(".LBB"):
            continue
        if l.startswith(".LBB"):
            continue
        if skip:
            continue
        op = l.split()[0]
        in_p1 = p1 in loops_of[ln]
        mult = loop_mult if in_p1 else 1.0
        key = LATCH if in_p1 and not cur_in_p1 else cur     # P1 blocks in front of the loop's first phase marker
        if (key, mult) not in phases:
            phases[(key, mult)] = {}
            order.append((key, mult))
        c = classify(op)
        phases[(key, mult)][c] = phases[(key, mult)].get(c, 0) + weight
        if in_p1:
            mz = re.match(r"v_mov_b32_e32 (v\d+), 0$", l)
            md = re.match(r"v_mov_b32_dpp (v\d+),", l)
            if md:
                waste["DPP move"] += weight
                if prev_zero == md.group(1):
                    waste["zero-move feeding a DPP move"] += weight
            if re.match(r"v_mov_b32_e32 v\d+, v\d+$", l):
                waste["register copy (v_mov_b32 v, v)"] += weight
            if op == "s_nop":
                waste["s_nop"] += weight
            if op.startswith(("v_max_f32", "v_max3_f32")) and key in PEAK_PHASES:
                waste["max of the peak"] += weight
            if op != "s_nop":
                prev_zero = mz.group(1) if mz else None
        if not in_p1:
            for h in loops_of[ln]:
                rolled.setdefault(h, [cur, 0])[1] += c == "valu"
    print(f"# K1 instruction budget, kernel = {args.kernel} ({KERNELS[args.kernel]}), gfx950, hipcc -O3")
    print("# wave-instructions PER WAVE (x4 waves = per clip); dynamic = static x trips (P1 loop membership from the compiler's block annotations)")
    print(f"{'phase':62s} {'trips':>6s} {'VALU':>7s} {'MFMA':>6s} {'LDS':>6s} {'VMEM':>6s} {'SALU':>6s} {'SMEM':>5s} {'wait':>5s}")
    tot, p1_valu = {}, 0.0
    for k, mu in order:
        st = phases[(k, mu)]
        row = {c: st.get(c, 0) * mu for c in ("valu", "mfma", "lds", "vmem", "salu", "smem", "wait")}
        for c, v in row.items():
            tot[c] = tot.get(c, 0) + v
        if mu != 1.0:
            p1_valu += st.get("valu", 0)
        print(f"{k:62s} {mu:6.1f} {row['valu']:7.0f} {row['mfma']:6.0f} {row['lds']:6.0f} {row['vmem']:6.0f} "
              f"{row['salu']:6.0f} {row['smem']:5.0f} {row['wait']:5.0f}")
    print(f"{'TOTAL per wave (rolled loops counted ONCE, see below)':62s} {'':6s} {tot['valu']:7.0f} {tot['mfma']:6.0f} "
          f"{tot['lds']:6.0f} {tot['vmem']:6.0f} {tot['salu']:6.0f} {tot['smem']:5.0f} {tot['wait']:5.0f}")
    print("# loops the compiler kept rolled outside the P1 loop (static VALU in the loop body; multiply by trips - 1 and add):")
    extra = 0.0
    for tgt, (cur, n) in rolled.items():
        trips = ROLLED_TRIPS.get(cur)
        add = n * (trips - 1) if trips else 0.0
        extra += add
        print(f"#   phase '{cur}': loop at {tgt}: {n} VALU per iteration" + (f", {trips:.1f} trips -> +{add:.0f}" if trips else ", trips: see source"))
    print(f"# VALU per wave incl. rolled loops with known trips ~ {tot['valu'] + extra:.0f}; per clip (4 waves) ~ {4 * (tot['valu'] + extra):.0f}")
    print(f"# P1 loop ({p1}), per four-frame group (edge-frame load paths weighted): {p1_valu:.0f} VALU, of which")
    for name, v in waste.items():
        print(f"#   {name:34s} {v:6.1f}")


if __name__ == "__main__":
    main()
