#!/usr/bin/env python3
"""What k_invert_band's vector pipe carries besides per-pixel arithmetic, read from the device assembly of the shipped sources.

    python3 profiles/band_vpipe_isa.py > profiles/band_vpipe_isa_new.txt      (hipcc only, no GPU)
    python3 profiles/band_vpipe_isa.py tu.s                                   (an assembly file of that compile line, kept)

xsw_invert_tu.hip is compiled for gfx950 with the build's own flags (the compile line of stage1_isa_breakdown.py: -DXSW_PAIR=0,
float32 rasters -> complex64, -gline-tables-only, which does not change the generated code).  For the four production
instantiations of k_invert_band (mono and dual-pol, direction table in LDS or in global memory, ROLE 1), for k_invert_band2 and
for k_invert_blocks -- the kernels that share wave_tail -- it prints

  * VGPRs, SGPRs, scratch and LDS bytes, as the assembler's own summary states them;
  * static VALU / SALU / VMEM / SMEM / LDS counts of stage 1, the passes and the tail.  An instruction belongs to the function
    its line-table entry names (the innermost inlined one); the small helpers that every phase calls (v_min / v_max wrappers,
    DPP minima, lane reads, the HIP headers) count for the phase of the instruction before them;
  * lane traffic: v_writelane_b32 / v_readlane_b32 in all and per VGPR -- a register that is both written and read lane by lane is
    a spill register of the scalar allocator; reads of a register that is never written lane by lane are data (rd_lane_d);
  * the slow integer multiplies of the vector pipe: v_mad_u64_u32 / v_mad_i64_i32 and v_mul_lo_u32 / v_mul_hi_u32;
  * ballots that went through data: v_cndmask_b32 x, 0, 1, mask whose result a v_cmp_ne / v_cmp_eq turns back into a mask.

Static counts: an instruction inside a loop counts once."""
import collections
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from stage1_isa_breakdown import CSRC, REPO, function_starts  # noqa: E402

KERNELS = [
    ("k_invert_band mono, table in LDS (the benchmark's)", "13k_invert_bandIffLb0ELb0ELi1ELb1EE"),
    ("k_invert_band mono, table in global memory", "13k_invert_bandIffLb0ELb0ELi1ELb0EE"),
    ("k_invert_band dual-pol, table in LDS", "13k_invert_bandIffLb1ELb0ELi1ELb1EE"),
    ("k_invert_band dual-pol, table in global memory", "13k_invert_bandIffLb1ELb0ELi1ELb0EE"),
    ("k_invert_band2 mono", "14k_invert_band2IffLb0EE"),
    ("k_invert_band2 dual-pol", "14k_invert_band2IffLb1EE"),
    ("k_invert_blocks mono", "15k_invert_blocksIffLb0EE"),
    ("k_invert_blocks dual-pol", "15k_invert_blocksIffLb1EE"),
]
HELPERS = {"vmin", "vmax", "vminf", "vmaxf", "dpp_d", "dpp_f", "seg_min_d", "wave_min_d", "rd_lane_d", "rd_lane_i", "mul24_sv", "wave_max_i",
           "ballot64", "byte_sum4", "ld", "to_db", "log10_fast"}
TAIL_FUNCS = {"wave_tail", "list_append", "mask_mark", "store_pixel", "angle_of_quotient", "hypot_glibc", "search_cr_scan", "search_cr_interval",
              "dsig_cr_at", "nearest_index_tail", "co_encode", "cr_encode", "store_opt"}
PASS_FUNCS = {"co_band_pass", "ld_co"}


def compile_asm(path):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           "-I" + CSRC, "-DXSW_PAIR=0", "-gline-tables-only", "--cuda-device-only", "-S", os.path.join(CSRC, "xsw_invert_tu.hip"), "-o", path],
                          stderr=subprocess.DEVNULL)
    return open(path).read().split("\n")


def kind_of(op):
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "SMEM"
    return "SALU" if op.startswith("s_") else "VALU"


def main():
    if len(sys.argv) > 1:  # an assembly file of the same compile line, kept from an earlier run
        text = open(sys.argv[1]).read().split("\n")
    else:
        with tempfile.TemporaryDirectory() as td:
            text = compile_asm(os.path.join(td, "tu.s"))
    files = {}
    for line in text:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"\s+"([^"]*)"', line)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3))
    headers = ("xsw_device.hpp", "xsw_band.hpp", "xsw_band2.hpp", "xsw_blocks.hpp", "xsw_codes.hpp")
    fstarts = {f: function_starts(os.path.join(CSRC, f)) for f in headers}
    band_src = open(os.path.join(CSRC, "xsw_band.hpp")).read().split("\n")
    l_passes = next(n for n, l in enumerate(band_src, 1) if "// ---- stage 2: band passes" in l)
    l_pickup = next(n for n, l in enumerate(band_src, 1) if "the workgroup's passes have settled every slot" in l)

    def phase_of(fname, line, prev):
        if fname not in fstarts:
            return prev  # the HIP headers' wrappers: whoever called them
        fn = "?"
        for n, name in fstarts[fname]:
            if n <= line:
                fn = name
        if fn in HELPERS:
            return prev
        if fn in TAIL_FUNCS:
            return "tail"
        if fn in PASS_FUNCS or fname in ("xsw_band2.hpp", "xsw_blocks.hpp"):
            return "passes"
        if fn == "band_wave":
            return "stage 1" if line < l_passes else "passes" if line < l_pickup else "tail"
        return "stage 1"

    labels = [(i, m.group(1)) for i, m in ((i, re.match(r"^(_Z\w+):", l)) for i, l in enumerate(text)) if m]
    print(__doc__)
    for title, want in KERNELS:
        hit = [(i, s) for i, s in labels if s.startswith("_ZN3xsw" + want + "EvNS_9DevTablesENS_5KArgsE")]
        if not hit:
            print(f"== {title}: not in this build\n")
            continue
        start, sym = hit[0]
        end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
        summary = {}
        for l in text[end:end + 80]:
            m = re.match(r";\s*(TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy):\s*(\d+)", l.strip())
            if m and m.group(1) not in summary:
                summary[m.group(1)] = int(m.group(2))
        counts = collections.defaultdict(collections.Counter)
        wl, rl = collections.Counter(), collections.Counter()
        slow = collections.Counter()
        sel01 = {}       # VGPR -> phase of a v_cndmask x, 0, 1 whose result is still in it
        n_sel01, pairs = 0, collections.Counter()
        cur, phase = ("?", 0), "stage 1"
        for l in text[start:end]:
            m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
            if m:
                cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
                continue
            ins = l.split(";")[0].strip()
            if not ins or ins.startswith(".") or ins.endswith(":"):
                continue
            op = ins.split()[0]
            if not re.match(r"^(v_|s_|global_|flat_|buffer_|ds_|scratch_)", op):
                continue
            phase = phase_of(cur[0], cur[1], phase)
            counts[phase][kind_of(op)] += 1
            args = [a.strip() for a in ins[len(op):].split(",")]
            if op == "v_writelane_b32":
                wl[args[0]] += 1
                counts[phase]["lane writes"] += 1
            elif op == "v_readlane_b32":
                rl[args[1]] += 1
                counts[phase]["lane reads"] += 1
            if op in ("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mul_hi_i32"):
                slow[op] += 1
                counts[phase]["slow multiplies"] += 1
            if op.startswith(("v_cmp_ne_u32", "v_cmp_eq_u32", "v_cmp_ne_i32", "v_cmp_eq_i32")):
                for a in args:
                    if a in sel01:
                        pairs[sel01.pop(a)] += 1
            elif op.startswith("v_") and args and args[0] in sel01:
                del sel01[args[0]]
            if op.startswith("v_cndmask_b32") and len(args) >= 3 and args[1] == "0" and args[2] == "1":
                sel01[args[0]] = phase
                n_sel01 += 1
        print(f"== {title}\n   {sym}")
        print(f"   VGPRs {summary.get('NumVgprs')}  AGPRs {summary.get('NumAgprs', 0)}  SGPRs {summary.get('TotalNumSgprs')}  scratch {summary.get('ScratchSize')} B"
              f"  LDS {summary.get('LDSByteSize')} B  occupancy {summary.get('Occupancy')} waves/SIMD")
        cols = ("VALU", "SALU", "VMEM", "SMEM", "LDS", "lane writes", "lane reads", "slow multiplies")
        print("   " + f"{'phase':<10s}" + "".join(f"{c:>16s}" for c in cols) + f"{'select+compare':>16s}")
        tot = collections.Counter()
        for ph in ("stage 1", "passes", "tail"):
            tot.update(counts[ph])
            print("   " + f"{ph:<10s}" + "".join(f"{counts[ph][c]:16d}" for c in cols) + f"{pairs[ph]:16d}")
        print("   " + f"{'total':<10s}" + "".join(f"{tot[c]:16d}" for c in cols) + f"{sum(pairs.values()):16d}")
        spill = sorted(r for r in wl)
        print(f"   lane traffic: v_writelane_b32 {sum(wl.values())}, v_readlane_b32 {sum(rl.values())};"
              f" spill registers (written lane by lane): {', '.join(f'{r} ({wl[r]} writes, {rl[r]} reads)' for r in spill) or 'none'};"
              f" reads of other registers (data): {sum(n for r, n in rl.items() if r not in wl)}")
        print(f"   SPILL LANE TRAFFIC: {sum(wl.values())} writes + {sum(n for r, n in rl.items() if r in wl)} reads")
        print(f"   slow multiplies: {', '.join(f'{k} {v}' for k, v in sorted(slow.items())) or 'none'}")
        print(f"   v_cndmask x, 0, 1: {n_sel01}, of which a v_cmp_ne / v_cmp_eq turns {sum(pairs.values())} back into a mask\n")


if __name__ == "__main__":
    sys.exit(main())
