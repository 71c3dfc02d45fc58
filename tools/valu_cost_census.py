#!/usr/bin/env python3
"""Cost-weighted VALU census of one kernel (default: the C2 kernel, the early-draw shape-1 row).

Is the kernel's VALU pipe full?  SQ_INSTS_VALU / (SIMD cycles / 2) prices every instruction at
the full rate; gfx950 issues min/max, compares, selects, conversions, 32-bit multiplies,
packed fp32 and 64-bit integer ops at half rate and transcendentals at a quarter
(tools/instr_rate.hip, profiles/r6_instr_rate.jsonl).  This tool

  1. takes the gfx950 code objects out of the built library, disassembles the kernel with the
     ROCm llvm-objdump and puts every VALU instruction into a cost class (CLASSES below; an
     opcode no rule knows is listed as unknown and priced with the widest bounds, not guessed);
  2. prints the static counts per cost class, per hardware counter class and per basic block
     (blocks cut at branches and branch targets);
  3. with --pmc FILE (a <tag>_pmc_C2.json of tools/pmc_traffic.py: counters collected in runs
     of their own) prices the dynamic mix: sum over the SQ_INSTS_VALU_* classes of count x
     cost.  A counter class's cost is the static-mix-weighted mean of its opcodes' costs,
     between a low and a high issue rate per cost class; "other" (SQ_INSTS_VALU minus the
     typed counters: moves, logic, compares, selects, min/max, lane ops) is bounded from both
     sides as well: all of it at its cheapest member's low cost, all of it at its dearest
     member's high cost, and the static mix in between;
  4. divides by the launch's SIMD cycles, GRBM_GUI_ACTIVE / 8 XCDs x 1,024 SIMDs.

usage:
  python tools/valu_cost_census.py [--lib LIB.so] [--kernel SUBSTR] [--pmc PMC.json] [--json OUT]
"""
import argparse
import collections
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
# the C2 kernel: k_fused<true, 0, 0, 1, 1, false, true, COST>, the lean-cost twin first, then the
# early-draw kernel itself (RT_LEAN_COST=0; the only one of a library from before the twin)
C2_KERNELS = ["_ZN2rt7k_fusedILb1ELj0ELi0ELi1ELi1ELb0ELb1ELb1EEEvNS_6ParamsE",
              "_ZN2rt7k_fusedILb1ELj0ELi0ELi1ELi1ELb0ELb1ELb0EEEvNS_6ParamsE",
              "_ZN2rt7k_fusedILb1ELj0ELi0ELi1ELi1ELb0ELb1EEEvNS_6ParamsE"]

# cost classes: SIMD cycles per wave64 instruction with 2-4 waves issuing, (low, high) over the
# members measured in profiles/r6_instr_rate.jsonl (waves_per_simd 4 and 2)
CLASSES = {
    "full": (2.15, 2.60),     # v_add/sub/mul_f32, v_add/sub_u32, and/or/xor, shifts, v_mov_b32
    "full3": (2.60, 2.95),    # v_fma/fmac_f32, v_bitop3 and three-operand integer adds (VOP3)
    "half": (4.19, 4.80),     # min/max, compares, conversions, 32-bit multiplies, packed fp32,
                              # 64-bit integer, v_mov_b64, e64 selects, v_mbcnt, v_writelane
    "trans": (8.20, 8.45),    # v_rcp / v_sqrt / v_rsq / v_sin / v_cos / v_exp / v_log
    "lane": (6.30, 12.3),     # v_readlane / v_readfirstlane (6.3 at 4 waves, 12.3 at 2)
    "sel_vcc": (4.22, 22.9),  # v_cndmask_b32_e32 (implicit vcc): 4.2 as e64, 22.8 back to back
}
UNKNOWN = (2.15, 22.9)

# opcode (suffixes _e32/_e64/_sdwa/_dpp stripped) -> (cost class, hardware counter class)
RULES = [
    (r"v_(rcp|sqrt|rsq|sin|cos|exp|log)(_iflag)?_f32", "trans", "trans_f32"),
    (r"v_(add|sub|subrev)_f32", "full", "add_f32"),
    (r"v_pk_add_f32", "half", "add_f32"),
    (r"v_mul_f32", "full", "mul_f32"),
    (r"v_pk_mul_f32", "half", "mul_f32"),
    (r"v_(fma|fmac|fmaak|fmamk|mad|mac)_f32", "full3", "fma_f32"),
    (r"v_pk_fma_f32", "half", "fma_f32"),
    (r"v_cvt_\w+", "half", "cvt"),
    (r"v_(mad_u64_u32|mad_i64_i32|lshl_add_u64|lshlrev_b64|lshrrev_b64|ashrrev_i64|add_co_u32|addc_co_u32"
     r"|sub_co_u32|subb_co_u32)", "half", "int64"),
    (r"v_cmp\w*_[ui]64", "half", "int64"),
    (r"v_(mul_lo_u32|mul_hi_u32|mul_hi_i32|mul_u32_u24|mul_i32_i24|mad_u32_u24|mad_i32_i24)", "half", "int32"),
    (r"v_(add|sub|subrev)_u32", "full", "int32"),
    (r"v_(add3_u32|lshl_add_u32|add_lshl_u32|xad_u32|lshl_or_b32|and_or_b32|or3_b32|bfe_[ui]32|perm_b32)",
     "full3", "int32"),
    (r"v_(max|min)_[ui]32", "half", "int32"),
    (r"v_bcnt_u32_b32", "half", "int32"),
    (r"v_(lshlrev|lshrrev|ashrrev)_b?i?(32|b32|i32)", "full", "other"),
    (r"v_(and|or|xor|not)_b32", "full", "other"),
    (r"v_bitop3_b32", "full3", "other"),
    (r"v_mov_b32", "full", "other"),
    (r"v_mov_b64", "half", "other"),
    (r"v_(max|min|max3|min3|med3)_f32", "half", "other"),
    (r"v_(floor|ceil|trunc|rndne|fract)_f32", "half", "other"),
    (r"v_cmpx?_\w+", "half", "other"),
    (r"v_mbcnt_(lo|hi)_u32_b32", "half", "other"),
    (r"v_writelane_b32", "half", "other"),
    (r"v_(readlane|readfirstlane)_b32", "lane", "other"),
]
PMC_CLASSES = ["add_f32", "mul_f32", "fma_f32", "trans_f32", "int32", "int64", "cvt", "other"]


def classify(op, enc):
    if op == "v_cndmask_b32":
        return ("sel_vcc" if enc == "e32" else "half"), "other"
    for pat, cls, pmc in RULES:
        if re.fullmatch(pat, op):
            return cls, pmc
    return None, "other"


def code_objects(lib):
    """the gfx950 code objects of a library's .hip_fatbin section (clang offload bundles)"""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        objcopy = os.path.join(os.path.dirname(OBJDUMP), "llvm-objcopy")
        subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "x")], check=True)
        data = open(fat, "rb").read()
    magic, pos = b"__CLANG_OFFLOAD_BUNDLE__", 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            return
        (n,) = struct.unpack_from("<Q", data, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, ts = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + ts].decode()
            p += ts
            if "gfx950" in triple and size:
                yield data[i + off:i + off + size]
        pos = i + 24


def disassemble(lib, kernels):
    """[(address, mnemonic, branch target or None)] of the first kernel whose symbol has one of
    `kernels`, tried in their order"""
    for kernel in kernels:
        got = disassemble_one(lib, kernel)
        if got:
            return got
    raise SystemExit(f"no kernel matching {kernels} in {lib}")


def disassemble_one(lib, kernel):
    with tempfile.TemporaryDirectory() as tmp:
        for n, co in enumerate(code_objects(lib)):
            path = os.path.join(tmp, f"co{n}.hsaco")
            open(path, "wb").write(co)
            syms = subprocess.run([OBJDUMP, "-t", path], capture_output=True, text=True, check=True).stdout
            names = [l.split()[-1] for l in syms.splitlines() if kernel in l and " F " in l and not l.endswith(".kd")]
            if not names:
                continue
            out = subprocess.run([OBJDUMP, "-d", "--disassemble-symbols=" + names[0], path],
                                 capture_output=True, text=True, check=True).stdout
            base, ins = None, []
            for line in out.splitlines():
                m = re.match(r"^([0-9a-f]+) <", line)
                if m:
                    base = int(m.group(1), 16)
                    continue
                m = re.match(r"^\s+(\w+)\s*(.*?)\s*// ([0-9A-F]+):", line)
                if not m:
                    continue
                t = re.search(r"<[^>]*\+0x([0-9a-f]+)>\s*$", line)
                is_br = m.group(1).startswith(("s_cbranch", "s_branch"))
                ins.append((int(m.group(3), 16), m.group(1), base + int(t.group(1), 16) if (t and is_br) else None))
            return names[0], ins
    return None


def census(ins):
    leaders = {ins[0][0]}
    for k, (addr, op, tgt) in enumerate(ins):
        if tgt is not None:
            leaders.add(tgt)
        if (op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc"))) and k + 1 < len(ins):
            leaders.add(ins[k + 1][0])
    blocks, cur = [], None
    by_cls, by_pmc, by_op, unknown = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    mix = {p: collections.Counter() for p in PMC_CLASSES}  # counter class -> cost class -> static count
    for addr, op, _ in ins:
        if addr in leaders:
            cur = {"addr": addr, "insts": 0, "valu": 0, "cls": collections.Counter()}
            blocks.append(cur)
        cur["insts"] += 1
        if not op.startswith("v_"):
            continue
        m = re.fullmatch(r"(v_\w+?)(?:_(e32|e64|sdwa|dpp|e64_dpp))?", op)
        base, enc = m.group(1), m.group(2)
        cls, pmc = classify(base, enc)
        if cls is None:
            unknown[op] += 1
            cls = "unknown"
        by_cls[cls] += 1
        by_pmc[pmc] += 1
        by_op[op] += 1
        mix[pmc][cls] += 1
        cur["valu"] += 1
        cur["cls"][cls] += 1
    return blocks, by_cls, by_pmc, by_op, unknown, mix


def bounds(cls):
    return CLASSES.get(cls, UNKNOWN)


def price(pmc, mix):
    """cost-weighted VALU cycles per launch from a pmc_traffic.py record of the kernel"""
    g = pmc["counters_per_launch"]
    total = g["SQ_INSTS_VALU"]
    counts = {p: g.get("SQ_INSTS_VALU_" + p.upper(), 0.0) for p in PMC_CLASSES if p != "other"}
    counts["other"] = total - sum(counts.values())
    rows, lo, mid, hi = {}, 0.0, 0.0, 0.0
    for p in PMC_CLASSES:
        n = sum(mix[p].values())
        if n == 0:  # the listing has no opcode of a class the counters saw: widest bounds
            c_lo, c_hi = UNKNOWN
        else:
            c_lo = sum(k * bounds(c)[0] for c, k in mix[p].items()) / n
            c_hi = sum(k * bounds(c)[1] for c, k in mix[p].items()) / n
        c_mid = (c_lo + c_hi) / 2
        if p == "other" and n:  # both sides: all at the cheapest member, all at the dearest
            o_lo = min(bounds(c)[0] for c in mix[p])
            # (lane ops and vcc selects are a few per cent of the class: their stall cases stay out of the bound)
            common = [c for c in mix[p] if c not in ("lane", "sel_vcc")]
            o_hi = max(bounds(c)[1] for c in common) if common else c_hi
            rows[p] = {"count": counts[p], "cost_static_mix": [c_lo, c_hi], "cost_bounds": [o_lo, o_hi]}
            lo += counts[p] * o_lo
            hi += counts[p] * o_hi
        else:
            rows[p] = {"count": counts[p], "cost_static_mix": [c_lo, c_hi]}
            lo += counts[p] * c_lo
            hi += counts[p] * c_hi
        mid += counts[p] * c_mid
    simd_cycles = g["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0
    res = {"valu_insts": total, "simd_cycles": simd_cycles, "simd_cycles_per_valu": simd_cycles / total,
           "classes": rows,
           "weighted_cycles": {"lower": lo, "static_mix": mid, "upper": hi},
           "weighted_frac": {"lower": lo / simd_cycles, "static_mix": mid / simd_cycles, "upper": hi / simd_cycles},
           "frac_at_2_cycles": 2.0 * total / simd_cycles}
    if "SQ_ACTIVE_INST_VALU" in g:
        res["valu_busy_counter"] = g["SQ_ACTIVE_INST_VALU"] * 2.0 / simd_cycles
    for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_WAVE_CYCLES"):
        if k in g:
            res[k] = g[k]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=os.path.join(REPO, "go_raytracer_amd", "librt_amd.so"))
    ap.add_argument("--kernel", default=None, help="substring of the kernel's (mangled) symbol (default: the C2 kernel)")
    ap.add_argument("--pmc", default=None, help="tools/pmc_traffic.py <tag>_pmc_<config>.json of the same build")
    ap.add_argument("--json", default=None, help="write the result here")
    ap.add_argument("--blocks", type=int, default=40, help="basic blocks printed (by VALU count)")
    a = ap.parse_args()
    name, ins = disassemble(a.lib, [a.kernel] if a.kernel else C2_KERNELS)
    blocks, by_cls, by_pmc, by_op, unknown, mix = census(ins)
    nv = sum(by_cls.values())
    print(f"kernel {name}\n{len(ins)} instructions, {nv} VALU, {len(blocks)} basic blocks")
    print("static VALU by cost class (SIMD cycles per wave instruction, low-high):")
    for c, n in by_cls.most_common():
        print(f"  {c:8s} {n:5d} {100.0 * n / nv:5.1f} %  {bounds(c)[0]:.2f}-{bounds(c)[1]:.2f}")
    print("static VALU by counter class:")
    for p in PMC_CLASSES:
        print(f"  {p:9s} {by_pmc[p]:5d} {100.0 * by_pmc[p] / nv:5.1f} %  " +
              " ".join(f"{c}={k}" for c, k in mix[p].most_common()))
    print("unknown opcodes:", dict(unknown) if unknown else "none")
    s_lo = sum(n * bounds(c)[0] for c, n in by_cls.items()) / nv
    s_hi = sum(n * bounds(c)[1] for c, n in by_cls.items()) / nv
    print(f"static mean cost {s_lo:.2f}-{s_hi:.2f} cycles per VALU instruction")
    print(f"basic blocks by VALU count (the top {a.blocks}): offset, instructions, VALU, cost classes, low-cost cycles")
    for b in sorted(blocks, key=lambda b: -b["valu"])[:a.blocks]:
        cyc = sum(k * bounds(c)[0] for c, k in b["cls"].items())
        print(f"  +0x{b['addr'] - ins[0][0]:05x} {b['insts']:5d} {b['valu']:5d}  " +
              " ".join(f"{c}={k}" for c, k in b["cls"].most_common()) + f"  {cyc:.0f}")
    res = {"kernel": name, "lib": os.path.relpath(a.lib, REPO), "instructions": len(ins), "valu": nv,
           "cost_classes": {c: list(v) for c, v in CLASSES.items()},
           "static_by_cost_class": dict(by_cls), "static_by_counter_class": dict(by_pmc),
           "static_by_opcode": dict(by_op.most_common()), "unknown_opcodes": dict(unknown),
           "static_mean_cost": [s_lo, s_hi],
           "blocks": [{"offset": b["addr"] - ins[0][0], "insts": b["insts"], "valu": b["valu"], "cls": dict(b["cls"])}
                      for b in blocks if b["valu"]]}
    if a.pmc:
        with open(a.pmc) as f:
            rec = json.load(f)
        dyn = price(rec["kernels"]["k_fused"], mix)
        res["pmc_source"] = os.path.relpath(a.pmc, REPO)
        res["dynamic"] = dyn
        print(f"dynamic ({res['pmc_source']}): {dyn['valu_insts'] / 1e9:.3f} G VALU, "
              f"{dyn['simd_cycles'] / 1e9:.2f} G SIMD cycles, {dyn['simd_cycles_per_valu']:.3f} cycles available per VALU")
        for p, r in dyn["classes"].items():
            b = r.get("cost_bounds")
            print(f"  {p:9s} {r['count'] / 1e9:7.3f} G  static-mix cost {r['cost_static_mix'][0]:.2f}-{r['cost_static_mix'][1]:.2f}" +
                  (f"  bounds {b[0]:.2f}-{b[1]:.2f}" if b else ""))
        wf = dyn["weighted_frac"]
        print(f"cost-weighted VALU cycles / SIMD cycles: lower {wf['lower']:.3f}  static mix {wf['static_mix']:.3f}  "
              f"upper {wf['upper']:.3f}   (at 2 cycles each: {dyn['frac_at_2_cycles']:.3f}; "
              f"counter busy: {dyn.get('valu_busy_counter', float('nan')):.3f})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
