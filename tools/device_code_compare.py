"""Is a tree's device code another tree's?  Per kernel: resources and instruction stream.

  python tools/device_code_compare.py emit CSRC OUTDIR [UNIT ...]   # compile CSRC's device side (or the named
                                                                    # units only) into OUTDIR
  python tools/device_code_compare.py diff PARENT_OUT NEW_OUT

`emit` compiles every device translation unit of a csrc directory with the Makefile's
flags (--cuda-device-only -S, plus the kernel-resource-usage remarks) in the default build
and in the opt-in builds a test or tool uses.  `diff` prints one line per kernel in the
form of profiles/render_host_stages_device_code.txt and ends with a RESULT line; the exit
status is 0 only if every kernel's resources and instructions are equal and the kernel
sets match.  Block labels are compared without their function number, which depends only
on a function's position in the module.  A kernel that became a template twin is compared with
its parent under the parent's name: `k<false>(args, Twin<false>)` in the new tree pairs with a
plain `k(args)` that only the parent has, and `k<A, B, false>` with the parent's `k<A, B>`.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

UNITS = ["rt_render", "rt_fused_sets", "rt_fused_map", "rt_aov", "rt_accum", "rt_multi", "rt_output", "rt_build",
         "rt_denoise", "rt_temporal", "rt_pipeline", "rt_gather"]
# units without the kernel headers: no build switch reaches them, the default build is all there is
PLAIN_UNITS = ["rt_output", "rt_build", "rt_denoise", "rt_temporal", "rt_pipeline", "rt_gather"]
NAME_MAX = 160  # a printed kernel name is cut here (hipCUB's run to kilobytes)
BUILDS = {"default": [], "bvh8": ["-DRT_BVH8_KERNELS"], "sweep": ["-DRT_SWEEP_ORDER"]}
# rt_fused_sets.hip's own flags (Makefile FUSED_SETS_FLAGS)
SETS_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]
KEYS = [("vgpr", "VGPRs", 3), ("sgpr", "TotalSGPRs", 3), ("agpr", "AGPRs", 2), ("spill", "VGPRs Spill", 2),
        ("sgpr-spill", "SGPRs Spill", 3), ("lds", "LDS Size [bytes/block]", 6),
        ("scratch", "ScratchSize [bytes/lane]", 4), ("occ", "Occupancy [waves/SIMD]", 1)]


def emit_one(csrc, out, build, unit):
    cmd = ["/opt/rocm/bin/hipcc", "-DBRUTE_WAVES=6", "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950",
           "-I../../include", "-I.", "-Wno-unused-result", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
           "-fno-slp-vectorize", "--cuda-device-only", "-S", unit + ".hip", "-o", os.path.join(out, f"{build}.{unit}.s"),
           "-Rpass-analysis=kernel-resource-usage"] + BUILDS[build] + (SETS_FLAGS if unit == "rt_fused_sets" else [])
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    with open(os.path.join(out, f"{build}.{unit}.remarks"), "w") as f:
        f.write(r.stderr)
    return build, unit, r.returncode


def emit(csrc, out, units=()):
    os.makedirs(out, exist_ok=True)
    out = os.path.abspath(out)
    jobs = [(b, u) for b in BUILDS for u in (units or UNITS)
            if os.path.exists(os.path.join(csrc, u + ".hip")) and (b == "default" or u not in PLAIN_UNITS)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda j: emit_one(csrc, out, *j), jobs))
    bad = [f"{b}.{u}" for b, u, rc in res if rc]
    print("emitted", len(res) - len(bad), "failed", bad)
    return 1 if bad else 0


def resources(path):
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*?): (.*?) \[-Rpass", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            cur = rows.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return rows


def streams(path):
    """name -> the function's instructions and labels, comments stripped, in order"""
    funcs, cur = {}, None
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(\w+):$", line)
        if m and cur is None and not m.group(1).startswith("."):
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        if re.match(r"^\.Lfunc_end\d+:$", line):
            cur = None
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", line.strip()))
    return funcs


def demangle(names, cut=True):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {k: v if len(v) <= NAME_MAX or not cut else v[:NAME_MAX] + "..." for k, v in zip(names, out)}


def base_name(name):
    """(the demangled kernel name without `void`, template arguments and argument list, its
    template arguments or None)"""
    depth, i = 0, len(name)
    while i > 0:  # the argument list: back from the end to its opening parenthesis
        i -= 1
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            break
    head = re.sub(r"^void ", "", name[:i])
    m = re.match(r"^(.*?)(<[^()]*>)$", head)
    return (m.group(1), m.group(2)) if m else (head, None)


def pair_twins(pres, nres, pins, nins, names):
    """rename the parent's plain kernel k to the new tree's k<false> where only the trees' own
    side has each"""
    full = demangle(list(dict.fromkeys(list(pres) + list(nres))), cut=False)
    for nk in [k for k in nres if k not in pres]:
        nb, nt = base_name(full[nk])
        # k<false> pairs with a plain k, k<A, B, false> with the parent's k<A, B>: a template that
        # gained a last parameter, switched off
        if nt == "<false>":
            want = (nb, None)
        elif nt and nt.endswith(", false>"):
            want = (nb, nt[:-len(", false>")] + ">")
        else:
            continue
        for pk in [k for k in pres if k not in nres]:
            if base_name(full[pk]) == want:
                print(f"   twin: {names[nk]} against the parent's {names[pk]}")
                pres[nk] = pres.pop(pk)
                if pk in pins:  # under the new name, so that only the code can differ
                    pins[nk] = [line.replace(pk, nk) for line in pins.pop(pk)]
                break


def diff(pdir, ndir):
    same = True
    for build in BUILDS:
        print(f"== build: {build}")
        for unit in UNITS:
            pr, nr = (os.path.join(d, f"{build}.{unit}.remarks") for d in (pdir, ndir))
            if not (os.path.exists(pr) or os.path.exists(nr)):
                continue
            pres, nres = (resources(p) if os.path.exists(p) else {} for p in (pr, nr))
            pins, nins = (streams(p[:-8] + ".s") if os.path.exists(p[:-8] + ".s") else {} for p in (pr, nr))
            names = demangle(list(dict.fromkeys(list(pres) + list(nres))))
            print(f"-- {unit}: parent {len(pres)} kernels, new {len(nres)} kernels")
            pair_twins(pres, nres, pins, nins, names)
            for k in pres:
                if k not in nres:
                    same = False
                    print(f"   only in parent: {names[k]}")
            for k in nres:
                if k not in pres:
                    same = False
                    print(f"   only in new:    {names[k]}")
            width = max([len(names[k]) for k in nres] + [1])
            for k, r in nres.items():
                cols = " ".join(f"{label} {r.get(key, '?'):>{w}s}" for label, key, w in KEYS)
                if k not in pres:
                    print(f"   {names[k]:{width}s} {cols}")
                    continue
                req = all(r.get(key) == pres[k].get(key) for _, key, _ in KEYS)
                ieq = k in pins and k in nins and pins[k] == nins[k]
                n = sum(1 for l in nins.get(k, []) if not l.endswith(":") and not l.startswith("."))
                same = same and req and ieq
                print(f"   {names[k]:{width}s} {cols}  resources {'equal' if req else 'DIFFER'}"
                      f"  instructions {n} {'equal' if ieq else 'DIFFER'}")
                if not ieq and k in pins and k in nins and len(pins[k]) == len(nins[k]):
                    for a, b in [(a, b) for a, b in zip(pins[k], nins[k]) if a != b][:8]:
                        print(f"      parent: {a}\n      new:    {b}")
    print("RESULT: device code is the parent's" if same else "RESULT: device code DIFFERS from the parent's")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "emit":
        sys.exit(emit(sys.argv[2], sys.argv[3], sys.argv[4:]))
    if len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
