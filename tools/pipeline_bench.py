"""The frame pipeline's measurements: what a frame costs a C client.

client: rtbench -S 6 -width 800 -spp 16 -passes 1 -accum-features -split-emitters -denoise-var
-temporal-emit -temporal-moments -frames 8 -orbit 1, the staged path (the host entries) against
-on-device (one rt_pipeline), the same binary, whole runs alternated: one warm-up run of each, then
--rounds of each.  Per frame after the first, from the statistics lines: ms_accum (the pass, and on
the staged path the image's resolve to the host), ms_aov (the staged path's feature resolve),
ms_reproject + ms_denoise, ms_pipeline, and ms_frame, the difference of consecutive wall_s (1 ms
steps: everything a frame costs, the PPM formatting and the file write included).  Median (min,
max) over every such frame of every run.  The images go to a temporary directory.

parent (--parent-rtbench PATH): the same line without -on-device, this build's binary against the
parent commit's, alternated in the same way.

headline (--parent-lib PATH): python bench.py --steps 20 --warmup 5 with this build's library and
with the parent's (RT_AMD_LIB), alternated --headline-rounds times.

Prints one JSON object; -o FILE also writes it.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CLI = os.path.join(REPO, "go_raytracer_amd", "rtbench")
LINE = ["-S", "6", "-width", "800", "-spp", "16", "-passes", "1", "-accum-features", "-split-emitters", "-denoise-var",
        "-temporal-emit", "-temporal-moments", "-frames", "8", "-orbit", "1"]
KEYS = ("ms_accum", "ms_aov", "ms_reproject", "ms_denoise", "ms_pipeline", "ms_render")


def stat(v):
    return [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)] if len(v) else None


def frames_of(exe, extra, tmp):
    """one whole run -> per frame after the first, the statistics line's figures and ms_frame"""
    r = subprocess.run([exe, *LINE, *extra, "-o", os.path.join(tmp, "f.ppm")], capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{exe} {extra}: exit {r.returncode}: {r.stderr[-400:]}")
    lines = [json.loads(ln) for ln in r.stderr.strip().splitlines() if ln.startswith("{")]
    out = []
    for prev, cur in zip(lines, lines[1:]):
        row = {k: cur.get(k, 0.0) for k in KEYS}
        row["ms_frame"] = (cur["wall_s"] - prev["wall_s"]) * 1e3
        out.append(row)
    return out


def alternate(variants, rounds, tmp):
    """variants: {name: (exe, extra flags)}; one warm-up run of each, then `rounds` of each in turn"""
    for exe, extra in variants.values():
        frames_of(exe, extra, tmp)
    rows = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (exe, extra) in variants.items():
            rows[name] += frames_of(exe, extra, tmp)
    return {name: dict({k: stat([r[k] for r in v]) for k in KEYS + ("ms_frame",)}, frames=len(v))
            for name, v in rows.items()}


def headline(lib, steps=20, warmup=5):
    env = dict(os.environ)
    if lib:
        env["RT_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup)], capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py: exit {r.returncode}: {r.stderr[-400:]}")
    js = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    return js["value"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-rtbench", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--headline-rounds", type=int, default=3)
    ap.add_argument("-o", default=None)
    a = ap.parse_args()
    res = {"line": "rtbench " + " ".join(LINE), "rounds": a.rounds, "stat": "[median, min, max]"}
    with tempfile.TemporaryDirectory() as tmp:
        res["client"] = alternate({"staged": (CLI, []), "on_device": (CLI, ["-on-device"])}, a.rounds, tmp)
        s, d = res["client"]["staged"], res["client"]["on_device"]
        res["client"]["staged_stages_ms"] = round(s["ms_aov"][0] + s["ms_reproject"][0] + s["ms_denoise"][0], 3)
        res["client"]["frame_speedup"] = round(s["ms_frame"][0] / d["ms_frame"][0], 2)
        if a.parent_rtbench:
            res["parent"] = alternate({"this": (CLI, []), "parent": (os.path.abspath(a.parent_rtbench), [])}, a.rounds,
                                      tmp)
            t, p = res["parent"]["this"]["ms_frame"], res["parent"]["parent"]["ms_frame"]
            res["parent"]["ms_frame_difference"] = round(t[0] - p[0], 3)
            res["parent"]["ms_frame_spread"] = round(max(t[2] - t[1], p[2] - p[1]), 3)
    if a.parent_lib:
        runs = {"this": [], "parent": []}
        for _ in range(a.headline_rounds):
            runs["this"].append(headline(None))
            runs["parent"].append(headline(os.path.abspath(a.parent_lib)))
        res["headline"] = {"unit": "Msamples/s", "runs": runs, "this": stat(runs["this"]), "parent": stat(runs["parent"])}
    text = json.dumps(res, indent=1)
    print(text)
    if a.o:
        with open(a.o, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
