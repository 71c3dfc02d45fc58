"""Accumulator-owned feature buffers: the measurements of DESIGN.md §16, on Cornell.

quality: §15's table again (mean squared error against a 1024-spp render of the same view, over
the whole image and, as a share of the same denominator, over the pixels with coverage > 0) with
two more columns: the plain and the variance-guided filter with split_emitters, fed by the
accumulator's own guides (every camera sample of the passes in the image) instead of the
separate feature pass (min(spp, 16) samples of seed 1).  The same two rows: 48 x 48 with 4
passes x 4 spp and 128 x 128 with 4 passes x 16 spp.

time: Cornell 800 x 800 x 16 spp, one pass (Accumulator.add) with features off, "guides" and
"emit", resolve_aov_device and the separate feature pass, alternated call by call: HIP events
around each blocking call, 5 warm-up rounds, then the median (min, max) of 25.  With
--parent-lib PATH (a librt_amd.so built from the parent commit) that library's rt_accum_add, on
a scene and an accumulator of its own, joins the alternation: the baseline of the comparison.

Prints one JSON object; -o FILE also writes it.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch  # before the library's HIP runtime initialises

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import go_raytracer_amd as rt  # noqa: E402
from go_raytracer_amd import _lib  # noqa: E402
from tools.denoise_emit_bench import buffers, feature_pass  # noqa: E402
from tools.denoise_var_bench import stat, timed  # noqa: E402


def quality(dev):
    rows = []
    for width, spp, passes in ((48, 4, 4), (128, 16, 4)):
        t, cam, w, l = rt.demo_scene("cornell")
        cam.Width, cam.SamplesPerPixel = width, spp
        d = cam.derived()
        shape = (d.height, d.width)
        mean = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
        var = torch.empty(shape, dtype=torch.float32, device=dev)
        with rt.Scene(t, w, l) as sc:
            with sc.accumulator(cam, max_passes=passes, features="emit") as acc:
                for seed in range(1, passes + 1):
                    acc.add(seed)
                acc.resolve_device(mean, var)
                own = {k: v.clone() for k, v in acc.resolve_aov_device().items()}
            aov = buffers(shape, dev)  # §15's guides: the separate feature pass of seed 1
            feature_pass(sc, cam, aov, dev, True)
            cam.SamplesPerPixel = 1024
            ref, _ = sc.render(cam, seed=9)
        cov, cov_own = aov["coverage"].cpu().numpy(), own["coverage"].cpu().numpy()
        lit = (cov > 0) | (cov_own > 0)
        images = {"mean": mean,
                  "plain": rt.denoise_device(mean, aov),
                  "guided": rt.denoise_var_device(mean, var, aov),
                  "plain_split": rt.denoise_device(mean, aov, split_emitters=True),
                  "guided_split": rt.denoise_var_device(mean, var, aov, split_emitters=True),
                  "plain_accum": rt.denoise_device(mean, own),
                  "guided_accum": rt.denoise_var_device(mean, var, own),
                  "plain_split_accum": rt.denoise_device(mean, own, split_emitters=True),
                  "guided_split_accum": rt.denoise_var_device(mean, var, own, split_emitters=True)}
        row = {"image": f"cornell {width}x{width}", "passes": passes, "spp_per_pass": spp,
               "light_pixels": int(lit.sum()), "covered_pixels_pass": int((cov == 1).sum()),
               "covered_pixels_accum": int((cov_own == 1).sum()),
               "coverage_differs_pixels": int((cov != cov_own).sum()),
               "mse": {}, "mse_on_light_pixels": {}}
        for k, x in images.items():
            e = ((x.cpu().numpy().astype(np.float64) - ref) ** 2).mean(-1)
            row["mse"][k] = float(e.mean())
            row["mse_on_light_pixels"][k] = float(e[lit].sum() / e.size)
        rows.append(row)
    return rows


def parent_adder(path, cam_c, max_passes):
    """rt_accum_add of the library at `path` on its own Cornell scene and accumulator -> a callable"""
    L = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    tree, scene, acc = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cam, w, l = _lib.RtCamera(), C.c_int(), C.c_int()
    assets = os.path.join(os.path.dirname(os.path.abspath(rt.__file__)), "..", "assets")
    assert L.rt_tree_create(C.byref(tree)) == 0 and L.rt_tree_seed(tree, 1) == 0
    assert L.rt_demo_scene(tree, b"cornell", assets.encode(), C.byref(cam), C.byref(w), C.byref(l)) == 0
    assert L.rt_scene_create(tree, w.value, l.value, C.byref(scene)) == 0
    o = _lib.RtRenderOpts()
    o.nranks = 1
    assert L.rt_accum_create(scene, C.byref(cam_c), C.byref(o), max_passes, C.byref(acc)) == 0, L.rt_last_error()
    st = _lib.RtStats()
    seed = [0]

    def call():
        seed[0] += 1
        rc = L.rt_accum_add(acc, seed[0], C.byref(st))
        assert rc == 0, L.rt_last_error()
    return call


def timing(dev, width, spp, runs, warmup, parent_lib):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = width, spp
    d = cam.derived()
    n_calls = warmup + runs
    with rt.Scene(t, w, l) as sc:
        accs = {f: sc.accumulator(cam, max_passes=n_calls + 1, features=f) for f in (None, "guides", "emit")}
        seeds = {f: [0] for f in accs}

        def adder(f):
            def call():
                seeds[f][0] += 1
                accs[f].add(seeds[f][0])
            return call
        aov = buffers((d.height, d.width), dev)
        calls = {"accum_add_ms": adder(None), "accum_add_guides_ms": adder("guides"),
                 "accum_add_emit_ms": adder("emit"),
                 "resolve_aov_device_ms": lambda: accs["emit"].resolve_aov_device(),
                 "render_aov_emit_device_ms": lambda: feature_pass(sc, cam, aov, dev, True)}
        if parent_lib:
            calls = {"parent_accum_add_ms": parent_adder(parent_lib, cam.to_c(), n_calls + 1), **calls}
        times = {k: [] for k in calls}
        for i in range(n_calls):  # alternated: one call of each per round
            for k, fn in calls.items():
                ms = timed(fn)
                if i >= warmup:
                    times[k].append(ms)
        for a in accs.values():
            a.close()
    ss = d.spp_sqrt ** 2
    res = {"image": f"cornell {d.width}x{d.height}", "spp_per_pass": ss, "runs": runs,
           "feature_pass_samples": min(ss, 16),
           "timer": "HIP events around the blocking call, median (min, max) ms"}
    res.update({k: stat(v) for k, v in times.items()})
    base = "parent_accum_add_ms" if parent_lib else "accum_add_ms"
    res["baseline"] = base
    for k in ("accum_add_ms", "accum_add_guides_ms", "accum_add_emit_ms"):
        if k != base:
            res[k.replace("_ms", "_over_baseline")] = res[k][0] / res[base][0]
            res[k.replace("_ms", "_extra_ms")] = res[k][0] - res[base][0]
    # per pixel and pass the fold reads and writes its fp64 sums: 56 B (guides) + 52 B (emit), twice
    res["state_bytes_per_pixel"] = {"guides": 56, "emit": 52}
    res["pixels"] = d.width * d.height
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.no_quality:
        res["quality"] = quality(dev)
    if not a.no_time:
        res["time"] = timing(dev, a.width, a.spp, a.runs, a.warmup, a.parent_lib)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
