"""The emission split's measurements on Cornell.

quality: mean squared error against a 1024-spp render of the same view, over the whole image
and over the pixels with coverage > 0 (their share of the image's MSE: the same denominator),
for the undenoised mean of the passes, the plain and the variance-guided filter, and both with
split_emitters, each demodulated and at its defaults; §13's two rows: 48 x 48 with 4 passes x
4 spp and 128 x 128 with 4 passes x 16 spp.

time: Cornell 800 x 800, the parent entry points against their _emit twins, alternated call by
call: HIP events around each blocking call, 5 warm-up rounds, then the median (min, max) of 25.

Prints one JSON object; -o FILE also writes it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library's HIP runtime initialises

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import go_raytracer_amd as rt  # noqa: E402
from tools.denoise_var_bench import stat, timed  # noqa: E402

PLANES = {"albedo": 3, "normal": 3, "depth": 0, "emission": 3, "surface_albedo": 3, "coverage": 0}


def buffers(shape, dev):
    return {k: torch.empty(shape + ((c,) if c else ()), dtype=torch.float32, device=dev)
            for k, c in PLANES.items()}


def feature_pass(sc, cam, aov, dev, split, n=None):
    d = cam.derived()
    p = {k: v.data_ptr() for k, v in aov.items()}
    extra = {k: p[k] for k in ("emission", "surface_albedo", "coverage")} if split else {}
    sc.render_aov_device(cam, p["albedo"], p["normal"], p["depth"], None,
                         n_samples=n or min(d.spp_sqrt ** 2, 16), seed=1,
                         stream=torch.cuda.current_stream(dev).cuda_stream, **extra)


def accumulate(sc, cam, passes, dev):
    """(mean, var, aov with the split buffers) on the device"""
    d = cam.derived()
    shape = (d.height, d.width)
    mean = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
    var = torch.empty(shape, dtype=torch.float32, device=dev)
    with sc.accumulator(cam, max_passes=passes) as acc:
        for seed in range(1, passes + 1):
            acc.add(seed)
        acc.resolve_device(mean, var)
    aov = buffers(shape, dev)
    feature_pass(sc, cam, aov, dev, True)
    return mean, var, aov


def quality(dev):
    rows = []
    for width, spp, passes in ((48, 4, 4), (128, 16, 4)):
        t, cam, w, l = rt.demo_scene("cornell")
        cam.Width, cam.SamplesPerPixel = width, spp
        with rt.Scene(t, w, l) as sc:
            mean, var, aov = accumulate(sc, cam, passes, dev)
            cam.SamplesPerPixel = 1024
            ref, _ = sc.render(cam, seed=9)
        cov = aov["coverage"].cpu().numpy()
        lit = cov > 0
        images = {"mean": mean,
                  "plain": rt.denoise_device(mean, aov),
                  "guided": rt.denoise_var_device(mean, var, aov),
                  "plain_split": rt.denoise_device(mean, aov, split_emitters=True),
                  "guided_split": rt.denoise_var_device(mean, var, aov, split_emitters=True)}
        row = {"image": f"cornell {width}x{width}", "passes": passes, "spp_per_pass": spp,
               "light_pixels": int(lit.sum()), "covered_pixels": int((cov == 1).sum()),
               "mse": {}, "mse_on_light_pixels": {}}
        for k, x in images.items():
            e = ((x.cpu().numpy().astype(np.float64) - ref) ** 2).mean(-1)
            row["mse"][k] = float(e.mean())
            row["mse_on_light_pixels"][k] = float(e[lit].sum() / e.size)
        rows.append(row)
    return rows


def timing(dev, width, spp, runs, warmup):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = width, spp
    with rt.Scene(t, w, l) as sc:
        mean, var, aov = accumulate(sc, cam, 2, dev)
        out, vout = torch.empty_like(mean), torch.empty_like(var)
        calls = {
            "render_aov_device_ms": lambda: feature_pass(sc, cam, aov, dev, False),
            "render_aov_emit_device_ms": lambda: feature_pass(sc, cam, aov, dev, True),
            "denoise_device_ms": lambda: rt.denoise_device(mean, aov, out=out, iterations=5),
            "denoise_emit_device_ms": lambda: rt.denoise_device(mean, aov, out=out, iterations=5,
                                                                split_emitters=True),
            "denoise_var_device_ms": lambda: rt.denoise_var_device(mean, var, aov, out=out, var_out=vout,
                                                                   iterations=5),
            "denoise_var_emit_device_ms": lambda: rt.denoise_var_device(mean, var, aov, out=out, var_out=vout,
                                                                        iterations=5, split_emitters=True)}
        times = {k: [] for k in calls}
        for i in range(warmup + runs):  # alternated: one call of each per round
            for k, fn in calls.items():
                ms = timed(fn)
                if i >= warmup:
                    times[k].append(ms)
    n = mean.shape[0] * mean.shape[1]
    res = {"image": f"cornell {mean.shape[1]}x{mean.shape[0]}", "iterations": 5, "runs": runs,
           "aov_samples": min(cam.derived().spp_sqrt ** 2, 16),
           "timer": "HIP events around the blocking call, median (min, max) ms"}
    res.update({k: stat(v) for k, v in times.items()})
    for a, b in (("render_aov", "render_aov_emit"), ("denoise", "denoise_emit"), ("denoise_var", "denoise_var_emit")):
        res[f"{b}_over_{a}"] = res[f"{b}_device_ms"][0] / res[f"{a}_device_ms"][0]
        res[f"{b}_extra_us"] = 1e3 * (res[f"{b}_device_ms"][0] - res[f"{a}_device_ms"][0])
    # extra bytes per pixel: the feature pass writes emission (12) + surface_albedo (12) + coverage
    # (4); the filters' prep reads emission (12) + coverage (4) more and the epilogue reads the
    # validity (4), out (12) and emission (12) and writes out (12)
    res["extra_bytes_per_pixel"] = {"render_aov_emit": 28, "denoise_emit": 16 + 40, "denoise_var_emit": 16 + 40}
    res["pixels"] = n
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.no_quality:
        res["quality"] = quality(dev)
    if not a.no_time:
        res["time"] = timing(dev, a.width, a.spp, a.runs, a.warmup)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
