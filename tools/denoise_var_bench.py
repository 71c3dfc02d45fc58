"""The variance-guided denoiser's measurements on Cornell.

sweep: mean squared error against a 1024-spp render of the same view for sigma_lum in
{1, 2, 4, 8, 16} (demodulated, the other options at their defaults), next to the undenoised
mean of the passes and to the plain a-trous filter at its defaults on the same mean, at
48 x 48 with 4 passes x 4 spp and at 128 x 128 with 4 passes x 16 spp.

time: Cornell 800 x 800, rt_denoise_device (5 iterations, all guides) against
rt_denoise_var_device (the same, with var_out; and without), alternated call by call: HIP
events around each blocking call, 5 warm-up rounds, then the median (min, max) of 25.

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

SIGMAS = (1.0, 2.0, 4.0, 8.0, 16.0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stat(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def accumulate(sc, cam, passes, dev):
    """(mean, var, aov) on the device: `passes` passes with seeds 1 .., the feature pass at
    min(spp, 16) samples"""
    d = cam.derived()
    shape = (d.height, d.width)
    mean = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
    var = torch.empty(shape, dtype=torch.float32, device=dev)
    with sc.accumulator(cam, max_passes=passes) as acc:
        for seed in range(1, passes + 1):
            acc.add(seed)
        acc.resolve_device(mean, var)
    aov = {"albedo": torch.empty(shape + (3,), dtype=torch.float32, device=dev),
           "normal": torch.empty(shape + (3,), dtype=torch.float32, device=dev),
           "depth": torch.empty(shape, dtype=torch.float32, device=dev)}
    sc.render_aov_device(cam, aov["albedo"].data_ptr(), aov["normal"].data_ptr(), aov["depth"].data_ptr(),
                         None, n_samples=min(d.spp_sqrt ** 2, 16), seed=1,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    return mean, var, aov


def sweep(dev):
    rows = []
    for width, spp, passes in ((48, 4, 4), (128, 16, 4)):
        t, cam, w, l = rt.demo_scene("cornell")
        cam.Width, cam.SamplesPerPixel = width, spp
        with rt.Scene(t, w, l) as sc:
            mean, var, aov = accumulate(sc, cam, passes, dev)
            cam.SamplesPerPixel = 1024
            ref, _ = sc.render(cam, seed=9)

        def mse(x):
            return float(((x.cpu().numpy().astype(np.float64) - ref) ** 2).mean())
        row = {"image": f"cornell {width}x{width}", "passes": passes, "spp_per_pass": spp,
               "mse_mean": mse(mean), "mse_plain_atrous": mse(rt.denoise_device(mean, aov)),
               "mse_var_guided": {f"{s:g}": mse(rt.denoise_var_device(mean, var, aov, sigma_lum=s))
                                  for s in SIGMAS}}
        # where the error sits: the pixels that see the light (albedo = its emission, 15) carry
        # most of it, and demodulation multiplies what leaks into them by that albedo
        light = (aov["albedo"].cpu().numpy().max(-1) > 1.5)

        def light_part(x):  # the light pixels' share of the image's mse (same denominator)
            e = ((x.cpu().numpy().astype(np.float64) - ref) ** 2).mean(-1)
            return float(e[light].sum() / e.size)
        row["light_pixels"] = int(light.sum())
        row["mse_on_light_pixels"] = {"mean": light_part(mean), "plain_atrous": light_part(rt.denoise_device(mean, aov)),
                                      "var_guided": light_part(rt.denoise_var_device(mean, var, aov))}
        row["mse_var_guided_no_demodulation"] = mse(rt.denoise_var_device(mean, var, aov, demodulate=0))
        row["mse_plain_atrous_no_demodulation"] = mse(rt.denoise_device(mean, aov, demodulate=0))
        vout = torch.empty_like(var)
        rt.denoise_var_device(mean, var, aov, var_out=vout)
        fin = torch.isfinite(var)
        row["var_mean_in"], row["var_mean_out"] = float(var[fin].mean()), float(vout[fin].mean())
        rows.append(row)
    return rows


def timing(dev, width, spp, runs, warmup):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = width, spp
    with rt.Scene(t, w, l) as sc:
        mean, var, aov = accumulate(sc, cam, 2, dev)
    out, vout = torch.empty_like(mean), torch.empty_like(var)
    calls = {"denoise_device_ms": lambda: rt.denoise_device(mean, aov, out=out, iterations=5),
             "denoise_var_device_ms": lambda: rt.denoise_var_device(mean, var, aov, out=out, var_out=vout,
                                                                    iterations=5),
             "denoise_var_device_no_var_out_ms": lambda: rt.denoise_var_device(mean, var, aov, out=out,
                                                                               iterations=5)}
    times = {k: [] for k in calls}
    for i in range(warmup + runs):  # alternated: one call of each per round
        for k, fn in calls.items():
            ms = timed(fn)
            if i >= warmup:
                times[k].append(ms)
    n = mean.shape[0] * mean.shape[1]
    res = {"image": f"cornell {mean.shape[1]}x{mean.shape[0]}", "iterations": 5, "runs": runs,
           "timer": "HIP events around the blocking call, median (min, max) ms"}
    res.update({k: stat(v) for k, v in times.items()})
    res["var_over_plain"] = res["denoise_var_device_ms"][0] / res["denoise_device_ms"][0]
    # bytes asked of L1/L2/LDS per call: prep + 5 iterations (2 tiled, 3 global) + output
    plain = n * (12 + 12 + 12 + 4 + 32 + 5 * (50 * 16 + 16) - 16 + 12 + 12)
    guided = plain + n * (4 + 2 * 9 * 16 + 3 * 9 * 4 + 4)
    res["stencil_bytes_plain"], res["stencil_bytes_var"] = plain, guided
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.no_sweep:
        res["sigma_lum_sweep"] = sweep(dev)
    if not a.no_time:
        res["time"] = timing(dev, a.width, a.spp, a.runs, a.warmup)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
