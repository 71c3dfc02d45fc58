"""Media in the feature pass: the measurements of DESIGN.md §18.

quality (asserted by nothing): cornell_smoke at 4 spp x 4 passes, mean squared error against a
1024-spp render of the same camera, for the raw mean and for denoise_var fed by the
accumulator's own guides, transparent (features="emit") and first-event ("emit+media"), each
without and with split_emitters.  Three pixel sets: all pixels; pixels with scatter > 0; pixels
within 2 pixels (Chebyshev) of a smoke-box silhouette, taken from the media depth plane: a
pixel is on a silhouette when its depth differs from a 4-neighbour's by more than 10 % and one
of the two has scatter > 0.  Every figure is the sum of squared errors over the set divided by
the set's pixel count (x 3 channels).

time: rt_render_aov_media_device against rt_render_aov_emit_device (cornell_smoke 800 x 800 and
book2 800 x 800, n = 16), and one accumulator pass with "emit+media" against "emit"
(cornell_smoke 800 x 800 x 16 spp), alternated call by call: HIP events around each blocking
call, 3 warm-up rounds, then the median (min, max) of 15.

Prints one JSON object; -o FILE also writes it.  --quality-only WIDTH: the quality table alone.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library's HIP runtime initialises

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import go_raytracer_amd as rt  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stat(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def silhouette_band(depth, scatter, reach=2):
    s = scatter > 0
    edge = np.zeros(depth.shape, bool)
    for ax in (0, 1):
        a, b = np.moveaxis(depth, ax, 0), np.moveaxis(s, ax, 0)
        jump = (np.abs(a[1:] - a[:-1]) > 0.1 * np.maximum(a[1:], a[:-1])) & (b[1:] | b[:-1])
        e = np.moveaxis(edge, ax, 0)
        e[1:] |= jump
        e[:-1] |= jump
    band = np.zeros_like(edge)
    h, w = edge.shape
    for y, x in np.argwhere(edge):
        band[max(0, y - reach):min(h, y + reach + 1), max(0, x - reach):min(w, x + reach + 1)] = True
    return band


def quality(width, spp=4, passes=4, ref_spp=1024):
    """-> {"sets": pixel counts, "mse": {result: {set: mse}}} for cornell_smoke at width x width"""
    t, cam, w, l = rt.demo_scene("cornell_smoke")
    cam.Width, cam.SamplesPerPixel = width, spp
    out = {}
    guides = {}
    with rt.Scene(t, w, l) as sc:
        for feat in ("emit", "emit+media"):
            with sc.accumulator(cam, max_passes=passes, features=feat) as acc:
                for seed in range(1, passes + 1):
                    acc.add(seed)
                mean, _ = acc.resolve()
                guides[feat] = acc.resolve_aov()
                tag = "media" if feat.endswith("media") else "transparent"
                out["denoise_var_" + tag] = acc.denoise_device(split_emitters=False).cpu().numpy()
                out["denoise_var_" + tag + "_split"] = acc.denoise_device(split_emitters=True).cpu().numpy()
        out["mean"] = mean
        cam.SamplesPerPixel = ref_spp
        ref, _ = sc.render(cam, seed=9)
    g = guides["emit+media"]
    sets = {"all": np.ones(g["scatter"].shape, bool), "scatter": g["scatter"] > 0,
            "silhouette": silhouette_band(g["depth"], g["scatter"])}
    mse = {k: {s: (float(((img - ref)[m] ** 2).mean()) if m.any() else None) for s, m in sets.items()}
           for k, img in out.items()}
    return {"width": width, "spp": spp, "passes": passes, "ref_spp": ref_spp,
            "sets": {s: int(m.sum()) for s, m in sets.items()}, "mse": mse}


def feature_times(name, dev, n=16, rounds=15, warm=3):
    t, cam, w, l = rt.demo_scene(name)
    cam.Width, cam.SamplesPerPixel = 800, 16
    d = cam.derived()
    shape = (d.height, d.width)
    f3 = lambda: torch.empty(shape + (3,), dtype=torch.float32, device=dev)  # noqa: E731
    f1 = lambda: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    b = {"albedo": f3(), "normal": f3(), "depth": f1(), "emission": f3(), "surface_albedo": f3(), "coverage": f1()}
    mat = torch.empty(shape, dtype=torch.int32, device=dev)
    sca = f1()
    ptr = {k: v.data_ptr() for k, v in b.items()}
    res = {"emit": [], "media": []}
    with rt.Scene(t, w, l) as sc:
        calls = {"emit": lambda: sc.render_aov_device(cam, material=mat.data_ptr(), n_samples=n, seed=1, **ptr),
                 "media": lambda: sc.render_aov_device(cam, material=mat.data_ptr(), n_samples=n, seed=1,
                                                       scatter=sca.data_ptr(), **ptr)}
        for i in range(warm + rounds):
            for k in ("emit", "media") if i % 2 == 0 else ("media", "emit"):
                ms = timed(calls[k])
                if i >= warm:
                    res[k].append(ms)
        tree = calls["media"]()["tree_width"]
    return {"scene": name, "size": list(shape), "n": n, "tree": tree, "scatter_pixels": int((sca > 0).sum()),
            "ms_emit": stat(res["emit"]), "ms_media": stat(res["media"]),
            "ratio_of_medians": float(np.median(res["media"]) / np.median(res["emit"]))}


def pass_times(dev, rounds=15, warm=3):
    t, cam, w, l = rt.demo_scene("cornell_smoke")
    cam.Width, cam.SamplesPerPixel = 800, 16
    res = {None: [], "emit": [], "emit+media": []}
    with rt.Scene(t, w, l) as sc:
        accs = {f: sc.accumulator(cam, max_passes=4, features=f) for f in res}
        for i in range(warm + rounds):
            order = list(res) if i % 2 == 0 else list(res)[::-1]
            for f in order:
                accs[f].reset()
                ms = timed(lambda: accs[f].add(1 + i))
                if i >= warm:
                    res[f].append(ms)
        for a in accs.values():
            a.close()
    return {"scene": "cornell_smoke", "size": [800, 800], "spp": 16,
            "ms_pass_no_features": stat(res[None]), "ms_pass_emit": stat(res["emit"]),
            "ms_pass_emit_media": stat(res["emit+media"]),
            "fold_ms_emit": float(np.median(res["emit"]) - np.median(res[None])),
            "fold_ms_emit_media": float(np.median(res["emit+media"]) - np.median(res[None]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o")
    ap.add_argument("--quality-only", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    if a.quality_only:
        out = {"quality": [quality(a.quality_only)]}
    else:
        out = {"device": torch.cuda.get_device_name(0), "timing": "HIP events around each blocking call, 3 warm-up "
               "rounds, median [min, max] of 15, alternated call by call",
               "quality": [quality(48), quality(128)],
               "feature_pass": [feature_times("cornell_smoke", dev), feature_times("book2", dev)],
               "accumulator_pass": pass_times(dev)}
    js = json.dumps(out, indent=1)
    print(js)
    if a.o:
        with open(a.o, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
