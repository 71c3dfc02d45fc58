"""First diffuse-hit guides: the measurements of DESIGN.md §19.

time: rt_render_aov_spec_device against rt_render_aov_device of the same build on book1 and on
cornell (no chain exists there) at 800 x 800, n = 16, by §11's protocol: HIP events around each
blocking call, 5 warm-up rounds, then the median (min, max) of 25, the two calls alternated.

quality (asserted by nothing): book1 without defocus at 128 x 128 x 16 spp, mean squared error
against a 1024-spp render of the same camera.  The image is the mean of 4 accumulator passes of
4 spp (seeds 1 .. 4), which also gives the variance; it is filtered by rt.denoise and by
rt.denoise_var, each guided by the first-hit planes and by the specular planes (n = 4, seed 1).
Two pixel sets: the whole image and the pixels with bounces > 0.

Prints one JSON object; -o FILE also writes it."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library's HIP runtime initialises

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import go_raytracer_amd as rt  # noqa: E402
from tools.aov_media_bench import stat, timed  # noqa: E402


def feature_times(name, dev, n=16, rounds=25, warm=5):
    t, cam, w, l = rt.demo_scene(name)
    cam.Width, cam.AspectRatio, cam.SamplesPerPixel = 800, 1.0, 16
    d = cam.derived()
    shape = (d.height, d.width)
    f3 = lambda: torch.empty(shape + (3,), dtype=torch.float32, device=dev)  # noqa: E731
    f1 = lambda: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    b = {"albedo": f3(), "normal": f3(), "depth": f1()}
    mat = torch.empty(shape, dtype=torch.int32, device=dev)
    bnc = f1()
    ptr = {k: v.data_ptr() for k, v in b.items()}
    res = {"first": [], "spec": []}
    with rt.Scene(t, w, l) as sc:
        calls = {"first": lambda: sc.render_aov_device(cam, material=mat.data_ptr(), n_samples=n, seed=1, **ptr),
                 "spec": lambda: sc.render_aov_device(cam, material=mat.data_ptr(), n_samples=n, seed=1,
                                                      specular=True, bounces=bnc.data_ptr(), **ptr)}
        for i in range(warm + rounds):
            for k in ("first", "spec") if i % 2 == 0 else ("spec", "first"):
                ms = timed(calls[k])
                if i >= warm:
                    res[k].append(ms)
        st0, st1 = calls["first"](), calls["spec"]()
    return {"scene": name, "size": list(shape), "n": n, "tree": st1["tree_width"],
            "chain_pixels": int((bnc > 0).sum()), "mean_bounces": float(bnc.mean()),
            "segments_first": st0["segments"], "segments_spec": st1["segments"],
            "ms_first": stat(res["first"]), "ms_spec": stat(res["spec"]),
            "ratio_of_medians": float(np.median(res["spec"]) / np.median(res["first"]))}


def quality(width=128, spp=4, passes=4, ref_spp=1024):
    t, cam, w, l = rt.demo_scene("book1")
    cam.DefocusAngle = 0.0
    cam.Width, cam.AspectRatio, cam.SamplesPerPixel = width, 1.0, spp
    with rt.Scene(t, w, l) as sc:
        with sc.accumulator(cam, max_passes=passes) as acc:
            for seed in range(1, passes + 1):
                acc.add(seed)
            mean, var = acc.resolve()
        guides = {"first": sc.render_aov(cam, n_samples=spp, seed=1),
                  "spec": sc.render_aov(cam, n_samples=spp, seed=1, specular=True)}
        cam.SamplesPerPixel = ref_spp
        ref, _ = sc.render(cam, seed=9)
    out = {"mean": mean}
    for k, g in guides.items():
        out["denoise_" + k] = rt.denoise(mean, g)
        out["denoise_var_" + k] = rt.denoise_var(mean, var, g)
    b = guides["spec"]["bounces"]
    sets = {"all": np.ones(b.shape, bool), "bounces>0": b > 0}
    mse = {k: {s: float(((img - ref)[m] ** 2).mean()) for s, m in sets.items()} for k, img in out.items()}
    return {"scene": "book1 (no defocus)", "width": width, "spp": spp * passes, "ref_spp": ref_spp,
            "sets": {s: int(m.sum()) for s, m in sets.items()}, "mse": mse}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "HIP events around each blocking call, 5 warm-up rounds, median [min, max] of 25, alternated",
           "feature_pass": [feature_times("book1", dev), feature_times("cornell", dev)],
           "quality": quality()}
    js = json.dumps(out, indent=1)
    print(js)
    if a.o:
        with open(a.o, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
