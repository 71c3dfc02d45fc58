"""Cost of the pass accumulator on Cornell 800 x 800 at 16 spp.

Times rt_accum_add against rt_render_device of the same camera, alternated call by call, and
rt_accum_resolve_device and rt_accum_info_get: HIP events around each blocking call, 5 warm-up
rounds, then the median (min, max) of 25.  With --parent-lib PATH (a librt_amd.so built from
the parent commit) that library's rt_render_device joins the alternation with a scene of its
own.  Prints one JSON object; -o FILE also writes it.
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stat(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def parent_renderer(path, cam_c, out_ptr):
    """rt_render_device of the library at `path` on its own Cornell scene -> a callable"""
    L = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    tree, scene = C.c_void_p(), C.c_void_p()
    cam, w, l = _lib.RtCamera(), C.c_int(), C.c_int()
    assets = os.path.join(os.path.dirname(os.path.abspath(rt.__file__)), "..", "assets")
    assert L.rt_tree_create(C.byref(tree)) == 0 and L.rt_tree_seed(tree, 1) == 0
    assert L.rt_demo_scene(tree, b"cornell", assets.encode(), C.byref(cam), C.byref(w), C.byref(l)) == 0
    assert L.rt_scene_create(tree, w.value, l.value, C.byref(scene)) == 0
    o = _lib.RtRenderOpts()
    o.nranks = 1
    st = _lib.RtStats()
    seed = [0]

    def call():
        seed[0] += 1
        o.seed = seed[0]
        rc = L.rt_render_device(scene, C.byref(cam_c), C.byref(o), C.c_void_p(out_ptr), C.byref(st))
        assert rc == 0, L.rt_last_error()
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = a.width, a.spp
    d = cam.derived()
    img = torch.empty((d.height, d.width, 3), dtype=torch.float32, device=dev)
    rgb, var = torch.empty_like(img), torch.empty((d.height, d.width), dtype=torch.float32, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "image": f"cornell {d.width}x{d.height}",
           "spp": d.spp_sqrt ** 2, "runs": a.runs,
           "timer": "HIP events around the blocking call, median (min, max) ms"}
    with rt.Scene(t, w, l) as sc, sc.accumulator(cam) as acc:
        seed = [0]

        def render():
            seed[0] += 1
            sc.render_device(cam, img.data_ptr(), seed=seed[0])

        def add():
            seed[0] += 1
            acc.add(seed[0])
        calls = {"render_device_ms": render, "accum_add_ms": add,
                 "accum_resolve_device_ms": lambda: acc.resolve_device(rgb, var),
                 "accum_info_ms": acc.info}
        if a.parent_lib:
            calls = {"parent_render_device_ms": parent_renderer(a.parent_lib, cam.to_c(), img.data_ptr()), **calls}
        times = {k: [] for k in calls}
        for i in range(a.warmup + a.runs):  # alternated: one call of each per round
            for k, fn in calls.items():
                ms = timed(fn)
                if i >= a.warmup:
                    times[k].append(ms)
        res.update({k: stat(v) for k, v in times.items()})
        res["passes_accumulated"] = acc.passes
        res["state_bytes_per_pixel"] = 68
        res["rel_error"] = acc.info()["rel_error"]
    res["add_minus_render_ms"] = res["accum_add_ms"][0] - res["render_device_ms"][0]
    if a.parent_lib:
        res["add_minus_parent_render_ms"] = res["accum_add_ms"][0] - res["parent_render_device_ms"][0]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
