"""Cost of adaptive passes on Cornell 800 x 800 at 16 spp.

Times, alternated call by call: rt_accum_add of a library built from the parent commit
(--parent-lib PATH, optional), this build's rt_accum_add (on an accumulator that takes whole passes only, and on the one the
active passes go to, which folds with per-pixel counts), rt_accum_add_active with 100 / 50 /
10 / 1 % of the 8 x 8 tiles active (chosen by a fixed random draw, set through
rt_accum_set_active outside the timed region) and rt_accum_select alone.  HIP events around
each blocking call, 5 warm-up rounds, then the median (min, max) of 25.  Prints one JSON
object; -o FILE also writes it (profiles/adaptive.json).
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


def parent_adder(path, cam_c):
    """rt_accum_add of the library at `path` on its own Cornell scene and accumulator"""
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
    assert L.rt_accum_create(scene, C.byref(cam_c), C.byref(o), 0, C.byref(acc)) == 0, L.rt_last_error()
    st = _lib.RtStats()
    seed = [0]

    def call():
        seed[0] += 1
        rc = L.rt_accum_add(acc, seed[0], C.byref(st))
        assert rc == 0, L.rt_last_error()
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tile", type=int, default=8)
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = a.width, a.spp
    d = cam.derived()
    res = {"device": torch.cuda.get_device_name(0), "image": f"cornell {d.width}x{d.height}",
           "spp": d.spp_sqrt ** 2, "runs": a.runs, "tile": a.tile,
           "timer": "HIP events around the blocking call, median (min, max) ms"}
    ty, tx = -(-d.height // a.tile), -(-d.width // a.tile)
    order = np.random.default_rng(1).permutation(ty * tx)
    masks = {}
    for pct in (100, 50, 10, 1):
        tiles = np.zeros(ty * tx, bool)
        tiles[order[: max(1, ty * tx * pct // 100)]] = True
        m = np.repeat(np.repeat(tiles.reshape(ty, tx), a.tile, 0), a.tile, 1)[: d.height, : d.width]
        masks[pct] = np.ascontiguousarray(m)
    # `uni` takes whole passes only (it stays uniform: the parent's kernels), `acc` the rest
    with rt.Scene(t, w, l) as sc, sc.accumulator(cam) as uni, sc.accumulator(cam) as acc:
        seed = [0]

        def add_uniform():
            seed[0] += 1
            uni.add(seed[0])

        def add():
            seed[0] += 1
            acc.add(seed[0])

        def active():
            seed[0] += 1
            acc.add_active(seed[0])
        calls = {"accum_add_ms": (None, add_uniform), "accum_add_per_pixel_ms": (None, add)}
        for pct, m in masks.items():
            calls[f"add_active_{pct}pct_ms"] = (lambda m=m: acc.set_active(m), active)
        calls["select_ms"] = (None, lambda: acc.select(0.05, tile=a.tile))
        if a.parent_lib:
            calls = {"parent_accum_add_ms": (None, parent_adder(a.parent_lib, cam.to_c())), **calls}
        times = {k: [] for k in calls}
        for i in range(a.warmup + a.runs):  # alternated: one call of each per round
            for k, (prep, fn) in calls.items():
                if prep:
                    prep()
                ms = timed(fn)
                if i >= a.warmup:
                    times[k].append(ms)
        res.update({k: stat(v) for k, v in times.items()})
        res["active_pixels"] = {str(p): int(m.sum()) for p, m in masks.items()}
        res["passes"] = acc.passes
    whole = res["accum_add_ms"][0]
    res["share_of_whole_pass"] = {str(p): res[f"add_active_{p}pct_ms"][0] / whole for p in masks}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
