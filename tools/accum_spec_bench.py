"""Temporal history for mirrors: the measurements of DESIGN.md §23.

fold: one pass (Accumulator.add) with features "emit" and "emit+spec", alternated call by call, on
Cornell 800 x 800 x 16 spp (no specular surface: the chain fold retraces first hits only) and on
book1 (mirrors, fuzzy metals, glass; --book-width wide, 16 spp, no lens).  HIP events around each
blocking call, warm-up rounds, then the median (min, max).  With --parent-lib PATH (a librt_amd.so
built from the parent commit) that library's rt_accum_add with the "emit" planes, on a scene and an
accumulator of its own, joins the alternation: the baseline of the comparison.

reproject: reproject_clip_device against reproject_spec_device at 800 x 800 in the emit mode, on two
one-pass frames of `quads` a 3 degree step apart, alternated; the spec call is fed the chain planes
and bounces, the clip call the first hit's.

quality: §22's tables with two more columns.  `quads` 128 x 128, an 8-frame orbit, ONE pass x 4 spp
per frame, steps of 1, 2 and 3 degrees, and `cornell`; mean squared error of the last frame against a
1024-spp render over all pixels, the metal quad's and the rest, for the frame, the history, history +
clip, history + specular and history + specular + clip, each also through the split variance-guided
filter; the share of metal pixels that found a history, and of those whose chains end in a miss (all
samples: depth 0; some: a mean normal shorter than 1), which have no surface to reproject.

Prints one JSON object; -o FILE also writes it.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch  # before the library's HIP runtime initialises

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import go_raytracer_amd as rt  # noqa: E402
from go_raytracer_amd import _lib  # noqa: E402
from tools.denoise_var_bench import stat, timed  # noqa: E402

FRAMES = 8


def orbit(cam, degrees):
    """rtbench's -orbit: look_from turned about the vup axis through look_at"""
    frm, at, up = (np.array(x, np.float64) for x in cam._pos)
    k = up / np.linalg.norm(up)
    v, th = frm - at, math.radians(degrees)
    out = type(cam).from_c(cam.to_c())
    out.PositionCamera(at + v * math.cos(th) + np.cross(k, v) * math.sin(th) + k * (k @ v) * (1 - math.cos(th)), at, up)
    return out


def parent_adder(path, scene_name, cam_c, max_passes):
    """rt_accum_add with the "emit" planes of the library at `path`, on its own scene -> a callable"""
    L = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    tree, scene, acc = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cam, w, l = _lib.RtCamera(), C.c_int(), C.c_int()
    assets = os.path.join(os.path.dirname(os.path.abspath(rt.__file__)), "..", "assets")
    assert L.rt_tree_create(C.byref(tree)) == 0 and L.rt_tree_seed(tree, 1) == 0
    assert L.rt_demo_scene(tree, scene_name.encode(), assets.encode(), C.byref(cam), C.byref(w), C.byref(l)) == 0
    assert L.rt_scene_create(tree, w.value, l.value, C.byref(scene)) == 0
    o = _lib.RtRenderOpts()
    o.nranks = 1
    assert L.rt_accum_create(scene, C.byref(cam_c), C.byref(o), max_passes, C.byref(acc)) == 0, L.rt_last_error()
    assert L.rt_accum_set_features(acc, _lib.RT_ACCUM_FEAT_GUIDES | _lib.RT_ACCUM_FEAT_EMIT) == 0, L.rt_last_error()
    st = _lib.RtStats()
    seed = [0]

    def call():
        seed[0] += 1
        assert L.rt_accum_add(acc, seed[0], C.byref(st)) == 0, L.rt_last_error()
    return call


def fold(scene_name, width, spp, runs, warmup, parent_lib):
    t, cam, w, l = rt.demo_scene(scene_name)
    cam.Width, cam.SamplesPerPixel, cam.DefocusAngle = width, spp, 0.0
    d = cam.derived()
    n_calls = warmup + runs
    with rt.Scene(t, w, l) as sc:
        accs = {f: sc.accumulator(cam, max_passes=n_calls + 1, features=f) for f in ("emit", "emit+spec")}
        seeds = {f: [0] for f in accs}

        def adder(f):
            def call():
                seeds[f][0] += 1
                accs[f].add(seeds[f][0])
            return call
        calls = {"accum_add_emit_ms": adder("emit"), "accum_add_emit_spec_ms": adder("emit+spec")}
        if parent_lib:
            calls = {"parent_accum_add_emit_ms": parent_adder(parent_lib, scene_name, cam.to_c(), n_calls + 1), **calls}
        times = {k: [] for k in calls}
        for i in range(n_calls):  # alternated: one call of each per round
            for k, fn in calls.items():
                ms = timed(fn)
                if i >= warmup:
                    times[k].append(ms)
        bounces = accs["emit+spec"].resolve_aov_spec()["bounces"]
        for a in accs.values():
            a.close()
    res = {"image": f"{scene_name} {d.width}x{d.height}", "spp_per_pass": d.spp_sqrt ** 2, "runs": runs,
           "timer": "HIP events around the blocking call, median (min, max) ms",
           "mean_bounces": float(bounces.mean()), "pixels_with_a_chain": float((bounces > 0).mean())}
    res.update({k: stat(v) for k, v in times.items()})
    base = "parent_accum_add_emit_ms" if parent_lib else "accum_add_emit_ms"
    res["baseline"] = base
    for k in ("accum_add_emit_ms", "accum_add_emit_spec_ms"):
        if k != base:
            res[k.replace("_ms", "_over_baseline")] = res[k][0] / res[base][0]
            res[k.replace("_ms", "_extra_ms")] = res[k][0] - res[base][0]
    res["state_bytes_per_pixel"] = {"guides": 56, "emit": 52, "spec": 40}
    return res


def _frame(sc, cam, seed):
    """one pass of features="emit+spec" -> (the first-hit frame dict, the chain frame dict), device tensors"""
    dev = torch.device("cuda", 0)
    with sc.accumulator(cam, max_passes=1, features="emit+spec") as acc:
        acc.add(seed)
        h, w = acc.shape
        rgb, var = torch.empty((h, w, 3), device=dev), torch.empty((h, w), device=dev)
        acc.resolve_device(rgb, var)
        first = {k: v.clone() for k, v in acc.resolve_aov_device().items()}
        chain = {k: v.clone() for k, v in acc.resolve_aov_spec_device().items()}
    base = {"rgb": rgb, "var": var, "count": 1.0, "emission": first["emission"], "coverage": first["coverage"]}
    return dict(base, normal=first["normal"], depth=first["depth"]), dict(base, **chain)


def reproject(width, runs, warmup):
    t, cam, w, l = rt.demo_scene("quads")
    cam.Width, cam.SamplesPerPixel = width, 4
    with rt.Scene(t, w, l) as sc:
        cam1 = orbit(cam, 3.0)
        f0, c0 = _frame(sc, cam, 1)
        f1, c1 = _frame(sc, cam1, 11)
    lum2 = torch.zeros_like(f0["var"])
    f0, c0 = dict(f0, lum2=lum2), dict(c0, lum2=lum2)
    out = {k: torch.empty_like(v) for k, v in (("rgb", f0["rgb"]), ("var", lum2), ("count", lum2), ("lum2", lum2))}
    res = {"image": f"quads {tuple(lum2.shape)[1]}x{tuple(lum2.shape)[0]}", "mode": "emit", "runs": runs,
           "timer": "HIP events around the blocking call, median (min, max) ms"}
    calls = {}
    for name, gamma in (("clip", 0.0), ("no_clamp", None)):
        if gamma is None:
            calls["reproject_moments_device_ms"] = lambda: rt.reproject_moments_device("emit", cam, f0, cam1, f1, out=out)
        else:
            calls["reproject_clip_device_ms"] = lambda: rt.reproject_clip_device("emit", cam, f0, cam1, f1, out=out)
        calls[f"reproject_spec_device_{name}_ms"] = (lambda g: lambda: rt.reproject_spec_device(
            "emit", cam, c0, cam1, c1, out=out, gamma=g))(gamma)
    times = {k: [] for k in calls}
    for i in range(warmup + runs):
        for k, fn in calls.items():
            ms = timed(fn)
            if i >= warmup:
                times[k].append(ms)
    res.update({k: stat(v) for k, v in times.items()})
    res["spec_over_clip"] = res["reproject_spec_device_clip_ms"][0] / res["reproject_clip_device_ms"][0]
    res["spec_over_moments"] = res["reproject_spec_device_no_clamp_ms"][0] / res["reproject_moments_device_ms"][0]
    return res


def quality(scene_name, step, width=128):
    t, cam, w, l = rt.demo_scene(scene_name)
    cam.Width, cam.SamplesPerPixel = width, 4
    kw = dict(split_emitters=True, moments=True)
    objs = {"history": rt.Temporal(**kw), "history + clip": rt.Temporal(clip=True, **kw),
            "history + specular": rt.Temporal(specular=True, **kw),
            "history + specular + clip": rt.Temporal(specular=True, clip=True, **kw)}
    with rt.Scene(t, w, l) as sc:
        for k in range(FRAMES):
            camk = orbit(cam, step * k)
            with sc.accumulator(camk, max_passes=1, features="emit+spec") as acc:
                acc.add(10 * k + 1)
                res = {n: tuple(x.cpu().numpy().copy() for x in o.push(acc)) for n, o in objs.items()}
                if k == FRAMES - 1:
                    mean, _ = acc.resolve()
                    aov = acc.resolve_aov_device()
                    filt = {n + ", filtered": rt.denoise_var_device(
                        torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[1]).cuda(), aov,
                        split_emitters=True).cpu().numpy() for n, x in res.items()}
                    chain = acc.resolve_aov_spec()
                    bounces = chain["bounces"]
        material = sc.render_aov(camk)["material"]
        camk.SamplesPerPixel = 1024
        ref, _ = sc.render(camk, seed=977)
    fin = np.isfinite(mean).all(-1) & np.isfinite(ref).all(-1)
    metal = material == _lib.RT_MAT_METAL
    sets = {"all": fin, "metal": fin & metal, "rest": fin & ~metal}
    cols = dict({"frame": mean}, **{n: x[0] for n, x in res.items()}, **filt)
    row = {"image": f"{scene_name} {mean.shape[1]}x{mean.shape[0]}", "frames": FRAMES, "step_degrees": step,
           "spp_per_frame": 4, "pixels": {r: int(m.sum()) for r, m in sets.items()},
           "mse": {r: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) if m.any() else None
                       for c, x in cols.items()} for r, m in sets.items()}}
    if sets["metal"].any():
        m = sets["metal"]
        row["metal_pixels_with_history"] = {n: float((x[2][m] > 1.5).mean()) for n, x in res.items()}
        row["metal_pixels_with_fractional_bounces"] = float((bounces[m] % 1 != 0).mean())
        # a chain that ends in a miss has depth 0: no surface, so no history, as for a directly seen miss
        row["metal_pixels_whose_chain_has_a_miss"] = float(((chain["normal"][m] ** 2).sum(-1) < 0.999).mean())
        row["metal_pixels_whose_chain_misses_entirely"] = float((chain["depth"][m] == 0).mean())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--book-width", type=int, default=400)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.no_time:
        res["fold"] = [fold("cornell", a.width, a.spp, a.runs, a.warmup, a.parent_lib),
                       fold("book1", a.book_width, a.spp, a.runs, a.warmup, a.parent_lib)]
        res["reproject"] = reproject(a.width, a.runs, a.warmup)
    if not a.no_quality:
        res["quality"] = [quality("quads", s) for s in (3.0, 2.0, 1.0)] + [quality("cornell", 1.0)]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
