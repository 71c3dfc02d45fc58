"""Feature pass and accumulator of two builds of the library, bit for bit, and their cost.

  dump FILE.npz     every output of the calls below with the library in use (RT_AMD_LIB=PATH
                    selects another build, e.g. tools/build_prev.sh's) -> FILE.npz
  compare A B [-o]  the two dumps, array by array as uint32 bits -> one line per array
  time FILE.json    rt_render_aov_device and rt_render_aov_emit_device on Cornell 800 x 800,
                    n = 4: HIP events around the blocking call, 5 warm-up calls, then
                    [median, min, max] ms of 25

Feature pass: the four rt_render_aov* entries on Cornell 40 x 30, n = 4 and on the sphere field
13 x 9, n = 1, rank 1 of 3, with each single plane wanted and with all planes wanted.
Accumulator: Cornell 37 x 23 at 16 spp; resolve, resolve_device, counts, counts_device, info,
adapt_info and tile_error after seeds 1, 2 and again after set_active(checker) + add_active(3).
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch  # before the library's HIP runtime initialises

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import go_raytracer_amd as rt  # noqa: E402

PLANES = {"albedo": 3, "normal": 3, "depth": 0, "material": 0, "emission": 3, "surface_albedo": 3, "coverage": 0}
FEATURE = ("albedo", "normal", "depth", "material")
EMIT = ("emission", "surface_albedo", "coverage")


def aov_calls(out):
    from tests.test_aov_gpu import _shape, sphere_field
    dev = torch.device("cuda", 0)
    for name, build, w, h, n, rank, nranks in (("cornell", lambda: rt.demo_scene("cornell"), 40, 30, 4, 0, 1),
                                               ("sphere_field", lambda: sphere_field(rt), 13, 9, 1, 1, 3)):
        t, cam, wd, l = build()
        _shape(cam, w, h, spp=4)
        rows = len(range(rank, h, nranks))
        with rt.Scene(t, wd, l) as sc:
            for want in [(k,) for k in PLANES] + [FEATURE, tuple(PLANES)]:
                for device in (False, True):
                    bufs = {}
                    for k in want:  # -7: what the call leaves untouched shows
                        shape = (rows, w, PLANES[k]) if PLANES[k] else (rows, w)
                        if device:
                            bufs[k] = torch.full(shape, -7, device=dev,
                                                 dtype=torch.int32 if k == "material" else torch.float32)
                        else:
                            bufs[k] = np.full(shape, -7, np.int32 if k == "material" else np.float32)
                    ptr = {k: (v.data_ptr() if device else v.ctypes.data) for k, v in bufs.items()}
                    emit = any(k in ptr for k in EMIT)
                    o = sc._opts(3, 0, rank, nranks, 0, 0, False, None)
                    sc._aov(cam, o, n, "emit" if emit else "first", device, ptr, (0, 0.0))
                    entry = "rt_render_aov" + ("_emit" if emit else "") + ("_device" if device else "")
                    for k, v in bufs.items():
                        label = f"{entry:26s} {name:12s} {w:3d} x {h:3d} n {n} rank {rank}/{nranks} wanted " \
                                f"{'+'.join(want) if len(want) < 7 else 'all':38s} {k}"
                        out[label] = v.cpu().numpy() if device else v


def accum_calls(out):
    from tests.test_accum_gpu import _shape
    dev = torch.device("cuda", 0)
    t, cam, wd, l = rt.demo_scene("cornell")
    _shape(cam)  # 37 x 23 at 16 spp: 851 pixels
    with rt.Scene(t, wd, l) as sc, sc.accumulator(cam) as acc:
        rows, W = acc.shape
        acc.add(1)
        acc.add(2)
        for stage in ("after seeds 1, 2", "after set_active(checker) + add_active(3)"):
            if stage != "after seeds 1, 2":
                acc.set_active((np.add.outer(np.arange(rows), np.arange(W)) % 2) == 0)
                acc.add_active(3)
            res = {}
            res["rt_accum_resolve rgb"], res["rt_accum_resolve var"] = acc.resolve()
            rgb = torch.full((rows, W, 3), -7.0, device=dev)
            var = torch.full((rows, W), -7.0, device=dev)
            acc.resolve_device(rgb, var)
            res["rt_accum_resolve_device rgb"], res["rt_accum_resolve_device var"] = rgb.cpu().numpy(), var.cpu().numpy()
            res["rt_accum_counts"] = acc.counts()
            cnt = torch.full((rows, W), -7, device=dev, dtype=torch.int32)
            rt.check(rt.lib().rt_accum_counts_device(acc._h(), C.c_void_p(cnt.data_ptr())))
            torch.cuda.synchronize()
            res["rt_accum_counts_device"] = cnt.cpu().numpy()
            for fn, d in (("rt_accum_info_get", acc.info()), ("rt_accum_adapt_info", acc.adapt_info())):
                for k, v in d.items():
                    res[f"{fn} {k}"] = np.array([v], np.float64)
            res["rt_accum_tile_error"] = acc.tile_error()
            for k, v in res.items():
                out[f"{k:40s} cornell  37 x  23 spp 16 {stage}"] = v


def dump(path):
    out = {}
    aov_calls(out)
    accum_calls(out)
    np.savez(path, **{f"{i:04d}|{k}": np.ascontiguousarray(v) for i, (k, v) in enumerate(out.items())})
    print(f"{len(out)} arrays -> {path} (library: {os.environ.get('RT_AMD_LIB', 'in-tree')})")


def bits(a):
    return np.frombuffer(a.tobytes(), np.uint32)


def compare(pa, pb, out_path=None):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different calls"
    lines, bad = [], 0
    for k in sorted(a.files):
        same = a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k]))
        bad += not same
        lines.append(f"{k.split('|', 1)[1]}: {'equal' if same else 'DIFFERENT'}")
    lines.append(f"{len(lines)} arrays compared as uint32 bits, {bad} different")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 1 if bad else 0


def time_aov(path):
    dev = torch.device("cuda", 0)
    t, cam, wd, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 800, 4
    d = cam.derived()
    bufs = {k: torch.empty((d.height, d.width, c) if c else (d.height, d.width), device=dev,
                           dtype=torch.int32 if k == "material" else torch.float32) for k, c in PLANES.items()}
    ptr = {k: v.data_ptr() for k, v in bufs.items()}
    res = {"device": torch.cuda.get_device_name(0), "image": f"cornell {d.width}x{d.height}", "n_samples": 4,
           "runs": 25, "warmup": 5, "library": os.environ.get("RT_AMD_LIB", "in-tree"),
           "timer": "HIP events around the blocking call, [median, min, max] ms, alternated call by call"}
    with rt.Scene(t, wd, l) as sc:
        calls = {"rt_render_aov_device_ms": lambda: sc.render_aov_device(cam, n_samples=4, **{k: ptr[k] for k in FEATURE}),
                 "rt_render_aov_emit_device_ms": lambda: sc.render_aov_device(cam, n_samples=4, **ptr)}
        times = {k: [] for k in calls}
        for i in range(30):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= 5:
                    times[k].append(e0.elapsed_time(e1))
    res.update({k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in times.items()})
    line = json.dumps(res, indent=1)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    if mode == "dump":
        dump(args[0])
    elif mode == "compare":
        sys.exit(compare(args[0], args[1], args[3] if len(args) > 3 and args[2] == "-o" else None))
    elif mode == "time":
        time_aov(args[0])
    else:
        sys.exit(__doc__)
