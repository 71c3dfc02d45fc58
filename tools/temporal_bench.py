"""Temporal reprojection's measurements on Cornell.

time: Cornell 800 x 800, two cameras 1 degree apart on the orbit, 2 passes x 4 spp each, resolved
on the device; rt_reproject_device (in place, all three outputs) against the guided filter
rt_denoise_var_device (5 iterations, all guides) on the same frame and against a device-to-device
copy of the bytes the reprojection moves (about 100 per pixel, read and written: 50 copied),
alternated call by call: HIP events around each blocking call, 5 warm-up rounds, then the median
(min, max) of 25.  rt_reproject_emit_device (the accumulators with features="emit", their emission
and coverage planes in both frames) is timed in the same alternation, and so is
rt_reproject_light_device (the same reads, 16 more bytes written per pixel).

quality: Cornell 128 x 128, an 8-frame orbit of 1 degree per frame, 2 passes x 4 spp per frame
(features="emit"), against a 1024-spp render of the last camera: mean squared error of the last
frame's own mean, of the temporal result, of the guided filter on the frame's mean, and of the
guided filter on the temporal result, over every pixel, over the rim pixels of directly seen
lights (0 < coverage < 1), over the pixels that found history, and split into the pixels within
2 of a directly seen light (the bilinear taps mix the emitter into its coplanar surroundings:
depth and normal cannot tell them apart) and the pixels elsewhere.  The same orbit is pushed through
Temporal(split_emitters=True) as well: the columns temporal_emit and temporal_emit_guided_filter;
and through Temporal(split_emitters=True, light_history=True), whose filter is given the blended
emission and coverage: the columns temporal_light and temporal_light_guided_filter.  rim_share_of_
squared_error is, per column, the rim pixels' part of the summed squared error over all pixels.

moments: rt_reproject_moments_device joins the time alternation in each mode, once
with its defaults (both frames count 2, so K = 2 < min_frames and every pixel runs the 7 x 7
window: the worst case) and once with var_radius = -1 (no window: what the moment plane alone
costs).  quality_one_pass is the same orbit with ONE pass x 4 spp per frame through
Temporal(split_emitters=True) and Temporal(split_emitters=True, moments=True), each followed by
the guided filter.

clip: rt_reproject_clip_device joins the time alternation in each mode with the
moments' worst-case frames (clip_*), and both entries once more with a previous count of 16, a
steady orbit's (K = 9 >= min_frames: the moments entry skips the window wherever it finds history,
the clip entry runs it in every lane: *_steady).  quality_clip holds, per scene and orbit step, the
one-pass orbit through Temporal(split_emitters=True, moments=True) without and with clip=True at
every gamma of the sweep, with and without the guided filter: `quads` (rows: all pixels, the pixels
whose first hit is the metal quad, the rest) at 1 and 3 degrees per frame, and `cornell` (§21's
rows) at 1 degree.  gamma_sweep sums, per gamma, the all-pixel MSE after the filter over the two
orbits (quads at --sweep-degrees, cornell at 1 degree); the lowest sum names the default.

Prints one JSON object; -o FILE also writes it.  --only time|quality|clip runs one part.
"""
import argparse
import json
import math
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


def orbit(cam, degrees):
    """look_from turned about the vup axis through look_at (rtbench's -orbit)"""
    frm, at, up = (np.array(x, np.float64) for x in cam._pos)
    k = up / np.linalg.norm(up)
    v, th = frm - at, math.radians(degrees)
    out = type(cam).from_c(cam.to_c())
    out.PositionCamera(at + v * math.cos(th) + np.cross(k, v) * math.sin(th) + k * (k @ v) * (1 - math.cos(th)), at, up)
    return out


def frame_tensors(sc, cam, seeds, dev):
    h = w = cam.Width
    f = {k: torch.empty((h, w, 3) if k in ("rgb", "normal") else (h, w), dtype=torch.float32, device=dev)
         for k in ("rgb", "var", "normal", "depth")}
    with sc.accumulator(cam, max_passes=len(seeds), features="emit") as acc:
        for s in seeds:
            acc.add(s)
        acc.resolve_device(f["rgb"], f["var"])
        aov = {k: v.clone() for k, v in acc.resolve_aov_device().items()}
    for k in ("normal", "depth", "emission", "coverage"):
        f[k] = aov[k]
    return f, aov


def bench_time(width, rounds, warm):
    dev = torch.device("cuda", 0)
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = width, 4
    cams = (cam, orbit(cam, 1.0))
    with rt.Scene(t, w, l) as sc:
        (prev, _), (cur, aov) = (frame_tensors(sc, c, s, dev) for c, s in zip(cams, ((1, 2), (3, 4))))
    prev["count"] = torch.full((width, width), 2.0, device=dev)
    out = {k: torch.empty_like(cur[k]) for k in ("rgb", "var")}
    out["count"] = torch.empty((width, width), device=dev)
    out_e = {k: torch.empty_like(v) for k, v in out.items()}
    out_l = {k: torch.empty_like(v) for k, v in out.items()}
    out_l.update({k: torch.empty_like(cur[k]) for k in ("emission", "coverage")})
    plain = [{k: v for k, v in f.items() if k not in ("emission", "coverage")} for f in (prev, cur)]
    n = width * width
    src = torch.empty(n * 50 // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    den, vout = torch.empty_like(cur["rgb"]), torch.empty_like(cur["var"])
    with torch.no_grad():
        z = (prev["rgb"] - prev["emission"]) / (1.0 - prev["coverage"]).clamp_min(0.125)[..., None]
        lum2 = torch.nan_to_num((z * torch.tensor([0.2126, 0.7152, 0.0722], device=dev)).sum(-1) ** 2).contiguous()
    mplain = [dict(plain[0], lum2=lum2), dict(plain[1], count=2.0)]
    mfull = [dict(prev, lum2=lum2), dict(cur, count=2.0)]
    out_m = {m: dict({k: torch.empty_like(v) for k, v in (out_l if m == "light" else out).items()},
                     lum2=torch.empty_like(lum2)) for m in ("plain", "emit", "light")}

    def moments(mode, **kw):
        f = mplain if mode == "plain" else mfull
        return lambda: rt.reproject_moments_device(mode, cams[0], f[0], cams[1], f[1], out=out_m[mode], **kw)
    steady = [dict(f[0], count=torch.full((width, width), 16.0, device=dev)) for f in (mplain, mfull)]

    def clip(mode, prev_steady=False, entry=rt.reproject_clip_device, **kw):
        f = mplain if mode == "plain" else mfull
        p = steady[mode != "plain"] if prev_steady else f[0]
        return lambda: entry(mode, cams[0], p, cams[1], f[1], out=out_m[mode], **kw)
    calls = {
        "reproject": lambda: rt.reproject_device(cams[0], plain[0], cams[1], dict(plain[1], count=2.0), out=out),
        "reproject_emit": lambda: rt.reproject_emit_device(cams[0], prev, cams[1], dict(cur, count=2.0), out=out_e),
        "reproject_light": lambda: rt.reproject_light_device(cams[0], prev, cams[1], dict(cur, count=2.0), out=out_l),
        "denoise_var": lambda: rt.denoise_var_device(cur["rgb"], cur["var"], aov, out=den, var_out=vout),
        "copy_50_bytes_per_pixel": lambda: (dst.copy_(src), torch.cuda.synchronize()),
    }
    for m in ("plain", "emit", "light"):
        calls[f"moments_{m}"] = moments(m)
        calls[f"moments_{m}_no_window"] = moments(m, var_radius=-1)
        calls[f"clip_{m}"] = clip(m)
        calls[f"moments_{m}_steady"] = clip(m, True, rt.reproject_moments_device)
        calls[f"clip_{m}_steady"] = clip(m, True)
    ms = {k: [] for k in calls}
    for r in range(warm + rounds):
        for k, fn in calls.items():
            v = timed(fn)
            if r >= warm:
                ms[k].append(v)
    found = float((out["count"] > 2.0).float().mean().item())
    return {"image": f"cornell {width}x{width}", "rounds": rounds, "warmup_rounds": warm,
            "ms_median_min_max": {k: stat(v) for k, v in ms.items()},
            "bytes_per_pixel_nominal": 100, "bytes_per_pixel_nominal_emit": 180, "bytes_per_pixel_nominal_light": 196,
            "history_found_share": found,
            "history_found_share_light": float((out_l["count"] > 2.0).float().mean().item()),
            "history_found_share_emit": float((out_e["count"] > 2.0).float().mean().item()),
            "note": "HIP events around each blocking call (launch, kernel and the stream synchronise)"}


def bench_quality(width, frames, degrees, ref_spp):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = width, 4
    temporal, split = rt.Temporal(), rt.Temporal(split_emitters=True)
    light = rt.Temporal(split_emitters=True, light_history=True)
    with rt.Scene(t, w, l) as sc:
        for k in range(frames):
            camk = orbit(cam, degrees * k)
            with sc.accumulator(camk, max_passes=2, features="emit") as acc:
                acc.add(10 * k + 1)
                acc.add(10 * k + 2)
                rgb, var, count = temporal.push(acc)
                rgb_e, var_e, count_e = split.push(acc)
                rgb_l, var_l, count_l = light.push(acc)
                if k == frames - 1:
                    mean, _ = acc.resolve()
                    aov = acc.resolve_aov_device()
                    cover = aov["coverage"].cpu().numpy()
                    both = rt.denoise_var_device(rgb, var, aov, split_emitters=True).cpu().numpy()
                    only = acc.denoise_device().cpu().numpy()
                    both_e = rt.denoise_var_device(rgb_e, var_e, aov, split_emitters=True).cpu().numpy()
                    temp, cnt = rgb.cpu().numpy(), count.cpu().numpy()
                    temp_e, cnt_e = rgb_e.cpu().numpy(), count_e.cpu().numpy()
                    both_l = rt.denoise_var_device(rgb_l, var_l, dict(aov, **light.light),
                                                   split_emitters=True).cpu().numpy()
                    temp_l, cnt_l = rgb_l.cpu().numpy(), count_l.cpu().numpy()
        camk.SamplesPerPixel = ref_spp
        ref, _ = sc.render(camk, seed=977)
    fin = np.isfinite(mean).all(-1) & np.isfinite(ref).all(-1)
    near = cover > 0  # the directly seen lights and the pixels within 2 of them
    for _ in range(2):
        pad = np.pad(near, 1)
        near = np.logical_or.reduce([pad[dy:dy + width, dx:dx + width] for dy in range(3) for dx in range(3)])
    sets = {"all": fin, "rim": fin & (cover > 0) & (cover < 1), "with_history": fin & (cnt > 2.0),
            "within_2_of_a_light": fin & near, "elsewhere": fin & ~near}
    cols = {"per_frame_mean": mean, "temporal": temp, "temporal_emit": temp_e, "temporal_light": temp_l,
            "guided_filter": only, "temporal_guided_filter": both, "temporal_emit_guided_filter": both_e,
            "temporal_light_guided_filter": both_l}
    sq = {c: (x.astype(np.float64) - ref) ** 2 for c, x in cols.items()}
    return {"image": f"cornell {width}x{width}", "frames": frames, "degrees_per_frame": degrees,
            "passes_per_frame": 2, "spp_per_pass": 4, "reference_spp": ref_spp,
            "pixels": {k: int(m.sum()) for k, m in sets.items()},
            "history_found_share": float((cnt > 2.0).mean()), "mean_count": float(cnt.mean()),
            "history_found_share_emit": float((cnt_e > 2.0).mean()), "mean_count_emit": float(cnt_e.mean()),
            "history_found_share_light": float((cnt_l > 2.0).mean()), "mean_count_light": float(cnt_l.mean()),
            "rim_share_of_squared_error": {c: float(v[sets["rim"]].sum() / v[fin].sum()) for c, v in sq.items()},
            "mse": {s: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) if m.any() else None
                        for c, x in cols.items()} for s, m in sets.items()}}


def bench_quality_one_pass(width, frames, degrees, ref_spp):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = width, 4
    today, moments = rt.Temporal(split_emitters=True), rt.Temporal(split_emitters=True, moments=True)
    with rt.Scene(t, w, l) as sc:
        for k in range(frames):
            camk = orbit(cam, degrees * k)
            with sc.accumulator(camk, max_passes=1, features="emit") as acc:
                acc.add(10 * k + 1)
                a, b = today.push(acc), moments.push(acc)
                if k == frames - 1:
                    mean, _ = acc.resolve()
                    aov = acc.resolve_aov_device()
                    cover = aov["coverage"].cpu().numpy()
                    cols = {"per_frame_mean": mean, "temporal_emit": a[0].cpu().numpy(),
                            "temporal_emit_guided_filter":
                                rt.denoise_var_device(a[0], a[1], aov, split_emitters=True).cpu().numpy(),
                            "temporal_emit_moments_guided_filter":
                                rt.denoise_var_device(b[0], b[1], aov, split_emitters=True).cpu().numpy()}
                    var, cnt = b[1].cpu().numpy(), b[2].cpu().numpy()
        camk.SamplesPerPixel = ref_spp
        ref, _ = sc.render(camk, seed=977)
    fin = np.isfinite(mean).all(-1) & np.isfinite(ref).all(-1)
    near = cover > 0
    for _ in range(2):
        pad = np.pad(near, 1)
        near = np.logical_or.reduce([pad[dy:dy + width, dx:dx + width] for dy in range(3) for dx in range(3)])
    sets = {"all": fin, "rim": fin & (cover > 0) & (cover < 1), "with_history": fin & (cnt > 1.0),
            "within_2_of_a_light": fin & near, "elsewhere": fin & ~near}
    return {"image": f"cornell {width}x{width}", "frames": frames, "degrees_per_frame": degrees,
            "passes_per_frame": 1, "spp_per_pass": 4, "reference_spp": ref_spp,
            "pixels": {k: int(m.sum()) for k, m in sets.items()},
            "moments_var_positive_share_with_history": float((var[sets["with_history"]] > 0).mean()),
            "mse": {s: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) if m.any() else None
                        for c, x in cols.items()} for s, m in sets.items()}}


GAMMAS = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0)


def bench_quality_clip(scene, width, frames, degrees, ref_spp, gammas=GAMMAS):
    t, cam, w, l = rt.demo_scene(scene)
    cam.Width, cam.SamplesPerPixel = width, 4
    kw = dict(split_emitters=True, moments=True)
    paths = {"history": rt.Temporal(**kw)}
    paths.update({f"clip_gamma_{g:g}": rt.Temporal(clip=True, clip_gamma=g, **kw) for g in gammas})
    with rt.Scene(t, w, l) as sc:
        for k in range(frames):
            camk = orbit(cam, degrees * k)
            with sc.accumulator(camk, max_passes=1, features="emit") as acc:
                acc.add(10 * k + 1)
                res = {name: tp.push(acc) for name, tp in paths.items()}
                if k == frames - 1:
                    mean, _ = acc.resolve()
                    aov = acc.resolve_aov_device()
                    cover = aov["coverage"].cpu().numpy()
                    cols = {"frame": mean}
                    for name, r in res.items():
                        cols[name] = r[0].cpu().numpy()
                        cols[name + "_filtered"] = rt.denoise_var_device(r[0], r[1], aov, split_emitters=True).cpu().numpy()
                    cnt = res["history"][2].cpu().numpy()
                    var = {name: float(r[1].mean().item()) for name, r in res.items()}
        material = sc.render_aov(camk)["material"]
        camk.SamplesPerPixel = ref_spp
        ref, _ = sc.render(camk, seed=977)
    fin = np.isfinite(mean).all(-1) & np.isfinite(ref).all(-1)
    metal = material == rt._lib.RT_MAT_METAL
    near = cover > 0
    for _ in range(2):
        pad = np.pad(near, 1)
        near = np.logical_or.reduce([pad[dy:dy + width, dx:dx + width] for dy in range(3) for dx in range(3)])
    sets = {"all": fin, "metal": fin & metal, "rest": fin & ~metal, "rim": fin & (cover > 0) & (cover < 1),
            "with_history": fin & (cnt > 1.0), "within_2_of_a_light": fin & near, "elsewhere": fin & ~near}
    return {"image": f"{scene} {width}x{width}", "frames": frames, "degrees_per_frame": degrees,
            "passes_per_frame": 1, "spp_per_pass": 4, "reference_spp": ref_spp,
            "pixels": {k: int(m.sum()) for k, m in sets.items()}, "mean_var": var,
            "mse": {s: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) if m.any() else None
                        for c, x in cols.items()} for s, m in sets.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=None)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--quality-width", type=int, default=128)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--only", choices=("time", "quality", "clip"), default=None)
    ap.add_argument("--sweep-degrees", type=float, default=3.0, help="the quads orbit's step in the gamma sweep")
    a = ap.parse_args()
    if rt.device_count() <= 0:
        raise SystemExit("temporal_bench: no HIP device visible")
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only in (None, "time"):
        res["time"] = bench_time(a.width, a.rounds, 5)
    if a.only in (None, "quality"):
        res["quality"] = bench_quality(a.quality_width, a.frames, 1.0, a.ref_spp)
        res["quality_one_pass"] = bench_quality_one_pass(a.quality_width, a.frames, 1.0, a.ref_spp)
    if a.only in (None, "clip"):
        q = {f"{scene}_{deg:g}deg": bench_quality_clip(scene, a.quality_width, a.frames, deg, a.ref_spp)
             for scene, deg in dict.fromkeys((("quads", 1.0), ("quads", 3.0), ("quads", a.sweep_degrees), ("cornell", 1.0)))}
        res["quality_clip"] = q
        res["gamma_sweep"] = {
            "orbits": [f"quads_{a.sweep_degrees:g}deg", "cornell_1deg"],
            "summed_all_pixel_mse_filtered": {
                f"{g:g}": sum(q[o]["mse"]["all"][f"clip_gamma_{g:g}_filtered"]
                              for o in (f"quads_{a.sweep_degrees:g}deg", "cornell_1deg")) for g in GAMMAS},
            "without_clip": sum(q[o]["mse"]["all"]["history_filtered"]
                                for o in (f"quads_{a.sweep_degrees:g}deg", "cornell_1deg"))}
    text = json.dumps(res, indent=1)
    print(text)
    if a.o:
        with open(a.o, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
