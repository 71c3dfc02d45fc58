"""rt.Temporal(split_emitters=True, light_history=True) on rendered frames: tests/
test_temporal_emit_gpu.py's sequence (Cornell 48 x 48, 2 passes x 4 spp per frame, features="emit", a
4-frame orbit of 1 degree per frame) through the split history and through the light history.

One ordering is asserted, the feature's claim: against a 1024-spp render of the last camera the
mean squared error over the rim pixels (0 < the frame's coverage < 1) is lower with the light
history than with the split history.  The rest of DESIGN.md §17's table is printed with the new
column, before and after the filter, not asserted."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_temporal_emit_gpu import FRAMES, bits
from tests.test_temporal_gpu import W, frame, host, orbit

pytestmark = pytest.mark.gpu
LIGHT_KEYS = ("emission", "coverage")


def test_light_history_on_the_cornell_orbit(rt, gpu):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    split, light = rt.Temporal(split_emitters=True), rt.Temporal(split_emitters=True, light_history=True)
    assert light.light is None and split.light is None
    kept = None  # the history as this test holds it: copies of what the last push returned
    with rt.Scene(t, w, l) as sc:
        for k in range(FRAMES):
            camk = orbit(cam, 1.0 * k)
            with frame(sc, camk, (10 * k + 1, 10 * k + 2)) as acc:
                mean, mvar = acc.resolve()
                own = acc.resolve_aov_device()
                cover = own["coverage"].cpu().numpy()
                s = host(*split.push(acc))
                rgb, var, count = light.push(acc)
                g = host(rgb, var, count)
                assert split.light is None and set(light.light) == set(LIGHT_KEYS)
                lp = {key: light.light[key].cpu().numpy() for key in LIGHT_KEYS}
                fin = np.isfinite(mean).all(-1) & np.isfinite(mvar)
                # finite wherever the frame is, the counts within the parent's bounds, coverage a share
                assert np.isfinite(g[0][fin]).all() and np.isfinite(g[1][fin]).all() and (g[1][fin] >= 0).all()
                assert (g[2] >= 2.0).all() and (g[2] <= 2.0 * (k + 1) * (1 + 1e-3)).all()
                assert np.isfinite(lp["emission"]).all() and (lp["coverage"] >= 0).all() and (lp["coverage"] <= 1).all()
                if k == 0:  # the first push is the current frame unchanged, its light planes the frame's own
                    assert np.array_equal(g[0], mean, equal_nan=True) and np.array_equal(g[1], mvar, equal_nan=True)
                    assert (g[2] == 2.0).all() and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(g, s))
                    assert all(np.array_equal(bits(lp[key]), bits(own[key].cpu().numpy())) for key in LIGHT_KEYS)
                else:
                    # the planes the last push left in temporal.light were this push's prev_emit: the
                    # same call on the copies kept then gives this push's bits in all five planes
                    cur = {"rgb": torch.from_numpy(mean).cuda(), "var": torch.from_numpy(mvar).cuda(), "count": 2.0,
                           "normal": own["normal"], "depth": own["depth"], "emission": own["emission"],
                           "coverage": own["coverage"]}
                    again = host(*rt.reproject_light_device(kept["cam"], kept["frame"], camk, cur))
                    for name, a, b in zip(("rgb", "var", "count") + LIGHT_KEYS, again, g + (lp["emission"], lp["coverage"])):
                        assert np.array_equal(bits(a), bits(b)), (k, name)
                kept = {"cam": camk, "frame": {"rgb": rgb.clone(), "var": var.clone(), "count": count.clone(),
                                               "normal": own["normal"].clone(), "depth": own["depth"].clone(),
                                               **{key: light.light[key].clone() for key in LIGHT_KEYS}}}
                if k == FRAMES - 1:
                    only = acc.denoise_device().cpu().numpy()
                    s_f = rt.denoise_var_device(torch.from_numpy(s[0]).cuda(), torch.from_numpy(s[1]).cuda(), own,
                                                split_emitters=True).cpu().numpy()
                    g_f = rt.denoise_var_device(rgb, var, dict(own, **light.light), split_emitters=True).cpu().numpy()
        camk.SamplesPerPixel = 1024
        ref, _ = sc.render(camk, seed=977)
    assert (g[2] > 2.0).mean() > 0.5  # the light history is found as the split one is
    fin &= np.isfinite(ref).all(-1)
    near = cover > 0  # the directly seen light and the pixels within 2 of it
    for _ in range(2):
        pad = np.pad(near, 1)
        near = np.logical_or.reduce([pad[dy:dy + W, dx:dx + W] for dy in range(3) for dx in range(3)])
    sets = {"all": fin, "rim (0 < coverage < 1)": fin & (cover > 0) & (cover < 1),
            "within 2 of the directly seen light": fin & near, "elsewhere": fin & ~near}
    cols = {"per-frame mean": mean, "temporal-emit": s[0], "temporal-light": g[0], "guided filter": only,
            "temporal-emit + filter": s_f, "temporal-light + filter": g_f}
    sq = {r: {c: ((x[m].astype(np.float64) - ref[m]) ** 2) for c, x in cols.items()} for r, m in sets.items()}
    print(f"cornell {W}x{W}, {FRAMES}-frame 1-degree orbit, 2 x 4 spp per frame, mse against 1024 spp; history found on "
          f"{(s[2] > 2.0).mean():.3f} (split) / {(g[2] > 2.0).mean():.3f} (light) of the pixels; coverage moved on "
          f"{int((lp['coverage'] != cover).sum())} pixels")
    for r, m in sets.items():
        print(f"  {r}, {int(m.sum())} pixels: " + ", ".join(f"{c} {float(v.mean()):.5f}" for c, v in sq[r].items()))
    print("  the rim's share of the squared error: " + ", ".join(
        f"{c} {float(sq['rim (0 < coverage < 1)'][c].sum() / sq['all'][c].sum()):.3f}" for c in cols))
    rim = {c: float(v.mean()) for c, v in sq["rim (0 < coverage < 1)"].items()}
    assert sets["rim (0 < coverage < 1)"].sum() > 0
    assert rim["temporal-light"] < rim["temporal-emit"], rim


def test_the_defaults_are_what_they_were(rt, gpu):
    """light_history=False is the split history's bits, and a light history object after reset()
    starts over: its first push is the frame"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 16, 4
    a, b = rt.Temporal(split_emitters=True), rt.Temporal(split_emitters=True, light_history=False)
    c = rt.Temporal(split_emitters=True, light_history=True)
    with rt.Scene(t, w, l) as sc:
        for k in range(2):
            with frame(sc, orbit(cam, 1.0 * k), (k + 1, k + 5)) as acc:
                for x, y in zip(host(*a.push(acc)), host(*b.push(acc))):
                    assert np.array_equal(bits(x), bits(y)), k
                c.push(acc)
                if k == 1:
                    c.reset()
                    assert c.light is None
                    g = host(*c.push(acc))
                    assert (g[2] == 2.0).all() and np.array_equal(g[0], acc.resolve()[0], equal_nan=True)
