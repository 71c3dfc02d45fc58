"""rt.Temporal(split_emitters=True) on rendered frames: Cornell 48 x 48, 2 passes x 4 spp per frame
(features="emit"), a 4-frame orbit of 1 degree per frame, as tests/test_temporal_gpu.py runs it.

One ordering is asserted, the feature's claim: against a 1024-spp render of the last camera the
mean squared error over the pixels within 2 pixels of the directly seen light is lower with the
split history than with the plain one.  The rest of DESIGN.md §17's table is printed, not
asserted."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_temporal_gpu import W, frame, host, orbit

pytestmark = pytest.mark.gpu
FRAMES = 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_split_history_on_the_cornell_orbit(rt, gpu):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    plain, split = rt.Temporal(), rt.Temporal(split_emitters=True)
    with rt.Scene(t, w, l) as sc:
        for k in range(FRAMES):
            camk = orbit(cam, 1.0 * k)
            with frame(sc, camk, (10 * k + 1, 10 * k + 2)) as acc:
                mean, mvar = acc.resolve()
                cover = acc.resolve_aov()["coverage"]
                p = host(*plain.push(acc))
                rgb, var, count = split.push(acc)
                s = host(rgb, var, count)
                fin = np.isfinite(mean).all(-1) & np.isfinite(mvar)
                # finite wherever the frame is, the counts within the parent's bounds
                assert np.isfinite(s[0][fin]).all() and np.isfinite(s[1][fin]).all() and (s[1][fin] >= 0).all()
                assert (s[2] >= 2.0).all() and (s[2] <= 2.0 * (k + 1) * (1 + 1e-3)).all()
                # a fully covered pixel neither takes nor gives history: the frame's own mean, bit for bit
                full = cover == 1.0
                assert full.sum() > 0
                assert np.array_equal(bits(s[0])[full], bits(mean)[full]) and np.array_equal(bits(s[1])[full], bits(mvar)[full])
                assert (s[2][full] == 2.0).all()
                if k == 0:  # the first push is the current frame unchanged, as without the split
                    assert np.array_equal(s[0], mean, equal_nan=True) and np.array_equal(s[1], mvar, equal_nan=True)
                    assert (s[2] == 2.0).all() and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(s, p))
                if k == FRAMES - 1:
                    aov = acc.resolve_aov_device()
                    only = acc.denoise_device().cpu().numpy()
                    p_f, s_f = (rt.denoise_var_device(torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[1]).cuda(), aov,
                                                      split_emitters=True).cpu().numpy() for x in (p, s))
        camk.SamplesPerPixel = 1024
        ref, _ = sc.render(camk, seed=977)
    assert (s[2] > 2.0).mean() > 0.5  # the split history is found as the plain one is
    fin &= np.isfinite(ref).all(-1)
    near = cover > 0  # the directly seen light and the pixels within 2 of it
    for _ in range(2):
        pad = np.pad(near, 1)
        near = np.logical_or.reduce([pad[dy:dy + W, dx:dx + W] for dy in range(3) for dx in range(3)])
    sets = {"all": fin, "rim (0 < coverage < 1)": fin & (cover > 0) & (cover < 1),
            "within 2 of the directly seen light": fin & near, "elsewhere": fin & ~near}
    cols = {"per-frame mean": mean, "temporal": p[0], "temporal-emit": s[0], "guided filter": only,
            "temporal + filter": p_f, "temporal-emit + filter": s_f}
    mse = {r: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) for c, x in cols.items()}
           for r, m in sets.items()}
    print(f"cornell {W}x{W}, {FRAMES}-frame 1-degree orbit, 2 x 4 spp per frame, mse against 1024 spp; history found on "
          f"{(p[2] > 2.0).mean():.3f} (plain) / {(s[2] > 2.0).mean():.3f} (split) of the pixels")
    for r, m in sets.items():
        print(f"  {r}, {int(m.sum())} pixels: " + ", ".join(f"{c} {v:.5f}" for c, v in mse[r].items()))
    row = mse["within 2 of the directly seen light"]
    assert row["temporal-emit"] < row["temporal"], row


def test_split_emitters_needs_an_emit_accumulator(rt, gpu):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 16, 4
    with rt.Scene(t, w, l) as sc, sc.accumulator(cam, max_passes=2, features="guides") as acc:
        acc.add(1)
        with pytest.raises(ValueError, match="features='emit'"):
            rt.Temporal(split_emitters=True).push(acc)
        rgb, var, count = rt.Temporal().push(acc)  # the default takes it as before
        assert float(count.min()) == 1.0
