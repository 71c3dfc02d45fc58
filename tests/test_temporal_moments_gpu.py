"""rt.Temporal(split_emitters=True, moments=True) on rendered frames, the feature's claim: Cornell
48 x 48, a 6-frame orbit of 1 degree per frame, ONE pass x 4 spp per frame (features="emit").

With one pass the accumulator's variance is 0 in every frame, so today's split history hands
rt_denoise_var a variance of 0 and the variance-guided filter's colour term switches the filter off.
With the moments the history itself gives a variance.  Asserted: (a)'s var is identically 0 and
(b)'s is positive on more than half of the pixels with history; and the filtered last frame's mean
squared error against a 1024-spp render of the last camera, over the pixels more than 2 pixels
from the directly seen light, is lower through (b) than through (a).  Both are computed here: an
ordering, not a figure.  The rows of DESIGN.md §17's table are printed for both paths."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_temporal_gpu import W, frame, host, orbit

pytestmark = pytest.mark.gpu
FRAMES = 6


def test_one_pass_frames_can_be_filtered(rt, gpu):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    today, moments = rt.Temporal(split_emitters=True), rt.Temporal(split_emitters=True, moments=True)
    with rt.Scene(t, w, l) as sc:
        for k in range(FRAMES):
            camk = orbit(cam, 1.0 * k)
            with frame(sc, camk, (10 * k + 1,)) as acc:
                mean, mvar = acc.resolve()
                assert not mvar[np.isfinite(mvar)].any()   # one pass: the accumulator has no variance
                a = host(*today.push(acc))
                b = host(*moments.push(acc))
                fin = np.isfinite(mean).all(-1)
                assert np.isfinite(b[0][fin]).all() and np.isfinite(b[1][fin]).all() and (b[1][fin] >= 0).all()
                assert (b[2] >= 1.0).all() and (b[2] <= (k + 1) * (1 + 1e-3)).all()
                if k == 0:   # the first push: the frame's own colour, and already a variance (the window's)
                    assert np.array_equal(b[0], mean, equal_nan=True) and (b[2] == 1.0).all()
                    assert (b[1][fin] > 0).mean() > 0.5
                if k == FRAMES - 1:
                    aov = acc.resolve_aov_device()
                    cover = acc.resolve_aov()["coverage"]
                    a_f, b_f = (rt.denoise_var_device(torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[1]).cuda(), aov,
                                                      split_emitters=True).cpu().numpy() for x in (a, b))
        camk.SamplesPerPixel = 1024
        ref, _ = sc.render(camk, seed=977)
    hist = fin & (b[2] > 1.0)
    assert hist.mean() > 0.5 and np.array_equal(a[2] > 1.0, b[2] > 1.0)   # the same history is found
    assert not a[1][fin].any()                                            # (a): var is identically 0
    assert (b[1][hist] > 0).mean() > 0.5                                  # (b): a variance where there is history
    fin &= np.isfinite(ref).all(-1)
    near = cover > 0  # the directly seen light and the pixels within 2 of it
    for _ in range(2):
        pad = np.pad(near, 1)
        near = np.logical_or.reduce([pad[dy:dy + W, dx:dx + W] for dy in range(3) for dx in range(3)])
    sets = {"all": fin, "rim (0 < coverage < 1)": fin & (cover > 0) & (cover < 1),
            "within 2 of the directly seen light": fin & near, "elsewhere": fin & ~near}
    cols = {"per-frame mean": mean, "temporal-emit": a[0], "temporal-emit moments": b[0],
            "temporal-emit + filter": a_f, "temporal-emit moments + filter": b_f}
    mse = {r: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) for c, x in cols.items()}
           for r, m in sets.items()}
    print(f"cornell {W}x{W}, {FRAMES}-frame 1-degree orbit, 1 x 4 spp per frame, mse against 1024 spp; history found on "
          f"{hist.mean():.3f} of the pixels; var > 0 on {(b[1][hist] > 0).mean():.3f} of them, median std error "
          f"{float(np.median(np.sqrt(b[1][hist]))):.4f}")
    for r, m in sets.items():
        print(f"  {r}, {int(m.sum())} pixels: " + ", ".join(f"{c} {v:.5f}" for c, v in mse[r].items()))
    row = mse["elsewhere"]
    assert row["temporal-emit moments + filter"] < row["temporal-emit + filter"], row


def test_moments_off_is_what_it_was(rt, gpu):
    """Temporal without moments, and with moments=False spelled out, give identical bits"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    x, y = rt.Temporal(split_emitters=True), rt.Temporal(split_emitters=True, moments=False)
    with rt.Scene(t, w, l) as sc:
        for k in range(2):
            with frame(sc, orbit(cam, 1.0 * k), (10 * k + 1, 10 * k + 2)) as acc:
                p, q = host(*x.push(acc)), host(*y.push(acc))
    assert all(np.array_equal(i, j, equal_nan=True) for i, j in zip(p, q))
