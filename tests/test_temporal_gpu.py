"""rt.Temporal on rendered frames: Cornell 48 x 48, 2 passes x 4 spp per frame, features="emit".

Pushing the same frame twice reprojects every pixel onto itself: (u, v) = (x, y) up to fp32
rounding, so the centre tap carries all the weight but |du| (a neighbour enters with that), and
it passes its own consistency test because the guides are its own.  The bound on that rounding
used below: q = s r - Ap is a difference of vectors of length about the focus distance (10, the
camera's default), each component a few roundings of 10 * 2^-24 = 6e-7 wrong, and a pixel of the
48-pixel image plane is 2 * 10 * tan(20 deg) / 48 = 0.15 wide: |du|, |dv| <= 1e-4 with a margin
of about 4.  A blend then differs from the centre-only blend by at most (|du| + |dv|) times the
largest colour difference to a neighbour, which is the tolerance per pixel, plus 8 fp32 roundings
of the value.

The orbit's quality figures are printed, not asserted (as tests/test_denoise_emit_gpu.py does)."""
import math

import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

pytestmark = pytest.mark.gpu
W = 48
DUV = 1e-4  # the bound on |u - x| and |v - y| derived above


def orbit(cam, degrees):
    """look_from turned about the vup axis through look_at"""
    frm, at, up = (np.array(x, np.float64) for x in cam._pos)
    k = up / np.linalg.norm(up)
    v, th = frm - at, math.radians(degrees)
    out = type(cam).from_c(cam.to_c())
    out.PositionCamera(at + v * math.cos(th) + np.cross(k, v) * math.sin(th) + k * (k @ v) * (1 - math.cos(th)), at, up)
    return out


def frame(sc, cam, seeds, features="emit"):
    acc = sc.accumulator(cam, max_passes=len(seeds), features=features)
    for s in seeds:
        acc.add(s)
    return acc


def neighbour_spread(a):
    """per pixel, the largest |a_q - a_p| over the 8 neighbours q (all channels)"""
    h, w = a.shape[:2]
    a = a.reshape(h, w, -1)
    pad = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
    out = np.zeros((h, w))
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out = np.maximum(out, np.abs(pad[dy:dy + h, dx:dx + w] - a).max(-1))
    return out


def check_blend(tag, first, second, got, passes=2.0):
    """second pushed after first (both (rgb, var, depth) host arrays of the same camera): where
    the count says the history was found whole, rgb is the blend of the two means"""
    rgb1, var1, depth1 = first
    rgb2, var2, depth2 = second
    rgb, var, count = got
    ok = (depth2 > 0) & np.isfinite(rgb2).all(-1) & np.isfinite(var2) & np.isfinite(rgb1).all(-1) & np.isfinite(var1)
    whole = ok & (np.abs(count - 2 * passes) <= 1e-3 * 2 * passes)
    want = (passes * rgb1.astype(np.float64) + passes * rgb2) / (2 * passes)
    tol = 2 * DUV * neighbour_spread(rgb1.astype(np.float64)) + 8 * 2.0 ** -24 * np.abs(want).max(-1) + 1e-6
    err = np.abs(rgb - want).max(-1)
    print(f"{tag}: {int(whole.sum())} of {int(ok.sum())} eligible pixels found their whole history; "
          f"rgb max err {err[whole].max():.3e}, largest tolerance used {tol[whole].max():.3e}")
    assert (err[whole] <= tol[whole]).all(), float((err[whole] - tol[whole]).max())
    return ok, whole


def host(*tensors):
    return tuple(t.cpu().numpy().copy() for t in tensors)


def test_same_frame_pushed_twice(rt, gpu):
    """every pixel with depth > 0, finite inputs and a previous count > 0 has count_out =
    min(count_prev, cap) + count_cur within 1e-3 relative (cap = 8 x 2 passes, count_prev = 2),
    and rgb is the blend of the two resolved means; misses and non-finite pixels keep their bits"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    temporal = rt.Temporal()
    with rt.Scene(t, w, l) as sc, frame(sc, cam, (1, 2)) as acc:
        first = host(*temporal.push(acc))
        depth = acc.resolve_aov()["depth"]
        mean, var = acc.resolve()
        assert np.array_equal(first[0], mean, equal_nan=True) and np.array_equal(first[1], var, equal_nan=True)
        assert (first[2] == 2.0).all()  # the first push is the current frame, every pixel weighing its passes
        got = host(*temporal.push(acc))
        ok, whole = check_blend("same frame twice", (mean, var, depth), (mean, var, depth), got)
        assert ok.sum() > 0.9 * W * W and np.array_equal(ok, whole)  # every eligible pixel
        keep = ~ok
        for g, cur in zip(got, (mean, var, np.full((W, W), 2.0, np.float32))):
            assert np.array_equal(g[keep].view(np.uint32), cur[keep].view(np.uint32))
        # a third push of it: the history now weighs 4, the frame 2
        third = host(*temporal.push(acc))
        assert np.abs(third[2][ok] - 6.0).max() <= 6e-3
        temporal.reset()
        again = host(*temporal.push(acc))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again, first))


def test_two_frames_of_one_camera(rt, gpu):
    """other seeds, the same camera: the guides of the two frames differ where a pixel's samples
    straddle an edge, so some pixels may refuse their history; wherever it was found whole, rgb is
    the blend of the two frames' means"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    temporal = rt.Temporal()
    with rt.Scene(t, w, l) as sc, frame(sc, cam, (1, 2)) as a, frame(sc, cam, (3, 4)) as b:
        temporal.push(a)
        got = host(*temporal.push(b))
        first = a.resolve() + (a.resolve_aov()["depth"],)
        second = b.resolve() + (b.resolve_aov()["depth"],)
    ok, whole = check_blend("two frames, one camera", first, second, got)
    assert whole.sum() > 0.5 * ok.sum()
    assert not np.array_equal(first[0], second[0])


def test_temporal_checks_its_accumulator(rt, gpu):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 16, 4
    temporal = rt.Temporal()
    with rt.Scene(t, w, l) as sc:
        with sc.accumulator(cam, max_passes=2) as plain, pytest.raises(ValueError, match="features"):
            plain.add(1)
            temporal.push(plain)
        with sc.accumulator(cam, max_passes=2, features="guides", rank=0, nranks=2) as share:
            share.add(1)
            with pytest.raises(ValueError, match="whole image"):
                temporal.push(share)
        with sc.accumulator(cam, max_passes=2, features="guides") as empty, pytest.raises(ValueError, match="no pass"):
            temporal.push(empty)


def test_orbit_is_finite_filters_and_reports_quality(rt, gpu):
    """a 4-frame orbit of 1 degree per frame: the pushed frames are finite wherever the frame is,
    the guided filter runs on them, and the error against a 64-pass render of the last camera is
    printed for the per-frame mean, temporal only, and temporal + guided filter (not asserted)"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    temporal = rt.Temporal()
    with rt.Scene(t, w, l) as sc:
        for k in range(4):
            camk = orbit(cam, 1.0 * k)
            with frame(sc, camk, (10 * k + 1, 10 * k + 2)) as acc:
                rgb, var, count = temporal.push(acc)
                mean, mvar = acc.resolve()
                fin = np.isfinite(mean).all(-1) & np.isfinite(mvar)
                g = host(rgb, var, count)
                assert np.isfinite(g[0][fin]).all() and np.isfinite(g[1][fin]).all() and (g[1][fin] >= 0).all()
                assert (g[2] >= 2.0).all() and (g[2] <= 2.0 * (k + 1) * (1 + 1e-3)).all()
                if k == 3:
                    aov = acc.resolve_aov_device()
                    both = rt.denoise_var_device(rgb, var, aov, split_emitters=True).cpu().numpy()
                    only = acc.denoise_device().cpu().numpy()
        with frame(sc, camk, tuple(range(100, 164)), features=None) as ref_acc:
            ref, _ = ref_acc.resolve()
    assert both.shape == (W, W, 3) and np.isfinite(both[fin]).all()
    found = float((g[2] > 2.0).mean())
    mse = {name: float(((x[fin].astype(np.float64) - ref[fin]) ** 2).mean())
           for name, x in (("per-frame mean", mean), ("temporal", g[0]), ("guided filter", only),
                           ("temporal + guided filter", both))}
    print(f"cornell {W}x{W}, 4-frame 1-degree orbit, 2 x 4 spp per frame: history found on {found:.3f} of the pixels, "
          f"mean count {g[2].mean():.2f}; mse against 64 passes: " + ", ".join(f"{k} {v:.5f}" for k, v in mse.items()))
    assert found > 0
