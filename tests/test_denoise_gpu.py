"""rt_denoise_device (rt_denoise.hip) against a numpy restatement of the pinned filter.

The checker below is written from the formulas in include/rt_abi.h / DESIGN.md "Feature
buffers and denoiser", not from the kernel.  Accuracy bar (a): the GPU's max abs error
against the restatement in fp64 must be <= 8 x the error of the same restatement run in
numpy fp32, plus 1e-6 (the margin covers the kernel's __expf and its non-correctly-rounded
division)."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

pytestmark = pytest.mark.gpu

H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
DEF = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.02)


def atrous(rgb, albedo=None, normal=None, depth=None, iterations=5, demodulate=False,
           sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.02, dt=np.float64):
    rgb = np.asarray(rgb).astype(dt)
    h, w = rgb.shape[:2]
    valid = np.isfinite(rgb).all(-1)
    alb = None if albedo is None else np.maximum(np.asarray(albedo).astype(dt), dt(1e-3))
    with np.errstate(all="ignore"):
        c = rgb / alb if demodulate else rgb.copy()
    c[~valid] = 0
    n = None if normal is None else np.asarray(normal).astype(dt)
    d = None if depth is None else np.asarray(depth).astype(dt)
    ys, xs = np.mgrid[0:h, 0:w]
    for i in range(iterations):
        step = 1 << i
        sc = dt(sigma_color) * dt(2.0 ** -i)
        acc = np.zeros((h, w, 3), dt)
        ws = np.zeros((h, w), dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * step, xs + dx * step
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                cq = c[cy, cx]
                wgt = dt(H5[dx + 2]) * dt(H5[dy + 2]) * np.exp(-((c - cq) ** 2).sum(-1) / (sc * sc))
                if n is not None:
                    wgt = wgt * np.exp(-((n - n[cy, cx]) ** 2).sum(-1) / (dt(sigma_normal) ** 2))
                if d is not None:
                    sd = dt(sigma_depth) * np.maximum(d, dt(1e-6))
                    wgt = wgt * np.exp(-((d - d[cy, cx]) ** 2) / (sd * sd))
                wgt = np.where(inside & valid[cy, cx], wgt, dt(0)).astype(dt)
                acc += wgt[..., None] * cq
                ws += wgt
        with np.errstate(all="ignore"):
            new = acc / ws[..., None]
        c = np.where(valid[..., None], new, c)
    out = c * alb if demodulate else c
    out = np.where(valid[..., None], out, rgb)
    return out


def synthetic(h=17, w=24, seed=7):
    """piecewise-constant colour + noise, two normal regions, a depth ramp with a step edge,
    one NaN and one Inf pixel"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    left = xs < w // 2
    top = ys < h // 3
    base = np.where(left[..., None], (0.8, 0.3, 0.2), (0.2, 0.5, 0.9))
    base = np.where(top[..., None], base * 0.5, base)
    rgb = (base + 0.08 * rng.standard_normal((h, w, 3))).astype(np.float32)
    normal = np.where(left[..., None], (0.0, 0.0, -1.0), (0.6, 0.0, -0.8)).astype(np.float32)
    depth = (2.0 + 0.05 * xs + np.where(ys > 2 * h // 3, 3.0, 0.0)).astype(np.float32)
    albedo = np.where(((xs // 3 + ys // 3) % 2 == 0)[..., None], (0.9, 0.8, 0.7),
                      (0.2, 0.3, 0.4)).astype(np.float32)
    if h > 6 and w > 9:
        rgb[5, 7, 1] = np.nan
        rgb[h - 3, w - 4, 0] = np.inf
    return rgb, albedo, normal, depth


def gpu_denoise(rt, rgb, albedo=None, normal=None, depth=None, inplace=False, **opts):
    import torch
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).to(dev)
    aov = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
           for k, v in (("albedo", albedo), ("normal", normal), ("depth", depth)) if v is not None}
    out = rt.denoise_device(t, aov, out=t if inplace else None, **opts)
    if inplace:
        assert out.data_ptr() == t.data_ptr()
    return out.cpu().numpy()


def check(rt, rgb, albedo=None, normal=None, depth=None, inplace=False, **opts):
    """GPU vs the fp64 restatement, to the bar measured from the fp32 restatement."""
    kw = dict(DEF)
    kw.update({k: v for k, v in opts.items() if k.startswith("sigma")})
    kw["iterations"] = opts.get("iterations", 5)
    kw["demodulate"] = bool(opts.get("demodulate", albedo is not None))
    r64 = atrous(rgb, albedo, normal, depth, dt=np.float64, **kw)
    r32 = atrous(rgb, albedo, normal, depth, dt=np.float32, **kw)
    got = gpu_denoise(rt, rgb, albedo, normal, depth, inplace=inplace, **opts)
    fin = np.isfinite(np.asarray(rgb)).all(-1)
    e32 = float(np.abs(r32[fin] - r64[fin]).max())
    eg = float(np.abs(got[fin] - r64[fin]).max())
    bar = 8 * e32 + 1e-6
    print(f"denoise err gpu {eg:.3e} fp32-numpy {e32:.3e} bar {bar:.3e} ratio {eg / max(e32, 1e-30):.2f}")
    assert np.array_equal(got[~fin], np.asarray(rgb, np.float32)[~fin], equal_nan=True)
    assert eg <= bar, (eg, e32, bar)
    return got, r64


def test_accuracy_and_nonfinite(rt, gpu):
    """(a) + (b): 24 x 17, 5 iterations (step 16 > half the height: every border), all three
    guides; the NaN and the Inf pixel pass through and their neighbours equal the
    restatement's (no contamination)."""
    rgb, albedo, normal, depth = synthetic()
    got, ref = check(rt, rgb, None, normal, depth, iterations=5)
    assert np.isnan(got[5, 7, 1]) and np.isinf(got[17 - 3, 24 - 4, 0])
    fin = np.isfinite(rgb).all(-1)
    assert np.isfinite(got[fin]).all()
    for (y, x) in ((5, 7), (14, 20)):
        nb = got[y - 1:y + 2, x - 1:x + 2].reshape(-1, 3)[[0, 1, 2, 3, 5, 6, 7, 8]]
        assert np.isfinite(nb).all()
    # smoother than the input inside a flat region
    assert got[8:12, 2:10].std(axis=(0, 1)).max() < 0.5 * rgb[8:12, 2:10].std(axis=(0, 1)).max()


@pytest.mark.parametrize("iterations", [1, 2, 3, 8])
def test_iteration_counts(rt, gpu, iterations):
    """every kernel variant: the LDS-tile steps (1, 2), the first global step (4), and each
    of them as the last iteration"""
    rgb, albedo, normal, depth = synthetic()
    check(rt, rgb, albedo, normal, depth, iterations=iterations)


def test_zero_sigmas_return_input(rt, gpu):
    """(c) sigma -> 0+: every tap but the centre (and exact duplicates) has weight 0"""
    rgb, albedo, normal, depth = synthetic()
    got, _ = check(rt, rgb, None, normal, depth, iterations=5, sigma_color=1e-6,
                   sigma_normal=1e-6, sigma_depth=1e-6)
    fin = np.isfinite(rgb).all(-1)
    e32 = np.abs(atrous(rgb, None, normal, depth, dt=np.float32, sigma_color=1e-6, sigma_normal=1e-6,
                        sigma_depth=1e-6)[fin] - rgb[fin].astype(np.float64)).max()
    assert np.abs(got[fin] - rgb[fin]).max() <= 8 * e32 + 1e-6


def test_pure_b3_smoothing(rt, gpu):
    """(d) no guides, a huge sigma_color, one iteration: the B3 spline smoothing h (x) h,
    renormalised at the borders (computed here by separable convolution)."""
    rng = np.random.default_rng(3)
    img = rng.random((17, 24, 3)).astype(np.float32)
    got = gpu_denoise(rt, img, iterations=1, sigma_color=1e18)
    k = np.array(H5)

    def conv(a, axis):
        out = np.zeros_like(a)
        for j, d in enumerate(range(-2, 3)):
            sl_src = [slice(None)] * a.ndim
            sl_dst = [slice(None)] * a.ndim
            n = a.shape[axis]
            sl_src[axis] = slice(max(d, 0), n + min(d, 0))
            sl_dst[axis] = slice(max(-d, 0), n + min(-d, 0))
            out[tuple(sl_dst)] += k[j] * a[tuple(sl_src)]
        return out
    a = img.astype(np.float64)
    num = conv(conv(a, 0), 1)
    den = conv(conv(np.ones(a.shape[:2]), 0), 1)
    b3 = num / den[..., None]
    ref = atrous(img, iterations=1, sigma_color=1e18)
    assert np.abs(ref - b3).max() < 1e-12  # the restatement is the B3 smoothing
    e32 = np.abs(atrous(img, iterations=1, sigma_color=1e18, dt=np.float32) - ref).max()
    assert np.abs(got - b3).max() <= 8 * e32 + 1e-6


def test_demodulation_roundtrip(rt, gpu):
    """(e) textured albedo x noisy irradiance: the irradiance gets smoother, the albedo's
    edges stay: the output is albedo x filtered irradiance, the restatement's, to the bar
    (filtering rgb itself across those edges would not be)."""
    rng = np.random.default_rng(11)
    h, w = 17, 24
    _, albedo, normal, depth = synthetic()
    irr = (1.0 + 0.2 * rng.standard_normal((h, w, 3))).astype(np.float32)
    rgb = albedo * irr
    got, ref = check(rt, rgb, albedo, None, None, iterations=3, demodulate=1)
    f_in, f_out = rgb / albedo, got / albedo
    assert f_out.std() < 0.5 * f_in.std()


def test_out_may_alias_rgb(rt, gpu):
    """(f)"""
    rgb, albedo, normal, depth = synthetic()
    a = gpu_denoise(rt, rgb, albedo, normal, depth, iterations=5)
    b = gpu_denoise(rt, rgb, albedo, normal, depth, iterations=5, inplace=True)
    assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 131)])
def test_other_sizes(rt, gpu, h, w):
    """(g) 1 x 1, 3 x 2 and a width over two 64-pixel tiles"""
    rgb, albedo, normal, depth = synthetic(h, w, seed=h * 100 + w)
    check(rt, rgb, albedo, normal, depth, iterations=5)


def test_host_entry_point_matches_device(rt, gpu):
    rgb, albedo, normal, depth = synthetic()
    aov = {"albedo": albedo, "normal": normal, "depth": depth}
    a = rt.denoise(rgb, aov, iterations=4)
    b = gpu_denoise(rt, rgb, albedo, normal, depth, iterations=4)
    assert np.array_equal(a, b, equal_nan=True)


def test_end_to_end_cornell_and_ppm(rt, gpu):
    """Cornell 48 x 48: render 4 spp -> feature pass -> denoise on the device; the mean squared
    error against a 1024-spp render of the same view is lower than the undenoised image's.
    The denoised tensor then goes through rt_format_ppm_device: a valid P3 file."""
    import torch
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 4
    dev = torch.device("cuda", 0)
    with rt.Scene(t, w, l) as sc:
        noisy = torch.empty((48, 48, 3), dtype=torch.float32, device=dev)
        sc.render_device(cam, noisy.data_ptr(), seed=2,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
        aov = {"albedo": torch.empty((48, 48, 3), dtype=torch.float32, device=dev),
               "normal": torch.empty((48, 48, 3), dtype=torch.float32, device=dev),
               "depth": torch.empty((48, 48), dtype=torch.float32, device=dev)}
        st = sc.render_aov_device(cam, aov["albedo"].data_ptr(), aov["normal"].data_ptr(),
                                  aov["depth"].data_ptr(), None, n_samples=4, seed=2,
                                  stream=torch.cuda.current_stream(dev).cuda_stream)
        assert st["samples"] == st["segments"] == 48 * 48 * 4
        den = rt.denoise_device(noisy, aov)
        cam.SamplesPerPixel = 1024
        ref, _ = sc.render(cam, seed=9)
    a, b = noisy.cpu().numpy().astype(np.float64), den.cpu().numpy().astype(np.float64)
    assert np.isfinite(b).all()
    mse_noisy, mse_den = ((a - ref) ** 2).mean(), ((b - ref) ** 2).mean()
    print(f"cornell 48x48 4 spp: mse noisy {mse_noisy:.5f} denoised {mse_den:.5f}")
    assert mse_den < mse_noisy
    ppm = rt.format_ppm_device(den)
    lines = ppm.decode().split("\n")
    assert lines[:3] == ["P3", "48 48", "255"] and lines[-1] == ""
    body = [list(map(int, ln.split())) for ln in lines[3:-1]]
    assert len(body) == 48 * 48 and all(len(p) == 3 and 0 <= min(p) and max(p) <= 255 for p in body)
    assert ppm == rt.format_ppm(den.cpu().numpy())


def test_out_is_validated(rt, gpu):
    dev = torch.device("cuda", 0)
    rgb = torch.rand((6, 8, 3), device=dev)
    for bad in (torch.empty((6, 8, 3), device=dev, dtype=torch.float64),
                torch.empty((8, 6, 3), device=dev), torch.empty((6, 8, 3)),
                torch.empty((6, 8, 6), device=dev)[..., ::2]):
        with pytest.raises(ValueError):
            rt.denoise_device(rgb, None, out=bad)
    strided = torch.rand((6, 8, 6), device=dev)[..., ::2]
    with pytest.raises(ValueError):
        rt.denoise_device(strided, None, out=strided)
    ok = rt.denoise_device(strided, None)  # a copy is made for the input only
    assert ok.shape == (6, 8, 3) and ok.is_contiguous()
