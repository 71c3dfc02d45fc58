"""The progressive pass accumulator (rt_accum.hip) on the GPU, stated against
rt_render only: one pass is Scene.render bit for bit, the sums are exact and independent of
the order of the passes, the variance and the error figures are Welford's recurrence over the
passes' luminance images, and the state survives renders in between, resets and refusals.

Images are 37 x 23: 851 pixels, no multiple of 64 or 256, and 23 rows are no multiple of the
4-row chunk group.  16 spp unless stated."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

pytestmark = pytest.mark.gpu

LUM = np.array([0.2126, 0.7152, 0.0722])
EPS = 2.0 ** -24  # half an ulp of fp32, relative: the rounding of one fp32 image value


def _shape(cam, w=37, h=23, spp=16):
    cam.Width, cam.AspectRatio, cam.SamplesPerPixel = w, w / (h + 0.5), spp
    assert cam.image_size()[:2] == (w, h)
    return cam


def _demo(rt, name, spp=16):
    t, cam, w, l = rt.demo_scene(name)
    return t, _shape(cam, spp=spp), w, l


def _accumulate(sc, cam, seeds, max_passes=0, **kw):
    with sc.accumulator(cam, max_passes=max_passes, **kw) as acc:
        stats = [acc.add(s) for s in seeds]
        rgb, var = acc.resolve()
        return rgb, var, acc.info(), stats


@pytest.fixture(scope="module")
def cornell(rt, gpu):
    """The Cornell scene, its 37 x 23 camera and Scene.render's images of seeds 1-4, rendered
    once and left unchanged."""
    t, cam, w, l = _demo(rt, "cornell")
    with rt.Scene(t, w, l) as sc:
        imgs = {s: sc.render(cam, seed=s)[0] for s in (1, 2, 3, 4)}
        for v in imgs.values():
            v.setflags(write=False)
        yield sc, cam, imgs


# ---------------------------------------------------------------- 1. one pass is rt_render --
def _one_pass_cases():
    # (id, scene, camera changes, render / accumulator options, knobs)
    return [
        ("cornell", "cornell", {}, {}, {}),                       # record-loop kernel, chunk records
        ("cornell_smoke", "cornell_smoke", {}, {}, {}),
        ("book1_fused", "book1", {"w": 40}, {"mode": "fused"}, {}),
        ("book1_wavefront", "book1", {"w": 40}, {"mode": "wavefront"}, {}),  # atomics, no records
        ("cornell_csum0", "cornell", {}, {}, {"RT_CSUM": "0"}),   # fused kernel on pixel atomics
        ("cornell_rank1of3", "cornell", {}, {"rank": 1, "nranks": 3}, {}),
        # the two-phase chunk plan, forced as tests/test_render_gpu.py test_tail_phase_is_bitwise
        # forces it (64 spp: a 32-sample first phase and 4-sample tail chunks)
        ("book1_two_phase", "book1", {"w": 40, "spp": 64}, {"chunk": 32},
         {"RT_TAIL_FRAC": "4", "RT_TAIL_K": "4"}),
    ]


@pytest.mark.parametrize("max_passes", [1, 64])
@pytest.mark.parametrize("case", _one_pass_cases(), ids=lambda c: c[0])
def test_one_pass_is_rt_render(rt, gpu, tune, case, max_passes):
    """A single pass resolves to Scene.render's image of the same seed, bit for bit, through
    every way a pass leaves its sums (chunk records of one and two phases, pixel atomics of the
    fused and the wavefront kernels, a row share), whether the accumulator is sized for 1 pass
    or for 64 (a lower fixed-point limit, which no sample of these scenes reaches)."""
    _, name, shape, opts, knobs = case
    t, cam, w, l = rt.demo_scene(name)
    if "w" in shape:  # book1: its own aspect ratio at width 40
        cam.Width, cam.SamplesPerPixel = shape["w"], shape.get("spp", 16)
    else:
        _shape(cam)
    for k, v in knobs.items():
        tune(k, v)
    seed = 5
    with rt.Scene(t, w, l) as sc:
        ref, st = sc.render(cam, seed=seed, **opts)
        with sc.accumulator(cam, max_passes=max_passes, **opts) as acc:
            ps = acc.add(seed)
            assert ps["overflow_samples"] == 0
            rgb, var = acc.resolve()
            assert acc.passes == 1
    assert ps["samples"] == st["samples"] and ps["segments"] == st["segments"]
    assert ps["chunk_records"] == st["chunk_records"] and ps["mode"] == st["mode"]
    if "two_phase" in case[0] or "csum0" in case[0] or "wavefront" in case[0]:
        assert ps["chunk_records"] == (1 if "two_phase" in case[0] else 0)
    assert rgb.shape == ref.shape and np.array_equal(rgb, ref, equal_nan=True)
    assert var.shape == ref.shape[:2] and not var.any()


# ------------------------------------------------------------------- 2. same seed twice --
def test_same_seed_twice(cornell):
    """Two passes of one seed: the integer sums double and the scale halves, both exactly, so
    the image is the single render's bits; the two luminances are equal, so var is exactly 0."""
    sc, cam, imgs = cornell
    rgb, var, info, _ = _accumulate(sc, cam, [3, 3], max_passes=2)
    assert np.array_equal(rgb, imgs[3])
    assert not var.any() and info["rms_std_error"] == 0.0 and info["passes"] == 2


# -------------------------------------------------------------------- 3. order invariance --
def test_order_invariance(cornell):
    """The sums are integers: any order of the same passes gives the same image bits.  Welford's
    fp64 recurrence depends on the order in its last bits only: var agrees to a relative 1e-9."""
    sc, cam, _ = cornell
    a, va, ia, _ = _accumulate(sc, cam, (1, 2, 3, 4))
    b, vb, ib, _ = _accumulate(sc, cam, (3, 1, 4, 2))
    assert np.array_equal(a, b)
    assert va.any()
    assert (np.abs(va.astype(np.float64) - vb) <= 1e-9 * np.maximum(va, vb)).all()
    assert abs(ia["rms_std_error"] - ib["rms_std_error"]) <= 1e-9 * ia["rms_std_error"]


# ----------------------------------------------------------------------- 4. against numpy --
def _welford(ys):
    """the fold kernel's recurrence, in fp64, over the luminance images in the given order"""
    mean, m2 = np.zeros_like(ys[0]), np.zeros_like(ys[0])
    for n, y in enumerate(ys, 1):
        d = y - mean
        mean = mean + d / n
        m2 = m2 + d * (y - mean)
    return mean, m2


def test_against_numpy(cornell):
    """The accumulator over seeds 1-4 against numpy on Scene.render's four fp32 images I_k.

    The device works on the exact pass values X_k (fp64 of exact integer sums); the test only
    has I_k = fl32(X_k), |I_k - X_k| <= EPS |X_k| with EPS = 2^-24 (half an ulp; the values are
    multiples of 2^-32 / 16, far above the denormal range).

    rgb: |mean_k I_k - mean_k X_k| <= EPS max|I| and the result's own rounding adds EPS max|I|:
    within 2^-23 max_p |I_p| per channel.

    Luminance: Y = 0.2126 r + 0.7152 g + 0.0722 b of non-negative values, so a pixel's pass
    luminance differs between test and device by at most e = EPS (1 + 2^-23) Ymax, Ymax the
    pixel's largest pass luminance (the factor turns a bound relative to X into one relative to
    I).  Taking the test's values as the base and the device's as y_k + delta_k, |delta_k| <= e,
    the deviations d_k = y_k - mean move by eta_k = delta_k - mean(delta), |eta_k| <= 2 e, and
      M2' - M2 = sum_k (2 d_k eta_k + eta_k^2)    exactly, so
      |var' - var| <= (4 e sum_k |d_k| + 4 n e^2) / (n (n - 1)).
    fp64 arithmetic adds at most 8 roundings of magnitudes <= Ymax^2 per Welford step on either
    side: n 2^-50 Ymax^2 / (n (n - 1)); the fp32 result adds EPS var (+ the smallest denormal).

    info: mean_luminance is a mean of Welford means, each within e of the test's, plus the
    reduction's npix fp64 roundings.  With a = mean(var) and Da the mean of the var bounds
    above (without the fp32 output rounding: info reduces the fp64 values),
    |sqrt(a') - sqrt(a)| <= min(sqrt(Da), Da / sqrt(a)).  rel_error = r / (m + 1e-6) moves by at
    most (Dr + (r / b) Dm) / (b - Dm) with b = m + 1e-6."""
    sc, cam, imgs = cornell
    seeds = (1, 2, 3, 4)
    n = len(seeds)
    rgb, var, info, _ = _accumulate(sc, cam, seeds, max_passes=4)
    I = np.stack([imgs[s].astype(np.float64) for s in seeds])
    assert np.isfinite(I).all() and (I >= 0).all()
    err = np.abs(rgb.astype(np.float64) - I.mean(axis=0))
    bound = 2.0 ** -23 * np.abs(I).max(axis=(0, 1, 2))
    print("rgb: max error per channel", err.max(axis=(0, 1)), "bound", bound)
    assert (err <= bound).all()

    Y = I @ LUM
    mean, m2 = _welford(list(Y))
    var_ref = m2 / (n * (n - 1))
    ymax = Y.max(axis=0)
    e = EPS * (1 + 2.0 ** -23) * ymax
    dvar = (4 * e * np.abs(Y - Y.mean(axis=0)).sum(axis=0) + 4 * n * e * e + n * 2.0 ** -50 * ymax ** 2) / (n * (n - 1))
    tol_var = dvar + EPS * (var_ref + dvar) + 2.0 ** -149
    verr = np.abs(var.astype(np.float64) - var_ref)
    print("var: max error", verr.max(), "of", var_ref.max(), "largest error / bound", (verr / tol_var).max())
    assert var_ref.max() > 0 and (verr <= tol_var).all()

    npix = Y[0].size
    assert info["passes"] == n and info["max_passes"] == 4 and info["samples_per_pixel"] == 16 * n
    assert info["nonfinite_pixels"] == 0
    m_ref, a_ref = mean.mean(), var_ref.mean()
    Dm = e.mean() + npix * 2.0 ** -52 * m_ref
    Da = dvar.mean() + npix * 2.0 ** -52 * a_ref
    r_ref = np.sqrt(a_ref)
    Dr = min(np.sqrt(Da), Da / r_ref) + 2.0 ** -52 * r_ref
    b = m_ref + 1e-6
    Drel = (Dr + r_ref / b * Dm) / (b - Dm) + 2.0 ** -51 * r_ref / b
    print("info", info, "reference", (r_ref, m_ref, r_ref / b), "bounds", (Dr, Dm, Drel))
    assert abs(info["mean_luminance"] - m_ref) <= Dm
    assert abs(info["rms_std_error"] - r_ref) <= Dr
    assert abs(info["rel_error"] - r_ref / b) <= Drel


# --------------------------------------------------------------------- 5. state handling --
def test_reset_is_a_fresh_accumulator(cornell):
    sc, cam, _ = cornell
    fresh = _accumulate(sc, cam, (2, 4, 1), max_passes=3)
    with sc.accumulator(cam, max_passes=3) as acc:
        for s in (7, 8, 9):
            acc.add(s)
        acc.reset()
        assert acc.passes == 0
        for s in (2, 4, 1):
            acc.add(s)
        rgb, var = acc.resolve()
        info = acc.info()
    assert np.array_equal(rgb, fresh[0]) and np.array_equal(var, fresh[1]) and info == fresh[2]


def test_pass_beyond_max_passes_is_refused(rt, cornell):
    sc, cam, _ = cornell
    with sc.accumulator(cam, max_passes=2) as acc:
        acc.add(1)
        acc.add(2)
        before = acc.resolve() + (acc.info(),)
        with pytest.raises(rt.RtError) as e:
            acc.add(3)
        assert e.value.code == rt._lib.RT_ERR_INVALID
        after = acc.resolve() + (acc.info(),)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert before[2] == after[2] and after[2]["passes"] == 2


def test_renders_between_passes_do_not_disturb(rt, cornell):
    """rt_render of another seed and size between two passes reuses (and regrows) the render
    buffers a pass uses, never the accumulator's."""
    sc, cam, _ = cornell
    plain = _accumulate(sc, cam, (1, 2), max_passes=2)
    t2, other, _, _ = rt.demo_scene("cornell")
    other.Width, other.SamplesPerPixel = 61, 4
    with sc.accumulator(cam, max_passes=2) as acc:
        acc.add(1)
        sc.render(other, seed=11)
        acc.add(2)
        rgb, var = acc.resolve()
    assert np.array_equal(rgb, plain[0]) and np.array_equal(var, plain[1])


def test_zero_passes_and_repeatable_info(cornell):
    sc, cam, _ = cornell
    with sc.accumulator(cam) as acc:
        rgb, var = acc.resolve()
        i0 = acc.info()
        assert not rgb.any() and not var.any()
        assert i0["passes"] == 0 and i0["max_passes"] == 1024 and i0["samples_per_pixel"] == 0
        assert i0["rms_std_error"] == 0.0 and i0["rel_error"] == 0.0
        for s in (1, 2, 3):
            acc.add(s)
        a, b = acc.info(), acc.info()
    assert a == b and a["rms_std_error"] > 0 and a["passes"] == 3


# -------------------------------------------------------------------------- 6. side plane --
def test_side_plane(rt, gpu):
    """One light far above the fixed-point range, as tests/test_render_gpu.py
    test_sample_overflow_is_flagged_not_clamped builds it: its samples go to the fp64 side
    plane in every pass (and in every separate render), counted in overflow_samples.

    Tolerance, per pixel and channel, against the fp64 mean R of the four separate fp32 renders
    I_k (as in test_against_numpy): the inputs' rounding moves R by at most EPS mean_k |I_k|
    (1 + 2^-23) and the result's own rounding is EPS |rgb| <= EPS (|R| + the former); the side
    sums are fp64 additions of at most 4 x 16 samples per pixel in an order that may differ
    between a pass and the separate render, each within 2^-53 of the running sum: 64 x 2^-53
    max_k |I_k|, doubled for the two sides."""
    t = rt.Tree(1)
    world = t.list()
    t.add(world, t.quad((-1, -1, -1), (2, 0, 0), (0, 2, 0), t.light((3.0e8, 1.0, 0.5))))
    cam = _shape(rt.Camera(Background=(0, 0, 0)))
    cam.PositionCamera((0, 0, 3), (0, 0, 0))
    seeds = (1, 2, 3, 4)
    with rt.Scene(t, world, -1) as sc:
        I = np.stack([sc.render(cam, seed=s)[0].astype(np.float64) for s in seeds])
        rgb, var, info, stats = _accumulate(sc, cam, seeds, max_passes=4)
    assert all(st["overflow_samples"] > 0 for st in stats)
    assert np.isfinite(rgb).all() and np.isfinite(var).all() and info["nonfinite_pixels"] == 0
    assert (I[..., 0] > 1e8).any()
    R = I.mean(axis=0)
    dR = EPS * (1 + 2.0 ** -23) * np.abs(I).mean(axis=0)
    tol = dR + EPS * (np.abs(R) + dR) + 2 * 64 * 2.0 ** -53 * np.abs(I).max(axis=0)
    err = np.abs(rgb.astype(np.float64) - R)
    print("side plane: largest error / bound", (err[tol > 0] / tol[tol > 0]).max(), "largest value", R.max())
    assert (err <= tol).all()


# --------------------------------------------------------------------- 7. device pipeline --
def test_device_pipeline(rt, cornell):
    """resolve_device -> denoise_device -> quantize_device without leaving the device: the same
    bytes as resolve -> denoise -> quantize on the host over the same passes."""
    sc, cam, _ = cornell
    dev = torch.device("cuda", 0)
    aov = sc.render_aov(cam, n_samples=16, seed=1)
    with sc.accumulator(cam, max_passes=3) as acc:
        for s in (1, 2, 3):
            acc.add(s)
        rgb, var = acc.resolve()
        d_rgb = torch.empty(rgb.shape, dtype=torch.float32, device=dev)
        d_var = torch.empty(var.shape, dtype=torch.float32, device=dev)
        acc.resolve_device(d_rgb, d_var)
        only_rgb = torch.empty_like(d_rgb)
        acc.resolve_device(only_rgb)
        with pytest.raises(ValueError):
            acc.resolve_device(torch.empty((3, 3, 3), dtype=torch.float32, device=dev))
    assert np.array_equal(d_rgb.cpu().numpy(), rgb) and np.array_equal(d_var.cpu().numpy(), var)
    assert torch.equal(only_rgb, d_rgb)
    d_aov = {k: torch.from_numpy(aov[k]).to(dev) for k in ("albedo", "normal", "depth")}
    out = rt.quantize_device(rt.denoise_device(d_rgb, d_aov)).cpu().numpy()
    assert out.tobytes() == rt.quantize(rt.denoise(rgb, aov)).tobytes()


# ------------------------------------------------------------------------ 8. render_until --
def test_render_until(cornell):
    sc, cam, _ = cornell
    with sc.accumulator(cam, max_passes=8) as acc:
        i = acc.render_until(0.0, 5, seed=1)  # unreachable: stops at max_passes
        assert i["passes"] == 5 and acc.passes == 5 and i["rel_error"] > 0
        rgb, _ = acc.resolve()
    assert np.array_equal(rgb, _accumulate(sc, cam, (1, 2, 3, 4, 5), max_passes=8)[0])
    with sc.accumulator(cam, max_passes=8) as acc:
        i = acc.render_until(1e9, 8, seed=1)  # met at the first check: after the second pass
        assert i["passes"] == 2 and i["rel_error"] <= 1e9
