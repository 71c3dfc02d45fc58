"""The denoisers' split mode (rt_denoise_emit_device, rt_denoise_var_emit_device and their host
entries; rt_denoise.hip k_dn_prep<VAR, true> / k_dn_emit_add) against a numpy
restatement of the definition in include/rt_abi.h / DESIGN.md §15.

The restatement is the definition's own reduction to the parents': with x = rgb - emission
(a pixel the split declares invalid set to NaN) the parents' restatements (imported from
tests/test_denoise_gpu.py and tests/test_denoise_var_gpu.py) filter x demodulated by
surface_albedo, and the emission is added to the valid pixels of the result; invalid pixels
take rgb and var.  Bars: the parents' (8 e32 + 1e-6 for out, 8 e32_var + 1e-6 max var for
var_out, e32 the fp32 restatement's error against the fp64 one).  Every check prints its
ratios."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_denoise_gpu import atrous
from tests.test_denoise_var_gpu import inputs, svgf

pytestmark = pytest.mark.gpu

E_VAL = 0.5  # the block's emission, every channel


def split_restated(filt, rgb, var, em, salb, cov, normal, depth, dt, **kw):
    """-> (out, var_out or None, valid), every operation in dtype dt"""
    r0, e = np.asarray(rgb).astype(dt), np.asarray(em).astype(dt)
    extra = np.isfinite(e).all(-1) & (np.asarray(cov) < 1)  # a NaN coverage: not below 1
    with np.errstate(all="ignore"):
        x = r0 - e
    x[~extra] = np.nan
    if filt == "plain":
        valid = np.isfinite(r0).all(-1) & extra
        o = atrous(x, salb, normal, depth, dt=dt, **kw)
        with np.errstate(all="ignore"):
            return np.where(valid[..., None], o + e, r0), None, valid
    v0 = np.asarray(var).astype(dt)
    valid = np.isfinite(r0).all(-1) & np.isfinite(v0) & extra
    o, v = svgf(x, var, salb, normal, depth, dt=dt, **kw)
    with np.errstate(all="ignore"):
        return np.where(valid[..., None], o + e, r0), np.where(valid, v, v0), valid


_split = {}


def block_of(h, w):
    """the 6 x 4 emitter block (clipped to the image) and its one-pixel rim, centred so that at
    width 131 it crosses the 64-pixel tile border"""
    ys, xs = np.mgrid[0:h, 0:w]
    r0, c0 = max(0, h // 2 - 2), w // 2 - 3
    if h < 5 or w < 9:  # 1 x 1, 3 x 2: no room for a block: pixel (0, 0) is a rim pixel
        return np.zeros((h, w), bool), (ys == 0) & (xs == 0)
    block = (ys >= r0) & (ys < r0 + 4) & (xs >= c0) & (xs < c0 + 6)
    ring = (ys >= r0 - 1) & (ys < r0 + 5) & (xs >= c0 - 1) & (xs < c0 + 7) & ~block
    return block, ring


def split_inputs(h=17, w=24, rim=True, nan_emission=True):
    """tests/test_denoise_var_gpu.py's inputs plus the emitter block: inside it coverage 1,
    emission 0.5 and rgb = emission; on its rim coverage 0.5 (emission 0.25 added to rgb); one
    NaN emission pixel; surface_albedo = albedo (1 - coverage).  Computed once, read-only.
    -> (rgb, var, emission, surface_albedo, coverage, normal, depth, albedo, block)"""
    key = (h, w, rim, nan_emission)
    if key not in _split:
        rgb0, albedo, normal, depth, var = inputs(h, w)
        block, ring = block_of(h, w)
        if not rim:
            ring = np.zeros_like(ring)
        cov = np.where(block, 1.0, np.where(ring, 0.5, 0.0)).astype(np.float32)
        em = (np.float32(E_VAL) * cov)[..., None].repeat(3, -1).astype(np.float32)
        rgb = np.array(rgb0)
        rgb[ring] += np.float32(E_VAL * 0.5)
        rgb[block] = E_VAL
        if nan_emission and h > 2 and w > 2:
            em[1, w - 2, 1] = np.nan
        salb = (albedo * (1 - cov)[..., None]).astype(np.float32)
        arrs = (rgb, np.array(var), em, salb, cov, normal, depth, albedo, block)
        for a in arrs:
            a.setflags(write=False)
        _split[key] = arrs
    return _split[key]


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, np.float32)).to(torch.device("cuda", 0))


def gpu_split(rt, filt, rgb, var, em, salb, cov, normal, depth, inplace=False, want_var=True, **opts):
    """-> (out, var_out or None) through the device entry points"""
    t, v = dev(rgb), dev(var)
    aov = {k: dev(a) for k, a in (("normal", normal), ("depth", depth), ("emission", em),
                                  ("surface_albedo", salb), ("coverage", cov)) if a is not None}
    if filt == "plain":
        out = rt.denoise_device(t, aov, out=t if inplace else None, split_emitters=True, **opts)
        vo = None
    else:
        vo = None if not want_var else v if inplace else torch.empty_like(v)
        out = rt.denoise_var_device(t, v, aov, out=t if inplace else None, var_out=vo, split_emitters=True,
                                    **opts)
    if inplace:
        assert out.data_ptr() == t.data_ptr()
    return out.cpu().numpy(), None if vo is None else vo.cpu().numpy()


def gpu_parent(rt, filt, rgb, var, albedo, normal, depth, **opts):
    t, v = dev(rgb), dev(var)
    aov = {k: dev(a) for k, a in (("albedo", albedo), ("normal", normal), ("depth", depth)) if a is not None}
    if filt == "plain":
        return rt.denoise_device(t, aov, **opts).cpu().numpy(), None
    vo = torch.empty_like(v)
    out = rt.denoise_var_device(t, v, aov, var_out=vo, **opts)
    return out.cpu().numpy(), vo.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(rt, filt, h=17, w=24, iterations=5, demodulate=1, want_var=True):
    rgb, var, em, salb, cov, normal, depth, _, block = split_inputs(h, w)
    kw = dict(iterations=iterations, demodulate=bool(demodulate))
    o64, v64, valid = split_restated(filt, rgb, var, em, salb, cov, normal, depth, np.float64, **kw)
    o32, v32, _ = split_restated(filt, rgb, var, em, salb, cov, normal, depth, np.float32, **kw)
    got, gvar = gpu_split(rt, filt, rgb, var, em, salb, cov, normal, depth, want_var=want_var,
                          iterations=iterations, demodulate=demodulate)
    e32 = float(np.abs(o32[valid] - o64[valid]).max()) if valid.any() else 0.0
    eg = float(np.abs(got[valid] - o64[valid]).max()) if valid.any() else 0.0
    bar = 8 * e32 + 1e-6
    msg = (f"{filt} emit {w}x{h} it {iterations} demod {int(demodulate)}: out gpu {eg:.3e} fp32-numpy "
           f"{e32:.3e} bar {bar:.3e} ratio {eg / max(e32, 1e-30):.2f}")
    # invalid pixels (the block, the NaN emission, the parents' NaN / Inf pixels): the input's bits
    assert np.array_equal(bits(got)[~valid], bits(rgb)[~valid])
    assert (~valid)[block].all() and np.isfinite(got[valid]).all()
    if filt == "var" and want_var:
        vmax = float(np.asarray(var)[np.isfinite(var)].max())
        e32v = float(np.abs(v32[valid] - v64[valid]).max()) if valid.any() else 0.0
        egv = float(np.abs(gvar[valid] - v64[valid]).max()) if valid.any() else 0.0
        barv = 8 * e32v + 1e-6 * vmax
        msg += f" | var gpu {egv:.3e} fp32-numpy {e32v:.3e} bar {barv:.3e} ratio {egv / max(e32v, 1e-30):.2f}"
        print(msg)
        assert np.array_equal(bits(gvar)[~valid], bits(var)[~valid])
        assert np.isfinite(gvar[valid]).all() and (gvar[valid] >= 0).all()
        assert egv <= barv, (egv, e32v, barv)
    else:
        assert gvar is None
        print(msg)
    assert eg <= bar, (eg, e32, bar)
    return got, gvar


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("filt", ["plain", "var"])
def test_numeric_parity(rt, gpu, filt, iterations, demodulate):
    """24 x 17 with the block, its rim, the NaN emission pixel and the parents' non-finite
    pixels: every kernel variant as the last iteration, with and without demodulation"""
    check(rt, filt, iterations=iterations, demodulate=demodulate)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 131)])
@pytest.mark.parametrize("filt", ["plain", "var"])
def test_other_sizes(rt, gpu, filt, h, w):
    """1 x 1, 3 x 2 and 131 x 5, where the block lies across the border of the first 64-pixel tile"""
    check(rt, filt, h, w)


def test_without_var_out(rt, gpu):
    a, _ = check(rt, "var", want_var=False)
    b, _ = check(rt, "var")
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("filt", ["plain", "var"])
def test_reduces_to_the_parent(rt, gpu, filt):
    """emission 0, coverage 0, surface_albedo = albedo: the parent's bits, out and var_out"""
    rgb, albedo, normal, depth, var = inputs()
    zero3, zero = np.zeros_like(rgb), np.zeros_like(var)
    a, av = gpu_split(rt, filt, rgb, var, zero3, albedo, zero, normal, depth, iterations=5)
    b, bv = gpu_parent(rt, filt, rgb, var, albedo, normal, depth, iterations=5)
    assert np.array_equal(a, b, equal_nan=True)
    fin = np.isfinite(rgb).all(-1)
    assert np.array_equal(bits(a)[~fin], bits(b)[~fin])
    if filt == "var":
        assert np.array_equal(av, bv, equal_nan=True)


@pytest.mark.parametrize("filt", ["plain", "var"])
def test_emitters_are_skipped_exactly(rt, gpu, filt):
    """coverage in {0, 1}: outside the block the result is the parent's on the image with the
    block cut out (NaN); inside it the input's bits.  The parent on the unsplit inputs (the
    light's albedo, 15, in the block) changes block pixels: the defect the split removes."""
    rgb, var, em, salb, cov, normal, depth, albedo, block = split_inputs(rim=False, nan_emission=False)
    assert set(np.unique(cov)) == {0.0, 1.0} and (em[~block] == 0).all()
    got, gvar = gpu_split(rt, filt, rgb, var, em, salb, cov, normal, depth, iterations=5)
    cut = np.array(rgb)
    cut[block] = np.nan
    ref, rvar = gpu_parent(rt, filt, cut, var, salb, normal, depth, iterations=5)
    assert np.array_equal(got[~block], ref[~block], equal_nan=True)
    assert np.array_equal(bits(got)[block], bits(rgb)[block])
    if filt == "var":
        assert np.array_equal(gvar[~block], rvar[~block], equal_nan=True)
        assert np.array_equal(bits(gvar)[block], bits(var)[block])
    # the unsplit inputs: first on the fp64 restatement, then on the GPU
    unsplit = np.where(block[..., None], np.float32(15.0), albedo).astype(np.float32)
    kw = dict(iterations=5, demodulate=True)
    r64 = (atrous(rgb, unsplit, normal, depth, **kw) if filt == "plain"
           else svgf(rgb, var, unsplit, normal, depth, **kw)[0])
    moved64 = float(np.abs(r64[block] - np.asarray(rgb, np.float64)[block]).max())
    par, _ = gpu_parent(rt, filt, rgb, var, unsplit, normal, depth, iterations=5)
    moved = float(np.abs(par[block] - rgb[block]).max())
    print(f"{filt}: the parent on the unsplit inputs moves a block pixel by {moved64:.3e} (fp64 restatement) "
          f"{moved:.3e} (gpu); the split by 0")
    assert moved64 > 1e-3
    assert moved > 1e-3


@pytest.mark.parametrize("filt", ["plain", "var"])
def test_aliasing(rt, gpu, filt):
    """out is rgb and var_out is var: the bits of separate buffers, pass-through pixels included"""
    rgb, var, em, salb, cov, normal, depth, _, block = split_inputs()
    a, av = gpu_split(rt, filt, rgb, var, em, salb, cov, normal, depth, iterations=5)
    b, bv = gpu_split(rt, filt, rgb, var, em, salb, cov, normal, depth, iterations=5, inplace=True)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(b)[block], bits(rgb)[block])
    if filt == "var":
        assert np.array_equal(bits(av), bits(bv)) and np.array_equal(bits(bv)[block], bits(var)[block])


@pytest.mark.parametrize("filt", ["plain", "var"])
def test_host_entry_points_match_device(rt, gpu, filt):
    rgb, var, em, salb, cov, normal, depth, _, _ = split_inputs()
    aov = {"normal": normal, "depth": depth, "emission": em, "surface_albedo": salb, "coverage": cov}
    b, bv = gpu_split(rt, filt, rgb, var, em, salb, cov, normal, depth, iterations=4)
    if filt == "plain":
        a = rt.denoise(rgb, aov, split_emitters=True, iterations=4)
    else:
        a, av = rt.denoise_var(rgb, var, aov, return_var=True, split_emitters=True, iterations=4)
        assert np.array_equal(bits(av), bits(bv))
    assert np.array_equal(bits(a), bits(b))


def test_end_to_end_cornell_and_ppm(rt, gpu):
    """Cornell 48 x 48, 4 passes x 4 spp -> split feature pass -> Accumulator.denoise_device(
    split_emitters=True) -> quantize and PPM.  The result is finite and the pixels the feature
    pass sees covered by the light keep the resolved mean's bits.  The MSE figures against a
    64-pass mean are printed, not asserted (DESIGN.md §15 reports the measurement)."""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 4
    d0 = torch.device("cuda", 0)
    shapes = {"albedo": 3, "normal": 3, "depth": 0, "emission": 3, "surface_albedo": 3, "coverage": 0}
    with rt.Scene(t, w, l) as sc:
        with sc.accumulator(cam, max_passes=4) as acc:
            for seed in (1, 2, 3, 4):
                acc.add(seed)
            aov = {k: torch.empty((48, 48, c) if c else (48, 48), dtype=torch.float32, device=d0)
                   for k, c in shapes.items()}
            sc.render_aov_device(cam, aov["albedo"].data_ptr(), aov["normal"].data_ptr(),
                                 aov["depth"].data_ptr(), None, n_samples=4, seed=1,
                                 stream=torch.cuda.current_stream(d0).cuda_stream,
                                 emission=aov["emission"].data_ptr(),
                                 surface_albedo=aov["surface_albedo"].data_ptr(),
                                 coverage=aov["coverage"].data_ptr())
            den = acc.denoise_device(aov, split_emitters=True)
            unsplit = acc.denoise_device(aov)
            mean = torch.empty((48, 48, 3), dtype=torch.float32, device=d0)
            acc.resolve_device(mean, None)
        with sc.accumulator(cam, max_passes=64) as big:
            for seed in range(101, 165):
                big.add(seed)
            ref, _ = big.resolve()
    a, b, u = (x.cpu().numpy() for x in (mean, den, unsplit))
    cov = aov["coverage"].cpu().numpy()
    assert np.isfinite(b).all()
    full = cov == 1.0
    assert full.any() and np.array_equal(bits(b)[full], bits(a)[full])
    lit = cov > 0
    ref = ref.astype(np.float64)
    mse = {k: (float(((x - ref) ** 2).mean()), float(((x - ref) ** 2)[lit].sum() / ref.size))
           for k, x in (("mean", a), ("guided", u), ("guided+split", b))}
    print("cornell 48x48 4 x 4 spp against a 64-pass mean, mse whole image (share of the "
          f"{int(lit.sum())} light pixels): " + ", ".join(f"{k} {v[0]:.5f} ({v[1]:.5f})" for k, v in mse.items()))
    q = rt.quantize_device(den)
    assert q.shape == (48, 48, 3) and q.dtype == torch.uint8
    ppm = rt.format_ppm_device(den)
    assert ppm.startswith(b"P3\n48 48\n255\n") and ppm == rt.format_ppm(b)
