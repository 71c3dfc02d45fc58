"""rt_reproject_spec_device (rt_temporal.hip's k_reproject<.., .., true, Clip, true>) against the numpy
restatement of the definition pinned in include/rt_abi.h (tests/reproject_spec_ref.py), in the three
modes, with and without copts, on the fixtures that restatement builds (the clip fixtures with
bounces planes).

Accuracy bars, tests/test_reproject_clip_gpu.py's: over the non-fragile pixels the GPU's max abs error
against the restatement in fp64 must be <= 8 x the error of the same restatement run in numpy fp32,
plus tests/test_reproject_moments_gpu.py's margins.  Every check prints its ratios."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import reproject_spec_ref as S
from tests.test_reproject_clip_gpu import run_clip, run_moments
from tests.test_reproject_clip_ref import CASES
from tests.test_reproject_emit_gpu import bits
from tests.test_reproject_moments_gpu import finite_inputs, margins, to_dev
from tests.test_reproject_ref import SIZES
from tests.test_reproject_spec_ref import assert_mirror_claim, mirror_figures

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("mode", S.MODES, ids=S.NAMES.values())


def run_spec(rt, mode, cam_p, prev, cam_c, cur, gamma=0.0, radius=0, **opts):
    res = rt.reproject_spec_device(S.NAMES[mode], cam_p, None if prev is None else to_dev(prev), cam_c, to_dev(cur),
                                   var_radius=radius, gamma=gamma, **opts)
    return {k: r.cpu().numpy() for k, r in zip(S.keys(mode), res)}


_ref = {}


def restated(rt, mode, w, h, case, clip):
    """(fp64, fp32) restatements of a fixture, computed once"""
    key = (mode, w, h, case, clip)
    if key not in _ref:
        fx = S.fixture(rt, mode, w, h)
        opts, mo, gamma = CASES[case]
        _ref[key] = tuple(S.reproject_spec(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"], gamma=gamma if clip else None,
                                           dt=dt, **opts, **mo) for dt in (np.float64, np.float32))
    return _ref[key]


@pytest.mark.parametrize("clip", [True, False], ids=["copts", "null-copts"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("w,h", SIZES)
@MODES
def test_parity(rt, gpu, mode, w, h, case, clip):
    fx = S.fixture(rt, mode, w, h)
    prev, cur = fx["prev"], fx["cur"]
    opts, mo, gamma = CASES[case]
    r64, r32 = restated(rt, mode, w, h, case, clip)
    got = run_spec(rt, mode, fx["cams"][0], prev, fx["cams"][1], cur, gamma=gamma if clip else None, **opts, **mo)
    assert r64["fragile"].mean() <= S.FRAGILE_CAP
    m = ~r64["fragile"] & finite_inputs(mode, cur)
    margin = margins(mode, prev, cur, r64)
    line = [f"reproject_spec {S.NAMES[mode]} {w}x{h} {case} {'copts' if clip else 'no copts'} ({int(m.sum())} of {w * h} "
            f"pixels, history {r64['history'].mean():.2f}, whole {r64['whole'].mean():.2f}):"]
    fails = []
    for k in S.keys(mode):
        e32 = float(np.abs(r32[k][m] - r64[k][m]).max()) if m.any() else 0.0
        eg = float(np.abs(got[k][m] - r64[k][m]).max()) if m.any() else 0.0
        bar = 8 * e32 + margin[k]
        line.append(f"{k} gpu {eg:.3e} fp32-numpy {e32:.3e} bar {bar:.3e} ratio {eg / max(e32, 1e-30):.2f}")
        if not eg <= bar:
            fails.append((k, eg, e32, bar))
    print(" | ".join(line))
    assert all(np.isfinite(got[k][m]).all() for k in S.keys(mode)) and (got["count"][m] > 0).all()
    assert (got["var"][m] >= 0).all() and (got["lum2"][m] >= 0).all()
    assert not fails, fails
    # a pixel whose b_c is not whole has the bits of the call without a previous frame
    alone = run_spec(rt, mode, None, None, fx["cams"][1], cur, gamma=gamma if clip else None, **opts, **mo)
    odd = ~r64["whole"]
    for k in S.keys(mode):
        assert np.array_equal(bits(got[k])[odd], bits(alone[k])[odd]), (k, "fractional b_c: the no-history path")
    if (w, h) == (24, 17):
        assert odd.sum() > 10


def _raw_call(rt, mode, fx, opts, mo, gamma, spec):
    """rt_reproject_spec_device through ctypes: spec None is spec == NULL, gamma None is copts == NULL"""
    import ctypes as C
    lib, dev = rt.lib(), torch.device("cuda", 0)
    w, h = fx["gc"]["w"], fx["gc"]["h"]
    prev, cur = to_dev(fx["prev"]), to_dev(fx["cur"])
    ptr = lambda t: t.data_ptr()  # noqa: E731
    fr = lambda f: rt._lib.RtFrame(ptr(f["rgb"]), ptr(f["var"]) if "var" in f else None, ptr(f["count"]),  # noqa: E731
                                   ptr(f["normal"]), ptr(f["depth"]), 0.0, 0)
    em = lambda f: rt.RtAovEmit(ptr(f["emission"]), None, ptr(f["coverage"])) if mode != S.PLAIN else None  # noqa: E731
    out = {k: torch.zeros((h, w, 3) if k in ("rgb", "emission") else (h, w), dtype=torch.float32, device=dev)
           for k in S.keys(S.LIGHT)}
    fo = rt._lib.RtFrame(ptr(out["rgb"]), ptr(out["var"]), ptr(out["count"]), None, None, 0.0, 0)
    eo = rt.RtAovEmit(ptr(out["emission"]), None, ptr(out["coverage"]))
    o, m = rt._reproject_opts(**opts), rt._lib.RtMomentsOpts(mo.get("min_frames", 0.0), mo.get("radius", 0))
    co = None if gamma is None else rt._lib.RtClipOpts(gamma)
    keep = None if spec is None else [torch.from_numpy(np.array(b, np.float32)).to(dev) for b in spec]
    sp = None if spec is None else rt._lib.RtSpecPlanes(ptr(keep[0]), ptr(keep[1]))
    fp, fc, ep, ec = fr(prev), fr(cur), em(prev), em(cur)
    cp, cc = fx["cams"][0].to_c(), fx["cams"][1].to_c()
    r = lambda x: None if x is None else C.byref(x)  # noqa: E731
    rc = lib.rt_reproject_spec_device(mode, r(cp), r(fp), r(ep), ptr(prev["lum2"]), r(cc), r(fc), r(ec), w, h, r(o), r(m),
                                      r(co), r(sp), r(fo), r(eo), ptr(out["lum2"]), 0, None)
    assert rc == 0, lib.rt_last_error()
    return {k: out[k].cpu().numpy() for k in S.keys(mode)}


@MODES
def test_null_spec_and_zero_bounces_are_the_clip_entry(rt, gpu, mode):
    """spec = NULL, and two bounces planes that are all zero: rt_reproject_clip_device's bits in every
    plane; with copts = NULL too, rt_reproject_moments_device's"""
    for (w, h), case in (((24, 17), "default"), ((131, 5), "nondefault"), ((3, 2), "radius8"), ((1, 1), "default")):
        fx = S.fixture(rt, mode, w, h)
        opts, mo, gamma = CASES[case]
        args = (rt, mode, fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        zero = (np.zeros((h, w), np.float32),) * 2
        for g, want in ((gamma, run_clip(*args, gamma=gamma, **opts, **mo)), (None, run_moments(*args, **opts, **mo))):
            for spec in (None, zero):
                got = _raw_call(rt, mode, fx, opts, mo, g, spec)
                for k in S.keys(mode):
                    assert np.array_equal(bits(got[k]), bits(want[k])), (w, h, case, g, spec is None, k)


@MODES
def test_repeatable_and_host_entry_matches_device(rt, gpu, mode):
    for (w, h), case in (((24, 17), "default"), ((131, 5), "nondefault"), ((3, 2), "radius8")):
        fx = S.fixture(rt, mode, w, h)
        opts, mo, gamma = CASES[case]
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        for g in (gamma, None):
            a, b = (run_spec(rt, mode, *args, gamma=g, **opts, **mo) for _ in range(2))
            kw = dict(opts, min_frames=mo.get("min_frames", 0.0), var_radius=mo.get("radius", 0), gamma=g)
            c = dict(zip(S.keys(mode), rt.reproject_spec(S.NAMES[mode], *args, **kw)))
            d = dict(zip(S.keys(mode), rt.reproject_spec(S.NAMES[mode], None, None, *args[2:], **kw)))
            e = run_spec(rt, mode, None, None, *args[2:], gamma=g, **opts, **mo)
            for k in S.keys(mode):
                assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k, "two calls")
                assert np.array_equal(bits(a[k]), bits(c[k])), (w, h, k, "host entry")
                assert np.array_equal(bits(d[k]), bits(e[k])), (w, h, k, "host entry, no prev")


def test_planar_mirror_claim(rt, gpu):
    """(a) and (b) of tests/test_reproject_spec_ref.py's claim, with the same assertions, through the
    device entries: the first-hit side through rt_reproject_clip_device with its default gamma and the
    chain side through rt_reproject_spec_device with the same; then both without the clamp (copts =
    NULL, which for the first-hit side is rt_reproject_moments_device)"""
    for gamma in (0.0, None):
        def reproject(cp, prev, cc, cur, chain):
            if chain:
                res = rt.reproject_spec_device("plain", cp, to_dev(prev), cc, to_dev(cur), gamma=gamma)
            elif gamma is None:
                res = rt.reproject_moments_device("plain", cp, to_dev(prev), cc, to_dev(cur))
            else:
                res = rt.reproject_clip_device("plain", cp, to_dev(prev), cc, to_dev(cur), gamma=gamma)
            return {k: r.cpu().numpy().astype(np.float64) for k, r in zip(S.keys(S.PLAIN), res)}
        assert_mirror_claim(f"GPU, gamma {gamma}", *mirror_figures(reproject, rt))
