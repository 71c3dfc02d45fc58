"""rt_reproject_clip_device (rt_temporal.hip's k_reproject<.., .., true, true>) against the numpy
restatement of the definition pinned in include/rt_abi.h (tests/reproject_clip_ref.py), in the three
modes, on the fixtures that restatement builds (the moments fixtures with a stale block).

Accuracy bars, the moments test's: over the non-fragile pixels the GPU's max abs error against the
restatement in fp64 must be <= 8 x the error of the same restatement run in numpy fp32, plus
tests/test_reproject_moments_gpu.py's margins (rgb scaled by the fixture's largest finite |rgb|,
var and lum2 by its largest lum2).  Every check prints its ratios."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import reproject_clip_ref as K
from tests.test_reproject_clip_ref import CASES
from tests.test_reproject_emit_gpu import bits
from tests.test_reproject_moments_gpu import finite_inputs, margins, to_dev
from tests.test_reproject_ref import SIZES

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("mode", K.MODES, ids=K.NAMES.values())


def _out(mode, res):
    return {k: r.cpu().numpy() for k, r in zip(K.keys(mode), res)}


def run_clip(rt, mode, cam_p, prev, cam_c, cur, gamma=0.0, radius=0, **opts):
    return _out(mode, rt.reproject_clip_device(K.NAMES[mode], cam_p, None if prev is None else to_dev(prev), cam_c,
                                               to_dev(cur), var_radius=radius, gamma=gamma, **opts))


def run_moments(rt, mode, cam_p, prev, cam_c, cur, radius=0, **opts):
    return _out(mode, rt.reproject_moments_device(K.NAMES[mode], cam_p, None if prev is None else to_dev(prev), cam_c,
                                                  to_dev(cur), var_radius=radius, **opts))


_ref = {}


def restated(rt, mode, w, h, case):
    """(fp64, fp32) restatements of a fixture, computed once"""
    if (mode, w, h, case) not in _ref:
        fx = K.fixture(rt, mode, w, h)
        opts, mo, gamma = CASES[case]
        _ref[(mode, w, h, case)] = tuple(
            K.reproject_clip(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"], gamma=gamma, dt=dt, **opts, **mo)
            for dt in (np.float64, np.float32))
    return _ref[(mode, w, h, case)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("w,h", SIZES)
@MODES
def test_parity(rt, gpu, mode, w, h, case):
    fx = K.fixture(rt, mode, w, h)
    prev, cur = fx["prev"], fx["cur"]
    opts, mo, gamma = CASES[case]
    r64, r32 = restated(rt, mode, w, h, case)
    args = (rt, mode, fx["cams"][0], prev, fx["cams"][1], cur)
    got = run_clip(*args, gamma=gamma, **opts, **mo)
    off = run_moments(*args, **opts, **mo)
    assert r64["fragile"].mean() <= K.FRAGILE_CAP
    m = ~r64["fragile"] & finite_inputs(mode, cur)
    margin = margins(mode, prev, cur, r64)
    line = [f"reproject_clip {K.NAMES[mode]} {w}x{h} {case} ({int(m.sum())} of {w * h} pixels, history "
            f"{r64['history'].mean():.2f}, clampable {r64['clampable'].mean():.2f}, clamped {r64['clamped'].mean():.2f}):"]
    fails = []
    for k in K.keys(mode):
        e32 = float(np.abs(r32[k][m] - r64[k][m]).max()) if m.any() else 0.0
        eg = float(np.abs(got[k][m] - r64[k][m]).max()) if m.any() else 0.0
        bar = 8 * e32 + margin[k]
        line.append(f"{k} gpu {eg:.3e} fp32-numpy {e32:.3e} bar {bar:.3e} ratio {eg / max(e32, 1e-30):.2f}")
        if not eg <= bar:
            fails.append((k, eg, e32, bar))
    print(" | ".join(line))
    assert all(np.isfinite(got[k][m]).all() for k in K.keys(mode)) and (got["count"][m] > 0).all()
    assert (got["var"][m] >= 0).all() and (got["lum2"][m] >= 0).all()
    assert not fails, fails
    # the set of clamped pixels is the restatement's: a clamped pixel's colour is not the moments
    # entry's, any other pixel's is, bit for bit; and the planes the clamp does not reach (count, lum2,
    # LIGHT's emission and coverage) are the moments entry's everywhere
    ok = ~r64["fragile"] & finite_inputs(mode, cur)
    moved = (bits(got["rgb"]) != bits(off["rgb"])).any(-1)
    assert np.array_equal(moved[ok], r64["clamped"][ok]), (int((moved & ok).sum()), int((r64["clamped"] & ok).sum()))
    same = ok & ~r64["clamped"]
    for k in K.keys(mode):
        where = same if k in ("rgb", "var") else np.ones((h, w), bool)
        assert np.array_equal(bits(got[k])[where], bits(off[k])[where]), (k, "not the moments entry's bits")
    # the pass-through sets keep the current frame's bits, lum2 = 0
    keep = r64["zero"] & ~r64["fragile"]
    assert not bits(got["lum2"])[keep].any()
    for k in K.keys(mode)[:-1]:
        assert np.array_equal(bits(got[k])[keep], bits(np.broadcast_to(cur[k], got[k].shape))[keep]), (k, "pass-through")
    if (w, h) == (24, 17):
        assert (r64["clamped"] & ok).sum() > 10 and (r64["clampable"] & ~r64["clamped"] & ok).sum() > 10


@MODES
def test_null_copts_is_the_moments_entry(rt, gpu, mode):
    """copts = NULL through rt_reproject_clip_device: rt_reproject_moments_device's bits in every plane,
    with and without a window"""
    import ctypes as C
    lib, dev = rt.lib(), torch.device("cuda", 0)
    for (w, h), case in (((24, 17), "default"), ((131, 5), "nondefault"), ((3, 2), "radius8"), ((1, 1), "default"),
                         ((24, 17), None)):
        fx = K.fixture(rt, mode, w, h)
        opts, mo, _ = CASES[case] if case else ({}, dict(radius=-1), 0.0)
        args = (rt, mode, fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        want = run_moments(*args, **opts, **mo)
        prev, cur = to_dev(fx["prev"]), to_dev(fx["cur"])
        ptr = lambda t: t.data_ptr()  # noqa: E731
        fr = lambda f: rt._lib.RtFrame(ptr(f["rgb"]), ptr(f["var"]) if "var" in f else None, ptr(f["count"]),  # noqa: E731
                                       ptr(f["normal"]), ptr(f["depth"]), 0.0, 0)
        em = lambda f: rt.RtAovEmit(ptr(f["emission"]), None, ptr(f["coverage"])) if mode != K.PLAIN else None  # noqa: E731
        out = {k: torch.zeros((h, w, 3) if k in ("rgb", "emission") else (h, w), dtype=torch.float32, device=dev)
               for k in K.keys(K.LIGHT)}
        fo = rt._lib.RtFrame(ptr(out["rgb"]), ptr(out["var"]), ptr(out["count"]), None, None, 0.0, 0)
        eo = rt.RtAovEmit(ptr(out["emission"]), None, ptr(out["coverage"]))
        o, m = rt._reproject_opts(**opts), rt._lib.RtMomentsOpts(mo.get("min_frames", 0.0), mo.get("radius", 0))
        fp, fc, ep, ec = fr(prev), fr(cur), em(prev), em(cur)
        cp, cc = fx["cams"][0].to_c(), fx["cams"][1].to_c()
        r = lambda x: None if x is None else C.byref(x)  # noqa: E731
        rc = lib.rt_reproject_clip_device(mode, r(cp), r(fp), r(ep), ptr(prev["lum2"]), r(cc), r(fc), r(ec), w, h, r(o),
                                          r(m), None, r(fo), r(eo), ptr(out["lum2"]), 0, None)
        assert rc == 0, lib.rt_last_error()
        for k in K.keys(mode):
            assert np.array_equal(bits(out[k].cpu().numpy()), bits(want[k])), (w, h, case, k)


@MODES
def test_repeatable_and_host_entry_matches_device(rt, gpu, mode):
    for (w, h), case in (((24, 17), "default"), ((131, 5), "nondefault"), ((3, 2), "radius8")):
        fx = K.fixture(rt, mode, w, h)
        opts, mo, gamma = CASES[case]
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a, b = (run_clip(rt, mode, *args, gamma=gamma, **opts, **mo) for _ in range(2))
        kw = dict(opts, min_frames=mo.get("min_frames", 0.0), var_radius=mo.get("radius", 0), gamma=gamma)
        c = dict(zip(K.keys(mode), rt.reproject_clip(K.NAMES[mode], *args, **kw)))
        d = dict(zip(K.keys(mode), rt.reproject_clip(K.NAMES[mode], None, None, *args[2:], **kw)))
        e = run_clip(rt, mode, None, None, *args[2:], gamma=gamma, **opts, **mo)
        f = run_moments(rt, mode, None, None, *args[2:], **opts, **mo)
        for k in K.keys(mode):
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k, "two calls")
            assert np.array_equal(bits(a[k]), bits(c[k])), (w, h, k, "host entry")
            assert np.array_equal(bits(d[k]), bits(e[k])), (w, h, k, "host entry, no prev")
            assert np.array_equal(bits(e[k]), bits(f[k])), (w, h, k, "no history: nothing to clamp")


def test_a_stale_block_on_a_noise_free_plane_is_overruled(rt, gpu):
    """the synthetic claim.  Identical cameras, one plane, the current colour 0.2 everywhere without
    noise, the previous frame 1.0 inside a block, equal counts.  rt_reproject_moments leaves the block
    at the blend, 0.6; rt_reproject_clip leaves every pixel at 0.2, exactly: s = 0, the box is the
    point x_p, and the blend of x_p with itself is x_p"""
    from tests.test_reproject_clip_ref import _frames
    from tests import reproject_ref as R
    w, h = 24, 17
    y_prev = np.full((h, w), 0.2)
    y_prev[5:11, 7:15] = 1.0
    _, prev, cur = _frames(rt, w, h, 0.2, y_prev)
    cam = R.cameras(rt, w, h)[1]
    for mode in (K.PLAIN, K.EMIT, K.LIGHT):
        if mode != K.PLAIN:
            zeros = dict(emission=np.zeros((h, w, 3), np.float32), coverage=np.zeros((h, w), np.float32))
            prev, cur = dict(prev, **zeros), dict(cur, **zeros)
        off = run_moments(rt, mode, cam, prev, cam, cur)
        got = run_clip(rt, mode, cam, prev, cam, cur)
        inner = np.zeros((h, w), bool)
        inner[6:10, 8:14] = True
        print(f"{K.NAMES[mode]}: moments block {off['rgb'][inner].min():.6f} .. {off['rgb'][inner].max():.6f}, clip "
              f"{got['rgb'].min():.9f} .. {got['rgb'].max():.9f}, count {got['count'].min()} .. {got['count'].max()}")
        assert np.abs(off["rgb"][inner] - 0.6).max() < 1e-5
        assert (got["count"] > 1.5).all()                    # every pixel found its history
        assert np.array_equal(bits(got["rgb"]), bits(np.broadcast_to(np.float32(0.2), (h, w, 3))))
