"""rt_reproject_moments_device (rt_temporal.hip's k_reproject<.., .., true>) against the numpy
restatement of the definition pinned in include/rt_abi.h (tests/reproject_moments_ref.py), in the
three modes, on the fixtures that restatement builds.

Accuracy bars, the siblings' form: over the non-fragile pixels the GPU's max abs error against the
restatement in fp64 must be <= 8 x the error of the same restatement run in numpy fp32, plus the
siblings' margins (1e-6 x the largest finite |rgb| for rgb, 1e-5 for count, 1e-6 x the largest
finite |emission| for emission, 1e-6 for coverage).  For var and lum2 the margin is 1e-6 x the
largest lum2 of the fixture (the previous frame's plane and the current frame's Y(x)^2): the
subtraction q - y^2 cancels against y^2, not against the variance.  Every check prints its ratios."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import reproject_moments_ref as M
from tests.test_reproject_emit_gpu import bits
from tests.test_reproject_moments_ref import CASES, UNREACHABLE
from tests.test_reproject_ref import NONDEFAULT, SIZES

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("mode", M.MODES, ids=M.NAMES.values())


def to_dev(f):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(np.array(v, np.float32)).to(dev) if np.ndim(v) else v  # copies: read-only inputs
            for k, v in f.items() if v is not None}


def run_gpu(rt, mode, cam_p, prev, cam_c, cur, radius=0, **opts):
    res = rt.reproject_moments_device(M.NAMES[mode], cam_p, None if prev is None else to_dev(prev), cam_c, to_dev(cur),
                                      var_radius=radius, **opts)
    return {k: r.cpu().numpy() for k, r in zip(M.keys(mode), res)}


_ref = {}


def restated(rt, mode, w, h, case):
    """(fp64, fp32) restatements of a fixture, computed once"""
    if (mode, w, h, case) not in _ref:
        fx = M.fixture(rt, mode, w, h)
        opts, mo = CASES[case]
        _ref[(mode, w, h, case)] = tuple(
            M.reproject_moments(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=dt, **opts, **mo)
            for dt in (np.float64, np.float32))
    return _ref[(mode, w, h, case)]


def margins(mode, prev, cur, r64):
    def top(a):
        a = np.abs(np.asarray(a, np.float64))
        return float(a[np.isfinite(a)].max()) if np.isfinite(a).any() else 0.0
    lum2 = 1e-6 * max(top(prev["lum2"]), top(r64["lum2"]))
    m = {"rgb": 1e-6 * max(top(prev["rgb"]), top(cur["rgb"])), "var": lum2, "count": 1e-5, "lum2": lum2}
    if mode == M.LIGHT:
        m.update(emission=1e-6 * max(top(prev["emission"]), top(cur["emission"])), coverage=1e-6)
    return m


def finite_inputs(mode, cur):
    m = np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"])
    return m & np.isfinite(cur["emission"]).all(-1) if mode != M.PLAIN else m


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("w,h", SIZES)
@MODES
def test_parity(rt, gpu, mode, w, h, case):
    fx = M.fixture(rt, mode, w, h)
    prev, cur = fx["prev"], fx["cur"]
    opts, mo = CASES[case]
    r64, r32 = restated(rt, mode, w, h, case)
    got = run_gpu(rt, mode, fx["cams"][0], prev, fx["cams"][1], cur, **opts, **mo)
    assert r64["fragile"].mean() <= M.FRAGILE_CAP
    m = ~r64["fragile"] & finite_inputs(mode, cur)
    margin = margins(mode, prev, cur, r64)
    line = [f"reproject_moments {M.NAMES[mode]} {w}x{h} {case} ({int(m.sum())} of {w * h} pixels, history "
            f"{r64['history'].mean():.2f}, v_t {r64['took_t'].mean():.2f}, v_s {r64['took_s'].mean():.2f}):"]
    fails = []
    for k in M.keys(mode):
        e32 = float(np.abs(r32[k][m] - r64[k][m]).max()) if m.any() else 0.0
        eg = float(np.abs(got[k][m] - r64[k][m]).max()) if m.any() else 0.0
        bar = 8 * e32 + margin[k]
        line.append(f"{k} gpu {eg:.3e} fp32-numpy {e32:.3e} bar {bar:.3e} ratio {eg / max(e32, 1e-30):.2f}")
        if not eg <= bar:
            fails.append((k, eg, e32, bar))
    print(" | ".join(line))
    assert all(np.isfinite(got[k][m]).all() for k in M.keys(mode)) and (got["count"][m] > 0).all()
    assert (got["var"][m] >= 0).all() and (got["lum2"][m] >= 0).all()
    assert not fails, fails


@pytest.mark.parametrize("case", ["default", "nondefault"])
@MODES
def test_every_pixel_takes_the_estimate_the_restatement_names(rt, gpu, mode, case):
    """the kernel shows which estimate a pixel took only through the value.  Two more runs make the
    sets visible: with an unreachable min_frames every pixel with a surface sample takes v_s, with
    min_frames = 2 every pixel with surface history takes v_t (K >= 2 whenever there is history: the
    counts are integers).  On the non-fragile pixels, a pixel the restatement sends to v_s has the
    first run's var bits, one it sends to v_t has the second run's, and the two differ wherever the
    restatement's own two estimates differ by more than the parity bars.  The pass-through set
    writes lum2 = 0 and the current frame's bits"""
    for w, h in SIZES:
        fx = M.fixture(rt, mode, w, h)
        prev, cur = fx["prev"], fx["cur"]
        opts, mo = CASES[case]
        r64, _ = restated(rt, mode, w, h, case)
        args = (rt, mode, fx["cams"][0], prev, fx["cams"][1], cur)
        got = run_gpu(*args, **opts, **mo)
        all_s = run_gpu(*args, **opts, **dict(mo, min_frames=UNREACHABLE))
        all_t = run_gpu(*args, **opts, **dict(mo, min_frames=2.0))
        ok = ~r64["fragile"] & finite_inputs(mode, cur)
        s, t, keep = r64["took_s"] & ok, r64["took_t"] & ok, r64["zero"] & ~r64["fragile"]
        assert np.array_equal(bits(got["var"])[s], bits(all_s["var"])[s]), (w, h, "v_s")
        assert np.array_equal(bits(got["var"])[t], bits(all_t["var"])[t]), (w, h, "v_t")
        s64 = M.reproject_moments(mode, fx["gp"], prev, fx["gc"], cur, **opts, **dict(mo, min_frames=UNREACHABLE))
        apart = t & (np.abs(s64["var"] - r64["var"]) > 1e-3 * np.abs(r64["var"]) + 16 * margins(mode, prev, cur, r64)["var"])
        assert (bits(all_s["var"]) != bits(got["var"]))[apart].all(), (w, h)
        assert w * h < 100 or (apart.sum() > 10 and s.sum() > 10)
        assert not bits(got["lum2"])[keep].any()
        for k in M.keys(mode)[:-1]:
            assert np.array_equal(bits(got[k])[keep], bits(np.broadcast_to(cur[k], got[k].shape))[keep]), (w, h, k)


@MODES
def test_no_prev_is_a_prev_without_counts(rt, gpu, mode):
    """prev = NULL gives the bits of a prev whose counts are all 0: every pixel takes the no-history
    path, rgb, count, emission and coverage are the current frame's, var is the window's"""
    for w, h in SIZES:
        fx = M.fixture(rt, mode, w, h)
        prev, cur = fx["prev"], fx["cur"]
        a = run_gpu(rt, mode, None, None, fx["cams"][1], cur)
        b = run_gpu(rt, mode, fx["cams"][0], dict(prev, count=np.zeros((h, w), np.float32)), fx["cams"][1], cur)
        r64 = M.reproject_moments(mode, None, None, fx["gc"], cur)
        assert not r64["blend"].any()
        for k in M.keys(mode):
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k)
            if k not in ("var", "lum2"):
                assert np.array_equal(bits(a[k]), bits(np.broadcast_to(cur[k], a[k].shape))), (w, h, k)
        if w * h >= 100:
            assert (a["var"][r64["took_s"]] > 0).mean() > 0.9


@MODES
def test_repeatable_and_host_entry_matches_device(rt, gpu, mode):
    for (w, h), case in (((24, 17), "default"), ((131, 5), "nondefault"), ((3, 2), "radius8")):
        fx = M.fixture(rt, mode, w, h)
        opts, mo = CASES[case]
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a, b = run_gpu(rt, mode, *args, **opts, **mo), run_gpu(rt, mode, *args, **opts, **mo)
        kw = dict(opts, min_frames=mo.get("min_frames", 0.0), var_radius=mo.get("radius", 0))
        c = dict(zip(M.keys(mode), rt.reproject_moments(M.NAMES[mode], *args, **kw)))
        d = dict(zip(M.keys(mode), rt.reproject_moments(M.NAMES[mode], None, None, *args[2:], **kw)))
        e = run_gpu(rt, mode, None, None, *args[2:], **opts, **mo)
        for k in M.keys(mode):
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k, "two calls")
            assert np.array_equal(bits(a[k]), bits(c[k])), (w, h, k, "host entry")
            assert np.array_equal(bits(d[k]), bits(e[k])), (w, h, k, "host entry, no prev")


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@MODES
def test_switched_off_it_is_the_modes_entry(rt, gpu, mode, opts):
    """radius = -1 and an unreachable min_frames: rgb, count, emission and coverage are
    rt_reproject_device's, _emit_device's or _light_device's bits on the same inputs (a finite lum2
    plane: a NaN there is a tap rule the older entries do not have)"""
    fn = {M.PLAIN: rt.reproject_device, M.EMIT: rt.reproject_emit_device, M.LIGHT: rt.reproject_light_device}[mode]
    for w, h in SIZES:
        fx = M.fixture(rt, mode, w, h)
        prev = dict(fx["prev"], lum2=np.nan_to_num(fx["prev"]["lum2"]))
        a = run_gpu(rt, mode, fx["cams"][0], prev, fx["cams"][1], fx["cur"], radius=-1, min_frames=UNREACHABLE, **opts)
        p = {k: v for k, v in prev.items() if k != "lum2"}
        b = dict(zip(M.keys(mode)[:-1], (r.cpu().numpy() for r in fn(fx["cams"][0], to_dev(p), fx["cams"][1],
                                                                   to_dev(fx["cur"]), **opts))))
        for k in M.keys(mode)[:-1]:
            if k != "var":
                assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k)
