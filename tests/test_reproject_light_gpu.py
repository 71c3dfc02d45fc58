"""rt_reproject_light_device (rt_temporal.hip's k_reproject<true, true>) against the numpy
restatement of the definition pinned in include/rt_abi.h (tests/reproject_light_ref.py), on the
fixtures that restatement uses.

Accuracy bars, the parent test's form: over the non-fragile pixels the GPU's max abs error against
the restatement in fp64 must be <= 8 x the error of the same restatement run in numpy fp32, plus
the parent's margins (1e-6 x the largest finite |rgb| for rgb, 1e-6 x the largest finite input
variance for var, 1e-5 for count) and 1e-6 x the largest finite |emission| for emission and 1e-6
for coverage.  Every check prints its ratios."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import reproject_emit_ref as E
from tests import reproject_light_ref as L
from tests import reproject_ref as R
from tests.test_reproject_emit_gpu import bits
from tests.test_reproject_emit_gpu import margins as emit_margins
from tests.test_reproject_emit_gpu import run_gpu as run_parent
from tests.test_reproject_ref import NONDEFAULT, SIZES

pytestmark = pytest.mark.gpu
KEYS = L.KEYS


def run_gpu(rt, cam_p, prev, cam_c, cur, inplace=False, **opts):
    dev = torch.device("cuda", 0)
    p, c = ({k: torch.from_numpy(np.array(v, np.float32)).to(dev) if np.ndim(v) else v  # copies: read-only inputs
             for k, v in f.items() if v is not None} for f in (prev, cur))
    inplace = inplace and all(torch.is_tensor(c.get(k)) for k in KEYS)
    out = {k: c[k] for k in KEYS} if inplace else None
    res = rt.reproject_light_device(cam_p, p, cam_c, c, out=out, **opts)
    if inplace:
        assert all(r.data_ptr() == c[k].data_ptr() for r, k in zip(res, KEYS))
    return {k: r.cpu().numpy() for k, r in zip(KEYS, res)}


_ref = {}


def restated(rt, w, h, opts):
    """(fp64, fp32) restatements of a fixture, computed once"""
    key = (w, h, tuple(sorted(opts.items())))
    if key not in _ref:
        fx = L.fixture(rt, w, h)
        _ref[key] = tuple(L.reproject_light(fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=dt, **opts)
                          for dt in (np.float64, np.float32))
    return _ref[key]


def margins(prev, cur):
    fin = [np.abs(f["emission"][np.isfinite(f["emission"])]) for f in (prev, cur)]
    return dict(emit_margins(prev, cur), emission=1e-6 * float(max(fin[0].max(), fin[1].max())), coverage=1e-6)


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_parity(rt, gpu, w, h, opts):
    fx = L.fixture(rt, w, h)
    prev, cur = fx["prev"], fx["cur"]
    r64, r32 = restated(rt, w, h, opts)
    got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], cur, **opts)
    assert r64["fragile"].mean() <= L.FRAGILE_CAP
    m = ~r64["fragile"] & np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"]) & np.isfinite(cur["emission"]).all(-1)
    margin = margins(prev, cur)
    line = [f"reproject_light {w}x{h} {'nondefault' if opts else 'default'} ({int(m.sum())} of {w * h} pixels, "
            f"surface history {r64['history'].mean():.2f}, light history {r64['light_history'].mean():.2f}):"]
    fails = []
    for k in KEYS:
        e32 = float(np.abs(r32[k][m] - r64[k][m]).max()) if m.any() else 0.0
        eg = float(np.abs(got[k][m] - r64[k][m]).max()) if m.any() else 0.0
        bar = 8 * e32 + margin[k]
        line.append(f"{k} gpu {eg:.3e} fp32-numpy {e32:.3e} bar {bar:.3e} ratio {eg / max(e32, 1e-30):.2f}")
        if not eg <= bar:
            fails.append((k, eg, e32, bar))
    print(" | ".join(line))
    assert all(np.isfinite(got[k][m]).all() for k in KEYS) and (got["count"][m] > 0).all()
    assert ((got["coverage"][m] >= 0) & (got["coverage"][m] <= 1)).all()
    assert not fails, fails


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
def test_history_sets_are_exact(rt, gpu, opts):
    """on the non-fragile pixels the set of blended pixels, the set that found surface history and
    the set that found light history are the restatement's.  The GPU shows them in its count plane:
    a blended pixel has count_out = max(n_h, m_h) + n_c > count_cur.  A pixel with a surface
    sample blends when it finds history of either kind, which is light history (a surface tap is a
    light tap); a fully covered one blends only on surface history.  Neither set depends on the
    current coverage otherwise, so the fixture with the current coverage set to 0 everywhere shows
    the light-history set and with 1 everywhere the surface-history set"""
    for w, h in SIZES:
        fx = L.fixture(rt, w, h)
        prev, cur = fx["prev"], fx["cur"]
        r64, _ = restated(rt, w, h, opts)
        ok = ~r64["fragile"]
        sets = {}
        for name, cov in (("blend", None), ("light_history", 0.0), ("history", 1.0)):
            c = cur if cov is None else dict(cur, coverage=np.full((h, w), cov, np.float32))
            ref = r64 if cov is None else L.reproject_light(fx["gp"], prev, fx["gc"], c, **opts)
            got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], c, **opts)
            with np.errstate(invalid="ignore"):
                sets[name] = got["count"] > cur["count"]
            assert np.array_equal(ref["fragile"], r64["fragile"]) and np.array_equal(ref[name], ref["blend"])
            assert np.array_equal(ref[name], r64[name]), (w, h, name)   # the coverage of cur decides neither
            assert np.array_equal(sets[name][ok], r64[name][ok]), (w, h, name)
        assert not sets["blend"][~np.isfinite(cur["emission"]).all(-1)].any()
        assert not (sets["history"] & ~sets["light_history"])[ok].any()
        if w * h >= 100:
            assert 0 < r64["history"][ok].sum() < ok.sum()
            assert (not opts and h < 17) or (r64["light_history"] & ~r64["history"])[ok].any()


def test_pass_through_bits(rt, gpu):
    """invalid current pixels, misses, the pixel with NaN emission, the inside of the covered
    block and every pixel without history keep the current frame's bits in all five planes; so does
    the whole frame when no previous pixel has a count"""
    for w, h in ((24, 17), (131, 5)):
        fx = L.fixture(rt, w, h)
        prev, cur = fx["prev"], fx["cur"]
        r64, _ = restated(rt, w, h, {})
        got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], cur)
        invalid = ~(np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"]))
        nan_e = ~np.isfinite(cur["emission"]).all(-1)
        miss = cur["depth"] == 0
        keep = (invalid | miss | ~r64["blend"]) & ~r64["fragile"]
        assert nan_e.sum() == 1 and keep[nan_e].all() and miss.sum() > 0 and keep[miss].all()
        assert h < 17 or (keep & fx["block"] & r64["light_history"]).any()   # the inside of the light
        for k in KEYS:
            assert np.array_equal(bits(got[k])[keep], bits(cur[k])[keep]), (w, h, k)
    empty = dict(prev, count=np.zeros((h, w), np.float32))
    got = run_gpu(rt, fx["cams"][0], empty, fx["cams"][1], cur)
    for k in KEYS:
        assert np.array_equal(bits(got[k]), bits(cur[k])), k


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
def test_zero_emission_and_coverage_give_rt_reproject_bits(rt, gpu, opts):
    """the parent's fixtures with emission = 0 and coverage = 0: every light tap is a surface tap,
    (c - 0) / 1 and (1 - 0) z + 0 are exact, and out_emit is all zero"""
    for w, h in SIZES:
        fx = R.fixture(rt, w, h)
        zero = {"emission": np.zeros((h, w, 3), np.float32), "coverage": np.zeros((h, w), np.float32)}
        a = run_parent(rt, fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"], emit=False, **opts)
        b = run_gpu(rt, fx["cams"][0], dict(fx["prev"], **zero), fx["cams"][1], dict(fx["cur"], **zero), **opts)
        for k in ("rgb", "var", "count"):
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k)
        assert not bits(b["emission"]).any() and not bits(b["coverage"]).any(), (w, h)


def test_in_place_and_repeatable(rt, gpu):
    """out = cur's buffers and out_emit = cur_emit's give the bits of separate buffers; two calls
    give identical bits"""
    for w, h in ((24, 17), (131, 5)):
        fx = L.fixture(rt, w, h)
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a, b, c = run_gpu(rt, *args), run_gpu(rt, *args), run_gpu(rt, *args, inplace=True)
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])), (w, h, k)


def test_host_entry_matches_device(rt, gpu):
    for w, h in ((24, 17), (3, 2)):
        fx = L.fixture(rt, w, h)
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a = run_gpu(rt, *args, **NONDEFAULT)
        b = dict(zip(KEYS, rt.reproject_light(*args, **NONDEFAULT)))
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k)
    # without var and count planes, one number for the counts
    keys = ("rgb", "normal", "depth", "emission", "coverage")
    prev, cur = ({k: v for k, v in fx[f].items() if k in keys} for f in ("prev", "cur"))
    a = run_gpu(rt, fx["cams"][0], dict(prev, count=3.0), fx["cams"][1], dict(cur, count=1.0))
    b = dict(zip(KEYS, rt.reproject_light(fx["cams"][0], dict(prev, count=3.0), fx["cams"][1], dict(cur, count=1.0))))
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_a_rim_takes_the_history_of_its_coverage(rt, gpu):
    """the point of the light history, built so that it is deterministic: test_a_light_in_the_plane_
    stays_out_of_its_surroundings' plane z = -5 of surface radiance 0.5 and its half-pixel shift
    (pixel x gathers the previous pixels x - 1 and x), a block of fully covered pixels of emission
    15, and between the block and the plane a rim three columns wide whose coverage is 3/8 in the
    previous frame and 5/8 in the current one: two estimates of a true 1/2.  On the rim pixels whose
    two taps are both rim pixels rt_reproject_light blends the two: coverage 1/2, emission 7.5,
    rgb = 0.5 x 0.5 + 7.5 = 7.75 within the parity bar.  rt_reproject_emit re-lights the same pixels
    with the current frame's 5/8 alone: 0.375 x 0.5 + 9.375 = 9.5625."""
    w, h = 16, 12
    _, cam = R.cameras(rt, w, h)
    g = R.geometry(cam)
    step = float(np.linalg.norm(g["U"])) * 5.0 / 10.0   # a pixel's footprint on the plane (focus distance 10)
    cam_p, cam_c = R.cameras(rt, w, h, offset=(0.5 * step, 0.0, 0.0), yaw_deg=0.0)
    gp, gc = R.geometry(cam_p), R.geometry(cam_c)
    ys, xs = np.mgrid[0:h, 0:w]
    d = g["P00"] + xs[..., None] * g["U"] + ys[..., None] * g["V"] - g["C"]
    depth = (5.0 * np.sqrt((d * d).sum(-1)) / -d[..., 2]).astype(np.float32)
    rows = (ys >= 4) & (ys < 7)
    block, rim = (xs >= 3) & (xs < 6) & rows, (xs >= 6) & (xs < 9) & rows
    frames = []
    for kappa in (3 / 8, 5 / 8):
        cov = np.where(block, 1.0, np.where(rim, kappa, 0.0))
        emission = (cov[..., None] * 15.0) * np.ones(3)
        frames.append({"rgb": ((1 - cov)[..., None] * 0.5 + emission).astype(np.float32),
                       "var": np.full((h, w), 0.01, np.float32), "count": 4.0,
                       "normal": np.broadcast_to(np.float32((0, 0, 1)), (h, w, 3)).copy(), "depth": depth,
                       "emission": emission.astype(np.float32), "coverage": cov.astype(np.float32)})
    prev, cur = frames
    both = (xs >= 7) & (xs < 9) & (ys == 5)   # taps x - 1 and x in row y (and y - 1 or y + 1 at weight ~0): all rim
    light = run_gpu(rt, cam_p, prev, cam_c, cur)
    split = run_parent(rt, cam_p, prev, cam_c, cur)
    r64, r32 = (L.reproject_light(gp, prev, gc, cur, dt=dt) for dt in (np.float64, np.float32))
    assert r64["history"][both].all() and r64["light_history"][both].all()
    assert np.abs(r64["rgb"][both] - 7.75).max() < 1e-9 and np.abs(r64["coverage"][both] - 0.5).max() < 1e-9
    e32 = {k: float(np.abs(r32[k][both] - r64[k][both]).max()) for k in KEYS}
    err = float(np.abs(light["rgb"][both] - 7.75).max())
    err_k = float(np.abs(light["coverage"][both] - 0.5).max())
    err_e = float(np.abs(light["emission"][both] - 7.5).max())
    print(f"rim pixels with two rim taps: light {light['rgb'][both].min():.7f} .. {light['rgb'][both].max():.7f}, "
          f"split {split['rgb'][both].min():.7f} .. {split['rgb'][both].max():.7f}")
    print(f"|rgb - 7.75| gpu {err:.3e} fp32-numpy {e32['rgb']:.3e} bar {8 * e32['rgb'] + 15e-6:.3e} | |coverage - 0.5| "
          f"gpu {err_k:.3e} fp32-numpy {e32['coverage']:.3e} | |emission - 7.5| gpu {err_e:.3e} fp32-numpy {e32['emission']:.3e}")
    assert err <= 8 * e32["rgb"] + 1e-6 * 15.0
    assert err_k <= 8 * e32["coverage"] + 1e-6 and err_e <= 8 * e32["emission"] + 1e-6 * 15.0
    assert np.abs(light["count"][both] - 8.0).max() <= 1e-5
    # the split history's answer on the same pixels, within the same bar
    s64, s32 = (E.reproject_emit(gp, prev, gc, cur, dt=dt) for dt in (np.float64, np.float32))
    assert np.abs(s64["rgb"][both] - 9.5625).max() < 1e-9
    bar = 8 * float(np.abs(s32["rgb"][both] - s64["rgb"][both]).max()) + 1e-6 * 15.0
    assert np.abs(split["rgb"][both] - 9.5625).max() <= bar
    # the plane beyond the rim stays 0.5 and the inside of the block keeps its bits
    plane = ~(block | rim) & (xs != 9)
    assert np.abs(r64["rgb"][plane] - 0.5).max() < 1e-5
    assert (np.abs(light["rgb"][plane] - r64["rgb"][plane]).max()
            <= 8 * float(np.abs(r32["rgb"][plane] - r64["rgb"][plane]).max()) + 15e-6)
    inside = (xs >= 4) & (xs < 6) & rows
    for k in KEYS:
        assert np.array_equal(bits(light[k])[inside], bits(np.broadcast_to(cur[k], light[k].shape))[inside]), k
