"""tests/reproject_moments_ref.py, the numpy restatement of rt_reproject_moments, on the CPU: hand
cases of the two variance estimates, its agreement with the modes' own restatements where the
moments are switched off, the statistical claim (v_t is an unbiased estimate of the variance of
the blended mean), and the fragile share of the fixtures the GPU test uses."""
import numpy as np
import pytest

from tests import reproject_moments_ref as M
from tests import reproject_ref as R
from tests.test_reproject_ref import NONDEFAULT, SIZES

# (rt_reproject_opts, min_frames and radius) of the parity cases: the defaults with every radius, and
# everything non-default together.  NONDEFAULT's depth_tol of 0.02 goes with the radius of 1 only: a
# plane's depth changes by about 2 % over 8 pixels of these small images, which would put every
# wide window on the threshold
CASES = {"default": ({}, {}), "radius8": ({}, dict(radius=8)), "radius-1": ({}, dict(radius=-1)),
         "nondefault": (NONDEFAULT, dict(min_frames=3.0, radius=1))}
UNREACHABLE = 1e30   # a min_frames no pixel reaches


def _plane(rt, w, h):
    """(geometry, normal, depth) of the plane z = -5 seen by reproject_ref's current camera"""
    _, cam = R.cameras(rt, w, h)
    g = R.geometry(cam)
    ys, xs = np.mgrid[0:h, 0:w]
    d = g["P00"] + xs[..., None] * g["U"] + ys[..., None] * g["V"] - g["C"]
    depth = (5.0 * np.sqrt((d * d).sum(-1)) / -d[..., 2]).astype(np.float32)
    return g, np.broadcast_to(np.float32((0, 0, 1)), (h, w, 3)).copy(), depth


def _sequence(g, normal, depth, frames, **opts):
    """push grey frames (luminance planes, one pass each: var 0, count 1) through PLAIN with
    identical cameras; -> the last result"""
    prev = res = None
    for y in frames:
        cur = {"rgb": np.repeat(y[..., None], 3, -1).astype(np.float32), "count": 1.0, "normal": normal, "depth": depth}
        res = M.reproject_moments(M.PLAIN, g, prev, g, cur, **opts)
        prev = dict(cur, rgb=res["rgb"], var=res["var"], count=res["count"], lum2=res["lum2"])
    return res


def test_equal_counts_give_the_sample_variance_over_k(rt):
    """identical cameras, K frames of values y_1 .. y_K with equal counts, the cap (8 n_c) not
    reached: v = max(mean(y^2) - mean(y)^2, 0) / (K - 1) = sample variance / K"""
    w, h = 6, 4
    g, normal, depth = _plane(rt, w, h)
    rng = np.random.default_rng(3)
    for K in (5, 6, 8):   # not 4: K would sit on the default min_frames, a fragile decision
        ys = [np.float32(0.5 + rng.random((h, w))) for _ in range(K)]
        res = _sequence(g, normal, depth, ys, radius=-1 if K == 6 else 0)
        y64 = np.array(ys, np.float64)
        sy = 0.2126 + 0.7152 + 0.0722    # Y of a grey pixel, with the kernel's fp32 constants: 1 to 1e-7
        assert res["took_t"].all() == (K != 6)
        if K != 6:
            want = y64.var(0, ddof=1) / K
            # the history planes pass from frame to frame as fp32: each of the K - 1 hand-overs rounds
            # lum2 and rgb by 2^-24 of their size, and q - y^2 cancels against lum2, not the variance
            assert np.abs(res["var"] / sy ** 2 - want).max() <= K * 2.0 ** -24 * (y64 ** 2).max()
        else:   # no spatial estimate asked for: the mode's v_blend of one-pass frames, 0
            assert not res["var"].any()
        assert np.abs(res["lum2"] / sy ** 2 - (y64 ** 2).mean(0)).max() < 1e-6
        assert np.abs(res["count"] - K).max() < 1e-9
    # below min_frames the window speaks: K = 3 < 4, v_s / 3
    res = _sequence(g, normal, depth, ys[:3])
    assert res["took_s"].all() and not res["took_t"].any() and (res["var"] > 0).all()


def test_a_single_pixel_has_no_spatial_variance(rt):
    g, normal, depth = _plane(rt, 1, 1)
    cur = {"rgb": np.full((1, 1, 3), 0.7, np.float32), "count": 1.0, "normal": normal, "depth": depth}
    for radius in (0, 1, 8):
        res = M.reproject_moments(M.PLAIN, g, None, g, cur, radius=radius)
        assert res["took_s"].all() and res["var"][0, 0] == 0.0     # T = 1
        assert abs(res["lum2"][0, 0] - M.lum(np.float64(cur["rgb"]))[0, 0] ** 2) < 1e-12


def test_one_outlier_in_a_constant_patch(rt):
    """3 x 3 of value c with the centre o, radius 1, no history (K = 1).  The centre sees all nine:
    b - a^2 = 8 (o - c)^2 / 81, times 9 / 8: (o - c)^2 / 9.  A corner sees four, the outlier among
    them: 3 (o - c)^2 / 16 times 4 / 3: (o - c)^2 / 4.  An edge sees six: 5 (o - c)^2 / 36 times
    6 / 5: (o - c)^2 / 6."""
    g, normal, depth = _plane(rt, 3, 3)
    c, o = 0.25, 1.5
    y = np.full((3, 3), c)
    y[1, 1] = o
    cur = {"rgb": np.repeat(y[..., None], 3, -1).astype(np.float32), "count": 2.0, "normal": normal, "depth": depth}
    # depth_tol 0.5: across the 40 degrees of this 3 x 3 image a plane's depth differs by more than 5 %
    res = M.reproject_moments(M.PLAIN, g, None, g, cur, radius=1, depth_tol=0.5)
    want = (o - c) ** 2 / np.array([[4, 6, 4], [6, 9, 6], [4, 6, 4]], np.float64)
    assert np.abs(res["var"] - want).max() < 1e-6
    assert np.array_equal(res["rgb"], cur["rgb"].astype(np.float64)) and (res["count"] == 2).all()
    # a neighbour beyond the depth tolerance does not count: the centre moved back by a quarter
    far = depth.copy()
    far[1, 1] *= 1.25
    res = M.reproject_moments(M.PLAIN, g, None, g, dict(cur, depth=far), radius=1, depth_tol=0.1)
    assert res["var"][1, 1] == 0.0 and np.abs(res["var"][0, 0]).max() < 1e-12    # T = 1; three equal values


@pytest.mark.parametrize("mode", M.MODES, ids=M.NAMES.values())
def test_switched_off_it_is_the_modes_restatement(rt, mode):
    """radius = -1 and a min_frames no pixel reaches: rgb, var (the mode's v_blend), count,
    emission and coverage are the selected mode's restatement's bits, in fp64 and in fp32"""
    for w, h in SIZES:
        fx = M.fixture(rt, mode, w, h)
        prev = dict(fx["prev"], lum2=np.nan_to_num(fx["prev"]["lum2"]))    # a NaN lum2 is a tap rule of its own
        for opts in ({}, NONDEFAULT):
            for dt in (np.float64, np.float32):
                a = M.reproject_moments(mode, fx["gp"], prev, fx["gc"], fx["cur"], min_frames=UNREACHABLE, radius=-1,
                                        dt=dt, **opts)
                b = M.mode_restatement(mode, fx["gp"], prev, fx["gc"], fx["cur"], dt=dt, **opts)
                for k in M.keys(mode)[:-1]:
                    assert np.array_equal(a[k], b[k], equal_nan=True), (w, h, k, dt)
                assert np.array_equal(a["history"], b["history"]) and not a["took_t"].any() and not a["took_s"].any()


def test_the_temporal_estimate_is_unbiased(rt):
    """a 64 x 64 plane of luminance 1 with iid Gaussian noise of sigma 0.1, identical cameras, 8
    frames of equal counts, default options: the mean of out.var is sigma^2 / 8 within 5 %, which
    is 6 standard errors of the mean of 4096 sample variances with 7 degrees of freedom
    (sqrt(2 / 7) / 64 = 0.8 %)"""
    w = h = 64
    sigma = 0.1
    g, normal, depth = _plane(rt, w, h)
    rng = np.random.default_rng(20171)
    ys = [np.float32(1.0 + sigma * rng.standard_normal((h, w))) for _ in range(8)]
    res = _sequence(g, normal, depth, ys)
    assert res["took_t"].all() and np.abs(res["count"] - 8).max() < 1e-9
    mean, want = float(res["var"].mean()), sigma ** 2 / 8
    print(f"mean out.var {mean:.6e}, sigma^2 / 8 {want:.6e}, ratio {mean / want:.4f}")
    assert abs(mean / want - 1.0) <= 0.05


@pytest.mark.parametrize("mode", M.MODES, ids=M.NAMES.values())
@pytest.mark.parametrize("w,h", SIZES)
def test_fixtures_stay_under_the_fragile_cap(rt, mode, w, h):
    """the reference alone, with the new decisions in the fragile set, stays within the project's
    2 %; the integer counts keep K (2.5 or 4.5 away from the seam of the counts) off min_frames"""
    fx = M.fixture(rt, mode, w, h)
    for name, (opts, mo) in CASES.items():
        res = M.reproject_moments(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"], **opts, **mo)
        share = float(res["fragile"].mean())
        print(f"{M.NAMES[mode]} {w}x{h} {name}: fragile {share:.4f}, history {res['history'].mean():.3f}, "
              f"v_t {res['took_t'].mean():.3f}, v_s {res['took_s'].mean():.3f}")
        assert share <= M.FRAGILE_CAP
        ok = res["history"] & (res["coverage"] < 1) & ~res["fragile"]
        mf = mo.get("min_frames", 4.0)
        assert (np.abs(res["K"][ok] - mf) > 1e-3 * mf).all()
    if (w, h) == (24, 17):   # both estimates and the pass-through occur
        res = M.reproject_moments(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"])
        assert res["took_t"].sum() > 10 and res["took_s"].sum() > 10 and (~res["took_t"] & ~res["took_s"]).sum() > 0
        assert (res["history"] & res["took_s"]).sum() > 0     # a history shorter than min_frames
