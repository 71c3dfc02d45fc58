"""tests/reproject_clip_ref.py, the numpy restatement of rt_reproject_clip, on the CPU: hand cases of
the box and the clamp, its identity with the moments restatement where clipping is off, and the
fragile share of the fixtures the GPU test uses (the moments fixtures with a stale block)."""
import numpy as np
import pytest

from tests import reproject_clip_ref as K
from tests import reproject_moments_ref as M
from tests.test_reproject_moments_ref import _plane
from tests.test_reproject_ref import NONDEFAULT, SIZES

# (rt_reproject_opts, rt_moments_opts, gamma) of the parity cases: the defaults (radius 3, the default
# gamma), radius 3, 8 and 1 with gamma 1, and everything non-default together.  NONDEFAULT's depth_tol
# goes with the radius of 1 only, as in tests/test_reproject_moments_ref.py
CASES = {"default": ({}, {}, 0.0), "radius3": ({}, dict(radius=3), 1.0), "radius8": ({}, dict(radius=8), 1.0),
         "radius1": ({}, dict(radius=1), 1.0),
         "nondefault": (NONDEFAULT, dict(min_frames=3.0, radius=1), 2.5)}


def _grey(y):
    return np.repeat(np.asarray(y, np.float64)[..., None], 3, -1).astype(np.float32)


def _frames(rt, w, h, y_cur, y_prev, count=1.0, depth=None):
    """identical cameras over the plane z = -5: (geometry, prev, cur) of grey frames"""
    g, normal, d = _plane(rt, w, h)
    d = d if depth is None else depth
    cur = {"rgb": _grey(np.broadcast_to(y_cur, (h, w))), "count": count, "normal": normal, "depth": d}
    prev = {"rgb": _grey(np.broadcast_to(y_prev, (h, w))), "count": count, "normal": normal, "depth": d,
            "lum2": np.zeros((h, w), np.float32)}
    return g, prev, cur


def test_a_constant_neighbourhood_returns_the_current_colour(rt):
    """s = 0: the box is the point x_p, whatever gamma.  A history of another colour is overruled
    entirely and the blend of x_p with x_p is x_p, exactly (counts of 1: n_h = sum beta / sum beta
    = 1, and (x + x) / 2 rounds nowhere)"""
    w, h = 8, 6
    y_prev = np.full((h, w), 0.2)
    y_prev[2:5, 3:6] = 1.0
    g, prev, cur = _frames(rt, w, h, 0.2, y_prev)
    x = np.float64(np.float32(0.2))
    for gamma in (0.0, 0.75, 3.0):
        res = K.reproject_clip(K.PLAIN, g, prev, g, cur, gamma=gamma)
        assert res["history"].all() and res["clampable"].all()
        assert np.array_equal(res["box_lo"], res["box_hi"]) and (res["box_lo"] == x).all()
        assert (res["rgb"] == x).all() and (res["count"] == 2).all()
        assert res["clamped"][2:5, 3:6].all()
    off = M.reproject_moments(M.PLAIN, g, prev, g, cur)
    assert np.abs(off["rgb"][3, 4] - 0.6).max() < 1e-6      # without the clamp: the blend of 1.0 and 0.2


def test_a_three_by_three_patch_by_hand(rt):
    """radius 1 on 3 x 3 grey values 0.1 .. 0.9, a history of 5.0 everywhere (above every box): the
    centre's window is all nine values, an edge's six, a corner's four; m and s are the window's
    mean and population standard deviation, and the history colour comes back as m + gamma s"""
    y = np.arange(1, 10, dtype=np.float64).reshape(3, 3) / 10
    g, prev, cur = _frames(rt, 3, 3, y, 5.0, count=2.0)
    y32 = np.float32(y).astype(np.float64)
    for gamma in (1.0, 1.5):
        # depth_tol 0.5: across the 40 degrees of this 3 x 3 image a plane's depth differs by more than 5 %
        res = K.reproject_clip(K.PLAIN, g, prev, g, cur, radius=1, depth_tol=0.5, gamma=gamma)
        assert res["history"].all() and res["clamped"].all()
        for (py, px), T in (((1, 1), 9), ((0, 1), 6), ((1, 0), 6), ((2, 1), 6), ((0, 0), 4), ((2, 2), 4), ((0, 2), 4)):
            win = y32[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2].ravel()
            assert res["T"][py, px] == T == win.size
            m, s = win.mean(), win.std()
            assert np.abs(res["box_hi"][py, px] - (m + gamma * s)).max() < 1e-12
            assert np.abs(res["box_lo"][py, px] - (m - gamma * s)).max() < 1e-12
            n = res["count"][py, px]                           # n_h + w_c, w_c = 2
            want = ((n - 2.0) * (m + gamma * s) + 2.0 * y32[py, px]) / n
            assert np.abs(res["rgb"][py, px] - want).max() < 1e-12
        # by hand, the centre: mean 0.5, variance (16 + 9 + 4 + 1) 2 / 9 / 100 = 0.6 / 9
        assert np.abs(res["box_hi"][1, 1] - (0.5 + gamma * np.sqrt(0.6 / 9))).max() < 1e-7
        # the corner (0, 0): 0.1, 0.2, 0.4, 0.5: mean 0.3, variance (4 + 1 + 1 + 4) / 4 / 100 = 0.025
        assert np.abs(res["box_hi"][0, 0] - (0.3 + gamma * np.sqrt(0.025))).max() < 1e-7
        # the edge (0, 1): 0.1 0.2 0.3 0.4 0.5 0.6: mean 0.35, variance 0.175 / 6
        assert np.abs(res["box_hi"][0, 1] - (0.35 + gamma * np.sqrt(0.175 / 6))).max() < 1e-7
    # a history below every box comes back as m - gamma s
    g, prev, cur = _frames(rt, 3, 3, y, 0.0, count=2.0)
    res = K.reproject_clip(K.PLAIN, g, prev, g, cur, radius=1, depth_tol=0.5, gamma=1.0)
    n = res["count"][1, 1]
    want = ((n - 2.0) * (0.5 - np.sqrt(0.6 / 9)) + 2.0 * y32[1, 1]) / n
    assert res["clamped"].all() and np.abs(res["rgb"][1, 1] - want).max() < 1e-7


def test_a_history_inside_the_box_is_untouched(rt):
    """the history 0.5 lies inside mean +- 3 sigma of values spread over 0.4 .. 0.6: no pixel is
    clamped, and every plane has the moments restatement's bits"""
    w, h = 6, 4
    rng = np.random.default_rng(11)
    g, prev, cur = _frames(rt, w, h, 0.4 + 0.2 * rng.random((h, w)), 0.5, count=2.0)
    for dt in (np.float64, np.float32):
        res = K.reproject_clip(K.PLAIN, g, prev, g, cur, depth_tol=0.5, gamma=3.0, dt=dt)
        off = M.reproject_moments(M.PLAIN, g, prev, g, cur, depth_tol=0.5, dt=dt)
        assert res["clampable"].all() and not res["clamped"].any()
        assert (res["box_lo"] < 0.5).all() and (res["box_hi"] > 0.5).all()
        for k in M.keys(M.PLAIN):
            assert np.array_equal(res[k], off[k]), (k, dt)


def test_a_window_of_one_pixel_is_not_clamped(rt):
    """T = 1 has no spread to clamp to: a 1 x 1 image, and a pixel gated off from all its
    neighbours (a quarter deeper than they, in both frames, so that it finds its history)"""
    g, prev, cur = _frames(rt, 1, 1, 0.2, 1.0)
    for radius in (0, 1, 8):
        res = K.reproject_clip(K.PLAIN, g, prev, g, cur, radius=radius)
        off = M.reproject_moments(M.PLAIN, g, prev, g, cur, radius=radius)
        assert res["history"].all() and res["T"][0, 0] == 1 and not res["clampable"].any()
        assert np.array_equal(res["rgb"], off["rgb"]) and np.abs(res["rgb"] - 0.6).max() < 1e-6
    _, _, depth = _plane(rt, 3, 3)
    far = depth.copy()
    far[1, 1] *= 1.25
    g, prev, cur = _frames(rt, 3, 3, 0.2, 1.0, depth=far)
    res = K.reproject_clip(K.PLAIN, g, prev, g, cur, radius=1, depth_tol=0.1)
    off = M.reproject_moments(M.PLAIN, g, prev, g, cur, radius=1, depth_tol=0.1)
    assert res["history"][1, 1] and res["T"][1, 1] == 1 and not res["clampable"][1, 1]
    assert np.array_equal(res["rgb"][1, 1], off["rgb"][1, 1]) and np.abs(res["rgb"][1, 1] - 0.6).max() < 1e-6
    assert res["clamped"][0, 0] and np.abs(res["rgb"][0, 0] - np.float32(0.2)).max() < 1e-12


def test_a_bright_history_clamped_down_leaves_a_larger_variance(rt):
    """q_h is not rectified: where the temporal estimate speaks and the clamp lowers the history's
    luminance, a clamped pixel's variance is at least the unclamped one's; count and lum2 are the
    moments restatement's"""
    w, h = 6, 4
    rng = np.random.default_rng(5)
    y_prev = 0.5 + 0.1 * rng.random((h, w))
    g, prev, cur = _frames(rt, w, h, 0.2 + 0.02 * rng.random((h, w)), y_prev, count=1.0)
    prev = dict(prev, count=np.full((h, w), 5.0, np.float32), lum2=(M.lum(_grey(y_prev).astype(np.float64)) ** 2
                                                                     * 1.05).astype(np.float32))
    res = K.reproject_clip(K.PLAIN, g, prev, g, cur, depth_tol=0.5)
    off = M.reproject_moments(M.PLAIN, g, prev, g, cur, depth_tol=0.5)
    assert res["clamped"].all() and res["took_t"].all()
    assert (res["var"] >= off["var"]).all() and np.array_equal(res["lum2"], off["lum2"])
    assert np.array_equal(res["count"], off["count"])


@pytest.mark.parametrize("mode", K.MODES, ids=K.NAMES.values())
def test_without_copts_it_is_the_moments_restatement(rt, mode):
    """gamma = None (copts = NULL): every plane and every set has the moments restatement's bits, in
    fp64 and in fp32, on the fixtures with the stale block"""
    for w, h in SIZES:
        fx = K.fixture(rt, mode, w, h)
        for opts, mo, _ in CASES.values():
            for dt in (np.float64, np.float32):
                a = K.reproject_clip(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"], gamma=None, dt=dt, **opts, **mo)
                b = M.reproject_moments(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=dt, **opts, **mo)
                for k in b:
                    assert np.array_equal(a[k], b[k], equal_nan=True), (w, h, k, dt)
                assert not a["clampable"].any() and not a["clamped"].any()


@pytest.mark.parametrize("mode", K.MODES, ids=K.NAMES.values())
@pytest.mark.parametrize("w,h", SIZES)
def test_fixtures_stay_under_the_fragile_cap(rt, mode, w, h):
    """the reference alone, with the new decisions in the fragile set, stays within the project's
    2 %; at 24 x 17 the stale block is clamped and pixels of every kind occur"""
    fx = K.fixture(rt, mode, w, h)
    for name, (opts, mo, gamma) in CASES.items():
        res = K.reproject_clip(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"], gamma=gamma, **opts, **mo)
        share = float(res["fragile"].mean())
        print(f"{K.NAMES[mode]} {w}x{h} {name}: fragile {share:.4f}, history {res['history'].mean():.3f}, "
              f"clampable {res['clampable'].mean():.3f}, clamped {res['clamped'].mean():.3f}")
        assert share <= K.FRAGILE_CAP
    if (w, h) == (24, 17):
        res = K.reproject_clip(mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"])
        ok = ~res["fragile"]
        stale = K.stale_block(w, h) & res["history"] & res["clampable"] & ok
        assert stale.sum() > 10 and res["clamped"][stale].mean() > 0.9
        assert (res["clampable"] & ~res["clamped"] & ok).sum() > 10       # a history inside its box
        assert (~res["history"] & ok).sum() > 10
