"""The numpy restatement of rt_reproject_light (tests/reproject_light_ref.py) against values computed
by hand and against the parent's restatement, and the condition its fixtures must meet before the
GPU tests rely on them: at most 2 % fragile pixels at every size (reproject_ref.FRAGILE_CAP; a
condition on the fixtures, never a cap to raise)."""
import numpy as np
import pytest

from tests import reproject_emit_ref as E
from tests import reproject_light_ref as L
from tests import reproject_ref as R
from tests.test_reproject_ref import NONDEFAULT, SIZES, _one_plane


def _plane(rt, cov_prev, cov_cur, z=0.5, light=15.0, count=4.0, var=0.01):
    """_one_plane's geometry with a surface radiance z under a light of `light`: per frame
    rgb = (1 - coverage) z + coverage light, emission = coverage light (coverage [h, w] in eighths,
    so every plane is exact in fp32)"""
    cam, g, (f, _) = _one_plane(rt)
    frames = []
    for cov in (cov_prev, cov_cur):
        cov = np.asarray(cov, np.float64) + np.zeros(f["depth"].shape)
        e = cov[..., None] * light * np.ones(3)
        frames.append({"rgb": ((1 - cov)[..., None] * z + e).astype(np.float32), "var": np.full(cov.shape, var, np.float32),
                       "count": np.full(cov.shape, count, np.float32), "normal": f["normal"], "depth": f["depth"],
                       "emission": e.astype(np.float32), "coverage": cov.astype(np.float32)})
    return g, frames[0], frames[1]


def test_a_rim_pixel_blends_coverage_and_emission(rt):
    """identical cameras and equal counts, coverage 3/8 before and 5/8 now on a plane of z = 0.5
    with a light of 15: kappa_out = 1/2, E_out = 7.5 and rgb = 0.5 x 0.5 + 7.5 = 7.75 exactly, where
    rt_reproject_emit re-lights with the current frame's 5/8: 0.375 x 0.5 + 9.375 = 9.5625"""
    g, prev, cur = _plane(rt, 3 / 8, 5 / 8)
    res = L.reproject_light(g, prev, g, cur)
    assert res["history"].all() and res["light_history"].all() and res["blend"].all()
    assert np.abs(res["coverage"] - 0.5).max() < 1e-12 and np.abs(res["emission"] - 7.5).max() < 1e-12
    assert np.abs(res["rgb"] - 7.75).max() < 1e-12 and np.abs(res["count"] - 8.0).max() < 1e-12
    # v_z = 0.01 / k^2 per frame, blended with equal weights, times (1 - 1/2)^2
    want_v = 0.25 * (16 * np.float64(np.float32(0.01)) / 0.625 ** 2 + 16 * np.float64(np.float32(0.01)) / 0.375 ** 2) / 64
    assert np.abs(res["var"] - want_v).max() < 1e-12
    emit = E.reproject_emit(g, prev, g, cur)
    assert np.abs(emit["rgb"] - 9.5625).max() < 1e-12
    # unequal counts: n_q = 12 against n_c = 4 -> kappa_out = (12 x 3/8 + 4 x 5/8) / 16 = 7/16
    res = L.reproject_light(g, dict(prev, count=np.full_like(prev["count"], 12.0)), g, cur)
    assert np.abs(res["coverage"] - 7 / 16).max() < 1e-12 and np.abs(res["emission"] - 15 * 7 / 16).max() < 1e-12
    assert np.abs(res["rgb"] - (9 / 16 * 0.5 + 15 * 7 / 16)).max() < 1e-12 and np.abs(res["count"] - 16.0).max() < 1e-12


def test_a_covered_pixel_with_surface_history_takes_z_h(rt):
    """coverage 1/4 before, 1 now at one pixel (x, y): no surface sample now (w_c = 0), so z_blend
    is the history's z_h = 0.5 and v_blend its v_h; kappa_out = (4 x 1/4 + 4 x 1) / 8 = 5/8"""
    cov_c = np.zeros((6, 8))
    x, y = 3, 2
    cov_c[y, x] = 1.0
    g, prev, cur = _plane(rt, 0.25, cov_c)
    res = L.reproject_light(g, prev, g, cur)
    assert res["blend"][y, x] and res["history"][y, x]
    assert abs(res["coverage"][y, x] - 0.625) < 1e-12 and np.abs(res["emission"][y, x] - 15 * 0.625).max() < 1e-12
    assert np.abs(res["rgb"][y, x] - (0.375 * 0.5 + 15 * 0.625)).max() < 1e-12
    assert abs(res["count"][y, x] - 8.0) < 1e-12
    assert abs(res["var"][y, x] - 0.375 ** 2 * np.float64(np.float32(0.01)) / 0.75 ** 2) < 1e-12
    # rt_reproject_emit passes such a pixel through
    emit = E.reproject_emit(g, prev, g, cur)
    assert not emit["history"][y, x] and np.array_equal(emit["rgb"][y, x], cur["rgb"][y, x].astype(np.float64))


def test_a_covered_pixel_without_surface_history_keeps_its_bits(rt):
    """the inside of a light: covered before and now.  The previous pixel is a light tap (m_h > 0)
    and no surface tap (n_h = 0), and n_h + w_c = 0: all five planes pass through.  Its uncovered
    neighbour under a half-pixel shift gathers the covered pixel as a light tap only"""
    cov = np.zeros((6, 8))
    x, y = 3, 2
    cov[y, x] = 1.0
    g, prev, cur = _plane(rt, cov, cov)
    cur = dict(cur, emission=cur["emission"].copy(), count=cur["count"] + 1)
    cur["emission"][y, x] = (14.0, 13.0, 12.0)   # not what a blend with prev's 15 would give
    res = L.reproject_light(g, prev, g, cur)
    assert res["light_history"][y, x] and not res["history"][y, x] and not res["blend"][y, x]
    for k in L.KEYS:
        assert np.array_equal(res[k][y, x], np.float64(cur[k][y, x])), k
    assert res["blend"].sum() == cov.size - 1
    # half a pixel to the right: pixel x + 1 gathers previous x (covered) and x + 1 at 1/2 each
    step = np.linalg.norm(g["U"]) * 5.0 / 10.0
    gp = dict(g, C=g["C"] + np.array((0.5 * step, 0, 0)), P00=g["P00"] + np.array((0.5 * step, 0, 0)))
    res = L.reproject_light(gp, prev, g, cur)
    # surface: the one uncovered tap, n_h = 4; light: both taps, m_h = 4, kappa_h = 1/2, E_h = 7.5
    kappa = (4 * 0.5 + 5 * 0.0) / 9
    assert abs(res["coverage"][y, x + 1] - kappa) < 1e-6 and np.abs(res["emission"][y, x + 1] - 4 * 7.5 / 9).max() < 1e-5
    assert np.abs(res["rgb"][y, x + 1] - ((1 - kappa) * 0.5 + 4 * 7.5 / 9)).max() < 1e-5
    assert abs(res["count"][y, x + 1] - 9.0) < 1e-6


def test_a_poisoned_previous_pixel_is_no_tap_of_either_kind(rt):
    """the case settled in the restatement: a previous pixel of NaN colour is neither a surface
    nor a light tap, whatever its emission and coverage"""
    g, prev, cur = _plane(rt, 3 / 8, 5 / 8)
    prev = dict(prev, rgb=prev["rgb"].copy())
    prev["rgb"][2, 3, 1] = np.nan
    res = L.reproject_light(g, prev, g, cur)
    assert not res["history"][2, 3] and not res["light_history"][2, 3] and not res["blend"][2, 3]
    for k in L.KEYS:
        assert np.array_equal(res[k][2, 3], np.float64(cur[k][2, 3])), k


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_zero_emission_and_coverage_is_the_parent_exactly(rt, w, h, opts, dt):
    fx = R.fixture(rt, w, h)
    zero = {"emission": np.zeros((h, w, 3), np.float32), "coverage": np.zeros((h, w), np.float32)}
    a = R.reproject(fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=dt, **opts)
    b = L.reproject_light(fx["gp"], dict(fx["prev"], **zero), fx["gc"], dict(fx["cur"], **zero), dt=dt, **opts)
    for k in ("rgb", "var", "count"):
        assert a[k].dtype == b[k].dtype == dt and np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(a["history"], b["history"]) and np.array_equal(a["fragile"], b["fragile"])
    assert np.array_equal(b["history"], b["light_history"]) and np.array_equal(b["history"], b["blend"])
    assert not b["emission"].any() and not b["coverage"].any()


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_fixtures_stay_under_the_fragile_cap(rt, w, h, opts):
    fx = L.fixture(rt, w, h)
    res = L.reproject_light(fx["gp"], fx["prev"], fx["gc"], fx["cur"], **opts)
    share = float(res["fragile"].mean())
    print(f"{w}x{h} {'nondefault' if opts else 'default'}: fragile {share:.4f}, surface history "
          f"{res['history'].mean():.3f}, light history {res['light_history'].mean():.3f}")
    assert share <= L.FRAGILE_CAP


def test_fixtures_exercise_the_light_history(rt):
    """24 x 17, and 131 x 5 at min_weight = 0.3 (its block is one row high, so a tap on the plane
    is always in reach): some pixel finds light history without surface history, some covered pixel
    takes surface history, at 24 x 17 some covered pixel passes through with light history in
    reach, the NaN-emission pixel of cur passes through, and fp32 decides the non-fragile pixels as
    fp64 does"""
    for (w, h), opts in (((24, 17), {}), ((131, 5), NONDEFAULT)):
        fx = L.fixture(rt, w, h)
        prev, cur, block = fx["prev"], fx["cur"], fx["block"]
        a = L.reproject_light(fx["gp"], prev, fx["gc"], cur, **opts)
        b = L.reproject_light(fx["gp"], prev, fx["gc"], cur, dt=np.float32, **opts)
        ok = ~a["fragile"]
        for k in ("history", "light_history", "blend"):
            assert np.array_equal(a[k][ok], b[k][ok]), k
        assert not (a["history"] & ~a["light_history"]).any()      # a surface tap is a light tap
        assert (a["light_history"] & ~a["history"]).any()
        assert (a["blend"] & block).any() and (h < 17 or (~a["blend"] & block & a["light_history"]).any())
        nan_c = ~np.isfinite(cur["emission"]).all(-1)
        assert nan_c.sum() == 1 and not a["blend"][nan_c].any()
        for k in L.KEYS:
            assert np.array_equal(a[k][~a["blend"]], cur[k][~a["blend"]].astype(np.float64), equal_nan=True), k
        # against rt_reproject_emit the rim's coverage moved and the plain pixels' did not
        m = a["blend"] & ok
        assert (np.abs(a["coverage"][m] - cur["coverage"][m]) > 1e-3).any()
        assert ((a["coverage"][m] >= 0) & (a["coverage"][m] <= 1)).all()
