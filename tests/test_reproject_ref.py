"""The numpy restatement of rt_reproject (tests/reproject_ref.py) against values computed by
hand, and the condition its fixtures must meet: at most 2 % fragile pixels (pixels with a
decision within a relative 1e-3 of its threshold, which value comparisons leave out).  The cap
is a condition on the fixtures, not a measurement: a size that exceeds it gets other camera
offsets (reproject_ref.OFFSETS), never a higher cap."""
import numpy as np
import pytest

from tests import reproject_ref as R

SIZES = [(1, 1), (3, 2), (24, 17), (131, 5)]
NONDEFAULT = dict(max_history=10.5, depth_tol=0.02, normal_tol=0.5, min_weight=0.3)


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_fixtures_stay_under_the_fragile_cap(rt, w, h, opts):
    fx = R.fixture(rt, w, h)
    res = R.reproject(fx["gp"], fx["prev"], fx["gc"], fx["cur"], **opts)
    share = float(res["fragile"].mean())
    print(f"{w}x{h} {'nondefault' if opts else 'default'}: fragile {share:.4f}, history {res['history'].mean():.3f}")
    assert share <= R.FRAGILE_CAP


def test_fixtures_exercise_every_rule(rt):
    """24 x 17: pixels with and without history, invalid current pixels, the cap, the count-0
    block, the misses and the step edge all occur; fp32 decides the non-fragile pixels alike"""
    fx = R.fixture(rt, 24, 17)
    prev, cur = fx["prev"], fx["cur"]
    a = R.reproject(fx["gp"], prev, fx["gc"], cur)
    b = R.reproject(fx["gp"], prev, fx["gc"], cur, dt=np.float32)
    ok = ~a["fragile"]
    assert np.array_equal(a["history"][ok], b["history"][ok])
    invalid = ~(np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"]))
    assert invalid.sum() >= 3 and not a["history"][invalid].any()
    assert (cur["depth"] == 0).sum() > 0 and not a["history"][cur["depth"] == 0].any()
    assert (prev["count"] == 0).sum() > 0 and (~np.isfinite(prev["rgb"]).all(-1)).sum() == 2
    assert 0.5 < a["history"].mean() < 1.0
    capped = a["history"] & (np.abs(a["count"] - 9 * cur["count"]) < 1e-9)  # n_h = 8 n_c exactly
    assert capped.sum() > 0
    assert len(set(np.unique(cur["depth"] > 5))) == 2  # both planes in view
    # a pixel of the far plane whose history the near plane hides in the previous view exists:
    # valid, hit, reprojected inside, and still without history
    far = (cur["depth"] > 5) & ~invalid & ~a["history"]
    assert far.sum() > 0


def _one_plane(rt, w=8, h=6):
    from tests.test_denoise_var_gpu import synthetic, variance
    _, cam = R.cameras(rt, w, h)
    g = R.geometry(cam)
    ys, xs = np.mgrid[0:h, 0:w]
    d = g["P00"] + xs[..., None] * g["U"] + ys[..., None] * g["V"] - g["C"]
    depth = (5.0 * np.sqrt((d * d).sum(-1)) / -d[..., 2]).astype(np.float32)  # the plane z = -5
    normal = np.broadcast_to(np.float32((0, 0, 1)), (h, w, 3)).copy()
    rng = np.random.default_rng(5)
    frames = [{"rgb": np.abs(synthetic(h, w, seed=s)[0]), "var": np.abs(variance(h, w, seed=s)),
               "count": rng.integers(1, 9, (h, w)).astype(np.float32), "normal": normal, "depth": depth}
              for s in (1, 2)]
    return cam, g, frames


def test_identical_cameras_reduce_to_the_blend(rt):
    """one plane, the same camera twice: u = x and v = y up to rounding, so the history of a
    pixel is the previous frame's pixel (a neighbour enters with a weight of 1e-12 at most) and
    the output is the blend formula, here computed by hand; counts 1 .. 8 never reach the cap
    8 n_c, and with max_history = 2 the weight is min(n_q, 2)"""
    cam, g, (prev, cur) = _one_plane(rt)
    for cap in (0.0, 2.0):
        res = R.reproject(g, prev, g, cur, max_history=cap)
        assert res["history"].all()
        nh = prev["count"].astype(np.float64) if cap == 0 else np.minimum(prev["count"], cap).astype(np.float64)
        nc = cur["count"].astype(np.float64)
        n = nh + nc
        rgb = (nh[..., None] * prev["rgb"] + nc[..., None] * cur["rgb"]) / n[..., None]
        var = (nh ** 2 * prev["var"] + nc ** 2 * cur["var"]) / n ** 2
        assert np.abs(res["count"] - n).max() < 1e-9
        assert np.abs(res["rgb"] - rgb).max() < 1e-9 and np.abs(res["var"] - var).max() < 1e-9
    # every pixel sits on an integer (u, v): the fragile flag's near-integer rule fires everywhere
    assert R.reproject(g, prev, g, cur)["fragile"].all()
    # one pixel by hand, nothing vectorised: pixel (x, y) = (3, 2)
    p, c = prev["rgb"][2, 3].astype(np.float64), cur["rgb"][2, 3].astype(np.float64)
    a, b = float(prev["count"][2, 3]), float(cur["count"][2, 3])
    assert np.abs(R.reproject(g, prev, g, cur)["rgb"][2, 3] - (a * p + b * c) / (a + b)).max() < 1e-9


def test_half_pixel_shift_is_the_bilinear_mean(rt):
    """the previous camera moved by half a pixel's footprint on the plane along +x: the history
    of pixel x is the mean of the previous pixels x - 1 and x, with variance (v_a + v_b) / 4"""
    cam, g, (prev, cur) = _one_plane(rt)
    # a pixel is |U| wide on the image plane at distance |P00 - C| . w = focus: on z = -5 it
    # covers |U| * 5 / 10 world units
    step = np.linalg.norm(g["U"]) * 5.0 / 10.0
    gp = dict(g, C=g["C"] + np.array((0.5 * step, 0, 0)), P00=g["P00"] + np.array((0.5 * step, 0, 0)))
    res = R.reproject(gp, prev, g, cur)
    x, y = 4, 3
    pa, pb = (prev["rgb"][y, x - 1].astype(np.float64), prev["rgb"][y, x].astype(np.float64))
    na, nb = float(prev["count"][y, x - 1]), float(prev["count"][y, x])
    nh, nc = 0.5 * (na + nb), float(cur["count"][y, x])
    want = (nh * 0.5 * (pa + pb) + nc * cur["rgb"][y, x]) / (nh + nc)
    vh = 0.25 * (float(prev["var"][y, x - 1]) + float(prev["var"][y, x]))
    want_v = (nh ** 2 * vh + nc ** 2 * float(cur["var"][y, x])) / (nh + nc) ** 2
    assert res["history"][y, x] and abs(res["count"][y, x] - (nh + nc)) < 1e-6
    assert np.abs(res["rgb"][y, x] - want).max() < 1e-6 and abs(res["var"][y, x] - want_v) < 1e-8
    # column 0 has one tap inside (x = 0, weight 1/2 >= min_weight): its history is that pixel
    assert res["history"][y, 0] and abs(res["count"][y, 0] - (prev["count"][y, 0] + cur["count"][y, 0])) < 1e-6


def test_camera_turned_away_returns_the_current_frame(rt):
    """the previous camera turned by 180 degrees: every point lies behind it (s < 0), no pixel
    has history, the output is the current frame"""
    fx = R.fixture(rt, 24, 17)
    gp =R.geometry(R.cameras(rt, 24, 17, yaw_deg=180.0, offset=(0.0, 0.0, 0.0))[0])
    res = R.reproject(gp, fx["prev"], fx["gc"], fx["cur"])
    assert not res["history"].any() and not res["fragile"].any()
    cur = fx["cur"]
    assert np.array_equal(res["rgb"], cur["rgb"].astype(np.float64), equal_nan=True)
    assert np.array_equal(res["var"], cur["var"].astype(np.float64), equal_nan=True)
    assert np.array_equal(res["count"], cur["count"].astype(np.float64))


def test_fp32_restatement_is_close(rt):
    """dt=np.float32 runs every operation in fp32 (the result arrays have that dtype) and agrees
    with fp64 to fp32's precision on the non-fragile pixels"""
    fx = R.fixture(rt, 24, 17)
    a = R.reproject(fx["gp"], fx["prev"], fx["gc"], fx["cur"])
    b = R.reproject(fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=np.float32)
    assert all(b[k].dtype == np.float32 and a[k].dtype == np.float64 for k in ("rgb", "var", "count"))
    m = ~a["fragile"] & np.isfinite(a["rgb"]).all(-1) & np.isfinite(a["var"])
    assert np.abs(a["rgb"][m] - b["rgb"][m]).max() < 1e-4 and np.abs(a["count"][m] - b["count"][m]).max() < 1e-2
