"""The numpy restatement of rt_reproject_emit (tests/reproject_emit_ref.py) against values computed
by hand and against the parent's restatement, and the condition its fixtures must meet before the
GPU tests rely on them: at most 2 % fragile pixels at every size (reproject_ref.FRAGILE_CAP; a
condition on the fixtures, never a cap to raise)."""
import numpy as np
import pytest

from tests import reproject_emit_ref as E
from tests import reproject_ref as R
from tests.test_reproject_ref import NONDEFAULT, SIZES, _one_plane

KEYS = ("rgb", "var", "count")


def _split(frames, seed):
    """_one_plane's frames as surface radiance z under a random coverage of 0 .. 7/8 in eighths:
    (frames with rgb' = k z + e, emission and coverage; z, k per frame in fp64)"""
    rng = np.random.default_rng(seed)
    out, zs, ks = [], [], []
    for f in frames:
        cov = rng.integers(0, 8, f["depth"].shape) / 8.0
        e = (cov[..., None] * np.array(E.LIGHT)).astype(np.float32)
        rgb = ((1 - cov)[..., None] * f["rgb"].astype(np.float64) + e).astype(np.float32)
        out.append(dict(f, rgb=rgb, emission=e, coverage=cov.astype(np.float32)))
        ks.append(1.0 - cov)
        zs.append((rgb.astype(np.float64) - e) / ks[-1][..., None])  # by hand, from the fp32 planes
    return out, zs, ks


def test_identical_cameras_blend_z_and_relight(rt):
    """one plane, the same camera twice: the history of a pixel is the previous frame's pixel, so
    rgb = k_c (n_q z_q + n_c z_c) / (n_q + n_c) + e_c and var = k_c^2 (n_q^2 v_q / k_q^2 + n_c^2
    v_c / k_c^2) / (n_q + n_c)^2, computed here by hand"""
    cam, g, frames = _one_plane(rt)
    (prev, cur), (zp, zc), (kp, kc) = _split(frames, 11)
    res = E.reproject_emit(g, prev, g, cur)
    assert res["history"].all()
    nh, nc = prev["count"].astype(np.float64), cur["count"].astype(np.float64)
    n = nh + nc
    z = (nh[..., None] * zp + nc[..., None] * zc) / n[..., None]
    want = kc[..., None] * z + cur["emission"]
    want_v = kc ** 2 * (nh ** 2 * prev["var"] / kp ** 2 + nc ** 2 * cur["var"] / kc ** 2) / n ** 2
    assert np.abs(res["count"] - n).max() < 1e-9
    assert np.abs(res["rgb"] - want).max() < 1e-9 and np.abs(res["var"] - want_v).max() < 1e-9
    # one pixel with nothing vectorised: (x, y) = (3, 2)
    a, b = float(prev["count"][2, 3]), float(cur["count"][2, 3])
    kq, k = 1 - float(prev["coverage"][2, 3]), 1 - float(cur["coverage"][2, 3])
    zq = (prev["rgb"][2, 3].astype(np.float64) - prev["emission"][2, 3]) / kq
    zz = (cur["rgb"][2, 3].astype(np.float64) - cur["emission"][2, 3]) / k
    assert np.abs(res["rgb"][2, 3] - (k * (a * zq + b * zz) / (a + b) + cur["emission"][2, 3])).max() < 1e-9
    # the plain history of the same frames differs wherever the two coverages do: the split matters
    plain = R.reproject(g, prev, g, cur)
    assert np.abs(plain["rgb"] - res["rgb"]).max() > 0.1


def test_half_pixel_shift_beside_a_covered_pixel_uses_the_uncovered_tap(rt):
    """the previous camera moved by half a pixel along +x, so pixel x gathers the previous pixels
    x - 1 and x at weight 1/2 each.  With previous pixel x - 1 fully covered only pixel x is a
    tap: S = 1/2, z_h = z_q, v_h = v_q / k_q^2, n_h = n_q; and a fully covered current pixel
    takes no history and keeps its bits"""
    cam, g, frames = _one_plane(rt)
    (prev, cur), (zp, zc), (kp, kc) = _split(frames, 12)
    x, y = 4, 3
    prev["coverage"][y, x - 1], prev["emission"][y, x - 1], prev["rgb"][y, x - 1] = 1.0, E.LIGHT, E.LIGHT
    cur["coverage"][y + 1, x], cur["emission"][y + 1, x], cur["rgb"][y + 1, x] = 1.0, E.LIGHT, E.LIGHT
    step = np.linalg.norm(g["U"]) * 5.0 / 10.0
    gp = dict(g, C=g["C"] + np.array((0.5 * step, 0, 0)), P00=g["P00"] + np.array((0.5 * step, 0, 0)))
    res = E.reproject_emit(gp, prev, g, cur)
    nh, nc = float(prev["count"][y, x]), float(cur["count"][y, x])
    k = kc[y, x]
    want = k * (nh * zp[y, x] + nc * zc[y, x]) / (nh + nc) + cur["emission"][y, x]
    want_v = k ** 2 * (nh ** 2 * float(prev["var"][y, x]) / kp[y, x] ** 2
                       + nc ** 2 * float(cur["var"][y, x]) / k ** 2) / (nh + nc) ** 2
    assert res["history"][y, x] and abs(res["count"][y, x] - (nh + nc)) < 1e-6
    assert np.abs(res["rgb"][y, x] - want).max() < 1e-6 and abs(res["var"][y, x] - want_v) < 1e-8
    # the light's 15 stays out: the plain history puts half of it into this pixel's history
    plain = R.reproject(gp, prev, g, cur)
    assert plain["rgb"][y, x].max() > res["rgb"][y, x].max() + 1.0
    # a pixel two columns on gathers two uncovered taps: the mean of their z
    x2 = x + 2
    na, nb = float(prev["count"][y, x2 - 1]), float(prev["count"][y, x2])
    nh2, nc2 = 0.5 * (na + nb), float(cur["count"][y, x2])
    want2 = kc[y, x2] * (nh2 * 0.5 * (zp[y, x2 - 1] + zp[y, x2]) + nc2 * zc[y, x2]) / (nh2 + nc2) + cur["emission"][y, x2]
    assert np.abs(res["rgb"][y, x2] - want2).max() < 1e-6
    # the covered current pixel
    assert not res["history"][y + 1, x]
    assert np.array_equal(res["rgb"][y + 1, x], np.float64(E.LIGHT)) and res["count"][y + 1, x] == cur["count"][y + 1, x]


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_zero_emission_and_coverage_is_the_parent_exactly(rt, w, h, opts, dt):
    fx = R.fixture(rt, w, h)
    zero = {"emission": np.zeros((h, w, 3), np.float32), "coverage": np.zeros((h, w), np.float32)}
    a = R.reproject(fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=dt, **opts)
    b = E.reproject_emit(fx["gp"], dict(fx["prev"], **zero), fx["gc"], dict(fx["cur"], **zero), dt=dt, **opts)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype == dt and np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(a["history"], b["history"]) and np.array_equal(a["fragile"], b["fragile"])


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_fixtures_stay_under_the_fragile_cap(rt, w, h, opts):
    fx = E.fixture(rt, w, h)
    res = E.reproject_emit(fx["gp"], fx["prev"], fx["gc"], fx["cur"], **opts)
    share = float(res["fragile"].mean())
    print(f"{w}x{h} {'nondefault' if opts else 'default'}: fragile {share:.4f}, history {res['history'].mean():.3f}")
    assert share <= E.FRAGILE_CAP


def test_fixtures_exercise_the_split(rt):
    """24 x 17 and 131 x 5: the covered block and the NaN-emission pixel of cur pass through, the
    block's neighbours find history with some taps refused (S < 1 where the parent has S = 1),
    coverage holds eighths only, and fp32 decides the non-fragile pixels as fp64 does"""
    for w, h in ((24, 17), (131, 5)):
        fx = E.fixture(rt, w, h)
        prev, cur, block, rim = fx["prev"], fx["cur"], fx["block"], fx["rim"]
        assert block.sum() > 0 and rim.sum() >= 2 * block.sum() ** 0.5 and (cur["depth"][block | rim] > 5).all()
        for f in (prev, cur):
            assert np.array_equal(f["coverage"] * 8, np.round(f["coverage"] * 8)) and (f["coverage"][block] == 1).all()
            assert ((f["coverage"][rim] > 0) & (f["coverage"][rim] < 1)).all()
            assert (~np.isfinite(f["emission"]).all(-1)).sum() == 1
        a = E.reproject_emit(fx["gp"], prev, fx["gc"], cur)
        b = E.reproject_emit(fx["gp"], prev, fx["gc"], cur, dt=np.float32)
        ok = ~a["fragile"]
        assert np.array_equal(a["history"][ok], b["history"][ok])
        nan_c = ~np.isfinite(cur["emission"]).all(-1)
        for m in (block, nan_c):
            assert not a["history"][m].any()
            for k in KEYS:
                assert np.array_equal(a[k][m], cur[k][m].astype(np.float64), equal_nan=True)
        assert a["history"][rim].any()
        # taps on the block and on prev's NaN-emission pixel are refused: against the plain history
        # of the same planes some pixel that keeps history has gathered less count weight
        plain = R.reproject(fx["gp"], prev, fx["gc"], cur)
        assert (plain["history"] & a["history"] & (np.abs(plain["count"] - a["count"]) > 1e-3)).sum() > 0
