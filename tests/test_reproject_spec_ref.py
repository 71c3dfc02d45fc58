"""tests/reproject_spec_ref.py, the numpy restatement of rt_reproject_spec, on the CPU: its identity
with the clip restatement where spec is NULL, the fragile share of the fixtures the GPU test uses (the
clip fixtures with bounces planes), hand cases of the two deltas, and the planar-mirror claim of
DESIGN.md section 23 on an analytic, noise-free scene."""
import numpy as np
import pytest

from tests import reproject_clip_ref as K
from tests import reproject_ref as R
from tests import reproject_spec_ref as S
from tests.test_reproject_clip_ref import CASES, _frames
from tests.test_reproject_ref import SIZES

MODES = pytest.mark.parametrize("mode", S.MODES, ids=S.NAMES.values())


@MODES
def test_without_spec_it_is_the_clip_restatement(rt, mode):
    """bounces=False (spec = NULL): every plane and every set has the clip restatement's bits, in fp64
    and in fp32, with the clamp and without it (gamma None), on the clip restatement's fixtures"""
    for w, h in SIZES:
        fx = K.fixture(rt, mode, w, h)
        for opts, mo, gamma in CASES.values():
            for g in (gamma, None):
                for dt in (np.float64, np.float32):
                    args = (mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"])
                    a = S.reproject_spec(*args, gamma=g, bounces=False, dt=dt, **opts, **mo)
                    b = K.reproject_clip(*args, gamma=g, dt=dt, **opts, **mo)
                    for k in b:
                        assert np.array_equal(a[k], b[k], equal_nan=True), (w, h, k, dt)
                    assert a["whole"].all()


@MODES
def test_all_zero_bounces_are_the_clip_restatement(rt, mode):
    """frames whose two bounces planes are all zero: the gate passes everywhere"""
    w, h = 24, 17
    fx = K.fixture(rt, mode, w, h)
    z = np.zeros((h, w), np.float32)
    args = (mode, fx["gp"], dict(fx["prev"], bounces=z), fx["gc"], dict(fx["cur"], bounces=z))
    for dt in (np.float64, np.float32):
        a, b = S.reproject_spec(*args, dt=dt), K.reproject_clip(*args, dt=dt)
        for k in b:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, dt)


@MODES
@pytest.mark.parametrize("w,h", SIZES)
def test_fixtures_stay_under_the_fragile_cap(rt, mode, w, h):
    """the gate adds no fragile flag (it compares the caller's values exactly; the clip restatement's
    flags follow the sums it changes), and the fragile share stays under the project's cap.
    At 24 x 17 every kind of pixel occurs: gated taps, pixels without a whole b_c, pixels with history
    inside the block of 1.0"""
    fx = S.fixture(rt, mode, w, h)
    args = (mode, fx["gp"], fx["prev"], fx["gc"], fx["cur"])
    for name, (opts, mo, gamma) in CASES.items():
        for g in (gamma, None):
            res = S.reproject_spec(*args, gamma=g, **opts, **mo)
            off = S.reproject_spec(*args, gamma=g, bounces=False, **opts, **mo)
            share = float(res["fragile"].mean())
            print(f"{S.NAMES[mode]} {w}x{h} {name} gamma {g}: fragile {share:.4f} (without bounces "
                  f"{off['fragile'].mean():.4f}), history {res['history'].mean():.3f}, whole {res['whole'].mean():.3f}")
            assert share <= S.FRAGILE_CAP
    if (w, h) == (24, 17):
        res = S.reproject_spec(*args)
        off = S.reproject_spec(*args, bounces=False)
        bp, bc = fx["prev"]["bounces"], fx["cur"]["bounces"]
        assert (~res["whole"]).sum() > 10 and not res["history"][~res["whole"]].any()
        assert (off["history"] & ~res["whole"]).sum() > 5                 # ... that had one without the gate
        assert (res["history"] & (bc == 1)).sum() > 5                     # history inside the block of 1.0
        lost = off["history"] & ~res["history"] & (bc == 1)
        assert lost.sum() > 5                                             # prev 2.0 against cur 1.0
        assert np.isnan(bp).sum() == 1 and np.isnan(bc).sum() == 1
        assert not res["history"][np.isnan(bc)].any()


def _shifted(rt, w, h, frac):
    """_frames' plane z = -5 and camera, with a previous camera moved along -x so that pixel (x, y)
    reprojects to (x + frac, y): the taps of a pixel are columns x and x + 1 of its own row with the
    weights 1 - frac and frac"""
    g, prev, cur = _frames(rt, w, h, 0.0, 0.0)
    focal = -(g["P00"] - g["C"])[2]
    delta = frac * np.sqrt((g["U"] ** 2).sum()) * 5.0 / focal
    off = np.array([delta, 0.0, 0.0])
    return g, dict(g, C=g["C"] - off, P00=g["P00"] - off), prev, cur


def test_a_tap_of_another_chain_length_is_left_out_by_hand(rt):
    """3 x 2, every pixel reprojects a quarter pixel to the right; prev's bounces are 1 but for pixel
    (row 0, column 1), which has 2, cur's are all 1.  Row 0 by hand: column 0 keeps its own tap only
    (S = 0.75, c_h = prev[0, 0]); column 1 loses its own and keeps column 2's (S = 0.25, c_h =
    prev[0, 2]); column 2's right tap is outside the image (S = 0.75).  Row 1 is untouched: S = 1 but
    at column 2, and c_h = the bilinear mix.  No clamp (gamma None), so x_h is the blend's colour"""
    w, h = 3, 2
    gc, gp, prev, cur = _shifted(rt, w, h, 0.25)
    y = np.array([[0.1, 0.5, 0.9], [0.2, 0.4, 0.8]])
    prev = dict(prev, rgb=np.repeat(y[..., None], 3, -1).astype(np.float32))
    bp = np.ones((h, w), np.float32)
    bp[0, 1] = 2.0
    prev["bounces"], cur["bounces"] = bp, np.ones((h, w), np.float32)
    y32 = np.float32(y).astype(np.float64)
    res = S.reproject_spec(S.PLAIN, gp, prev, gc, cur, depth_tol=0.5, gamma=None)
    want_S = np.array([[0.75, 0.25, 0.75], [1.0, 1.0, 0.75]])
    want_c = np.array([[y32[0, 0], y32[0, 2], y32[0, 2]],
                       [0.75 * y32[1, 0] + 0.25 * y32[1, 1], 0.75 * y32[1, 1] + 0.25 * y32[1, 2], y32[1, 2]]])
    print("S", res["S"], "c_h", res["x_h"][..., 0])
    assert res["history"].all()
    assert np.abs(res["S"] - want_S).max() < 1e-5
    assert np.abs(res["x_h"] - want_c[..., None]).max() < 1e-5
    # ... and without the plane the tap is back
    off = S.reproject_spec(S.PLAIN, gp, prev, gc, cur, depth_tol=0.5, gamma=None, bounces=False)
    assert np.abs(off["S"][0] - [1.0, 1.0, 0.75]).max() < 1e-5
    assert np.abs(off["x_h"][0, 0, 0] - (0.75 * y32[0, 0] + 0.25 * y32[0, 1])) < 1e-5
    # a NaN tap fails the comparison like any other value
    prev["bounces"] = np.where(bp == 2, np.float32(np.nan), bp)
    nan = S.reproject_spec(S.PLAIN, gp, prev, gc, cur, depth_tol=0.5, gamma=None)
    for k in ("S", "x_h", "rgb", "var", "count", "lum2"):
        assert np.array_equal(nan[k], res[k]), k


@MODES
def test_a_fractional_b_c_takes_the_no_history_path(rt, mode):
    """a pixel with b_c = 0.5 (and a negative, an infinite and a NaN one) has the bits of the same call
    with prev = None, in every plane; its neighbours keep their history"""
    w, h = 24, 17
    fx = S.fixture(rt, mode, w, h)
    bc = np.zeros((h, w), np.float32)
    bc[5, 7], bc[6, 9], bc[8, 3], bc[9, 12] = 0.5, -1.0, np.inf, np.nan
    odd = bc != 0
    prev, cur = dict(fx["prev"], bounces=np.zeros((h, w), np.float32)), dict(fx["cur"], bounces=bc)
    for dt in (np.float64, np.float32):
        res = S.reproject_spec(mode, fx["gp"], prev, fx["gc"], cur, dt=dt)
        alone = S.reproject_spec(mode, None, None, fx["gc"], cur, dt=dt)
        assert not res["whole"][odd].any() and res["whole"][~odd].all()
        assert not res["history"][odd].any() and res["history"][~odd].sum() > 100
        for k in S.keys(mode):
            assert np.array_equal(res[k][odd], alone[k][odd], equal_nan=True), (k, dt)


def mirror_figures(reproject, rt):
    """the planar-mirror claim on the analytic scene, through `reproject(prev, cur, chain)` -> a dict of
    rgb and count: (the pixels whose (u, v) lies inside the previous image, the counts there through
    the chain planes, mean |out - cur| there through the chain planes, and through the first hit's)"""
    cp, cc = S.mirror_cameras(rt)
    gp, gc = R.geometry(cp), R.geometry(cc)
    w, h = S.MIRROR_W, S.MIRROR_H
    first_p, chain_p = S.mirror_frame(gp, w, h)
    first_c, chain_c = S.mirror_frame(gc, w, h)
    # (u, v) of the virtual point in the previous camera, in fp64 from the exact geometry
    ys, xs = np.mgrid[0:h, 0:w]
    d = gc["P00"] + xs[..., None] * gc["U"] + ys[..., None] * gc["V"] - gc["C"]
    d = d / np.sqrt((d * d).sum(-1))[..., None]
    r = gc["C"] + ((gc["C"][1] + 2.0) / -d[..., 1])[..., None] * d - gp["C"]
    Ap, Wp = gp["P00"] - gp["C"], np.cross(gp["U"], gp["V"])
    q = (Ap @ Wp / (r @ Wp))[..., None] * r - Ap
    u, v = q @ gp["U"] / (gp["U"] @ gp["U"]), q @ gp["V"] / (gp["V"] @ gp["V"])
    inside = (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    a = reproject(cp, chain_p, cc, chain_c, True)
    b = reproject(cp, first_p, cc, first_c, False)
    cur = chain_c["rgb"].astype(np.float64)
    e_chain = float(np.abs(a["rgb"] - cur)[inside].mean())
    e_first = float(np.abs(b["rgb"] - cur)[inside].mean())
    return inside, a["count"][inside], e_chain, e_first, b["count"][inside]


def assert_mirror_claim(who, inside, count, e_chain, e_first, count_first):
    print(f"{who}: planar mirror, {int(inside.sum())} of {inside.size} pixels reproject inside the previous image; "
          f"count through the chain planes {count.min():.6f} .. {count.max():.6f}; mean |out - cur| through the chain "
          f"planes {e_chain:.3e}, through the first hit's {e_first:.3e} (ratio {e_first / max(e_chain, 1e-30):.1f}); "
          f"first-hit count {count_first.min():.3f} .. {count_first.max():.3f}")
    assert inside.sum() > 50
    assert np.abs(count - 2.0).max() < 1e-4          # (a) every such pixel finds its whole history
    assert e_chain <= e_first / 10                   # (b)


def test_planar_mirror_claim(rt):
    """(a) and (b) of the issue, in the fp64 restatement.  The first-hit side goes through
    reproject_clip_ref, as the issue says: with its default gamma (the clamp bounds the stale history,
    the harder comparison) and, for the lookup alone, without the clamp (gamma None); the chain side
    through reproject_spec_ref with the same gamma.  Both are asserted"""
    for gamma in (0.0, None):
        def reproject(cp, prev, cc, cur, chain):
            gp, gc = R.geometry(cp), R.geometry(cc)
            if chain:
                return S.reproject_spec(S.PLAIN, gp, prev, gc, cur, gamma=gamma)
            return K.reproject_clip(K.PLAIN, gp, prev, gc, cur, gamma=gamma)
        assert_mirror_claim(f"fp64 restatement, gamma {gamma}", *mirror_figures(reproject, rt))
