"""rt_reproject_device (rt_temporal.hip) against the numpy restatement of the definition pinned in
include/rt_abi.h (tests/reproject_ref.py), on the fixtures that restatement builds.

Accuracy bars, the form of the filter tests': over the non-fragile pixels the GPU's max abs error
against the restatement in fp64 must be <= 8 x the error of the same restatement run in numpy
fp32, plus 1e-6 for rgb, 1e-6 x the largest finite input variance for var and 1e-5 for count (the
margins cover the kernel's non-correctly-rounded division and square root).  Every check prints
its ratios."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import reproject_ref as R
from tests.test_reproject_ref import NONDEFAULT, SIZES

pytestmark = pytest.mark.gpu
KEYS = ("rgb", "var", "count")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_gpu(rt, cam_p, prev, cam_c, cur, inplace=False, **opts):
    dev = torch.device("cuda", 0)
    p, c = ({k: torch.from_numpy(np.array(v, np.float32)).to(dev) if np.ndim(v) else v  # copies: read-only inputs
             for k, v in f.items() if v is not None} for f in (prev, cur))
    out = {k: c[k] for k in KEYS} if inplace else None
    res = rt.reproject_device(cam_p, p, cam_c, c, out=out, **opts)
    if inplace:
        assert all(r.data_ptr() == c[k].data_ptr() for r, k in zip(res, KEYS))
    return {k: r.cpu().numpy() for k, r in zip(KEYS, res)}


_ref = {}


def restated(rt, w, h, opts):
    """(fp64, fp32) restatements of a fixture, computed once"""
    key = (w, h, tuple(sorted(opts.items())))
    if key not in _ref:
        fx = R.fixture(rt, w, h)
        _ref[key] = tuple(R.reproject(fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=dt, **opts)
                          for dt in (np.float64, np.float32))
    return _ref[key]


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_parity(rt, gpu, w, h, opts):
    fx = R.fixture(rt, w, h)
    prev, cur = fx["prev"], fx["cur"]
    r64, r32 = restated(rt, w, h, opts)
    got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], cur, **opts)
    assert r64["fragile"].mean() <= R.FRAGILE_CAP
    m = ~r64["fragile"] & np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"])
    vin = np.concatenate([f["var"][np.isfinite(f["var"])] for f in (prev, cur)])
    margin = {"rgb": 1e-6, "var": 1e-6 * float(vin.max()), "count": 1e-5}
    line = [f"reproject {w}x{h} {'nondefault' if opts else 'default'} ({int(m.sum())} of {w * h} pixels, "
            f"history {r64['history'].mean():.2f}):"]
    fails = []
    for k in KEYS:
        e32 = float(np.abs(r32[k][m] - r64[k][m]).max()) if m.any() else 0.0
        eg = float(np.abs(got[k][m] - r64[k][m]).max()) if m.any() else 0.0
        bar = 8 * e32 + margin[k]
        line.append(f"{k} gpu {eg:.3e} fp32-numpy {e32:.3e} bar {bar:.3e} ratio {eg / max(e32, 1e-30):.2f}")
        if not eg <= bar:
            fails.append((k, eg, e32, bar))
    print(" | ".join(line))
    assert np.isfinite(got["rgb"][m]).all() and np.isfinite(got["var"][m]).all() and (got["count"][m] > 0).all()
    assert not fails, fails


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
def test_history_set_is_exact(rt, gpu, opts):
    """on the non-fragile pixels (decisions away from their thresholds) the set of pixels that
    found history, count_out > count_cur, is the restatement's"""
    for w, h in SIZES:
        fx = R.fixture(rt, w, h)
        r64, _ = restated(rt, w, h, opts)
        got = run_gpu(rt, fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"], **opts)
        ok = ~r64["fragile"]
        with np.errstate(invalid="ignore"):
            found = got["count"] > fx["cur"]["count"]
        assert np.array_equal(found[ok], r64["history"][ok]), (w, h)
        assert 0 < r64["history"][ok].sum() and (w * h < 100 or r64["history"][ok].sum() < ok.sum())


def test_pass_through_bits(rt, gpu):
    """invalid current pixels, misses and every pixel without history keep the current frame's
    bits in all three planes; so does the whole frame when the previous camera looks the other
    way, and when the history has no weight anywhere"""
    fx = R.fixture(rt, 24, 17)
    prev, cur = fx["prev"], fx["cur"]
    r64, _ = restated(rt, 24, 17, {})
    got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], cur)
    invalid = ~(np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"]))
    miss = cur["depth"] == 0
    assert invalid.sum() == 3 and miss.sum() > 0
    keep = (invalid | miss | ~r64["history"]) & ~r64["fragile"]
    for k in KEYS:
        assert np.array_equal(bits(got[k])[keep], bits(cur[k])[keep]), k
    away = R.cameras(rt, 24, 17, yaw_deg=180.0, offset=(0.0, 0.0, 0.0))[0]
    for cam_p, p in ((away, prev), (fx["cams"][0], dict(prev, count=0.0))):
        got = run_gpu(rt, cam_p, p, fx["cams"][1], cur)
        for k in KEYS:
            assert np.array_equal(bits(got[k]), bits(cur[k])), k


def test_scalar_counts_and_missing_variance(rt, gpu):
    """count = one number (count_scalar) and frames without a variance plane follow the
    restatement too: the accumulator's frames have no count plane"""
    fx = R.fixture(rt, 24, 17)
    prev = {k: v for k, v in fx["prev"].items() if k != "var"}
    cur = {k: v for k, v in fx["cur"].items() if k != "var"}
    prev["count"], cur["count"] = 6.0, 2.0
    r64, r32 = (R.reproject(fx["gp"], prev, fx["gc"], cur, dt=dt) for dt in (np.float64, np.float32))
    got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], cur)
    m = ~r64["fragile"] & np.isfinite(cur["rgb"]).all(-1)
    assert r64["history"][m].sum() > 100 and (r64["var"] == 0).all() and (got["var"] == 0).all()
    for k, margin in (("rgb", 1e-6), ("count", 1e-5)):
        e32, eg = np.abs(r32[k][m] - r64[k][m]).max(), np.abs(got[k][m] - r64[k][m]).max()
        print(f"scalar counts: {k} gpu {eg:.3e} fp32-numpy {e32:.3e}")
        assert eg <= 8 * e32 + margin
    assert np.abs(got["count"][m & r64["history"]] - 8.0).max() < 1e-5


def test_in_place_and_repeatable(rt, gpu):
    """out = cur's buffers gives the bits of separate buffers; two calls give identical bits"""
    for w, h in ((24, 17), (131, 5)):
        fx = R.fixture(rt, w, h)
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a, b, c = run_gpu(rt, *args), run_gpu(rt, *args), run_gpu(rt, *args, inplace=True)
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])), (w, h, k)


def test_host_entry_matches_device(rt, gpu):
    for w, h in ((24, 17), (3, 2)):
        fx = R.fixture(rt, w, h)
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a = run_gpu(rt, *args, **NONDEFAULT)
        b = dict(zip(KEYS, rt.reproject(*args, **NONDEFAULT)))
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k)
    # without var and count planes, one number for the counts
    prev = {k: v for k, v in fx["prev"].items() if k in ("rgb", "normal", "depth")}
    cur = {k: v for k, v in fx["cur"].items() if k in ("rgb", "normal", "depth")}
    a = run_gpu(rt, fx["cams"][0], dict(prev, count=3.0), fx["cams"][1], dict(cur, count=1.0))
    b = dict(zip(KEYS, rt.reproject(fx["cams"][0], dict(prev, count=3.0), fx["cams"][1], dict(cur, count=1.0))))
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
