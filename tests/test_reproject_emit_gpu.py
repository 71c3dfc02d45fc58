"""rt_reproject_emit_device (rt_temporal.hip's k_reproject<true>) against the numpy restatement of
the definition pinned in include/rt_abi.h (tests/reproject_emit_ref.py), on the fixtures that
restatement builds.

Accuracy bars, the parent test's form: over the non-fragile pixels the GPU's max abs error against
the restatement in fp64 must be <= 8 x the error of the same restatement run in numpy fp32, plus
the parent's margins: 1e-6 for rgb, here scaled by the largest finite |rgb| of the fixture (the
planes now hold an emission of 15), 1e-6 x the largest finite input variance for var and 1e-5 for
count.  Every check prints its ratios."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import reproject_emit_ref as E
from tests import reproject_ref as R
from tests.test_reproject_ref import NONDEFAULT, SIZES

pytestmark = pytest.mark.gpu
KEYS = ("rgb", "var", "count")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_gpu(rt, cam_p, prev, cam_c, cur, inplace=False, emit=True, **opts):
    dev = torch.device("cuda", 0)
    p, c = ({k: torch.from_numpy(np.array(v, np.float32)).to(dev) if np.ndim(v) else v  # copies: read-only inputs
             for k, v in f.items() if v is not None} for f in (prev, cur))
    out = {k: c[k] for k in KEYS} if inplace else None
    res = (rt.reproject_emit_device if emit else rt.reproject_device)(cam_p, p, cam_c, c, out=out, **opts)
    if inplace:
        assert all(r.data_ptr() == c[k].data_ptr() for r, k in zip(res, KEYS))
    return {k: r.cpu().numpy() for k, r in zip(KEYS, res)}


_ref = {}


def restated(rt, w, h, opts):
    """(fp64, fp32) restatements of a fixture, computed once"""
    key = (w, h, tuple(sorted(opts.items())))
    if key not in _ref:
        fx = E.fixture(rt, w, h)
        _ref[key] = tuple(E.reproject_emit(fx["gp"], fx["prev"], fx["gc"], fx["cur"], dt=dt, **opts)
                          for dt in (np.float64, np.float32))
    return _ref[key]


def margins(prev, cur):
    fin = [np.abs(f[k][np.isfinite(f[k])]) for f in (prev, cur) for k in ("rgb", "var")]
    return {"rgb": 1e-6 * float(max(fin[0].max(), fin[2].max())), "var": 1e-6 * float(max(fin[1].max(), fin[3].max())),
            "count": 1e-5}


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
@pytest.mark.parametrize("w,h", SIZES)
def test_parity(rt, gpu, w, h, opts):
    fx = E.fixture(rt, w, h)
    prev, cur = fx["prev"], fx["cur"]
    r64, r32 = restated(rt, w, h, opts)
    got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], cur, **opts)
    assert r64["fragile"].mean() <= E.FRAGILE_CAP
    m = ~r64["fragile"] & np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"]) & np.isfinite(cur["emission"]).all(-1)
    margin = margins(prev, cur)
    line = [f"reproject_emit {w}x{h} {'nondefault' if opts else 'default'} ({int(m.sum())} of {w * h} pixels, "
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
    """on the non-fragile pixels the set of pixels that found history, count_out > count_cur, is the
    restatement's: no pixel of the covered block, none with NaN emission"""
    for w, h in SIZES:
        fx = E.fixture(rt, w, h)
        r64, _ = restated(rt, w, h, opts)
        got = run_gpu(rt, fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"], **opts)
        ok = ~r64["fragile"]
        with np.errstate(invalid="ignore"):
            found = got["count"] > fx["cur"]["count"]
        assert np.array_equal(found[ok], r64["history"][ok]), (w, h)
        assert not found[fx["block"]].any() and not found[~np.isfinite(fx["cur"]["emission"]).all(-1)].any()
        assert 0 < r64["history"][ok].sum() and (w * h < 100 or r64["history"][ok].sum() < ok.sum())


def test_pass_through_bits(rt, gpu):
    """invalid current pixels, misses, the covered block, the pixel with NaN emission and every
    pixel without history keep the current frame's bits in all three planes; so does the whole
    frame when every previous pixel is fully covered"""
    for w, h in ((24, 17), (131, 5)):
        fx = E.fixture(rt, w, h)
        prev, cur = fx["prev"], fx["cur"]
        r64, _ = restated(rt, w, h, {})
        got = run_gpu(rt, fx["cams"][0], prev, fx["cams"][1], cur)
        invalid = ~(np.isfinite(cur["rgb"]).all(-1) & np.isfinite(cur["var"]))
        nan_e = ~np.isfinite(cur["emission"]).all(-1)
        miss = cur["depth"] == 0
        keep = (invalid | miss | ~r64["history"]) & ~r64["fragile"]
        assert nan_e.sum() == 1 and keep[nan_e].all() and keep[fx["block"]].all() and miss.sum() > 0
        for k in KEYS:
            assert np.array_equal(bits(got[k])[keep], bits(cur[k])[keep]), (w, h, k)
    covered = dict(prev, coverage=np.ones((h, w), np.float32))
    got = run_gpu(rt, fx["cams"][0], covered, fx["cams"][1], cur)
    for k in KEYS:
        assert np.array_equal(bits(got[k]), bits(cur[k])), k


@pytest.mark.parametrize("opts", [{}, NONDEFAULT], ids=["default", "nondefault"])
def test_zero_emission_and_coverage_give_rt_reproject_bits(rt, gpu, opts):
    """the parent's fixtures with emission = 0 and coverage = 0: (c - 0) / 1 and 1 z + 0 are exact"""
    for w, h in SIZES:
        fx = R.fixture(rt, w, h)
        zero = {"emission": np.zeros((h, w, 3), np.float32), "coverage": np.zeros((h, w), np.float32)}
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a = run_gpu(rt, *args, emit=False, **opts)
        b = run_gpu(rt, fx["cams"][0], dict(fx["prev"], **zero), fx["cams"][1], dict(fx["cur"], **zero), **opts)
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k)


def test_in_place_and_repeatable(rt, gpu):
    """out = cur's buffers gives the bits of separate buffers; two calls give identical bits"""
    for w, h in ((24, 17), (131, 5)):
        fx = E.fixture(rt, w, h)
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a, b, c = run_gpu(rt, *args), run_gpu(rt, *args), run_gpu(rt, *args, inplace=True)
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])), (w, h, k)


def test_host_entry_matches_device(rt, gpu):
    for w, h in ((24, 17), (3, 2)):
        fx = E.fixture(rt, w, h)
        args = (fx["cams"][0], fx["prev"], fx["cams"][1], fx["cur"])
        a = run_gpu(rt, *args, **NONDEFAULT)
        b = dict(zip(KEYS, rt.reproject_emit(*args, **NONDEFAULT)))
        for k in KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])), (w, h, k)
    # without var and count planes, one number for the counts
    keys = ("rgb", "normal", "depth", "emission", "coverage")
    prev, cur = ({k: v for k, v in fx[f].items() if k in keys} for f in ("prev", "cur"))
    a = run_gpu(rt, fx["cams"][0], dict(prev, count=3.0), fx["cams"][1], dict(cur, count=1.0))
    b = dict(zip(KEYS, rt.reproject_emit(fx["cams"][0], dict(prev, count=3.0), fx["cams"][1], dict(cur, count=1.0))))
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_a_light_in_the_plane_stays_out_of_its_surroundings(rt, gpu):
    """the point of the split, built so that it is deterministic: one plane z = -5 of surface
    radiance 0.5, a block of fully covered pixels with rgb = emission = 15 in it, equal counts, the
    previous camera half a pixel to the right, so pixel x gathers the previous pixels x - 1 and x.
    rt_reproject cannot tell the block from the plane (same depth, same normal): the pixels right
    of it come out at (7.75 + 0.5) / 2 > 1.  rt_reproject_emit refuses the covered taps and every
    uncovered pixel stays 0.5 within the parity bar."""
    w, h = 16, 12
    _, cam = R.cameras(rt, w, h)
    g = R.geometry(cam)
    step = float(np.linalg.norm(g["U"])) * 5.0 / 10.0   # a pixel's footprint on the plane (focus distance 10)
    cam_p, cam_c = R.cameras(rt, w, h, offset=(0.5 * step, 0.0, 0.0), yaw_deg=0.0)
    gp, gc = R.geometry(cam_p), R.geometry(cam_c)
    ys, xs = np.mgrid[0:h, 0:w]
    d = g["P00"] + xs[..., None] * g["U"] + ys[..., None] * g["V"] - g["C"]
    depth = (5.0 * np.sqrt((d * d).sum(-1)) / -d[..., 2]).astype(np.float32)
    block = (xs >= 6) & (xs < 9) & (ys >= 4) & (ys < 7)
    cov = block.astype(np.float32)
    emission = (cov[..., None] * np.float32(15.0)) * np.ones(3, np.float32)
    frame = {"rgb": np.where(block[..., None], np.float32(15.0), np.float32(0.5)) * np.ones(3, np.float32),
             "var": np.full((h, w), 0.01, np.float32), "count": 4.0,
             "normal": np.broadcast_to(np.float32((0, 0, 1)), (h, w, 3)).copy(), "depth": depth,
             "emission": emission, "coverage": cov}
    plain = run_gpu(rt, cam_p, frame, cam_c, frame, emit=False)
    split = run_gpu(rt, cam_p, frame, cam_c, frame)
    right = (xs == 9) & (ys >= 4) & (ys < 7)   # their x - 1 tap is the block's last column
    print(f"beside the block: plain {plain['rgb'][right].min():.4f} .. {plain['rgb'][right].max():.4f}, "
          f"split {split['rgb'][right].min():.7f} .. {split['rgb'][right].max():.7f}")
    assert (plain["rgb"][right] > 1.0).all()
    r64, r32 = (E.reproject_emit(gp, frame, gc, frame, dt=dt) for dt in (np.float64, np.float32))
    assert np.abs(r64["rgb"][~block] - 0.5).max() < 1e-12 and r64["history"][right].all()
    e32 = float(np.abs(r32["rgb"][~block] - r64["rgb"][~block]).max())
    err = float(np.abs(split["rgb"][~block] - 0.5).max())
    print(f"uncovered pixels: |rgb - 0.5| gpu {err:.3e} fp32-numpy {e32:.3e} bar {8 * e32 + 15e-6:.3e}")
    assert err <= 8 * e32 + 1e-6 * 15.0
    assert np.array_equal(bits(split["rgb"])[block], bits(frame["rgb"])[block])
    assert (split["count"][right] > 4.0).all() and (split["count"][block] == 4.0).all()
