"""Accumulator-owned feature buffers (rt_accum_set_features / rt_accum_resolve_aov, k_aov_fold in
rt_aov.hip and k_feat_resolve in rt_accum.hip).

The reference is the feature pass itself, which tests/test_aov_gpu.py and
tests/test_aov_emit_gpu.py check against the fp64 oracle: ref(s) is
Scene.render_aov(cam, n_samples=ss, seed=s, emit=True), every sample of a pass of seed s.  With
S the fp32 sum of a pixel's ss samples, ref = fl(S inv), inv within 1 ulp of 1 / ss (the build's
fp32 reciprocal is not correctly rounded), so ref is within 2.5 ulps of S / ss; the accumulator
gives S / ss rounded once: at most 3 ulps apart, the ulp taken at the reference value.  Both
divide the light-sample count in fp64, so coverage is bit-equal.  Over several passes the fp64
sums of at most 1024 fp32 terms are exact or one rounding away after the cast, and the bars are
absolute, in ulps of the largest reference (normals cancel).

Every test but the structure test uses Cornell 40 x 30 at 4 samples per pixel: the smallest
size with both a pixel the light covers and a rim pixel (tests/test_aov_emit_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_aov_gpu import _shape

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 30, 4
FLOAT_PLANES = ("albedo", "normal", "depth", "emission", "surface_albedo")
PLANES = FLOAT_PLANES + ("coverage",)


def ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Ctx:
    """One Cornell scene for the module, and ref(s) computed once per seed and kept unchanged"""

    def __init__(self, rt):
        self.rt = rt
        t, cam, w, l = rt.demo_scene("cornell")
        self.cam = _shape(cam, W, H, SPP)
        self.ss = SPP
        self.sc = rt.Scene(t, w, l)
        self._ref = {}

    def ref(self, s):
        if s not in self._ref:
            r = self.sc.render_aov(self.cam, n_samples=self.ss, seed=s, emit=True)
            for k in PLANES:
                r[k].setflags(write=False)
            self._ref[s] = r
        return self._ref[s]

    def acc(self, features="emit", **kw):
        return self.sc.accumulator(self.cam, max_passes=8, features=features, **kw)

    def resolved(self, seeds, **kw):
        with self.acc(**kw) as a:
            for s in seeds:
                a.add(s)
            return a.resolve_aov()


@pytest.fixture(scope="module")
def ctx(rt, gpu):
    c = Ctx(rt)
    yield c
    c.sc.close()


def check_one_pass(got, ref, what):
    """test 1's bar: every float plane within 3 ulps of the reference, coverage bit-equal"""
    worst = 0.0
    for k in FLOAT_PLANES:
        d = np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64)) / ulp(ref[k])
        worst = max(worst, float(d.max()))
        print(f"{what} {k}: max {d.max():.2f} ulps, bit-equal {np.array_equal(bits(got[k]), bits(ref[k]))}")
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float32
        assert d.max() <= 3.0, (what, k, float(d.max()))
    assert np.array_equal(bits(got["coverage"]), bits(ref["coverage"])), what
    return worst


def check_mean(got, refs, weights, sel, what, ss, bar=3.0):
    """test 2's bar on the pixels `sel`: the light-sample count exact; every other plane within
    bar * ulp(max_s |ref(s)|) of the fp64 mean of the references that the pixel took"""
    n = float(sum(weights))
    cov = sum(w * r["coverage"].astype(np.float64) * ss for w, r in zip(weights, refs))
    assert np.array_equal(cov, np.rint(cov))  # light samples: integers
    # the count over the pixel's samples, divided in fp64 and rounded once (n ss = 16: exact,
    # coverage 16 is the integer itself)
    assert np.array_equal(bits(got["coverage"])[sel], bits((cov / (n * ss)).astype(np.float32))[sel]), what
    assert np.array_equal(np.rint(got["coverage"].astype(np.float64) * n * ss)[sel], cov[sel]), what
    for k in FLOAT_PLANES:
        mean = sum(w * r[k].astype(np.float64) for w, r in zip(weights, refs)) / n
        top = np.max([np.abs(r[k]) for w, r in zip(weights, refs) if w], axis=0)
        d = np.abs(got[k].astype(np.float64) - mean) / ulp(top)
        print(f"{what} {k}: max {d[sel].max():.3f} ulps of the largest reference")
        assert d[sel].max() <= bar, (what, k, float(d[sel].max()))


def test_one_pass_equals_the_feature_pass(ctx):
    ref = ctx.ref(3)
    assert ref["coverage"].max() == 1.0 and ((ref["coverage"] > 0) & (ref["coverage"] < 1)).any()
    with ctx.acc() as a:
        assert a.features == "emit"
        st = a.add(3)
        got = a.resolve_aov()
    assert sorted(got) == sorted(PLANES)
    assert st["samples"] == W * H * SPP  # the render's stats, not the feature rays'
    check_one_pass(got, ref, "spp 4")


def test_one_pass_at_nine_samples(ctx):
    """3 x 3 samples: 1 / 9 is not a power of two, so the reference's reciprocal rounds"""
    rt = ctx.rt
    _, cam, _, _ = rt.demo_scene("cornell")
    _shape(cam, W, H, 9)
    ref = ctx.sc.render_aov(cam, n_samples=9, seed=3, emit=True)
    with ctx.sc.accumulator(cam, max_passes=2, features="emit") as a:
        a.add(3)
        got = a.resolve_aov()
    check_one_pass(got, ref, "spp 9")


def test_several_passes(ctx):
    seeds = (3, 4, 5, 6)
    got = ctx.resolved(seeds)
    every = np.ones((H, W), bool)
    lights = sum(ctx.ref(s)["coverage"].astype(np.float64) * ctx.ss for s in seeds)
    assert np.array_equal(got["coverage"].astype(np.float64) * 4 * ctx.ss, lights)  # as integers
    assert lights.max() == 4 * ctx.ss
    check_mean(got, [ctx.ref(s) for s in seeds], [1] * 4, every, "4 passes", ctx.ss)


@pytest.fixture(scope="module")
def active(ctx):
    """Two whole passes (3, 4), then an active pass (7) over the left half plus one covered and
    one rim pixel, in an accumulator with features and in one without"""
    cov = ctx.ref(3)["coverage"]
    light = np.any([ctx.ref(s)["coverage"] > 0 for s in (3, 4, 7)], axis=0)
    mask = np.zeros((H, W), bool)
    mask[:, : W // 2] = True
    right = np.zeros((H, W), bool)
    right[:, W // 2:] = True
    covered, rim = cov == 1.0, (cov > 0) & (cov < 1)
    picks = []
    for sel in (covered, rim):  # one of each, from the right half when there is one
        cand = np.argwhere(sel & right) if (sel & right).any() else np.argwhere(sel)
        assert len(cand), "the fixture needs a covered and a rim pixel"
        picks.append(tuple(cand[0]))
        mask[picks[-1]] = True
    assert covered[mask].any() and rim[mask].any()
    assert (light & ~mask).any(), "the mask must leave a light pixel out"
    out = {"mask": mask, "picks": picks}
    for feat in ("emit", None):
        with ctx.acc(features=feat) as a:
            a.add(3)
            a.add(4)
            before = a.resolve_aov() if feat else None
            assert a.set_active(mask) == int(mask.sum())
            a.add_active(7)
            out[feat] = {"before": before, "after": a.resolve_aov() if feat else None,
                         "counts": a.counts(), "image": a.resolve(), "info": a.info()}
    return out


def test_active_passes(ctx, active):
    mask, r = active["mask"], active["emit"]
    assert np.array_equal(r["counts"], np.where(mask, 3, 2))
    refs = [ctx.ref(3), ctx.ref(4), ctx.ref(7)]
    check_mean(r["after"], refs, [1, 1, 1], mask, "active pixels", ctx.ss)
    for k in PLANES:
        assert np.array_equal(bits(r["after"][k])[~mask], bits(r["before"][k])[~mask]), k
    check_mean(r["after"], refs, [1, 1, 0], ~mask, "inactive pixels", ctx.ss)
    for y, x in active["picks"]:  # the covered and the rim pixel took the third pass
        assert r["counts"][y, x] == 3


def test_the_image_is_untouched(ctx, active):
    seeds = (3, 4, 5)
    res = {}
    for feat in ("emit", None):
        with ctx.acc(features=feat) as a:
            for s in seeds:
                a.add(s)
            res[feat] = (a.resolve(), a.info())
    for (on, i_on), (off, i_off) in ((res["emit"], res[None]),
                                     ((active["emit"]["image"], active["emit"]["info"]),
                                      (active[None]["image"], active[None]["info"]))):
        assert np.array_equal(bits(on[0]), bits(off[0])) and np.array_equal(bits(on[1]), bits(off[1]))
        assert i_on == i_off
    assert np.array_equal(active["emit"]["counts"], active[None]["counts"])


def test_order(ctx):
    a, b = ctx.resolved((3, 4, 5)), ctx.resolved((5, 3, 4))
    assert np.array_equal(bits(a["coverage"]), bits(b["coverage"]))
    for k in FLOAT_PLANES:
        top = np.max([np.abs(ctx.ref(s)[k]) for s in (3, 4, 5)], axis=0)
        d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)) / ulp(top)
        print(f"order {k}: max {d.max():.3f} ulps of the largest reference")
        assert d.max() <= 1.0, (k, float(d.max()))


def test_row_share(ctx):
    seeds = (3, 4)
    full = ctx.resolved(seeds)
    share = ctx.resolved(seeds, rank=1, nranks=3)
    assert share["depth"].shape == (10, W)
    assert share["coverage"].max() > 0
    for k in PLANES:
        assert np.array_equal(bits(share[k]), bits(full[k][1::3])), k


def _book1(rt):
    t, cam, wd, l = rt.demo_scene("book1")
    cam.DefocusAngle = 0.0
    cam.VerticalFOV = 100.0
    cam.PositionCamera((13, 2, 3), (0, 15, 0), (0, 1, 0))
    return t, _shape(cam, 32, 24, 4), wd, l


@pytest.mark.parametrize("scene,knob,value,width", [("cornell", "RT_TREE", "2", 2), ("cornell", "RT_TREE", "4", 4),
                                                    ("book1", "RT_QBVH", "1", 5), ("book1", "RT_QBVH", "0", 4)])
def test_structures(rt, gpu, tune, scene, knob, value, width):
    if scene == "cornell":
        t, cam, wd, l = rt.demo_scene("cornell")
        _shape(cam, W, H, SPP)
    else:
        t, cam, wd, l = _book1(rt)
    tune(knob, value)
    with rt.Scene(t, wd, l) as sc:
        ref = sc.render_aov(cam, n_samples=4, seed=3, emit=True)
        assert ref["stats"]["tree_width"] == width
        with sc.accumulator(cam, max_passes=2, features="emit") as a:
            a.add(3)
            got = a.resolve_aov()
    assert ref["coverage"].max() > 0
    check_one_pass(got, ref, f"{scene} {knob}={value}")


def test_refusals_and_lifecycle(ctx):
    rt = ctx.rt
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    buf = np.zeros((H, W, 3), np.float32)
    one = np.zeros((H, W), np.float32)
    ibuf = np.zeros((H, W), np.int32)
    guides = rt._lib.RtAov(buf.ctypes.data, None, None, None)
    emit = rt._lib.RtAovEmit(None, None, one.ctypes.data)
    with ctx.acc(features=None) as a:  # features off
        assert a.features is None
        assert L.rt_accum_resolve_aov(a._p, C.byref(guides), None) == E
        assert b"not enabled" in L.rt_last_error()
        with pytest.raises(ValueError):
            a.resolve_aov()
        with pytest.raises(ValueError):
            a.denoise_device()
    with ctx.acc(features="guides") as a:
        assert a.features == "guides"
        z = a.resolve_aov()  # before any pass: zeros
        assert sorted(z) == ["albedo", "depth", "normal"] and all(not v.any() for v in z.values())
        assert L.rt_accum_resolve_aov(a._p, C.byref(guides), C.byref(emit)) == E  # emit planes under "guides"
        assert b"emit" in L.rt_last_error()
        assert L.rt_accum_resolve_aov(a._p, C.byref(rt._lib.RtAov(None, None, None, ibuf.ctypes.data)), None) == E
        assert b"material" in L.rt_last_error()
        assert L.rt_accum_resolve_aov(a._p, C.byref(rt._lib.RtAov(None, None, None, None)), None) == E
        assert L.rt_accum_resolve_aov(a._p, None, None) == E
        assert L.rt_accum_set_features(a._p, 4) == E  # unknown bits
        a.add(3)
        for planes in (0, 1, 3):
            assert L.rt_accum_set_features(a._p, planes) == E  # after a pass
        assert a.features == "guides"
        got = a.resolve_aov()
        assert np.array_equal(bits(got["albedo"]), bits(ctx.ref(3)["albedo"]))  # 1 / 4 is exact
        a.reset()
        assert a.features == "guides" and a.passes == 0
        assert all(not v.any() for v in a.resolve_aov().values())
        a.add(4)
        assert np.array_equal(bits(a.resolve_aov()["depth"]), bits(ctx.ref(4)["depth"]))
        a.reset()
        assert L.rt_accum_set_features(a._p, 0) == 0 and a.features is None  # off again, planes freed
        assert L.rt_accum_set_features(a._p, 3) == 0 and a.features == "emit"
        a.add(3)
        assert np.array_equal(bits(a.resolve_aov()["coverage"]), bits(ctx.ref(3)["coverage"]))


def test_closing_the_scene_closes_the_accumulator(rt, gpu):
    t, cam, w, l = rt.demo_scene("cornell")
    _shape(cam, W, H, SPP)
    sc = rt.Scene(t, w, l)
    a = sc.accumulator(cam, max_passes=2, features="emit")
    a.add(3)
    assert a.resolve_aov()["coverage"].max() == 1.0
    sc.close()
    assert a._p is None
    with pytest.raises(ValueError):
        a.resolve_aov()
    a.close()


def test_denoiser_hook(ctx):
    rt = ctx.rt
    with ctx.acc() as a:
        for s in (3, 4, 5, 6):
            a.add(s)
        out = a.denoise_device()
        dev = out.device
        mean = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        var = torch.empty((H, W), dtype=torch.float32, device=dev)
        a.resolve_device(mean, var)
        aov = a.resolve_aov_device()
        assert aov is a.resolve_aov_device()  # owned and reused
        host = a.resolve_aov()
        for k in PLANES:
            assert np.array_equal(bits(aov[k].cpu().numpy()), bits(host[k])), k
        want = rt.denoise_var_device(mean, var, aov, split_emitters=True)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        plain = rt.denoise_var_device(mean, var, aov)
        assert not torch.equal(out, plain)  # the split did something: the light is in view
        # passing an aov behaves as before: no split unless asked for
        assert torch.equal(a.denoise_device(aov).view(torch.int32), plain.view(torch.int32))
    with ctx.acc(features=None) as a:
        a.add(3)
        a.add(4)
        with pytest.raises(ValueError):
            a.denoise_device()
