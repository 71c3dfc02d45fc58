"""Accumulator-owned chain sums (RT_ACCUM_FEAT_SPEC: rt_accum_set_features_spec,
rt_accum_resolve_aov_spec, k_aov_spec_fold in rt_aov.hip) against
Scene.render_aov(specular=True) for the same seeds.

Scenes: `quads` at 24 x 24 (the record loop; a fuzz-0 metal quad) and `book1` at 16 x 12 (a tree;
mirrors, fuzzy metals and glass).  Bars: at 4 samples per pixel 1 / 4 is exact and every plane is
bit-equal; at 9 the reference's reciprocal rounds and tests/test_accum_feat_gpu.py's bar holds for
normal and depth alike (check_one_pass's: 3 ulps per element, the ulp taken at the reference value:
both sides round the same fp32 sum once); bounces is an exact count and always bit-equal."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library's HIP runtime initialises (one runtime per process)

from tests.test_accum_feat_gpu import bits, ulp
from tests.test_aov_gpu import _shape

pytestmark = pytest.mark.gpu
PLANES = ("normal", "depth", "bounces")
SCENES = {"quads": (24, 24), "book1": (16, 12)}


class Ctx:
    def __init__(self, rt, name):
        self.rt, self.name = rt, name
        t, cam, w, l = rt.demo_scene(name)
        self.cam = _shape(cam, *SCENES[name], 4)
        self.sc = rt.Scene(t, w, l)
        self._ref = {}

    def ref(self, s, **kw):
        key = (s, tuple(sorted(kw.items())))
        if key not in self._ref:
            r = self.sc.render_aov(self.cam, n_samples=4, seed=s, specular=True, **kw)
            for k in PLANES:
                r[k].setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def acc(self, features="emit+spec", **kw):
        return self.sc.accumulator(self.cam, max_passes=8, features=features, **kw)


@pytest.fixture(scope="module", params=list(SCENES))
def ctx(request, rt, gpu):
    c = Ctx(rt, request.param)
    yield c
    c.sc.close()


def mean_of(refs, n):
    """float32(sum float64(plane_pass) * 4 / (4 n)): every pass's fp32 sum is plane * 4 exactly"""
    return {k: (sum(r[k].astype(np.float64) * 4 for r in refs) / (4 * n)).astype(np.float32) for k in PLANES}


def test_one_pass_at_four_samples_is_bit_equal(ctx):
    ref = ctx.ref(3)
    assert ref["bounces"].max() >= 1.0, "the scene has a specular surface in view"
    with ctx.acc() as a:
        assert a.features == "emit+spec"
        a.add(3)
        got, dev = a.resolve_aov_spec(), a.resolve_aov_spec_device()
    assert sorted(got) == sorted(PLANES)
    for k in PLANES:
        assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape
        assert np.array_equal(bits(got[k]), bits(ref[k])), (ctx.name, k)
        assert np.array_equal(bits(dev[k].cpu().numpy()), bits(ref[k])), (ctx.name, k, "device entry")
    with ctx.acc("guides+spec") as a:
        a.add(3)
        g = a.resolve_aov_spec()
    assert all(np.array_equal(bits(g[k]), bits(ref[k])) for k in PLANES)


def test_one_pass_at_nine_samples(ctx):
    _, cam, _, _ = ctx.rt.demo_scene(ctx.name)
    _shape(cam, *SCENES[ctx.name], 9)
    ref = ctx.sc.render_aov(cam, n_samples=9, seed=3, specular=True)
    with ctx.sc.accumulator(cam, max_passes=2, features="emit+spec") as a:
        a.add(3)
        got = a.resolve_aov_spec()
    assert np.array_equal(bits(got["bounces"]), bits(ref["bounces"]))
    d = np.abs(got["depth"].astype(np.float64) - ref["depth"]) / ulp(ref["depth"])
    n = np.abs(got["normal"].astype(np.float64) - ref["normal"]) / ulp(ref["normal"])
    print(f"{ctx.name} spp 9: depth max {d.max():.2f} ulps, normal max {n.max():.2f} ulps, each at its reference value")
    assert d.max() <= 3.0 and n.max() <= 3.0


def test_three_passes(ctx):
    seeds = (3, 4, 5)
    with ctx.acc() as a:
        for s in seeds:
            a.add(s)
        got = a.resolve_aov_spec()
    want = mean_of([ctx.ref(s) for s in seeds], 3)
    for k in PLANES:
        assert np.array_equal(bits(got[k]), bits(want[k])), (ctx.name, k)
    same = np.all([ctx.ref(s)["bounces"] == ctx.ref(3)["bounces"] for s in seeds], 0) & (ctx.ref(3)["bounces"] % 1 == 0)
    assert np.array_equal(got["bounces"][same], ctx.ref(3)["bounces"][same])   # exactly (float)k over passes


def test_active_passes(ctx):
    h, w = ctx.cam.image_size()[1], ctx.cam.image_size()[0]
    ys, xs = np.mgrid[0:h, 0:w]
    mask = ((xs + 2 * ys) % 5 < 2) | ((ys >= h // 3) & (ys < h // 2))
    with ctx.acc() as a:
        a.add(3)
        assert a.set_active(mask) == int(mask.sum())
        a.add_active(4)
        a.set_active(mask)
        a.add_active(5)
        got, counts = a.resolve_aov_spec(), a.counts()
    assert np.array_equal(counts, np.where(mask, 3, 1))
    three, one = mean_of([ctx.ref(s) for s in (3, 4, 5)], 3), mean_of([ctx.ref(3)], 1)
    for k in PLANES:
        m = mask[..., None] if k == "normal" else mask
        assert np.array_equal(bits(got[k]), bits(np.where(m, three[k], one[k]))), (ctx.name, k)


def test_the_limits_reach_the_kernel(ctx):
    ref = ctx.ref(3, max_bounces=1, max_fuzz=0.3)
    with ctx.acc(spec_bounces=1, spec_fuzz=0.3) as a:
        a.add(3)
        got = a.resolve_aov_spec()
    for k in PLANES:
        assert np.array_equal(bits(got[k]), bits(ref[k])), (ctx.name, k)
    assert got["bounces"].max() == 1.0
    if ctx.name == "book1":   # fuzzy metals and glass: the limits change the planes
        assert not np.array_equal(bits(ref["depth"]), bits(ctx.ref(3)["depth"]))


def test_the_first_hit_planes_and_the_image_are_untouched(ctx):
    with ctx.acc("emit+spec") as a, ctx.acc("emit") as b:
        for x in (a, b):
            x.add(3)
            x.add(4)
        fa, fb = a.resolve_aov(), b.resolve_aov()
        ia, ib = a.resolve(), b.resolve()
    assert sorted(fa) == sorted(fb)
    for k in fb:
        assert np.array_equal(bits(fa[k]), bits(fb[k])), (ctx.name, k)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(ia, ib))


def test_reset_and_refusals(ctx):
    rt = ctx.rt
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    with ctx.acc() as a:
        a.add(3)
        a.add(4)
        a.reset()
        a.add(5)
        got = a.resolve_aov_spec()
        for k in PLANES:
            assert np.array_equal(bits(got[k]), bits(ctx.ref(5)[k])), (k, "reset clears the sums")
        # refused calls: the accumulator stays usable
        so = rt._lib.RtAovSpecOpts(0, 0.0)
        assert L.rt_accum_set_features_spec(a._h(), 11, C.byref(so)) == E and b"holds 1 passes" in L.rt_last_error()
        buf = np.zeros(a.shape + (3,), np.float32)
        sp = rt._lib.RtAovSpec(buf.ctypes.data)
        for out in (rt.RtAov(buf.ctypes.data, None, None, None), rt.RtAov(None, None, None, buf.ctypes.data)):
            assert L.rt_accum_resolve_aov_spec(a._h(), C.byref(out), C.byref(sp)) == E
        none = rt.RtAov(None, None, None, None)
        assert L.rt_accum_resolve_aov_spec(a._h(), C.byref(none), None) == E and b"no buffer" in L.rt_last_error()
        again = a.resolve_aov_spec()
        assert all(np.array_equal(bits(again[k]), bits(got[k])) for k in PLANES)
        a.reset()
        for planes, word in ((8, b"needs one"), (12, b"MEDIA"), (13, b"MEDIA"), (16, b"unknown"), (32 | 9, b"unknown")):
            assert L.rt_accum_set_features_spec(a._h(), planes, None) == E and word in L.rt_last_error(), planes
        for bad in (rt._lib.RtAovSpecOpts(-1, 0.0), rt._lib.RtAovSpecOpts(65, 0.0), rt._lib.RtAovSpecOpts(0, -1.0),
                    rt._lib.RtAovSpecOpts(0, float("nan"))):
            assert L.rt_accum_set_features_spec(a._h(), 11, C.byref(bad)) == E
        assert a.features == "emit+spec"
        # rt_accum_set_features is what it was: the bit is unknown to it, and nothing changes
        assert L.rt_accum_set_features(a._h(), 9) == E and b"rt_accum_set_features_spec" in L.rt_last_error()
        assert a.features == "emit+spec"
        assert L.rt_accum_set_features_spec(a._h(), 9, None) == 0 and a.features == "guides+spec"   # the defaults
        a.add(3)
        got = a.resolve_aov_spec()
        assert all(np.array_equal(bits(got[k]), bits(ctx.ref(3)[k])) for k in PLANES)
    with ctx.acc("emit") as b:
        b.add(3)
        with pytest.raises(ValueError, match="chain planes"):
            b.resolve_aov_spec()
        out = rt.RtAov(None, buf.ctypes.data, None, None)
        assert L.rt_accum_resolve_aov_spec(b._h(), C.byref(out), None) == E and b"not enabled" in L.rt_last_error()
