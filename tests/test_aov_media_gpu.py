"""The media-aware feature pass (rt_render_aov_media, rt_aov.hip k_aov<TREE, EMIT, true>,
DESIGN.md §18) against the CPU oracle, and its identities with the passes it extends.

Checker.  pyoracle.trace(pixel, sample)[0] is the first world.Hit call of the sample in fp64:
its material kind is RT_MAT_ISOTROPIC (4) exactly when a constant medium won (isotropic
materials occur only as phase functions) and its t is the event's.  A surface event is evaluated
by tests/test_aov_gpu.py's numpy Flat; MediaFlat below adds the medium event: the medium is the
one whose boundary (a sphere, or the quads of a box, flattened like the world) holds o + t d,
albedo = the phase material's texture there at u = v = 0, normal = 0, depth = t |d|.  The
GPU's event of sample j comes from the prefix calls n_samples = 1 .. n as in test_aov_gpu.py:
M_j from the exact scatter counts, the primitive or the medium from the point at the sample's
depth.

Bars, as test_aov_gpu.py's.  Outside fork pixels: per sample, scatter's M_j equals the oracle's
and material equals the oracle's kind; per pixel, scatter is exactly count / n, and the GPU's max
error in depth / normal / albedo against the fp64 trace is <= 4 x the max error of the oracle's
own precision=32 trace through the same evaluation on the same pixels, with a floor of one fp32
ulp of the plane's scale.  A fork pixel has a sample whose GPU event lies on another primitive
or medium, or on the other side of scatter / surface, than the fp64 oracle's: at most 1 % of a
scene's pixels.

The fp32 twin alone against fp64 (CPU, 24 x 24, n = 4, seed 3: 576 pixels each): smoke_box 0
fork pixels (399 scatter samples), dup_medium 0 (1352), fog 0 (1166), water 0 (no scatter sample:
the medium fills a glass sphere that is in the world too, so the surface always wins -- the case
this scene is here for).  Those are within the 1 % cap, which is asserted for the twin there.
cornell_smoke: 51 fork pixels at seed 3 (55 at seed 5; 22 of 256 at 16 x 16), every one a scatter
the twin loses (146 of them at seed 5, none the other way): constantMedium.Hit looks for the
boundary's exit in (t1 + 1e-4, inf), and at the box's coordinates (555) one fp32 ulp of t is
6e-5, so the twin finds the entry face again and sees an empty medium.  No seed or size avoids
that, so, as test_aov_gpu.py does for Cornell's rotated box, the twin's error is measured where
the twin agrees with fp64, the GPU (whose boundary roots are fp64) is held to the resulting bar on
ALL its non-fork pixels, and the twin's cap is not asserted for that scene."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import scenes
from tests.cli import CLI
from tests.test_aov_gpu import Flat, _shape, expected

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISOTROPIC = 4
SURF = ("albedo", "normal", "depth", "material")
EMIT = ("emission", "surface_albedo", "coverage")
MEDIA_SCENES = ("smoke_box", "dup_medium", "fog", "water", "cornell_smoke")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def build(rt, name, w=24, h=24, spp=4):
    t, cam, wd, l = rt.demo_scene(name) if name in ("cornell_smoke", "cornell", "book2") else getattr(scenes, name)(rt)
    return t, _shape(cam, w, h, spp), wd, l


# ---------------------------------------------------------------- numpy checker ---
class MediaFlat(Flat):
    """Flat with the constant media: (phase material, boundary spheres, boundary quads) each"""

    def __init__(self, tree, world):
        self.med = []
        super().__init__(tree, world)

    def _walk(self, i, c, s, T):
        n = self.nodes[i]
        if int(n["kind"]) != 7:
            return super()._walk(i, c, s, T)
        self.media += 1
        keep = self.sph, self.quad, self.tri
        self.sph, self.quad, self.tri = [], [], []
        super()._walk(int(n["a"]), c, s, T)  # the boundary, flattened as the world is
        assert not self.tri and (self.sph or self.quad)
        self.med.append((int(n["mat"]), self.sph, self.quad))
        self.sph, self.quad, self.tri = keep

    def medium_at(self, p, time, tol=1e-6):
        """the medium whose boundary holds p (a convex one: a sphere, or a box's quads)"""
        for mi, (_, sph, quad) in enumerate(self.med):
            ok = True
            for c1, c2, r, _m in sph:
                ok &= np.linalg.norm(p - (c1 + time * (c2 - c1))) <= abs(r) * (1 + tol)
            if quad:
                cen = np.mean([Q + 0.5 * (u + v) for Q, u, v, _m in quad], axis=0)
                for Q, u, v, _m in quad:  # the side of every face its centre is on
                    nrm = np.cross(u, v)
                    nrm /= np.linalg.norm(nrm)
                    ext = np.linalg.norm(cen - Q)
                    ok &= np.dot(p - Q, nrm) * np.sign(np.dot(cen - Q, nrm)) >= -tol * ext
            if ok:
                return mi
        return -1

    def evaluate(self, rec, bg):
        if int(rec[11]) != ISOTROPIC:
            return super().evaluate(rec, bg)
        o, time, d = rec[0:3].astype(float), float(rec[3]), rec[4:7].astype(float)
        t = float(rec[8])
        p = o + t * d
        mi = self.medium_at(p, time)
        assert mi >= 0, "the oracle's scatter point is in no medium"
        M = self.mats[self.med[mi][0]]
        assert int(M["kind"]) == ISOTROPIC
        alb, solid = self.tex_value(int(M["tex"]), 0.0, 0.0, p)
        return -10 - mi, ISOTROPIC, np.zeros(3), alb, t * np.linalg.norm(d), solid

    def event_at(self, o, d, time, depth, scattered):
        """the GPU's event from its depth and its M_j: a medium's id, or the primitive's"""
        if not scattered:
            return self.prim_at(o, d, time, depth)
        mi = self.medium_at(o + (depth / np.linalg.norm(d)) * d, time, tol=1e-3)
        return -10 - mi if mi >= 0 else -2


def count_of(scatter, k):
    """the exact scatter count of a k-sample call's plane (count / k rounded once to fp32)"""
    c = np.rint(scatter.astype(np.float64) * k).astype(int)
    assert np.array_equal(scatter, (c / k).astype(np.float32)), "scatter is not count / n"
    return c


@pytest.fixture(scope="module")
def smoke(rt, gpu):
    """cornell_smoke 24 x 24: the media, the transparent and the split planes of seed 3, n = 4"""
    t, cam, wd, l = build(rt, "cornell_smoke")
    with rt.Scene(t, wd, l) as sc:
        return {"media": sc.render_aov(cam, n_samples=4, seed=3, emit=True, media=True),
                "plain": sc.render_aov(cam, n_samples=4, seed=3),
                "emit": sc.render_aov(cam, n_samples=4, seed=3, emit=True)}


@pytest.mark.parametrize("name", MEDIA_SCENES)
def test_first_events_match_oracle(rt, oracle, gpu, name):
    n, seed = 4, 3
    t, cam, wd, l = build(rt, name)
    flat = MediaFlat(t, wd)
    assert flat.media > 0
    W = H = 24
    rows = list(range(H))
    with rt.Scene(t, wd, l) as sc:
        got = [sc.render_aov(cam, n_samples=k, seed=seed, media=True) for k in range(1, n + 1)]
        again = sc.render_aov(cam, n_samples=n, seed=seed, media=True)
    g = got[-1]
    for k in SURF + ("scatter",):  # two calls: the same bits
        assert np.array_equal(bits(g[k]), bits(again[k])), k
    assert g["stats"]["samples"] == g["stats"]["segments"] == W * H * n  # feature rays, not media tests
    counts = [count_of(got[k]["scatter"], k + 1) for k in range(n)]
    e64 = expected(oracle, flat, t, wd, l, cam, rows, n, seed, 64)
    e32 = expected(oracle, flat, t, wd, l, cam, rows, n, seed, 32)
    fork = np.zeros((H, W), bool)
    fork32 = np.zeros((H, W), bool)
    x64 = {k: np.zeros(g[k].shape) for k in ("albedo", "normal", "depth")}
    x32 = {k: np.zeros(g[k].shape) for k in ("albedo", "normal", "depth")}
    solid = np.ones((H, W), bool)
    mat0 = np.zeros((H, W), int)
    m64 = np.zeros((n, H, W), bool)   # the oracle's M_j
    mg = np.zeros((n, H, W), bool)    # the GPU's
    for r in rows:
        for x in range(W):
            for j in range(n):
                a, b = e64[(r, x, j)], e32[(r, x, j)]
                cj = int(counts[j][r, x]) - (int(counts[j - 1][r, x]) if j else 0)
                assert cj in (0, 1)
                mg[j, r, x], m64[j, r, x] = cj == 1, a[1] == ISOTROPIC
                dj = (j + 1) * float(got[j]["depth"][r, x]) - (j * float(got[j - 1]["depth"][r, x]) if j else 0.0)
                rec = a[6]
                eps = 1e-5 * (j + 1) * max(1.0, float(got[j]["depth"][r, x]))
                gp = -1 if abs(dj) <= eps else (-3 if dj < 0.0 else flat.event_at(
                    rec[0:3].astype(float), rec[4:7].astype(float), float(rec[3]), dj, cj == 1))
                fork[r, x] |= gp != a[0]
                fork32[r, x] |= b[0] != a[0]
                solid[r, x] &= a[5] and b[5]
                for k, idx in (("normal", 2), ("albedo", 3), ("depth", 4)):
                    x64[k][r, x] += np.asarray(a[idx]) / n
                    x32[k][r, x] += np.asarray(b[idx]) / n
                if j == 0:
                    mat0[r, x] = a[1]
    npx = W * H
    print(f"{name}: fork pixels gpu {fork.sum()} fp32 twin {fork32.sum()} of {npx}; "
          f"scatter samples {m64.sum()} of {n * npx}, scatter pixels {m64.any(0).sum()}")
    if name != "cornell_smoke":  # (see the module docstring)
        assert fork32.mean() <= 0.01, "the fp32 oracle twin alone exceeds the fork cap"
    assert fork.mean() <= 0.01, (fork.sum(), npx)
    assert m64.any() == (name != "water"), "water: the glass surface always wins; elsewhere media events"
    ok = ~fork
    for j in range(n):  # per sample
        assert np.array_equal(mg[j][ok], m64[j][ok]), j
    assert np.array_equal(g["material"][ok], mat0[ok])
    # per pixel: exactly count / n
    assert np.array_equal(g["scatter"][ok], (m64.sum(0) / n).astype(np.float32)[ok])
    for k in ("depth", "normal", "albedo"):
        m = ok & solid if k == "albedo" else ok
        mt = m & ~fork32
        scale = max(1.0, float(np.abs(x64[k][m]).max())) if m.any() else 1.0
        floor = scale * 2.0 ** -23
        eg = float(np.abs(g[k][m] - x64[k][m]).max()) if m.any() else 0.0
        eo = float(np.abs(x32[k][mt] - x64[k][mt]).max()) if mt.any() else 0.0
        print(f"{name} {k}: gpu err {eg:.3e} fp32-oracle err {eo:.3e} ratio {eg / max(eo, 1e-30):.2f} floor {floor:.2e}")
        assert eg <= max(4 * eo, floor), (k, eg, eo, floor)


# ------------------------------------------------------------------- identities ---
@pytest.mark.parametrize("name", ["cornell", "tri_mesh"])
def test_scene_without_media(rt, gpu, name):
    """the existing kernels: rt_render_aov_emit's bits in all seven planes, scatter all zeros"""
    t, cam, wd, l = build(rt, name)
    with rt.Scene(t, wd, l) as sc:
        m = sc.render_aov(cam, n_samples=4, seed=3, emit=True, media=True)
        e = sc.render_aov(cam, n_samples=4, seed=3, emit=True)
        only = sc.render_aov(cam, n_samples=4, seed=3, media=True)
    for k in SURF + EMIT:
        assert np.array_equal(bits(m[k]), bits(e[k])), k
    for k in SURF:
        assert np.array_equal(bits(only[k]), bits(e[k])), k
    assert m["scatter"].dtype == np.float32 and not bits(m["scatter"]).any() and not bits(only["scatter"]).any()
    for k in ("samples", "segments", "rows", "tree_width", "kernel_features"):
        assert m["stats"][k] == e["stats"][k], k


@pytest.mark.parametrize("name", MEDIA_SCENES)
def test_unscattered_pixels_keep_the_transparent_bits(rt, gpu, name):
    """scatter == 0: the same samples, sums and order as rt_render_aov"""
    t, cam, wd, l = build(rt, name)
    with rt.Scene(t, wd, l) as sc:
        m = sc.render_aov(cam, n_samples=4, seed=3, emit=True, media=True)
        p = sc.render_aov(cam, n_samples=4, seed=3, emit=True)
    clear = m["scatter"] == 0
    if name == "smoke_box":
        assert clear.any() and (~clear).any()
    for k in SURF + EMIT:
        assert np.array_equal(bits(m[k])[clear], bits(p[k])[clear]), k
    s = ~clear
    assert (m["scatter"][s] > 0).all() and (m["scatter"] <= 1).all()
    assert (m["depth"][s] > 0).all()          # a miss behind a scatter is a medium event
    full = m["scatter"] == 1                  # every sample scattered: no normal, no light
    assert not m["normal"][full].any() and not m["coverage"][full].any()
    assert (m["material"][full] == ISOTROPIC).all()
    # a medium event is never a light sample: A_j = the albedo, E_j = 0
    assert np.array_equal(bits(m["surface_albedo"])[full], bits(m["albedo"])[full])


def test_cornell_smoke_depths(smoke):
    """every camera ray that meets the smoke ends on a wall (the border pixels' rays pass outside
    the box and miss: depth 0 in both), and a medium only wins with a smaller t"""
    m, p = smoke["media"], smoke["plain"]
    assert (m["depth"] <= p["depth"] * (1 + 1e-6)).all()
    s = m["scatter"] > 0
    assert s.any() and (m["depth"][s] < p["depth"][s]).all()
    for k in EMIT:  # with and without the split the first four planes are the same
        assert k in m
    assert not np.array_equal(m["albedo"], p["albedo"])


def test_agreement_with_the_render_trace(rt, gpu):
    """rt_render's trace_out record 0 of (pixel, sample): a medium prim-ref exactly when M_j, and
    the feature depth is its t |d|.  Sample 0 directly from n = 1 calls of several seeds; sample 1
    from the n = 2 prefix (the count exactly; the depth as 2 mean_2 - mean_1, so to the rounding of
    two fp32 means).  The tolerance is test_ray_identity_with_render_trace's 4 ulp, for its reason:
    |d| is recomputed here in numpy while the device's length() takes a sqrt that is not
    correctly rounded."""
    t, cam, wd, l = build(rt, "cornell_smoke")
    W = 24
    seen = set()
    with rt.Scene(t, wd, l) as sc:
        for seed in (3, 5):
            a1 = sc.render_aov(cam, n_samples=1, seed=seed, media=True)
            a2 = sc.render_aov(cam, n_samples=2, seed=seed, media=True)
            c1, c2 = count_of(a1["scatter"], 1), count_of(a2["scatter"], 2)
            for pix in (12 * W + 6, 13 * W + 7, 14 * W + 16, 16 * W + 15, 2 * W + 2, 12 * W + 12):
                y, x = divmod(pix, W)
                for j in (0, 1):
                    _, st = sc.render(cam, seed=seed, trace=(pix, j), mode="fused")
                    v0 = st["trace"][0]
                    ref = int(v0[11:12].view(np.uint32)[0])
                    medium = ref != 0xFFFFFFFF and (ref >> 30) == 3
                    mj = bool(c1[y, x]) if j == 0 else bool(c2[y, x] - c1[y, x])
                    assert medium == mj, (seed, pix, j)
                    seen.add(medium)
                    dlen = np.float32(np.sqrt(np.float32(v0[4]) ** 2 + np.float32(v0[5]) ** 2 + np.float32(v0[6]) ** 2))
                    want = np.float32(v0[8]) * dlen
                    if j == 0:
                        assert abs(a1["depth"][y, x] - want) <= 4 * np.spacing(a1["depth"][y, x]), (seed, pix)
                    else:
                        dj = 2.0 * float(a2["depth"][y, x]) - float(a1["depth"][y, x])
                        assert abs(dj - float(want)) <= 8 * np.spacing(np.float32(2 * a2["depth"][y, x])), (seed, pix)
    assert seen == {True, False}, "the pairs must hold scatters and surface hits"


def test_row_shares(rt, gpu, smoke):
    t, cam, wd, l = build(rt, "cornell_smoke")
    with rt.Scene(t, wd, l) as sc:
        part = sc.render_aov(cam, n_samples=4, seed=3, emit=True, media=True, rank=1, nranks=3)
    for k in SURF + EMIT + ("scatter",):
        assert np.array_equal(bits(smoke["media"][k][1::3]), bits(part[k])), k


def test_compressed_tree_and_plain_bvh4(rt, gpu, tune):
    """book2 takes the compressed BVH4 (tree 5); RT_QBVH=0 puts it on the 128-B nodes: the same
    closest hits under the same media, equal bits"""
    t, cam, wd, l = build(rt, "book2", 24, 24, 4)
    res = {}
    for q in ("1", "0"):
        tune("RT_QBVH", q)
        with rt.Scene(t, wd, l) as sc:
            res[q] = sc.render_aov(cam, n_samples=4, seed=3, emit=True, media=True)
    assert [res[q]["stats"]["tree_width"] for q in ("1", "0")] == [5, 4]
    assert (res["1"]["scatter"] > 0).any()
    for k in SURF + EMIT + ("scatter",):
        assert np.array_equal(bits(res["1"][k]), bits(res["0"][k])), k


def test_host_entry_equals_device_entry(rt, gpu, smoke):
    t, cam, wd, l = build(rt, "cornell_smoke")
    dev = torch.device("cuda", 0)
    shp = {"albedo": (24, 24, 3), "normal": (24, 24, 3), "depth": (24, 24), "emission": (24, 24, 3),
           "surface_albedo": (24, 24, 3), "coverage": (24, 24), "scatter": (24, 24)}
    tz = {k: torch.full(s, -7.0, dtype=torch.float32, device=dev) for k, s in shp.items()}
    tz["material"] = torch.full((24, 24), -7, dtype=torch.int32, device=dev)
    with rt.Scene(t, wd, l) as sc:
        st = sc.render_aov_device(cam, n_samples=4, seed=3, **{k: v.data_ptr() for k, v in tz.items()})
        # scatter alone is a call too; out and emit are NULL
        alone = torch.full((24, 24), -7.0, dtype=torch.float32, device=dev)
        sc.render_aov_device(cam, n_samples=4, seed=3, scatter=alone.data_ptr())
    torch.cuda.synchronize()
    for k in SURF + EMIT + ("scatter",):
        assert np.array_equal(bits(tz[k].cpu().numpy()), bits(smoke["media"][k])), k
    assert np.array_equal(bits(alone.cpu().numpy()), bits(smoke["media"]["scatter"]))
    assert st["samples"] == st["segments"] == 24 * 24 * 4


# ------------------------------------------------------------------ accumulator ---
@pytest.mark.parametrize("spp", [4, 16])
def test_one_pass_equals_the_media_feature_pass(rt, gpu, spp):
    t, cam, wd, l = build(rt, "cornell_smoke", 24, 24, spp)
    with rt.Scene(t, wd, l) as sc:
        ref = sc.render_aov(cam, n_samples=spp, seed=5, emit=True, media=True)
        with sc.accumulator(cam, features="emit+media") as a:
            assert a.features == "emit+media"
            a.add(5)
            got = a.resolve_aov()
        with sc.accumulator(cam, features="guides+media") as a:
            assert a.features == "guides+media"
            a.add(5)
            g2 = a.resolve_aov()
    assert set(got) == set(SURF[:3] + EMIT + ("scatter",)) and set(g2) == set(SURF[:3] + ("scatter",))
    assert (ref["scatter"] > 0).any()
    for k in SURF[:3] + EMIT + ("scatter",):  # spp a power of two: bit-equal
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    for k in SURF[:3] + ("scatter",):
        assert np.array_equal(bits(g2[k]), bits(ref[k])), k


def test_passes_active_pixels_and_reset(rt, gpu):
    t, cam, wd, l = build(rt, "cornell_smoke")
    H = W = 24
    with rt.Scene(t, wd, l) as sc:
        refs = {s: sc.render_aov(cam, n_samples=4, seed=s, emit=True, media=True) for s in (3, 4, 7)}
        cnt = {s: count_of(refs[s]["scatter"], 4) for s in refs}
        mask = np.zeros((H, W), bool)
        mask[:, : W // 2] = True
        mask[13, 16] = True
        assert (cnt[7] > 0)[mask].any() and (cnt[7] > 0)[~mask].any()
        with sc.accumulator(cam, features="emit+media") as a:
            a.add(3)
            a.add(4)
            two = a.resolve_aov()
            # two passes of different seeds: the total count over N = 8
            assert np.array_equal(two["scatter"], ((cnt[3] + cnt[4]) / 8).astype(np.float32))
            assert np.array_equal(two["coverage"],
                                  ((refs[3]["coverage"].astype(float) + refs[4]["coverage"]) / 2).astype(np.float32))
            assert a.set_active(mask) == int(mask.sum())
            a.add_active(7)
            three = a.resolve_aov()
            for k in three:  # only the masked pixels moved
                assert np.array_equal(bits(three[k])[~mask], bits(two[k])[~mask]), k
            assert np.array_equal(three["scatter"][mask], ((cnt[3] + cnt[4] + cnt[7]) / 12).astype(np.float32)[mask])
            # ... to the bits of three whole passes
            with sc.accumulator(cam, features="emit+media") as b:
                for s in (3, 4, 7):
                    b.add(s)
                whole = b.resolve_aov()
            for k in three:
                assert np.array_equal(bits(three[k])[mask], bits(whole[k])[mask]), k
            a.reset()
            assert a.features == "emit+media"
            a.add(7)
            one = a.resolve_aov()
            for k in one:  # the count was cleared with the sums
                assert np.array_equal(bits(one[k]), bits(refs[7][k])), k


def test_without_the_bit_the_parent_bits(rt, gpu, smoke):
    """the same accumulator without RT_ACCUM_FEAT_MEDIA: rt_render_aov_emit's planes, no scatter
    plane, and asking for one is refused; the bit alone is refused too"""
    import ctypes as C
    t, cam, wd, l = build(rt, "cornell_smoke")
    E = rt._lib.RT_ERR_INVALID
    with rt.Scene(t, wd, l) as sc:
        with sc.accumulator(cam, features="emit") as a:
            a.add(3)
            got = a.resolve_aov()
            buf = np.zeros((24, 24), np.float32)
            md = rt._lib.RtAovMedia(buf.ctypes.data)
            assert rt.lib().rt_accum_resolve_aov_media(a._h(), None, None, C.byref(md)) == E
            assert b"scatter" in rt.lib().rt_last_error()
            assert rt.lib().rt_accum_resolve_aov_media(a._h(), None, None, C.byref(rt._lib.RtAovMedia())) == E
            # the other planes through the media entry: the same bits
            alb = np.zeros((24, 24, 3), np.float32)
            ao = rt._lib.RtAov(alb.ctypes.data, None, None, None)
            assert rt.lib().rt_accum_resolve_aov_media(a._h(), C.byref(ao), None, C.byref(rt._lib.RtAovMedia())) == 0
            assert np.array_equal(bits(alb), bits(got["albedo"]))
        with sc.accumulator(cam) as a:
            assert rt.lib().rt_accum_set_features(a._h(), rt._lib.RT_ACCUM_FEAT_MEDIA) == E
            assert rt.lib().rt_accum_set_features(a._h(), 8 | 1) == E
            assert a.features is None
            assert rt.lib().rt_accum_set_features(a._h(), 5) == 0
            a.add(3)
            assert rt.lib().rt_accum_set_features(a._h(), 1) == E  # holds a pass
            first = a.resolve_aov()
    assert "scatter" not in got
    for k in SURF[:3] + EMIT:
        assert np.array_equal(bits(got[k]), bits(smoke["emit"][k])), k
    for k in SURF[:3]:  # rt_accum_resolve_aov on a media accumulator: the first-event planes
        assert np.array_equal(bits(first[k]), bits(smoke["media"][k])), k


def test_denoiser_and_temporal_run_on_a_media_accumulator(rt, gpu):
    t, cam, wd, l = build(rt, "cornell_smoke")
    with rt.Scene(t, wd, l) as sc, sc.accumulator(cam, features="emit+media") as a:
        for s in (3, 4, 5, 6):
            a.add(s)
        out = a.denoise_device()
        aov = a.resolve_aov_device()
        assert "scatter" in aov and aov["scatter"].shape == (24, 24)
        mean = torch.empty((24, 24, 3), dtype=torch.float32, device=out.device)
        var = torch.empty((24, 24), dtype=torch.float32, device=out.device)
        a.resolve_device(mean, var)
        want = rt.denoise_var_device(mean, var, aov, split_emitters=True)  # the planes it reads today
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        assert torch.isfinite(out).all()
        tp = rt.Temporal(split_emitters=True)
        rgb, v, cnt = tp.push(a)
        assert torch.equal(rgb, mean) and float(cnt.min()) == 4.0
        rgb2, _, cnt2 = tp.push(a)
        assert torch.isfinite(rgb2).all() and float(cnt2.max()) > 4.0


# -------------------------------------------------------------------------- CLI ---
def test_cli_planes(rt, gpu, tmp_path):
    """rtbench -S 7 -width 32 -spp 4 -aov feat: with -aov-media the Python path's bytes, and a
    scatter plane; without the flag the transparent planes and no such file"""
    t, cam, wd, l = build(rt, "cornell_smoke", 32, 32, 4)
    with rt.Scene(t, wd, l) as sc:
        m = sc.render_aov(cam, n_samples=4, seed=1, media=True)
        p = sc.render_aov(cam, n_samples=4, seed=1)

    def planes(a):
        dmax = a["depth"].max()
        return {"albedo": a["albedo"], "normal": a["normal"] * np.float32(0.5) + np.float32(0.5),
                "depth": np.repeat((a["depth"] / dmax)[..., None], 3, -1)}

    for flag, ref in ((["-aov-media"], m), ([], p)):
        d = tmp_path / ("m" if flag else "p")
        d.mkdir()
        r = subprocess.run([CLI, "-S", "7", "-width", "32", "-spp", "4", "-aov", str(d / "feat"), *flag, "-stats",
                            "-o", str(d / "o.ppm")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for k, img in planes(ref).items():
            assert (d / f"feat_{k}.ppm").read_bytes() == rt.format_ppm(img), (flag, k)
        js = json.loads(r.stderr.strip().splitlines()[-1])
        if flag:
            grey = np.repeat(m["scatter"][..., None], 3, -1)
            assert (d / "feat_scatter.ppm").read_bytes() == rt.format_ppm(grey)
            assert js["aov_media"] == 1
        else:
            assert not (d / "feat_scatter.ppm").exists() and "aov_media" not in js
    assert (tmp_path / "m" / "o.ppm").read_bytes() == (tmp_path / "p" / "o.ppm").read_bytes()
    assert (tmp_path / "m" / "feat_depth.ppm").read_bytes() != (tmp_path / "p" / "feat_depth.ppm").read_bytes()


# ------------------------------------------------- measured, asserted by nothing ---
def test_quality_table_is_reported(rt, gpu):
    """tools/aov_media_bench.py's table at 48 x 48 (cornell_smoke, 4 spp x 4 passes, MSE against
    1024 spp): printed, with DESIGN.md §18's 128 x 128 table beside it.  Whether first-event
    guides lower the filtered error is a measurement, not a bar: only the table's shape and
    finiteness are checked."""
    from tools.aov_media_bench import quality
    q = quality(48)
    print(json.dumps(q, indent=1))
    assert set(q["mse"]) == {"mean", "denoise_var_transparent", "denoise_var_transparent_split",
                             "denoise_var_media", "denoise_var_media_split"}
    assert q["sets"]["all"] == 48 * 48 and 0 < q["sets"]["scatter"] < 48 * 48 and q["sets"]["silhouette"] > 0
    for row in q["mse"].values():
        assert set(row) == {"all", "scatter", "silhouette"} and all(np.isfinite(v) for v in row.values())
