"""Adaptive passes of the accumulator (rt_accum.hip, rt_fused_map.hip) on the GPU.

The random stream is keyed by (seed, global pixel, sample) and the pixel sums are integers, so a
pass over any subset of the pixels gives each of them exactly what a whole pass of that seed
gives it: the exactness tests are bitwise.  Images are 37 x 23 at 16 spp unless stated, as in
tests/test_accum_gpu.py (851 pixels: no multiple of 64 or 256, more than one 256-pixel block)."""
import numpy as np
import pytest
import torch  # noqa: F401  before the library's HIP runtime initialises (one runtime per process)

pytestmark = pytest.mark.gpu

LUM = np.array([0.2126, 0.7152, 0.0722])
EPS = 2.0 ** -24


def _shape(cam, w=37, h=23, spp=16):
    cam.Width, cam.AspectRatio, cam.SamplesPerPixel = w, w / (h + 0.5), spp
    assert cam.image_size()[:2] == (w, h)
    return cam


def _cases():
    # (id, scene, camera changes, accumulator options, knobs): tests/test_accum_gpu.py _one_pass_cases
    # without the wavefront one (refused: test_refusals)
    return [
        ("cornell", "cornell", {}, {}, {}),                       # record loop, chunk records
        ("cornell_csum0", "cornell", {}, {}, {"RT_CSUM": "0"}),   # pixel atomics
        ("cornell_rank1of3", "cornell", {}, {"rank": 1, "nranks": 3}, {}),
        ("book1", "book1", {"w": 40}, {"mode": "fused"}, {}),     # trees 4 / 5 as planned
        ("book1_two_phase", "book1", {"w": 40, "spp": 64}, {"chunk": 32},
         {"RT_TAIL_FRAC": "4", "RT_TAIL_K": "4"}),
        ("cornell_smoke", "cornell_smoke", {}, {}, {}),
    ]


def _masks(shape):
    rows, W = shape
    m = {}
    m["first"] = np.zeros(shape, bool)
    m["first"][0, 0] = True
    m["last"] = np.zeros(shape, bool)
    m["last"][-1, -1] = True
    m["checker"] = (np.add.outer(np.arange(rows), np.arange(W)) % 2) == 0
    m["row"] = np.zeros(shape, bool)
    m["row"][rows // 2] = True
    m["all"] = np.ones(shape, bool)  # takes the whole-pass path
    m["all_but_one"] = np.ones(shape, bool)
    m["all_but_one"][rows // 3, W // 3] = False
    return m


# ------------------------------------------------------------------------- 1. exactness --
@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_active_pass_is_exact(rt, gpu, tune, case):
    """Passes 1 and 2, set_active(M), add_active(3): the pixels of M hold the bits of whole
    passes 1, 2, 3, the others those of passes 1, 2."""
    _, name, shape, opts, knobs = case
    t, cam, w, l = rt.demo_scene(name)
    if "w" in shape:
        cam.Width, cam.SamplesPerPixel = shape["w"], shape.get("spp", 16)
    else:
        _shape(cam)
    spp = shape.get("spp", 16)
    for k, v in knobs.items():
        tune(k, v)
    with rt.Scene(t, w, l) as sc, sc.accumulator(cam, max_passes=4, **opts) as acc:
        acc.add(1)
        acc.add(2)
        rgb2, var2 = acc.resolve()
        acc.add(3)
        rgb3, var3 = acc.resolve()
        assert not np.array_equal(rgb2, rgb3)
        for mid, M in _masks(acc.shape).items():
            acc.reset()
            acc.add(1)
            acc.add(2)
            assert acc.set_active(M) == M.sum(), mid
            st = acc.add_active(3)
            rgb, var = acc.resolve()
            cnt = acc.counts()
            assert st["samples"] == int(M.sum()) * spp and st["overflow_samples"] == 0, mid
            if name == "cornell":  # chunk records unless RT_CSUM=0: the pass fits the whole passes' buffer
                assert st["chunk_records"] == (0 if knobs else 1), mid
            assert np.array_equal(cnt, np.where(M, 3, 2)), mid
            for got, in3, in2 in ((rgb, rgb3, rgb2), (var, var3, var2)):
                assert np.array_equal(got[M], in3[M], equal_nan=True), mid
                assert np.array_equal(got[~M], in2[~M], equal_nan=True), mid
            i = acc.info()
            assert i["passes"] == 3 and i["samples_per_pixel"] == 3 * spp, mid
            a = acc.adapt_info()
            assert a["active_pixels"] == M.sum() and a["total_samples"] == int(cnt.sum()) * spp, mid
            assert (a["min_count"], a["max_count"]) == (cnt.min(), cnt.max()), mid


def test_default_bvh2_scene_takes_the_bvh4(rt, gpu, tune):
    """The BVH2 as the dispatcher's own choice, not RT_TREE's: a lean scene above the record
    loop's limit whose BVH2 and records fit the LDS budget.  With the default limit of 48 that
    takes 49..64 leaf entries in a handful of 16-prim leaves (the media set's budget is 56
    slots, the lean set's 34), which no scene here has; RT_BRUTE_MAX=8 puts Cornell's 18 entries
    there through the same rule.  The active-pixel kernels have no BVH2 twin: an active pass
    traverses the BVH4 of the same leaf records (the same closest hits) instead of refusing,
    and stays bit for bit what the BVH2's whole pass gives those pixels."""
    t, cam, w, l = rt.demo_scene("cornell")
    _shape(cam)
    tune("RT_BRUTE_MAX", "8")
    with rt.Scene(t, w, l) as sc, sc.accumulator(cam, max_passes=4) as acc:
        st = [acc.add(1), acc.add(2)]
        rgb2, var2 = acc.resolve()
        st.append(acc.add(3))
        rgb3, var3 = acc.resolve()
        assert [x["tree_width"] for x in st] == [2, 2, 2] and not np.array_equal(rgb2, rgb3)
        for mid, M in _masks(acc.shape).items():
            acc.reset()
            acc.add(1)
            acc.add(2)
            acc.set_active(M)
            sa = acc.add_active(3)
            assert sa["tree_width"] == (2 if M.all() else 4), mid
            rgb, var = acc.resolve()
            for got, in3, in2 in ((rgb, rgb3, rgb2), (var, var3, var2)):
                assert np.array_equal(got[M], in3[M], equal_nan=True), mid
                assert np.array_equal(got[~M], in2[~M], equal_nan=True), mid
        i = acc.render_adaptive(1e-3, 4, seed=1)  # goes on past the whole passes without a refusal
        assert i["passes"] == 4


# ---------------------------------------------------- 2. pass order and interleaving --
@pytest.fixture(scope="module")
def cornell(rt, gpu):
    t, cam, w, l = rt.demo_scene("cornell")
    _shape(cam)
    with rt.Scene(t, w, l) as sc:
        imgs = {s: sc.render(cam, seed=s)[0] for s in (1, 2, 3, 4, 5)}
        for v in imgs.values():
            v.setflags(write=False)
        yield sc, cam, imgs


def _welford(ys):
    mean, m2 = np.zeros_like(ys[0]), np.zeros_like(ys[0])
    for n, y in enumerate(ys, 1):
        d = y - mean
        mean = mean + d / n
        m2 = m2 + d * (y - mean)
    return mean, m2


def test_whole_pass_after_active_passes(rt, cornell):
    """add 1, 2; active 3 on A; a render of another size; whole pass 4; active 5 on B.  Every
    pixel then holds Welford's recurrence over the passes it took, in their order, and the mean
    of those passes: against numpy on Scene.render's fp32 images with the bars derived in
    tests/test_accum_gpu.py test_against_numpy (n is the pixel's own count)."""
    sc, cam, imgs = cornell
    other = rt.demo_scene("cornell")[1]
    other.Width, other.SamplesPerPixel = 61, 4
    with sc.accumulator(cam, max_passes=8) as acc:
        rows, W = acc.shape
        A = np.zeros(acc.shape, bool)
        A[:, : W // 2] = True
        B = np.zeros(acc.shape, bool)
        B[rows // 3:, W // 4:] = True
        acc.add(1)
        acc.add(2)
        acc.set_active(A)
        acc.add_active(3)
        sc.render(other, seed=11)
        acc.add(4)
        acc.set_active(B)
        acc.add_active(5)
        rgb, var = acc.resolve()
        cnt = acc.counts()
        info = acc.info()
    assert info["passes"] == 5 and info["samples_per_pixel"] == 5 * 16
    assert np.array_equal(cnt, 3 + A.astype(int) + B.astype(int))
    worst = 0.0
    for a in (False, True):
        for b in (False, True):
            sel = (A == a) & (B == b)
            assert sel.any()
            seeds = [1, 2] + ([3] if a else []) + [4] + ([5] if b else [])
            n = len(seeds)
            I = np.stack([imgs[s].astype(np.float64)[sel] for s in seeds])
            err = np.abs(rgb.astype(np.float64)[sel] - I.mean(axis=0))
            assert (err <= 2.0 ** -23 * np.abs(I).max()).all(), seeds
            Y = I @ LUM
            _, m2 = _welford(list(Y))
            var_ref = m2 / (n * (n - 1))
            ymax = Y.max(axis=0)
            e = EPS * (1 + 2.0 ** -23) * ymax
            dvar = (4 * e * np.abs(Y - Y.mean(axis=0)).sum(axis=0) + 4 * n * e * e + n * 2.0 ** -50 * ymax ** 2) / (n * (n - 1))
            tol = dvar + EPS * (var_ref + dvar) + 2.0 ** -149
            verr = np.abs(var.astype(np.float64)[sel] - var_ref)
            worst = max(worst, (verr / tol).max())
            assert (verr <= tol).all(), seeds
    print("var: largest error / bound", worst)


def test_whole_passes_stay_uniform(cornell):
    """After three whole passes counts() is 3 everywhere and adapt_info() has min = max = 3
    (the uniform accumulator answers without per-pixel counts); a pass over a selection of
    every pixel is the whole pass: set_active(all) + add_active(4) resolves to the bits of
    add(4), and the counts stay uniform."""
    sc, cam, _ = cornell
    with sc.accumulator(cam, max_passes=8) as acc, sc.accumulator(cam, max_passes=8) as ref:
        for a in (acc, ref):
            for seed in (1, 2, 3):
                a.add(seed)
        assert (acc.counts() == 3).all()
        i = acc.adapt_info()
        assert (i["min_count"], i["max_count"]) == (3, 3)
        assert acc.set_active(np.ones(acc.shape, bool)) == acc.shape[0] * acc.shape[1]
        acc.add_active(4)
        ref.add(4)
        assert _same(_state(acc), _state(ref))
        assert (acc.counts() == 4).all()
        i = acc.adapt_info()
        assert (i["min_count"], i["max_count"], i["total_samples"]) == (4, 4, 4 * 16 * acc.counts().size)


# ------------------------------------------------------------------------ 3. refusals --
def _state(acc):
    return acc.resolve() + (acc.counts(), acc.info())


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_refusals(rt, cornell, tune):
    sc, cam, _ = cornell
    U, E = rt._lib.RT_ERR_UNSUPPORTED, rt._lib.RT_ERR_INVALID
    with sc.accumulator(cam, max_passes=4) as acc:
        M = np.zeros(acc.shape, bool)
        M[2:5, 3:9] = True
        with pytest.raises(rt.RtError) as e:  # no selection yet
            acc.add_active(1)
        assert e.value.code == E
        acc.add(1)
        acc.add(2)
        before = _state(acc)
        assert acc.set_active(np.zeros(acc.shape, bool)) == 0
        assert acc.add_active(3)["samples"] == 0 and _same(before, _state(acc))  # a no-op, no pass
        acc.set_active(M)
        tune("RT_TREE", "2")  # the BVH2 kernels have no active-pixel twin
        with pytest.raises(rt.RtError) as e:
            acc.add_active(3)
        assert e.value.code == U and "RT_TREE" in str(e.value) and _same(before, _state(acc))
        rt.untune()
        acc.add_active(3)  # the selection survived the refusal
        assert acc.counts()[3, 4] == 3 and acc.counts()[0, 0] == 2
        with pytest.raises(rt.RtError) as e:  # consumed by that pass
            acc.add_active(4)
        assert e.value.code == E
        acc.set_active(M)
        acc.add(4)  # a whole pass drops the selection too
        with pytest.raises(rt.RtError) as e:
            acc.add_active(5)
        assert e.value.code == E
        acc.set_active(M)
        with pytest.raises(rt.RtError) as e:  # the accumulator holds its 4 passes
            acc.add_active(5)
        assert e.value.code == E
        acc.set_active(M)
        acc.reset()
        with pytest.raises(rt.RtError) as e:
            acc.add_active(1)
        assert e.value.code == E and not acc.counts().any()
    with sc.accumulator(cam, max_passes=4, mode="wavefront") as acc:
        acc.add(1)
        acc.add(2)
        before = _state(acc)
        acc.set_active(M)
        with pytest.raises(rt.RtError) as e:
            acc.add_active(3)
        assert e.value.code == U and _same(before, _state(acc))
        acc.set_active(np.ones(acc.shape, bool))  # every pixel: the whole-pass path, any mode
        acc.add_active(3)
        assert (acc.counts() == 3).all()


# ----------------------------------------------------------------------- 4. selection --
def _tile_error_numpy(rgb, var, cnt, tile, lum_floor=1e-2):
    rows, W = var.shape
    ty, tx = -(-rows // tile), -(-W // tile)
    out = np.zeros((ty, tx))
    v = var.astype(np.float64)
    m = rgb.astype(np.float64) @ LUM
    ok = np.isfinite(v) & np.isfinite(m)
    for j in range(ty):
        for i in range(tx):
            s = (slice(j * tile, (j + 1) * tile), slice(i * tile, (i + 1) * tile))
            k = ok[s].sum()
            if k:
                out[j, i] = np.sqrt(v[s][ok[s]].sum() / k) / (max(m[s][ok[s]].sum() / k, 0.0) + lum_floor)
    return out


def _expand(tiles, tile, shape):
    return np.repeat(np.repeat(tiles, tile, axis=0), tile, axis=1)[: shape[0], : shape[1]]


def test_tile_error_and_selection(cornell):
    """e_T against numpy from resolve() and counts(): the inputs are fp32 roundings of the fp64
    values the device sums (2^-24 each, relative, on non-negative terms: 2^-24 on either mean,
    2^-25 after the root) and the result is rounded to fp32: within 3 x 2^-24; the bar is
    8 x 2^-24 relative + 1e-12.  Then the selection at the median of the device's own e_T."""
    sc, cam, _ = cornell
    with sc.accumulator(cam, max_passes=8) as acc:
        for s in (1, 2, 3, 4):
            acc.add(s)
        rgb, var = acc.resolve()
        cnt = acc.counts()
        assert (cnt == 4).all()
        worst = 0.0
        for tile in (8, 1, 5):
            e = acc.tile_error(tile=tile)
            ref = _tile_error_numpy(rgb, var, cnt, tile)
            assert e.shape == ref.shape == (-(-23 // tile), -(-37 // tile))
            d = np.abs(e - ref)
            worst = max(worst, (d / (8 * EPS * ref + 1e-12)).max())
            assert (d <= 8 * EPS * ref + 1e-12).all(), tile
        print("tile error: largest error / bound", worst)
        e = acc.tile_error(tile=8)
        assert np.array_equal(e, acc.tile_error(tile=8)) and e.max() > 0
        med = float(np.median(e))
        want = _expand(e > np.float32(med), 8, acc.shape)
        assert 0 < want.sum() < want.size
        assert acc.select(med, tile=8) == want.sum()
        a = acc.adapt_info()
        assert a["active_pixels"] == want.sum() and a["n_tiles"] == e.size and a["active_tiles"] == (e > med).sum()
        st = acc.add_active(5)
        assert st["samples"] == int(want.sum()) * 16
        assert np.array_equal(acc.counts(), 4 + want)
        # min_passes: every tile holds a pixel with fewer than 6 passes now
        assert acc.select(1e9, tile=8, min_passes=6) == want.size
        assert acc.select(1e9, tile=8, min_passes=4) == 0
        assert acc.select(1e9, tile=8, min_passes=5) == (~want).sum()


def test_nonfinite_pixels_are_ignored(rt, gpu):
    """A light whose emission is not finite: the pixels that see it hold non-finite means and
    variances.  They are left out of every tile's sums, and a tile made only of them has
    e_T = 0 and is inactive."""
    t = rt.Tree(1)
    world = t.list()
    t.add(world, t.quad((-2, -2, -1), (4, 0, 0), (0, 4, 0), t.light((float("inf"), 1.0, 0.5))))
    # in the light's plane, beside it: its edge pixels mix its colour and the background's from
    # pass to pass (finite, noisy), and no path from it reaches the light
    t.add(world, t.quad((-3.8, -1, -1), (1.2, 0, 0), (0, 2, 0), t.lambertian((0.7, 0.2, 0.2))))
    cam = _shape(rt.Camera(Background=(0.2, 0.3, 0.4)))
    cam.PositionCamera((0, 0, 3), (0, 0, 0))
    tile = 4
    with rt.Scene(t, world, -1) as sc, sc.accumulator(cam, max_passes=8) as acc:
        for s in (1, 2, 3, 4):
            acc.add(s)
        rgb, var = acc.resolve()
        bad = ~(np.isfinite(var) & np.isfinite(rgb).all(axis=2))
        assert acc.info()["nonfinite_pixels"] == bad.sum() > 0
        e = acc.tile_error(tile=tile)
        ref = _tile_error_numpy(rgb, var, acc.counts(), tile)
        assert np.isfinite(e).all() and (np.abs(e - ref) <= 8 * EPS * ref + 1e-12).all()
        all_bad = np.array([[bad[j:j + tile, i:i + tile].all() for i in range(0, 37, tile)]
                            for j in range(0, 23, tile)])
        assert all_bad.any() and not e[all_bad].any()
        n = acc.select(1e-9, tile=tile)  # every tile with a finite, noisy pixel
        acc.add_active(5)
        got = acc.counts() == 5
        assert 0 < n == got.sum() and not got[_expand(all_bad, tile, acc.shape)].any()
        assert np.array_equal(got, _expand(e > np.float32(1e-9), tile, acc.shape))


# ------------------------------------------------------------------ 5. render_adaptive --
def test_render_adaptive(rt, gpu):
    """Cornell 48 x 48 at 4 spp, at most 32 passes.  rel_error is the upper quartile of e_T after
    8 whole passes of the same camera (measured here, on the device that runs the test)."""
    t, cam, w, l = rt.demo_scene("cornell")
    _shape(cam, 48, 48, 4)
    with rt.Scene(t, w, l) as sc:
        with sc.accumulator(cam, max_passes=8) as acc:
            for s in range(1, 9):
                acc.add(s)
            target = float(np.quantile(acc.tile_error(), 0.75))
        assert target > 0
        with sc.accumulator(cam, max_passes=32) as acc:
            a = acc.render_adaptive(target, 32, seed=1)
            e, cnt, info = acc.tile_error(), acc.counts(), acc.info()
            rgb, _ = acc.resolve()
    print("render_adaptive:", a, "target", target)
    full = _expand(np.ones_like(e, bool), 8, cnt.shape)
    assert full.all()
    tile_max = np.array([[cnt[j:j + 8, i:i + 8].max() for i in range(0, 48, 8)] for j in range(0, 48, 8)])
    assert ((e <= np.float32(target)) | (tile_max == 32)).all()
    assert a["total_samples"] == int(cnt.sum()) * 4 <= 32 * 4 * cnt.size
    assert a["max_count"] > a["min_count"] >= 4 and a["passes"] == info["passes"] <= 32
    assert a["max_count"] == cnt.max() and info["samples_per_pixel"] == 4 * cnt.max()
    assert np.isfinite(rgb).all()
