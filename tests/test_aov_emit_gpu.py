"""The emission split of the feature pass (rt_render_aov_emit, k_aov<TREE, true> in rt_aov.hip).

1. rt_render_aov's four buffers are unchanged, and two calls give the same bits.
2. Self-consistency on Cornell, derived from the definition: the light is solid e = 15 and the
   demo camera never sees its back, so albedo = surface_albedo + coverage e and emission =
   coverage e, and coverage is a multiple of 1 / n.  (The emission is not clamped: rayColor
   returns a light's emission, camera.go:312-314, before the clampContribution of
   camera.go:330, and the oracle of check 3 renders 15 on a covered pixel, not
   clampContribution(15, 15, 15) = 0.5.)  Cornell 16 x 12 shows
   the light on a strip 2 pixels wide and 0.4 pixels tall: no pixel is covered entirely.  The
   smallest 4 : 3 size (in steps of 8 x 6, seed 3, n = 4) at which the fp64 oracle has both a
   pixel with every sample on the light and a rim pixel is 40 x 30, used here.
3. Against the oracle, without touching it: in a Cornell box whose Lambertians are all black,
   pyoracle.render with spp = n IS the emission buffer (a surface returns 0, a first-hit light
   its emission), and the number of pyoracle.trace first hits on the light's front
   is coverage n.  Bar: tests/test_aov_gpu.py's (4 x the error of the oracle's own
   precision=32 run, floored at one fp32 ulp of the buffer's scale), with that file's 1 % cap
   on the pixels where the GPU, or the fp32 twin, counts another number of light samples
   than the fp64 oracle (silhouette samples).
4. Row shares and the other structures (BVH2, BVH4, compressed BVH4) agree with the default."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_aov_gpu import _shape

pytestmark = pytest.mark.gpu

LIGHT = 3  # RT_MAT_DIFFUSE_LIGHT
E = (15.0, 15.0, 15.0)
FORK_CAP = 0.01  # tests/test_aov_gpu.py run_scene's fork_cap


def shape(cam, w, h, n):
    """w x h pixels, n samples per pixel: n_samples = n is every sample of the camera"""
    return _shape(cam, w, h, spp=n)


def black_cornell(rt, light="solid"):
    """The demo Cornell box (tests/scenes.py cornell_room) with every Lambertian black.
    light: "solid" (15, 15, 15); "checker" (cells of 40: no cell border at the light's
    y = 550); "flipped" (u and v swapped: the demo camera sees the one-sided light's back).
    -> (tree, camera, world, lights, outward normal of the light quad)"""
    t = rt.Tree(1)
    black = t.lambertian((0.0, 0.0, 0.0))
    lm = t.light(t.checker(40.0, t.solid(*E), t.solid(4.0, 2.0, 1.0))) if light == "checker" else t.light(E)
    world = t.list()
    t.add(world, t.quad((555, 0, 0), (0, 555, 0), (0, 0, 555), black))
    t.add(world, t.quad((0, 0, 0), (0, 555, 0), (0, 0, 555), black))
    t.add(world, t.quad((0, 0, 0), (555, 0, 0), (0, 0, 555), black))
    t.add(world, t.quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), black))
    t.add(world, t.quad((0, 0, 555), (555, 0, 0), (0, 555, 0), black))
    u, v = (-130, 0, 0), (0, 0, -105)
    if light == "flipped":
        u, v = v, u
    ll = t.list()
    t.add(ll, t.quad((343, 550, 332), u, v, lm))
    t.add(world, ll)
    t.add(world, t.translate(t.rotate_y(t.box((0, 0, 0), (165, 330, 165), black), 15), (265, 0, 295)))
    t.add(world, t.translate(t.rotate_y(t.box((0, 0, 0), (165, 165, 165), black), -18), (130, 0, 65)))
    _, cam, _, _ = rt.demo_scene("cornell")
    nrm = np.cross(u, v).astype(float)
    return t, cam, t.bvh(world), ll, nrm / np.linalg.norm(nrm)


def light_count(oracle, t, world, lights, cam, n, seed, precision, normal=None):
    """int [H, W]: the samples < n whose first world.Hit is a light (pyoracle.trace record 0
    of kind RT_MAT_DIFFUSE_LIGHT); with `normal`, only those that see its front"""
    import copy
    c1 = copy.copy(cam)
    c1.MaxDepth = 1  # the camera ray does not depend on it; one world.Hit per trace
    d = cam.derived()
    out = np.zeros((d.height, d.width), int)
    for p in range(d.width * d.height):
        for j in range(n):
            rec = oracle.trace(t, world, lights, c1, p, j, seed=seed, precision=precision)[0]
            if int(rec[11]) == LIGHT and (normal is None or np.dot(rec[4:7].astype(float), normal) < 0):
                out[p // d.width, p % d.width] += 1
    return out


EMIT = ("emission", "surface_albedo", "coverage")


@pytest.mark.parametrize("w,h,n", [(16, 12, 4), (13, 9, 1)])
def test_aov_buffers_unchanged_and_deterministic(rt, gpu, w, h, n):
    t, cam, wd, l = rt.demo_scene("cornell")
    shape(cam, w, h, 4)
    with rt.Scene(t, wd, l) as sc:
        old = sc.render_aov(cam, n_samples=n, seed=3)
        new = sc.render_aov(cam, n_samples=n, seed=3, emit=True)
        again = sc.render_aov(cam, n_samples=n, seed=3, emit=True)
    for k in ("albedo", "normal", "depth", "material"):
        assert np.array_equal(old[k].view(np.uint32), new[k].view(np.uint32)), k
    for k in EMIT:
        assert new[k].shape == ((h, w, 3) if k != "coverage" else (h, w))
        assert np.array_equal(new[k].view(np.uint32), again[k].view(np.uint32)), k
    assert new["stats"]["samples"] == old["stats"]["samples"] == w * h * n
    assert new["stats"]["tree_width"] == old["stats"]["tree_width"]


def test_self_consistency_on_cornell(rt, gpu):
    w, h, n = 40, 30, 4  # the smallest size with a fully covered pixel: the module docstring
    t, cam, wd, l = rt.demo_scene("cornell")
    shape(cam, w, h, n)
    with rt.Scene(t, wd, l) as sc:
        g = sc.render_aov(cam, n_samples=n, seed=3, emit=True)
    cov = g["coverage"]
    k = np.rint(cov.astype(float) * n)
    assert np.array_equal(cov, (k.astype(np.float32) / np.float32(n)))  # exactly k / n, k integer
    assert cov.min() == 0.0 and cov.max() == 1.0
    full, rim = cov == 1.0, (cov > 0) & (cov < 1)
    print(f"cornell {w}x{h} n={n}: {int(full.sum())} pixels covered, {int(rim.sum())} rim pixels")
    assert full.any() and rim.any(), "the fixture must exercise the rim and a covered pixel"
    e = np.array(E)
    ulp15 = float(np.spacing(np.float32(15.0)))  # the scale of the albedo and of the emission
    sa = g["surface_albedo"].astype(float) + cov.astype(float)[..., None] * e
    ea = np.abs(g["albedo"].astype(float) - sa).max()
    ee = np.abs(g["emission"].astype(float) - cov.astype(float)[..., None] * e).max()
    print(f"albedo - (surface_albedo + coverage e): {ea:.3e}; emission - coverage e: {ee:.3e} "
          f"(4 ulp {4 * ulp15:.3e})")
    assert ea <= 4 * ulp15
    assert ee <= 4 * ulp15
    assert (g["surface_albedo"][full] == 0).all() and (g["emission"][cov == 0] == 0).all()


def test_device_entry_with_one_buffer_wanted(rt, gpu):
    """render_aov_device asked for exactly one of the seven buffers writes that buffer with the
    bits of the call that asks for all seven, for each buffer in turn (Cornell 40 x 30, n = 4:
    covered and rim pixels, 1200 pixels = more than one block and no multiple of 256)."""
    w, h, n = 40, 30, 4
    t, cam, wd, l = rt.demo_scene("cornell")
    shape(cam, w, h, n)
    dev = torch.device("cuda", 0)
    planes = {"albedo": 3, "normal": 3, "depth": 0, "material": 0, "emission": 3, "surface_albedo": 3,
              "coverage": 0}

    def buf(k):
        dt = torch.int32 if k == "material" else torch.float32
        return torch.full((h, w, planes[k]) if planes[k] else (h, w), -7, dtype=dt, device=dev)

    stream = torch.cuda.current_stream(dev).cuda_stream
    with rt.Scene(t, wd, l) as sc:
        every = {k: buf(k) for k in planes}
        sc.render_aov_device(cam, n_samples=n, seed=3, stream=stream,
                             **{k: v.data_ptr() for k, v in every.items()})
        every = {k: v.cpu().numpy() for k, v in every.items()}
        assert every["coverage"].max() == 1.0 and (every["material"] == LIGHT).any()
        for k in planes:
            one = buf(k)
            sc.render_aov_device(cam, n_samples=n, seed=3, stream=stream, **{k: one.data_ptr()})
            assert np.array_equal(one.cpu().numpy(), every[k]), k


_oracle_cache = {}


def oracle_side(rt, oracle, kind, w, h, n, seed):
    """the CPU side of one case, computed once: fp64 and fp32 renders and light counts"""
    key = (kind, w, h, n, seed)
    if key not in _oracle_cache:
        t, cam, world, lights, nrm = black_cornell(rt, kind)
        shape(cam, w, h, n)
        r = {p: oracle.render(t, world, lights, cam, seed=seed, precision=p)[0].astype(np.float64)
             for p in (64, 32)}
        c = {p: light_count(oracle, t, world, lights, cam, n, seed, p, nrm) for p in (64, 32)}
        seen = light_count(oracle, t, world, lights, cam, n, seed, 64)  # either face
        _oracle_cache[key] = (r, c, seen)
    return _oracle_cache[key]


@pytest.mark.parametrize("kind,w,h,n", [("solid", 16, 12, 4), ("solid", 37, 29, 1), ("solid", 40, 30, 4),
                                        ("checker", 40, 30, 4), ("flipped", 16, 12, 4)])
def test_emission_and_coverage_match_oracle(rt, oracle, gpu, kind, w, h, n):
    seed = 3
    t, cam, world, lights, _ = black_cornell(rt, kind)
    shape(cam, w, h, n)
    with rt.Scene(t, world, lights) as sc:
        g = sc.render_aov(cam, n_samples=n, seed=seed, emit=True)
    r, c, seen = oracle_side(rt, oracle, kind, w, h, n, seed)
    assert seen.sum() > 0, "the light is in view"
    gk = np.rint(g["coverage"].astype(float) * n).astype(int)
    fork, fork32 = gk != c[64], c[32] != c[64]
    print(f"{kind} {w}x{h} n={n}: light samples {int(c[64].sum())}, fork pixels gpu {int(fork.sum())} "
          f"fp32 twin {int(fork32.sum())} of {w * h}")
    assert fork32.mean() <= FORK_CAP, "the fp32 oracle twin alone exceeds the fork cap"
    assert (fork | fork32).mean() <= FORK_CAP, (int(fork.sum()), int(fork32.sum()), w * h)
    ok = ~(fork | fork32)
    assert np.array_equal(g["coverage"][ok], (c[64].astype(np.float32) / np.float32(n))[ok])
    scale = max(1.0, float(np.abs(r[64][ok]).max()))
    floor = scale * 2.0 ** -23
    eo = float(np.abs(r[32][ok] - r[64][ok]).max())
    eg = float(np.abs(g["emission"].astype(float)[ok] - r[64][ok]).max())
    print(f"emission: gpu err {eg:.3e} fp32-oracle err {eo:.3e} floor {floor:.2e}")
    assert eg <= max(4 * eo, floor), (eg, eo, floor)
    if kind == "flipped":  # the back of a one-sided light: nothing emitted, nothing covered
        assert c[64].sum() == 0 and (g["coverage"] == 0).all() and (g["emission"] == 0).all()
        assert np.array_equal(g["surface_albedo"], g["albedo"])  # a back-facing light: albedo 0, as now
    else:
        assert c[64].sum() > 0 and (g["emission"] > 0).any()
    if kind == "checker":  # both cell colours are seen (their clamped sums differ)
        lit = g["coverage"] > 0
        per_sample = g["emission"][lit] / g["coverage"][lit][:, None]
        assert len(np.unique(np.round(per_sample, 3), axis=0)) >= 2


def _close(a, b):
    """tests/test_aov_gpu.py test_bvh2_and_bvh4_by_knob's bars: the same closest hits in another
    test order: coverage as material (equal), the colours as depth (rtol 1e-5) and normal (atol 1e-6)"""
    assert np.array_equal(a["coverage"], b["coverage"])
    assert np.array_equal(a["material"], b["material"])
    for k in ("emission", "surface_albedo", "albedo"):
        assert np.allclose(a[k], b[k], rtol=1e-5, atol=1e-6), k


def test_row_share(rt, gpu):
    """rank 1 of 3: the rows of rt_render's partition, bit for bit"""
    t, cam, wd, l = rt.demo_scene("cornell")
    shape(cam, 40, 30, 4)
    with rt.Scene(t, wd, l) as sc:
        full = sc.render_aov(cam, n_samples=4, seed=3, emit=True)
        part = sc.render_aov(cam, n_samples=4, seed=3, rank=1, nranks=3, emit=True)
    assert part["coverage"].shape == (10, 40) and part["coverage"].max() > 0
    for k in EMIT + ("albedo", "normal", "depth", "material"):
        assert np.array_equal(full[k][1::3].view(np.uint32), part[k].view(np.uint32)), k


def test_bvh2_and_bvh4_by_knob(rt, gpu, tune):
    t, cam, wd, l = rt.demo_scene("cornell")
    shape(cam, 40, 30, 4)
    res = {}
    for knob in (None, "2", "4"):
        if knob:
            tune("RT_TREE", knob)
        with rt.Scene(t, wd, l) as sc:
            res[knob] = sc.render_aov(cam, n_samples=4, seed=3, emit=True)
    assert [res[k]["stats"]["tree_width"] for k in (None, "2", "4")] == [0, 2, 4]
    assert res[None]["coverage"].max() == 1.0
    for k in ("2", "4"):
        _close(res[k], res[None])


def test_compressed_bvh4_sphere_light(rt, gpu, tune):
    """book1 without defocus (a field of spheres under a sphere sun, its tree read through
    L1/L2): the compressed BVH4 by default, the 128-B nodes with RT_QBVH=0; both give the
    split buffers consistent with their own albedo, and agree with each other"""
    t, cam, wd, l = rt.demo_scene("book1")
    cam.DefocusAngle = 0.0
    cam.VerticalFOV = 100.0  # from the horizon's spheres up to the sun (radius 50 at (0, 100, 0))
    cam.PositionCamera((13, 2, 3), (0, 15, 0), (0, 1, 0))
    shape(cam, 32, 24, 4)
    res = {}
    for knob in ("1", "0"):
        tune("RT_QBVH", knob)
        with rt.Scene(t, wd, l) as sc:
            res[knob] = sc.render_aov(cam, n_samples=4, seed=3, emit=True)
    assert [res[k]["stats"]["tree_width"] for k in ("1", "0")] == [5, 4]
    g = res["1"]
    assert g["coverage"].max() == 1.0 and ((g["coverage"] > 0) & (g["coverage"] < 1)).any()
    lit = g["coverage"] == 1.0
    assert (g["surface_albedo"][lit] == 0).all() and (g["emission"][lit] > 0).all()
    assert (g["emission"][lit] == 5.0).all()  # the sun's (5, 5, 5), above MaxContribution: not clamped
    assert np.array_equal(g["surface_albedo"][g["coverage"] == 0], g["albedo"][g["coverage"] == 0])
    _close(res["0"], res["1"])
