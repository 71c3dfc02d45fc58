"""The specular feature pass (rt_render_aov_spec, rt_aov.hip k_aov<.., SPEC>)
against the CPU oracle, the first-hit pass, the render's own trace and itself.

Checker: pyoracle.trace(pixel, sample) with the camera's own MaxDepth records every vertex of the
sample's path in fp64 (and in fp32, the twin).  `walk` follows those records by rt_abi.h's chain
rule with tests/test_aov_gpu.py's Flat.evaluate: while vertex k < K is a dielectric or a metal of
fuzz <= max_fuzz whose scattered direction (the next record's) leaves its surface, its albedo is
multiplied into T and its segment added to the depth; the terminal gives T * albedo, its normal,
the summed depth (0 on a miss), its kind, and k is the sample's `bounces`.

Bars, in run_scene's form.  depth / normal / albedo: the GPU's max error against the fp64 walk is
at most 4 x the twin's on the same pixels, with a floor of one fp32 ulp of the plane's scale;
material and bounces equal outside fork pixels.  A fork pixel has a sample whose chain length, or
whose primitive at a chain vertex, is not the fp64 oracle's; on the GPU side that is read from the
per-sample depth differences (Flat.prim_at) where the sample passed no vertex, and from the
per-sample chain length and sample 0's terminal material otherwise.  Forks are capped at 2 % of
the pixels (twice the first-hit test's: a chain takes up to eight more hit and coin decisions) and
the twin is held to the same cap.  Twin fork pixels measured on the CPU for these cases, of 192:
sphere_field 1, book1 0, quads 0, sphere_field max_fuzz 1 -> 1, book1 max_fuzz 1 -> 1."""
import copy

import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests import scenes
from tests.test_aov_gpu import Flat, _shape, sphere_field

pytestmark = pytest.mark.gpu

PLANES = ("albedo", "normal", "depth", "material")
N, SEED, W, H = 4, 3, 16, 12


def _build(rt, name):
    if name == "sphere_field":
        t, cam, wd, l = sphere_field(rt)
    else:
        t, cam, wd, l = rt.demo_scene(name)
    if name == "book1":
        cam.DefocusAngle = 0.0
    return t, _shape(cam, W, H), wd, l


def _mat_of(flat, bid):
    ns, nq = len(flat.sph_r), len(flat.q_mat)
    return int(flat.sph_mat[bid] if bid < ns else flat.q_mat[bid - ns] if bid < ns + nq else flat.t_mat[bid - ns - nq])


def walk(flat, recs, bg, K, max_fuzz):
    """one sample's trace records -> (k, prims of vertices 0 .. k, kind, normal, albedo, depth, solid)"""
    T, dsum, k, prims, solid = np.ones(3), 0.0, 0, [], True
    while True:
        bid, kind, n, alb, depth, sol = flat.evaluate(recs[k], bg)
        prims.append(bid)
        solid = solid and sol
        if kind < 0:
            return k, prims, -1, np.zeros(3), T * alb, 0.0, solid
        fuzz = float(flat.mats[_mat_of(flat, bid)]["fuzz"]) if kind == 1 else 0.0
        if k < K and (kind == 2 or (kind == 1 and fuzz <= max_fuzz)):
            s = recs[k + 1][4:7].astype(float)  # the scattered direction: the next segment's
            if kind == 2 or float(np.dot(s, n)) > 0.0:
                T, dsum, k = T * alb, dsum + depth, k + 1
                continue
        return k, prims, kind, n, T * alb, dsum + depth, solid


_TRACES = {}


def traces(rt, oracle, name):
    """every (pixel, sample)'s records in fp64 and in fp32, once per scene"""
    if name not in _TRACES:
        t, cam, wd, l = _build(rt, name)
        out = {}
        for prec in (64, 32):
            for pix in range(W * H):
                for j in range(N):
                    out[(prec, pix, j)] = np.array(oracle.trace(t, wd, l, cam, pix, j, seed=SEED, precision=prec))
        _TRACES[name] = (t, cam, wd, l, Flat(t, wd), out)
    return _TRACES[name]


@pytest.mark.parametrize("name,max_fuzz", [("sphere_field", 0.0), ("book1", 0.0), ("quads", 0.0),
                                           ("sphere_field", 1.0), ("book1", 1.0)])
def test_chain_planes_match_oracle(rt, oracle, gpu, name, max_fuzz):
    t, cam, wd, l, flat, recs = traces(rt, oracle, name)
    assert flat.media == 0
    bg = tuple(cam.Background)
    K = max(0, min(8, cam.derived().max_depth - 1))
    with rt.Scene(t, wd, l) as sc:
        got = [sc.render_aov(cam, n_samples=k, seed=SEED, specular=True, max_fuzz=max_fuzz) for k in range(1, N + 1)]
    g = got[-1]
    fork, fork32 = np.zeros((H, W), bool), np.zeros((H, W), bool)
    x64 = {k: np.zeros(g[k].shape) for k in ("albedo", "normal", "depth")}
    x32 = {k: np.zeros(g[k].shape) for k in ("albedo", "normal", "depth")}
    solid = np.ones((H, W), bool)
    mat0, bsum, longest = np.zeros((H, W), int), np.zeros((H, W)), 0
    for y in range(H):
        for x in range(W):
            for j in range(N):
                r64 = recs[(64, y * W + x, j)]
                a, b = walk(flat, r64, bg, K, max_fuzz), walk(flat, recs[(32, y * W + x, j)], bg, K, max_fuzz)
                fork32[y, x] |= b[0] != a[0] or b[1] != a[1]
                prev = lambda key: j * float(got[j - 1][key][y, x]) if j else 0.0  # noqa: E731
                bj = (j + 1) * float(got[j]["bounces"][y, x]) - prev("bounces")
                dj = (j + 1) * float(got[j]["depth"][y, x]) - prev("depth")
                if round(bj) != a[0] or abs(bj - round(bj)) > 1e-4:
                    fork[y, x] = True
                elif j == 0 and int(g["material"][y, x]) != a[2]:
                    fork[y, x] = True
                elif a[0] == 0:  # no vertex passed: the first-hit test's primitive check
                    eps = 1e-5 * (j + 1) * max(1.0, float(got[j]["depth"][y, x]))
                    gp = -1 if abs(dj) <= eps else (-3 if dj < 0.0 else flat.prim_at(
                        r64[0][0:3].astype(float), r64[0][4:7].astype(float), float(r64[0][3]), dj))
                    fork[y, x] |= gp != a[1][0]
                solid[y, x] &= a[6] and b[6]
                for key, idx in (("normal", 3), ("albedo", 4), ("depth", 5)):
                    x64[key][y, x] += np.asarray(a[idx]) / N
                    x32[key][y, x] += np.asarray(b[idx]) / N
                bsum[y, x] += a[0]
                longest = max(longest, a[0])
                if j == 0:
                    mat0[y, x] = a[2]
    npx = W * H
    chains = int((bsum > 0).sum())
    print(f"{name} max_fuzz {max_fuzz}: fork pixels gpu {fork.sum()} fp32 twin {fork32.sum()} of {npx}; "
          f"{chains} pixels pass a specular vertex, longest chain {longest}")
    assert 25 <= chains <= 100, "the case's coverage of chains"
    if name == "sphere_field":
        assert longest == K == 8, "the max_bounces terminal is exercised"
    assert fork32.mean() <= 0.02, "the fp32 oracle twin alone exceeds the fork cap"
    assert fork.mean() <= 0.02, (fork.sum(), npx)
    ok = ~fork
    assert np.array_equal(g["material"][ok], mat0[ok])
    assert np.array_equal(g["bounces"][ok], (bsum / N).astype(np.float32)[ok])
    assert g["stats"]["segments"] == npx * N + int(round(float(g["bounces"].astype(np.float64).sum()) * N))
    for key in ("depth", "normal", "albedo"):
        m = ok & solid if key == "albedo" else ok
        mt = m & ~fork32
        scale = max(1.0, float(np.abs(x64[key][m]).max())) if m.any() else 1.0
        floor = scale * 2.0 ** -23
        eg = float(np.abs(g[key][m] - x64[key][m]).max()) if m.any() else 0.0
        eo = float(np.abs(x32[key][mt] - x64[key][mt]).max()) if mt.any() else 0.0
        print(f"{name} max_fuzz {max_fuzz} {key}: gpu err {eg:.3e} fp32-oracle err {eo:.3e} "
              f"ratio {eg / max(eo, 1e-30):.2f} floor {floor:.2e}")
        assert eg <= max(4 * eo, floor), (key, eg, eo, floor)


@pytest.mark.parametrize("name", ["cornell", "sphere_field", "book1", "quads"])
def test_identity_where_nothing_is_specular(rt, gpu, name):
    t, cam, wd, l = _build(rt, name)
    with rt.Scene(t, wd, l) as sc:
        first = sc.render_aov(cam, n_samples=N, seed=SEED)
        spec = sc.render_aov(cam, n_samples=N, seed=SEED, specular=True)
    same = spec["bounces"] == 0
    if name == "cornell":
        assert same.all()
        assert spec["stats"]["segments"] == first["stats"]["segments"]
    else:
        assert same.any() and not same.all()
    for k in PLANES:
        assert np.array_equal(first[k][same].view(np.uint32), spec[k][same].view(np.uint32)), k


def test_max_bounces_is_capped_by_max_depth(rt, gpu):
    t, cam, wd, l = _build(rt, "sphere_field")
    cam.MaxDepth = 4
    with rt.Scene(t, wd, l) as sc:
        a = sc.render_aov(cam, n_samples=N, seed=SEED, specular=True, max_bounces=3)
        b = sc.render_aov(cam, n_samples=N, seed=SEED, specular=True, max_bounces=20)
        c = sc.render_aov(cam, n_samples=N, seed=SEED, specular=True, max_bounces=2)
    for k in PLANES + ("bounces",):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert a["bounces"].max() <= 3.0 and c["bounces"].max() <= 2.0
    assert not np.array_equal(a["bounces"], c["bounces"]), "chains reach vertex 3 in this scene"


def test_same_path_as_the_render(rt, oracle, gpu):
    """8 pixels of sphere_field whose sample 0 passes a specular vertex: the fused render's trace of
    (pixel, sample 0), walked by the chain rule through Flat.identify, has the feature pass's chain
    length and the material plane's kind at the terminal.  The feature pass exports no primitive
    id, so the primitive at every chain vertex is held against the fp64 walk of the same sample,
    which test_chain_planes_match_oracle holds the feature pass to (no fork pixel in this case).
    Discrete only: the two fp32 texts may round their rays differently.  The walk below is the
    chain rule at max_fuzz 0: a followed metal has fuzz 0, reflects off the normal facing its ray
    and so never meets the absorbing terminal (dot(s, n) > 0 always)."""
    t, cam, wd, l, flat, recs = traces(rt, oracle, "sphere_field")
    K = max(0, min(8, cam.derived().max_depth - 1))
    with rt.Scene(t, wd, l) as sc:
        a = sc.render_aov(cam, n_samples=1, seed=SEED, specular=True)
        ys, xs = np.nonzero(a["bounces"] >= 1)
        assert len(ys) >= 8
        pick = np.linspace(0, len(ys) - 1, 8).astype(int)
        for y, x in zip(ys[pick], xs[pick]):
            _, st = sc.render(cam, seed=SEED, trace=(int(y) * W + int(x), 0), mode="fused")
            tr = st["trace"]
            k, prims = 0, []
            while True:
                v = tr[k]
                ref = v[11:12].view(np.uint32)[0]
                if ref == 0xFFFFFFFF:
                    kind = -1
                    prims.append(-1)
                    break
                o, d, tm = v[0:3].astype(float), v[4:7].astype(float), float(v[3])
                bid = flat.identify(o + float(v[8]) * d, tm, float(v[8]) * float(np.linalg.norm(d)))[0]
                assert bid >= 0
                prims.append(bid)
                M = flat.mats[_mat_of(flat, bid)]
                kind = int(M["kind"])
                if k < K and (kind == 2 or (kind == 1 and float(M["fuzz"]) <= 0.0)):
                    k += 1
                    continue
                break
            assert k == int(a["bounces"][y, x]), (y, x)
            assert kind == int(a["material"][y, x]), (y, x)
            want = walk(flat, recs[(64, int(y) * W + int(x), 0)], tuple(cam.Background), K, 0.0)
            assert (k, prims) == (want[0], want[1]), (y, x)


def test_determinism_and_entries(rt, gpu):
    t, cam, wd, l = _build(rt, "sphere_field")
    keys = PLANES + ("bounces",)
    with rt.Scene(t, wd, l) as sc:
        a = sc.render_aov(cam, n_samples=N, seed=SEED, specular=True)
        b = sc.render_aov(cam, n_samples=N, seed=SEED, specular=True)
        part = sc.render_aov(cam, n_samples=N, seed=SEED, specular=True, rank=1, nranks=3)
        dev = {k: torch.zeros(a[k].shape, dtype=torch.int32 if k == "material" else torch.float32, device="cuda")
               for k in keys}
        st = sc.render_aov_device(cam, n_samples=N, seed=SEED, specular=True, **{k: dev[k].data_ptr() for k in keys})
        torch.cuda.synchronize()
    assert st["segments"] == a["stats"]["segments"] > W * H * N
    for k in keys:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert np.array_equal(a[k].view(np.uint32), dev[k].cpu().numpy().view(np.uint32)), k
        assert np.array_equal(a[k][1::3], part[k]), k


def mirror_and_checker(rt):
    """a fuzz-0 metal quad of albedo 0.9 facing a checker-textured Lambertian wall, lit from above"""
    t = rt.Tree(5)
    world = t.list()
    chk = t.lambertian(t.checker(0.8, t.solid(0.1, 0.1, 0.6), t.solid(0.9, 0.9, 0.9)))
    t.add(world, t.quad((-6, 0, -6), (12, 0, 0), (0, 8, 0), chk))                          # the wall, z = -6
    t.add(world, t.quad((-6, 0, -6), (12, 0, 0), (0, 0, 12), t.lambertian((0.6, 0.6, 0.6))))  # the floor
    t.add(world, t.quad((-3, 0.5, 4), (6, 0, 0), (0, 5, 0), t.metal((0.9, 0.9, 0.9), 0.0)))  # the mirror, z = 4
    light = t.quad((-3, 7.9, -4), (6, 0, 0), (0, 0, 6), t.light((6, 6, 6)))
    t.add(world, light)
    cam = scenes._cam(rt, (0, 3, -2), (0, 3, 4), vfov=60.0, bg=(0.05, 0.05, 0.05))
    return t, cam, world, t.list(light)


def test_specular_guides_denoise_a_reflection_better(rt, gpu):
    """The point of the feature: rt.denoise of a 4-spp render guided by the specular planes against
    the same filter guided by the first-hit planes, both against 1024 spp over the pixels with
    bounces > 0.  Both errors are printed.  The ordering (specular-guided lower) did NOT hold on an
    MI355X and is not asserted: MSE over the 394 mirror pixels unfiltered 4.0400e-02, first-hit
    guides 3.6549e-02, specular guides 3.7908e-02.  The scene is as first
    written: it was not tuned towards either outcome."""
    t, cam, wd, l = mirror_and_checker(rt)
    _shape(cam, 32, 24, spp=4)
    ref_cam = _shape(copy.copy(cam), 32, 24, spp=1024)
    with rt.Scene(t, wd, l) as sc:
        img, _ = sc.render(cam, seed=SEED)
        ref, _ = sc.render(ref_cam, seed=SEED + 1)
        first = sc.render_aov(cam, n_samples=4, seed=SEED)
        spec = sc.render_aov(cam, n_samples=4, seed=SEED, specular=True)
    m = spec["bounces"] > 0
    assert m.sum() >= 50, "the mirror covers part of the image"
    img = np.ascontiguousarray(img, np.float32)
    e_first = float(((rt.denoise(img, first) - ref)[m] ** 2).mean())
    e_spec = float(((rt.denoise(img, spec) - ref)[m] ** 2).mean())
    e_none = float(((img - ref)[m] ** 2).mean())
    print(f"MSE over {int(m.sum())} mirror pixels: unfiltered {e_none:.4e} first-hit guides {e_first:.4e} "
          f"specular guides {e_spec:.4e}")
    assert np.isfinite([e_none, e_first, e_spec]).all()
