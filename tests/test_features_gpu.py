"""Per-feature GPU-vs-oracle parity: one small scene per reference feature.

Tolerance: >= 99.5 % of linear-RGB channels within
2^-10 * max(1, |ref|) and of 8-bit outputs equal, for every feature scene (round 6: the
`cluster` scene renders at 64 x 64 x 32 and no longer needs its own bar; measured 8-bit
equality 0.9990 fused and wavefront, profiles/r6_parity_final.jsonl).  The oracle's fp32
twin (the reference's algorithm evaluated in float) is rendered on the same pixels and
logged next to the GPU's numbers (PARITY_LOG) for information only; it sets no bar.
"""
import os

import pytest

from tests import scenes
from tests.parity import compare, p1_bar

pytestmark = pytest.mark.gpu
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


@pytest.mark.parametrize("mode", ["fused", "wavefront"])
@pytest.mark.parametrize("name", scenes.FEATURES)
def test_feature_parity(rt, oracle, gpu, name, mode):
    t, cam, w, l = scenes.build(rt, name, ASSETS)
    with rt.Scene(t, w, l) as sc:
        img, st = sc.render(cam, seed=11, mode=mode)
    ref, ost = oracle.render(t, w, l, cam, seed=11, threads=8)
    m = compare(img, ref)
    # the fp32 floor: the oracle's fp32 twin (the reference's algorithm in float)
    # against its fp64 path, logged next to the GPU's numbers (PARITY_LOG)
    ref32, _ = oracle.render(t, w, l, cam, seed=11, threads=8, precision=32)
    m32 = compare(ref32, ref, label="fp32_oracle")
    print(name, mode, m, m32, st["segments"], ost["segments"])
    assert st["samples"] == ost["samples"]
    assert abs(st["segments"] - ost["segments"]) <= 0.01 * ost["segments"] + 10
    assert m["frac_close"] >= p1_bar(name, "frac_close"), (m, m32)
    assert m["q_equal"] >= p1_bar(name, "q_equal"), (m, m32)


@pytest.mark.parametrize("tables", [1, 3])
def test_noise_tables_kernel_choice(rt, oracle, gpu, tables):
    """Feature-set kernels read perlin table 0 from LDS only (rt_shade.h LdsPerlin); a
    scene whose reachable noise textures use other tables runs the all-features kernel
    (generic table pointers).  Both match the oracle."""
    t = rt.Tree(9)
    world, lights = scenes._room(t)
    for i, (sc_, var) in enumerate(((0.2, rt.RT_NOISE_MARBLE), (4, rt.RT_NOISE_TURBULENT),
                                    (4, rt.RT_NOISE_PERLIN))[:tables]):
        t.add(world, t.sphere((-3 + 3 * i, 1, 0), 1, t.lambertian(t.noise(sc_, var))))
    cam = scenes._cam(rt, (0, 3, -9), (0, 2, 0))
    with rt.Scene(t, world, lights) as sc:
        img, st = sc.render(cam, seed=5)
    ref, _ = oracle.render(t, world, lights, cam, seed=5, threads=8)
    assert (st["kernel_features"] == rt.RT_FT_ALL) == (tables > 1), st["kernel_features"]
    m = compare(img, ref)
    # measured 0.9971 / 1.0 (profiles/r3_parity_v5.jsonl)
    assert m["frac_close"] >= 0.995, m
    assert m["q_equal"] >= 0.995, m


def test_box_leaves_match_per_quad_faces(rt, oracle, gpu, tune):
    """Box leaves (one slab test per NewBox, rt_kernels.h hit_box_rec) against the same
    scene built with the six quads as leaves (RT_BOX_LEAVES=0): the two differ only
    where the slab and the quad tests round differently at box edges, and both meet P1
    against the oracle.  Includes image-textured faces (alpha, beta derived in
    shade_core from the face's quad record) and rotated boxes."""
    t, cam, w, l = scenes.build(rt, "box_leaves", ASSETS)
    with rt.Scene(t, w, l) as sc:
        assert sc.info()["features"] & rt.RT_FT_BOX
        on, st_on = sc.render(cam, seed=4)
    tune("RT_BOX_LEAVES", "0")
    with rt.Scene(t, w, l) as sc:
        assert not sc.info()["features"] & rt.RT_FT_BOX
        off, st_off = sc.render(cam, seed=4)
    ref, ost = oracle.render(t, w, l, cam, seed=4, threads=8)
    m_on, m_off, m_pair = compare(on, ref), compare(off, ref), compare(on, off)
    print(m_on, m_off, m_pair)
    for m in (m_on, m_off):
        assert m["frac_close"] >= p1_bar("box_leaves", "frac_close"), m
        assert m["q_equal"] >= p1_bar("box_leaves", "q_equal"), m
    assert m_pair["q_equal"] >= 0.995, m_pair
    assert abs(st_on["segments"] - st_off["segments"]) <= 0.01 * st_off["segments"]
