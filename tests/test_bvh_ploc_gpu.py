"""The device BVH builder's clustering loop (rt_build.hip: k_bounds, k_morton, k_nn, k_flags,
k_emit, the scans between them, the SAH top and the layout) against the plain restatement in
tests/ploc_ref.py.  RT_BVH_TOP brings the loop, which production scenes only enter above
16,384 clusters, down to a few boxes; rt_bvh_build_boxes feeds the builder boxes on an exact
lattice, for which the float64 reference is bit-exact."""
import numpy as np
import pytest

from tests import ploc_ref as P
from tests.parity import compare
from tests.test_bvh_boxes import tree_invariants
from tests.test_scene import bvh_invariants, qbvh_invariants

pytestmark = pytest.mark.gpu

QUALITY_BOUND = 1e-3  # test_ploc_tree_quality_against_replay

TOPS = [1, 64, 1 << 30]  # pure PLOC, PLOC + SAH top, SAH top only


def assert_same_tree(dev, ref):
    assert dev["root"] == ref["root"] and dev["root4"] == ref["root4"]
    assert dev["bvh_depth"] == ref["bvh_depth"]
    for k in ("nodes", "nodes4"):
        a, b = dev[k].view(np.uint32), ref[k].view(np.uint32)
        assert a.shape == b.shape, k
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (k, len(bad), bad[:4].tolist())


# ---- a. exact replay on an integer lattice ------------------------------------------------
@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("n", [2, 3, 17, 33, 256, 257, 700, 3000])
def test_device_tree_equals_replay_on_lattice(rt, gpu, tune, n, top):
    """2, 3: the smallest trees; 17, 33: around the radius; 256, 257: around one block; 700:
    three blocks with a ragged last one (the LDS window crosses two block boundaries); 3000:
    many iterations.  The leaf order is the device's own (checked in the curve-order tests)."""
    boxes = P.lattice_boxes(n, seed=n)
    tune("RT_BVH_TOP", top)
    dev = rt.build_bvh_boxes(boxes, 1)
    assert sorted(dev["refs"].tolist()) == list(range(n))
    ref, tree = P.build(boxes, dev["refs"], top)
    assert tree.forced == 0
    assert_same_tree(dev, ref)
    assert dev["max_leaf"] == 1


@pytest.mark.parametrize("n,top", [(40, 1), (300, 1), (300, 64)])
def test_device_tree_equals_replay_when_areas_overflow(rt, gpu, tune, n, top):
    """The lattice scaled by 2^64: finite boxes, every merged half-area +inf in fp32.  No area
    compares less than +inf, k_nn finds no neighbour, no pair is mutual, and the next iteration
    is the `force` one (positions 2k, 2k+1 pair).  The replay says how often that happened."""
    boxes = P.lattice_boxes(n, seed=n, scale=2.0 ** 64)
    tune("RT_BVH_TOP", top)
    dev = rt.build_bvh_boxes(boxes, 1)
    ref, tree = P.build(boxes, dev["refs"], top)
    assert tree.forced >= 2
    assert_same_tree(dev, ref)
    tree_invariants(dev, boxes)


# ---- b. curve order ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [5000, 262144 + 256 + 77])
def test_curve_order_on_lattice(rt, gpu, n):
    """Centroids on k * 2^-18 with an extent of exactly 8: the quotient is exact (if dividing by
    a power of two is, under -fno-hip-fp32-correctly-rounded-divide-sqrt), all 63 code bits
    occur, t = 1.0 meets the clamp, equal codes must come out in input order.  The large size
    takes k_bounds' grid-stride branch and k_morton's 1,024 partials."""
    boxes = P.curve_boxes(n, seed=n)
    dev = rt.build_bvh_boxes(boxes, 1)
    want = P.morton_order(boxes)
    bad = np.flatnonzero(dev["refs"] != want)
    assert len(bad) == 0, (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_curve_order_on_random_floats(rt, gpu, seed):
    """The device's quotient may be 2 ulp off the correctly rounded one (0.25 in t * 2^21), so
    the comparison is on the 36-bit prefix of the code, without the prims whose prefix such an
    error could change (at most 2 %)."""
    boxes = P.random_boxes(5000, seed)
    dev = rt.build_bvh_boxes(boxes, 1)
    refs = dev["refs"].astype(np.int64)
    assert sorted(refs.tolist()) == list(range(5000))
    codes, flagged = P.prefix_codes(boxes)
    print("flagged share", flagged.mean())
    assert flagged.mean() <= 0.02
    along = codes[refs][~flagged[refs]]
    assert (along[1:] >= along[:-1]).all()


# ---- c. degenerate inputs: invariants only -----------------------------------------------
def _degenerate(kind, n):
    rng = np.random.default_rng(n)
    if kind == "identical":  # one merge per iteration
        return np.tile(np.array([[1, 2, 3, 2, 4, 6]], np.float32), (n, 1))
    if kind == "same_centroid":
        h = rng.uniform(0.1, 2.0, (n, 3))
        return np.concatenate([5 - h, 5 + h], axis=1).astype(np.float32)
    if kind == "flat_axis":
        b = P.random_boxes(n, seed=n)
        b[:, 2], b[:, 5] = 1.5, 1.5
        return b
    assert kind == "nan"
    b = P.lattice_boxes(n, seed=n)
    b[[1, 4, 7]] = np.nan
    return b


@pytest.mark.parametrize("kind,n", [("identical", 40), ("identical", 300), ("same_centroid", 300),
                                    ("flat_axis", 300), ("nan", 9)])
def test_degenerate_inputs_build_valid_trees(rt, gpu, tune, kind, n):
    """The build returns RT_OK inside its own iteration cap and every leaf is reached exactly
    once in the BVH2 and in the BVH4; boxes are checked for containment where they are numbers."""
    boxes = _degenerate(kind, n)
    tune("RT_BVH_TOP", 1)
    dev = rt.build_bvh_boxes(boxes, 1)  # raises unless RT_OK
    tree_invariants(dev, boxes, check_boxes=kind != "nan")
    assert len(dev["nodes"]) == n - 1


def test_device_builder_needs_two_boxes(rt, gpu):
    with pytest.raises(rt.RtError) as e:
        rt.build_bvh_boxes(P.lattice_boxes(1, seed=1), 1)
    assert e.value.code == -1


# ---- d. through scene creation, on real padded boxes ---------------------------------------
def _scene(rt, name):
    t, cam, w, l = rt.demo_scene(name)
    return t, cam, w, l, rt.Scene(t, w, l)


@pytest.mark.parametrize("top", [1, 64])
def test_scene_tree_invariants_with_ploc(rt, gpu, tune, top):
    tune("RT_BVH_BUILDER", "device")
    tune("RT_BVH_TOP", top)
    t, cam, w, l, sc = _scene(rt, "model:96x24")
    with sc:
        assert sc.info()["bvh_builder"] == 1
        nodes, refs, _ = bvh_invariants(sc)
        qbvh_invariants(sc)
        with rt.Scene(t, w, l) as again:
            n2, r2, _, _ = again.export_bvh()
    assert np.array_equal(nodes, n2) and np.array_equal(refs, r2), "device build is deterministic"


@pytest.mark.parametrize("top", [1, 64])
def test_ploc_tree_renders_like_host_tree(rt, gpu, tune, top):
    imgs, stats = [], []
    for builder in ("host", "device"):
        tune("RT_BVH_BUILDER", builder)
        tune("RT_BVH_TOP", top)
        t, cam, w, l, sc = _scene(rt, "model:256x32")
        cam.Width, cam.SamplesPerPixel = 64, 8
        with sc:
            img, st = sc.render(cam, seed=5)
            assert sc.info()["bvh_builder"] == (builder == "device")
        imgs.append(img)
        stats.append(st)
    m = compare(imgs[1], imgs[0])
    print(top, m, stats[0]["segments"], stats[1]["segments"])
    assert m["frac_close"] >= 0.9999 and m["q_equal"] >= 0.9999, m
    assert abs(stats[0]["segments"] - stats[1]["segments"]) <= 1e-5 * stats[0]["segments"] + 2


@pytest.mark.parametrize("top", [1, 64])
@pytest.mark.parametrize("name", ["model:96x24", "model:256x32"])
def test_ploc_tree_quality_against_replay(rt, gpu, tune, name, top):
    """sah_cost(device tree) / sah_cost(replay from the device's order and exported bounds).
    On real boxes the two trees may differ where two merged areas lie within fp32 rounding of
    each other (the kernels may contract d*d + d*d into FMAs, the replay rounds the float64 sum
    once).  Measured on an MI355X: model:96x24 top 1 and 64: 1.0000000000000002; model:256x32
    top 1: 1.0000000000000002, top 64: 0.9999999999999998 (the same trees, the sums taken in
    another order).  The bound is twice the largest deviation seen and not below 1e-3: 1e-3."""
    tune("RT_BVH_BUILDER", "device")
    tune("RT_BVH_TOP", top)
    t, cam, w, l, sc = _scene(rt, name)
    with sc:
        nodes, refs, root, bounds = sc.export_bvh()
    tree = P.Tree(bounds, np.arange(len(bounds)))
    cl = P.ploc(tree, top)
    if len(cl) > 1:
        P.sah_top(tree, cl)
    ratio = P.sah_cost(nodes) / P.tree_sah_cost(tree)
    print("sah ratio", name, top, repr(ratio))
    assert abs(ratio - 1) <= QUALITY_BOUND, ratio


