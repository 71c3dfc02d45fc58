"""rt_bvh_build_boxes (a tree over caller-supplied boxes) with the host builder, and the
PLOC reference of tests/ploc_ref.py checked against itself.  CPU-only: the device builder
is compared with the reference in test_bvh_ploc_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import ploc_ref as P
from tests.test_scene import bvh4_tree_invariants, bvh_tree_invariants


def tree_invariants(out, boxes, check_boxes=True):
    """Leaf-once and containment, BVH2 and BVH4, of a build_bvh_boxes-shaped result."""
    refs = out["refs"]
    assert sorted(refs.tolist()) == list(range(len(boxes))), "refs is a permutation"
    bounds = np.asarray(boxes, np.float32)[refs.astype(np.int64)]
    bvh_tree_invariants(out["nodes"], refs, out["root"], bounds, len(boxes), out["max_leaf"],
                        boxes=check_boxes)
    bvh4_tree_invariants(out["nodes4"], out["root4"], bounds, boxes=check_boxes)


# ---- the reference checks itself --------------------------------------------------------
@pytest.mark.parametrize("top", [1, 64, 1 << 30])
@pytest.mark.parametrize("make,n", [(P.lattice_boxes, 1), (P.lattice_boxes, 2), (P.lattice_boxes, 257),
                                    (P.lattice_boxes, 700), (P.random_boxes, 500)])
def test_reference_trees_are_valid(make, n, top):
    boxes = make(n, seed=n)
    out, tree = P.build(boxes, P.morton_order(boxes), top)
    tree_invariants(out, boxes)
    assert len(out["nodes"]) == n - 1 and tree.forced == 0
    assert n == 1 or P.sah_cost(out["nodes"]) == pytest.approx(P.tree_sah_cost(tree), rel=1e-12)


def brute_merges(lo, hi):
    """All mutual nearest pairs merge, every cluster sees every other: [(left id, right id)]
    of the nodes made, in order.  Written on its own, a cluster at a time."""
    n = len(lo)
    cl = [(i, lo[i], hi[i]) for i in range(n)]
    merges = []

    def area(a, b):
        d = np.maximum(a[2], b[2]) - np.minimum(a[1], b[1])
        return np.float32(d[0] * d[1] + d[1] * d[2] + d[2] * d[0])

    while len(cl) > 1:
        m = len(cl)
        nn = [min((j for j in range(m) if j != i), key=lambda j: (area(cl[i], cl[j]), j)) for i in range(m)]
        nxt = []
        for i in range(m):
            j = nn[i]
            if nn[j] != i:
                nxt.append(cl[i])
            elif i < j:
                merges.append((cl[i][0], cl[j][0]))
                nxt.append((n + len(merges) - 1, np.minimum(cl[i][1], cl[j][1]), np.maximum(cl[i][2], cl[j][2])))
        cl = nxt
    return merges


@pytest.mark.parametrize("make", [P.lattice_boxes, P.random_boxes])
@pytest.mark.parametrize("n", [2, 3, 5, 9, 16, 17])
def test_reference_replay_equals_brute_force_inside_the_window(make, n):
    """n <= 17: the window of 16 positions on each side holds every cluster."""
    for seed in range(4):
        boxes = make(n, seed=100 * n + seed)
        order = P.morton_order(boxes)
        tree = P.Tree(boxes, order)
        assert len(P.ploc(tree, 1)) == 1
        got = list(zip(tree.left[n:].tolist(), tree.right[n:].tolist()))
        assert got == brute_merges(tree.lo[:n], tree.hi[:n]), (n, seed)


def test_reference_overflowing_areas_take_the_forced_pairs():
    """Boxes whose merged half-area overflows fp32: no area compares less than +inf, no pair
    is mutual, and every second iteration pairs positions 2k, 2k+1."""
    boxes = P.lattice_boxes(40, seed=5, scale=2.0 ** 64)
    out, tree = P.build(boxes, P.morton_order(boxes), 1)
    assert tree.forced >= 5 and tree.iterations == 2 * tree.forced
    tree_invariants(out, boxes)
    assert list(zip(tree.left[40:60].tolist(), tree.right[40:60].tolist())) == [(2 * k, 2 * k + 1) for k in range(20)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_order_case_flags_few_prims(seed):
    """The curve-order test on random floats may leave out at most 2 % of the prims; the
    reference alone flags about 0.3 % at these seeds."""
    _, flagged = P.prefix_codes(P.random_boxes(5000, seed))
    assert flagged.mean() < 0.01


def test_curve_lattice_is_what_it_says():
    boxes = P.curve_boxes(5000, seed=1)
    c = P.centroids(boxes).astype(np.float64)
    k = c * 2.0 ** 18
    assert (k == np.round(k)).all() and (c.min(0) == 0).all() and (c.max(0) == 8).all()
    q, _ = P.quantized(boxes)
    assert (q == np.minimum(k, 2 ** 21 - 1)).all() and (q.max(0) == 2 ** 21 - 1).all()
    codes = P.interleave(q)
    assert len(np.unique(codes)) < len(codes), "repeated codes: stability is exercised"
    assert int(np.bitwise_or.reduce(codes)) == (1 << 63) - 1, "all 63 bits occur"
    order = P.morton_order(boxes).astype(np.int64)
    same = codes[order][1:] == codes[order][:-1]
    assert (np.diff(order)[same] > 0).all()


# ---- the host builder through rt_bvh_build_boxes ------------------------------------------
@pytest.mark.parametrize("make,n", [(P.lattice_boxes, 5), (P.lattice_boxes, 700), (P.random_boxes, 1000),
                                    (P.lattice_boxes, 2), (P.lattice_boxes, 1)])
def test_host_builder_on_boxes(rt, make, n):
    boxes = make(n, seed=7)
    out = rt.build_bvh_boxes(boxes, 0)
    tree_invariants(out, boxes)
    again = rt.build_bvh_boxes(boxes, 0)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    assert out["bvh_depth"] >= (n > 4) and 1 <= out["max_leaf"] <= 16  # up to 4 prims: one leaf


def test_host_builder_on_no_boxes(rt):
    out = rt.build_bvh_boxes(np.zeros((0, 6), np.float32), 0)
    assert out["root"] == 0xFFFFFFFF and len(out["nodes"]) == len(out["nodes4"]) == len(out["refs"]) == 0


def test_build_boxes_argument_errors(rt):
    boxes = P.lattice_boxes(8, seed=1)
    with pytest.raises(rt.RtError) as e:
        rt.build_bvh_boxes(boxes, 2)
    assert e.value.code == -1 and "rt_bvh_build_boxes" in rt.lib().rt_last_error().decode()
    with pytest.raises(ValueError):
        rt.build_bvh_boxes(boxes[:, :5], 0)
    nn = C.c_int32()
    z = [None, C.byref(nn), None, None, None, None, None, None, None, None]
    assert rt.lib().rt_bvh_build_boxes(None, 8, 0, *z) == -1  # boxes missing
    assert rt.lib().rt_bvh_build_boxes(boxes.ctypes.data, -1, 0, *z) == -1
    if rt.device_count() <= 0:
        with pytest.raises(rt.RtError) as e:
            rt.build_bvh_boxes(boxes, 1)
        assert e.value.code == -3  # RT_ERR_DEVICE
    else:
        tree_invariants(rt.build_bvh_boxes(boxes, 1), boxes)


def test_build_boxes_size_query(rt):
    """NULL buffers return the counts; buffers of exactly those sizes receive the tree."""
    boxes = P.random_boxes(300, seed=3)
    want = rt.build_bvh_boxes(boxes, 0)
    nn, nr, n4, depth, leaf = (C.c_int32(-1) for _ in range(5))
    root, root4 = C.c_uint32(), C.c_uint32()
    L = rt.lib()
    assert L.rt_bvh_build_boxes(boxes.ctypes.data, 300, 0, None, C.byref(nn), None, C.byref(nr),
                                C.byref(root), None, C.byref(n4), C.byref(root4), C.byref(depth),
                                C.byref(leaf)) == 0
    assert (nn.value, nr.value, n4.value) == (len(want["nodes"]), 300, len(want["nodes4"]))
    assert (root.value, root4.value, depth.value, leaf.value) == (
        want["root"], want["root4"], want["bvh_depth"], want["max_leaf"])
    nodes, refs = np.zeros((nn.value, 16), np.float32), np.zeros(nr.value, np.uint32)
    nodes4 = np.zeros((n4.value, 32), np.uint32)
    assert L.rt_bvh_build_boxes(boxes.ctypes.data, 300, 0, nodes.ctypes.data, None, refs.ctypes.data,
                                None, None, nodes4.ctypes.data, None, None, None, None) == 0
    assert np.array_equal(nodes, want["nodes"]) and np.array_equal(refs, want["refs"])
    assert np.array_equal(nodes4, want["nodes4"])
