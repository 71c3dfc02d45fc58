"""A plain numpy restatement of the device BVH build (rt_build.hip), written from Meister &
Bittner's PLOC paper and the builder's comments: Morton order, the clustering loop, the SAH
top, the BVH2/BVH4 layout.  Box arithmetic is float64 on float32 inputs, codes and ids are
Python/numpy integers.  Two things are taken from the number format the kernels work in:
a merged half-area is rounded to float32 at the end (a no-op on the integer lattices the
exact tests use; it turns an fp32 overflow into +inf, which is what reaches the builder's
`force` step), and min/max ignore NaN as fminf/fmaxf do.

The tree every stage works on: nodes 0..n-1 are the leaves in curve order, inner nodes follow,
`lo`/`hi` [2n-1, 3] float64, `left`/`right` [2n-1] (-1 for leaves)."""
import sys

import numpy as np

R = 16  # search radius: clusters on each side
LEAF, EMPTY = 0x80000000, 0xFFFFFFFE


# ---- Morton codes ---------------------------------------------------------------------
def centroids(boxes):
    b = np.asarray(boxes, np.float32)
    return np.float32(0.5) * (b[:, :3] + b[:, 3:])  # float32, as the kernels compute it


def quantized(boxes):
    """(q int64 [n, 3], t float32 [n, 3]): the 21-bit cell of every centroid in the centroid
    bounds; t is the correctly rounded float32 quotient."""
    c = centroids(boxes)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mn, mx = np.fmin.reduce(c, axis=0), np.fmax.reduce(c, axis=0)
        ext = (mx - mn).astype(np.float32)
        t = np.where(ext > 0, (c - mn).astype(np.float32) / np.where(ext > 0, ext, np.float32(1)),
                     np.float32(0)).astype(np.float32)
        s = np.nan_to_num(t.astype(np.float64) * 2097152.0, nan=0.0)
    return np.clip(np.floor(s), 0, 2097151).astype(np.int64), t


def interleave(q):
    """63-bit code: bit b of x, y, z at 3b+2, 3b+1, 3b (x most significant)."""
    q = np.asarray(q, np.uint64)
    code = np.zeros(len(q), np.uint64)
    for b in range(21):
        for k in range(3):
            code |= ((q[:, k] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - k)
    return code


def morton_order(boxes):
    """Leaf order: stable sort by code, so equal codes stay in input-index order."""
    q, _ = quantized(boxes)
    return np.argsort(interleave(q), kind="stable").astype(np.uint32)


def prefix_codes(boxes):
    """(codes of q >> 9 per axis, flagged): the 36-bit code prefix of every prim, and the prims
    whose prefix a quotient 2 ulp off the correctly rounded one (0.25 in t * 2^21) could move."""
    q, t = quantized(boxes)
    s = t.astype(np.float64) * 2097152.0
    cell = lambda v: np.clip(np.floor(v), 0, 2097151).astype(np.int64) >> 9
    flagged = (cell(s - 0.25) != cell(s + 0.25)).any(axis=1)
    return interleave(q >> 9), flagged


# ---- the clustering loop --------------------------------------------------------------
def _half_area(lo, hi):
    d = hi - lo
    with np.errstate(over="ignore", invalid="ignore"):
        a = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
        return a.astype(np.float32)  # fp32's range: an overflowing area is +inf


def _nearest(lo, hi):
    """nn[i]: the position within R of i whose union with i has the smallest half-area, the
    lower position on ties; -1 when no area compares less than +inf."""
    m = len(lo)
    best = np.full(m, np.inf, np.float32)
    nn = np.full(m, -1, np.int64)
    pos = np.arange(m)
    area = {}
    for d in range(1, min(R, m - 1) + 1):  # pair (i, i + d)
        area[d] = _half_area(np.fmin(lo[:-d], lo[d:]), np.fmax(hi[:-d], hi[d:]))
    for d in sorted(area, reverse=True):  # candidates below i, lowest first
        better = np.zeros(m, bool)
        better[d:] = area[d] < best[d:]
        best[d:] = np.where(better[d:], area[d], best[d:])
        nn[better] = pos[better] - d
    for d in sorted(area):  # candidates above i
        better = np.zeros(m, bool)
        better[:-d] = area[d] < best[:-d]
        best[:-d] = np.where(better[:-d], area[d], best[:-d])
        nn[better] = pos[better] + d
    return nn


class Tree:
    def __init__(self, boxes, order):
        b = np.asarray(boxes, np.float32).astype(np.float64)[np.asarray(order, np.int64)]
        n = self.n = len(b)
        self.lo = np.zeros((2 * n - 1, 3))
        self.hi = np.zeros((2 * n - 1, 3))
        self.lo[:n], self.hi[:n] = b[:, :3], b[:, 3:]
        self.left = np.full(2 * n - 1, -1, np.int64)
        self.right = np.full(2 * n - 1, -1, np.int64)
        self.made = n  # nodes so far
        self.iterations = self.forced = 0

    @property
    def root(self):
        return 0 if self.n == 1 else 2 * self.n - 2


def ploc(tree, top):
    """Merge mutual nearest neighbours until at most `top` clusters are left; returns their
    node ids in curve order."""
    cl = np.arange(tree.n, dtype=np.int64)
    force = False
    while len(cl) > top:
        m = len(cl)
        pos = np.arange(m)
        lo, hi = tree.lo[cl], tree.hi[cl]
        if force:  # the last iteration made no pair: pair 2k, 2k+1
            nn = np.where((pos ^ 1) < m, pos ^ 1, -1)
            mutual = nn >= 0
            tree.forced += 1
        else:
            nn = _nearest(lo, hi)
            mutual = (nn >= 0) & (nn[np.maximum(nn, 0)] == pos)
        create = mutual & (pos < nn)
        keep = ~(mutual & (pos > nn))
        ids = tree.made + np.cumsum(create) - 1  # rank among the creators, in position order
        a, b = pos[create], nn[create]
        tree.lo[ids[create]] = np.fmin(lo[a], lo[b])
        tree.hi[ids[create]] = np.fmax(hi[a], hi[b])
        tree.left[ids[create]], tree.right[ids[create]] = cl[a], cl[b]
        tree.made += int(create.sum())
        cl = np.where(create, ids, cl)[keep]
        force = not create.any()
        tree.iterations += 1
        assert tree.iterations <= 4 * 64 + tree.n, "the builder's own iteration cap"
    return cl


# ---- SAH top --------------------------------------------------------------------------
def _area(lo, hi):
    d = np.maximum(0.0, hi - lo)
    return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])


def sah_top(tree, ids):
    """Full sweep over the clusters `ids`: per axis a stable sort by lo + hi (float32), cost
    left_area * count + right_area * count in float64, strict < so the first axis and the
    first split win; nodes numbered in post-order."""
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * len(ids) + 1000))
    try:
        return _sah(tree, np.asarray(ids, np.int64))
    finally:
        sys.setrecursionlimit(old)


def _sah(tree, ids):
    count = len(ids)
    if count == 1:
        return int(ids[0])
    lo, hi = tree.lo[ids], tree.hi[ids]
    best, best_k, best_perm = np.inf, count // 2, np.arange(count)
    for axis in range(3):
        key = lo[:, axis].astype(np.float32) + hi[:, axis].astype(np.float32)
        perm = np.argsort(key, kind="stable")
        l, h = lo[perm], hi[perm]
        left = _area(np.minimum.accumulate(l), np.maximum.accumulate(h)) * np.arange(1, count + 1)
        right = _area(np.minimum.accumulate(l[::-1])[::-1], np.maximum.accumulate(h[::-1])[::-1])
        for i in range(count - 1, 0, -1):  # split: [0, i) | [i, count)
            c = left[i - 1] + right[i] * (count - i)
            if c < best:
                best, best_k, best_perm = c, i, perm
    ids = ids[best_perm]
    a = _sah(tree, ids[:best_k])
    b = _sah(tree, ids[best_k:])
    v = tree.made
    tree.made += 1
    tree.lo[v], tree.hi[v] = np.minimum(tree.lo[a], tree.lo[b]), np.maximum(tree.hi[a], tree.hi[b])
    tree.left[v], tree.right[v] = a, b
    return v


# ---- layout ---------------------------------------------------------------------------
def _u32(x):
    return np.asarray(x, np.float32).view(np.uint32)


def layout(tree):
    """BVH2 in BFS order (both children's boxes in the parent) and the BVH4 made by expanding
    the largest-area inner child, the first on ties, until a node has four children."""
    n, root = tree.n, tree.root
    out = {"root": 0, "root4": 0, "max_leaf": 1}
    if n == 1:
        out.update(nodes=np.zeros((0, 16), np.float32), nodes4=np.zeros((0, 32), np.uint32),
                   root=LEAF, root4=LEAF, bvh_depth=0)
        return out
    inner = lambda v: v >= n
    kids = lambda v: (int(tree.left[v]), int(tree.right[v]))
    code = lambda v, idx: idx[v] if inner(v) else LEAF | (v << 4)
    # BVH2
    bfs, idx2, level, depth = [root], {}, [root], 0
    while level:
        depth += 1
        level = [c for v in level for c in kids(v) if inner(c)]
        bfs += level
    idx2 = {v: o for o, v in enumerate(bfs)}
    nodes = np.zeros((len(bfs), 16), np.uint32)
    for o, v in enumerate(bfs):
        a, b = kids(v)
        nodes[o, 0:3], nodes[o, 4:7] = _u32(tree.lo[a]), _u32(tree.hi[a])
        nodes[o, 8:11], nodes[o, 12:15] = _u32(tree.lo[b]), _u32(tree.hi[b])
        nodes[o, 3], nodes[o, 7] = code(a, idx2), code(b, idx2)
    # BVH4
    q4, rows, head = [root], [], 0
    while head < len(q4):
        ch = list(kids(q4[head]))
        head += 1
        while len(ch) < 4:
            cand = [k for k in range(len(ch)) if inner(ch[k])]
            if not cand:
                break
            areas = [_area(tree.lo[ch[k]], tree.hi[ch[k]]) for k in cand]
            k = cand[max(range(len(cand)), key=lambda i: (areas[i], -i))]  # first of the largest
            c = ch[k]
            ch[k] = kids(c)[0]
            ch.append(kids(c)[1])
        q4 += [c for c in ch if inner(c)]
        rows.append(ch)
    idx4 = {v: o for o, v in enumerate(q4)}
    nodes4 = np.zeros((len(q4), 32), np.uint32)
    pinf, ninf = _u32([np.inf])[0], _u32([-np.inf])[0]
    for o, ch in enumerate(rows):
        for k in range(4):
            nodes4[o, k] = EMPTY
            nodes4[o, 4 + k:28:8], nodes4[o, 8 + k:28:8] = pinf, ninf
            if k < len(ch):
                nodes4[o, k] = code(ch[k], idx4)
                nodes4[o, 4 + k:28:8], nodes4[o, 8 + k:28:8] = _u32(tree.lo[ch[k]]), _u32(tree.hi[ch[k]])
    out.update(nodes=nodes.view(np.float32), nodes4=nodes4, bvh_depth=depth)
    return out


def build(boxes, order, top):
    """The whole build from a given leaf order -> (layout dict as rt.build_bvh_boxes returns
    it, with "refs" = order; the Tree)."""
    tree = Tree(boxes, order)
    cl = ploc(tree, max(1, top))
    if len(cl) > 1:
        sah_top(tree, cl)
    assert tree.made == 2 * tree.n - 1
    out = layout(tree)
    out["refs"] = np.asarray(order, np.uint32)
    return out, tree


def sah_cost(nodes):
    """SAH cost of an exported BVH2 ([N, 16], root = node 0) in float64, traversal and
    intersection cost 1: the areas of the root box and of every child box (inner or leaf),
    over the root's area."""
    nd = np.asarray(nodes, np.float32).astype(np.float64)
    a, b = (nd[:, 0:3], nd[:, 4:7]), (nd[:, 8:11], nd[:, 12:15])
    root = _area(np.minimum(a[0][0], b[0][0]), np.maximum(a[1][0], b[1][0]))
    return float((root + _area(*a).sum() + _area(*b).sum()) / root)


def tree_sah_cost(tree):
    """sah_cost of a Tree without laying it out: all node areas over the root's."""
    return float(_area(tree.lo, tree.hi).sum() / _area(tree.lo[tree.root], tree.hi[tree.root]))


# ---- inputs for which the reference is exact --------------------------------------------
def lattice_boxes(n, seed, scale=1.0):
    """Integer corners in [0, 64), sizes 1..4 per axis, every seventh box flat on one axis,
    every fifth box two or three times: all the builder computes on them (unions, d*d sums)
    is an integer below 2^24 or a half-integer, so fp32 is exact whatever the contraction,
    and exact ties are everywhere.  `scale` (a power of two) moves the lattice in range."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = len(out)
        size = rng.integers(1, 5, 3)
        if k % 7 == 3:
            size[rng.integers(0, 3)] = 0
        lo = rng.integers(0, 60, 3)
        box = np.concatenate([lo, lo + size])
        out += [box] * (int(rng.integers(2, 4)) if k % 5 == 0 else 1)
    b = np.array(out[:n], np.float32)
    return np.ascontiguousarray(b[rng.permutation(n)] * np.float32(scale))


def curve_boxes(n, seed, p=3):
    """Centroids k * 2^(p-21) with k over all 21 bits per axis, k = 0 and k = 2^21 on every
    axis (so the extent is 2^p exactly and t = 1.0 meets the clamp), a tenth of the centroids
    repeated under other box sizes (equal codes: the order must be stable)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, (1 << 21) + 1, (n, 3))
    k[0], k[1] = 0, 1 << 21
    dup = rng.choice(np.arange(2, n), n // 10, replace=False)
    k[dup] = k[rng.integers(0, n, len(dup))]
    half = rng.integers(0, 4, (n, 3))
    u = 2.0 ** (p - 21)
    return np.concatenate([(k - half) * u, (k + half) * u], axis=1).astype(np.float32)


def random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10, 10, (n, 3))
    h = rng.uniform(0, 0.3, (n, 3))
    return np.concatenate([c - h, c + h], axis=1).astype(np.float32)
