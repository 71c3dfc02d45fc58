"""The feature pass (rt_render_aov, rt_aov.hip) against the CPU oracle.

Checker: pyoracle.trace(pixel, sample) gives the camera ray (o, d, time) and the first
world.Hit (t, u, v, material kind) of every (pixel, sample) in fp64; the expected normal,
albedo and depth are computed from it and the Tree view in numpy below (a small flattener:
Translate / RotateY baked into world-space spheres, quads and triangles; the hit primitive
is the one whose surface holds o + t d).

Bars.  material: equal to the oracle's outside fork pixels.  depth / normal / albedo: the
GPU's max error against the fp64 trace must be <= 4 x the max error of the oracle's own
precision=32 trace (through the same numpy evaluation) on the same pixels, with an absolute
floor of one fp32 ulp of the buffer's scale; the 4 x covers the GPU's non-correctly-rounded
div / sqrt and rcp.  Fork pixels (a sample whose GPU hit lies on another primitive than the
fp64 oracle's: silhouettes) are excluded, at most 1 % of the pixels per scene.

The fp32 twin alone, checked on the CPU for every scene, size and seed used here, forks on
0-1 pixels (<= 1 %) everywhere except Cornell, where it passes through the front face of the
rotated tall box on 8 % of the pixels whatever the seed or size (every view of the box shows
that face).  So the twin's error is measured where the twin hits the fp64 primitive, and the
GPU is held to the resulting bar on ALL its non-fork pixels, the twin's fork pixels included;
outside Cornell the twin's forks are asserted within the cap."""
import os

import numpy as np
import pytest

from tests import scenes
from tests.test_obj_loader import IMG, MAT, NODE, TEX, TRI, _arr

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


# ---------------------------------------------------------------- numpy checker ---
class Flat:
    """world-space primitives of a tree (fp64) + its materials and textures"""

    def __init__(self, tree, world):
        v = tree.view()
        self.nodes = _arr(v.nodes, v.n_nodes, NODE)
        self.kids = _arr(v.children, v.n_children, np.dtype("<i4"))
        self.tris = _arr(v.tris, v.n_tris, TRI)
        self.mats = _arr(v.materials, v.n_materials, MAT)
        self.texs = _arr(v.textures, v.n_textures, TEX)
        imgs = _arr(v.images, v.n_images, IMG)
        self.images = []
        for im in imgs:
            import ctypes as C
            n = int(im["w"]) * int(im["h"]) * 3
            data = bytes((C.c_char * n).from_address(int(im["rgb"])))
            self.images.append(np.frombuffer(data, np.uint8).reshape(int(im["h"]), int(im["w"]), 3))
        self.sph, self.quad, self.tri = [], [], []
        self.media = 0
        self._walk(world, 1.0, 0.0, np.zeros(3))
        self.sph_c1 = np.array([s[0] for s in self.sph]).reshape(-1, 3)
        self.sph_c2 = np.array([s[1] for s in self.sph]).reshape(-1, 3)
        self.sph_r = np.array([s[2] for s in self.sph])
        self.sph_mat = np.array([s[3] for s in self.sph], int)
        self.q_Q = np.array([q[0] for q in self.quad]).reshape(-1, 3)
        self.q_u = np.array([q[1] for q in self.quad]).reshape(-1, 3)
        self.q_v = np.array([q[2] for q in self.quad]).reshape(-1, 3)
        self.q_mat = np.array([q[3] for q in self.quad], int)
        self.t_v = np.array([t[0] for t in self.tri]).reshape(-1, 3, 3)
        self.t_n = np.array([t[1] for t in self.tri]).reshape(-1, 3, 3)
        self.t_flags = np.array([t[2] for t in self.tri], int)
        self.t_mat = np.array([t[3] for t in self.tri], int)

    @staticmethod
    def _rot(c, s, v):  # Ry: transformation.go:87-93
        v = np.asarray(v, float)
        return np.array([c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]])

    def _walk(self, i, c, s, T):
        n = self.nodes[i]
        k, p = int(n["kind"]), n["p"]
        pt = lambda x: self._rot(c, s, x) + T  # noqa: E731
        if k in (0, 1):  # LIST / BVH
            for j in self.kids[int(n["a"]):int(n["a"]) + int(n["b"])]:
                self._walk(int(j), c, s, T)
        elif k == 2:
            c1 = pt(p[0:3])
            c2 = pt(p[3:6]) if p[7] != 0 else c1
            self.sph.append((c1, c2, float(p[6]), int(n["mat"])))
        elif k == 3:
            self.quad.append((pt(p[0:3]), self._rot(c, s, p[3:6]), self._rot(c, s, p[6:9]), int(n["mat"])))
        elif k == 4:
            t = self.tris[int(n["a"])]
            vv = np.array([pt(t["v"][3 * j:3 * j + 3]) for j in range(3)])
            nn = np.array([self._rot(c, s, t["n"][3 * j:3 * j + 3]) for j in range(3)])
            self.tri.append((vv, nn, int(t["flags"]), int(t["mat"])))
        elif k == 5:
            self._walk(int(n["a"]), c, s, T + self._rot(c, s, p[0:3]))
        elif k == 6:
            rad = np.deg2rad(p[0])
            cs, sn = np.cos(rad), np.sin(rad)
            self._walk(int(n["a"]), c * cs - s * sn, s * cs + c * sn, T)
        else:
            self.media += 1

    def tex_value(self, tex, u, v, p):
        """(rgb, solid) -- solid False where a noise texture decides (not checked)"""
        for _ in range(64):
            T = self.texs[tex]
            k = int(T["kind"])
            if k == 0:
                return np.array(T["color"], float), True
            if k == 1:  # texture.go:50-60
                inv = float(T["scale"])
                q = np.floor(inv * p).astype(int)
                tex = int(T["a"]) if int(q.sum()) % 2 == 0 else int(T["b"])
                continue
            if k == 2:  # texture.go:70-86
                im = self.images[int(T["a"])]
                h, w = im.shape[:2]
                uu = abs(u - np.trunc(u))
                vv = 1.0 - abs(v - np.trunc(v))
                i, j = min(int(uu * (w - 1)), w - 1), min(int(vv * (h - 1)), h - 1)
                return im[j, i].astype(float) / 255.0, True
            return np.zeros(3), False
        return np.zeros(3), False

    def evaluate(self, rec, bg):
        """one trace record -> (prim id, kind, normal, albedo, depth, solid)"""
        o, time, d = rec[0:3].astype(float), float(rec[3]), rec[4:7].astype(float)
        t, u, v, kind = float(rec[8]), float(rec[9]), float(rec[10]), int(rec[11])
        if kind < 0:
            return -1, -1, np.zeros(3), np.array(bg, float), 0.0, True
        p = o + t * d
        bid, tbu, tbv, tun = self.identify(p, time, t * np.linalg.norm(d), kind)
        assert bid >= 0, "the oracle's hit point is on no primitive"
        nq = len(self.q_mat)
        ns = len(self.sph_r)
        if bid < ns:
            c = self.sph_c1[bid] + time * (self.sph_c2[bid] - self.sph_c1[bid])
            nout = (p - c) / self.sph_r[bid]  # objects.go:102
            mat = self.sph_mat[bid]
        elif bid < ns + nq:
            j = bid - ns
            nout = np.cross(self.q_u[j], self.q_v[j])
            nout /= np.linalg.norm(nout)
            mat = self.q_mat[j]
        else:
            j = bid - ns - nq
            if self.t_flags[j] & 1:  # interpolateNormal objects.go:389-405
                nout = (1 - tbu - tbv) * self.t_n[j, 0] + tbu * self.t_n[j, 1] + tbv * self.t_n[j, 2]
                nout /= np.linalg.norm(nout)
            else:
                nout = tun
            mat = self.t_mat[j]
        ff = np.dot(d, nout) < 0
        n = nout if ff else -nout
        M = self.mats[mat]
        assert int(M["kind"]) == kind
        solid = True
        if kind == 1:
            alb = np.array(M["albedo"], float)
        elif kind == 2:
            alb = np.ones(3)
        elif kind == 3 and not ff:
            alb = np.zeros(3)
        else:
            alb, solid = self.tex_value(int(M["tex"]), u, v, p)
        return bid, kind, n, alb, t * np.linalg.norm(d), solid

    def identify(self, p, time, dist, kind=None, tol=1e-3):
        """the primitive whose surface holds p (distance to it relative to the ray length
        `dist`, >= 1), among those of material kind `kind` when given -> (id or -2, the
        triangle's barycentrics and unit face normal)"""
        sc = max(1.0, dist)
        mk = self.mats["kind"]
        cands = []
        tb = None
        if len(self.sph_r):
            cc = self.sph_c1 + time * (self.sph_c2 - self.sph_c1)
            r = np.abs(np.linalg.norm(p - cc, axis=1) - np.abs(self.sph_r)) / sc
            cands.append(r if kind is None else np.where(mk[self.sph_mat] == kind, r, np.inf))
        if len(self.q_mat):
            nrm = np.cross(self.q_u, self.q_v)
            w = nrm / (nrm * nrm).sum(1, keepdims=True)
            un = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
            pp = p - self.q_Q
            a = (w * np.cross(pp, self.q_v)).sum(1)
            b = (w * np.cross(self.q_u, pp)).sum(1)
            r = np.abs((un * pp).sum(1)) / sc
            r = np.where((a > -tol) & (a < 1 + tol) & (b > -tol) & (b < 1 + tol), r, np.inf)
            cands.append(r if kind is None else np.where(mk[self.q_mat] == kind, r, np.inf))
        if len(self.t_mat):
            v0 = self.t_v[:, 0]
            e0, e1 = self.t_v[:, 1] - v0, self.t_v[:, 2] - v0
            nrm = np.cross(e0, e1)
            w = nrm / (nrm * nrm).sum(1, keepdims=True)
            un = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
            pp = p - v0
            bu = (w * np.cross(pp, e1)).sum(1)
            bv = (w * np.cross(e0, pp)).sum(1)
            r = np.abs((un * pp).sum(1)) / sc
            r = np.where((bu > -tol) & (bv > -tol) & (bu + bv < 1 + tol), r, np.inf)
            cands.append(r if kind is None else np.where(mk[self.t_mat] == kind, r, np.inf))
            tb = (bu, bv, un)
        r = np.concatenate(cands)
        j = int(r.argmin())
        if not r[j] < tol:
            return -2, 0.0, 0.0, None
        k = j - len(self.sph_r) - len(self.q_mat)
        if k >= 0:
            return j, tb[0][k], tb[1][k], tb[2][k]
        return j, 0.0, 0.0, None

    def prim_at(self, o, d, time, depth):
        """the primitive holding the point at `depth` along the ray (GPU fork detection)"""
        dl = np.linalg.norm(d)
        return self.identify(o + (depth / dl) * d, time, depth)[0]


def expected(oracle, flat, tree, world, lights, cam, rows, n, seed, precision):
    """per (pixel of `rows`, sample < n): prim id, kind, normal, albedo, depth, solid, ray"""
    import copy
    c1 = copy.copy(cam)
    c1.MaxDepth = 1  # the camera ray does not depend on it; one world.Hit per trace
    d = cam.derived()
    W = d.width
    out = {}
    for r in rows:
        for x in range(W):
            for j in range(n):
                rec = oracle.trace(tree, world, lights, c1, r * W + x, j, seed=seed, precision=precision)[0]
                out[(r, x, j)] = flat.evaluate(rec, tuple(cam.Background)) + (rec,)
    return out


def run_scene(rt, oracle, t, cam, w, l, n, seed=3, rank=0, nranks=1, fork_cap=0.01, tree=None,
              material_only=False, label="", twin_cap=True):
    flat = Flat(t, w)
    assert flat.media == 0
    d = cam.derived()
    W, H = d.width, d.height
    rows = list(range(rank, H, nranks))
    with rt.Scene(t, w, l) as sc:
        got = [sc.render_aov(cam, n_samples=k, seed=seed, rank=rank, nranks=nranks) for k in range(1, n + 1)]
        again = sc.render_aov(cam, n_samples=n, seed=seed, rank=rank, nranks=nranks)
        _, rst = sc.render(cam, seed=seed, rank=rank, nranks=nranks, mode="fused")
    g = got[-1]
    for k in ("albedo", "normal", "depth", "material"):  # determinism: bit-identical
        assert np.array_equal(g[k], again[k], equal_nan=True), k
    assert g["albedo"].shape == (len(rows), W, 3) and g["depth"].shape == (len(rows), W)
    assert g["stats"]["samples"] == g["stats"]["segments"] == len(rows) * W * n
    if rst["tree_width"] != 8:  # (BVH8 experiment builds: the feature pass takes the BVH4)
        assert g["stats"]["tree_width"] == rst["tree_width"], "feature pass and render: same structure"
    if tree is not None:
        assert g["stats"]["tree_width"] == tree
    e64 = expected(oracle, flat, t, w, l, cam, rows, n, seed, 64)
    e32 = expected(oracle, flat, t, w, l, cam, rows, n, seed, 32)
    npx = len(rows) * W
    fork = np.zeros((len(rows), W), bool)     # GPU vs fp64 oracle
    fork32 = np.zeros((len(rows), W), bool)   # fp32 twin vs fp64 oracle
    x64 = {k: np.zeros(g[k].shape) for k in ("albedo", "normal", "depth")}
    x32 = {k: np.zeros(g[k].shape) for k in ("albedo", "normal", "depth")}
    solid = np.ones((len(rows), W), bool)
    mat0 = np.zeros((len(rows), W), int)
    for ri, r in enumerate(rows):
        for x in range(W):
            for j in range(n):
                a, b = e64[(r, x, j)], e32[(r, x, j)]
                # sample j's GPU depth from the means over j+1 and j samples
                dj = (j + 1) * float(got[j]["depth"][ri, x]) - (j * float(got[j - 1]["depth"][ri, x]) if j else 0.0)
                rec = a[6]
                # (a missed sample adds 0: the difference is then 0 to the rounding of the means)
                eps = 1e-5 * (j + 1) * max(1.0, float(got[j]["depth"][ri, x]))
                gp = -1 if abs(dj) <= eps else (-3 if dj < 0.0 else flat.prim_at(
                    rec[0:3].astype(float), rec[4:7].astype(float), float(rec[3]), dj))
                fork[ri, x] |= gp != a[0]
                fork32[ri, x] |= b[0] != a[0]
                solid[ri, x] &= a[5] and b[5]
                for k, idx in (("normal", 2), ("albedo", 3), ("depth", 4)):
                    x64[k][ri, x] += np.asarray(a[idx]) / n
                    x32[k][ri, x] += np.asarray(b[idx]) / n
                if j == 0:
                    mat0[ri, x] = a[1]
    print(f"fork pixels: gpu {fork.sum()} fp32 twin {fork32.sum()} of {npx}")
    if twin_cap:  # (not Cornell: see the module docstring)
        assert fork32.mean() <= fork_cap, "the fp32 oracle twin alone exceeds the fork cap"
    assert fork.mean() <= fork_cap, (fork.sum(), npx)
    ok = ~fork
    assert np.array_equal(g["material"][ok], mat0[ok])
    if material_only:
        return
    for k in ("depth", "normal", "albedo"):
        m = ok & solid if k == "albedo" else ok  # the GPU: every non-fork pixel
        mt = m & ~fork32                         # the twin: where it hits the fp64 primitive
        scale = max(1.0, float(np.abs(x64[k][m]).max())) if m.any() else 1.0
        floor = scale * 2.0 ** -23
        eg = float(np.abs(g[k][m] - x64[k][m]).max()) if m.any() else 0.0
        eo = float(np.abs(x32[k][mt] - x64[k][mt]).max()) if mt.any() else 0.0
        bar = max(4 * eo, floor)
        print(f"{label} {k}: gpu err {eg:.3e} fp32-oracle err {eo:.3e} ratio {eg / max(eo, 1e-30):.2f} floor {floor:.2e}")
        assert eg <= bar, (k, eg, eo, floor)


def _shape(cam, w, h, spp=4):
    cam.Width, cam.AspectRatio, cam.SamplesPerPixel = w, w / h, spp
    return cam


def sphere_field(rt):
    """320 small spheres (solid, metal, glass, checker) over the room: BVH4"""
    t = rt.Tree(11)
    world, lights = scenes._room(t)
    mats = [t.lambertian((0.7, 0.3, 0.1)), t.metal((0.8, 0.8, 0.9), 0.2), t.dielectric(1.5),
            t.lambertian(t.checker(0.7, t.solid(0.2, 0.3, 0.1), t.solid(0.9, 0.9, 0.9)))]
    for i in range(320):
        c = (t.rand_range(-6, 6), t.rand_range(0.3, 5), t.rand_range(-3, 6))
        t.add(world, t.sphere(c, t.rand_range(0.15, 0.4), mats[i % 4]))
    return t, scenes._cam(rt, (0, 3, -9), (0, 2, 0)), world, lights


def _build(rt, name):
    if name == "sphere_field":
        return sphere_field(rt)
    if name == "obj_mixed":
        return scenes.obj_mixed(rt, ASSETS)
    return rt.demo_scene(name)


@pytest.mark.parametrize("name,w,h,n", [
    ("cornell", 16, 12, 4), ("cornell", 13, 9, 1), ("simple_light", 16, 12, 4), ("quads", 16, 12, 4),
    ("sphere_field", 16, 12, 4), ("sphere_field", 13, 9, 1), ("obj_mixed", 16, 12, 4)])
def test_feature_buffers_match_oracle(rt, oracle, gpu, name, w, h, n):
    t, cam, wd, l = _build(rt, name)
    _shape(cam, w, h)
    run_scene(rt, oracle, t, cam, wd, l, n, label=f"{name} {w}x{h} n={n}", twin_cap=name != "cornell")


def test_row_shares(rt, oracle, gpu):
    """rank 1 of 3: the rows of rt_render's partition"""
    t, cam, wd, l = rt.demo_scene("cornell")
    _shape(cam, 16, 12)
    run_scene(rt, oracle, t, cam, wd, l, 4, rank=1, nranks=3, label="cornell rows 1/3", twin_cap=False)
    with rt.Scene(t, wd, l) as sc:
        full = sc.render_aov(cam, n_samples=4, seed=3)
        part = sc.render_aov(cam, n_samples=4, seed=3, rank=1, nranks=3)
    for k in ("albedo", "normal", "depth", "material"):
        assert np.array_equal(full[k][1::3], part[k])


@pytest.mark.parametrize("qbvh,tree", [("1", 5), ("0", 4)])
def test_compressed_bvh4(rt, oracle, gpu, tune, qbvh, tree):
    """book1 without defocus: its tree is read through L1/L2, so the render (and the feature
    pass) takes the compressed BVH4; RT_QBVH=0 puts both on the 128-B nodes.  (RT_TREE selects
    among the LDS-resident structures only: it cannot force tree 5.)"""
    tune("RT_QBVH", qbvh)
    t, cam, wd, l = rt.demo_scene("book1")
    cam.DefocusAngle = 0.0
    _shape(cam, 16, 12)
    run_scene(rt, oracle, t, cam, wd, l, 4, tree=tree, label=f"book1 tree {tree}")


def test_bvh2_and_bvh4_by_knob(rt, gpu, tune):
    """RT_TREE moves a tiny scene between the record loop, the BVH2 and the BVH4: the same
    closest hits, so the same material and (to rounding of another test order) depth"""
    t, cam, wd, l = rt.demo_scene("cornell")
    _shape(cam, 16, 12)
    res = {}
    for knob in (None, "2", "4"):
        if knob:
            tune("RT_TREE", knob)
        with rt.Scene(t, wd, l) as sc:
            res[knob] = sc.render_aov(cam, n_samples=4, seed=3)
    assert [res[k]["stats"]["tree_width"] for k in (None, "2", "4")] == [0, 2, 4]
    for k in ("2", "4"):
        assert np.array_equal(res[k]["material"], res[None]["material"])
        assert np.allclose(res[k]["depth"], res[None]["depth"], rtol=1e-5, atol=0)
        assert np.allclose(res[k]["normal"], res[None]["normal"], atol=1e-6)


def test_defocus_material(rt, oracle, gpu):
    """book1's defocused camera: material only, fork cap 3 % (the lens draw is 16-bit)"""
    t, cam, wd, l = rt.demo_scene("book1")
    _shape(cam, 16, 12)
    assert cam.DefocusAngle > 0
    run_scene(rt, oracle, t, cam, wd, l, 1, fork_cap=0.03, material_only=True)


@pytest.mark.parametrize("name", ["cornell", "sphere_field"])
def test_ray_identity_with_render_trace(rt, gpu, name):
    """rt_render's trace_out of (pixel, sample 0) reports the t and the primitive of the
    feature pass's ray: the same camera ray through the same structure.  rt_aov carries no
    primitive id, so both hit points (the trace's o + t d and the point at the feature pass's
    depth along the same ray) are mapped to the primitive whose surface holds them, and the
    primitive's material kind must be the material buffer's."""
    t, cam, wd, l = _build(rt, name)
    _shape(cam, 16, 12)
    d = cam.derived()
    flat = Flat(t, wd)
    with rt.Scene(t, wd, l) as sc:
        a = sc.render_aov(cam, n_samples=1, seed=5)
        for pix in (0, 5 * 16 + 7, 11 * 16 + 15, 8 * 16 + 3):
            _, st = sc.render(cam, seed=5, trace=(pix, 0), mode="fused")
            v0 = st["trace"][0]
            y, x = divmod(pix, d.width)
            ref = v0[11:12].view(np.uint32)[0]
            if ref == 0xFFFFFFFF:
                assert a["material"][y, x] == -1 and a["depth"][y, x] == 0
                continue
            dlen = np.float32(np.sqrt(np.float32(v0[4]) ** 2 + np.float32(v0[5]) ** 2 + np.float32(v0[6]) ** 2))
            assert abs(a["depth"][y, x] - v0[8] * dlen) <= 4 * np.spacing(np.float32(a["depth"][y, x]))
            o, dd, tm = v0[0:3].astype(float), v0[4:7].astype(float), float(v0[3])
            p_trace = flat.prim_at(o, dd, tm, float(v0[8]) * float(np.linalg.norm(dd)))
            p_aov = flat.prim_at(o, dd, tm, float(a["depth"][y, x]))
            assert p_trace >= 0 and p_trace == p_aov
            ns, nq = len(flat.sph_r), len(flat.q_mat)
            mat = (flat.sph_mat[p_aov] if p_aov < ns else flat.q_mat[p_aov - ns] if p_aov < ns + nq
                   else flat.t_mat[p_aov - ns - nq])
            assert a["material"][y, x] == int(flat.mats[mat]["kind"])


def test_n_samples_zero_means_one(rt, gpu):
    t, cam, wd, l = rt.demo_scene("cornell")
    _shape(cam, 16, 12)
    with rt.Scene(t, wd, l) as sc:
        a, b = sc.render_aov(cam, n_samples=0, seed=2), sc.render_aov(cam, n_samples=1, seed=2)
        with pytest.raises(rt.RtError):
            sc.render_aov(cam, n_samples=5, seed=2)
    assert np.array_equal(a["depth"], b["depth"]) and a["stats"]["samples"] == 16 * 12
