"""go_raytracer_amd — MI355X-native drop-in for go_raytracer's render loop.

Python face of the C ABI (include/rt_abi.h).  The object model mirrors the
reference package API: ``Tree`` methods are the hittable constructors
(NewSphere, NewQuad, NewBox, RotateY, Translate, ConstantMedium, BuildBVH, ...),
``Camera`` mirrors camera.Camera's public fields (camera.go:26-36) with the
same zero-means-default rules, and ``Camera.Render(world, lights)`` renders
through the HIP path (camera.go:156).  There is no CPU render path here: the
HIP library must be built and a GPU present, otherwise calls raise.
"""
import ctypes as C
import math
import weakref

import numpy as np

from . import _lib
from ._lib import (RT_FT_ALL, RT_FT_BOX, RT_NOISE_MARBLE, RT_NOISE_PERLIN,  # noqa: F401
                   RT_NOISE_TURBULENT, RtAccumInfo, RtAov, RtAovEmit, RtAovMedia, RtAovSpec, RtAovSpecOpts,
                   RtCamera, RtDenoiseOpts,
                   RtDenoiseVarOpts, RtCameraDerived, RtError, RtRenderOpts, RtSceneInfo, RtStats, RtTreeView,
                   check, lib)

__all__ = ["Tree", "Camera", "Scene", "Accumulator", "quantize", "format_ppm", "device_count", "RtError",
           "tune", "untune", "tuning", "tune_knobs", "tune_from_env",
           "demo_scene", "DEMO_SCENES", "build_bvh_boxes", "LoadObjOptions", "DefaultLoadOptions", "quantize_device",
           "format_ppm_device", "denoise", "denoise_device", "denoise_var", "denoise_var_device",
           "RtDenoiseVarOpts", "reproject", "reproject_device", "reproject_emit", "reproject_emit_device", "reproject_light", "reproject_light_device", "reproject_moments", "reproject_moments_device", "reproject_clip", "reproject_clip_device", "reproject_spec", "reproject_spec_device",
           "Temporal", "Pipeline", "AccumulatorShares"]

DEMO_SCENES = ("book1", "book2", "book3", "simple_light", "quads", "cornell", "cornell_smoke",
               "model")


def _d3(v):
    return _lib.D3(*[float(x) for x in v])


def _as_dict(s):
    """A ctypes structure (RtStats, RtAccumInfo, ...) as {field: value}."""
    return {f: getattr(s, f) for f, _ in s._fields_}


class Tree:
    """A scene under construction (rt_tree).  Handles are plain ints."""

    def __init__(self, seed=1):
        p = C.c_void_p()
        check(lib().rt_tree_create(C.byref(p)))
        self._p = p
        # bound now: at interpreter shutdown module globals (lib) may already be None
        self._destroy = lib().rt_tree_destroy
        check(lib().rt_tree_seed(self._p, seed))

    def __del__(self):
        if getattr(self, "_p", None):
            self._destroy(self._p)
            self._p = None

    @property
    def ptr(self):
        return self._p

    # scene RNG (replaces math/rand for scene content)
    def rand(self):
        return lib().rt_tree_rand(self._p)

    def rand_range(self, lo, hi):
        return lib().rt_tree_rand_range(self._p, lo, hi)

    def randn(self, n):
        return lib().rt_tree_randn(self._p, n)

    # textures
    def solid(self, r, g, b):
        return check(lib().rt_tex_solid(self._p, r, g, b))

    def checker(self, scale, even, odd):
        return check(lib().rt_tex_checker(self._p, scale, even, odd))

    def image(self, rgb):
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w = a.shape[:2]
        return check(lib().rt_tex_image(self._p, a.ctypes.data, w, h))

    def noise(self, scale, variant=RT_NOISE_PERLIN):
        return check(lib().rt_tex_noise(self._p, scale, variant))

    def noise_tables(self, scale, variant, ranvec, perm):
        rv = np.ascontiguousarray(ranvec, dtype=np.float64).reshape(256, 3)
        pm = np.ascontiguousarray(perm, dtype=np.int32).reshape(3, 256)
        return check(lib().rt_tex_noise_tables(
            self._p, scale, variant, rv.ctypes.data_as(C.POINTER(C.c_double)),
            pm.ctypes.data_as(C.POINTER(C.c_int32))))

    # materials (a colour tuple means NewLambertian / NewDiffuseLight / NewIsotropic)
    def _tex(self, t):
        return t if isinstance(t, int) else self.solid(*t)

    def lambertian(self, tex):
        return check(lib().rt_mat_lambertian(self._p, self._tex(tex)))

    def metal(self, albedo, fuzz):
        return check(lib().rt_mat_metal(self._p, *[float(x) for x in albedo], fuzz))

    def dielectric(self, ior):
        return check(lib().rt_mat_dielectric(self._p, ior))

    def light(self, tex):
        return check(lib().rt_mat_diffuse_light(self._p, self._tex(tex)))

    def isotropic(self, tex):
        return check(lib().rt_mat_isotropic(self._p, self._tex(tex)))

    # hittables
    def list(self, *objs):
        h = check(lib().rt_new_list(self._p))
        for o in objs:
            self.add(h, o)
        return h

    def add(self, lst, obj):
        check(lib().rt_list_add(self._p, lst, obj))

    def bvh(self, lst):
        return check(lib().rt_build_bvh(self._p, lst))

    def sphere(self, center, radius, mat):
        return check(lib().rt_new_sphere(self._p, _d3(center), radius, mat))

    def motion_sphere(self, c1, c2, radius, mat):
        return check(lib().rt_new_motion_sphere(self._p, _d3(c1), _d3(c2), radius, mat))

    def quad(self, Q, u, v, mat):
        return check(lib().rt_new_quad(self._p, _d3(Q), _d3(u), _d3(v), mat))

    def box(self, a, b, mat):
        return check(lib().rt_new_box(self._p, _d3(a), _d3(b), mat))

    def triangle(self, verts, mat, normals=None, uv=None):
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(9)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64).reshape(9)
        t = None if uv is None else np.ascontiguousarray(uv, dtype=np.float64).reshape(6)
        dp = C.POINTER(C.c_double)
        return check(lib().rt_new_triangle(
            self._p, v.ctypes.data_as(dp), None if n is None else n.ctypes.data_as(dp),
            None if t is None else t.ctypes.data_as(dp), mat))

    def triangles(self, verts, mats, normals=None, uv=None):
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 9)
        n_tri = v.shape[0]
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(mats, dtype=np.int32), (n_tri,)))
        dp = C.POINTER(C.c_double)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 9)
        t = None if uv is None else np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 6)
        return check(lib().rt_new_triangles(
            self._p, n_tri, v.ctypes.data_as(dp), None if n is None else n.ctypes.data_as(dp),
            None if t is None else t.ctypes.data_as(dp), m.ctypes.data_as(C.POINTER(C.c_int32))))

    def translate(self, obj, offset):
        return check(lib().rt_translate(self._p, obj, _d3(offset)))

    def rotate_y(self, obj, degrees):
        return check(lib().rt_rotate_y(self._p, obj, degrees))

    def medium(self, boundary, density, tex):
        return check(lib().rt_constant_medium(self._p, boundary, density, self._tex(tex)))

    # OBJ/MTL loader (objLoader.go:63-538)
    def LoadObjWithOptions(self, filename, options=None, mtl_text=None, obj_text=None):
        """LoadObjWithOptions objLoader.go:72: returns (model, lights) node ids —
        BuildBVH over every triangle and the list of emissive (and, with
        FindWindows, dielectric) triangles.  ``obj_text``/``mtl_text`` load from
        memory instead of the files.  Image maps the C loader cannot decode
        (anything but binary PPM) are decoded here with PIL, when importable."""
        o = options if options is not None else DefaultLoadOptions()
        c, keep = o.to_c(self, filename, mtl_text)
        model, lights, info = C.c_int(-1), C.c_int(-1), _lib.RtObjInfo()
        if obj_text is None:
            check(lib().rt_load_obj(self._p, filename.encode(), C.byref(c), C.byref(model),
                                    C.byref(lights), C.byref(info)))
        else:
            ob = obj_text.encode() if isinstance(obj_text, str) else bytes(obj_text)
            mb = None if mtl_text is None else (
                mtl_text.encode() if isinstance(mtl_text, str) else bytes(mtl_text))
            check(lib().rt_load_obj_memory(
                self._p, ob, len(ob), mb, 0 if mb is None else len(mb),
                None if filename is None else filename.encode(), C.byref(c), C.byref(model),
                C.byref(lights), C.byref(info)))
        del keep
        self.last_obj_info = info
        return model.value, lights.value

    def LoadObj(self, filename, mat=-1):
        """LoadObj objLoader.go:64: default options with DefaultMaterial = mat."""
        o = DefaultLoadOptions()
        o.DefaultMaterial = mat
        return self.LoadObjWithOptions(filename, o)

    def view(self):
        v = RtTreeView()
        check(lib().rt_tree_get_view(self._p, C.byref(v)))
        return v


class LoadObjOptions:
    """LoadObjOptions objLoader.go:18-29 (DefaultMaterial: a material id, -1 = nil)."""

    def __init__(self, **kw):
        self.ScaleFactor = 1.0
        self.FlipYZ = False
        self.Debug = True
        self.IgnoreNormals = False
        self.Center = True
        self.FlipFaces = False
        self.Position = (0.0, 0.0, 0.0)
        self.DefaultMaterial = -1
        self.IgnoreMtl = False
        self.FindWindows = False
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def to_c(self, tree, filename, mtl_text=None):
        c = _lib.RtObjOptions()
        check(lib().rt_obj_default_options(C.byref(c)))
        c.scale_factor = float(self.ScaleFactor)
        c.flip_yz, c.debug = int(bool(self.FlipYZ)), int(bool(self.Debug))
        c.ignore_normals, c.center = int(bool(self.IgnoreNormals)), int(bool(self.Center))
        c.flip_faces = int(bool(self.FlipFaces))
        c.default_material = int(self.DefaultMaterial)
        c.position = _d3(self.Position)
        c.ignore_mtl, c.find_windows = int(bool(self.IgnoreMtl)), int(bool(self.FindWindows))
        keep = []
        names = [] if self.IgnoreMtl else _mtl_image_names(filename, mtl_text)
        imgs = []
        for n in names:
            rgb = _decode_image(n)
            if rgb is None:
                continue
            keep.append(rgb)
            imgs.append(_lib.RtObjImage(n.encode(), rgb.ctypes.data, rgb.shape[1], rgb.shape[0]))
        if imgs:
            arr = (_lib.RtObjImage * len(imgs))(*imgs)
            keep.append(arr)
            c.n_images, c.images = len(imgs), C.cast(arr, C.POINTER(_lib.RtObjImage))
        return c, keep


def DefaultLoadOptions():
    """DefaultLoadOptions objLoader.go:32-45."""
    return LoadObjOptions()


def _mtl_image_names(filename, mtl_text):
    """map_Kd / map_Ka names of the MTL an OBJ references (mtlLoader.go:174-184)."""
    import os
    text = mtl_text
    if text is None:
        if filename is None or not os.path.exists(filename):
            return []
        import re
        with open(filename, "rb") as f:
            data = f.read()
        k = data.find(b"mtllib")  # C-speed scan first: most meshes have none
        m = None if k < 0 else re.search(rb"^[ \t]*mtllib[ \t]+([^\r\n]+)",
                                         data[max(0, data.rfind(b"\n", 0, k) + 1):], re.M)
        if m is None:
            return []
        lib_name = " ".join(m.group(1).decode("utf-8", "replace").split())
        path = os.path.join(os.path.dirname(filename), lib_name)
        if not os.path.exists(path):
            return []
        with open(path, "rb") as f:
            text = f.read()
    if isinstance(text, bytes):
        text = text.decode("utf-8", "replace")
    names = []
    for line in text.splitlines():
        p = line.split()
        if len(p) >= 2 and p[0] in ("map_Kd", "map_Ka"):
            names.append(" ".join(p[1:]))
    return names


def _decode_image(name):
    """image.Decode of a map file (imageLoader.go:29-46) for formats the C loader
    does not read; None leaves the file to the C loader (PPM, or its error)."""
    import os
    if not os.path.exists(name):
        return None
    with open(name, "rb") as f:
        if f.read(2) == b"P6":
            return None
    try:
        from PIL import Image
    except ImportError:
        return None
    return np.ascontiguousarray(np.asarray(Image.open(name).convert("RGB")), dtype=np.uint8)


class Camera:
    """camera.Camera (camera.go:24-62): public fields, 0 means default."""

    _FIELDS = ("AspectRatio", "Width", "SamplesPerPixel", "MaxDepth", "MaxThreads", "VerticalFOV",
               "DefocusAngle", "FocusDistance", "Background", "MaxContribution")

    def __init__(self, **kw):
        self.AspectRatio = 0.0
        self.Width = 0
        self.SamplesPerPixel = 0
        self.MaxDepth = 0
        self.MaxThreads = 0
        self.VerticalFOV = 0.0
        self.DefocusAngle = 0.0
        self.FocusDistance = 0.0
        self.Background = (0.0, 0.0, 0.0)
        self.MaxContribution = 0.0
        self._pos = None
        for k, v in kw.items():
            if k not in self._FIELDS:
                raise AttributeError(k)
            setattr(self, k, v)

    def PositionCamera(self, lookFrom=None, lookAt=None, vup=None):  # camera.go:65-81
        self._pos = (tuple(lookFrom) if lookFrom is not None else (0.0, 0.0, 0.0),
                     tuple(lookAt) if lookAt is not None else (0.0, 0.0, -1.0),
                     tuple(vup) if vup is not None else (0.0, 1.0, 0.0))

    def to_c(self):
        c = RtCamera()
        c.aspect_ratio = self.AspectRatio
        c.width = int(self.Width)
        c.samples_per_pixel = int(self.SamplesPerPixel)
        c.max_depth = int(self.MaxDepth)
        c.max_threads = int(self.MaxThreads)
        c.vertical_fov = self.VerticalFOV
        c.defocus_angle = self.DefocusAngle
        c.focus_distance = self.FocusDistance
        c.background = _d3(self.Background)
        c.max_contribution = self.MaxContribution
        if self._pos is not None:
            c.positioned = 1
            c.look_from, c.look_at, c.vup = (_d3(x) for x in self._pos)
        return c

    @classmethod
    def from_c(cls, c):
        cam = cls()
        cam.AspectRatio = c.aspect_ratio
        cam.Width = c.width
        cam.SamplesPerPixel = c.samples_per_pixel
        cam.MaxDepth = c.max_depth
        cam.MaxThreads = c.max_threads
        cam.VerticalFOV = c.vertical_fov
        cam.DefocusAngle = c.defocus_angle
        cam.FocusDistance = c.focus_distance
        cam.Background = tuple(c.background)
        cam.MaxContribution = c.max_contribution
        if c.positioned:
            cam._pos = (tuple(c.look_from), tuple(c.look_at), tuple(c.vup))
        return cam

    def derived(self):
        d = RtCameraDerived()
        c = self.to_c()
        check(lib().rt_camera_derive(C.byref(c), C.byref(d)))
        return d

    def image_size(self):
        d = self.derived()
        return d.width, d.height, d.spp_sqrt

    def Render(self, tree, world, lights, seed=1, device=0):
        """Render the full image on one GPU -> float32 [H, W, 3] linear mean RGB."""
        with Scene(tree, world, lights) as sc:
            img, _ = sc.render(self, seed=seed, device=device)
        return img


class Scene:
    """A flattened scene (rt_scene): BVH built on the host, uploaded on first render."""

    def __init__(self, tree, world, lights=-1):
        p = C.c_void_p()
        check(lib().rt_scene_create(tree.ptr, world, lights, C.byref(p)))
        self._p = p
        self._destroy = lib().rt_scene_destroy  # usable at interpreter shutdown
        self.tree = tree
        self._accums = weakref.WeakSet()

    def close(self):
        if getattr(self, "_p", None):
            for a in list(self._accums):  # rt_scene_destroy frees them: their handles die here
                a._p = None
            self._destroy(self._p)
            self._p = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def progress(self):
        """(samples done, samples total) of the render in flight (rt_progress);
        callable from another thread while render() blocks."""
        d, t = C.c_uint64(0), C.c_uint64(0)
        check(lib().rt_progress(self._p, C.byref(d), C.byref(t)))
        return d.value, t.value

    def info(self):
        i = RtSceneInfo()
        check(lib().rt_scene_info_get(self._p, C.byref(i)))
        return _as_dict(i)

    def export_bvh(self):
        nn, nr, root = C.c_int32(), C.c_int32(), C.c_uint32()
        check(lib().rt_scene_export_bvh(self._p, None, C.byref(nn), None, C.byref(nr), C.byref(root)))
        nodes = np.zeros((max(nn.value, 0), 16), np.float32)
        refs = np.zeros(max(nr.value, 0), np.uint32)
        check(lib().rt_scene_export_bvh(self._p, nodes.ctypes.data or None, C.byref(nn),
                                        refs.ctypes.data or None, C.byref(nr), C.byref(root)))
        n = C.c_int32()
        check(lib().rt_scene_export_prim_bounds(self._p, None, C.byref(n)))
        bounds = np.zeros((n.value, 6), np.float32)
        check(lib().rt_scene_export_prim_bounds(self._p, bounds.ctypes.data or None, C.byref(n)))
        return nodes, refs, int(root.value), bounds

    def export_bvh8(self):
        """(nodes uint32 [N, 32] in the rt_device.h BVH8 layout, refs8 uint32 [R])."""
        nn, nr = C.c_int32(), C.c_int32()
        check(lib().rt_scene_export_bvh8(self._p, None, C.byref(nn), None, C.byref(nr)))
        nodes = np.zeros((max(nn.value, 0), 32), np.uint32)
        refs = np.zeros(max(nr.value, 0), np.uint32)
        check(lib().rt_scene_export_bvh8(self._p, nodes.ctypes.data or None, C.byref(nn),
                                         refs.ctypes.data or None, C.byref(nr)))
        return nodes, refs

    def export_qbvh(self):
        """(items uint32 [N, 16]: the compressed BVH4's 64-B items, nodes4 uint32 [M, 32]:
        the BVH4 they encode, root4) -- rt_device.h layouts, for structural tests."""
        ni, nn, root = C.c_int32(), C.c_int32(), C.c_uint32()
        check(lib().rt_scene_export_qbvh(self._p, None, C.byref(ni), None, C.byref(nn), C.byref(root)))
        items = np.zeros((max(ni.value, 0), 16), np.uint32)
        nodes = np.zeros((max(nn.value, 0), 32), np.uint32)
        check(lib().rt_scene_export_qbvh(self._p, items.ctypes.data or None, C.byref(ni),
                                         nodes.ctypes.data or None, C.byref(nn), C.byref(root)))
        return items, nodes, int(root.value)

    def export_records(self, fill=True):
        """(pairs uint32 [4 * n_slots + shade_n, 4]: the record loop's pair array with the shade
        table appended, n_slots, the seven layout counts in rt_brute_shape's order, shade_n,
        n_boxes); n_slots = 0 for a scene too large to have pairs.  fill=False: sizes only."""
        ns, sn, nb, counts = C.c_int32(), C.c_int32(), C.c_int32(), (C.c_int32 * 7)()
        check(lib().rt_scene_export_records(self._p, None, C.byref(ns), counts, C.byref(sn), C.byref(nb)))
        pairs = np.zeros((4 * ns.value + sn.value, 4), np.uint32)
        if fill:
            check(lib().rt_scene_export_records(self._p, pairs.ctypes.data or None, C.byref(ns), counts,
                                                C.byref(sn), C.byref(nb)))
        return pairs, ns.value, tuple(counts), sn.value, nb.value

    def lean_light(self):
        """(kind, block uint32 [n_floats]): the lean light kind the host matcher gives the
        scene's light list (rt_scene_lean_light; 0 = the general light code) and the light
        as the kernel of that kind reads it (all zero for kind 0).  No device needed."""
        k, n = C.c_int32(), C.c_int32()
        check(lib().rt_scene_lean_light(self._p, C.byref(k), None, C.byref(n)))
        block = np.zeros(n.value, np.uint32)
        check(lib().rt_scene_lean_light(self._p, C.byref(k), block.ctypes.data or None, C.byref(n)))
        return k.value, block

    def plan_light(self, device=0):
        """The lean light kind a fused render of this scene on `device` launches with now
        (rt_scene_plan_light; honours RT_LEAN_LIGHT)."""
        k = C.c_int32()
        check(lib().rt_scene_plan_light(self._p, device, C.byref(k)))
        return k.value

    def lean_emitter(self):
        """The emitter slot of the scene's record layout (rt_scene_lean_emitter): the slot of
        its one emissive record when the record-loop kernel may draw a vertex's numbers
        before it resolves the winner, else -1.  No device needed."""
        k = C.c_int32()
        check(lib().rt_scene_lean_emitter(self._p, C.byref(k)))
        return k.value

    def plan_early(self, device=0):
        """1 when a fused render of this scene on `device` launches the early-draw record-loop
        kernel now (rt_scene_plan_early; honours RT_LEAN_EARLY_DRAW), else 0."""
        k = C.c_int32()
        check(lib().rt_scene_plan_early(self._p, device, C.byref(k)))
        return k.value

    def plan_cost(self, device=0):
        """1 when that launch takes the early-draw kernel's lean-cost twin (rt_scene_plan_cost;
        honours RT_LEAN_COST), else 0."""
        k = C.c_int32()
        check(lib().rt_scene_plan_cost(self._p, device, C.byref(k)))
        return k.value

    MODES = {"auto": 0, "wavefront": 1, "fused": 2}

    @staticmethod
    def _opts(seed, device, rank, nranks, path_slots, chunk, profile, stream, mode="auto"):
        o = RtRenderOpts()
        o.mode = Scene.MODES[mode]
        o.seed = seed
        o.device = device
        o.rank = rank
        o.nranks = nranks
        o.path_slots = path_slots
        o.chunk = chunk
        o.flags = _lib.RT_FLAG_PROFILE if profile else 0
        o.stream = stream
        return o

    def render(self, camera, seed=1, device=0, rank=0, nranks=1, path_slots=0, chunk=0,
               profile=False, trace=None, mode="auto", progress_slices=0):
        """Render this rank's rows -> (float32 [rows, W, 3], stats dict).

        progress_slices=S runs the fused render as S launches so that progress()
        (from another thread) advances per slice; the image is the same.

        trace=(pixel, sample) additionally returns stats["trace"]: float32 [V, 12]
        {o.xyz, time, d.xyz, vertex, t, u, v, ref bits} per world.Hit of that sample.
        """
        d = camera.derived()
        rows = len(range(rank, d.height, nranks))
        out = np.zeros((rows, d.width, 3), np.float32)
        st = RtStats()
        c = camera.to_c()
        o = self._opts(seed, device, rank, nranks, path_slots, chunk, profile, None, mode)
        o.progress_slices = progress_slices
        tbuf = None
        if trace is not None:
            tbuf = np.zeros((d.max_depth + 1, 12), np.float32)
            o.trace_pixel, o.trace_sample = int(trace[0]), int(trace[1])
            o.trace_cap = tbuf.shape[0]
            o.trace_out = tbuf.ctypes.data
        check(lib().rt_render(self._p, C.byref(c), C.byref(o), out.ctypes.data, C.byref(st)))
        res = _as_dict(st)
        if tbuf is not None:
            res["trace"] = tbuf[tbuf[:, 7] >= 0]
        return out, res

    def render_multi(self, camera, devices, seed=1, path_slots=0, chunk=0, profile=False,
                     mode="auto", rccl=False):
        """The whole image over several devices (rt_render_multi: row r on
        devices[r % n], gathered to devices[0] by peer copies, or by one RCCL
        ncclGather with rccl=True) -> (float32 [H, W, 3], stats)."""
        d = camera.derived()
        out = np.zeros((d.height, d.width, 3), np.float32)
        st = _multi(self, camera, devices, (out.ctypes.data, False), seed, path_slots, chunk,
                    profile, mode, rccl)
        return out, st

    def render_multi_device(self, camera, devices, out_ptr, seed=1, path_slots=0, chunk=0,
                            profile=False, mode="auto", rccl=False):
        """rt_render_multi_device: the whole image into a device buffer on devices[0]."""
        return _multi(self, camera, devices, (out_ptr, True), seed, path_slots, chunk, profile,
                      mode, rccl)

    def render_device(self, camera, out_ptr, seed=1, device=0, rank=0, nranks=1, path_slots=0,
                      chunk=0, profile=False, stream=None, mode="auto"):
        """Render into a device buffer (e.g. torch tensor .data_ptr()) on `stream`."""
        st = RtStats()
        c = camera.to_c()
        o = self._opts(seed, device, rank, nranks, path_slots, chunk, profile, stream, mode)
        check(lib().rt_render_device(self._p, C.byref(c), C.byref(o), C.c_void_p(out_ptr),
                                     C.byref(st)))
        return _as_dict(st)

    def render_aov(self, camera, n_samples=1, seed=1, device=0, rank=0, nranks=1, emit=False, media=False,
                   specular=False, max_bounces=0, max_fuzz=0.0):
        """Feature buffers of this rank's rows (rt_render_aov): the first hit of the camera
        rays render() gives samples 0 .. n_samples-1 of every pixel, averaged.  Returns
        {"albedo": float32 [rows, W, 3], "normal": float32 [rows, W, 3] (world space, facing
        the ray, 0 on a miss), "depth": float32 [rows, W], "material": int32 [rows, W]
        (RT_MAT_* of sample 0, -1 on a miss), "stats": dict}.  emit=True (rt_render_aov_emit)
        adds the emission split: "emission" float32 [rows, W, 3] (what directly seen lights add
        to the pixel: their emission, which the render does not clamp), "surface_albedo" float32 [rows, W, 3]
        (the albedo of the samples that see no light) and "coverage" float32 [rows, W] (the
        fraction of samples that see a light's front face).  media=True (rt_render_aov_media)
        traces the constant media as the render's camera vertex does: every buffer is then of the
        sample's first event, a scatter inside a volume included (the phase material's albedo,
        no normal, the scatter's depth), and "scatter" float32 [rows, W] is the fraction of
        samples whose first event is a scatter.  With emit=True it returns both sets.
        specular=True (rt_render_aov_spec) follows dielectrics and metals of fuzz <= max_fuzz as
        the render's paths do, up to vertex max_bounces (0 = 8): the four buffers are then of the
        first non-specular vertex, the albedo times the mirrors' on the way and the depth summed
        along the chain, and "bounces" float32 [rows, W] is the mean number of specular vertices
        passed (0: the pixel has the first hit's bits).  It combines with neither emit nor media."""
        if specular and (emit or media):
            raise ValueError("render_aov: specular=True does not combine with emit=True or media=True")
        mode = _aov_mode(emit, media, specular)
        d = camera.derived()
        shape = (len(range(rank, d.height, nranks)), d.width)
        planes = [kc for _, keys in _AOV_MODES[mode][1] for kc in keys]
        res = {k: np.zeros(shape + ((3,) if ch else ()), np.float32) for k, ch in planes}
        res["material"] = np.full(shape, -1, np.int32)  # (the key keeps its place)
        o = self._opts(seed, device, rank, nranks, 0, 0, False, None)
        res["stats"] = self._aov(camera, o, n_samples, mode, False, {k: v.ctypes.data for k, v in res.items()},
                                 (max_bounces, max_fuzz))
        return res

    def _aov(self, camera, o, n_samples, mode, device, ptr, spec_opts):
        """One of the eight rt_render_aov entries, by _AOV_MODES' mode and `device` -> the stats
        dict.  ptr: plane name -> pointer (missing or None: not wanted); spec_opts: the "spec"
        mode's (max_bounces, max_fuzz)."""
        suffix, structs = _AOV_MODES[mode]
        keep = [None if cls is None else cls(*[ptr.get(k) for k, _ in keys]) for cls, keys in structs]
        if mode == "spec":
            keep.insert(0, RtAovSpecOpts(*spec_opts))
        st = RtStats()
        c = camera.to_c()
        fn = getattr(lib(), "rt_render_aov" + suffix + ("_device" if device else ""))
        args = [None if s is None else C.byref(s) for s in keep]
        check(fn(self._p, C.byref(c), C.byref(o), n_samples, *args, C.byref(st)))
        return _as_dict(st)

    def render_aov_device(self, camera, albedo=None, normal=None, depth=None, material=None,
                          n_samples=1, seed=1, device=0, rank=0, nranks=1, stream=None,
                          emission=None, surface_albedo=None, coverage=None, media=False, scatter=None,
                          specular=False, bounces=None, max_bounces=0, max_fuzz=0.0):
        """rt_render_aov_device: the same buffers written to device pointers (e.g. torch
        tensors' .data_ptr(); None = not wanted) on `stream`.  With any of emission /
        surface_albedo / coverage the call is rt_render_aov_emit_device; with media=True or a
        `scatter` pointer it is rt_render_aov_media_device.  With specular=True or a `bounces`
        pointer it is rt_render_aov_spec_device, which takes none of the emit or media buffers.
        Returns the stats dict."""
        ptr = {"albedo": albedo, "normal": normal, "depth": depth, "material": material, "emission": emission,
               "surface_albedo": surface_albedo, "coverage": coverage, "scatter": scatter, "bounces": bounces}
        emit = any(ptr[k] is not None for k, _ in _EMIT_KEYS)
        media = media or scatter is not None
        specular = specular or bounces is not None
        if specular and (emit or media):
            raise ValueError("render_aov_device: specular does not combine with the emit or media buffers")
        o = self._opts(seed, device, rank, nranks, 0, 0, False, stream)
        return self._aov(camera, o, n_samples, _aov_mode(emit, media, specular), True, ptr, (max_bounces, max_fuzz))

    def accumulator(self, camera, max_passes=0, device=0, rank=0, nranks=1, path_slots=0, chunk=0,
                    profile=False, stream=None, mode="auto", progress_slices=0, features=None,
                    spec_bounces=0, spec_fuzz=0.0):
        """A progressive pass accumulator (rt_accum_create) for this rank's rows of `camera`:
        see Accumulator.  max_passes=0 means 1024.  features="guides" keeps the albedo, normal
        and depth of the passes' own camera samples next to the image sums, "emit" also the
        emission split (rt_accum_set_features): see Accumulator.resolve_aov.  "guides+media" and
        "emit+media" keep the same planes of the samples' first events, constant media traced
        (Scene.render_aov(media=True)), and a scatter plane.  "guides+spec" and "emit+spec" also
        keep the specular chains' normal, depth and bounces (Scene.render_aov(specular=True) with
        max_bounces=spec_bounces, max_fuzz=spec_fuzz): see Accumulator.resolve_aov_spec."""
        return Accumulator(self, camera, max_passes, device, rank, nranks, path_slots, chunk,
                           profile, stream, mode, progress_slices, features, spec_bounces, spec_fuzz)

    def accumulator_shares(self, camera, devices, max_passes=0, features=None, spec_bounces=0, spec_fuzz=0.0,
                           path_slots=0, chunk=0, profile=False, mode="auto"):
        """One frame of `camera` accumulated as len(devices) row-interleaved shares: rank i of
        len(devices) on devices[i] (a device may repeat).  See AccumulatorShares; the other
        arguments are Scene.accumulator's."""
        return AccumulatorShares(self, camera, devices, max_passes, features, spec_bounces, spec_fuzz,
                                 path_slots, chunk, profile, mode)


class Accumulator:
    """The exact running sum of render passes of one camera, kept on the device (rt_accum).

    ``add(seed)`` renders one pass, exactly the samples ``Scene.render(camera, seed=seed)``
    computes, and adds it to per-pixel integer sums, so the resolved image is a function of
    the set of seeds, not of their order, and one pass resolves to ``Scene.render``'s bits.
    ``resolve()`` returns the running mean image and the per-pixel variance of its luminance,
    ``info()`` one error figure for the whole image, ``render_until()`` adds passes until that
    figure is small enough.  A context manager; closing the scene closes its accumulators.

    ``features="guides"`` or ``"emit"`` makes every pass also sum the first-hit features of its
    own camera samples (all of them, for whole and for active-pixel passes): ``resolve_aov()``
    returns their means, the guides of exactly the samples in the image, and
    ``denoise_device()`` then needs no ``aov``.  ``"guides+media"`` / ``"emit+media"`` trace the
    constant media in those feature rays (``Scene.render_aov(media=True)``): the planes are of the
    samples' first events and ``resolve_aov()`` adds ``"scatter"``.  ``"guides+spec"`` /
    ``"emit+spec"`` also sum, in a second fold, the planes of the passes' specular chains
    (``Scene.render_aov(specular=True)``): ``resolve_aov_spec()`` returns them, the planes
    ``Temporal(specular=True)`` looks a mirror's history up with; ``resolve_aov()`` and
    ``denoise_device()`` keep the first-hit guides."""

    FEATURES = {None: 0, "guides": _lib.RT_ACCUM_FEAT_GUIDES,
                "emit": _lib.RT_ACCUM_FEAT_GUIDES | _lib.RT_ACCUM_FEAT_EMIT,
                "guides+media": _lib.RT_ACCUM_FEAT_GUIDES | _lib.RT_ACCUM_FEAT_MEDIA,
                "emit+media": _lib.RT_ACCUM_FEAT_GUIDES | _lib.RT_ACCUM_FEAT_EMIT | _lib.RT_ACCUM_FEAT_MEDIA}
    # ... and with the specular chains' planes (rt_accum_set_features_spec), a table of their own
    SPEC_FEATURES = {"guides+spec": _lib.RT_ACCUM_FEAT_GUIDES | _lib.RT_ACCUM_FEAT_SPEC,
                     "emit+spec": _lib.RT_ACCUM_FEAT_GUIDES | _lib.RT_ACCUM_FEAT_EMIT | _lib.RT_ACCUM_FEAT_SPEC}

    def __init__(self, scene, camera, max_passes=0, device=0, rank=0, nranks=1, path_slots=0,
                 chunk=0, profile=False, stream=None, mode="auto", progress_slices=0, features=None,
                 spec_bounces=0, spec_fuzz=0.0):
        self._p = None
        self._device, self._mean, self._var = device, None, None  # denoise_device's tensors
        self._aov = None  # resolve_aov_device's
        self._aov_spec = None  # resolve_aov_spec_device's
        if features not in self.FEATURES and features not in self.SPEC_FEATURES:
            raise ValueError("Accumulator: features must be None, 'guides', 'emit', 'guides+media', "
                             f"'emit+media', 'guides+spec' or 'emit+spec', not {features!r}")
        spec = features in self.SPEC_FEATURES
        if not spec and (spec_bounces or spec_fuzz):
            raise ValueError("Accumulator: spec_bounces and spec_fuzz are options of features='guides+spec' "
                             "or 'emit+spec'")
        d = camera.derived()
        self.shape = (len(range(rank, d.height, nranks)), d.width)
        c = camera.to_c()
        self.camera, self.nranks = Camera.from_c(c), nranks  # the camera as it is now: a copy
        o = Scene._opts(0, device, rank, nranks, path_slots, chunk, profile, stream, mode)
        o.progress_slices = progress_slices
        p = C.c_void_p()
        check(lib().rt_accum_create(scene._p, C.byref(c), C.byref(o), max_passes, C.byref(p)))
        self._p = p
        self._destroy = lib().rt_accum_destroy  # usable at interpreter shutdown
        self.scene = scene
        scene._accums.add(self)
        if features is not None:
            try:
                if spec:
                    so = RtAovSpecOpts(int(spec_bounces), float(spec_fuzz))
                    check(lib().rt_accum_set_features_spec(self._p, self.SPEC_FEATURES[features], C.byref(so)))
                else:
                    check(lib().rt_accum_set_features(self._p, self.FEATURES[features]))
            except BaseException:
                self.close()
                raise

    def close(self):
        if getattr(self, "_p", None):
            self._destroy(self._p)
            self._p = None

    @property
    def features(self):
        """None, "guides", "emit", "guides+media", "emit+media", "guides+spec" or "emit+spec": the
        feature planes the passes keep (rt_accum_get_features)."""
        m = C.c_uint32()
        check(lib().rt_accum_get_features(self._h(), C.byref(m)))
        return {v: k for k, v in {**self.FEATURES, **self.SPEC_FEATURES}.items()}.get(m.value, m.value)

    def _aov_keys(self):
        f = self.features
        if f is None:
            raise ValueError("Accumulator: no feature planes (Scene.accumulator(features=...))")
        f = str(f)
        return (("albedo", "normal", "depth")
                + (("emission", "surface_albedo", "coverage") if f.startswith("emit") else ())
                + (("scatter",) if f.endswith("+media") else ()))

    @staticmethod
    def _aov_args(keys, ptr):
        """rt_accum_resolve_aov's or, with a scatter plane, rt_accum_resolve_aov_media's arguments
        for the planes `keys`, ptr(key) -> the plane's address; (the _media entry?, the arguments)"""
        a = RtAov(*[ptr(k) for k in keys[:3]], None)
        e = RtAovEmit(*[ptr(k) for k in keys[3:6]]) if "coverage" in keys else None
        args = (C.byref(a), None if e is None else C.byref(e))
        if "scatter" not in keys:
            return False, args, (a, e)
        m = RtAovMedia(ptr("scatter"))
        return True, args + (C.byref(m),), (a, e, m)

    def resolve_aov(self):
        """The feature buffers of exactly the camera samples the passes rendered
        (rt_accum_resolve_aov): {"albedo", "normal", "depth"}, with features="emit" also
        {"emission", "surface_albedo", "coverage"} and with "+media" also {"scatter"}
        (rt_accum_resolve_aov_media), float32 arrays shaped as
        Scene.render_aov's: per pixel the mean over its passes' samples, zeros without a pass."""
        keys = self._aov_keys()
        res = {k: np.zeros(self.shape + ((3,) if k not in ("depth", "coverage", "scatter") else ()), np.float32)
               for k in keys}
        media, args, _keep = self._aov_args(keys, lambda k: res[k].ctypes.data)
        check((lib().rt_accum_resolve_aov_media if media else lib().rt_accum_resolve_aov)(self._h(), *args))
        return res

    def resolve_aov_device(self):
        """resolve_aov() into torch tensors on the accumulator's device, which the accumulator
        owns (allocated on first use, overwritten by the next call)."""
        import torch
        keys = self._aov_keys()
        if self._aov is None or tuple(self._aov) != keys:
            dev = torch.device("cuda", self._device)
            self._aov = {k: torch.empty(self.shape + ((3,) if k not in ("depth", "coverage", "scatter") else ()),
                                        dtype=torch.float32, device=dev) for k in keys}
        t = self._aov
        media, args, _keep = self._aov_args(keys, lambda k: t[k].data_ptr())
        check((lib().rt_accum_resolve_aov_media_device if media else lib().rt_accum_resolve_aov_device)(
            self._h(), *args))
        return t

    def _spec_check(self):
        if not str(self.features).endswith("+spec"):
            raise ValueError("Accumulator: no chain planes (Scene.accumulator(features='guides+spec' or "
                             f"'emit+spec')), features={self.features!r}")

    def resolve_aov_spec(self):
        """The specular chains' planes of exactly the camera samples the passes rendered
        (rt_accum_resolve_aov_spec): {"normal", "depth", "bounces"} as
        Scene.render_aov(specular=True) gives them, per pixel the mean over its passes' samples
        (bounces exactly: a pixel whose samples all passed k vertices has float32(k)), zeros
        without a pass.  Needs features "guides+spec" or "emit+spec"."""
        self._spec_check()
        res = {"normal": np.zeros(self.shape + (3,), np.float32), "depth": np.zeros(self.shape, np.float32),
               "bounces": np.zeros(self.shape, np.float32)}
        a = RtAov(None, res["normal"].ctypes.data, res["depth"].ctypes.data, None)
        sp = RtAovSpec(res["bounces"].ctypes.data)
        check(lib().rt_accum_resolve_aov_spec(self._h(), C.byref(a), C.byref(sp)))
        return res

    def resolve_aov_spec_device(self):
        """resolve_aov_spec() into torch tensors on the accumulator's device, which the accumulator
        owns (allocated on first use, overwritten by the next call)."""
        import torch
        self._spec_check()
        if self._aov_spec is None:
            dev = torch.device("cuda", self._device)
            self._aov_spec = {k: torch.empty(self.shape + ((3,) if k == "normal" else ()), dtype=torch.float32,
                                             device=dev) for k in ("normal", "depth", "bounces")}
        t = self._aov_spec
        a = RtAov(None, t["normal"].data_ptr(), t["depth"].data_ptr(), None)
        sp = RtAovSpec(t["bounces"].data_ptr())
        check(lib().rt_accum_resolve_aov_spec_device(self._h(), C.byref(a), C.byref(sp)))
        return t

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _h(self):
        if not self._p:
            raise ValueError("Accumulator is closed")
        return self._p

    def add(self, seed):
        """One pass with render seed `seed` (rt_accum_add) -> the pass's stats dict."""
        st = RtStats()
        check(lib().rt_accum_add(self._h(), seed, C.byref(st)))
        return _as_dict(st)

    def resolve(self):
        """(rgb float32 [rows, W, 3]: the mean of all passes, var float32 [rows, W]: the
        variance of its luminance, 0 before the second pass)."""
        rgb = np.zeros(self.shape + (3,), np.float32)
        var = np.zeros(self.shape, np.float32)
        check(lib().rt_accum_resolve(self._h(), rgb.ctypes.data, var.ctypes.data))
        return rgb, var

    def resolve_device(self, rgb_tensor, var_tensor=None):
        """rt_accum_resolve_device into contiguous float32 torch tensors on the accumulator's
        device: rgb [rows, W, 3] (or None) and var [rows, W] (or None)."""
        import torch
        for t, shape in ((rgb_tensor, self.shape + (3,)), (var_tensor, self.shape)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()
                                  or tuple(t.shape) != shape or not t.is_cuda):
                raise ValueError(f"resolve_device: needs a contiguous float32 device tensor of shape {shape}")
        check(lib().rt_accum_resolve_device(
            self._h(), None if rgb_tensor is None else rgb_tensor.data_ptr(),
            None if var_tensor is None else var_tensor.data_ptr()))

    _OWN_GUIDES = object()  # denoise_device's default aov

    def denoise_device(self, aov=_OWN_GUIDES, out=None, var_out=None, split_emitters=None, **opts):
        """The running mean through the variance-guided denoiser, all on the device: resolves
        into tensors the accumulator owns (allocated on first use, then reused) and runs
        denoise_var_device(mean, var, aov, out, var_out, **opts).  Returns `out` (a new tensor by
        default).  Needs two passes: one pass has no variance.  split_emitters=True: the
        emission split (aov from render_aov_device's emission / surface_albedo / coverage).
        Without an aov, an accumulator with features uses its own guides
        (resolve_aov_device()), and split_emitters then defaults to on with features="emit";
        without features that is a ValueError.  An explicit aov=None on an accumulator without
        features still means the unguided filter."""
        import torch
        own = aov is None or aov is self._OWN_GUIDES
        if own and self.features is None:
            if aov is not None:
                raise ValueError("Accumulator.denoise_device: needs aov, or an accumulator with features")
            own = False
        if own and split_emitters is None:
            split_emitters = str(self.features).startswith("emit")
        split_emitters = bool(split_emitters)
        if self.passes < 2:
            raise ValueError("Accumulator.denoise_device: needs at least 2 passes (no variance yet)")
        if own:
            aov = self.resolve_aov_device()
        if self._mean is None:
            dev = torch.device("cuda", self._device)
            self._mean = torch.empty(self.shape + (3,), dtype=torch.float32, device=dev)
            self._var = torch.empty(self.shape, dtype=torch.float32, device=dev)
        self.resolve_device(self._mean, self._var)
        return denoise_var_device(self._mean, self._var, aov, out=out, var_out=var_out,
                                  split_emitters=split_emitters, **opts)

    def info(self):
        """rt_accum_info as a dict: passes, max_passes, samples_per_pixel, nonfinite_pixels,
        rms_std_error, mean_luminance, rel_error."""
        i = RtAccumInfo()
        check(lib().rt_accum_info_get(self._h(), C.byref(i)))
        return _as_dict(i)

    def reset(self):
        check(lib().rt_accum_reset(self._h()))

    @property
    def passes(self):
        return self.info()["passes"]

    def render_until(self, rel_error, max_passes, seed=1):
        """Add passes with seeds seed, seed + 1, ... (pass number p of the accumulator takes
        seed + p, so a second call goes on where the first stopped) until
        info()["rel_error"] <= rel_error (checked from the second pass on: one pass has no
        variance) or the accumulator holds max_passes passes.  Returns the last info()."""
        i = self.info()
        while i["passes"] < max_passes:
            self.add(seed + i["passes"])
            i = self.info()
            if i["passes"] >= 2 and i["rel_error"] <= rel_error:
                break
        return i

    # ---- adaptive passes: resample only the noisy tiles
    def select(self, rel_error, lum_floor=0, tile=0, min_passes=0):
        """rt_accum_select: the pixels of the tiles whose error figure e_T exceeds `rel_error`
        (or that hold a pixel with fewer than `min_passes` passes) become the selection of the
        next add_active().  0 takes a default: lum_floor 1e-2, tile 8, min_passes 4.  Returns
        the number of active pixels."""
        o = _lib.RtAdaptOpts(rel_error, lum_floor, tile, min_passes)
        n = C.c_uint64()
        check(lib().rt_accum_select(self._h(), C.byref(o), C.byref(n)))
        return n.value

    def set_active(self, mask):
        """rt_accum_set_active: the selection from a [rows, W] mask (nonzero = active).
        Returns the number of active pixels."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != self.shape:
            raise ValueError(f"set_active: needs a mask of shape {self.shape}")
        n = C.c_uint64()
        check(lib().rt_accum_set_active(self._h(), m.ctypes.data, C.byref(n)))
        return n.value

    def add_active(self, seed):
        """One pass over the current selection only (rt_accum_add_active): every selected pixel
        gets exactly the samples add(seed) would give it.  Returns the pass's stats dict."""
        st = RtStats()
        check(lib().rt_accum_add_active(self._h(), seed, C.byref(st)))
        return _as_dict(st)

    def counts(self):
        """int32 [rows, W]: the passes every pixel has taken (rt_accum_counts)."""
        c = np.zeros(self.shape, np.int32)
        check(lib().rt_accum_counts(self._h(), c.ctypes.data))
        return c

    def tile_error(self, lum_floor=0, tile=0, min_passes=0):
        """float32 [tiles_y, tiles_x]: e_T of every tile, as select() compares it
        (rt_accum_tile_error)."""
        o = _lib.RtAdaptOpts(1.0, lum_floor, tile, min_passes)
        tx, ty = C.c_int32(), C.c_int32()
        check(lib().rt_accum_tile_error(self._h(), C.byref(o), None, C.byref(tx), C.byref(ty)))
        e = np.zeros((ty.value, tx.value), np.float32)
        check(lib().rt_accum_tile_error(self._h(), C.byref(o), e.ctypes.data, C.byref(tx), C.byref(ty)))
        return e

    def adapt_info(self):
        """rt_adapt_info as a dict: active_pixels, total_samples, min_count, max_count, n_tiles,
        active_tiles."""
        i = _lib.RtAdaptInfo()
        check(lib().rt_accum_adapt_info(self._h(), C.byref(i)))
        return _as_dict(i)

    def render_adaptive(self, rel_error, max_passes, seed=1, **opts):
        """select() / add_active() until the selection is empty or the accumulator holds
        max_passes passes.  While some pixel has fewer than min_passes passes every tile is
        selected, so the first min_passes passes are whole passes (add_active then takes
        add()'s path).  Pass number p takes seed + p, as render_until.  opts: select()'s
        lum_floor, tile, min_passes.  Returns adapt_info() with "passes" added."""
        p = self.info()["passes"]
        while p < max_passes and self.select(rel_error, **opts) > 0:
            self.add_active(seed + p)
            p += 1
        return dict(self.adapt_info(), passes=p)


def _share_array(accs):
    """rt_accum* const* for the share entries, and the handles it points at"""
    hs = [a._h() for a in accs]
    return (C.c_void_p * len(hs))(*[h.value for h in hs]), len(hs)


class AccumulatorShares:
    """The accumulators of one frame held as row shares: ``shares[i]`` is the
    Accumulator of rank i of n on ``devices[i]``.  ``add(seed)`` takes one pass on every share, a
    host thread each (rt_accum_add_shares), and returns the combined stats; each share ends up with
    exactly the state its own ``add(seed)`` leaves.  ``resolve()`` interleaves the shares' rows on
    the host; ``Pipeline.push`` takes the object as one frame.  A context manager owning its
    accumulators."""

    def __init__(self, scene, camera, devices, max_passes=0, features=None, spec_bounces=0, spec_fuzz=0.0,
                 path_slots=0, chunk=0, profile=False, mode="auto"):
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("AccumulatorShares: needs at least one device")
        self.shares, self.devices = [], devices
        self.height = camera.derived().height
        try:
            for i, d in enumerate(devices):
                self.shares.append(Accumulator(scene, camera, max_passes, d, i, len(devices), path_slots, chunk,
                                               profile, None, mode, 0, features, spec_bounces, spec_fuzz))
        except BaseException:
            self.close()
            raise

    def close(self):
        for a in getattr(self, "shares", ()):
            a.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __len__(self):
        return len(self.shares)

    def add(self, seed):
        """One pass with render seed `seed` on every share -> the combined stats dict."""
        arr, n = _share_array(self.shares)
        st = RtStats()
        check(lib().rt_accum_add_shares(arr, n, seed, C.byref(st)))
        return _as_dict(st)

    @property
    def passes(self):
        return self.shares[0].passes

    def resolve(self):
        """(rgb float32 [H, W, 3], var float32 [H, W]) of the whole image: the shares' resolve()
        rows interleaved (row r is local row r // n of share r % n)."""
        from .shard import rows_of_rank
        n, w = len(self.shares), self.shares[0].shape[1]
        rgb, var = np.zeros((self.height, w, 3), np.float32), np.zeros((self.height, w), np.float32)
        for i, a in enumerate(self.shares):
            rows = list(rows_of_rank(self.height, i, n))
            rgb[rows], var[rows] = a.resolve()
        return rgb, var


def _multi(scene, camera, devices, out_ptr, seed, path_slots, chunk, profile, mode, rccl=False):
    devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    st = RtStats()
    c = camera.to_c()
    o = scene._opts(seed, int(devices[0]) if len(devices) else 0, 0, 1, path_slots, chunk,
                    profile, None, mode)
    if rccl:
        o.flags |= _lib.RT_FLAG_GATHER_RCCL
    fn = lib().rt_render_multi_device if out_ptr[1] else lib().rt_render_multi
    check(fn(scene._p, C.byref(c), C.byref(o), devs, len(devices), C.c_void_p(out_ptr[0]),
             C.byref(st)))
    return _as_dict(st)


def demo_scene(name, seed=1, asset_dir=None):
    """Build a main.go scene -> (tree, camera, world, lights)."""
    import os
    if asset_dir is None:
        asset_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                 "assets")
    t = Tree(seed)
    cam = RtCamera()
    w, l = C.c_int(), C.c_int()
    check(lib().rt_demo_scene(t.ptr, name.encode(), asset_dir.encode(), C.byref(cam), C.byref(w),
                              C.byref(l)))
    return t, Camera.from_c(cam), w.value, l.value


def build_bvh_boxes(boxes, builder=0):
    """A tree over caller-supplied boxes (rt_bvh_build_boxes, a structural test export):
    `boxes` float32 [n, 6] (lo xyz, hi xyz), builder 0 = host binned SAH, 1 = device PLOC.
    Returns {"nodes": float32 [N, 16], "refs": uint32 [n] (leaf position -> box index), "root",
    "nodes4": uint32 [M, 32], "root4", "bvh_depth", "max_leaf"}, the arrays as
    Scene.export_bvh / export_qbvh give them."""
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    if b.ndim != 2 or b.shape[1] != 6:
        raise ValueError(f"build_bvh_boxes: boxes must have shape [n, 6], not {b.shape}")
    n = b.shape[0]
    cap = max(n - 1, 0)  # no tree over n boxes has more inner nodes
    nodes, nodes4 = np.zeros((cap, 16), np.float32), np.zeros((cap, 32), np.uint32)
    refs = np.zeros(n, np.uint32)
    nn, nr, n4, depth, leaf = (C.c_int32() for _ in range(5))
    root, root4 = C.c_uint32(), C.c_uint32()
    check(lib().rt_bvh_build_boxes(b.ctypes.data or None, n, int(builder), nodes.ctypes.data or None,
                                   C.byref(nn), refs.ctypes.data or None, C.byref(nr), C.byref(root),
                                   nodes4.ctypes.data or None, C.byref(n4), C.byref(root4),
                                   C.byref(depth), C.byref(leaf)))
    assert nn.value <= cap and n4.value <= cap and nr.value == n
    return {"nodes": nodes[:nn.value], "refs": refs, "root": int(root.value),
            "nodes4": nodes4[:n4.value], "root4": int(root4.value),
            "bvh_depth": depth.value, "max_leaf": leaf.value}


def substitute_mesh_obj(nu=0, nv=0):
    """The "model" scene's dragon.obj substitute as OBJ bytes (rt_substitute_mesh_obj)."""
    n = check(int(lib().rt_substitute_mesh_obj(nu, nv, None, 0)))
    buf = C.create_string_buffer(n)
    check(int(lib().rt_substitute_mesh_obj(nu, nv, buf, n)))
    return buf.raw[:n]


def quantize(rgb):
    """PrintColor (vec/color.go:23-46) on a float32 [..., 3] image -> uint8."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.zeros(a.shape, np.uint8)
    check(lib().rt_quantize(a.ctypes.data, a.size // 3, out.ctypes.data))
    return out


def format_ppm(rgb):
    """PPM P3 text exactly as the reference writes it (camera.go:160 + PrintColor)."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = a.shape[:2]
    n = lib().rt_format_ppm(a.ctypes.data, w, h, None, 0)
    check(int(n))
    buf = C.create_string_buffer(int(n))
    check(int(lib().rt_format_ppm(a.ctypes.data, w, h, buf, n)))
    return buf.raw[:n]


def _stream_of(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def quantize_device(rgb):
    """PrintColor on a device float32 [..., 3] torch tensor -> device uint8 tensor
    (HIP kernel, rt_quantize_device)."""
    import torch
    a = rgb.contiguous().to(torch.float32)
    out = torch.empty(a.shape, dtype=torch.uint8, device=a.device)
    check(lib().rt_quantize_device(a.data_ptr(), a.numel() // 3, out.data_ptr(),
                                   a.device.index or 0, _stream_of(a)))
    return out


def format_ppm_device(rgb, to_host=True):
    """The P3 text of camera.go:160 built on the GPU from a device float32
    [H, W, 3] tensor (rt_format_ppm_device).  Returns bytes, or the device
    uint8 tensor when to_host is False."""
    import torch
    a = rgb.contiguous().to(torch.float32)
    h, w = a.shape[:2]
    dev, st = a.device.index or 0, _stream_of(a)
    n = int(lib().rt_format_ppm_device(a.data_ptr(), w, h, None, 0, dev, st))
    check(n)
    out = torch.empty(n, dtype=torch.uint8, device=a.device)
    check(int(lib().rt_format_ppm_device(a.data_ptr(), w, h, out.data_ptr(), n, dev, st)))
    return out.cpu().numpy().tobytes() if to_host else out


def _denoise_opts(var, iterations=0, demodulate=None, sigma_normal=0.0, sigma_depth=0.0,
                  has_albedo=False, **sigma):
    """RtDenoiseVarOpts (its colour sigma: sigma_lum) with a variance, else RtDenoiseOpts
    (sigma_color)"""
    o = RtDenoiseVarOpts() if var else RtDenoiseOpts()
    o.iterations = iterations
    o.demodulate = int(has_albedo if demodulate is None else demodulate)
    o.sigma_normal, o.sigma_depth = sigma_normal, sigma_depth
    key = "sigma_lum" if var else "sigma_color"
    setattr(o, key, sigma.pop(key, 0.0))
    if sigma:
        raise TypeError(f"_denoise_opts() got an unexpected keyword argument {next(iter(sigma))!r}")
    return o


_EMIT_KEYS = (("emission", 3), ("surface_albedo", 3), ("coverage", 0))
_OUT = (RtAov, (("albedo", 3), ("normal", 3), ("depth", 0), ("material", 0)))
_EMIT = (RtAovEmit, _EMIT_KEYS)
_MEDIA = (RtAovMedia, (("scatter", 0),))
# The feature pass's modes (Scene.render_aov, render_aov_device): the suffix of the mode's
# rt_render_aov entries and the pointer structs they take, each with its planes (name, channels)
# in field order.  (None: a NULL struct.)
_AOV_MODES = {"first": ("", (_OUT,)),
              "emit": ("_emit", (_OUT, _EMIT)),
              "media": ("_media", (_OUT, (None, ()), _MEDIA)),
              "emit+media": ("_media", (_OUT, _EMIT, _MEDIA)),
              "spec": ("_spec", (_OUT, (RtAovSpec, (("bounces", 0),))))}


def _aov_mode(emit, media, specular):
    return "spec" if specular else "+".join(m for m, on in (("emit", emit), ("media", media)) if on) or "first"


def _emit_host(who, aov, h, w):
    """split_emitters on host arrays: (RtAovEmit, the arrays it points into)"""
    keep = []
    for k, ch in _EMIT_KEYS:
        if (aov or {}).get(k) is None:
            raise ValueError(f"{who}: split_emitters needs aov[{k!r}] (Scene.render_aov(emit=True))")
        t = np.ascontiguousarray(aov[k], dtype=np.float32)
        shape = (h, w, ch) if ch else (h, w)
        if t.shape != shape:
            raise ValueError(f"{who}: {k} must have shape {shape}, not {t.shape}")
        keep.append(t)
    return RtAovEmit(*[t.ctypes.data for t in keep]), keep


def _emit_device(who, aov, a):
    """split_emitters on device tensors: the checks denoise_var_device applies to var"""
    import torch
    h, w = a.shape[:2]
    keep = []
    for k, ch in _EMIT_KEYS:
        t = (aov or {}).get(k)
        if t is None:
            raise ValueError(f"{who}: split_emitters needs aov[{k!r}] (render_aov_device's {k})")
        shape = (h, w, ch) if ch else (h, w)
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous()
                or tuple(t.shape) != shape or t.device != a.device):
            raise ValueError(f"{who}: {k} must be a contiguous float32 tensor of shape {shape} "
                             "on rgb's device")
        keep.append(t)
    return RtAovEmit(*[t.data_ptr() for t in keep]), keep


def _denoise_host(has_var, rgb, var, aov, return_var, split_emitters, opts):
    """denoise and denoise_var (has_var): rt_denoise[_var][_emit] on host arrays"""
    who = "denoise_var" if has_var else "denoise"
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = a.shape[:2]
    if has_var:
        if var is None:
            raise ValueError("denoise_var: var is required")
        v = np.ascontiguousarray(var, dtype=np.float32)
        if v.shape != (h, w):
            raise ValueError(f"denoise_var: var must have shape {(h, w)}, not {v.shape}")
    aov = aov or {}
    if split_emitters:
        e, _keep = _emit_host(who, aov, h, w)
    keep = [None if aov.get(k) is None else np.ascontiguousarray(aov[k], dtype=np.float32)
            for k in ("albedo", "normal", "depth")]
    f = RtAov(*[None if k is None else k.ctypes.data for k in keep], None)
    o = _denoise_opts(has_var, has_albedo=split_emitters or keep[0] is not None, **opts)
    out = np.empty_like(a)
    vout = np.empty_like(v) if return_var else None
    fn = getattr(lib(), "rt_denoise" + "_var" * has_var + "_emit" * split_emitters)
    check(fn(a.ctypes.data, *([v.ctypes.data] if has_var else []), C.byref(f),
             *([C.byref(e)] if split_emitters else []), w, h, C.byref(o), out.ctypes.data,
             *([None if vout is None else vout.ctypes.data] if has_var else [])))
    return (out, vout) if return_var else out


def _denoise_dev(has_var, rgb, var, aov, out, var_out, split_emitters, opts):
    """denoise_device and denoise_var_device (has_var): rt_denoise[_var][_emit]_device on torch
    tensors"""
    import torch
    who = "denoise_var_device" if has_var else "denoise_device"
    a = rgb if (rgb.is_contiguous() and rgb.dtype == torch.float32) else \
        rgb.contiguous().to(torch.float32)
    h, w = a.shape[:2]
    for name, t in (("var", var), ("var_out", var_out)) if has_var else ():
        if name == "var_out" and t is None:
            continue
        if (t is None or not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous()
                or tuple(t.shape) != (h, w) or t.device != a.device):
            raise ValueError(f"{who}: {name} must be a contiguous float32 tensor of shape "
                             f"{(h, w)} on rgb's device")
    aov = aov or {}
    if split_emitters:
        e, _keep = _emit_device(who, aov, a)
    keep = [None if aov.get(k) is None else aov[k].contiguous().to(torch.float32)
            for k in ("albedo", "normal", "depth")]
    f = RtAov(*[None if k is None else k.data_ptr() for k in keep], None)
    o = _denoise_opts(has_var, has_albedo=split_emitters or keep[0] is not None, **opts)
    if out is None:
        out = torch.empty_like(a)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.shape != a.shape
          or out.device != a.device):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor of rgb's shape "
                         "on rgb's device")
    elif out is rgb and a is not rgb:
        raise ValueError(f"{who}: in place needs a contiguous float32 rgb")
    fn = getattr(lib(), "rt_denoise" + "_var" * has_var + "_emit" * split_emitters + "_device")
    check(fn(a.data_ptr(), *([var.data_ptr()] if has_var else []), C.byref(f),
             *([C.byref(e)] if split_emitters else []), w, h, C.byref(o), out.data_ptr(),
             *([None if var_out is None else var_out.data_ptr()] if has_var else []),
             a.device.index or 0, _stream_of(a)))
    return out


def denoise(rgb, aov=None, split_emitters=False, **opts):
    """Edge-avoiding a-trous denoise (rt_denoise) of a host float32 [H, W, 3] image guided by
    `aov`, a dict as Scene.render_aov returns it (any of "albedo", "normal", "depth"; None or
    missing = that guide off).  opts: iterations (0 = 5), demodulate (default: on when an
    albedo is given), sigma_color / sigma_normal / sigma_depth (0 = the library defaults).
    split_emitters=True (rt_denoise_emit): aov must also hold "emission", "surface_albedo" and
    "coverage" (Scene.render_aov(emit=True)); the emission is kept out of the filter, which
    demodulates by surface_albedo ("albedo" is not read).  Returns a new float32 [H, W, 3]
    array."""
    return _denoise_host(False, rgb, None, aov, False, split_emitters, opts)


def denoise_device(rgb, aov=None, out=None, split_emitters=False, **opts):
    """rt_denoise_device on device float32 torch tensors: rgb [H, W, 3], aov a dict of
    "albedo" [H, W, 3] / "normal" [H, W, 3] / "depth" [H, W] tensors on the same device.
    `out` may be rgb itself (in place); by default a new tensor.  split_emitters=True
    (rt_denoise_emit_device): aov must also hold "emission" [H, W, 3], "surface_albedo"
    [H, W, 3] and "coverage" [H, W] as contiguous float32 tensors on rgb's device.  Runs on the
    tensor's current stream and returns after the work completes."""
    return _denoise_dev(False, rgb, None, aov, out, None, split_emitters, opts)


def denoise_var(rgb, var, aov=None, return_var=False, split_emitters=False, **opts):
    """Variance-guided a-trous denoise (rt_denoise_var) of a host float32 [H, W, 3] image and
    the variance [H, W] of its mean luminance, as Accumulator.resolve returns them, guided by
    `aov` as denoise is.  opts: iterations (0 = 5), demodulate (default: on when an albedo is
    given), sigma_lum (0 = 1.0) / sigma_normal / sigma_depth.  Returns a new float32
    [H, W, 3] array, or with return_var (out, var_out [H, W]: the variance of the filtered
    image's luminance).  split_emitters=True (rt_denoise_var_emit): as denoise's."""
    return _denoise_host(True, rgb, var, aov, return_var, split_emitters, opts)


def denoise_var_device(rgb, var, aov=None, out=None, var_out=None, split_emitters=False, **opts):
    """rt_denoise_var_device on device float32 torch tensors: rgb [H, W, 3], var [H, W]
    (contiguous float32 on rgb's device), aov as denoise_device's.  `out` may be rgb itself and
    `var_out` (None: the filtered variance is not written) var itself.  split_emitters=True
    (rt_denoise_var_emit_device): as denoise_device's.  Runs on the tensor's current stream and
    returns `out` after the work completes."""
    return _denoise_dev(True, rgb, var, aov, out, var_out, split_emitters, opts)


_FRAME_KEYS = (("rgb", 3), ("var", 0), ("count", 0), ("normal", 3), ("depth", 0))


def _reproject_opts(max_history=0.0, depth_tol=0.0, normal_tol=0.0, min_weight=0.0):
    return _lib.RtReprojectOpts(max_history, depth_tol, normal_tol, min_weight)


def _frame(who, name, f, h, w, conv, ptr):
    """An RtFrame over the dict `f` ("rgb", "normal", "depth"; optional "var" and "count", the
    count an array or one number for every pixel) -> (RtFrame, the arrays it points into).
    conv(key, value, shape) checks or converts one buffer, ptr(buffer) is its address."""
    if not isinstance(f, dict):
        raise ValueError(f"{who}: {name} must be a dict of rgb, normal, depth (and var, count)")
    keep, ptrs, scalar = [], [], 0.0
    for k, ch in _FRAME_KEYS:
        t = f.get(k)
        if k == "count" and isinstance(t, (int, float)):
            t, scalar = None, float(t)
        if t is None:
            if k in ("rgb", "normal", "depth"):
                raise ValueError(f"{who}: {name}[{k!r}] is required")
            ptrs.append(None)
            continue
        t = conv(f"{name}[{k!r}]", t, (h, w, ch) if ch else (h, w))
        keep.append(t)
        ptrs.append(ptr(t))
    return _lib.RtFrame(*ptrs, scalar, 0), keep


def _frame_emit(who, name, f, h, w, conv, ptr):
    """The RtAovEmit of a frame dict for the _emit entries: "emission" [H, W, 3] and "coverage"
    [H, W] are required (surface_albedo is not read: NULL) -> (RtAovEmit, the buffers)"""
    keep = []
    for k, ch in (("emission", 3), ("coverage", 0)):
        if f.get(k) is None:
            raise ValueError(f"{who}: {name}[{k!r}] is required (an accumulator with features='emit', "
                             "resolve_aov / resolve_aov_device)")
        keep.append(conv(f"{name}[{k!r}]", f[k], (h, w, ch) if ch else (h, w)))
    return RtAovEmit(ptr(keep[0]), None, ptr(keep[1])), keep


_LIGHT_KEYS = (("emission", 3), ("coverage", 0))


_MOMENT_MODES = {"plain": 0, "emit": 1, "light": 2, 0: 0, 1: 1, 2: 2}


def _moments_opts(min_frames=0.0, var_radius=0):
    return _lib.RtMomentsOpts(float(min_frames), int(var_radius))


def _host_buffers(who, cur):
    """The host entries' buffers: (h, w, conv, ptr, new) for _frame over numpy arrays of the size
    of cur["rgb"]; new(shape) is a new float32 array"""
    if not isinstance(cur, dict) or cur.get("rgb") is None:
        raise ValueError(f"{who}: cur['rgb'] is required")
    h, w = np.shape(cur["rgb"])[:2]

    def conv(name, t, shape):
        a = np.ascontiguousarray(t, dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{who}: {name} must have shape {shape}, not {a.shape}")
        return a
    return h, w, conv, (lambda a: a.ctypes.data), (lambda shape: np.empty(shape, np.float32))


def _device_buffers(who, cur):
    """The device entries' buffers: _host_buffers' tuple over torch tensors on cur["rgb"]'s device"""
    import torch
    if not isinstance(cur, dict) or not torch.is_tensor(cur.get("rgb")) or cur["rgb"].dim() != 3:
        raise ValueError(f"{who}: cur['rgb'] must be a [H, W, 3] tensor")
    a = cur["rgb"]
    h, w = a.shape[:2]

    def conv(name, t, shape):
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous()
                or tuple(t.shape) != shape or t.device != a.device):
            raise ValueError(f"{who}: {name} must be a contiguous float32 tensor of shape {shape} "
                             "on cur['rgb']'s device")
        return t

    def new(shape):
        return torch.empty(shape, dtype=torch.float32, device=a.device)
    return h, w, conv, (lambda t: t.data_ptr()), new


def _reproject_call(family, device, mode, cam_prev, prev, cam_cur, cur, out, opts, min_frames=0.0, var_radius=0,
                    gamma=None):
    """The twelve reproject functions: rt_reproject[_emit | _light | _moments | _clip | _spec][_device]
    by `family` ("plain", "emit", "light", whose mode is their own, or "moments", "clip", "spec" in
    the caller's mode) on host arrays or, with device, torch tensors.  gamma None: copts == NULL"""
    mom = family in ("moments", "clip", "spec")
    who = "reproject" + ("" if family == "plain" else "_" + family) + ("_device" if device else "")
    if not mom:
        mode = ("plain", "emit", "light").index(family)
    elif isinstance(mode, bool) or mode not in _MOMENT_MODES:
        raise ValueError(f"{who}: mode must be 'plain', 'emit' or 'light' (or 0, 1, 2), not {mode!r}")
    else:
        mode = _MOMENT_MODES[mode]
    emit, light = mode >= 1, mode == 2
    h, w, conv, ptr, new = (_device_buffers if device else _host_buffers)(who, cur)
    # the frames' structs.  The moments family checks frame by frame, cur first, and takes prev=None
    # (no history at all); the older entries check both frames, then both emit structs
    frames = {"prev": prev, "cur": cur}
    kinds = (_frame, _frame_emit) if emit else (_frame,)
    if mom:
        steps = [(s, kind) for s in ("cur", "prev") if frames[s] is not None for kind in kinds]
    else:
        steps = [(s, kind) for kind in kinds for s in ("prev", "cur")]
    c = {}  # (frame, kind) -> its struct
    keep = {"prev": [], "cur": []}  # the buffers the structs point into
    for s, kind in steps:
        if mom and s == "prev" and kind is _frame and cam_prev is None:
            raise ValueError(f"{who}: prev without cam_prev")
        c[s, kind], bufs = kind(who, s, frames[s], h, w, conv, ptr)
        keep[s] += bufs
    lp = sp = None
    if mom and prev is not None:
        if prev.get("lum2") is None:
            raise ValueError(f"{who}: prev['lum2'] is required (the lum2 plane an earlier call returned)")
        keep["prev"].append(conv("prev['lum2']", prev["lum2"], (h, w)))
        lp = ptr(keep["prev"][-1])
    if family == "spec":  # the frames' chain lengths: inputs as the rest, never an out buffer
        if cur.get("bounces") is None:
            raise ValueError(f"{who}: cur['bounces'] is required (resolve_aov_spec / resolve_aov_spec_device)")
        keep["cur"].append(conv("cur['bounces']", cur["bounces"], (h, w)))
        sp = _lib.RtSpecPlanes(None, ptr(keep["cur"][-1]))
        if prev is not None:
            if prev.get("bounces") is None:
                raise ValueError(f"{who}: prev['bounces'] is required (the bounces plane of the previous frame)")
            keep["prev"].append(conv("prev['bounces']", prev["bounces"], (h, w)))
            sp.prev_bounces = ptr(keep["prev"][-1])
    res = []
    taken = {s: {ptr(p) for p in keep[s]} if device else () for s in keep}  # (a host call's out arrays are new)
    for k, ch in _FRAME_KEYS[:3] + (_LIGHT_KEYS if light else ()) + ((("lum2", 0),) if mom else ()):
        shape = (h, w, ch) if ch else (h, w)
        t = (out or {}).get(k)
        t = new(shape) if t is None else conv(f"out[{k!r}]", t, shape)
        if ptr(t) in taken["prev"]:
            raise ValueError(f"{who}: out[{k!r}] is a buffer of prev (the taps gather from prev)")
        if mom and ptr(t) in taken["cur"]:
            raise ValueError(f"{who}: out[{k!r}] is a buffer of cur (the window reads the current frame's "
                             "neighbours)")
        res.append(t)
    fo = _lib.RtFrame(*[ptr(t) for t in res[:3]], None, None, 0.0, 0)
    eo = RtAovEmit(ptr(res[3]), None, ptr(res[4])) if light else None
    o, mo = _reproject_opts(**opts), _moments_opts(min_frames, var_radius)
    co = None
    if mom and gamma is not None:
        if gamma > 0 and C.c_float(gamma).value == 0.0:
            raise ValueError(f"{who}: gamma {gamma!r} rounds to 0 as a float, which selects the default")
        co = _lib.RtClipOpts(float(gamma))
    r = lambda x: None if x is None else C.byref(x)  # noqa: E731
    cp = cam_prev.to_c() if not mom or prev is not None else None
    cc = cam_cur.to_c()
    cp, fp, ep, cc, fc, ec, o, mo, co, sp, fo, eo = map(r, (
        cp, c.get(("prev", _frame)), c.get(("prev", _frame_emit)), cc, c["cur", _frame], c.get(("cur", _frame_emit)),
        o, mo, co, sp, fo, eo))
    head = (mode, cp, fp, ep, lp, cc, fc, ec, w, h, o, mo)  # the moments family's, up to mopts
    tail = (fo, eo, ptr(res[-1]))  # ... and from out on
    args = {"plain": (cp, fp, cc, fc, w, h, o, fo),
            "emit": (cp, fp, ep, cc, fc, ec, w, h, o, fo),
            "light": (cp, fp, ep, cc, fc, ec, w, h, o, fo, eo),
            "moments": head + tail,
            "clip": head + (co,) + tail,
            "spec": head + (co, sp) + tail}[family]
    if device:
        args += (cur["rgb"].device.index or 0, _stream_of(cur["rgb"]))
    check(getattr(lib(), "rt_" + who)(*args))
    return tuple(res)


def reproject(cam_prev, prev, cam_cur, cur, **opts):
    """Temporal reprojection (rt_reproject) on host arrays: the frame `cur` seen by `cam_cur`
    blended with the history `prev` seen by `cam_prev` that lies behind each of its pixels.  A
    frame is a dict of float32 arrays "rgb" [H, W, 3], "normal" [H, W, 3] and "depth" [H, W] (as
    Accumulator.resolve / resolve_aov give them) with an optional "var" [H, W] (missing: 0) and
    "count" ([H, W], or one number for every pixel; missing: 0, which marks every pixel
    invalid).  opts: max_history, depth_tol, normal_tol, min_weight (0 = the library defaults).
    Returns new arrays (rgb, var, count)."""
    return _reproject_call("plain", False, None, cam_prev, prev, cam_cur, cur, None, opts)


def reproject_device(cam_prev, prev, cam_cur, cur, out=None, **opts):
    """rt_reproject_device on torch tensors: frames as reproject's, every buffer a contiguous
    float32 tensor on cur["rgb"]'s device.  `out`: a dict of the "rgb" / "var" / "count" tensors
    to write (missing or None: a new tensor); they may be cur's own (in place), never prev's.
    Runs on the tensors' current stream and returns (rgb, var, count) after the work completes."""
    return _reproject_call("plain", True, None, cam_prev, prev, cam_cur, cur, out, opts)


def reproject_emit(cam_prev, prev, cam_cur, cur, **opts):
    """reproject with the directly seen emission kept out of the history (rt_reproject_emit): both
    frames must also hold "emission" [H, W, 3] and "coverage" [H, W] (resolve_aov of an
    accumulator with features="emit").  The history carries (rgb - emission) / (1 - coverage),
    the current frame's own emission is added back, and a fully covered pixel neither gives nor
    takes history.  Returns new arrays (rgb, var, count)."""
    return _reproject_call("emit", False, None, cam_prev, prev, cam_cur, cur, None, opts)


def reproject_emit_device(cam_prev, prev, cam_cur, cur, out=None, **opts):
    """rt_reproject_emit_device on torch tensors: frames as reproject_emit's, every buffer a
    contiguous float32 tensor on cur["rgb"]'s device; `out` as reproject_device's (never a buffer
    of prev, its emission and coverage included)."""
    return _reproject_call("emit", True, None, cam_prev, prev, cam_cur, cur, out, opts)


def reproject_light(cam_prev, prev, cam_cur, cur, **opts):
    """reproject_emit with emission and coverage carried as history planes of their own
    (rt_reproject_light): frames as reproject_emit's, prev's "emission" and "coverage" being the
    planes an earlier call returned (or the first frame's own).  Both are reprojected and blended
    with the surface radiance's weights and the pixel is re-lit from the blend, so the rim of a
    light, where coverage is a few samples' estimate, gains from the history too.  Returns new
    arrays (rgb, var, count, emission, coverage): the last two are the next call's prev planes and
    the planes to hand the split filter."""
    return _reproject_call("light", False, None, cam_prev, prev, cam_cur, cur, None, opts)


def reproject_light_device(cam_prev, prev, cam_cur, cur, out=None, **opts):
    """rt_reproject_light_device on torch tensors: frames as reproject_light's, every buffer a
    contiguous float32 tensor on cur["rgb"]'s device; `out` as reproject_device's and may also name
    "emission" and "coverage" (cur's own allowed, never a buffer of prev).  Returns (rgb, var,
    count, emission, coverage)."""
    return _reproject_call("light", True, None, cam_prev, prev, cam_cur, cur, out, opts)


def reproject_moments(mode, cam_prev, prev, cam_cur, cur, min_frames=0.0, var_radius=0, **opts):
    """reproject ('plain'), reproject_emit ('emit') or reproject_light ('light') with the second
    moment of luminance carried through the history and the variance taken from the moments
    (rt_reproject_moments; DESIGN.md "Luminance moments"), so that frames of ONE pass, whose own
    variance is 0, come out with a variance rt_denoise_var can use.  Frames as the mode's, prev also
    with "lum2" [H, W], the plane an earlier call returned.  prev=None (and cam_prev=None): no
    history at all, a sequence's first frame.  A pixel whose history is at least min_frames frames
    long (0: 4) takes the variance of its moments, any other the variance of the current frame's
    window of var_radius (0: 3; -1: none, the mode's own variance).  Returns new arrays (rgb, var,
    count, lum2), in the 'light' mode (rgb, var, count, emission, coverage, lum2)."""
    return _reproject_call("moments", False, mode, cam_prev, prev, cam_cur, cur, None, opts, min_frames, var_radius)


def reproject_moments_device(mode, cam_prev, prev, cam_cur, cur, out=None, min_frames=0.0, var_radius=0, **opts):
    """rt_reproject_moments_device on torch tensors: frames as reproject_moments', every buffer a
    contiguous float32 tensor on cur["rgb"]'s device.  `out` as reproject_device's, with "lum2" (and
    "emission", "coverage" in the 'light' mode); here no out tensor may be one of cur's either: the
    window reads the current frame's neighbours.  Returns reproject_moments' tuple."""
    return _reproject_call("moments", True, mode, cam_prev, prev, cam_cur, cur, out, opts, min_frames, var_radius)


def reproject_clip(mode, cam_prev, prev, cam_cur, cur, min_frames=0.0, var_radius=0, gamma=0.0, **opts):
    """reproject_moments with the history colour clamped, per channel, to mean +- gamma sigma of
    the current frame's window before the blend (rt_reproject_clip; DESIGN.md "Clamping the
    history"): a history the current frame contradicts, as a reflection that moved over a mirror
    whose depth and normal did not, is overruled.  Arguments and result as reproject_moments';
    gamma 0: the library default; var_radius = -1 is refused (there is no window)."""
    return _reproject_call("clip", False, mode, cam_prev, prev, cam_cur, cur, None, opts, min_frames, var_radius, gamma)


def reproject_clip_device(mode, cam_prev, prev, cam_cur, cur, out=None, min_frames=0.0, var_radius=0, gamma=0.0,
                          **opts):
    """rt_reproject_clip_device on torch tensors: reproject_moments_device with reproject_clip's
    gamma."""
    return _reproject_call("clip", True, mode, cam_prev, prev, cam_cur, cur, out, opts, min_frames, var_radius, gamma)


def reproject_spec(mode, cam_prev, prev, cam_cur, cur, min_frames=0.0, var_radius=0, gamma=0.0, **opts):
    """reproject_clip for mirrors (rt_reproject_spec; DESIGN.md "Temporal history for mirrors"): the
    frames' "normal" and "depth" are the specular chains' (Accumulator.resolve_aov_spec), so the
    history is looked up through the mirror's virtual point, and both frames also hold "bounces"
    [H, W]: a pixel whose bounces value is not a whole number has no history, and a tap is taken
    only where its bounces value equals the pixel's.  Arguments and result as reproject_clip's;
    gamma=None: no clamp (reproject_moments' blend)."""
    return _reproject_call("spec", False, mode, cam_prev, prev, cam_cur, cur, None, opts, min_frames, var_radius, gamma)


def reproject_spec_device(mode, cam_prev, prev, cam_cur, cur, out=None, min_frames=0.0, var_radius=0, gamma=0.0,
                          **opts):
    """rt_reproject_spec_device on torch tensors: reproject_clip_device with reproject_spec's frames."""
    return _reproject_call("spec", True, mode, cam_prev, prev, cam_cur, cur, out, opts, min_frames, var_radius, gamma)


class Temporal:
    """The history of a moving camera (DESIGN.md "Temporal reprojection"): ``push(acc)`` takes the
    accumulator of the next frame, reprojects the stored history into its camera
    (reproject_device) and keeps the result as the new history.  Two sets of device tensors are
    owned and used in turn, so a push allocates nothing once warm.  opts: reproject's
    (max_history, depth_tol, normal_tol, min_weight).  The scene is static and the cameras have
    no defocus; ``reset()`` drops the history (a cut, a changed scene).  split_emitters=True
    (reproject_emit_device) keeps directly seen lights out of the history: the accumulators must
    then have features="emit", whose emission and coverage are kept with the history.
    light_history=True (reproject_light_device; needs split_emitters) carries emission and
    coverage as history planes too: ``light`` is then the dict {"emission", "coverage"} of the
    tensors the last push wrote, the planes to hand the split filter in place of the frame's own:
    ``denoise_var_device(rgb, var, dict(acc.resolve_aov_device(), **temporal.light),
    split_emitters=True)``.
    moments=True (reproject_moments_device, DESIGN.md "Luminance moments"; combines with both
    flags above) also carries the second moment of luminance and returns the variance of the
    moments, or of a window of the frame while the history is shorter than min_frames (0: 4)
    frames; var_radius is the window's (0: 3, -1: none).  The accumulators may then hold ONE pass
    each: the returned variance is not 0 as the accumulator's own is, the first push's included.
    clip=True (reproject_clip_device, DESIGN.md "Clamping the history"; needs moments=True and a
    window) clamps the reprojected colour to the current frame's neighbourhood before the blend,
    mean +- clip_gamma sigma (0: the library default), so that a stale reflection on metal or glass
    is overruled.
    specular=True (reproject_spec_device, DESIGN.md "Temporal history for mirrors"; needs
    moments=True, combines with clip) looks the history of a mirror up through its virtual point: the
    accumulators must have features "guides+spec" or "emit+spec", and the history's normal, depth
    and bounces are their chain planes (resolve_aov_spec_device), not the first hit's."""

    def __init__(self, split_emitters=False, light_history=False, moments=False, min_frames=0.0, var_radius=0,
                 clip=False, clip_gamma=0.0, specular=False, **opts):
        _reproject_opts(**opts)  # a wrong name fails here, not at the second push
        if specular and not moments:
            raise ValueError("Temporal: specular=True needs moments=True (the chain gate is a step of "
                             "reproject_moments): Temporal(moments=True, specular=True)")
        self._specular = bool(specular)
        if not moments and (min_frames or var_radius):
            raise ValueError("Temporal: min_frames and var_radius are options of moments=True")
        if clip and not moments:
            raise ValueError("Temporal: clip=True needs moments=True (the clamp is a step of reproject_moments)")
        if clip and int(var_radius) == -1:
            raise ValueError("Temporal: clip=True needs a window: var_radius >= 0, not -1")
        if not clip and clip_gamma:
            raise ValueError("Temporal: clip_gamma is an option of clip=True")
        if clip and (not (math.isfinite(clip_gamma) and clip_gamma >= 0)
                     or (clip_gamma > 0 and C.c_float(clip_gamma).value == 0.0)):
            raise ValueError("Temporal: clip_gamma must be 0 (the default) or a finite positive float")
        self._clip = float(clip_gamma) if clip else None
        self._moments = bool(moments)
        self._mopts = dict(min_frames=float(min_frames), var_radius=int(var_radius))
        self._cur = None
        if light_history and not split_emitters:
            raise ValueError("Temporal: light_history needs split_emitters=True (the history of the emission "
                             "split's planes)")
        self._opts = opts
        self._split = bool(split_emitters)
        self._light = bool(light_history)
        self._sets = [None, None]
        self.reset()

    def reset(self):
        """Drop the history: the next push returns its frame unchanged."""
        self._prev, self._cam = None, None
        self.light = None

    def push(self, acc):
        """`acc`: an Accumulator with features ("guides" or "emit") of the whole image
        (nranks == 1) holding at least one pass.  Resolves its mean, variance, normal and depth on
        the device, every pixel weighing acc.passes, and blends the history into them.  Returns
        the tensors (rgb [H, W, 3], var [H, W], count [H, W]) ready for denoise_var_device; they
        belong to this object and are overwritten by the push after the next.  The first push
        (and the first after reset()) returns the current frame unchanged.  With light_history the
        blended emission and coverage are left in ``light`` (the first push: the frame's own).
        With moments=True the returned var is not the accumulator's: it is the variance of the
        history's luminance moments, or of a window of the frame where the history is shorter than
        min_frames, so the first push returns the frame's colour and count with the window's
        variance; the tensors then come from the object's own sets, never the accumulator's
        resolve targets."""
        import torch
        if acc.features is None:
            raise ValueError("Temporal.push: needs an accumulator with features (the normal and depth guides)")
        if self._split and not str(acc.features).startswith("emit"):
            raise ValueError("Temporal.push: split_emitters needs an accumulator with features='emit' "
                             f"(Scene.accumulator(..., features='emit')), not features={acc.features!r}")
        if self._specular and not str(acc.features).endswith("+spec"):
            raise ValueError("Temporal.push: specular=True needs an accumulator with the chain planes "
                             "(Scene.accumulator(..., features='guides+spec' or 'emit+spec')), not "
                             f"features={acc.features!r}")
        if acc.nranks != 1:
            raise ValueError("Temporal.push: needs the whole image (nranks == 1)")
        passes = acc.passes
        if passes < 1:
            raise ValueError("Temporal.push: the accumulator holds no pass")
        k = 0 if self._prev != 0 else 1  # the set the history is not in
        h, w = acc.shape
        dev = torch.device("cuda", acc._device)
        if self._moments:
            return self._push_moments(acc, k, h, w, dev, float(passes))
        s = self._sets[k]
        keys = _FRAME_KEYS + ((("emission", 3), ("coverage", 0)) if self._split else ())
        if s is None or s["depth"].shape != (h, w) or s["depth"].device != dev:
            s = self._sets[k] = {key: torch.empty((h, w, ch) if ch else (h, w), dtype=torch.float32, device=dev)
                                 for key, ch in keys}
        acc.resolve_device(s["rgb"], s["var"])
        guides = RtAov(None, s["normal"].data_ptr(), s["depth"].data_ptr(), None)
        emit = RtAovEmit(s["emission"].data_ptr(), None, s["coverage"].data_ptr()) if self._split else None
        check(lib().rt_accum_resolve_aov_device(acc._h(), C.byref(guides), emit and C.byref(emit)))
        p = None if self._prev is None else self._sets[self._prev]
        if p is None or p["depth"].shape != (h, w) or p["depth"].device != dev:
            s["count"].fill_(float(passes))
        else:
            fn = (reproject_light_device if self._light else reproject_emit_device if self._split
                  else reproject_device)
            fn(self._cam, p, acc.camera, dict(s, count=float(passes)), out=s, **self._opts)
        self._prev, self._cam = k, acc.camera
        if self._light:
            self.light = {"emission": s["emission"], "coverage": s["coverage"]}
        return s["rgb"], s["var"], s["count"]

    def _push_moments(self, acc, k, h, w, dev, passes):
        """push with moments=True.  out may not be cur here (the window reads the frame's
        neighbours), so the planes the kernel writes are resolved into a third set, `_cur`; normal
        and depth, which it only reads, go straight into the new history's set, as do emission and
        coverage unless the light history writes them."""
        import torch

        def tensors(keys):
            return {key: torch.empty((h, w, ch) if ch else (h, w), dtype=torch.float32, device=dev) for key, ch in keys}
        split = (("emission", 3), ("coverage", 0)) if self._split else ()
        s = self._sets[k]
        spec = (("bounces", 0),) if self._specular else ()
        if s is None or "lum2" not in s or s["depth"].shape != (h, w) or s["depth"].device != dev:
            s = self._sets[k] = tensors(_FRAME_KEYS + split + (("lum2", 0),) + spec)
        c = self._cur
        if c is None or c["var"].shape != (h, w) or c["var"].device != dev:
            c = self._cur = tensors((("rgb", 3), ("var", 0)) + (split if self._light else ()))
        acc.resolve_device(c["rgb"], c["var"])
        guides = RtAov(None, s["normal"].data_ptr(), s["depth"].data_ptr(), None)
        e = c if self._light else s
        emit = RtAovEmit(e["emission"].data_ptr(), None, e["coverage"].data_ptr()) if self._split else None
        if self._specular:  # the chain's normal, depth and bounces in the first hit's place
            chain = RtAovSpec(s["bounces"].data_ptr())
            check(lib().rt_accum_resolve_aov_spec_device(acc._h(), C.byref(guides), C.byref(chain)))
            if emit:
                check(lib().rt_accum_resolve_aov_device(acc._h(), None, C.byref(emit)))
        else:
            check(lib().rt_accum_resolve_aov_device(acc._h(), C.byref(guides), emit and C.byref(emit)))
        cur = dict(c, count=passes, normal=s["normal"], depth=s["depth"])
        if self._specular:
            cur["bounces"] = s["bounces"]
        if self._split:
            cur.update(emission=e["emission"], coverage=e["coverage"])
        p = None if self._prev is None else self._sets[self._prev]
        if p is not None and (p["depth"].shape != (h, w) or p["depth"].device != dev):
            p = None
        out = {key: s[key] for key in ("rgb", "var", "count", "lum2") + (("emission", "coverage") if self._light else ())}
        mode = "light" if self._light else "emit" if self._split else "plain"
        if self._specular:
            reproject_spec_device(mode, None if p is None else self._cam, p, acc.camera, cur, out=out,
                                  gamma=self._clip, **self._mopts, **self._opts)
        elif self._clip is None:
            reproject_moments_device(mode, None if p is None else self._cam, p, acc.camera, cur, out=out,
                                     **self._mopts, **self._opts)
        else:
            reproject_clip_device(mode, None if p is None else self._cam, p, acc.camera, cur, out=out,
                                  gamma=self._clip, **self._mopts, **self._opts)
        self._prev, self._cam = k, acc.camera
        if self._light:
            self.light = {"emission": s["emission"], "coverage": s["coverage"]}
        return s["rgb"], s["var"], s["count"]


class _DevicePlane:
    """A borrowed float32 device plane for torch.as_tensor (the CUDA array interface): no copy."""

    def __init__(self, addr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(addr), False),
                                         "version": 2, "strides": None}


class Pipeline:
    """rt_pipeline (DESIGN.md "Frame pipeline"): Temporal and the spatial filter behind one object
    of the C ABI that owns its device buffers, the form a C or cgo client uses.  ``push(acc)``
    does what ``temporal.push(acc)`` followed by ``denoise_var_device`` (filter="var"),
    ``denoise_device`` (filter="plain") or nothing (filter=None) over ``acc.resolve_aov_device()``
    does, bit for bit; temporal=False skips the history.  split_emitters, light_history, moments,
    clip, specular: Temporal's flags.  filter_split (None: as split_emitters) selects the filter's
    split entries.  opts: Temporal's (max_history, depth_tol, normal_tol, min_weight, min_frames,
    var_radius, clip_gamma) and the filter's (iterations, demodulate (default on, as the filter
    functions' with an albedo), sigma_lum or sigma_color, sigma_normal, sigma_depth)."""

    _FILTERS = {None: _lib.RT_PIPE_FILTER_NONE, "plain": _lib.RT_PIPE_FILTER_PLAIN, "var": _lib.RT_PIPE_FILTER_VAR}

    def __init__(self, temporal=True, split_emitters=False, light_history=False, moments=False, clip=False,
                 specular=False, filter="var", filter_split=None, **opts):
        self._p = None
        if filter not in self._FILTERS:
            raise ValueError(f"Pipeline: filter must be 'var', 'plain' or None, not {filter!r}")
        if light_history and not split_emitters:
            raise ValueError("Pipeline: light_history needs split_emitters=True (the history of the emission "
                             "split's planes)")
        o = _lib.RtPipelineOpts()
        o.temporal, o.moments, o.clip, o.specular = int(bool(temporal)), int(bool(moments)), int(bool(clip)), \
            int(bool(specular))
        o.mode = (_lib.RT_REPROJECT_LIGHT if light_history else _lib.RT_REPROJECT_EMIT if split_emitters
                  else _lib.RT_REPROJECT_PLAIN)
        o.reproject = _reproject_opts(**{k: opts.pop(k) for k in ("max_history", "depth_tol", "normal_tol",
                                                                  "min_weight") if k in opts})
        o.mopts = _moments_opts(opts.pop("min_frames", 0.0), opts.pop("var_radius", 0))
        o.copts = _lib.RtClipOpts(float(opts.pop("clip_gamma", 0.0)))
        o.filter = self._FILTERS[filter]
        o.split_emitters = int(bool(split_emitters if filter_split is None else filter_split))
        if filter == "plain":
            o.dopts = _denoise_opts(False, has_albedo=True, **opts)
        else:
            o.vopts = _denoise_opts(True, has_albedo=True, **opts)
        p = C.c_void_p()
        check(lib().rt_pipeline_create(C.byref(o), C.byref(p)))
        self._p = p
        self._destroy = lib().rt_pipeline_destroy  # usable at interpreter shutdown
        self.opts = o

    def close(self):
        if getattr(self, "_p", None):
            self._destroy(self._p)
            self._p = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _h(self):
        if not self._p:
            raise ValueError("Pipeline is closed")
        return self._p

    def push(self, acc):
        """The next frame: `acc` as Temporal.push's (rt_pipeline_push), or a frame held as row
        shares, an AccumulatorShares or a list or tuple of the shares' Accumulators in rank order
        (rt_pipeline_push_shares: the same bits as the whole accumulator's push).  Returns self."""
        if isinstance(acc, AccumulatorShares):
            acc = acc.shares
        if isinstance(acc, (list, tuple)):
            arr, n = _share_array(acc)
            check(lib().rt_pipeline_push_shares(self._h(), arr, n))
        else:
            check(lib().rt_pipeline_push(self._h(), acc._h()))
        return self

    def reset(self):
        """Drop the history (a cut); the buffers stay."""
        check(lib().rt_pipeline_reset(self._h()))

    def info(self):
        """rt_pipeline_info as a dict: width, height, device, frames, had_history, device_bytes,
        allocations."""
        i = _lib.RtPipelineInfo()
        check(lib().rt_pipeline_info_get(self._h(), C.byref(i)))
        d = _as_dict(i)
        d.pop("_pad")
        return d

    def image(self):
        """The last push's image as a host float32 [H, W, 3] array: one copy."""
        i = self.info()
        out = np.empty((i["height"], i["width"], 3), np.float32)
        check(lib().rt_pipeline_image(self._h(), out.ctypes.data))
        return out

    def ppm(self):
        """The last push's image as P3 text (bytes), formatted on the device: one copy."""
        n = int(lib().rt_pipeline_ppm(self._h(), None, 0))
        check(n)
        buf = C.create_string_buffer(n)
        check(int(lib().rt_pipeline_ppm(self._h(), buf, n)))
        return buf.raw[:n]

    def planes_device(self):
        """The last push's planes as borrowed device pointers, valid until the push after the
        next: a dict of zero-copy float32 torch tensors "rgb" [H, W, 3], "var", "count" [H, W],
        "normal" [H, W, 3], "depth" and "image" [H, W, 3], with "emission" [H, W, 3] and "coverage"
        where the pipeline holds them (the blended ones with light_history) and "lum2" with
        moments.  Without torch: the same keys with (address, shape) pairs."""
        f, e = _lib.RtFrame(), RtAovEmit()
        lum2, image = C.c_void_p(), C.c_void_p()
        check(lib().rt_pipeline_planes_device(self._h(), C.byref(f), C.byref(e), C.byref(lum2), C.byref(image)))
        i = self.info()
        h, w = i["height"], i["width"]
        raw = {"rgb": (f.rgb, (h, w, 3)), "var": (f.var, (h, w)), "count": (f.count, (h, w)),
               "normal": (f.normal, (h, w, 3)), "depth": (f.depth, (h, w)), "emission": (e.emission, (h, w, 3)),
               "coverage": (e.coverage, (h, w)), "lum2": (lum2.value, (h, w)), "image": (image.value, (h, w, 3))}
        raw = {k: v for k, v in raw.items() if v[0]}
        try:
            import torch
        except ImportError:
            return raw
        dev = torch.device("cuda", i["device"])
        return {k: torch.as_tensor(_DevicePlane(a, s), device=dev) for k, (a, s) in raw.items()}


def device_count():
    return lib().rt_device_count()


# ---- tuning knobs (rt_tune_set): the library never reads the process environment ----
def tune_knobs():
    """{knob name: changes_image_bits} for every knob the library consults."""
    n = lib().rt_tune_list(-1, None, None)
    out = {}
    for i in range(n):
        name, bits = C.c_char_p(), C.c_int32()
        check(lib().rt_tune_list(i, C.byref(name), C.byref(bits)))
        out[name.value.decode()] = bool(bits.value)
    return out


def tune(name, value):
    """Set knob `name` (e.g. "RT_TAIL_FRAC") to `value`; None clears it."""
    v = None if value is None else str(value).encode()
    check(lib().rt_tune_set(name.encode(), v))


def tune_get(name):
    """The text knob `name` is set to, or None when it is at its default."""
    n = int(lib().rt_tune_get(name.encode(), None, 0))
    check(n)
    if n == 0:
        return None
    buf = C.create_string_buffer(n)
    check(int(lib().rt_tune_get(name.encode(), buf, n)))
    return buf.value.decode()


def untune(name=None):
    """Clear one knob, or every knob (name None)."""
    check(lib().rt_tune_set(None if name is None else name.encode(), None))


class tuning:
    """Context manager: ``with rt.tuning(RT_SPLIT_MIN=0): ...`` sets knobs, then puts back the
    values they had on entry (cleared if they were unset)."""

    def __init__(self, **knobs):
        self.knobs = knobs
        self.saved = {}

    def __enter__(self):
        self.saved = {k: tune_get(k) for k in self.knobs}
        try:
            for k, v in self.knobs.items():
                tune(k, v)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *a):
        for k, v in self.saved.items():
            tune(k, v)


def tune_from_env(environ=None):
    """Dev tools only (tools/*): copy RT_* knobs from the environment into the library, an
    explicit opt-in of the calling process.  Returns the knobs set."""
    import os
    env = os.environ if environ is None else environ
    got = {k: env[k] for k in tune_knobs() if env.get(k)}
    for k, v in got.items():
        tune(k, v)
    return got
