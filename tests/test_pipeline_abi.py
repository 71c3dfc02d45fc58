"""rt_pipeline (include/rt_abi.h) on a host without a GPU: the symbols exist with the header's
signatures and structure sizes, rt_pipeline_create refuses what it must with RT_ERR_INVALID before
any device is touched, the entries that need a frame refuse before the first push, and create,
info_get, reset and destroy work with no device at all."""
import ctypes as C
import math
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_pipeline_create", "rt_pipeline_destroy", "rt_pipeline_reset", "rt_pipeline_push", "rt_pipeline_image",
           "rt_pipeline_ppm", "rt_pipeline_planes_device", "rt_pipeline_info_get")
# the header's C types as ctypes (structures by their rt_ name)
INT32 = {"temporal", "mode", "moments", "clip", "specular", "filter", "split_emitters"}


def _header():
    return open(os.path.join(REPO, "include", "rt_abi.h")).read()


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    assert "Pipeline" in rt.__all__ and "Temporal" in rt.__all__
    assert rt.lib().rt_abi_version() == 4  # additive: callers detect the feature by the symbols
    text = _header()
    for name, value in (("NONE", 0), ("PLAIN", 1), ("VAR", 2)):
        assert re.search(r"#define RT_PIPE_FILTER_%s\s+%d\b" % (name, value), text)
        assert getattr(rt._lib, "RT_PIPE_FILTER_" + name) == value


def test_structures_match_the_header(rt):
    lb, text = rt._lib, _header()
    m = re.search(r"typedef struct \{([^}]*)\} rt_pipeline_opts;", text)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)]
    assert [n for _, n in fields] == [f[0] for f in lb.RtPipelineOpts._fields_]
    by_c = {"int32_t": C.c_int32, "rt_reproject_opts": lb.RtReprojectOpts, "rt_moments_opts": lb.RtMomentsOpts,
            "rt_clip_opts": lb.RtClipOpts, "rt_denoise_opts": lb.RtDenoiseOpts, "rt_denoise_var_opts": lb.RtDenoiseVarOpts}
    assert [by_c[t] for t, _ in fields] == [f[1] for f in lb.RtPipelineOpts._fields_]
    assert {n for t, n in fields if t == "int32_t"} == INT32
    assert C.sizeof(lb.RtPipelineOpts) == 104  # 7 x 4 + 16 + 8 + 4 + 24 + 24, no padding
    assert lb.RtPipelineOpts.reproject.offset == 20 and lb.RtPipelineOpts.filter.offset == 48
    assert lb.RtPipelineOpts.dopts.offset == 56 and lb.RtPipelineOpts.vopts.offset == 80
    m = re.search(r"typedef struct \{([^}]*)\} rt_pipeline_info;", text)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for _, ns in re.findall(r"^\s*(\w+)\s+([\w, ]+);", body, re.M) for n in ns.split(",")]
    assert names == [f[0] for f in lb.RtPipelineInfo._fields_]
    assert C.sizeof(lb.RtPipelineInfo) == 40 and lb.RtPipelineInfo.device_bytes.offset == 24


def test_ctypes_signatures_match_the_header(rt):
    lb, text = rt._lib, _header()
    P = C.c_void_p
    by_c = {"const rt_pipeline_opts*": C.POINTER(lb.RtPipelineOpts), "rt_pipeline**": C.POINTER(P), "rt_pipeline*": P,
            "rt_accum*": P, "float*": P, "char*": P, "int64_t": C.c_int64, "rt_frame*": C.POINTER(lb.RtFrame),
            "rt_aov_emit*": C.POINTER(lb.RtAovEmit), "float**": C.POINTER(P),
            "rt_pipeline_info*": C.POINTER(lb.RtPipelineInfo)}
    for name in SYMBOLS:
        m = re.search(r"^(int|int64_t) " + name + r"\(([^)]*)\);", text, re.M)
        assert m, name
        res, args = lb.SIGNATURES[name]
        assert res == {"int": C.c_int, "int64_t": C.c_int64}[m.group(1)], name
        types = [p.strip().rsplit(" ", 1)[0].strip() for p in m.group(2).replace("\n", " ").split(",")]
        assert [by_c[t] for t in types] == args, name


def _opts(rt, **kw):
    o = rt._lib.RtPipelineOpts()
    o.temporal, o.filter = 1, rt._lib.RT_PIPE_FILTER_VAR
    for k, v in kw.items():
        obj, path = o, k.split("__")
        for p in path[:-1]:
            obj = getattr(obj, p)
        setattr(obj, path[-1], v)
    return o


def _create(rt, o):
    p = C.c_void_p()
    rc = rt.lib().rt_pipeline_create(None if o is None else C.byref(o), C.byref(p))
    return rc, p


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw,word", [
    (dict(mode=3), b"mode"), (dict(mode=-1), b"mode"),
    (dict(filter=3), b"filter"), (dict(filter=-1), b"filter"),
    (dict(clip=1), b"moments"), (dict(specular=1), b"moments"), (dict(clip=1, specular=1), b"moments"),
    (dict(moments=1, clip=1, mopts__radius=-1), b"window"),
    (dict(reproject__max_history=-1.0), b"reproject"), (dict(reproject__depth_tol=NAN), b"reproject"),
    (dict(reproject__normal_tol=INF), b"reproject"), (dict(reproject__min_weight=-0.5), b"reproject"),
    (dict(moments=1, mopts__radius=-2), b"radius"), (dict(moments=1, mopts__radius=9), b"radius"),
    (dict(moments=1, mopts__min_frames=-1.0), b"min_frames"), (dict(moments=1, mopts__min_frames=1.5), b"min_frames"),
    (dict(moments=1, mopts__min_frames=INF), b"min_frames"),
    (dict(moments=1, clip=1, copts__gamma=-1.0), b"gamma"), (dict(moments=1, clip=1, copts__gamma=NAN), b"gamma"),
    (dict(moments=1, clip=1, copts__gamma=INF), b"gamma"),
    (dict(vopts__iterations=9), b"iterations"), (dict(dopts__iterations=-1), b"iterations"),
    (dict(vopts__sigma_lum=-1.0), b"sigma"), (dict(vopts__sigma_normal=NAN), b"sigma"),
    (dict(dopts__sigma_color=-1.0), b"sigma"), (dict(dopts__sigma_depth=NAN), b"sigma"),
    (dict(temporal=0, moments=1), b"temporal = 1"), (dict(temporal=0, mode=1), b"temporal = 1"),
    (dict(temporal=0, mode=2), b"temporal = 1"), (dict(temporal=0, moments=1, clip=1), b"temporal = 1"),
    (dict(temporal=0, moments=1, specular=1), b"temporal = 1"),
])
def test_create_refusals(rt, kw, word):
    rc, p = _create(rt, _opts(rt, **kw))
    err = rt.lib().rt_last_error()
    assert rc == rt._lib.RT_ERR_INVALID and not p.value, (kw, err)
    assert b"rt_pipeline_create" in err and word in err, err


def test_null_arguments(rt):
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    assert _create(rt, None)[0] == E and b"rt_pipeline_create" in L.rt_last_error()
    assert L.rt_pipeline_create(C.byref(_opts(rt)), None) == E
    assert L.rt_pipeline_reset(None) == E and L.rt_pipeline_push(None, None) == E
    assert L.rt_pipeline_image(None, None) == E and L.rt_pipeline_ppm(None, None, 0) == E
    assert L.rt_pipeline_planes_device(None, None, None, None, None) == E
    assert L.rt_pipeline_info_get(None, None) == E
    assert L.rt_pipeline_destroy(None) == rt._lib.RT_OK
    rc, p = _create(rt, _opts(rt))
    assert rc == 0
    assert L.rt_pipeline_push(p, None) == E and b"rt_pipeline_push" in L.rt_last_error()
    assert L.rt_pipeline_info_get(p, None) == E
    assert L.rt_pipeline_destroy(p) == 0


@pytest.mark.parametrize("kw", [
    dict(), dict(mode=1), dict(mode=2, moments=1, clip=1, copts__gamma=1.5), dict(mode=1, moments=1, specular=1),
    dict(moments=1, mopts__radius=-1), dict(temporal=0, filter=1), dict(temporal=0, filter=0), dict(filter=0, split_emitters=1),
    dict(vopts__sigma_lum=INF),  # the filters take +Inf (no edge stopping); so does the object
])
def test_lifecycle_without_a_device(rt, kw):
    """create, info_get, reset and destroy touch no device; what needs a frame refuses"""
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    rc, p = _create(rt, _opts(rt, **kw))
    assert rc == 0 and p.value, L.rt_last_error()
    i = rt._lib.RtPipelineInfo()
    for _ in range(2):
        assert L.rt_pipeline_info_get(p, C.byref(i)) == 0
        assert (i.width, i.height, i.device, i.frames, i.had_history) == (0, 0, -1, 0, 0)
        assert i.device_bytes == 0 and i.allocations == 0
        buf = C.create_string_buffer(64)
        assert L.rt_pipeline_image(p, buf) == E and b"rt_pipeline_push first" in L.rt_last_error()
        assert L.rt_pipeline_ppm(p, None, 0) == E and b"rt_pipeline_ppm" in L.rt_last_error()
        assert L.rt_pipeline_ppm(p, buf, 64) == E
        f, e, a, b = rt._lib.RtFrame(), rt._lib.RtAovEmit(), C.c_void_p(), C.c_void_p()
        assert L.rt_pipeline_planes_device(p, C.byref(f), C.byref(e), C.byref(a), C.byref(b)) == E
        assert b"rt_pipeline_planes_device" in L.rt_last_error()
        assert L.rt_pipeline_reset(p) == 0
    assert L.rt_pipeline_destroy(p) == 0


def test_python_class(rt):
    with pytest.raises(ValueError, match="filter"):
        rt.Pipeline(filter="median")
    with pytest.raises(ValueError, match="split_emitters=True"):
        rt.Pipeline(light_history=True)
    with pytest.raises(TypeError):
        rt.Pipeline(sigma_colour=1.0)
    with pytest.raises(TypeError):
        rt.Pipeline(filter="plain", sigma_lum=1.0)  # the plain filter's is sigma_color
    for kw, code in ((dict(clip=True), "moments"), (dict(specular=True), "moments"),
                     (dict(temporal=False, moments=True), "temporal = 1"),
                     (dict(moments=True, clip=True, var_radius=-1), "window"),
                     (dict(moments=True, min_frames=1.0), "min_frames"), (dict(max_history=-1.0), "reproject")):
        with pytest.raises(rt.RtError, match=code) as e:
            rt.Pipeline(**kw)
        assert e.value.code == rt._lib.RT_ERR_INVALID
    with rt.Pipeline(split_emitters=True, light_history=True, moments=True, clip=True, clip_gamma=1.5, min_frames=3.0,
                     var_radius=2, max_history=16.0, iterations=3, sigma_lum=2.0) as p:
        o = p.opts
        assert (o.temporal, o.mode, o.moments, o.clip, o.specular) == (1, rt._lib.RT_REPROJECT_LIGHT, 1, 1, 0)
        assert (o.filter, o.split_emitters) == (rt._lib.RT_PIPE_FILTER_VAR, 1)
        assert (o.mopts.min_frames, o.mopts.radius, o.copts.gamma, o.reproject.max_history) == (3.0, 2, 1.5, 16.0)
        assert (o.vopts.iterations, o.vopts.demodulate, o.vopts.sigma_lum) == (3, 1, 2.0)
        assert p.info() == dict(width=0, height=0, device=-1, frames=0, had_history=0, device_bytes=0, allocations=0)
        p.reset()
        for call in (p.image, p.ppm, p.planes_device):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == rt._lib.RT_ERR_INVALID
    with pytest.raises(ValueError, match="closed"):
        p.info()
    p.close()  # twice is fine
    q = rt.Pipeline(split_emitters=True, filter="plain", filter_split=False, demodulate=False, sigma_color=0.25)
    assert (q.opts.mode, q.opts.filter, q.opts.split_emitters) == (1, 1, 0)
    assert q.opts.dopts.demodulate == 0 and math.isclose(q.opts.dopts.sigma_color, 0.25)
    assert rt.Pipeline(filter=None).opts.filter == 0 and rt.Pipeline(temporal=False).opts.temporal == 0
