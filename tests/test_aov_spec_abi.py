"""The specular feature pass's entry points (include/rt_abi.h: rt_render_aov_spec[_device];
DESIGN.md §19) on a host without a GPU: the symbols exist with the header's prototypes,
rt_aov_spec_opts and rt_aov_spec have the header's layout, the ABI version stays 4, every
argument error is RT_ERR_INVALID before any device is touched (a correct call gets as far as the
device: RT_ERR_DEVICE here), and the Python wrappers refuse specular=True with emit or media."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = ("rt_render_aov_spec", "rt_render_aov_spec_device")


def test_symbols_exist_and_are_bound(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SPEC if not hasattr(L, s)] == []
    P = C.POINTER
    lb = rt._lib
    args = [C.c_void_p, P(lb.RtCamera), P(lb.RtRenderOpts), C.c_int32, P(lb.RtAovSpecOpts), P(lb.RtAov),
            P(lb.RtAovSpec), P(lb.RtStats)]
    for s in SPEC:
        f = getattr(rt.lib(), s)
        assert f.restype is C.c_int and list(f.argtypes) == args, s
    assert C.sizeof(lb.RtAovSpec) == C.sizeof(C.c_void_p)
    assert C.sizeof(lb.RtAovSpecOpts) == 8
    assert [(n, t) for n, t in lb.RtAovSpecOpts._fields_] == [("max_bounces", C.c_int32), ("max_fuzz", C.c_float)]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_c99_client_sees_the_prototypes(rt, tmp_path):
    """the header's prototypes are the library's and the ctypes declarations' (a C99 client assigns
    each entry to a pointer of the issue's type, -Werror), the structs have the ctypes layout, the
    version stays 4"""
    c = tmp_path / "spec.c"
    c.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
        "int main(void){\n"
        "  int (*r)(rt_scene*, const rt_camera*, const rt_render_opts*, int32_t, const rt_aov_spec_opts*,\n"
        "           const rt_aov*, const rt_aov_spec*, rt_stats*) = rt_render_aov_spec;\n"
        "  int (*rd)(rt_scene*, const rt_camera*, const rt_render_opts*, int32_t, const rt_aov_spec_opts*,\n"
        "            const rt_aov*, const rt_aov_spec*, rt_stats*) = rt_render_aov_spec_device;\n"
        "  rt_aov_spec m = {NULL};\n"
        '  printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(rt_aov_spec), offsetof(rt_aov_spec, bounces),\n'
        "         sizeof(rt_aov_spec_opts), offsetof(rt_aov_spec_opts, max_bounces), offsetof(rt_aov_spec_opts, max_fuzz),\n"
        "         RT_ABI_VERSION, r(NULL, NULL, NULL, 1, NULL, NULL, &m, NULL) + rd(NULL, NULL, NULL, 1, NULL, NULL, &m, NULL));\n"
        "  return 0;}\n")
    exe = tmp_path / "spec"
    lib_dir = os.path.dirname(rt._lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c), "-o",
                    str(exe), "-L", lib_dir, "-lrt_amd", f"-Wl,-rpath,{lib_dir}"], check=True)
    sz, off, osz, ob, of, ver, null_sum = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                                  text=True, timeout=60).stdout.split())
    lb = rt._lib
    assert (sz, off) == (C.sizeof(lb.RtAovSpec), lb.RtAovSpec.bounces.offset)
    assert (osz, ob, of) == (C.sizeof(lb.RtAovSpecOpts), lb.RtAovSpecOpts.max_bounces.offset,
                             lb.RtAovSpecOpts.max_fuzz.offset)
    assert ver == 4 and rt.lib().rt_abi_version() == 4  # additive: detect by the symbols
    assert null_sum == 2 * lb.RT_ERR_INVALID


def _spec(rt, fn, scene_p, cam_c, n, so, out, sp, rank=0, nranks=1):
    o = rt._lib.RtRenderOpts()
    o.seed, o.rank, o.nranks = 1, rank, nranks
    r = lambda s: None if s is None else C.byref(s)  # noqa: E731
    return getattr(rt.lib(), fn)(scene_p, r(cam_c), C.byref(o), n, r(so), r(out), r(sp), None)


@pytest.mark.parametrize("fn", SPEC)
def test_render_aov_spec_argument_errors(rt, fn):
    E = rt._lib.RT_ERR_INVALID
    lb = rt._lib
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    buf = np.zeros((8, 8, 3), np.float32)
    p = buf.ctypes.data
    sp = lb.RtAovSpec(p)
    err = rt.lib().rt_last_error
    with rt.Scene(t, w, l) as sc:
        assert _spec(rt, fn, sc._p, c, 1, None, lb.RtAov(p, None, None, None), None) == E
        assert b"null spec" in err()                                        # NULL spec: it selects the mode
        assert _spec(rt, fn, sc._p, c, 1, None, None, lb.RtAovSpec()) == E  # no buffer at all
        assert b"no buffer" in err()
        assert _spec(rt, fn, sc._p, c, 1, None, lb.RtAov(), lb.RtAovSpec()) == E
        assert b"no buffer" in err()
        for mb in (-1, 65, -2 ** 31, 2 ** 31 - 1):
            assert _spec(rt, fn, sc._p, c, 1, lb.RtAovSpecOpts(mb, 0.0), None, sp) == E, mb
            assert b"max_bounces" in err()
        for mf in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan")):
            assert _spec(rt, fn, sc._p, c, 1, lb.RtAovSpecOpts(0, mf), None, sp) == E, mf
            assert b"max_fuzz" in err()
        assert _spec(rt, fn, None, c, 1, None, None, sp) == E               # rt_render_aov's rules
        assert _spec(rt, fn, sc._p, None, 1, None, None, sp) == E
        assert _spec(rt, fn, sc._p, c, 5, None, None, sp) == E              # spp_sqrt^2 = 4
        assert _spec(rt, fn, sc._p, c, -1, None, None, sp) == E
        assert b"samples" in err()
        assert _spec(rt, fn, sc._p, c, 1, None, None, sp, rank=3, nranks=3) == E
        assert _spec(rt, fn, sc._p, c, 1, None, None, sp, rank=-1, nranks=2) == E
        assert b"rank" in err()


def test_valid_arguments_reach_the_device(rt):
    """nothing wrong: past the checks, so RT_ERR_DEVICE on a host without a GPU.  out and the
    options may be NULL, the limits of the options are inside, one buffer is enough"""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are the gpu tests'
    D = rt._lib.RT_ERR_DEVICE
    lb = rt._lib
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    buf = np.zeros((8, 8, 3), np.float32)
    p = buf.ctypes.data
    with rt.Scene(t, w, l) as sc:
        for fn in SPEC:
            assert _spec(rt, fn, sc._p, c, 4, None, None, lb.RtAovSpec(p)) == D
            assert _spec(rt, fn, sc._p, c, 4, None, lb.RtAov(None, None, p, None), lb.RtAovSpec()) == D
            assert _spec(rt, fn, sc._p, c, 4, lb.RtAovSpecOpts(0, 0.0), None, lb.RtAovSpec(p)) == D
            assert _spec(rt, fn, sc._p, c, 4, lb.RtAovSpecOpts(64, 3.5), None, lb.RtAovSpec(p)) == D
        with pytest.raises(rt.RtError) as e:
            sc.render_aov(cam, n_samples=2, specular=True)
        assert e.value.code == D


def test_python_refuses_specular_with_emit_or_media(rt):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    with rt.Scene(t, w, l) as sc:
        for kw in ({"emit": True}, {"media": True}, {"emit": True, "media": True}):
            with pytest.raises(ValueError):
                sc.render_aov(cam, specular=True, **kw)
        for kw in ({"media": True}, {"scatter": 8}, {"emission": 8}, {"surface_albedo": 8}, {"coverage": 8}):
            with pytest.raises(ValueError):
                sc.render_aov_device(cam, depth=8, specular=True, **kw)
            with pytest.raises(ValueError):
                sc.render_aov_device(cam, depth=8, bounces=8, **kw)
