"""The media-aware feature pass's entry points (include/rt_abi.h: rt_render_aov_media[_device],
rt_accum_resolve_aov_media[_device], RT_ACCUM_FEAT_MEDIA) on a host without a
GPU: the symbols exist with the header's prototypes, rt_aov_media has the header's layout, the
ABI version stays 4, every argument error is RT_ERR_INVALID before any device is touched (a
correct call gets as far as the device: RT_ERR_DEVICE here), the Python wrappers refuse the
feature names they do not know, and `rtbench -aov-media` alone is a usage error."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.cli import CLI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AOV = ("rt_render_aov_media", "rt_render_aov_media_device")
ACC = ("rt_accum_resolve_aov_media", "rt_accum_resolve_aov_media_device")


def test_symbols_exist_and_are_bound(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in AOV + ACC if not hasattr(L, s)] == []
    P = C.POINTER
    lb = rt._lib
    want = {s: [C.c_void_p, P(lb.RtCamera), P(lb.RtRenderOpts), C.c_int32, P(lb.RtAov), P(lb.RtAovEmit),
                P(lb.RtAovMedia), P(lb.RtStats)] for s in AOV}
    want.update({s: [C.c_void_p, P(lb.RtAov), P(lb.RtAovEmit), P(lb.RtAovMedia)] for s in ACC})
    for s, args in want.items():
        f = getattr(rt.lib(), s)
        assert f.restype is C.c_int and list(f.argtypes) == args, s
    assert lb.RT_ACCUM_FEAT_MEDIA == 4
    assert C.sizeof(lb.RtAovMedia) == C.sizeof(C.c_void_p)
    assert set(rt.Accumulator.FEATURES) == {None, "guides", "emit", "guides+media", "emit+media"}
    assert rt.Accumulator.FEATURES["guides+media"] == 5 and rt.Accumulator.FEATURES["emit+media"] == 7


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_c99_client_sees_the_prototypes(rt, tmp_path):
    """the header's prototypes are the library's (a C99 client assigns each entry to a pointer of
    the issue's type, -Werror), the struct is one pointer, the flag is 4, the version stays 4"""
    c = tmp_path / "media.c"
    c.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
        "int main(void){\n"
        "  int (*r)(rt_scene*, const rt_camera*, const rt_render_opts*, int32_t, const rt_aov*, const rt_aov_emit*,\n"
        "           const rt_aov_media*, rt_stats*) = rt_render_aov_media;\n"
        "  int (*rd)(rt_scene*, const rt_camera*, const rt_render_opts*, int32_t, const rt_aov*, const rt_aov_emit*,\n"
        "            const rt_aov_media*, rt_stats*) = rt_render_aov_media_device;\n"
        "  int (*a)(rt_accum*, const rt_aov*, const rt_aov_emit*, const rt_aov_media*) = rt_accum_resolve_aov_media;\n"
        "  int (*ad)(rt_accum*, const rt_aov*, const rt_aov_emit*, const rt_aov_media*) =\n"
        "      rt_accum_resolve_aov_media_device;\n"
        "  rt_aov_media m = {NULL};\n"
        '  printf("%zu %zu %u %d %d\\n", sizeof(rt_aov_media), offsetof(rt_aov_media, scatter), RT_ACCUM_FEAT_MEDIA,\n'
        "         RT_ABI_VERSION, r(NULL, NULL, NULL, 1, NULL, NULL, &m, NULL) + rd(NULL, NULL, NULL, 1, NULL, NULL, &m, NULL)\n"
        "         + a(NULL, NULL, NULL, &m) + ad(NULL, NULL, NULL, &m));\n"
        "  return 0;}\n")
    exe = tmp_path / "media"
    lib_dir = os.path.dirname(rt._lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c), "-o",
                    str(exe), "-L", lib_dir, "-lrt_amd", f"-Wl,-rpath,{lib_dir}"], check=True)
    sz, off, flag, ver, null_sum = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                           text=True, timeout=60).stdout.split())
    assert (sz, off) == (C.sizeof(rt._lib.RtAovMedia), rt._lib.RtAovMedia.scatter.offset)
    assert flag == 4
    assert ver == 4 and rt.lib().rt_abi_version() == 4  # additive: detect by the symbols
    assert null_sum == 4 * rt._lib.RT_ERR_INVALID


def _aov(rt, fn, scene_p, cam_c, n, out, emit, media, rank=0, nranks=1):
    o = rt._lib.RtRenderOpts()
    o.seed, o.rank, o.nranks = 1, rank, nranks
    r = lambda s: None if s is None else C.byref(s)  # noqa: E731
    return getattr(rt.lib(), fn)(scene_p, r(cam_c), C.byref(o), n, r(out), r(emit), r(media), None)


@pytest.mark.parametrize("fn", AOV)
def test_render_aov_media_argument_errors(rt, fn):
    E = rt._lib.RT_ERR_INVALID
    lb = rt._lib
    t, cam, w, l = rt.demo_scene("cornell_smoke")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    buf = np.zeros((8, 8, 3), np.float32)
    p = buf.ctypes.data
    md = lb.RtAovMedia(p)
    with rt.Scene(t, w, l) as sc:
        assert _aov(rt, fn, sc._p, c, 1, lb.RtAov(p, None, None, None), lb.RtAovEmit(p, None, None), None) == E
        assert b"media" in rt.lib().rt_last_error()                       # NULL media: it selects the mode
        assert _aov(rt, fn, sc._p, c, 1, None, None, lb.RtAovMedia()) == E  # no buffer at all
        assert b"no buffer" in rt.lib().rt_last_error()
        assert _aov(rt, fn, sc._p, c, 1, lb.RtAov(), lb.RtAovEmit(), lb.RtAovMedia()) == E
        assert b"no buffer" in rt.lib().rt_last_error()
        assert _aov(rt, fn, None, c, 1, None, None, md) == E              # rt_render_aov's rules
        assert _aov(rt, fn, sc._p, None, 1, None, None, md) == E
        assert _aov(rt, fn, sc._p, c, 5, None, None, md) == E             # spp_sqrt^2 = 4
        assert _aov(rt, fn, sc._p, c, -1, None, None, md) == E
        assert b"samples" in rt.lib().rt_last_error()
        assert _aov(rt, fn, sc._p, c, 1, None, None, md, rank=3, nranks=3) == E
        assert _aov(rt, fn, sc._p, c, 1, None, None, md, rank=-1, nranks=2) == E
        assert b"rank" in rt.lib().rt_last_error()


def test_valid_arguments_reach_the_device(rt):
    """nothing wrong: past the checks, so RT_ERR_DEVICE on a host without a GPU.  out and emit
    may be NULL, and a buffer in any one of the three structs is enough"""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are the gpu tests'
    D = rt._lib.RT_ERR_DEVICE
    lb = rt._lib
    t, cam, w, l = rt.demo_scene("cornell_smoke")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    buf = np.zeros((8, 8, 3), np.float32)
    p = buf.ctypes.data
    with rt.Scene(t, w, l) as sc:
        for fn in AOV:
            assert _aov(rt, fn, sc._p, c, 4, None, None, lb.RtAovMedia(p)) == D
            assert _aov(rt, fn, sc._p, c, 4, lb.RtAov(None, None, p, None), None, lb.RtAovMedia()) == D
            assert _aov(rt, fn, sc._p, c, 4, None, lb.RtAovEmit(None, None, p), lb.RtAovMedia()) == D
        for emit in (False, True):
            with pytest.raises(rt.RtError) as e:
                sc.render_aov(cam, n_samples=2, emit=emit, media=True)
            assert e.value.code == D


def test_null_accumulator_and_null_media_are_refused_by_name(rt):
    E = rt._lib.RT_ERR_INVALID
    L = rt.lib()
    buf = (C.c_float * 3)()
    a = rt._lib.RtAov(C.addressof(buf), None, None, None)
    m = rt._lib.RtAovMedia(C.addressof(buf))
    for name in ACC:
        assert getattr(L, name)(None, C.byref(a), None, C.byref(m)) == E, name
        assert name.encode() in L.rt_last_error(), (name, L.rt_last_error())
        assert getattr(L, name)(None, C.byref(a), None, None) == E, name
    # the mask's own rules need no accumulator to be wrong
    assert L.rt_accum_set_features(None, rt._lib.RT_ACCUM_FEAT_MEDIA) == E
    assert L.rt_accum_set_features(None, 8) == E


def test_python_refuses_the_feature_names_it_does_not_know(rt):
    t, cam, w, l = rt.demo_scene("cornell_smoke")
    cam.Width, cam.SamplesPerPixel = 8, 4
    with rt.Scene(t, w, l) as sc:
        for bad in ("media", "+media", "media+emit", "emit+Media", "guides+emit", 4):
            with pytest.raises(ValueError):
                sc.accumulator(cam, features=bad)


def test_cli_aov_media_alone_is_a_usage_error(tmp_path):
    out = tmp_path / "o.ppm"
    r = subprocess.run([CLI, "-S", "7", "-width", "8", "-spp", "1", "-aov-media", "-o", str(out)],
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 2
    assert "-aov-media needs" in r.stderr and "Usage of" in r.stderr
    assert not out.exists() and list(tmp_path.iterdir()) == []
    h = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "-aov-media" in h.stderr
