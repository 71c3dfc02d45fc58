"""The feature-buffer and denoiser entry points of include/rt_abi.h on a host without a GPU:
the symbols exist, the ctypes layouts match the header, arguments are validated before any
device is touched (RT_ERR_INVALID), and with valid arguments and no device the calls return
RT_ERR_DEVICE instead of crashing."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_render_aov", "rt_render_aov_device", "rt_denoise", "rt_denoise_device")


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)


def test_struct_sizes(rt):
    assert C.sizeof(rt._lib.RtAov) == 4 * C.sizeof(C.c_void_p)
    if C.sizeof(C.c_void_p) == 8:
        assert C.sizeof(rt._lib.RtAov) == 32  # LP64
    assert C.sizeof(rt._lib.RtDenoiseOpts) == 24


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_struct_sizes_match_header(rt, tmp_path):
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include "rt_abi.h"\nint main(void){'
                 'printf("%zu %zu %d\\n", sizeof(rt_aov), sizeof(rt_denoise_opts), RT_ABI_VERSION);'
                 "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    a, d, ver = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                        text=True).stdout.split())
    assert (a, d) == (C.sizeof(rt._lib.RtAov), C.sizeof(rt._lib.RtDenoiseOpts))
    assert ver == 4  # additive: callers detect the feature by the symbols


def _aov_call(rt, fn, scene_p, cam_c, n_samples, aov=None):
    o = rt._lib.RtRenderOpts()
    o.seed, o.nranks = 1, 1
    a = aov if aov is not None else rt._lib.RtAov()
    return getattr(rt.lib(), fn)(scene_p, C.byref(cam_c) if cam_c is not None else None,
                                 C.byref(o), n_samples, C.byref(a), None)


@pytest.mark.parametrize("fn", ["rt_render_aov", "rt_render_aov_device"])
def test_render_aov_argument_errors(rt, fn):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    with rt.Scene(t, w, l) as sc:
        assert _aov_call(rt, fn, None, c, 1) == rt._lib.RT_ERR_INVALID
        assert _aov_call(rt, fn, sc._p, None, 1) == rt._lib.RT_ERR_INVALID
        assert _aov_call(rt, fn, sc._p, c, 5) == rt._lib.RT_ERR_INVALID  # spp_sqrt^2 = 4
        assert _aov_call(rt, fn, sc._p, c, -1) == rt._lib.RT_ERR_INVALID
        assert b"samples" in rt.lib().rt_last_error()
        o = rt._lib.RtRenderOpts()
        o.rank, o.nranks = 3, 3
        a = rt._lib.RtAov()
        assert getattr(rt.lib(), fn)(sc._p, C.byref(c), C.byref(o), 1, C.byref(a),
                                     None) == rt._lib.RT_ERR_INVALID


def _dn(rt, fn, rgb, feat, w, h, opts, out):
    args = [rgb.ctypes.data, C.byref(feat) if feat is not None else None, w, h,
            C.byref(opts) if opts is not None else None, out.ctypes.data]
    if fn == "rt_denoise_device":
        args += [0, None]
    return getattr(rt.lib(), fn)(*args)


@pytest.mark.parametrize("fn", ["rt_denoise", "rt_denoise_device"])
def test_denoise_argument_errors(rt, fn):
    E = rt._lib.RT_ERR_INVALID
    rgb = np.zeros((4, 4, 3), np.float32)
    out = np.zeros_like(rgb)
    alb = np.ones_like(rgb)
    assert _dn(rt, fn, rgb, None, 0, 4, None, out) == E
    assert _dn(rt, fn, rgb, None, 4, -1, None, out) == E
    o = rt._lib.RtDenoiseOpts()
    o.demodulate = 1
    assert _dn(rt, fn, rgb, None, 4, 4, o, out) == E  # demodulate without a feature struct
    assert _dn(rt, fn, rgb, rt._lib.RtAov(), 4, 4, o, out) == E  # ... without an albedo
    assert b"albedo" in rt.lib().rt_last_error()
    o = rt._lib.RtDenoiseOpts()
    o.iterations = 9
    assert _dn(rt, fn, rgb, rt._lib.RtAov(alb.ctypes.data, None, None, None), 4, 4, o, out) == E
    o.iterations = -1
    assert _dn(rt, fn, rgb, None, 4, 4, o, out) == E
    o = rt._lib.RtDenoiseOpts()
    o.sigma_color = -1.0
    assert _dn(rt, fn, rgb, None, 4, 4, o, out) == E


def test_no_device_is_a_code_not_a_crash(rt):
    """Valid arguments on a host without a GPU: RT_ERR_DEVICE from all four entry points."""
    if rt.device_count() > 0:
        pytest.skip("a HIP device is visible: covered by tests/test_aov_gpu.py")
    D = rt._lib.RT_ERR_DEVICE
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    alb = np.zeros((8, 8, 3), np.float32)
    with rt.Scene(t, w, l) as sc:
        a = rt._lib.RtAov(alb.ctypes.data, None, None, None)
        assert _aov_call(rt, "rt_render_aov", sc._p, c, 4, a) == D
        assert _aov_call(rt, "rt_render_aov_device", sc._p, c, 0, a) == D
        with pytest.raises(rt.RtError) as e:
            sc.render_aov(cam, n_samples=2)
        assert e.value.code == D
    rgb = np.zeros((4, 4, 3), np.float32)
    assert _dn(rt, "rt_denoise", rgb, None, 4, 4, None, rgb) == D
    assert _dn(rt, "rt_denoise_device", rgb, None, 4, 4, None, rgb) == D
    with pytest.raises(rt.RtError) as e:
        rt.denoise(rgb)
    assert e.value.code == D


def test_denoise_height_above_the_grid_limit(rt):
    """one block row per 4 image rows: a height the launch grid cannot hold is refused"""
    rgb = np.zeros((4, 4, 3), np.float32)
    for fn in ("rt_denoise", "rt_denoise_device"):
        assert _dn(rt, fn, rgb, None, 1, 4 * 65535 + 1, None, rgb) == rt._lib.RT_ERR_INVALID
