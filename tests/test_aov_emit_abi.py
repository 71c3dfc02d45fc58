"""The emission split's entry points (include/rt_abi.h: rt_render_aov_emit[_device],
rt_denoise_emit[_device], rt_denoise_var_emit[_device]) on a host without a GPU: the symbols
exist, rt_aov_emit has the header's layout, every argument error is RT_ERR_INVALID before any
device is touched, the Python wrappers refuse an aov dict without the three split buffers, and
`rtbench -split-emitters` alone is a usage error that creates no file."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.cli import CLI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AOV = ("rt_render_aov_emit", "rt_render_aov_emit_device")
DN = ("rt_denoise_emit", "rt_denoise_emit_device")
DV = ("rt_denoise_var_emit", "rt_denoise_var_emit_device")


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in AOV + DN + DV if not hasattr(L, s)] == []
    assert set(AOV + DN + DV) <= set(rt._lib.SIGNATURES)


def test_struct_size(rt):
    assert C.sizeof(rt._lib.RtAovEmit) == 3 * C.sizeof(C.c_void_p)
    assert C.sizeof(rt._lib.RtAov) == 4 * C.sizeof(C.c_void_p)  # unchanged


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_struct_matches_header(rt, tmp_path):
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){'
                 'printf("%zu %zu %zu %zu %d\\n", sizeof(rt_aov_emit), offsetof(rt_aov_emit, surface_albedo),'
                 " offsetof(rt_aov_emit, coverage), sizeof(rt_aov), RT_ABI_VERSION);"
                 "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    sz, o1, o2, aov, ver = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.split())
    E = rt._lib.RtAovEmit
    assert (sz, o1, o2) == (C.sizeof(E), E.surface_albedo.offset, E.coverage.offset)
    assert aov == C.sizeof(rt._lib.RtAov)
    assert ver == 4  # additive: callers detect the feature by the symbols


def _aov(rt, fn, scene_p, cam_c, n, out, emit, rank=0, nranks=1):
    o = rt._lib.RtRenderOpts()
    o.seed, o.rank, o.nranks = 1, rank, nranks
    return getattr(rt.lib(), fn)(scene_p, None if cam_c is None else C.byref(cam_c), C.byref(o), n,
                                 None if out is None else C.byref(out),
                                 None if emit is None else C.byref(emit), None)


@pytest.mark.parametrize("fn", AOV)
def test_render_aov_emit_argument_errors(rt, fn):
    E = rt._lib.RT_ERR_INVALID
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    buf = np.zeros((8, 8, 3), np.float32)
    em = rt._lib.RtAovEmit(buf.ctypes.data, None, None)
    with rt.Scene(t, w, l) as sc:
        assert _aov(rt, fn, sc._p, c, 1, rt._lib.RtAov(buf.ctypes.data, None, None, None), None) == E
        assert b"emit" in rt.lib().rt_last_error()                       # NULL emit struct
        assert _aov(rt, fn, sc._p, c, 1, None, rt._lib.RtAovEmit()) == E  # no buffer at all
        assert _aov(rt, fn, sc._p, c, 1, rt._lib.RtAov(), rt._lib.RtAovEmit()) == E
        assert b"no buffer" in rt.lib().rt_last_error()
        assert _aov(rt, fn, None, c, 1, None, em) == E                   # rt_render_aov's rules
        assert _aov(rt, fn, sc._p, None, 1, None, em) == E
        assert _aov(rt, fn, sc._p, c, 5, None, em) == E                  # spp_sqrt^2 = 4
        assert _aov(rt, fn, sc._p, c, -1, None, em) == E
        assert b"samples" in rt.lib().rt_last_error()
        assert _aov(rt, fn, sc._p, c, 1, None, em, rank=3, nranks=3) == E
        assert _aov(rt, fn, sc._p, c, 1, None, em, rank=-1, nranks=2) == E
        assert b"rank" in rt.lib().rt_last_error()


def _dn(rt, fn, rgb, var, feat, emit, w, h, opts, out, var_out=None):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    r = lambda s: None if s is None else C.byref(s)  # noqa: E731
    args = [p(rgb)] + ([p(var)] if fn in DV else []) + [r(feat), r(emit), w, h, r(opts), p(out)]
    if fn in DV:
        args.append(p(var_out))
    if fn.endswith("_device"):
        args += [0, None]
    return getattr(rt.lib(), fn)(*args)


@pytest.mark.parametrize("fn", DN + DV)
def test_denoise_emit_argument_errors(rt, fn):
    E = rt._lib.RT_ERR_INVALID
    O = rt._lib.RtDenoiseVarOpts if fn in DV else rt._lib.RtDenoiseOpts
    rgb = np.zeros((4, 4, 3), np.float32)
    var = np.zeros((4, 4), np.float32)
    cov = np.zeros((4, 4), np.float32)
    out = np.zeros_like(rgb)
    p = rgb.ctypes.data
    full = rt._lib.RtAovEmit(p, p, cov.ctypes.data)
    assert _dn(rt, fn, rgb, var, None, None, 4, 4, None, out) == E        # NULL emit
    assert b"emission" in rt.lib().rt_last_error()
    for miss in ((None, p, cov.ctypes.data), (p, None, cov.ctypes.data), (p, p, None)):
        assert _dn(rt, fn, rgb, var, None, rt._lib.RtAovEmit(*miss), 4, 4, None, out) == E, miss
        assert b"coverage" in rt.lib().rt_last_error()
    assert _dn(rt, fn, rgb, var, None, full, 0, 4, None, out) == E        # w, h <= 0
    assert _dn(rt, fn, rgb, var, None, full, 4, -1, None, out) == E
    assert _dn(rt, fn, rgb, var, None, full, 1, 4 * 65535 + 1, None, out) == E
    assert _dn(rt, fn, None, var, None, full, 4, 4, None, out) == E       # null image
    assert _dn(rt, fn, rgb, var, None, full, 4, 4, None, None) == E
    if fn in DV:
        assert _dn(rt, fn, rgb, None, None, full, 4, 4, None, out) == E   # null variance
        assert b"variance" in rt.lib().rt_last_error()
    for it in (9, -1):
        o = O()
        o.iterations = it
        assert _dn(rt, fn, rgb, var, None, full, 4, 4, o, out) == E
    for field in ("sigma_lum" if fn in DV else "sigma_color", "sigma_normal", "sigma_depth"):
        for bad in (-1.0, float("nan")):
            o = O()
            setattr(o, field, bad)
            assert _dn(rt, fn, rgb, var, None, full, 4, 4, o, out) == E, (field, bad)


def test_valid_arguments_reach_the_device(rt):
    """with nothing wrong the calls get past the checks (demodulating without feat->albedo, and
    with a NULL feat, included): RT_ERR_DEVICE on a host without a GPU"""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are the gpu tests'
    D = rt._lib.RT_ERR_DEVICE
    rgb = np.zeros((4, 4, 3), np.float32)
    var = np.zeros((4, 4), np.float32)
    cov = np.zeros((4, 4), np.float32)
    full = rt._lib.RtAovEmit(rgb.ctypes.data, rgb.ctypes.data, cov.ctypes.data)
    for fn in DN + DV:
        o = (rt._lib.RtDenoiseVarOpts if fn in DV else rt._lib.RtDenoiseOpts)()
        o.demodulate = 1
        assert _dn(rt, fn, rgb, var, None, full, 4, 4, o, rgb, var) == D
        assert _dn(rt, fn, rgb, var, rt._lib.RtAov(), full, 4, 4, o, rgb) == D
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    c = cam.to_c()
    buf = np.zeros((8, 8, 3), np.float32)
    with rt.Scene(t, w, l) as sc:
        for fn in AOV:
            assert _aov(rt, fn, sc._p, c, 4, None, rt._lib.RtAovEmit(buf.ctypes.data, None, None)) == D
        with pytest.raises(rt.RtError) as e:
            sc.render_aov(cam, n_samples=2, emit=True)
        assert e.value.code == D


def test_python_wrappers_need_the_split_buffers(rt):
    import torch
    rgb = np.zeros((4, 6, 3), np.float32)
    var = np.zeros((4, 6), np.float32)
    good = {"emission": rgb, "surface_albedo": rgb, "coverage": var}
    for drop in good:
        aov = {k: v for k, v in good.items() if k != drop}
        with pytest.raises(ValueError):
            rt.denoise(rgb, aov, split_emitters=True)
        with pytest.raises(ValueError):
            rt.denoise_var(rgb, var, aov, split_emitters=True)
    with pytest.raises(ValueError):
        rt.denoise(rgb, None, split_emitters=True)
    for key, bad in (("coverage", np.zeros((6, 4), np.float32)), ("emission", np.zeros((4, 6), np.float32)),
                     ("surface_albedo", np.zeros((4, 6, 4), np.float32))):
        with pytest.raises(ValueError):
            rt.denoise_var(rgb, var, dict(good, **{key: bad}), split_emitters=True)
    t, tv = torch.zeros((4, 6, 3)), torch.zeros((4, 6))
    tg = {"emission": t, "surface_albedo": t, "coverage": tv}
    for drop in tg:
        aov = {k: v for k, v in tg.items() if k != drop}
        with pytest.raises(ValueError):
            rt.denoise_device(t, aov, split_emitters=True)
        with pytest.raises(ValueError):
            rt.denoise_var_device(t, tv, aov, split_emitters=True)
    for key, bad in (("coverage", torch.zeros((6, 4))), ("coverage", torch.zeros((4, 6), dtype=torch.float64)),
                     ("coverage", torch.zeros((4, 12))[:, ::2]), ("coverage", var),
                     ("emission", torch.zeros((4, 6, 6))[..., ::2])):
        with pytest.raises(ValueError):
            rt.denoise_var_device(t, tv, dict(tg, **{key: bad}), split_emitters=True)
        with pytest.raises(ValueError):
            rt.denoise_device(t, dict(tg, **{key: bad}), split_emitters=True)


def test_cli_split_emitters_alone_is_a_usage_error(tmp_path):
    out = tmp_path / "o.ppm"
    r = subprocess.run([CLI, "-S", "6", "-width", "8", "-spp", "1", "-split-emitters", "-o", str(out)],
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 2
    assert "-split-emitters needs" in r.stderr and "Usage of" in r.stderr
    assert not out.exists() and list(tmp_path.iterdir()) == []
    h = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "-split-emitters" in h.stderr
