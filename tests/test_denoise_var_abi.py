"""rt_denoise_var / rt_denoise_var_device (include/rt_abi.h) on a host without a GPU: the
symbols exist, rt_denoise_var_opts is 24 bytes in ctypes and in the header, every argument
error is RT_ERR_INVALID before any device is touched, and the Python wrappers refuse a missing
or mis-shaped variance."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_denoise_var", "rt_denoise_var_device")


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    assert {"denoise_var", "denoise_var_device", "RtDenoiseVarOpts"} <= set(rt.__all__)


def test_struct_size(rt):
    assert C.sizeof(rt._lib.RtDenoiseVarOpts) == 24
    assert C.sizeof(rt._lib.RtDenoiseOpts) == 24  # unchanged


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_struct_size_matches_header(rt, tmp_path):
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){'
                 'printf("%zu %zu %zu %d\\n", sizeof(rt_denoise_var_opts), sizeof(rt_denoise_opts),'
                 " offsetof(rt_denoise_var_opts, sigma_lum), RT_ABI_VERSION);"
                 "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    v, d, off, ver = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                             text=True).stdout.split())
    assert v == C.sizeof(rt._lib.RtDenoiseVarOpts) == 24 and d == 24
    assert off == rt._lib.RtDenoiseVarOpts.sigma_lum.offset == 8
    assert ver == 4  # additive: callers detect the feature by the symbols


def _dv(rt, fn, rgb, var, feat, w, h, opts, out, var_out=None):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    args = [p(rgb), p(var), C.byref(feat) if feat is not None else None, w, h,
            C.byref(opts) if opts is not None else None, p(out), p(var_out)]
    if fn == "rt_denoise_var_device":
        args += [0, None]
    return getattr(rt.lib(), fn)(*args)


@pytest.mark.parametrize("fn", SYMBOLS)
def test_argument_errors(rt, fn):
    E = rt._lib.RT_ERR_INVALID
    O = rt._lib.RtDenoiseVarOpts
    rgb = np.zeros((4, 4, 3), np.float32)
    var = np.zeros((4, 4), np.float32)
    out = np.zeros_like(rgb)
    alb = np.ones_like(rgb)
    feat = rt._lib.RtAov(alb.ctypes.data, None, None, None)
    assert _dv(rt, fn, rgb, var, None, 0, 4, None, out) == E          # size
    assert _dv(rt, fn, rgb, var, None, 4, -1, None, out) == E
    assert _dv(rt, fn, rgb, var, None, 1 << 16, 1 << 16, None, out) == E
    assert _dv(rt, fn, rgb, var, None, 1, 4 * 65535 + 1, None, out) == E  # the grid's height limit
    assert _dv(rt, fn, None, var, None, 4, 4, None, out) == E          # null image
    assert _dv(rt, fn, rgb, var, None, 4, 4, None, None) == E
    assert b"null image" in rt.lib().rt_last_error()
    assert _dv(rt, fn, rgb, None, None, 4, 4, None, out) == E          # null variance
    assert b"variance" in rt.lib().rt_last_error()
    assert _dv(rt, fn, rgb, None, feat, 4, 4, O(), out, var) == E
    for it in (9, -1):                                                 # iterations range
        o = O()
        o.iterations = it
        assert _dv(rt, fn, rgb, var, feat, 4, 4, o, out) == E
    o = O()
    o.demodulate = 1
    assert _dv(rt, fn, rgb, var, None, 4, 4, o, out) == E              # demodulate without albedo
    assert _dv(rt, fn, rgb, var, rt._lib.RtAov(), 4, 4, o, out) == E
    assert b"albedo" in rt.lib().rt_last_error()
    for field in ("sigma_lum", "sigma_normal", "sigma_depth"):         # negative or NaN sigma
        for bad in (-1.0, float("nan")):
            o = O()
            setattr(o, field, bad)
            assert _dv(rt, fn, rgb, var, None, 4, 4, o, out) == E, (field, bad)


def test_valid_arguments_reach_the_device(rt):
    """with nothing wrong the call gets past the checks: RT_ERR_DEVICE on a host without a GPU"""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are tests/test_denoise_var_gpu.py's
    rgb = np.zeros((4, 4, 3), np.float32)
    var = np.zeros((4, 4), np.float32)
    for fn in SYMBOLS:
        assert _dv(rt, fn, rgb, var, None, 4, 4, None, rgb, var) == rt._lib.RT_ERR_DEVICE
        assert _dv(rt, fn, rgb, var, None, 4, 4, None, rgb, None) == rt._lib.RT_ERR_DEVICE


def test_python_wrappers_refuse_a_bad_var(rt):
    import torch
    rgb = np.zeros((4, 6, 3), np.float32)
    with pytest.raises(ValueError):
        rt.denoise_var(rgb, None)
    for bad in (np.zeros((6, 4), np.float32), np.zeros((4, 6, 3), np.float32), np.zeros(24, np.float32)):
        with pytest.raises(ValueError):
            rt.denoise_var(rgb, bad)
    t = torch.zeros((4, 6, 3))
    for bad in (None, torch.zeros((6, 4)), torch.zeros((4, 6), dtype=torch.float64),
                torch.zeros((4, 12))[:, ::2], np.zeros((4, 6), np.float32)):
        with pytest.raises(ValueError):
            rt.denoise_var_device(t, bad)
    for bad in (torch.zeros((6, 4)), torch.zeros((4, 6), dtype=torch.float64), torch.zeros((4, 12))[:, ::2]):
        with pytest.raises(ValueError):
            rt.denoise_var_device(t, torch.zeros((4, 6)), var_out=bad)
