"""The accumulator's feature-buffer entry points of include/rt_abi.h on a host
without a GPU: the four symbols exist and are bound, a C99 client sees the two flag values and
an unchanged ABI version, and every entry refuses a null accumulator with RT_ERR_INVALID and a
message that names the entry, before any device is touched."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_accum_set_features", "rt_accum_get_features", "rt_accum_resolve_aov",
           "rt_accum_resolve_aov_device")


def test_symbols_exist_and_are_bound(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    for s in SYMBOLS:
        res, args = rt._lib.SIGNATURES[s]
        f = getattr(rt.lib(), s)
        assert f.restype is res and list(f.argtypes) == args and args[0] is C.c_void_p, s
    assert (rt._lib.RT_ACCUM_FEAT_GUIDES, rt._lib.RT_ACCUM_FEAT_EMIT) == (1, 2)
    for name in ("features", "resolve_aov", "resolve_aov_device"):
        assert hasattr(rt.Accumulator, name), name


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_c99_client_sees_the_flags_and_the_version_stays(rt, tmp_path):
    c = tmp_path / "feat.c"
    c.write_text('#include <stdio.h>\n#include "rt_abi.h"\n'
                 "int main(void){\n"
                 "  int (*set)(rt_accum*, uint32_t) = rt_accum_set_features;\n"
                 "  int (*get)(rt_accum*, uint32_t*) = rt_accum_get_features;\n"
                 "  int (*res)(rt_accum*, const rt_aov*, const rt_aov_emit*) = rt_accum_resolve_aov;\n"
                 "  int (*resd)(rt_accum*, const rt_aov*, const rt_aov_emit*) = rt_accum_resolve_aov_device;\n"
                 '  printf("%u %u %d %d\\n", RT_ACCUM_FEAT_GUIDES, RT_ACCUM_FEAT_EMIT, RT_ABI_VERSION,\n'
                 "         set(NULL, 1u) + get(NULL, NULL) + res(NULL, NULL, NULL) + resd(NULL, NULL, NULL));\n"
                 "  return 0;}\n")
    exe = tmp_path / "feat"
    lib_dir = os.path.dirname(rt._lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c), "-o",
                    str(exe), "-L", lib_dir, "-lrt_amd", f"-Wl,-rpath,{lib_dir}"], check=True)
    guides, emit, ver, null_sum = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                          text=True, timeout=60).stdout.split())
    assert (guides, emit) == (1, 2)
    assert ver == 4 and rt.lib().rt_abi_version() == 4  # additive: detect by the symbols
    assert null_sum == 4 * rt._lib.RT_ERR_INVALID


def test_null_accumulator_is_refused_by_name(rt):
    E = rt._lib.RT_ERR_INVALID
    L = rt.lib()
    m = C.c_uint32(7)
    buf = (C.c_float * 3)()
    a = rt._lib.RtAov(C.addressof(buf), None, None, None)
    e = rt._lib.RtAovEmit(None, None, C.addressof(buf))
    calls = {"rt_accum_set_features": (None, 1), "rt_accum_get_features": (None, C.byref(m)),
             "rt_accum_resolve_aov": (None, C.byref(a), C.byref(e)),
             "rt_accum_resolve_aov_device": (None, C.byref(a), C.byref(e))}
    for name, args in calls.items():
        assert getattr(L, name)(*args) == E, name
        assert name.encode() in L.rt_last_error(), (name, L.rt_last_error())
    assert m.value == 7  # untouched
    assert L.rt_accum_set_features(None, 8) == E  # unknown bits, null accumulator: still a code


def test_python_refuses_an_unknown_feature_name(rt):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    with rt.Scene(t, w, l) as sc:
        with pytest.raises(ValueError):
            sc.accumulator(cam, features="material")
