"""The pass accumulator's entry points of include/rt_abi.h on a host without a GPU: the symbols
exist and are bound, rt_accum_info has the header's layout, the ABI version is unchanged,
rt_accum_create validates its arguments before any device is touched (RT_ERR_INVALID), and
with valid arguments and no device it returns RT_ERR_DEVICE instead of crashing."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_accum_create", "rt_accum_destroy", "rt_accum_reset", "rt_accum_add",
           "rt_accum_resolve", "rt_accum_resolve_device", "rt_accum_info_get")


def test_symbols_exist_and_are_bound(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    assert hasattr(rt, "Accumulator") and hasattr(rt.Scene, "accumulator")


def test_info_struct_size(rt):
    assert C.sizeof(rt._lib.RtAccumInfo) == 2 * 4 + 2 * 8 + 3 * 8


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_info_struct_matches_header_and_version_stays(rt, tmp_path):
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){'
                 'printf("%zu %zu %zu %d\\n", sizeof(rt_accum_info), offsetof(rt_accum_info, nonfinite_pixels),'
                 " offsetof(rt_accum_info, rel_error), RT_ABI_VERSION);return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    size, off_nf, off_rel, ver = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                         text=True).stdout.split())
    I = rt._lib.RtAccumInfo
    assert (size, off_nf, off_rel) == (C.sizeof(I), I.nonfinite_pixels.offset, I.rel_error.offset)
    assert ver == 4 and rt.lib().rt_abi_version() == 4  # additive: detect by the symbols


def _create(rt, scene_p, cam_c, max_passes=1, out=True, **opts):
    o = rt._lib.RtRenderOpts()
    o.nranks = 1
    for k, v in opts.items():
        setattr(o, k, v)
    p = C.c_void_p()
    rc = rt.lib().rt_accum_create(scene_p, C.byref(cam_c) if cam_c is not None else None, C.byref(o),
                                  max_passes, C.byref(p) if out else None)
    if rc == 0:
        rt.lib().rt_accum_destroy(p)
    else:
        assert not p.value
    return rc


def test_create_argument_errors(rt):
    """Every refusal of rt_accum_create, on any host: none of them needs a device."""
    E = rt._lib.RT_ERR_INVALID
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 16
    c = cam.to_c()
    with rt.Scene(t, w, l) as sc:
        assert _create(rt, None, c) == E
        assert _create(rt, sc._p, None) == E
        assert _create(rt, sc._p, c, out=False) == E
        assert _create(rt, sc._p, c, rank=3, nranks=3) == E
        assert _create(rt, sc._p, c, rank=-1, nranks=2) == E
        assert b"rank" in rt.lib().rt_last_error()
        buf = (C.c_float * 12)()
        assert _create(rt, sc._p, c, trace_out=C.addressof(buf), trace_cap=1) == E
        assert b"trace" in rt.lib().rt_last_error()
        assert _create(rt, sc._p, c, max_passes=-1) == E
        # spp_sqrt^2 * max_passes >= 2^31: 16 * 2^27 is refused, one pass fewer is not
        assert _create(rt, sc._p, c, max_passes=1 << 27) == E
        assert b"2^31" in rt.lib().rt_last_error()
        assert _create(rt, sc._p, c, max_passes=(1 << 27) - 1) != E
        big = rt.Camera(Width=8, SamplesPerPixel=1 << 22)  # 2048^2 samples: 0 = 1024 passes is 2^32
        big.PositionCamera((0, 0, 3), (0, 0, 0))
        assert _create(rt, sc._p, big.to_c(), max_passes=0) == E
        assert _create(rt, sc._p, big.to_c(), max_passes=511) != E
        for fn in ("rt_accum_reset", "rt_accum_resolve", "rt_accum_info_get", "rt_accum_add"):
            args = {"rt_accum_reset": (None,), "rt_accum_resolve": (None, None, None),
                    "rt_accum_info_get": (None, None), "rt_accum_add": (None, 1, None)}[fn]
            assert getattr(rt.lib(), fn)(*args) == E, fn
        assert rt.lib().rt_accum_destroy(None) == 0
        with pytest.raises(rt.RtError) as e:
            sc.accumulator(cam, max_passes=-2)
        assert e.value.code == E


def test_no_device_is_a_code_not_a_crash(rt):
    """Valid arguments on a host without a GPU: RT_ERR_DEVICE, from C and from Python."""
    if rt.device_count() > 0:
        pytest.skip("a HIP device is visible: covered by tests/test_accum_gpu.py")
    D = rt._lib.RT_ERR_DEVICE
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 8, 4
    with rt.Scene(t, w, l) as sc:
        assert _create(rt, sc._p, cam.to_c(), max_passes=0) == D
        assert _create(rt, sc._p, cam.to_c(), max_passes=8, rank=1, nranks=3) == D
        with pytest.raises(rt.RtError) as e:
            sc.accumulator(cam)
        assert e.value.code == D
