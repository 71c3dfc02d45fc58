"""The adaptive-pass entry points of include/rt_abi.h on a host without a GPU:
the symbols exist and are bound, the structs have the header's layout, the ABI version is
unchanged, and every bad argument is refused with RT_ERR_INVALID before a device is touched.

An accumulator cannot be created without a device, so the handle is NULL in every call here.
The options and the mask pointer are checked before the handle (rt_abi.h), and the message of
rt_last_error tells which check refused the call."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_accum_select", "rt_accum_set_active", "rt_accum_add_active", "rt_accum_counts",
           "rt_accum_counts_device", "rt_accum_tile_error", "rt_accum_adapt_info")


def test_symbols_exist_and_are_bound(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    for m in ("select", "set_active", "add_active", "counts", "tile_error", "adapt_info", "render_adaptive"):
        assert hasattr(rt.Accumulator, m), m


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_structs_match_header_and_version_stays(rt, tmp_path):
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){'
                 'printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(rt_adapt_opts), offsetof(rt_adapt_opts, tile),'
                 " offsetof(rt_adapt_opts, min_passes), sizeof(rt_adapt_info), offsetof(rt_adapt_info, min_count),"
                 " offsetof(rt_adapt_info, active_tiles), RT_ABI_VERSION);return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    O, I = rt._lib.RtAdaptOpts, rt._lib.RtAdaptInfo
    assert got[:6] == [C.sizeof(O), O.tile.offset, O.min_passes.offset, C.sizeof(I), I.min_count.offset,
                       I.active_tiles.offset]
    assert got[6] == 4 and rt.lib().rt_abi_version() == 4  # additive: detect by the symbols


def _opts(rt, rel_error=0.1, lum_floor=0.0, tile=0, min_passes=0):
    return rt._lib.RtAdaptOpts(rel_error, lum_floor, tile, min_passes)


def test_argument_errors(rt):
    """Every refusal that needs no accumulator, on any host."""
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    n = C.c_uint64(7)
    err = lambda: L.rt_last_error()
    # NULL handle with otherwise valid arguments
    assert L.rt_accum_select(None, C.byref(_opts(rt)), C.byref(n)) == E and b"null accumulator" in err()
    assert L.rt_accum_add_active(None, 1, None) == E
    assert L.rt_accum_counts(None, None) == E and L.rt_accum_counts_device(None, None) == E
    assert L.rt_accum_adapt_info(None, None) == E
    mask = (C.c_uint8 * 4)()
    assert L.rt_accum_set_active(None, C.addressof(mask), C.byref(n)) == E and b"null accumulator" in err()
    assert L.rt_accum_tile_error(None, C.byref(_opts(rt)), None, None, None) == E and b"null accumulator" in err()
    # the options, refused before the handle is looked at
    for fn, extra in ((L.rt_accum_select, (C.byref(n),)), (L.rt_accum_tile_error, (None, None, None))):
        assert fn(None, None, *extra) == E and b"options" in err()
        for bad in (0.0, -1.0, float("nan")):
            assert fn(None, C.byref(_opts(rt, rel_error=bad)), *extra) == E and b"rel_error" in err()
        assert fn(None, C.byref(_opts(rt, lum_floor=-1.0)), *extra) == E and b"lum_floor" in err()
        for bad in (65, -1):
            assert fn(None, C.byref(_opts(rt, tile=bad)), *extra) == E and b"tile" in err()
        for bad in (1, -3):
            assert fn(None, C.byref(_opts(rt, min_passes=bad)), *extra) == E and b"min_passes" in err()
        # the limits themselves pass the option checks: the handle is what is refused
        assert fn(None, C.byref(_opts(rt, tile=64, min_passes=2)), *extra) == E and b"null accumulator" in err()
        assert fn(None, C.byref(_opts(rt, tile=1)), *extra) == E and b"null accumulator" in err()
    # a NULL mask
    assert L.rt_accum_set_active(None, None, C.byref(n)) == E and b"mask" in err()
    assert n.value == 7  # no output was written
