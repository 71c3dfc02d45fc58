"""The record loop compiled for a scene's record layout (rt_device.h brute_shape,
k_fused<true, 0, 0, SHAPE>) finds the hits of the generic loop bit for bit, and the host
matcher sends exactly the listed layouts to it."""
import ctypes as C

import numpy as np
import pytest

from tests import scenes

# counts: general, y-parallel, x, y, z axis-aligned pairs, mixed-pair code, box pairs
MIX_XY, MIX_XZ, MIX_YZ = 1 | (2 << 2), 1 | (3 << 2), 2 | (3 << 2)
LISTED = {1: (0, 0, 1, 1, 0, MIX_YZ, 1),   # Cornell: one or two boxes
          2: (0, 0, 1, 1, 0, MIX_YZ, 0)}   # Cornell without boxes


def _shape(rt, counts):
    return rt.lib().rt_brute_shape((C.c_int32 * 7)(*counts))


def test_listed_layouts_map_to_their_shape(rt):
    for sid, counts in LISTED.items():
        assert _shape(rt, counts) == sid


@pytest.mark.parametrize("sid", sorted(LISTED))
@pytest.mark.parametrize("field", range(7))
def test_layout_off_by_one_is_generic(rt, sid, field):
    """One more or one fewer in any single count (for the mixed pair: every other code)
    is not the listed layout."""
    base = LISTED[sid]
    if field == 5:
        others = [m for m in (0, MIX_XY, MIX_XZ, MIX_YZ) if m != base[5]]
    else:
        others = [v for v in (base[field] - 1, base[field] + 1) if v >= 0]
    for v in others:
        counts = base[:field] + (v,) + base[field + 1:]
        other_listed = [s for s, c in LISTED.items() if c == counts]
        assert _shape(rt, counts) == (other_listed[0] if other_listed else 0), counts


def test_unlisted_layouts_are_generic(rt):
    """Every count at 24 pairs (kBruteMax = 48 records), and no records at all."""
    for mx in (0, MIX_XY, MIX_XZ, MIX_YZ):
        assert _shape(rt, (24, 24, 24, 24, 24, mx, 24)) == 0
    assert _shape(rt, (0, 0, 0, 0, 0, 0, 0)) == 0


def _both(rt, tune, t, cam, w, l, record_loop=True, **kw):
    out = []
    for flag in ("0", "1"):
        tune("RT_BRUTE_SHAPE", flag)
        with rt.Scene(t, w, l) as sc:
            img, st = sc.render(cam, **kw)
        assert not record_loop or st["tree_width"] == 0
        out.append((img, st))
    (a, sa), (b, sb) = out
    assert a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sa["segments"] == sb["segments"] and sa["samples"] == sb["samples"]
    return sb


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "no_boxes", "one_box", "quads", "tilted_room",
                                  "two_lights"])
def test_shaped_record_loop_matches_generic(rt, gpu, tune, name):
    """RT_BRUTE_SHAPE=0 (generic kernel) and 1 (the layout's kernel when listed) in one
    process: the same image bits and the same segment count.  Cornell as shipped, without
    boxes and with one box are listed layouts; the quads demo (general pairs, another
    feature set), the 23-record room and a Cornell with two lights are not, so both settings
    run the generic kernel there."""
    t, cam, w, l = scenes.record_scene(rt, name)
    cam.Width, cam.SamplesPerPixel = 48, 16
    st = _both(rt, tune, t, cam, w, l, record_loop=name != "quads", seed=5)
    if name in ("cornell", "no_boxes", "one_box", "two_lights"):
        assert st["kernel_features"] == 0  # the lean set
        assert st["record_boxes"] == {"cornell": 2, "no_boxes": 0, "one_box": 1, "two_lights": 2}[name]


@pytest.mark.gpu
def test_shaped_record_loop_with_progress_slices(rt, gpu, tune):
    """1,024 progress slices at test_cli_short_progress_slices_terminate's sizes (slices
    shorter than one chunk batch, the drain split on): the chunk bookkeeping around the
    loop is the generic kernel's."""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel, cam.MaxDepth = 40, 9, 6
    sliced = _both(rt, tune, t, cam, w, l, seed=5, progress_slices=1024)
    with rt.Scene(t, w, l) as sc:
        one, st = sc.render(cam, seed=5)
    assert st["segments"] == sliced["segments"]


@pytest.mark.gpu
def test_brute_max_raised_after_upload_takes_the_bvh4(rt, gpu, tune):
    """A room of 103 leaf entries (over the 64 a device copy carries record pairs and a BVH2
    for, under 128) renders through the BVH4.  RT_BRUTE_MAX=128 set after the upload asks for
    the record loop, whose pairs this copy does not have: the render keeps the BVH4, bit for
    bit, as the feature pass always did."""
    t, cam, w, l = scenes.tilted_room(rt, 100)
    cam.Width, cam.SamplesPerPixel = 32, 4
    with rt.Scene(t, w, l) as sc:
        assert 64 < len(sc.export_bvh()[1]) < 128
        a, sa = sc.render(cam, seed=7)
        tune("RT_BRUTE_MAX", "128")
        b, sb = sc.render(cam, seed=7)
    assert sa["tree_width"] == 4 and sb["tree_width"] == 4
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
