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


def _cornell(rt, boxes=2, lights=1):
    """The Cornell box of the demo scene through the public constructors, with 0-2 boxes
    and 1-2 quad lights."""
    t = rt.Tree(1)
    red, white, green = (t.lambertian(c) for c in ((.65, .05, .05), (.73, .73, .73), (.12, .45, .15)))
    lm = t.light((15, 15, 15))
    world = t.list()
    t.add(world, t.quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green))
    t.add(world, t.quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red))
    t.add(world, t.quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white))
    t.add(world, t.quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white))
    t.add(world, t.quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white))
    ll = t.list()
    t.add(ll, t.quad((343, 550, 332), (-130, 0, 0), (0, 0, -105), lm))
    if lights == 2:
        t.add(ll, t.quad((150, 550, 150), (-60, 0, 0), (0, 0, -60), lm))
    t.add(world, ll)
    if boxes >= 1:
        b1 = t.box((0, 0, 0), (165, 330, 165), white)
        t.add(world, t.translate(t.rotate_y(b1, 15), (265, 0, 295)))
    if boxes >= 2:
        b2 = t.box((0, 0, 0), (165, 165, 165), white)
        t.add(world, t.translate(t.rotate_y(b2, -18), (130, 0, 65)))
    _, cam, _, _ = rt.demo_scene("cornell")
    return t, cam, t.bvh(world), ll


def _tilted_room(rt):
    """The room of test_record_loop_lds_budget_with_shade_table with 20 tilted quads: 23
    records, a layout outside the list."""
    t = rt.Tree(5)
    world, lights = scenes._room(t)
    grey = t.lambertian((0.6, 0.5, 0.4))
    for i in range(20):
        x, z = -6 + (i % 6) * 2.3, -3 + (i // 6) * 1.7
        t.add(world, t.quad((x, 0.5 + 0.1 * i, z), (0.9, 0.3, 0.1), (0.1, 1.1, 0.4), grey))
    return t, scenes._cam(rt, (0, 4, -14), (0, 2, 0)), world, lights


def _scene(rt, name):
    if name == "cornell":
        return rt.demo_scene("cornell")
    if name == "quads":
        return rt.demo_scene("quads")
    if name == "tilted_room":
        return _tilted_room(rt)
    boxes, lights = {"no_boxes": (0, 1), "one_box": (1, 1), "two_lights": (2, 2)}[name]
    return _cornell(rt, boxes, lights)


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
    t, cam, w, l = _scene(rt, name)
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
