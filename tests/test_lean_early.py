"""The emitter slot (csrc/host_records.cpp emitter_slot_of, exported by rt_scene_lean_emitter):
the slot of the scene's one emissive record, reported exactly for the scenes in which the
record-loop kernel may take "the hit scatters" from the winning slot alone -- a listed record
layout, lean light kind 1, one emissive quad in the world, which is the light list's and is
tested as an ordinary record.  No device needed."""
import numpy as np
import pytest

from tests import scenes

LIGHT = ((343, 550, 332), (-130, 0, 0), (0, 0, -105))
# larger than the floor and the ceiling's 555 x 555: the y group's first record (pair 1, half 0)
# instead of its odd one (the mixed pair)
BIG_LIGHT = ((-10, 550, -10), (600, 0, 0), (0, 0, 600))
# between the floor and a smaller ceiling (SMALL_CEILING) in area: the y group's second record
MID_LIGHT = ((540, 550, 540), (-520, 0, 0), (0, 0, -520))
CEILING = ((555, 555, 555), (-555, 0, 0), (0, 0, -555))
SMALL_CEILING = ((525, 555, 525), (-500, 0, 0), (0, 0, -500))


def room(rt, light=LIGHT, boxes=0, lights_weight_1=True, second_emitter=False, tilted=False,
         ceiling=CEILING):
    """scenes.cornell_room with the light quad, the ceiling, an emissive back wall outside the
    lights list, a two-entry lights list and an extra general quad open to the test."""
    t = rt.Tree(1)
    red, white, green = (t.lambertian(c) for c in ((.65, .05, .05), (.73, .73, .73), (.12, .45, .15)))
    lm = t.light((15, 15, 15))
    world = t.list()
    t.add(world, t.quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green))
    t.add(world, t.quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red))
    t.add(world, t.quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white))
    t.add(world, t.quad(*ceiling, white))
    t.add(world, t.quad((0, 0, 555), (555, 0, 0), (0, 555, 0), lm if second_emitter else white))
    lq = t.quad(*light, lm)
    ll = t.list(lq) if lights_weight_1 else t.list(lq, t.list())
    t.add(world, lq)
    if tilted:
        t.add(world, t.quad((100, 100, 400), (50, 10, 0), (0, 50, 10), white))
    if boxes >= 1:
        b1 = t.box((0, 0, 0), (165, 330, 165), white)
        t.add(world, t.translate(t.rotate_y(b1, 15), (265, 0, 295)))
    if boxes >= 2:
        b2 = t.box((0, 0, 0), (165, 165, 165), white)
        t.add(world, t.translate(t.rotate_y(b2, -18), (130, 0, 65)))
    _, cam, _, _ = rt.demo_scene("cornell")
    return t, cam, t.bvh(world), ll


def box_top_light_room(rt):
    """The room's only emissive quad is the top of a box built from six quads (the record
    loop tests the box as slabs); a white panel takes the light's place in the layout."""
    t = rt.Tree(1)
    red, white, green = (t.lambertian(c) for c in ((.65, .05, .05), (.73, .73, .73), (.12, .45, .15)))
    lm = t.light((15, 15, 15))
    world = t.list()
    t.add(world, t.quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green))
    t.add(world, t.quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red))
    t.add(world, t.quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white))
    t.add(world, t.quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white))
    t.add(world, t.quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white))
    t.add(world, t.quad(*LIGHT, white))
    x0, y0, z0, e = 200.0, 0.0, 200.0, 100.0
    top = t.quad((x0, y0 + e, z0), (e, 0, 0), (0, 0, e), lm)
    for q in (t.quad((x0, y0, z0), (e, 0, 0), (0, 0, e), white), top,
              t.quad((x0, y0, z0), (e, 0, 0), (0, e, 0), white),
              t.quad((x0, y0, z0 + e), (e, 0, 0), (0, e, 0), white),
              t.quad((x0, y0, z0), (0, 0, e), (0, e, 0), white),
              t.quad((x0 + e, y0, z0), (0, 0, e), (0, e, 0), white)):
        t.add(world, q)
    _, cam, _, _ = rt.demo_scene("cornell")
    return t, cam, t.bvh(world), t.list(top)


def _slot_of(rt, sc, Q):
    """the slot (2 * pair + half) of the record whose corner is Q in the exported pair array"""
    pairs, n_slots, counts, _, n_boxes = sc.export_records()
    f = pairs[:4 * n_slots].reshape(-1, 32)  # one pair per row (rt_device.h pair layout)
    want = np.array(Q, np.float32).view(np.uint32)
    found = [2 * p + h for p, row in enumerate(f) for h in (0, 1)
             if np.array_equal(row[8 + h:14:2], want) and row[28 + h] != 0]
    assert len(found) == 1, found
    assert f[found[0] // 2][26 + (found[0] & 1)] == found[0]  # the record's own bk word
    return found[0], rt_shape(rt, counts)


def rt_shape(rt, counts):
    import ctypes as C
    return rt.lib().rt_brute_shape((C.c_int32 * 7)(*counts))


ACCEPTED = {
    "demo_cornell": (lambda rt: rt.demo_scene("cornell"), LIGHT, 1),
    "room_2_boxes": (lambda rt: scenes.cornell_room(rt, 2, 1), LIGHT, 1),
    "room_1_box": (lambda rt: scenes.cornell_room(rt, 1, 1), LIGHT, 1),
    "room_0_boxes": (lambda rt: scenes.cornell_room(rt, 0, 1), LIGHT, 2),
    "big_light_boxes": (lambda rt: room(rt, BIG_LIGHT, boxes=2), BIG_LIGHT, 1),
    "big_light_no_boxes": (lambda rt: room(rt, BIG_LIGHT), BIG_LIGHT, 2),
    "mid_light_boxes": (lambda rt: room(rt, MID_LIGHT, boxes=2, ceiling=SMALL_CEILING), MID_LIGHT, 1),
    "mid_light_no_boxes": (lambda rt: room(rt, MID_LIGHT, ceiling=SMALL_CEILING), MID_LIGHT, 2),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_emitter_slot_is_the_lights_record(rt, name):
    make, light, shape = ACCEPTED[name]
    t, _, w, l = make(rt)
    with rt.Scene(t, w, l) as sc:
        slot, got_shape = _slot_of(rt, sc, light[0])
        assert got_shape == shape
        assert sc.lean_light()[0] == 1
        assert sc.lean_emitter() == slot


def test_moved_light_lands_in_other_slots(rt):
    """the three lights take three different slots: the mixed pair's half and both halves of
    the y pair"""
    slots = set()
    for light, ceiling in ((LIGHT, CEILING), (BIG_LIGHT, CEILING), (MID_LIGHT, SMALL_CEILING)):
        t, _, w, l = room(rt, light, boxes=2, ceiling=ceiling)
        with rt.Scene(t, w, l) as sc:
            slots.add(sc.lean_emitter())
    assert len(slots) == 3 and min(slots) >= 0
    assert {s >> 1 for s in slots} == {1, 2} and {s & 1 for s in slots} == {0, 1}


REFUSED = {
    "second_emitter_outside_the_list": lambda rt: room(rt, second_emitter=True),
    "box_face_emitter": box_top_light_room,
    "light_weight_half": lambda rt: room(rt, lights_weight_1=False),
    "two_lights": lambda rt: scenes.cornell_room(rt, 2, 2),
    "unlisted_layout": lambda rt: room(rt, tilted=True),
    "tilted_room": scenes.tilted_room,
    "sphere_light": scenes.sphere_light,
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_other_scenes_have_no_emitter_slot(rt, name):
    t, _, w, l = REFUSED[name](rt)
    with rt.Scene(t, w, l) as sc:
        assert sc.lean_emitter() == -1


def test_refusals_are_for_the_stated_reason(rt):
    """each refused room differs from an accepted one in the one property its name states"""
    t, _, w, l = REFUSED["second_emitter_outside_the_list"](rt)
    with rt.Scene(t, w, l) as sc:
        _, _, counts, _, _ = sc.export_records()
        assert rt_shape(rt, counts) != 0 and sc.lean_light()[0] == 1
    t, _, w, l = REFUSED["box_face_emitter"](rt)
    with rt.Scene(t, w, l) as sc:
        _, _, counts, _, n_boxes = sc.export_records()
        assert rt_shape(rt, counts) == 1 and n_boxes == 1 and sc.lean_light()[0] == 1
    t, _, w, l = REFUSED["light_weight_half"](rt)
    with rt.Scene(t, w, l) as sc:
        _, _, counts, _, _ = sc.export_records()
        assert rt_shape(rt, counts) == 2 and sc.lean_light()[0] == 0
    t, _, w, l = REFUSED["unlisted_layout"](rt)
    with rt.Scene(t, w, l) as sc:
        _, _, counts, _, _ = sc.export_records()
        assert rt_shape(rt, counts) == 0 and sc.lean_light()[0] == 1


def test_null_arguments(rt):
    t, _, w, l = rt.demo_scene("cornell")
    with rt.Scene(t, w, l) as sc:
        assert rt.lib().rt_scene_lean_emitter(sc._p, None) == 0
    assert rt.lib().rt_scene_lean_emitter(None, None) < 0


def test_knob_is_listed_and_validated(rt, tune):
    assert rt.tune_knobs()["RT_LEAN_EARLY_DRAW"] is False  # moves work only
    tune("RT_LEAN_EARLY_DRAW", 0)
    with pytest.raises(rt.RtError, match="rt_tune_set"):
        rt.tune("RT_LEAN_EARLY_DRAW", 2)
    assert rt.tune_get("RT_LEAN_EARLY_DRAW") == "0"
