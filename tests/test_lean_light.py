"""The lean light kind (rt_device.h "lean light kinds"): the host matcher lean_light_of
(csrc/host_records.cpp, exported by rt_scene_lean_light) sends exactly the one-quad-light
scenes whose light lies on the y axis to the record-loop kernel compiled for them, and the
block it packs is a copy of the light's own fields.  No device needed.

Block layout (include/rt_abi.h): [0..2] Q, [3] D / n_y, [4..6] A, [7] area, [8..10] B,
[12..14] u, [16..18] v."""
import numpy as np
import pytest

from tests import scenes

LIGHT_Q, LIGHT_U, LIGHT_V, LIGHT_AREA = (343, 550, 332), (-130, 0, 0), (0, 0, -105), 13650.0


def _f32(*v):
    return np.array(v, np.float32).view(np.uint32)


def _room(rt, light=(LIGHT_Q, LIGHT_U, LIGHT_V), red=(.65, .05, .05), extra_lights=()):
    """scenes.cornell_room without boxes, with the light quad, one albedo and the lights
    list open to the test."""
    t = rt.Tree(1)
    r, white, green = (t.lambertian(c) for c in (red, (.73, .73, .73), (.12, .45, .15)))
    lm = t.light((15, 15, 15))
    world = t.list()
    t.add(world, t.quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green))
    t.add(world, t.quad((0, 0, 0), (0, 555, 0), (0, 0, 555), r))
    t.add(world, t.quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white))
    t.add(world, t.quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white))
    t.add(world, t.quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white))
    ll = t.list()
    t.add(ll, t.quad(*light, lm))
    for e in extra_lights:
        t.add(ll, e(t))
    t.add(world, ll)
    _, cam, _, _ = rt.demo_scene("cornell")
    return t, cam, t.bvh(world), ll


def x_wall_room(rt):
    """the light on the x = 555 wall: normal +-e_x (only y is a listed kind)"""
    return _room(rt, light=((554, 343, 332), (0, 0, -105), (0, -130, 0)))


def tilted_light_room(rt):
    """v = (0, 5, -105): the normal leaves the y axis and A_y != 0"""
    return _room(rt, light=(LIGHT_Q, LIGHT_U, (0, 5, -105)))


def light_and_empty_list_room(rt):
    """lights = list(light, list()): two entries, one of them PRIM_NONE"""
    return _room(rt, extra_lights=(lambda t: t.list(),))


def negative_albedo_room(rt):
    """one albedo below zero: merge_ok is 0"""
    return _room(rt, red=(-0.1, 0.5, 0.5))


LISTED = {
    "demo_cornell": lambda rt: rt.demo_scene("cornell"),
    "room_0_boxes": lambda rt: scenes.cornell_room(rt, 0, 1),
    "room_1_box": lambda rt: scenes.cornell_room(rt, 1, 1),
    "room_2_boxes": lambda rt: scenes.cornell_room(rt, 2, 1),
}
GENERAL = {
    "two_lights": lambda rt: scenes.cornell_room(rt, 2, 2),
    "x_wall": x_wall_room,  # the one line to change when a kind for x is listed
    "tilted_light": tilted_light_room,
    "light_and_empty_list": light_and_empty_list_room,
    "negative_albedo": negative_albedo_room,
    "sphere_light": scenes.sphere_light,
    "no_lights": scenes.no_lights,
}


def _light_pair_fields(sc):
    """(Q, A, B, D', n) of the light's record in the record loop's pair array, as uint32 [3]
    each (D' one word): the record whose Q is the light's."""
    pairs, n_slots, _, _, _ = sc.export_records()
    f = pairs[:4 * n_slots].reshape(-1, 32)  # one pair per row (rt_device.h pair layout)
    want = _f32(*LIGHT_Q)
    for row in f:
        for h in (0, 1):
            if np.array_equal(row[8 + h:14:2], want) and row[28 + h] != 0:
                return (row[8 + h:14:2], row[14 + h:20:2], row[20 + h:26:2], row[6 + h], row[h:6:2])
    raise AssertionError("the light's record is not in the pair array")


@pytest.mark.parametrize("name", sorted(LISTED))
def test_one_y_quad_light_is_kind_1_and_its_block_copies_the_light(rt, name):
    t, _, w, l = LISTED[name](rt)
    with rt.Scene(t, w, l) as sc:
        kind, blk = sc.lean_light()
        Q, A, B, Dp, n = _light_pair_fields(sc)
    assert kind == 1
    assert blk.dtype == np.uint32 and blk.size == 20
    assert np.array_equal(blk[0:3], _f32(*LIGHT_Q))
    assert np.array_equal(blk[12:15], _f32(*LIGHT_U))
    assert np.array_equal(blk[16:19], _f32(*LIGHT_V))
    assert blk[7] == _f32(LIGHT_AREA)[0]
    assert blk[3] == _f32(LIGHT_Q[1])[0]  # D / n_y = Q.y for a quad in the plane y = Q.y
    assert not blk[[11, 15, 19]].any()
    # the pdf's fields: the light's record as the record loop tests it on the y axis
    assert n.view(np.float32).tolist() == [0.0, -1.0, 0.0]  # u x v = (0, -13650, 0); zeros of either sign
    assert blk[3] == Dp
    assert np.array_equal(blk[0:3], Q)
    assert np.array_equal(blk[4:7], A)  # the in-plane fields (x, z) and the exact zero on y
    assert np.array_equal(blk[8:11], B)
    assert A[1] == 0 and B[1] == 0  # exact zeros (+0 bits): n = +-e_y, so t takes the axis form


@pytest.mark.parametrize("name", sorted(GENERAL))
def test_any_other_light_list_is_kind_0(rt, name):
    t, _, w, l = GENERAL[name](rt)
    with rt.Scene(t, w, l) as sc:
        kind, blk = sc.lean_light()
    assert kind == 0
    assert blk.size == 20 and not blk.any()


def test_size_query(rt):
    import ctypes as C
    t, _, w, l = rt.demo_scene("cornell")
    with rt.Scene(t, w, l) as sc:
        k, n = C.c_int32(-1), C.c_int32(-1)
        assert rt.lib().rt_scene_lean_light(sc._p, C.byref(k), None, C.byref(n)) == 0
        assert (k.value, n.value) == (1, 20)
        assert rt.lib().rt_scene_lean_light(sc._p, None, None, None) == 0
    assert rt.lib().rt_scene_lean_light(None, None, None, None) < 0
