"""The record-loop kernel compiled for a lean light kind (k_fused<true, 0, 0, SHAPE, LIGHT>,
rt_device.h "lean light kinds") renders the image of the general light code bit for bit, the
plan says which of them a launch takes (rt_scene_plan_light), and every scene outside the
kind, a render with a negative background and a layout without such a kernel fall back."""
import numpy as np
import pytest

from tests import scenes
from tests.test_lean_light import tilted_light_room, x_wall_room

SCENES = {
    "cornell": lambda rt: rt.demo_scene("cornell"),
    "no_boxes": lambda rt: scenes.record_scene(rt, "no_boxes"),
    "one_box": lambda rt: scenes.record_scene(rt, "one_box"),
    "two_lights": lambda rt: scenes.record_scene(rt, "two_lights"),
    "tilted_room": lambda rt: scenes.record_scene(rt, "tilted_room"),
    "x_wall": x_wall_room,
    "tilted_light": tilted_light_room,
}


def _both(rt, tune, t, cam, w, l, fixed=(), **kw):
    """RT_LEAN_LIGHT=0 and 1 in one process -> [(image, stats, plan)] in that order"""
    out = []
    for flag in ("0", "1"):
        for k, v in fixed:
            tune(k, v)
        tune("RT_LEAN_LIGHT", flag)
        with rt.Scene(t, w, l) as sc:
            plan = sc.plan_light()
            img, st = sc.render(cam, **kw)
        assert img.dtype == np.float32
        out.append((img, st, plan))
    (a, sa, _), (b, sb, _) = out
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sa["segments"] == sb["segments"] and sa["samples"] == sb["samples"]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "no_boxes", "one_box"])
def test_lean_light_kernel_matches_general_light_code(rt, gpu, tune, name):
    t, cam, w, l = SCENES[name](rt)
    cam.Width, cam.SamplesPerPixel = 48, 16
    (a, sa, pa), (b, sb, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert (pa, pb) == (0, 1)
    assert np.isfinite(a).all()
    for st in (sa, sb):
        assert st["tree_width"] == 0 and st["kernel_features"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two_lights", "tilted_room", "x_wall", "tilted_light"])
def test_scenes_outside_the_kind_take_the_general_code(rt, gpu, tune, name):
    t, cam, w, l = SCENES[name](rt)
    cam.Width, cam.SamplesPerPixel = 48, 16
    (a, _, pa), (_, _, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert (pa, pb) == (0, 0)
    assert np.isfinite(a).all()


@pytest.mark.gpu
def test_negative_background_clears_merge_ok_per_render(rt, gpu, tune):
    """The background is part of the camera, so the plan (1) cannot know it: the launch
    itself takes the general light code, which reads merge_ok."""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 16
    cam.Background = (-0.1, 0, 0)
    (a, _, _), (b, _, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert pb == 1
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isfinite(a), np.isfinite(b))


@pytest.mark.gpu
def test_lean_light_kernel_with_progress_slices(rt, gpu, tune):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel, cam.MaxDepth = 40, 9, 6
    (_, sa, _), (_, sb, pb) = _both(rt, tune, t, cam, w, l, seed=5, progress_slices=1024)
    assert pb == 1
    with rt.Scene(t, w, l) as sc:
        _, st = sc.render(cam, seed=5)
    assert st["segments"] == sa["segments"] == sb["segments"]


@pytest.mark.gpu
def test_generic_record_loop_has_no_lean_light_kernel(rt, gpu, tune):
    """RT_BRUTE_SHAPE=0 takes the generic record loop, which is not compiled for a light
    kind: the plan says 0 and the image is the one of both knobs at 0."""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 16
    (a, _, pa), (b, _, pb) = _both(rt, tune, t, cam, w, l, fixed=(("RT_BRUTE_SHAPE", "0"),), seed=5)
    assert (pa, pb) == (0, 0)
    assert np.isfinite(a).all()
