"""The early-draw record-loop kernel (k_fused<true, 0, 0, SHAPE, LIGHT, false, EARLY>: the
vertex's Philox draw issued before the winner is resolved, rt_path.h shade_core) renders the
image of the kernel that draws after, bit for bit, the plan says which of them a launch takes
(rt_scene_plan_early), and a scene without an emitter slot keeps the old kernel.  Shape 1 has
the early-draw kernel; shape 2 keeps the late draw and must render the same
with the knob at either value."""
import numpy as np
import pytest

from tests import scenes
from tests.test_lean_early import REFUSED


def _both(rt, tune, t, cam, w, l, **kw):
    """RT_LEAN_EARLY_DRAW=0 and 1 in one process -> [(image, stats, plan)] in that order"""
    out = []
    for flag in ("0", "1"):
        tune("RT_LEAN_EARLY_DRAW", flag)
        with rt.Scene(t, w, l) as sc:
            plan = (sc.plan_light(), sc.plan_early())
            img, st = sc.render(cam, **kw)
        assert img.dtype == np.float32
        out.append((img, st, plan))
    (a, sa, _), (b, sb, _) = out
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sa["segments"] == sb["segments"] and sa["samples"] == sb["samples"]
    return out


def _pulled_back(rt, boxes=0):
    """the room seen from far outside its open side and off its axis: camera rays pass the
    room, and bounces leave it through the front"""
    t, cam, w, l = scenes.cornell_room(rt, boxes, 1)
    cam.PositionCamera((900, 278, -2400), (278, 278, 0), (0, 1, 0))
    cam.Background = (0.25, 0.5, 0.75)
    return t, cam, w, l


SCENES = {
    "cornell": lambda rt: rt.demo_scene("cornell"),           # shape 1
    "no_boxes": lambda rt: scenes.cornell_room(rt, 0, 1),     # shape 2
    "pulled_back": _pulled_back,                              # shape 2
    "pulled_back_boxes": lambda rt: _pulled_back(rt, 2),      # shape 1: the early kernel's misses
}
EARLY = {"cornell": 1, "no_boxes": 0, "pulled_back": 0, "pulled_back_boxes": 1}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_early_draw_kernel_matches_the_late_draw(rt, gpu, tune, name):
    t, cam, w, l = SCENES[name](rt)
    cam.Width, cam.SamplesPerPixel = 48, 16
    (a, sa, pa), (b, sb, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert (pa, pb) == ((1, 0), (1, EARLY[name]))
    assert np.isfinite(a).all()
    for st in (sa, sb):
        assert st["tree_width"] == 0 and st["kernel_features"] == 0
    if name.startswith("pulled_back"):  # some camera rays miss everything: background pixels
        bg = np.array(cam.Background, np.float32)
        assert (a.reshape(-1, 3) == bg).all(axis=1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
def test_early_draw_at_the_depth_limit(rt, gpu, tune, depth):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel, cam.MaxDepth = 48, 16, depth
    (a, _, _), (_, _, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert pb == (1, 1)
    assert np.isfinite(a).all() and a.any()


@pytest.mark.gpu
def test_early_draw_with_progress_slices(rt, gpu, tune):
    """1,024 launches: drain splits and F_SPLIT takers in most of them"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel, cam.MaxDepth = 40, 9, 6
    (_, sa, _), (_, sb, pb) = _both(rt, tune, t, cam, w, l, seed=5, progress_slices=1024)
    assert pb == (1, 1)
    with rt.Scene(t, w, l) as sc:
        _, st = sc.render(cam, seed=5)
    assert st["segments"] == sa["segments"] == sb["segments"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["second_emitter_outside_the_list", "box_face_emitter"])
def test_scene_without_emitter_slot_keeps_the_late_draw(rt, gpu, tune, name):
    t, cam, w, l = REFUSED[name](rt)
    cam.Width, cam.SamplesPerPixel = 48, 16
    (a, _, pa), (_, _, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert (pa, pb) == ((1, 0), (1, 0))  # the lean light kernel, never its early-draw variant
    assert np.isfinite(a).all()


@pytest.mark.gpu
def test_debug_trace_is_the_late_draws(rt, gpu, tune):
    """The early kernel records its trace in shade_core and recomputes alpha and beta there
    (brute_slot_uv): every word of every vertex's record (o, time, d, vertex, t, u, v, ref)
    equals the late-draw kernel's, for pixels on the walls, the light and both boxes."""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 16
    pixels = [r * 48 + c for r, c in ((2, 24), (12, 30), (24, 10), (24, 24), (30, 16), (34, 30),
                                      (40, 12), (45, 24))]
    traces = []
    for flag in ("0", "1"):
        tune("RT_LEAN_EARLY_DRAW", flag)
        with rt.Scene(t, w, l) as sc:
            assert sc.plan_early() == int(flag)
            traces.append([sc.render(cam, seed=5, trace=(pix, 0), mode="fused")[1]["trace"]
                           for pix in pixels])
    refs = set()
    for a, b in zip(*traces):
        assert a.dtype == np.float32 and a.shape == b.shape and a.shape[0] >= 1
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        hits = a[a.view(np.uint32)[:, 11] != 0xFFFFFFFF]
        refs.update(hits.view(np.uint32)[:, 11].tolist())
        # alpha and beta of a hit lie in the quad (a box face's by the slab test: to fp32 rounding)
        assert ((hits[:, 9:11] >= -1e-3) & (hits[:, 9:11] <= 1 + 1e-3)).all()
    print("traced refs", sorted(refs), "vertices", [len(a) for a in traces[0]])
    assert len(refs) >= 4  # the traced vertices cover several records, box faces among them
    assert max(len(a) for a in traces[0]) >= 3  # and bounces, not only camera rays


@pytest.mark.gpu
def test_negative_background_renders_the_same_at_either_knob(rt, gpu, tune):
    """(the launch takes the general kernel, kind 0, whatever the plan says: test_lean_light_gpu)"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 16
    cam.Background = (-0.1, 0, 0)
    _both(rt, tune, t, cam, w, l, seed=5)
