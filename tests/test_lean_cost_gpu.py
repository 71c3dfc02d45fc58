"""The early-draw kernel's lean-cost twin (k_fused<true, 0, 0, 1, 1, false, true, COST>: the
round without the tree scheduler's state, rt_fused.h) renders the early-draw kernel's image, segments and samples bit for bit:
RT_LEAN_COST at 0 and 1 in one process, Cornell (shape 1) at 48 x 48 x 16 and the cases that
take other paths of the kernel or leave it."""
import numpy as np
import pytest

from tests import scenes
from tests.test_lean_early import REFUSED


def _both(rt, tune, t, cam, w, l, **kw):
    """RT_LEAN_COST=0 and 1 in one process -> [(image, stats, plan_cost)] in that order"""
    out = []
    for flag in ("0", "1"):
        tune("RT_LEAN_COST", flag)
        with rt.Scene(t, w, l) as sc:
            plan = (sc.plan_early(), sc.plan_cost())
            img, st = sc.render(cam, **kw)
        assert img.dtype == np.float32
        out.append((img, st, plan))
    (a, sa, _), (b, sb, _) = out
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sa["segments"] == sb["segments"] and sa["samples"] == sb["samples"]
    return out


def _pulled_back_boxes(rt):
    """the room (shape 1) seen from far outside its open side: camera rays that miss everything"""
    t, cam, w, l = scenes.cornell_room(rt, 2, 1)
    cam.PositionCamera((900, 278, -2400), (278, 278, 0), (0, 1, 0))
    cam.Background = (0.25, 0.5, 0.75)
    return t, cam, w, l


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "pulled_back_boxes"])
def test_lean_cost_kernel_matches_the_early_draw_kernel(rt, gpu, tune, name):
    t, cam, w, l = rt.demo_scene("cornell") if name == "cornell" else _pulled_back_boxes(rt)
    cam.Width, cam.SamplesPerPixel = 48, 16
    (a, sa, pa), (b, sb, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert (pa, pb) == ((1, 0), (1, 1))
    assert np.isfinite(a).all() and a.any()
    for st in (sa, sb):
        assert st["tree_width"] == 0 and st["kernel_features"] == 0
    if name == "pulled_back_boxes":  # background pixels: the kernel's misses
        bg = np.array(cam.Background, np.float32)
        assert (a.reshape(-1, 3) == bg).all(axis=1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
def test_lean_cost_at_the_depth_limit(rt, gpu, tune, depth):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel, cam.MaxDepth = 48, 16, depth
    (a, _, _), (_, _, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert pb == (1, 1)
    assert np.isfinite(a).all() and a.any()


@pytest.mark.gpu
def test_lean_cost_with_progress_slices(rt, gpu, tune):
    """1,024 launches: drain splits and F_SPLIT takers in most of them"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel, cam.MaxDepth = 40, 9, 6
    (_, sa, _), (_, sb, pb) = _both(rt, tune, t, cam, w, l, seed=5, progress_slices=1024)
    assert pb == (1, 1)
    with rt.Scene(t, w, l) as sc:
        _, st = sc.render(cam, seed=5)
    assert st["segments"] == sa["segments"] == sb["segments"]


@pytest.mark.gpu
def test_negative_background_renders_the_same_at_either_knob(rt, gpu, tune):
    """(the launch takes the general light code, kind 0, whatever the plan says)"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 16
    cam.Background = (-0.1, 0, 0)
    _both(rt, tune, t, cam, w, l, seed=5)


@pytest.mark.gpu
def test_scene_the_matcher_refuses_keeps_its_kernel(rt, gpu, tune):
    t, cam, w, l = REFUSED["box_face_emitter"](rt)
    cam.Width, cam.SamplesPerPixel = 48, 16
    (a, _, pa), (_, _, pb) = _both(rt, tune, t, cam, w, l, seed=5)
    assert (pa, pb) == ((0, 0), (0, 0))  # no early-draw kernel, so no lean-cost twin
    assert np.isfinite(a).all()


@pytest.mark.gpu
def test_debug_trace_matches_word_for_word(rt, gpu, tune):
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 48, 16
    pixels = [r * 48 + c for r, c in ((2, 24), (12, 30), (24, 10), (24, 24), (30, 16), (34, 30),
                                      (40, 12), (45, 24))]
    traces = []
    for flag in ("0", "1"):
        tune("RT_LEAN_COST", flag)
        with rt.Scene(t, w, l) as sc:
            assert sc.plan_cost() == int(flag)
            traces.append([sc.render(cam, seed=5, trace=(pix, 0), mode="fused")[1]["trace"]
                           for pix in pixels])
    for a, b in zip(*traces):
        assert a.dtype == np.float32 and a.shape == b.shape and a.shape[0] >= 1
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert max(len(a) for a in traces[0]) >= 3  # bounces, not only camera rays
