"""The record loop's pair layout, packed on the host (csrc/host_records.cpp pack_records,
exported by rt_scene_export_records): bit-equal to the arrays the renderer uploaded before
the packing moved out of the upload (tests/golden/record_packing.npz: per case `meta` =
n_slots, the seven layout counts in rt_brute_shape's order, shade_n, n_boxes, and `pairs` =
the uploaded float4 array as uint32 words, the shade table appended)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import scenes

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_packing.npz"))
KNOBS = ("RT_BRUTE_AXIS", "RT_BRUTE_VERT", "RT_BRUTE_BOX", "RT_BRUTE_MIXED", "RT_SHADE_LDS")
CASES = ["cornell", "quads", "no_boxes", "one_box", "two_lights", "tilted_room"] + [
    f"cornell.{k}=0" for k in KNOBS]
# the listed layouts (rt_device.h brute_shape): 1 Cornell with boxes, 2 without
SHAPES = {"cornell": 1, "one_box": 1, "no_boxes": 2}


def _export(rt, tune, case, fill=True):
    name, _, knob = case.partition(".")
    if knob:
        tune(knob.split("=")[0], "0")
    t, _, w, l = scenes.record_scene(rt, name)
    with rt.Scene(t, w, l) as sc:
        return sc.export_records(fill=fill)


def test_golden_covers_the_cases():
    assert sorted(GOLDEN.files) == sorted(f"{c}.{k}" for c in CASES for k in ("meta", "pairs"))


@pytest.mark.parametrize("case", CASES)
def test_packing_is_the_uploaded_bytes(rt, tune, case):
    pairs, n_slots, counts, shade_n, n_boxes = _export(rt, tune, case)
    meta = GOLDEN[case + ".meta"].tolist()
    assert (n_slots, *counts, shade_n, n_boxes) == tuple(meta)
    want = GOLDEN[case + ".pairs"]
    assert pairs.dtype == np.uint32 and pairs.size == want.size == 16 * n_slots + 4 * shade_n
    assert np.array_equal(pairs.ravel(), want)


@pytest.mark.parametrize("case", CASES[:6])
def test_exported_counts_name_the_listed_shape(rt, tune, case):
    _, _, counts, _, _ = _export(rt, tune, case)
    assert rt.lib().rt_brute_shape((C.c_int32 * 7)(*counts)) == SHAPES.get(case, 0)


@pytest.mark.parametrize("case", ["cornell", "quads", "tilted_room"])
def test_size_query_matches_filled_form(rt, tune, case):
    q = _export(rt, tune, case, fill=False)
    f = _export(rt, tune, case)
    assert q[1:] == f[1:] and q[0].shape == f[0].shape
    assert not q[0].any() and f[0].any()


def test_scene_above_the_upload_threshold_has_no_pairs(rt, tune):
    """book1 has more leaf entries than tiny scenes may (RT_BRUTE_MAX, at least 64)."""
    t, _, w, l = rt.demo_scene("book1")
    with rt.Scene(t, w, l) as sc:
        assert len(sc.export_bvh()[1]) > 64
        pairs, n_slots, counts, shade_n, n_boxes = sc.export_records()
    assert n_slots == 0 and pairs.size == 0
    assert counts == (0,) * 7 and shade_n == 0 and n_boxes == 0
