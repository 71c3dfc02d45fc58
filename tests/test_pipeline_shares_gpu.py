"""rt_pipeline_push_shares against rt_pipeline_push: the same frames accumulated as n
row shares and as one whole accumulator, pushed into two pipelines of the same configuration.  The
shares resolve to rows i::n of the whole accumulator bit for bit (tests/test_accum_shares_gpu.py) and
the gather only moves them, so every comparison is bit for bit (int32 views): there is no tolerance.

Sizes and share counts: 1 x 1 with n = 1; 3 x 2 with n = 2 (one row per share); 24 x 17 with n = 3 (a
short last share, 6 + 6 + 5 rows); 131 x 5 with n = 5 (one row per share, a width that is no multiple
of 4 or 64, and 393 floats a row: more than one 256-lane block).  All shares run on device 0; one
case runs shares on two devices where there are two.  Three frames of a 1-degree orbit, one pass of
4 spp per frame."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_temporal_gpu import orbit

pytestmark = pytest.mark.gpu
FRAMES = 3
EMIT = dict(split_emitters=True)
CONFIGS = {
    # name: (scene, accumulator features, Pipeline's arguments)
    "plain": ("cornell", "guides", dict(temporal=False, filter="plain")),
    "emit+moments+var+split": ("cornell", "emit", dict(EMIT, moments=True, filter="var")),
    "light+moments+clip": ("cornell", "emit", dict(EMIT, light_history=True, moments=True, clip=True)),
    "specular": ("quads", "emit+spec", dict(EMIT, moments=True, specular=True)),
    "unfiltered": ("cornell", "emit", dict(EMIT, filter=None)),
}
SHAPES = [((1, 1), 1), ((3, 2), 2), ((24, 17), 3), ((131, 5), 5)]


def camera(rt, scene, size):
    t, cam, w, l = rt.demo_scene(scene)
    cam.Width, cam.SamplesPerPixel, cam.AspectRatio = size[0], 4, size[0] / size[1]
    d = cam.derived()
    assert (d.width, d.height) == size
    return t, cam, w, l


def snapshot(pipe):
    """everything a pipeline shows of its last push, on the host"""
    out = {k: v.cpu().numpy().copy() for k, v in pipe.planes_device().items()}
    out["image()"] = pipe.image()
    out["ppm"] = pipe.ppm()
    i = pipe.info()
    out["info"] = (i["width"], i["height"], i["device"], i["frames"], i["had_history"])
    return out


def assert_same(tag, got, want):
    assert got.keys() == want.keys(), tag
    for k in want:
        if k in ("ppm", "info"):
            assert got[k] == want[k], f"{tag}: {k}"
        else:
            assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), \
                f"{tag}: {k}"


def whole_frame(sc, cam, features, k):
    acc = sc.accumulator(cam, max_passes=1, features=features)
    acc.add(1 + k)
    return acc


def share_frame(sc, cam, features, k, devices):
    sh = sc.accumulator_shares(cam, devices, max_passes=1, features=features)
    sh.add(1 + k)
    return sh


_WHOLE = {}


def whole_run(rt, name, size):
    """the yardstick: FRAMES whole accumulators through rt_pipeline_push, computed once"""
    if (name, size) not in _WHOLE:
        scene, features, kw = CONFIGS[name]
        t, cam, w, l = camera(rt, scene, size)
        frames = []
        with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe:
            for k in range(FRAMES):
                with whole_frame(sc, orbit(cam, 1.0 * k), features, k) as acc:
                    frames.append(snapshot(pipe.push(acc)))
        _WHOLE[name, size] = frames
    return _WHOLE[name, size]


@pytest.mark.parametrize("size,n", SHAPES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_shares_push_has_the_whole_pushs_bits(rt, gpu, name, size, n):
    scene, features, kw = CONFIGS[name]
    want = whole_run(rt, name, size)
    t, cam, w, l = camera(rt, scene, size)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe:
        for k in range(FRAMES):
            with share_frame(sc, orbit(cam, 1.0 * k), features, k, [0] * n) as sh:
                assert pipe.push(sh) is pipe
                assert_same(f"{name} {size} n={n}, frame {k}", snapshot(pipe), want[k])
    temporal = kw.get("temporal", True)
    assert [f["info"][3:] for f in want] == [(k + 1, int(temporal and k > 0)) for k in range(FRAMES)]


def test_a_list_of_accumulators_is_a_frame_too(rt, gpu):
    name, size, n = "emit+moments+var+split", (24, 17), 3
    scene, features, kw = CONFIGS[name]
    want = whole_run(rt, name, size)
    t, cam, w, l = camera(rt, scene, size)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe:
        with share_frame(sc, cam, features, 0, [0] * n) as sh:
            assert_same("list", snapshot(pipe.push(list(sh.shares))), want[0])
        with share_frame(sc, orbit(cam, 1.0), features, 1, [0] * n) as sh:
            assert_same("tuple", snapshot(pipe.push(tuple(sh.shares))), want[1])


def test_alternating_entries(rt, gpu):
    """frame 0 through shares, frame 1 through a whole accumulator, frame 2 through shares: three
    whole pushes"""
    name, size, n = "emit+moments+var+split", (24, 17), 3
    scene, features, kw = CONFIGS[name]
    want = whole_run(rt, name, size)
    t, cam, w, l = camera(rt, scene, size)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe:
        for k in range(FRAMES):
            c = orbit(cam, 1.0 * k)
            with (whole_frame(sc, c, features, k) if k == 1 else share_frame(sc, c, features, k, [0] * n)) as f:
                assert_same(f"alternating, frame {k}", snapshot(pipe.push(f)), want[k])


def test_allocations_stop_once_warm(rt, gpu):
    name, size, n = "light+moments+clip", (24, 17), 3
    scene, features, kw = CONFIGS[name]
    t, cam, w, l = camera(rt, scene, size)
    infos = []
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe, rt.Pipeline(**kw) as whole:
        for k in range(4):
            with share_frame(sc, orbit(cam, 1.0 * k), features, k, [0] * n) as sh:
                infos.append(pipe.push(sh).info())
        with whole_frame(sc, cam, features, 0) as acc:
            whole.push(acc)
            first_whole = whole.info()
            after_whole = pipe.push(acc).info()  # the gather buffer stays for the next shares push
        with share_frame(sc, cam, features, 0, [0] * n) as sh:
            again = pipe.push(sh).info()
    assert infos[1]["allocations"] > infos[0]["allocations"] > 0
    assert [(i["allocations"], i["device_bytes"]) for i in infos[2:]] == [(infos[1]["allocations"],
                                                                          infos[1]["device_bytes"])] * 2
    assert (after_whole["allocations"], again["allocations"]) == (infos[1]["allocations"],) * 2
    # the gather buffer is in the figures: one allocation and its bytes more than the whole push's first frame
    assert infos[0]["allocations"] == first_whole["allocations"] + 1
    assert infos[0]["device_bytes"] > first_whole["device_bytes"]


def test_refusals_leave_the_last_frame(rt, gpu):
    E = rt._lib.RT_ERR_INVALID
    L = rt.lib()
    name, size, n = "emit+moments+var+split", (24, 17), 3
    scene, features, kw = CONFIGS[name]
    want = whole_run(rt, name, size)
    t, cam, w, l = camera(rt, scene, size)
    _, tiny, _, _ = camera(rt, scene, (3, 2))

    def shares(sc, cams=None, feats=None, passes=None, spec=None, devices=(0, 0, 0)):
        """three shares of one frame, share i with its own camera, features, pass count and chain limit"""
        out = []
        for i, d in enumerate(devices):
            f = (feats or [features] * 3)[i]
            a = sc.accumulator((cams or [cam] * 3)[i], max_passes=4, device=d, rank=i, nranks=len(devices), features=f,
                               spec_bounces=(spec or [0] * 3)[i] if str(f).endswith("+spec") else 0)
            for p in range((passes or [1] * 3)[i]):
                a.add(1 + p)
            out.append(a)
        return out

    with rt.Scene(t, w, l) as sc, rt.Scene(t, w, l) as other, rt.Pipeline(**kw) as pipe:
        good = shares(sc)
        pipe.push(good)
        before = snapshot(pipe)
        assert_same("frame 0", before, want[0])

        def refused(accs, word):
            with pytest.raises(rt.RtError, match=word) as e:
                pipe.push(accs)
            assert e.value.code == E and b"rt_pipeline_push_shares" in L.rt_last_error(), L.rt_last_error()

        refused([], "n = 0")
        arr = (C.c_void_p * 3)(good[0]._p.value, None, good[2]._p.value)
        assert L.rt_pipeline_push_shares(pipe._p, arr, 3) == E and b"rt_pipeline_push_shares: accs[1] is null" in L.rt_last_error()
        assert L.rt_pipeline_push_shares(pipe._p, None, 3) == E and L.rt_pipeline_push_shares(None, arr, 3) == E
        assert L.rt_pipeline_push_shares(pipe._p, arr, -1) == E and b"rt_pipeline_push_shares" in L.rt_last_error()
        refused([good[0], good[0], good[2]], "same accumulator")
        refused([good[1], good[0], good[2]], "rank")
        refused(good[:2], "rank 0 of 3, not rank 0 of 2")
        # more shares than rows: the third share of a 2-row image is empty
        refused(shares(sc, cams=[tiny] * 3, passes=[0, 0, 0]), "empty share")
        refused(shares(sc, passes=[0, 0, 0]), "no pass")
        refused(shares(sc, feats=["guides"] * 3), "RT_ACCUM_FEAT_EMIT")
        refused(shares(sc, feats=[None] * 3), "features")
        refused([good[0], shares(other)[1], good[2]], "scene")
        refused(shares(sc, cams=[cam, orbit(cam, 1.0), cam]), "camera")
        wide = type(cam).from_c(cam.to_c())
        wide.Width, wide.AspectRatio = 25, 25 / 17
        refused(shares(sc, cams=[cam, wide, cam]), "camera")
        deep = type(cam).from_c(cam.to_c())
        deep.MaxDepth = cam.derived().max_depth + 1
        refused(shares(sc, cams=[cam, cam, deep]), "camera")
        more = type(cam).from_c(cam.to_c())
        more.SamplesPerPixel = 9
        refused(shares(sc, cams=[cam, more, cam]), "camera")
        refused(shares(sc, feats=["emit", "emit+media", "emit"]), "feature planes")
        refused(shares(sc, feats=["emit+spec"] * 3, spec=[2, 4, 2]), "chain limits")
        refused(shares(sc, passes=[1, 2, 1]), "pass count")
        with pytest.raises(rt.RtError, match="whole image"):  # and the single push still refuses a share
            pipe.push(good[0])
        assert_same("after the refusals", snapshot(pipe), before)
        # the history is as it was: the next frame blends with frame 0
        with share_frame(sc, orbit(cam, 1.0), features, 1, [0] * n) as sh:
            assert_same("frame 1", snapshot(pipe.push(sh)), want[1])


def test_two_devices(rt, gpu):
    if rt.device_count() < 2:
        pytest.skip("one HIP device: shares on two devices need two")
    name, size = "emit+moments+var+split", (24, 17)
    scene, features, kw = CONFIGS[name]
    t, cam, w, l = camera(rt, scene, size)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as a, rt.Pipeline(**kw) as b:
        for k in range(FRAMES):
            c = orbit(cam, 1.0 * k)
            with share_frame(sc, c, features, k, [0, 0]) as one, share_frame(sc, c, features, k, [0, 1]) as two:
                assert_same(f"two devices, frame {k}", snapshot(b.push(two)), snapshot(a.push(one)))
