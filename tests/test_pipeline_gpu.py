"""rt.Pipeline (rt_pipeline) against the Python sequence it restates: rt.Temporal with the same flags,
then acc.resolve_aov_device() and the Python filter call.  Both sides run the same kernels on the
same inputs in the same order, so every comparison is bit for bit (the int32 views, so a NaN compares
by its bits) and any difference is a bookkeeping error of the object: there is no tolerance here.

37 x 23 is neither a multiple of the reprojection's 64 x 4 tile nor of the 8 x 8 adaptive tile, and the
window and the a-trous halos reach the border from most of its pixels.  Three frames of a 1-degree
orbit, 4 spp per pass: one pass per frame with moments (their point), two without (the accumulator's
variance needs two).  1 x 1 and 131 x 5 are tests/test_reproject_gpu.py's degenerate tiles."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_temporal_gpu import orbit

pytestmark = pytest.mark.gpu
SIZE = (37, 23)
FRAMES = 3
EMIT = dict(split_emitters=True)
CONFIGS = {
    # name: (scene, accumulator features, passes per frame, Temporal's flags)
    "plain": ("cornell", "guides", 2, {}),
    "emit": ("cornell", "emit", 2, EMIT),
    "light": ("cornell", "emit", 2, dict(EMIT, light_history=True)),
    "emit+moments": ("cornell", "emit", 1, dict(EMIT, moments=True)),
    "light+moments+clip": ("cornell", "emit", 1, dict(EMIT, light_history=True, moments=True, clip=True)),
    # tests/test_temporal_spec_gpu.py's: the quads scene's own camera, Temporal(split_emitters, moments, specular)
    "emit+moments+specular": ("quads", "emit+spec", 1, dict(EMIT, moments=True, specular=True)),
}
PLANES = ("rgb", "var", "count", "lum2", "emission", "coverage")


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def camera(rt, scene, size):
    t, cam, w, l = rt.demo_scene(scene)
    cam.Width, cam.SamplesPerPixel, cam.AspectRatio = size[0], 4, size[0] / size[1]
    d = cam.derived()
    assert (d.width, d.height) == size
    return t, cam, w, l


def accumulate(sc, cam, features, passes, k):
    """frame k's accumulator: pass p takes seed 1 + k + 100 p"""
    acc = sc.accumulator(cam, max_passes=passes, features=features)
    for p in range(passes):
        acc.add(1 + k + 100 * p)
    return acc


def python_frame(rt, temporal, acc, split, filt="var"):
    """the yardstick: Temporal.push, the guides, the filter, the text -> device tensors and bytes"""
    rgb, var, count = temporal.push(acc)
    aov = acc.resolve_aov_device()
    out = {"rgb": rgb, "var": var, "count": count}
    if temporal.light:
        aov = dict(aov, **temporal.light)
        out.update(temporal.light)
    if temporal._moments:
        out["lum2"] = temporal._sets[temporal._prev]["lum2"]
    out["image"] = rt.denoise_var_device(rgb, var, aov, split_emitters=split) if filt == "var" else rgb
    out["ppm"] = rt.format_ppm_device(out["image"])
    return out


def check_frame(tag, pipe, want):
    """every plane the object lends, its image and its text against the yardstick's; -> the object's
    frame as host arrays"""
    got = pipe.planes_device()
    for k in PLANES:
        if k in want:
            assert same(got[k], want[k]), f"{tag}: {k}"
    assert ("lum2" in got) == ("lum2" in want), tag
    assert same(got["image"], want["image"]), f"{tag}: image (device)"
    img = pipe.image()
    assert np.array_equal(img.view(np.int32), want["image"].cpu().numpy().view(np.int32)), f"{tag}: image"
    ppm = pipe.ppm()
    assert ppm == want["ppm"], f"{tag}: ppm"
    host = {k: v.cpu().numpy().copy() for k, v in got.items()}
    host["ppm"] = ppm
    return host


_RUNS = {}


def run(rt, name, size=SIZE):
    """configuration `name` at `size`, Python and the object side by side on the same accumulators,
    every frame compared; computed once -> (the object's frames as host arrays, its info after each
    push)"""
    if (name, size) in _RUNS:
        return _RUNS[name, size]
    scene, features, passes, kw = CONFIGS[name]
    split = bool(kw.get("split_emitters"))
    t, cam, w, l = camera(rt, scene, size)
    temporal = rt.Temporal(**kw)
    frames, infos = [], []
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe:
        assert pipe.opts.split_emitters == int(split) and pipe.opts.vopts.demodulate == 1
        for k in range(FRAMES):
            with accumulate(sc, orbit(cam, 1.0 * k), features, passes, k) as acc:
                want = python_frame(rt, temporal, acc, split)
                assert pipe.push(acc) is pipe
                frames.append(check_frame(f"{name} {size}, frame {k}", pipe, want))
                infos.append(pipe.info())
    _RUNS[name, size] = frames, infos
    return frames, infos


def equal_frames(a, b):
    return a.keys() == b.keys() and all(
        (a[k] == b[k]) if k == "ppm" else np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_frame_has_the_python_sequences_bits(rt, gpu, name):
    frames, infos = run(rt, name)
    assert [i["had_history"] for i in infos] == [0, 1, 1] and [i["frames"] for i in infos] == [1, 2, 3]
    assert all((i["width"], i["height"], i["device"]) == SIZE + (0,) for i in infos)
    # the history did something: the blended frame is not the filter's input of a fresh object
    assert frames[2]["count"].max() > frames[0]["count"].max()
    # allocation happens while the two sets warm up, and never again
    assert infos[0]["allocations"] > 0 and infos[1]["allocations"] > infos[0]["allocations"]
    assert infos[1]["device_bytes"] > infos[0]["device_bytes"] > 0
    assert (infos[2]["allocations"], infos[2]["device_bytes"]) == (infos[1]["allocations"], infos[1]["device_bytes"])
    if "light" in name:
        assert "emission" in frames[0] and "coverage" in frames[0]
    assert ("lum2" in frames[0]) == ("moments" in name)


@pytest.mark.parametrize("name,size", [("plain", (1, 1)), ("emit+moments", (131, 5))])
def test_degenerate_tiles(rt, gpu, name, size):
    frames, infos = run(rt, name, size)
    assert frames[0]["image"].shape == (size[1], size[0], 3) and infos[-1]["had_history"] == 1


def test_no_history_with_the_plain_filter(rt, gpu):
    """temporal = 0: resolve -> rt_denoise_device, count the pass count"""
    t, cam, w, l = camera(rt, "cornell", SIZE)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(temporal=False, filter="plain") as pipe:
        for k in range(2):
            with accumulate(sc, orbit(cam, 1.0 * k), "guides", 2, k) as acc:
                rgb = torch.empty(acc.shape + (3,), device="cuda")
                var = torch.empty(acc.shape, device="cuda")
                acc.resolve_device(rgb, var)
                want = {"rgb": rgb, "var": var, "count": torch.full_like(var, 2.0),
                        "image": rt.denoise_device(rgb, acc.resolve_aov_device())}
                want["ppm"] = rt.format_ppm_device(want["image"])
                check_frame(f"no history, frame {k}", pipe.push(acc), want)
                assert pipe.info()["had_history"] == 0 and pipe.info()["frames"] == k + 1
        assert not same(want["image"], rgb)  # the filter ran


def test_unfiltered_and_differently_split_pipelines(rt, gpu):
    """filter=None: the blended frame is the image; filter_split=False under an emit history: the
    unsplit filter over the accumulator's albedo"""
    t, cam, w, l = camera(rt, "cornell", SIZE)
    ta, tb = rt.Temporal(**EMIT), rt.Temporal(**EMIT)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(filter=None, **EMIT) as a, rt.Pipeline(filter_split=False, **EMIT) as b:
        for k in range(2):
            with accumulate(sc, orbit(cam, 1.0 * k), "emit", 2, k) as acc:
                check_frame(f"unfiltered, frame {k}", a.push(acc), python_frame(rt, ta, acc, True, filt=None))
                check_frame(f"unsplit filter, frame {k}", b.push(acc), python_frame(rt, tb, acc, False))


def test_reset_and_another_size_start_over(rt, gpu):
    name = "emit+moments"
    scene, features, passes, kw = CONFIGS[name]
    frames, _ = run(rt, name)
    small = (24, 17)
    t, cam, w, l = camera(rt, scene, SIZE)
    _, cam_small, _, _ = camera(rt, scene, small)
    fresh = rt.Temporal(**kw)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe:
        for k in range(FRAMES):
            with accumulate(sc, orbit(cam, 1.0 * k), features, passes, k) as acc:
                pipe.push(acc)
        before = pipe.info()
        pipe.reset()
        assert pipe.info()["frames"] == 0
        with accumulate(sc, cam, features, passes, 0) as acc:  # frame 0 again
            got = check_frame("after reset", pipe.push(acc), python_frame(rt, rt.Temporal(**kw), acc, True))
        assert equal_frames(got, frames[0])
        after = pipe.info()
        assert (after["had_history"], after["frames"]) == (0, 1)
        assert (after["allocations"], after["device_bytes"]) == (before["allocations"], before["device_bytes"])
        with accumulate(sc, cam_small, features, passes, 0) as acc:
            check_frame("another size", pipe.push(acc), python_frame(rt, fresh, acc, True))
        i = pipe.info()
        assert (i["width"], i["height"], i["had_history"], i["frames"]) == small + (0, 1)
        assert i["allocations"] > after["allocations"] and i["device_bytes"] < after["device_bytes"]
        with accumulate(sc, orbit(cam_small, 1.0), features, passes, 1) as acc:  # and goes on from there
            check_frame("another size, frame 1", pipe.push(acc), python_frame(rt, fresh, acc, True))
        assert pipe.info()["had_history"] == 1


def test_push_refusals_leave_the_last_frame(rt, gpu):
    E = rt._lib.RT_ERR_INVALID
    t, cam, w, l = camera(rt, "cornell", SIZE)
    kw = dict(EMIT, moments=True)

    def refused(pipe, acc, word):
        with pytest.raises(rt.RtError, match=word) as e:
            pipe.push(acc)
        assert e.value.code == E and b"rt_pipeline_push" in rt.lib().rt_last_error()

    with rt.Scene(t, w, l) as sc, rt.Pipeline(**kw) as pipe, rt.Pipeline(specular=True, **kw) as spec, \
            rt.Pipeline(filter_split=True) as plain_split:
        with accumulate(sc, cam, "emit", 1, 0) as acc:
            pipe.push(acc)
        image, ppm, info = pipe.image(), pipe.ppm(), pipe.info()
        with sc.accumulator(cam, max_passes=2, features="emit") as empty:
            refused(pipe, empty, "no pass")
        with accumulate(sc, cam, None, 1, 0) as bare:
            refused(pipe, bare, "features")
        with accumulate(sc, cam, "guides", 1, 0) as guides:
            refused(pipe, guides, "RT_ACCUM_FEAT_EMIT")          # mode != PLAIN
            refused(plain_split, guides, "RT_ACCUM_FEAT_EMIT")   # split_emitters
        with accumulate(sc, cam, "emit", 1, 0) as acc:
            refused(spec, acc, "RT_ACCUM_FEAT_SPEC")
        with sc.accumulator(cam, max_passes=1, features="emit", rank=0, nranks=2) as share:
            share.add(1)
            refused(pipe, share, "whole image")
        assert pipe.info() == info
        assert np.array_equal(pipe.image().view(np.int32), image.view(np.int32)) and pipe.ppm() == ppm
        for p in (spec, plain_split):  # nothing was pushed, nothing was allocated
            assert p.info()["allocations"] == 0 and p.info()["frames"] == 0
            with pytest.raises(rt.RtError):
                p.image()
        # the history is as it was: the next frame blends with frame 0, as the undisturbed run's did
        with accumulate(sc, orbit(cam, 1.0), "emit", 1, 1) as acc:
            pipe.push(acc)
        got = pipe.planes_device()
        frames, _ = run(rt, "emit+moments")
        assert all(np.array_equal(got[k].cpu().numpy().view(np.int32), frames[1][k].view(np.int32))
                   for k in ("rgb", "var", "count", "lum2", "image"))
        # a cap too small for the text is rt_format_ppm's refusal; the size query is not
        n = int(rt.lib().rt_pipeline_ppm(pipe._p, None, 0))
        assert n == len(pipe.ppm())
        import ctypes as C
        buf = C.create_string_buffer(n)
        assert rt.lib().rt_pipeline_ppm(pipe._p, buf, n - 1) == E and b"too small" in rt.lib().rt_last_error()
        assert rt.lib().rt_pipeline_ppm(pipe._p, buf, n) == n and buf.raw == pipe.ppm()


def test_two_pipelines_fed_alternately(rt, gpu):
    """what one holds is its own: "emit" and "light" over the same accumulators, in turn, give what
    each gives alone"""
    alone = {n: run(rt, n)[0] for n in ("emit", "light")}
    t, cam, w, l = camera(rt, "cornell", SIZE)
    with rt.Scene(t, w, l) as sc, rt.Pipeline(**CONFIGS["emit"][3]) as a, rt.Pipeline(**CONFIGS["light"][3]) as b:
        for k in range(FRAMES):
            with accumulate(sc, orbit(cam, 1.0 * k), "emit", 2, k) as acc:
                for name, pipe in (("emit", a), ("light", b)) if k % 2 == 0 else (("light", b), ("emit", a)):
                    pipe.push(acc)
                    got = {key: v.cpu().numpy() for key, v in pipe.planes_device().items()}
                    got["ppm"] = pipe.ppm()
                    assert equal_frames(got, alone[name][k]), (name, k)


def test_the_scene_may_go_first(rt, gpu):
    t, cam, w, l = camera(rt, "cornell", SIZE)
    pipe = rt.Pipeline(**EMIT)
    sc = rt.Scene(t, w, l)
    acc = accumulate(sc, cam, "emit", 2, 0)
    pipe.push(acc)
    ppm = pipe.ppm()
    sc.close()  # frees the accumulator with it
    assert pipe.ppm() == ppm and pipe.image().shape == (SIZE[1], SIZE[0], 3) and pipe.info()["frames"] == 1
    pipe.reset()
    pipe.close()
