"""The host path of the eight rt_render_aov entries (rt_aov.hip: the plane table, the staging
slots of a host entry, the copy back) when only some of a mode's planes are asked for.

Each of the four modes on `cornell` (the record loop; no media, so the media entries run the
kernels without the mode and clear the scatter plane) and on `cornell_smoke` (which has media:
the MEDIA kernels run), 33 x 9 pixels, n = 2: 297 pixels are two blocks, the second one partial.

The C host entry writes into one arena of uint32 words, laid out as the mode's planes back to
back in the order of the entries' structs with three planes' worth of guard words behind them,
filled with a sentinel.  Only the wanted planes' addresses are passed; the other pointers are
NULL inside the same structs, so the kernel is the all-planes call's.  Afterwards the wanted
planes hold the bits of the all-planes host call and of the `_device` entry into torch tensors,
and every other word of the arena, unwanted planes and guard, is still the sentinel: a plane
copied back with another plane's size or from another plane's slot shows in one or the other.
Two subsets per mode: the mode's last plane (`coverage`, `scatter`, `bounces`; `material` for the
plain entries) with `depth`, whose staging slots have absent planes before and between them,
and `material` alone.  The media entries also take a NULL emit struct (slots 4 to 6 absent, the
kernels without the split): `scatter` with `depth` that way, against render_aov(media=True)."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_aov_gpu import _shape

pytestmark = pytest.mark.gpu

W, H, N, SEED = 33, 9, 2, 3
SENTINEL = 0xA5A5A5A5
OUT = ("albedo", "normal", "depth", "material")
EMIT = ("emission", "surface_albedo", "coverage")
CHANNELS = {"albedo": 3, "normal": 3, "emission": 3, "surface_albedo": 3}  # else 1
# mode: (Scene.render_aov's keywords, the planes in the order of the entry's structs, the host entry)
MODES = {"first": ({}, OUT, "rt_render_aov"),
         "emit": ({"emit": True}, OUT + EMIT, "rt_render_aov_emit"),
         "media": ({"emit": True, "media": True}, OUT + EMIT + ("scatter",), "rt_render_aov_media"),
         "spec": ({"specular": True}, OUT + ("bounces",), "rt_render_aov_spec")}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def scene(rt, gpu):
    """name -> (the open Scene, its camera at W x H), built once"""
    made = {}

    def get(name):
        if name not in made:
            t, cam, wd, l = rt.demo_scene(name)
            made[name] = (rt.Scene(t, wd, l), _shape(cam, W, H))
        return made[name]

    yield get
    for sc, _ in made.values():
        sc.close()


def host_entry(rt, sc, cam, mode, ptr, emit=True):
    """the mode's C host entry with the addresses of `ptr` (plane -> address), NULL for the rest;
    emit=False: the emit struct itself is NULL (the media entry without the split)"""
    lb = rt._lib
    a = lb.RtAov(*[ptr.get(k) for k in OUT])
    e = lb.RtAovEmit(*[ptr.get(k) for k in EMIT]) if emit else None
    structs = {"first": (a,), "emit": (a, e), "media": (a, e, lb.RtAovMedia(ptr.get("scatter"))),
               "spec": (lb.RtAovSpecOpts(0, 0.0), a, lb.RtAovSpec(ptr.get("bounces")))}[mode]
    c = cam.to_c()
    o = sc._opts(SEED, 0, 0, 1, 0, 0, False, None)  # render_aov's own
    rc = getattr(rt.lib(), MODES[mode][2])(sc._p, C.byref(c), C.byref(o), N,
                                           *[None if s is None else C.byref(s) for s in structs], None)
    assert rc == lb.RT_OK, rt.lib().rt_last_error()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["cornell", "cornell_smoke"])
def test_sparse_planes_of_the_host_entries(rt, scene, name, mode):
    sc, cam = scene(name)
    kw, planes, _ = MODES[mode]
    npix = W * H
    full = sc.render_aov(cam, n_samples=N, seed=SEED, **kw)
    assert tuple(k for k in full if k != "stats") == planes
    assert name != "cornell" or full["stats"]["tree_width"] == 0
    assert (full["material"] >= 0).any() and full["depth"].max() > 0.0
    if mode == "media":
        assert (full["scatter"] > 0.0).any() == (name == "cornell_smoke")

    # the _device entry into torch tensors: the all-planes host call's bits
    dev = {k: torch.full((H, W) + ((3,) if k in CHANNELS else ()), -7, device="cuda:0",
                         dtype=torch.int32 if k == "material" else torch.float32) for k in planes}
    sc.render_aov_device(cam, n_samples=N, seed=SEED, **{k: v.data_ptr() for k, v in dev.items()},
                         **{k: v for k, v in kw.items() if k != "emit"})
    torch.cuda.synchronize()
    for k in planes:
        assert np.array_equal(bits(dev[k].cpu().numpy()), bits(full[k])), k

    words = {k: CHANNELS.get(k, 1) * npix for k in planes}
    start = dict(zip(planes, np.cumsum([0] + [words[k] for k in planes[:-1]])))
    total = sum(words.values())
    devnp = {k: v.cpu().numpy() for k, v in dev.items()}
    cases = [(want, True, (full, devnp)) for want in ((planes[-1], "depth"), ("material",))]
    if mode == "media":  # the media entry given no emit struct at all: the kernels without the split
        cases.append((("scatter", "depth"), False, (sc.render_aov(cam, n_samples=N, seed=SEED, media=True),)))
    for want, emit, refs in cases:
        arena = np.full(total + 9 * npix, SENTINEL, np.uint32)
        host_entry(rt, sc, cam, mode, {k: arena.ctypes.data + 4 * int(start[k]) for k in want}, emit)
        untouched = np.ones(arena.size, bool)
        for k in want:
            got = arena[start[k]:start[k] + words[k]]
            for ref in refs:
                assert np.array_equal(got, bits(ref[k]).ravel()), (want, emit, k)
            untouched[start[k]:start[k] + words[k]] = False
        assert (arena[untouched] == SENTINEL).all(), (want, emit)
