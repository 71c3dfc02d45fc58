"""The host side's device resources (rt_hip_util.h's owners, DESIGN.md "Device resources"), seen
from the ABI: every entry leaves the caller's current device as it found it, the buffers a scene
grows, shrinks and releases give the same bits every time round, and the RCCL gather's send
buffers grow and shrink like the peer-copy path's.  The images are tiny (16 x 16 to 48 x 32
Cornell, a few samples): what is under test is which buffer is allocated when, not the render."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

two_devices = pytest.mark.skipif("__import__('go_raytracer_amd').device_count() < 2")


def _cornell(rt, w=16, h=16, spp=1):
    t, cam, wd, l = rt.demo_scene("cornell")
    cam.Width, cam.AspectRatio, cam.SamplesPerPixel = w, w / (h + 0.5), spp
    assert cam.image_size()[:2] == (w, h)
    return t, cam, wd, l


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a if k != "stats")
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, bytes):
        return a == b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# --------------------------------------------------------------- current device restored --
def _entries(rt):
    """name -> f(device): one call of the entry on `device`, its outputs on the host"""
    import torch
    img = np.random.default_rng(5).uniform(-0.1, 1.3, (16, 16, 3)).astype(np.float32)
    boxes = np.random.default_rng(6).uniform(0.0, 1.0, (17, 6)).astype(np.float32)
    boxes[:, 3:] += boxes[:, :3]
    t, cam, w, l = _cornell(rt)
    sc = rt.Scene(t, w, l)
    guides = {k: v for k, v in sc.render_aov(cam, seed=2, device=0).items() if k in ("albedo", "normal", "depth")}

    def on(device, a):
        return torch.from_numpy(a).to(f"cuda:{device}")

    def accum(device):
        with sc.accumulator(cam, max_passes=2, device=device) as acc:
            acc.add(7)
            return acc.resolve()

    def build(device):  # the box builder runs on the caller's current device
        with torch.cuda.device(device):
            res = rt.build_bvh_boxes(boxes, builder=1)
            assert torch.cuda.current_device() == device
        return res

    return sc, {
        "quantize_device": lambda d: rt.quantize_device(on(d, img)).cpu().numpy(),
        "format_ppm_device": lambda d: rt.format_ppm_device(on(d, img)),
        "render": lambda d: sc.render(cam, seed=2, device=d)[0],
        "render_aov": lambda d: sc.render_aov(cam, seed=2, device=d),
        "denoise_device": lambda d: rt.denoise_device(on(d, img), {k: on(d, v) for k, v in guides.items()}).cpu().numpy(),
        "accumulator": accum,
        "build_bvh_boxes": build,
    }


@two_devices
def test_entries_restore_the_current_device(rt, gpu):
    """With device 0 current in torch, every entry called for device 1 returns with device 0
    still current, and gives the bits of the same call for device 0."""
    import torch
    torch.cuda.set_device(0)
    sc, entries = _entries(rt)
    try:
        wrong, differ = [], []
        for name, call in entries.items():
            ref = call(0)
            assert torch.cuda.current_device() == 0, name
            got = call(1)
            if torch.cuda.current_device() != 0:
                wrong.append((name, torch.cuda.current_device()))
                torch.cuda.set_device(0)
            if not _same(ref, got):
                differ.append(name)
        assert wrong == [] and differ == []
    finally:
        sc.close()
        torch.cuda.set_device(0)


# ------------------------------------------------------------------- regrow and release --
def _round(rt):
    """One scene's life: its render state grown, regrown and given the wavefront buffers, an
    accumulator whose feature planes go on, off and on, the gather buffer grown; then closed"""
    L = rt.lib()
    t, cam, w, l = _cornell(rt, 16, 16, 4)
    _, big, _, _ = _cornell(rt, 48, 32, 4)
    _, tall, _, _ = _cornell(rt, 16, 18, 4)
    out = []
    with rt.Scene(t, w, l) as sc:
        out.append(sc.render(cam, seed=3)[0])
        out.append(sc.render(big, seed=3)[0])  # RenderState regrown
        out.append(sc.render(cam, seed=3)[0])
        out.append(sc.render(cam, seed=3, mode="wavefront")[0])  # the SoA buffers appear
        with sc.accumulator(cam, max_passes=4, features="emit") as acc:
            for planes in (None, 0, 3):  # on (as created), off, on again
                if planes is not None:
                    acc.reset()
                    rt.check(L.rt_accum_set_features(acc._p, planes))
                acc.add(1)
                acc.add(2)
                out.append(acc.resolve())
                if acc.features is not None:
                    out.append(acc.resolve_aov())
        out.append(sc.render_multi(cam, [0, 0], seed=3)[0])      # the gather buffer
        out.append(sc.render_multi(tall, [0, 0, 0], seed=3)[0])  # ... regrown
    return out


def test_regrow_and_release_rounds_are_bitwise(rt, gpu):
    """Three lives of the same scene in one process: every image of the second and third equals
    the first's bit for bit, the small render equals itself across the regrown state, the
    shares equal the one-device render, and no call fails."""
    rounds = [_round(rt) for _ in range(3)]
    first = rounds[0]
    assert len(first) == 11
    assert _same(first[0], first[2])
    assert _same(first[0], first[9])    # render_multi over [0, 0], 16 x 16
    assert _same(first[4], first[6])    # features off: the same image and variance
    assert _same(first[4], first[7]) and _same(first[5], first[8])  # ... and on again: and planes
    for later in rounds[1:]:
        assert len(later) == len(first)
        for i, (a, b) in enumerate(zip(first, later)):
            assert _same(a, b), i


# ---------------------------------------------------------------------------- RCCL path --
@two_devices
def test_rccl_send_buffers_grow_and_shrink(rt, gpu):
    """rt_render_multi with the RCCL gather at 16 x 16, 16 x 64 (the send buffers grown) and
    16 x 16 again: each image equals the peer-copy path's, bit for bit."""
    t, cam, w, l = _cornell(rt, 16, 16, 4)
    _, tall, _, _ = _cornell(rt, 16, 64, 4)
    with rt.Scene(t, w, l) as sc:
        for c in (cam, tall, cam):
            peer, _ = sc.render_multi(c, [0, 1], seed=3)
            rccl, _ = sc.render_multi(c, [0, 1], seed=3, rccl=True)
            assert np.array_equal(peer, rccl, equal_nan=True), c.image_size()
