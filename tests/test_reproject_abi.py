"""rt_reproject / rt_reproject_device (include/rt_abi.h) on a host without a GPU: the symbols
exist, rt_frame and rt_reproject_opts have the header's layout, every refusal returns its code
before any device is touched, and the Python wrappers and Temporal refuse what they must."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_reproject", "rt_reproject_device")
W, H = 6, 4


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    assert {"reproject", "reproject_device", "Temporal"} <= set(rt.__all__)
    assert rt.lib().rt_abi_version() == 4  # additive: callers detect the feature by the symbols


def test_struct_sizes(rt):
    assert C.sizeof(rt._lib.RtFrame) == 48 and C.sizeof(rt._lib.RtReprojectOpts) == 16


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_struct_layout_matches_header(rt, tmp_path):
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){'
                 'printf("%zu %zu %zu %zu %zu\\n", sizeof(rt_frame), sizeof(rt_reproject_opts),'
                 " offsetof(rt_frame, depth), offsetof(rt_frame, count_scalar),"
                 " offsetof(rt_reproject_opts, min_weight));return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    f, o, depth, scalar, mw = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                      text=True).stdout.split())
    F, O = rt._lib.RtFrame, rt._lib.RtReprojectOpts
    assert (f, o) == (C.sizeof(F), C.sizeof(O))
    assert (depth, scalar, mw) == (F.depth.offset, F.count_scalar.offset, O.min_weight.offset)


def _cam(rt, w=W, h=H, **kw):
    cam = rt.Camera(Width=w, AspectRatio=w / (h + 0.25), VerticalFOV=40.0, **kw)
    cam.PositionCamera((0, 0, 0), (0, 0, -1), (0, 1, 0))
    return cam


class Args:
    """a valid call's arguments, each replaceable"""

    def __init__(self, rt):
        self.rt = rt
        self.keep = {k: np.zeros((2, H, W, 3) if k in ("rgb", "normal") else (2, H, W), np.float32)
                     for k in ("rgb", "var", "count", "normal", "depth")}
        self.keep["out"] = np.zeros((H, W, 5), np.float32)
        F = rt._lib.RtFrame
        self.prev = F(*[self.keep[k][0].ctypes.data for k in ("rgb", "var", "count", "normal", "depth")], 1.0, 0)
        self.cur = F(*[self.keep[k][1].ctypes.data for k in ("rgb", "var", "count", "normal", "depth")], 1.0, 0)
        o = self.keep["out"]
        self.out = F(o[..., :3].ctypes.data, o[..., 3].ctypes.data, o[..., 4].ctypes.data, None, None, 0.0, 0)
        self.cam_prev, self.cam_cur = _cam(rt).to_c(), _cam(rt).to_c()
        self.opts = rt._lib.RtReprojectOpts()
        self.w, self.h = W, H

    def call(self, fn):
        r = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = [r(self.cam_prev), r(self.prev), r(self.cam_cur), r(self.cur), self.w, self.h, r(self.opts),
                r(self.out)]
        if fn == "rt_reproject_device":
            args += [0, None]
        return getattr(self.rt.lib(), fn)(*args)


@pytest.mark.parametrize("fn", SYMBOLS)
def test_argument_errors(rt, fn):
    E, U = rt._lib.RT_ERR_INVALID, rt._lib.RT_ERR_UNSUPPORTED

    def refused(change, code=E, word=None):
        a = Args(rt)
        change(a)
        assert a.call(fn) == code, rt.lib().rt_last_error()
        if word:
            assert word in rt.lib().rt_last_error(), rt.lib().rt_last_error()

    for name in ("cam_prev", "cam_cur", "prev", "cur", "out"):          # a NULL camera, frame or out
        refused(lambda a, name=name: setattr(a, name, None))
    for frame in ("prev", "cur"):                                          # a missing rgb, normal or depth
        for key in ("rgb", "normal", "depth"):
            refused(lambda a, frame=frame, key=key: setattr(getattr(a, frame), key, None), word=b"rgb, normal and depth")

    def no_buffer(a):
        a.out.rgb = a.out.var = a.out.count = None
    refused(no_buffer, word=b"no buffer")                                  # at least one out buffer
    for w, h in ((0, H), (W, -1), (1 << 16, 1 << 16)):                     # the size
        refused(lambda a, w=w, h=h: (setattr(a, "w", w), setattr(a, "h", h)))
    refused(lambda a: setattr(a, "w", W + 1), word=b"cameras of")          # a camera that is not w x h
    refused(lambda a: setattr(a, "cam_prev", _cam(rt, W + 2, H).to_c()), word=b"cameras of")
    refused(lambda a: setattr(a, "cam_cur", _cam(rt, W, H + 1).to_c()), word=b"cameras of")
    for field in ("max_history", "depth_tol", "normal_tol", "min_weight"):  # negative or non-finite options
        for bad in (-1.0, float("nan"), float("inf")):
            refused(lambda a, field=field, bad=bad: setattr(a.opts, field, bad), word=b"option")
    for ok in ("rgb", "var", "count"):                                     # out may not be a prev buffer
        for pk in ("rgb", "var", "count", "normal", "depth"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out, ok, getattr(a.prev, pk)), word=b"aliases")
    for which in ("cam_prev", "cam_cur"):                                  # a defocus camera
        refused(lambda a, which=which: setattr(a, which, _cam(rt, DefocusAngle=0.5).to_c()), code=U, word=b"defocus")


def test_valid_arguments_reach_the_device(rt):
    """with nothing wrong the call gets past the checks: RT_ERR_DEVICE on a host without a GPU.
    So do the optional parts: NULL options, out = cur's buffers, frames without var and count, one
    out buffer only."""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are tests/test_reproject_gpu.py's
    D = rt._lib.RT_ERR_DEVICE

    def inplace(a):
        a.out.rgb, a.out.var, a.out.count = a.cur.rgb, a.cur.var, a.cur.count

    def bare(a):
        a.prev.var = a.prev.count = a.cur.var = a.cur.count = None
        a.out.rgb = a.out.count = None
    for fn in SYMBOLS:
        for change in (lambda a: None, lambda a: setattr(a, "opts", None), inplace, bare):
            a = Args(rt)
            change(a)
            assert a.call(fn) == D, rt.lib().rt_last_error()


def _frames(w=W, h=H):
    f = {"rgb": np.zeros((h, w, 3), np.float32), "var": np.zeros((h, w), np.float32),
         "count": np.ones((h, w), np.float32), "normal": np.zeros((h, w, 3), np.float32),
         "depth": np.ones((h, w), np.float32)}
    return f, dict(f)


def test_python_host_wrapper_refuses_bad_frames(rt):
    cam = _cam(rt)
    prev, cur = _frames()
    for key in ("rgb", "normal", "depth"):
        for frames in ((dict(prev, **{key: None}), cur), (prev, dict(cur, **{key: None}))):
            with pytest.raises(ValueError):
                rt.reproject(cam, frames[0], cam, frames[1])
    bad = {"rgb": np.zeros((W, H, 3), np.float32), "var": np.zeros((H, W, 1), np.float32),
           "count": np.zeros((H + 1, W), np.float32), "normal": np.zeros((H, W), np.float32),
           "depth": np.zeros((H, W, 3), np.float32)}
    for key, arr in bad.items():
        with pytest.raises(ValueError):
            rt.reproject(cam, dict(prev, **{key: arr}), cam, cur)
        if key != "rgb":  # cur's rgb gives the size
            with pytest.raises(ValueError):
                rt.reproject(cam, prev, cam, dict(cur, **{key: arr}))
    with pytest.raises(ValueError):
        rt.reproject(cam, None, cam, cur)
    with pytest.raises(TypeError):
        rt.reproject(cam, prev, cam, cur, sigma=1.0)
    if rt.device_count() == 0:  # past the wrapper's checks: the library's answer without a GPU
        with pytest.raises(rt.RtError) as e:
            rt.reproject(cam, prev, cam, dict(cur, count=3))
        assert e.value.code == rt._lib.RT_ERR_DEVICE
        with pytest.raises(rt.RtError) as e:
            rt.reproject(_cam(rt, W + 1, H), prev, cam, cur)
        assert e.value.code == rt._lib.RT_ERR_INVALID


def test_python_device_wrapper_refuses_bad_tensors(rt):
    import torch
    cam = _cam(rt)
    prev, cur = ({k: torch.from_numpy(v.copy()) for k, v in f.items()} for f in _frames())
    wrong = {"rgb": (torch.zeros((H, W, 3), dtype=torch.float64), torch.zeros((W, H, 3)),
                     torch.zeros((H, W, 6))[..., ::2], np.zeros((H, W, 3), np.float32)),
             "plane": (torch.zeros((H, W), dtype=torch.float64), torch.zeros((W, H)), torch.zeros((H, 2 * W))[:, ::2],
                       torch.zeros((H, W, 1)), np.zeros((H, W), np.float32))}
    for key in ("rgb", "var", "count", "normal", "depth"):
        for bad in wrong["rgb" if key in ("rgb", "normal") else "plane"]:
            with pytest.raises(ValueError):
                rt.reproject_device(cam, dict(prev, **{key: bad}), cam, cur)
            with pytest.raises(ValueError):
                rt.reproject_device(cam, prev, cam, dict(cur, **{key: bad}))
    for key in ("rgb", "var", "count"):
        for bad in wrong["rgb" if key == "rgb" else "plane"]:
            with pytest.raises(ValueError):
                rt.reproject_device(cam, prev, cam, cur, out={key: bad})
        with pytest.raises(ValueError):  # the taps gather from prev
            rt.reproject_device(cam, prev, cam, cur, out={key: prev[key]})
    with pytest.raises(ValueError):
        rt.reproject_device(cam, dict(prev, depth=None), cam, cur)
    if torch.cuda.is_available():  # another device than cur's rgb
        with pytest.raises(ValueError):
            rt.reproject_device(cam, prev, cam, dict(cur, depth=cur["depth"].cuda()))


class _NoFeatures:
    features, nranks, passes, shape, _device = None, 1, 2, (H, W), 0


def test_temporal_refuses_what_it_cannot_use(rt):
    t = rt.Temporal(max_history=16.0)
    with pytest.raises(TypeError):
        rt.Temporal(sigma=1.0)
    with pytest.raises(ValueError, match="features"):
        t.push(_NoFeatures())
    shares, empty = _NoFeatures(), _NoFeatures()
    shares.features, shares.nranks = "guides", 2
    empty.features, empty.passes = "emit", 0
    with pytest.raises(ValueError, match="whole image"):
        t.push(shares)
    with pytest.raises(ValueError, match="no pass"):
        t.push(empty)
    t.reset()
    # a real accumulator without features, where one can be made (rt_accum_create needs a device)
    if rt.device_count() > 0:
        tr, cam, w, l = rt.demo_scene("cornell")
        cam.Width, cam.SamplesPerPixel = 8, 1
        with rt.Scene(tr, w, l) as sc, sc.accumulator(cam, max_passes=1) as acc:
            assert acc.nranks == 1 and acc.camera.Width == 8
            with pytest.raises(ValueError, match="features"):
                t.push(acc)
