"""rt_reproject_light / rt_reproject_light_device (include/rt_abi.h) on a host without a GPU: the
symbols exist with the header's signatures, every refusal returns its code before any device is
touched, and the Python wrappers and Temporal(light_history=True) refuse what they must."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_reproject_abi import H, W, _cam
from tests.test_reproject_emit_abi import Args as EmitArgs
from tests.test_reproject_emit_abi import _Acc, _emit_frames

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_reproject_light", "rt_reproject_light_device")


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    assert {"reproject_light", "reproject_light_device"} <= set(rt.__all__)
    assert rt.lib().rt_abi_version() == 4  # additive: callers detect the feature by the symbols
    assert C.sizeof(rt._lib.RtFrame) == 48 and C.sizeof(rt._lib.RtReprojectOpts) == 16  # unchanged
    assert C.sizeof(rt._lib.RtAovEmit) == 24


def test_ctypes_signatures_match_the_header(rt):
    """the prototypes as include/rt_abi.h declares them, parameter by parameter"""
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    kinds = {"const rt_camera*": C.POINTER(rt._lib.RtCamera), "const rt_frame*": C.POINTER(rt._lib.RtFrame),
             "const rt_aov_emit*": C.POINTER(rt._lib.RtAovEmit),
             "const rt_reproject_opts*": C.POINTER(rt._lib.RtReprojectOpts), "int": C.c_int, "void*": C.c_void_p}
    for name in SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert m, name
        params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
        res, args = rt._lib.SIGNATURES[name]
        assert res is C.c_int and args == [kinds[p] for p in params], (name, params)
    host, dev = (rt._lib.SIGNATURES[s][1] for s in SYMBOLS)
    assert dev == host + [C.c_int, C.c_void_p]
    # rt_reproject_emit's arguments with the new history's rt_aov_emit after out
    assert host == rt._lib.SIGNATURES["rt_reproject_emit"][1] + [C.POINTER(rt._lib.RtAovEmit)]


class Args(EmitArgs):
    """a valid call's arguments, each replaceable"""

    def __init__(self, rt):
        super().__init__(rt)
        self.keep["out_emission"] = np.zeros((H, W, 3), np.float32)
        self.keep["out_coverage"] = np.zeros((H, W), np.float32)
        self.out_emit = rt._lib.RtAovEmit(self.keep["out_emission"].ctypes.data, None,
                                          self.keep["out_coverage"].ctypes.data)

    def call(self, fn):
        r = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = [r(self.cam_prev), r(self.prev), r(self.prev_emit), r(self.cam_cur), r(self.cur), r(self.cur_emit),
                self.w, self.h, r(self.opts), r(self.out), r(self.out_emit)]
        if fn == "rt_reproject_light_device":
            args += [0, None]
        return getattr(self.rt.lib(), fn)(*args)


@pytest.mark.parametrize("fn", SYMBOLS)
def test_argument_errors(rt, fn):
    E, U = rt._lib.RT_ERR_INVALID, rt._lib.RT_ERR_UNSUPPORTED

    def refused(change, code=E, word=None):
        a = Args(rt)
        change(a)
        assert a.call(fn) == code, rt.lib().rt_last_error()
        assert fn.encode() in rt.lib().rt_last_error()
        if word:
            assert word in rt.lib().rt_last_error(), rt.lib().rt_last_error()

    # rt_reproject's refusals
    for name in ("cam_prev", "cam_cur", "prev", "cur", "out"):
        refused(lambda a, name=name: setattr(a, name, None))
    for frame in ("prev", "cur"):
        for key in ("rgb", "normal", "depth"):
            refused(lambda a, frame=frame, key=key: setattr(getattr(a, frame), key, None), word=b"rgb, normal and depth")

    def no_buffer(a):
        a.out.rgb = a.out.var = a.out.count = None
    refused(no_buffer, word=b"no buffer")
    for w, h in ((0, H), (W, -1), (1 << 16, 1 << 16)):
        refused(lambda a, w=w, h=h: (setattr(a, "w", w), setattr(a, "h", h)))
    refused(lambda a: setattr(a, "w", W + 1), word=b"cameras of")
    refused(lambda a: setattr(a, "cam_prev", _cam(rt, W + 2, H).to_c()), word=b"cameras of")
    for field in ("max_history", "depth_tol", "normal_tol", "min_weight"):
        for bad in (-1.0, float("nan"), float("inf")):
            refused(lambda a, field=field, bad=bad: setattr(a.opts, field, bad), word=b"option")
    for ok in ("rgb", "var", "count"):
        for pk in ("rgb", "var", "count", "normal", "depth"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out, ok, getattr(a.prev, pk)), word=b"aliases")
    for which in ("cam_prev", "cam_cur"):
        refused(lambda a, which=which: setattr(a, which, _cam(rt, DefocusAngle=0.5).to_c()), code=U, word=b"defocus")
    # rt_reproject_emit's
    for name in ("prev_emit", "cur_emit"):
        refused(lambda a, name=name: setattr(a, name, None), word=b"null emit")
        for key in ("emission", "coverage"):
            refused(lambda a, name=name, key=key: setattr(getattr(a, name), key, None), word=b"emission and coverage")
    for ok in ("rgb", "var", "count"):
        for pk in ("emission", "surface_albedo", "coverage"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out, ok, getattr(a.prev_emit, pk)), word=b"aliases")
    # the light entries' own: a NULL out_emit; an out_emit buffer that is a buffer of prev or prev_emit
    refused(lambda a: setattr(a, "out_emit", None), word=b"null out_emit")
    for ok in ("emission", "coverage"):
        for pk in ("rgb", "var", "count", "normal", "depth"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out_emit, ok, getattr(a.prev, pk)), word=b"out_emit aliases")
        for pk in ("emission", "surface_albedo", "coverage"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out_emit, ok, getattr(a.prev_emit, pk)), word=b"out_emit aliases")


def test_valid_arguments_reach_the_device(rt):
    """with nothing wrong the call gets past the checks: RT_ERR_DEVICE on a host without a GPU.
    So do the optional parts: either plane of out_emit NULL (or both), out_emit's surface_albedo
    set to a buffer of prev (it is never read or written), NULL options, out = cur's buffers and
    out_emit = cur_emit's."""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are tests/test_reproject_light_gpu.py's
    D = rt._lib.RT_ERR_DEVICE

    def inplace(a):
        a.out.rgb, a.out.var, a.out.count = a.cur.rgb, a.cur.var, a.cur.count
        a.out_emit.emission, a.out_emit.coverage = a.cur_emit.emission, a.cur_emit.coverage

    def no_planes(a):
        a.out_emit.emission = a.out_emit.coverage = None
    for fn in SYMBOLS:
        for change in (lambda a: None, lambda a: setattr(a.out_emit, "emission", None),
                       lambda a: setattr(a.out_emit, "coverage", None), no_planes,
                       lambda a: setattr(a.out_emit, "surface_albedo", a.prev.rgb),
                       lambda a: setattr(a, "opts", None), inplace):
            a = Args(rt)
            change(a)
            assert a.call(fn) == D, rt.lib().rt_last_error()


def test_python_host_wrapper_refuses_bad_frames(rt):
    cam = _cam(rt)
    prev, cur = _emit_frames()
    for key in ("rgb", "normal", "depth", "emission", "coverage"):
        for frames in ((dict(prev, **{key: None}), cur), (prev, dict(cur, **{key: None}))):
            with pytest.raises(ValueError, match=key):
                rt.reproject_light(cam, frames[0], cam, frames[1])
    bad = {"emission": np.zeros((H, W), np.float32), "coverage": np.zeros((H, W, 3), np.float32)}
    for key, arr in bad.items():
        for frames in ((dict(prev, **{key: arr}), cur), (prev, dict(cur, **{key: arr}))):
            with pytest.raises(ValueError, match=key):
                rt.reproject_light(cam, frames[0], cam, frames[1])
    with pytest.raises(TypeError):
        rt.reproject_light(cam, prev, cam, cur, sigma=1.0)
    if rt.device_count() == 0:  # past the wrapper's checks: the library's answer without a GPU
        with pytest.raises(rt.RtError) as e:
            rt.reproject_light(cam, prev, cam, dict(cur, count=3))
        assert e.value.code == rt._lib.RT_ERR_DEVICE and b"rt_reproject_light" in rt.lib().rt_last_error()


def test_python_device_wrapper_refuses_bad_tensors(rt):
    import torch
    cam = _cam(rt)
    prev, cur = ({k: torch.from_numpy(v.copy()) for k, v in f.items()} for f in _emit_frames())
    wrong = {"emission": (torch.zeros((H, W, 3), dtype=torch.float64), torch.zeros((W, H, 3)),
                          torch.zeros((H, W, 6))[..., ::2], np.zeros((H, W, 3), np.float32)),
             "coverage": (torch.zeros((H, W), dtype=torch.float64), torch.zeros((W, H)), torch.zeros((H, 2 * W))[:, ::2],
                          torch.zeros((H, W, 1)), np.zeros((H, W), np.float32))}
    for key, bads in wrong.items():
        for bad in bads:
            with pytest.raises(ValueError, match=key):
                rt.reproject_light_device(cam, dict(prev, **{key: bad}), cam, cur)
            with pytest.raises(ValueError, match=key):
                rt.reproject_light_device(cam, prev, cam, cur, out={key: bad})
    # the taps gather from prev: no out tensor, emission and coverage included, is one of prev's
    for ok, pk in (("rgb", "emission"), ("emission", "rgb"), ("emission", "emission"), ("coverage", "coverage"),
                   ("coverage", "var"), ("count", "coverage")):
        with pytest.raises(ValueError, match="prev"):
            rt.reproject_light_device(cam, prev, cam, cur, out={ok: prev[pk]})


def test_temporal_light_history_needs_split_emitters(rt):
    with pytest.raises(ValueError, match="split_emitters"):
        rt.Temporal(light_history=True)
    with pytest.raises(ValueError, match="split_emitters"):
        rt.Temporal(split_emitters=False, light_history=True, max_history=4.0)
    t = rt.Temporal(split_emitters=True, light_history=True, max_history=16.0)
    assert t.light is None
    with pytest.raises(ValueError, match="features='emit'"):
        t.push(_Acc())
    assert rt.Temporal().light is None and rt.Temporal(split_emitters=True).light is None
