"""rt_reproject_moments / rt_reproject_moments_device (include/rt_abi.h) on a host without a GPU:
the symbols exist with the header's signatures, every refusal returns its code before any device
is touched, and the Python wrappers and Temporal(moments=True) refuse what they must."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_reproject_abi import H, W, _cam
from tests.test_reproject_emit_abi import _Acc, _emit_frames
from tests.test_reproject_light_abi import Args as LightArgs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_reproject_moments", "rt_reproject_moments_device")
PLAIN, EMIT, LIGHT = 0, 1, 2


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    assert {"reproject_moments", "reproject_moments_device"} <= set(rt.__all__)
    assert rt.lib().rt_abi_version() == 4  # additive: callers detect the feature by the symbols
    assert C.sizeof(rt._lib.RtFrame) == 48 and C.sizeof(rt._lib.RtReprojectOpts) == 16  # unchanged
    assert C.sizeof(rt._lib.RtMomentsOpts) == 8
    assert (rt._lib.RT_REPROJECT_PLAIN, rt._lib.RT_REPROJECT_EMIT, rt._lib.RT_REPROJECT_LIGHT) == (0, 1, 2)
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    assert re.search(r"enum \{ RT_REPROJECT_PLAIN = 0, RT_REPROJECT_EMIT = 1, RT_REPROJECT_LIGHT = 2 \};", text)
    m = re.search(r"typedef struct \{([^}]*)\} rt_moments_opts;", text)
    assert m and re.findall(r"^\s*(\w+)\s+(\w+);", m.group(1), re.M) == [("float", "min_frames"), ("int32_t", "radius")]
    assert [f[0] for f in rt._lib.RtMomentsOpts._fields_] == ["min_frames", "radius"]


def test_ctypes_signatures_match_the_header(rt):
    """the prototypes as include/rt_abi.h declares them, parameter by parameter"""
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    kinds = {"const rt_camera*": C.POINTER(rt._lib.RtCamera), "const rt_frame*": C.POINTER(rt._lib.RtFrame),
             "const rt_aov_emit*": C.POINTER(rt._lib.RtAovEmit),
             "const rt_reproject_opts*": C.POINTER(rt._lib.RtReprojectOpts),
             "const rt_moments_opts*": C.POINTER(rt._lib.RtMomentsOpts), "int": C.c_int, "void*": C.c_void_p,
             "const float*": C.c_void_p, "float*": C.c_void_p}
    for name in SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert m, name
        params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
        res, args = rt._lib.SIGNATURES[name]
        assert res is C.c_int and args == [kinds[p] for p in params], (name, params)
    host, dev = (rt._lib.SIGNATURES[s][1] for s in SYMBOLS)
    assert dev == host + [C.c_int, C.c_void_p]
    # rt_reproject_light's arguments after the mode, with prev_lum2 after prev_emit, the moments'
    # options after the reprojection's and out_lum2 last
    light = rt._lib.SIGNATURES["rt_reproject_light"][1]
    assert host == ([C.c_int] + light[:3] + [C.c_void_p] + light[3:9] + [C.POINTER(rt._lib.RtMomentsOpts)]
                    + light[9:] + [C.c_void_p])


class Args(LightArgs):
    """a valid call's arguments, each replaceable"""

    def __init__(self, rt, mode=LIGHT):
        super().__init__(rt)
        self.mode = mode
        self.keep["lum2"] = np.zeros((2, H, W), np.float32)
        self.prev_lum2, self.out_lum2 = (self.keep["lum2"][i].ctypes.data for i in (0, 1))
        self.mopts = rt._lib.RtMomentsOpts(0.0, 0)

    def call(self, fn):
        r = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = [self.mode, r(self.cam_prev), r(self.prev), r(self.prev_emit), self.prev_lum2, r(self.cam_cur),
                r(self.cur), r(self.cur_emit), self.w, self.h, r(self.opts), r(self.mopts), r(self.out),
                r(self.out_emit), self.out_lum2]
        if fn == "rt_reproject_moments_device":
            args += [0, None]
        return getattr(self.rt.lib(), fn)(*args)


def _no_prev(a):
    a.cam_prev = a.prev = a.prev_emit = a.prev_lum2 = None


@pytest.mark.parametrize("fn", SYMBOLS)
def test_argument_errors(rt, fn):
    E, U = rt._lib.RT_ERR_INVALID, rt._lib.RT_ERR_UNSUPPORTED

    def refused(change, code=E, word=None, mode=LIGHT):
        a = Args(rt, mode)
        change(a)
        assert a.call(fn) == code, rt.lib().rt_last_error()
        assert fn.encode() in rt.lib().rt_last_error()
        if word:
            assert word in rt.lib().rt_last_error(), rt.lib().rt_last_error()

    # the selected mode's own refusals (prev = NULL is none here: no history at all)
    for mode in (PLAIN, EMIT, LIGHT):
        for name in ("cam_prev", "cam_cur", "cur", "out"):
            refused(lambda a, name=name: setattr(a, name, None), mode=mode)
        for frame in ("prev", "cur"):
            for key in ("rgb", "normal", "depth"):
                refused(lambda a, frame=frame, key=key: setattr(getattr(a, frame), key, None), mode=mode,
                        word=b"rgb, normal and depth")

        def no_buffer(a):
            a.out.rgb = a.out.var = a.out.count = None
        refused(no_buffer, word=b"no buffer", mode=mode)
        for w, h in ((0, H), (W, -1), (1 << 16, 1 << 16)):
            refused(lambda a, w=w, h=h: (setattr(a, "w", w), setattr(a, "h", h)), mode=mode)
        refused(lambda a: setattr(a, "w", W + 1), word=b"cameras of", mode=mode)
        refused(lambda a: setattr(a, "cam_prev", _cam(rt, W + 2, H).to_c()), word=b"cameras of", mode=mode)
        for field in ("max_history", "depth_tol", "normal_tol", "min_weight"):
            for bad in (-1.0, float("nan"), float("inf")):
                refused(lambda a, field=field, bad=bad: setattr(a.opts, field, bad), word=b"option", mode=mode)
        for ok in ("rgb", "var", "count"):
            for pk in ("rgb", "var", "count", "normal", "depth"):
                refused(lambda a, ok=ok, pk=pk: setattr(a.out, ok, getattr(a.prev, pk)), word=b"aliases", mode=mode)
        for which in ("cam_prev", "cam_cur"):
            refused(lambda a, which=which: setattr(a, which, _cam(rt, DefocusAngle=0.5).to_c()), code=U,
                    word=b"defocus", mode=mode)
    for mode in (EMIT, LIGHT):
        for name in ("prev_emit", "cur_emit"):
            refused(lambda a, name=name: setattr(a, name, None), word=b"null emit", mode=mode)
            for key in ("emission", "coverage"):
                refused(lambda a, name=name, key=key: setattr(getattr(a, name), key, None), mode=mode,
                        word=b"emission and coverage")
        for ok in ("rgb", "var", "count"):
            for pk in ("emission", "surface_albedo", "coverage"):
                refused(lambda a, ok=ok, pk=pk: setattr(a.out, ok, getattr(a.prev_emit, pk)), word=b"aliases", mode=mode)
    refused(lambda a: setattr(a, "out_emit", None), word=b"null out_emit")
    for ok in ("emission", "coverage"):
        for pk in ("rgb", "var", "count", "normal", "depth"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out_emit, ok, getattr(a.prev, pk)), word=b"out_emit aliases")
        for pk in ("emission", "surface_albedo", "coverage"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out_emit, ok, getattr(a.prev_emit, pk)), word=b"out_emit aliases")
    # the moments entries' own
    for mode in (-1, 3, 7):
        refused(lambda a: None, word=b"mode", mode=mode)
    for mode in (PLAIN, EMIT, LIGHT):
        refused(lambda a: setattr(a, "out_lum2", None), word=b"null out_lum2", mode=mode)
        refused(lambda a: setattr(a, "prev_lum2", None), word=b"prev without prev_lum2", mode=mode)
        # prev_lum2 is gathered by the taps like prev's planes: no out buffer is it; nor is one out_lum2
        for ok in ("rgb", "var", "count"):
            refused(lambda a, ok=ok: setattr(a.out, ok, a.prev_lum2), word=b"out aliases prev_lum2", mode=mode)
            refused(lambda a, ok=ok: setattr(a, "out_lum2", getattr(a.out, ok)), word=b"out_lum2 aliases", mode=mode)
        for radius in (-2, -100, 9, 1 << 20):
            refused(lambda a, radius=radius: setattr(a.mopts, "radius", radius), word=b"radius", mode=mode)
        for bad in (-1.0, float("nan"), float("inf"), 1e-3, 1.0, 1.999):
            refused(lambda a, bad=bad: setattr(a.mopts, "min_frames", bad), word=b"min_frames", mode=mode)
        # out_lum2 is no input plane
        for frame in ("prev", "cur"):
            for pk in ("rgb", "var", "count", "normal", "depth"):
                refused(lambda a, frame=frame, pk=pk: setattr(a, "out_lum2", getattr(getattr(a, frame), pk)),
                        word=b"out_lum2 aliases", mode=mode)
        refused(lambda a: setattr(a, "out_lum2", a.prev_lum2), word=b"out_lum2 aliases", mode=mode)
        # no out buffer is a buffer of cur: the window reads the current frame's neighbours
        for ok in ("rgb", "var", "count"):
            for pk in ("rgb", "var", "count", "normal", "depth"):
                refused(lambda a, ok=ok, pk=pk: setattr(a.out, ok, getattr(a.cur, pk)), word=b"buffer of cur", mode=mode)

                def both(a, ok=ok, pk=pk):   # also without a history
                    _no_prev(a)
                    setattr(a.out, ok, getattr(a.cur, pk))
                refused(both, word=b"buffer of cur", mode=mode)
    for mode in (EMIT, LIGHT):
        for frame in ("prev_emit", "cur_emit"):
            for pk in ("emission", "surface_albedo", "coverage"):
                if pk == "surface_albedo" and frame == "cur_emit":
                    continue   # NULL in these arguments
                refused(lambda a, frame=frame, pk=pk: setattr(a, "out_lum2", getattr(getattr(a, frame), pk)),
                        word=b"out_lum2 aliases", mode=mode)
        for ok in ("rgb", "var", "count"):
            for pk in ("emission", "coverage"):
                refused(lambda a, ok=ok, pk=pk: setattr(a.out, ok, getattr(a.cur_emit, pk)), word=b"buffer of cur",
                        mode=mode)
    for ok in ("emission", "coverage"):
        refused(lambda a, ok=ok: setattr(a.out_emit, ok, a.prev_lum2), word=b"out aliases prev_lum2")
        refused(lambda a, ok=ok: setattr(a, "out_lum2", getattr(a.out_emit, ok)), word=b"out_lum2 aliases")
        for pk in ("rgb", "var", "count", "normal", "depth"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out_emit, ok, getattr(a.cur, pk)), word=b"buffer of cur")
        for pk in ("emission", "coverage"):
            refused(lambda a, ok=ok, pk=pk: setattr(a.out_emit, ok, getattr(a.cur_emit, pk)), word=b"buffer of cur")


def test_valid_arguments_reach_the_device(rt):
    """with nothing wrong the call gets past the checks: RT_ERR_DEVICE on a host without a GPU.  So
    do no history at all, NULL options of either kind, every legal radius and min_frames, and in
    PLAIN and EMIT the arguments the mode does not read, whatever they hold"""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are tests/test_reproject_moments_gpu.py's
    D = rt._lib.RT_ERR_DEVICE

    def emits_unread(a):
        a.prev_emit = a.cur_emit = a.out_emit = None
    changes = [lambda a: None, _no_prev, lambda a: setattr(a, "opts", None), lambda a: setattr(a, "mopts", None)]
    changes += [lambda a, r=r: setattr(a.mopts, "radius", r) for r in (-1, 0, 1, 8)]
    changes += [lambda a, m=m: setattr(a.mopts, "min_frames", m) for m in (0.0, 2.0, 4.5, 1e30)]
    for fn in SYMBOLS:
        for mode in (PLAIN, EMIT, LIGHT):
            for change in changes:
                a = Args(rt, mode)
                change(a)
                assert a.call(fn) == D, rt.lib().rt_last_error()
        for mode, change in ((PLAIN, emits_unread), (EMIT, lambda a: setattr(a, "out_emit", None)),
                             (EMIT, lambda a: setattr(a.out_emit, "emission", a.cur.rgb))):
            a = Args(rt, mode)
            change(a)
            assert a.call(fn) == D, rt.lib().rt_last_error()


def _moment_frames():
    prev, cur = _emit_frames()
    return dict(prev, lum2=np.zeros((H, W), np.float32)), cur


def test_python_host_wrapper_refuses_bad_frames(rt):
    cam = _cam(rt)
    prev, cur = _moment_frames()
    for mode in ("plain", "emit", "light"):
        need = ("rgb", "normal", "depth", "lum2") + (() if mode == "plain" else ("emission", "coverage"))
        for key in need:
            with pytest.raises(ValueError, match=key):
                rt.reproject_moments(mode, cam, dict(prev, **{key: None}), cam, cur)
            if key != "lum2":
                with pytest.raises(ValueError, match=key):
                    rt.reproject_moments(mode, cam, prev, cam, dict(cur, **{key: None}))
        with pytest.raises(ValueError, match="lum2"):
            rt.reproject_moments(mode, cam, dict(prev, lum2=np.zeros((H, W, 3), np.float32)), cam, cur)
        with pytest.raises(ValueError, match="cam_prev"):
            rt.reproject_moments(mode, None, prev, cam, cur)
        with pytest.raises(TypeError):
            rt.reproject_moments(mode, cam, prev, cam, cur, sigma=1.0)
    for bad in ("surface", 3, -1, None, True):
        with pytest.raises(ValueError, match="mode"):
            rt.reproject_moments(bad, cam, prev, cam, cur)
    for kw in (dict(var_radius=9), dict(var_radius=-2), dict(min_frames=1.5), dict(min_frames=-4.0)):
        with pytest.raises(rt.RtError) as e:
            rt.reproject_moments("emit", cam, prev, cam, dict(cur, count=3), **kw)
        assert e.value.code == rt._lib.RT_ERR_INVALID
    if rt.device_count() == 0:  # past the wrapper's checks: the library's answer without a GPU
        for args in ((cam, prev), (None, None)):
            with pytest.raises(rt.RtError) as e:
                rt.reproject_moments("light", *args, cam, dict(cur, count=3), min_frames=3.0, var_radius=-1)
            assert e.value.code == rt._lib.RT_ERR_DEVICE and b"rt_reproject_moments" in rt.lib().rt_last_error()


def test_python_device_wrapper_refuses_bad_tensors(rt):
    import torch
    cam = _cam(rt)
    prev, cur = ({k: torch.from_numpy(v.copy()) for k, v in f.items()} for f in _moment_frames())
    bads = (torch.zeros((H, W), dtype=torch.float64), torch.zeros((W, H)), torch.zeros((H, 2 * W))[:, ::2],
            torch.zeros((H, W, 1)), np.zeros((H, W), np.float32))
    for bad in bads:
        with pytest.raises(ValueError, match="lum2"):
            rt.reproject_moments_device("light", cam, dict(prev, lum2=bad), cam, cur)
        with pytest.raises(ValueError, match="lum2"):
            rt.reproject_moments_device("plain", cam, prev, cam, cur, out={"lum2": bad})
    # the taps gather from prev and the window from cur: no out tensor is one of either
    for ok, pk in (("rgb", "emission"), ("emission", "rgb"), ("lum2", "lum2"), ("coverage", "lum2"), ("lum2", "var")):
        with pytest.raises(ValueError, match="prev"):
            rt.reproject_moments_device("light", cam, prev, cam, cur, out={ok: prev[pk]})
    for ok, pk in (("rgb", "rgb"), ("var", "var"), ("emission", "emission"), ("coverage", "coverage"), ("lum2", "depth"),
                   ("var", "coverage")):
        with pytest.raises(ValueError, match="cur"):
            rt.reproject_moments_device("light", cam, prev, cam, cur, out={ok: cur[pk]})
        with pytest.raises(ValueError, match="cur"):
            rt.reproject_moments_device("light", None, None, cam, cur, out={ok: cur[pk]})


def test_temporal_moments_options(rt):
    with pytest.raises(ValueError, match="moments"):
        rt.Temporal(min_frames=3.0)
    with pytest.raises(ValueError, match="moments"):
        rt.Temporal(split_emitters=True, var_radius=2)
    with pytest.raises(ValueError, match="split_emitters"):
        rt.Temporal(moments=True, light_history=True)
    with pytest.raises(TypeError):
        rt.Temporal(moments=True, sigma=1.0)
    for kw in ({}, dict(split_emitters=True), dict(split_emitters=True, light_history=True)):
        t = rt.Temporal(moments=True, min_frames=3.0, var_radius=2, max_history=16.0, **kw)
        assert t.light is None
    with pytest.raises(ValueError, match="features='emit'"):
        rt.Temporal(split_emitters=True, moments=True).push(_Acc())
