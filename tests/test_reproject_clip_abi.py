"""rt_reproject_clip / rt_reproject_clip_device (include/rt_abi.h) on a host without a GPU: the
symbols exist with the header's signatures, every refusal returns its code before any device is
touched (a call with nothing wrong answers RT_ERR_DEVICE here, a refused one RT_ERR_INVALID), and
the Python wrappers and Temporal(clip=True) refuse what they must."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_reproject_abi import H, W, _cam
from tests.test_reproject_emit_abi import _Acc
from tests.test_reproject_moments_abi import EMIT, LIGHT, PLAIN, _moment_frames, _no_prev
from tests.test_reproject_moments_abi import Args as MomentArgs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_reproject_clip", "rt_reproject_clip_device")


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert set(SYMBOLS) <= set(rt._lib.SIGNATURES)
    assert {"reproject_clip", "reproject_clip_device"} <= set(rt.__all__)
    assert rt.lib().rt_abi_version() == 4  # additive: callers detect the feature by the symbols
    assert C.sizeof(rt._lib.RtMomentsOpts) == 8 and C.sizeof(rt._lib.RtClipOpts) == 4
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} rt_clip_opts;", text)
    assert m and re.findall(r"^\s*(\w+)\s+(\w+);", m.group(1), re.M) == [("float", "gamma")]
    assert [f[0] for f in rt._lib.RtClipOpts._fields_] == ["gamma"]


def test_ctypes_signatures_match_the_header(rt):
    """the prototypes as include/rt_abi.h declares them, parameter by parameter: the moments
    entries' with copts directly after mopts"""
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    kinds = {"const rt_camera*": C.POINTER(rt._lib.RtCamera), "const rt_frame*": C.POINTER(rt._lib.RtFrame),
             "const rt_aov_emit*": C.POINTER(rt._lib.RtAovEmit),
             "const rt_reproject_opts*": C.POINTER(rt._lib.RtReprojectOpts),
             "const rt_moments_opts*": C.POINTER(rt._lib.RtMomentsOpts),
             "const rt_clip_opts*": C.POINTER(rt._lib.RtClipOpts), "int": C.c_int, "void*": C.c_void_p,
             "const float*": C.c_void_p, "float*": C.c_void_p}
    for name in SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert m, name
        params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
        names = [p.split()[-1] for p in m.group(1).replace("\n", " ").split(",")]
        res, args = rt._lib.SIGNATURES[name]
        assert res is C.c_int and args == [kinds[p] for p in params], (name, params)
        assert names[names.index("mopts") + 1] == "copts"
    host, dev = (rt._lib.SIGNATURES[s][1] for s in SYMBOLS)
    assert dev == host + [C.c_int, C.c_void_p]
    for clip, mom in zip(SYMBOLS, ("rt_reproject_moments", "rt_reproject_moments_device")):
        a = rt._lib.SIGNATURES[mom][1]
        assert rt._lib.SIGNATURES[clip][1] == a[:12] + [C.POINTER(rt._lib.RtClipOpts)] + a[12:]


class Args(MomentArgs):
    """a valid call's arguments, each replaceable"""

    def __init__(self, rt, mode=LIGHT):
        super().__init__(rt, mode)
        self.copts = rt._lib.RtClipOpts(0.0)

    def call(self, fn):
        r = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = [self.mode, r(self.cam_prev), r(self.prev), r(self.prev_emit), self.prev_lum2, r(self.cam_cur),
                r(self.cur), r(self.cur_emit), self.w, self.h, r(self.opts), r(self.mopts), r(self.copts), r(self.out),
                r(self.out_emit), self.out_lum2]
        if fn == "rt_reproject_clip_device":
            args += [0, None]
        return getattr(self.rt.lib(), fn)(*args)


@pytest.mark.parametrize("with_copts", [True, False], ids=["copts", "null-copts"])
@pytest.mark.parametrize("fn", SYMBOLS)
def test_argument_errors(rt, fn, with_copts):
    E, U = rt._lib.RT_ERR_INVALID, rt._lib.RT_ERR_UNSUPPORTED

    def refused(change, code=E, word=None, mode=LIGHT):
        a = Args(rt, mode)
        if not with_copts:
            a.copts = None
        change(a)
        assert a.call(fn) == code, rt.lib().rt_last_error()
        assert fn.encode() in rt.lib().rt_last_error()
        if word:
            assert word in rt.lib().rt_last_error(), rt.lib().rt_last_error()

    # rt_reproject_moments' own, with and without copts: the selected mode's ...
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
    refused(lambda a: setattr(a, "out_emit", None), word=b"null out_emit")
    # ... and the moments entries' own
    for mode in (-1, 3, 7):
        refused(lambda a: None, word=b"mode", mode=mode)
    for mode in (PLAIN, EMIT, LIGHT):
        refused(lambda a: setattr(a, "out_lum2", None), word=b"null out_lum2", mode=mode)
        refused(lambda a: setattr(a, "prev_lum2", None), word=b"prev without prev_lum2", mode=mode)
        for ok in ("rgb", "var", "count"):
            refused(lambda a, ok=ok: setattr(a.out, ok, a.prev_lum2), word=b"out aliases prev_lum2", mode=mode)
            refused(lambda a, ok=ok: setattr(a, "out_lum2", getattr(a.out, ok)), word=b"out_lum2 aliases", mode=mode)
            refused(lambda a, ok=ok: setattr(a.out, ok, a.cur.rgb), word=b"buffer of cur", mode=mode)
        for radius in (-2, -100, 9, 1 << 20):
            refused(lambda a, radius=radius: setattr(a.mopts, "radius", radius), word=b"radius", mode=mode)
        for bad in (-1.0, float("nan"), float("inf"), 1e-3, 1.0, 1.999):
            refused(lambda a, bad=bad: setattr(a.mopts, "min_frames", bad), word=b"min_frames", mode=mode)
        refused(lambda a: setattr(a, "out_lum2", a.prev_lum2), word=b"out_lum2 aliases", mode=mode)
    if not with_copts:
        return
    # the clip entries' own: no window, and a gamma that is negative or not finite
    for mode in (PLAIN, EMIT, LIGHT):
        refused(lambda a: setattr(a.mopts, "radius", -1), word=b"window", mode=mode)

        def no_window_no_prev(a):
            _no_prev(a)
            a.mopts.radius = -1
        refused(no_window_no_prev, word=b"window", mode=mode)
        for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            refused(lambda a, bad=bad: setattr(a.copts, "gamma", bad), word=b"gamma", mode=mode)


def test_valid_arguments_reach_the_device(rt):
    """with nothing wrong the call gets past the checks: RT_ERR_DEVICE on a host without a GPU.  So
    do NULL copts (also with radius -1: the moments entry's call), every legal gamma and radius,
    and no history at all"""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are tests/test_reproject_clip_gpu.py's
    D = rt._lib.RT_ERR_DEVICE

    def null_copts_no_window(a):
        a.copts = None
        a.mopts.radius = -1
    changes = [lambda a: None, _no_prev, lambda a: setattr(a, "opts", None), lambda a: setattr(a, "mopts", None),
               lambda a: setattr(a, "copts", None), null_copts_no_window]
    changes += [lambda a, r=r: setattr(a.mopts, "radius", r) for r in (0, 1, 8)]
    changes += [lambda a, g=g: setattr(a.copts, "gamma", g) for g in (0.0, 0.75, 1.0, 3.0, 1e30)]
    for fn in SYMBOLS:
        for mode in (PLAIN, EMIT, LIGHT):
            for change in changes:
                a = Args(rt, mode)
                change(a)
                assert a.call(fn) == D, rt.lib().rt_last_error()
                assert fn.encode() in rt.lib().rt_last_error()


def test_python_wrappers_refuse_what_they_must(rt):
    import torch
    cam = _cam(rt)
    prev, cur = _moment_frames()
    for mode in ("plain", "emit", "light"):
        for key in ("rgb", "normal", "depth", "lum2"):
            with pytest.raises(ValueError, match=key):
                rt.reproject_clip(mode, cam, dict(prev, **{key: None}), cam, cur)
        with pytest.raises(ValueError, match="cam_prev"):
            rt.reproject_clip(mode, None, prev, cam, cur)
        with pytest.raises(TypeError):
            rt.reproject_clip(mode, cam, prev, cam, cur, sigma=1.0)
    with pytest.raises(ValueError, match="reproject_clip: mode"):
        rt.reproject_clip("surface", cam, prev, cam, cur)
    for kw in (dict(var_radius=-1), dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(var_radius=9), dict(min_frames=1.5)):
        with pytest.raises(rt.RtError) as e:
            rt.reproject_clip("emit", cam, prev, cam, dict(cur, count=3), **kw)
        assert e.value.code == rt._lib.RT_ERR_INVALID and b"rt_reproject_clip" in rt.lib().rt_last_error()
    if rt.device_count() == 0:  # past the wrapper's checks: the library's answer without a GPU
        for args in ((cam, prev), (None, None)):
            with pytest.raises(rt.RtError) as e:
                rt.reproject_clip("light", *args, cam, dict(cur, count=3), gamma=1.5, var_radius=2)
            assert e.value.code == rt._lib.RT_ERR_DEVICE and b"rt_reproject_clip" in rt.lib().rt_last_error()
    tp, tc = ({k: torch.from_numpy(v.copy()) for k, v in f.items()} for f in (prev, cur))
    with pytest.raises(ValueError, match="reproject_clip_device: .*lum2"):
        rt.reproject_clip_device("light", cam, dict(tp, lum2=np.zeros((H, W), np.float32)), cam, tc)
    with pytest.raises(ValueError, match="prev"):
        rt.reproject_clip_device("light", cam, tp, cam, tc, out={"rgb": tp["emission"]})
    with pytest.raises(ValueError, match="cur"):
        rt.reproject_clip_device("light", cam, tp, cam, tc, out={"rgb": tc["rgb"]})


def test_temporal_clip_options(rt):
    with pytest.raises(ValueError, match="moments=True"):
        rt.Temporal(clip=True)
    with pytest.raises(ValueError, match="moments=True"):
        rt.Temporal(split_emitters=True, clip=True)
    with pytest.raises(ValueError, match="var_radius >= 0"):
        rt.Temporal(moments=True, clip=True, var_radius=-1)
    with pytest.raises(ValueError, match="clip=True"):
        rt.Temporal(moments=True, clip_gamma=1.5)
    with pytest.raises(ValueError, match="rounds to 0"):
        rt.reproject_clip("plain", _cam(rt), _moment_frames()[0], _cam(rt), _moment_frames()[1], gamma=1e-60)
    for bad in (-1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="clip_gamma"):
            rt.Temporal(moments=True, clip=True, clip_gamma=bad)
    for kw in ({}, dict(split_emitters=True), dict(split_emitters=True, light_history=True)):
        t = rt.Temporal(moments=True, clip=True, clip_gamma=1.5, min_frames=3.0, var_radius=2, max_history=16.0, **kw)
        assert t.light is None
    with pytest.raises(ValueError, match="features='emit'"):
        rt.Temporal(split_emitters=True, moments=True, clip=True).push(_Acc())
