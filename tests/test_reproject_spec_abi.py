"""rt_reproject_spec[_device], rt_accum_set_features_spec and rt_accum_resolve_aov_spec[_device]
(include/rt_abi.h) on a host without a GPU: the symbols exist with the header's signatures, every
refusal returns its code before any device is touched (a reprojection with nothing wrong answers
RT_ERR_DEVICE here, a refused one RT_ERR_INVALID), and the Python wrappers and
Temporal(specular=True) refuse what they must."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_reproject_abi import H, W, _cam
from tests.test_reproject_clip_abi import Args as ClipArgs
from tests.test_reproject_emit_abi import _Acc
from tests.test_reproject_moments_abi import EMIT, LIGHT, PLAIN, _moment_frames, _no_prev

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_reproject_spec", "rt_reproject_spec_device")
ACCUM = ("rt_accum_set_features_spec", "rt_accum_resolve_aov_spec", "rt_accum_resolve_aov_spec_device")


def test_symbols_exist(rt):
    L = C.CDLL(rt._lib.LIB_PATH)
    assert [s for s in SYMBOLS + ACCUM if not hasattr(L, s)] == []
    assert set(SYMBOLS + ACCUM) <= set(rt._lib.SIGNATURES)
    assert {"reproject_spec", "reproject_spec_device"} <= set(rt.__all__)
    assert rt.lib().rt_abi_version() == 4  # additive: callers detect the feature by the symbols
    assert rt._lib.RT_ACCUM_FEAT_SPEC == 8 and C.sizeof(rt._lib.RtSpecPlanes) == 2 * C.sizeof(C.c_void_p)
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    assert re.search(r"#define RT_ACCUM_FEAT_SPEC\s+8u", text)
    m = re.search(r"typedef struct \{([^}]*)\} rt_spec_planes;", text)
    assert m and re.findall(r"^\s*const float\*\s+(\w+);", m.group(1), re.M) == ["prev_bounces", "cur_bounces"]
    assert [f[0] for f in rt._lib.RtSpecPlanes._fields_] == ["prev_bounces", "cur_bounces"]
    assert rt.Accumulator.SPEC_FEATURES == {"guides+spec": 9, "emit+spec": 11}


def test_ctypes_signatures_match_the_header(rt):
    """rt_reproject_clip's argument list with spec directly after copts"""
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    for name in SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert m, name
        names = [p.split()[-1] for p in m.group(1).replace("\n", " ").split(",")]
        assert names[names.index("copts") + 1] in ("spec", "spec_dev")
    for spec, clip in zip(SYMBOLS, ("rt_reproject_clip", "rt_reproject_clip_device")):
        a = rt._lib.SIGNATURES[clip][1]
        assert rt._lib.SIGNATURES[spec][1] == a[:13] + [C.POINTER(rt._lib.RtSpecPlanes)] + a[13:]
    lb = rt._lib
    assert lb.SIGNATURES["rt_accum_set_features_spec"][1] == [C.c_void_p, C.c_uint32, C.POINTER(lb.RtAovSpecOpts)]
    for s in ACCUM[1:]:
        assert lb.SIGNATURES[s][1] == [C.c_void_p, C.POINTER(lb.RtAov), C.POINTER(lb.RtAovSpec)]


class Args(ClipArgs):
    """a valid call's arguments, each replaceable"""

    def __init__(self, rt, mode=LIGHT):
        super().__init__(rt, mode)
        self.keep["bounces"] = np.zeros((2, H, W), np.float32)
        self.spec = rt._lib.RtSpecPlanes(*(self.keep["bounces"][i].ctypes.data for i in (0, 1)))

    def call(self, fn):
        r = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = [self.mode, r(self.cam_prev), r(self.prev), r(self.prev_emit), self.prev_lum2, r(self.cam_cur),
                r(self.cur), r(self.cur_emit), self.w, self.h, r(self.opts), r(self.mopts), r(self.copts), r(self.spec),
                r(self.out), r(self.out_emit), self.out_lum2]
        if fn == "rt_reproject_spec_device":
            args += [0, None]
        return getattr(self.rt.lib(), fn)(*args)


@pytest.mark.parametrize("fn", SYMBOLS)
def test_argument_errors(rt, fn):
    E = rt._lib.RT_ERR_INVALID

    def refused(change, word, mode=LIGHT):
        a = Args(rt, mode)
        change(a)
        assert a.call(fn) == E, rt.lib().rt_last_error()
        assert fn.encode() in rt.lib().rt_last_error() and word in rt.lib().rt_last_error(), rt.lib().rt_last_error()

    for mode in (PLAIN, EMIT, LIGHT):
        refused(lambda a: setattr(a.spec, "cur_bounces", None), b"cur_bounces", mode)
        refused(lambda a: setattr(a.spec, "prev_bounces", None), b"prev_bounces", mode)

        def no_prev_no_cur(a):
            _no_prev(a)
            a.spec.cur_bounces = None
        refused(no_prev_no_cur, b"cur_bounces", mode)
        for which in ("prev_bounces", "cur_bounces"):
            for ok in ("rgb", "var", "count"):
                refused(lambda a, ok=ok, which=which: setattr(a.out, ok, getattr(a.spec, which)), b"bounces plane", mode)
            refused(lambda a, which=which: setattr(a, "out_lum2", getattr(a.spec, which)), b"bounces plane", mode)
        # rt_reproject_clip's refusals are still there, with and without spec
        for spec in (True, False):
            def change(a, f, spec=spec):
                if not spec:
                    a.spec = None
                f(a)
            refused(lambda a: change(a, lambda a: setattr(a.mopts, "radius", -1)), b"window", mode)
            refused(lambda a: change(a, lambda a: setattr(a.copts, "gamma", -1.0)), b"gamma", mode)
            refused(lambda a: change(a, lambda a: setattr(a, "out_lum2", None)), b"null out_lum2", mode)
            refused(lambda a: change(a, lambda a: setattr(a.cur, "depth", None)), b"rgb, normal and depth", mode)
    for which in ("prev_bounces", "cur_bounces"):
        for ok in ("emission", "coverage"):
            refused(lambda a, ok=ok, which=which: setattr(a.out_emit, ok, getattr(a.spec, which)), b"bounces plane")
    for mode in (-1, 3):
        refused(lambda a: None, b"mode", mode)


def test_valid_arguments_reach_the_device(rt):
    """with nothing wrong the call gets past the checks: RT_ERR_DEVICE on a host without a GPU.  So do
    spec == NULL, copts == NULL (also with radius -1), both, and no history at all, where prev_bounces
    is not needed"""
    if rt.device_count() > 0:
        return  # a HIP device is visible: the calls themselves are tests/test_reproject_spec_gpu.py's
    D = rt._lib.RT_ERR_DEVICE

    def null_copts_no_window(a):
        a.copts = None
        a.mopts.radius = -1

    def no_prev_no_prev_bounces(a):
        _no_prev(a)
        a.spec.prev_bounces = None
    changes = [lambda a: None, _no_prev, no_prev_no_prev_bounces, lambda a: setattr(a, "spec", None),
               lambda a: setattr(a, "copts", None), null_copts_no_window,
               lambda a: (setattr(a, "copts", None), setattr(a, "spec", None))]
    for fn in SYMBOLS:
        for mode in (PLAIN, EMIT, LIGHT):
            for change in changes:
                a = Args(rt, mode)
                change(a)
                assert a.call(fn) == D, rt.lib().rt_last_error()
                assert fn.encode() in rt.lib().rt_last_error()


def test_accum_entries_refuse_without_a_device(rt):
    """what can be refused without an accumulator is: a null one, after the checks that need none"""
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    so = rt._lib.RtAovSpecOpts(0, 0.0)
    for planes in (0, 8, 9, 11, 12, 13, 16):
        assert L.rt_accum_set_features_spec(None, planes, C.byref(so)) == E
        assert b"rt_accum_set_features_spec" in L.rt_last_error()
    assert L.rt_accum_set_features(None, 8) == E and b"rt_accum_set_features:" in L.rt_last_error()
    buf = np.zeros((H, W, 3), np.float32)
    a, sp = rt.RtAov(None, buf.ctypes.data, None, None), rt._lib.RtAovSpec(buf.ctypes.data)
    for fn in ACCUM[1:]:
        assert getattr(L, fn)(None, C.byref(a), C.byref(sp)) == E and fn.encode() in L.rt_last_error()


def test_python_wrappers_refuse_what_they_must(rt):
    cam = _cam(rt)
    prev, cur = _moment_frames()
    b = np.zeros((H, W), np.float32)
    for mode in ("plain", "emit", "light"):
        with pytest.raises(ValueError, match=r"cur\['bounces'\]"):
            rt.reproject_spec(mode, cam, dict(prev, bounces=b), cam, cur)
        with pytest.raises(ValueError, match=r"prev\['bounces'\]"):
            rt.reproject_spec(mode, cam, prev, cam, dict(cur, bounces=b))
        with pytest.raises(ValueError, match="shape"):
            rt.reproject_spec(mode, cam, dict(prev, bounces=b), cam, dict(cur, bounces=b[:1]))
    with pytest.raises(ValueError, match="reproject_spec: mode"):
        rt.reproject_spec("surface", cam, prev, cam, cur)
    for kw in (dict(var_radius=-1), dict(gamma=-1.0)):
        with pytest.raises(rt.RtError) as e:
            rt.reproject_spec("emit", cam, dict(prev, bounces=b), cam, dict(cur, count=3, bounces=b), **kw)
        assert e.value.code == rt._lib.RT_ERR_INVALID and b"rt_reproject_spec" in rt.lib().rt_last_error()
    if rt.device_count() == 0:  # past the wrapper's checks, with and without the clamp and the history
        for args, gamma in (((cam, dict(prev, bounces=b)), 0.0), ((None, None), 0.0), ((cam, dict(prev, bounces=b)), None)):
            with pytest.raises(rt.RtError) as e:
                rt.reproject_spec("light", *args, cam, dict(cur, count=3, bounces=b), gamma=gamma)
            assert e.value.code == rt._lib.RT_ERR_DEVICE and b"rt_reproject_spec" in rt.lib().rt_last_error()


def test_temporal_and_accumulator_options(rt):
    with pytest.raises(ValueError, match="moments=True"):
        rt.Temporal(specular=True)
    with pytest.raises(ValueError, match="moments=True"):
        rt.Temporal(split_emitters=True, clip=False, specular=True)
    for kw in ({}, dict(clip=True), dict(split_emitters=True, light_history=True, clip=True, clip_gamma=1.5)):
        assert rt.Temporal(moments=True, specular=True, **kw).light is None
    with pytest.raises(ValueError, match=r"features='guides\+spec' or 'emit\+spec'"):
        rt.Temporal(moments=True, specular=True).push(_Acc())
    with pytest.raises(ValueError, match="guides\\+spec"):
        rt.Accumulator(None, _cam(rt), features="spec")
    with pytest.raises(ValueError, match="spec_bounces and spec_fuzz"):
        rt.Accumulator(None, _cam(rt), features="emit", spec_bounces=2)
