"""rt_accum_add_shares and rt_pipeline_push_shares (include/rt_abi.h) on a host without a
GPU: both symbols exist with the header's prototypes, the ABI version is unchanged, and the
arguments that can be refused without looking at an accumulator are refused with RT_ERR_INVALID and
the entry's name in rt_last_error.  None of this touches a device."""
import ctypes as C
import re

import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_accum_add_shares", "rt_pipeline_push_shares")


def test_symbols_and_prototypes(rt):
    lb = rt._lib
    L = C.CDLL(lb.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert rt.lib().rt_abi_version() == 4  # additive: callers detect the feature by the symbols
    text = open(os.path.join(REPO, "include", "rt_abi.h")).read()
    P = C.c_void_p
    by_c = {"rt_accum* const*": C.POINTER(P), "rt_pipeline*": P, "int32_t": C.c_int32, "uint64_t": C.c_uint64,
            "rt_stats*": C.POINTER(lb.RtStats)}
    want = {"rt_accum_add_shares": "rt_accum* const* accs, int32_t n, uint64_t seed, rt_stats* stats",
            "rt_pipeline_push_shares": "rt_pipeline* p, rt_accum* const* accs, int32_t n"}
    for name in SYMBOLS:
        m = re.search(r"^int " + name + r"\(([^)]*)\);", text, re.M)
        assert m and " ".join(m.group(1).split()) == want[name], name
        res, args = lb.SIGNATURES[name]
        types = [p.strip().rsplit(" ", 1)[0].strip() for p in m.group(1).split(",")]
        assert res == C.c_int and [by_c[t] for t in types] == args, name
    assert "AccumulatorShares" in rt.__all__ and hasattr(rt.Scene, "accumulator_shares")


def test_push_shares_refuses_null_and_empty(rt):
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    o = rt._lib.RtPipelineOpts()
    o.temporal, o.filter = 1, rt._lib.RT_PIPE_FILTER_VAR
    p = C.c_void_p()
    assert L.rt_pipeline_create(C.byref(o), C.byref(p)) == 0
    arr = (C.c_void_p * 2)(None, None)
    for args in ((None, arr, 2), (p, None, 2), (p, arr, 0), (p, arr, -1), (p, arr, 2)):
        assert L.rt_pipeline_push_shares(*args) == E, args
        assert b"rt_pipeline_push_shares" in L.rt_last_error(), args
    i = rt._lib.RtPipelineInfo()
    assert L.rt_pipeline_info_get(p, C.byref(i)) == 0
    assert (i.width, i.height, i.device, i.frames, i.allocations, i.device_bytes) == (0, 0, -1, 0, 0, 0)
    assert L.rt_pipeline_destroy(p) == 0
    with rt.Pipeline() as pipe:
        for empty in ([], ()):
            try:
                pipe.push(empty)
            except rt.RtError as e:
                assert e.code == E and "rt_pipeline_push_shares" in str(e)
            else:
                raise AssertionError("an empty list of shares was pushed")


def test_add_shares_refuses_null_and_empty(rt):
    L, E = rt.lib(), rt._lib.RT_ERR_INVALID
    arr = (C.c_void_p * 2)(None, None)
    st = rt._lib.RtStats()
    for args in ((None, 2, 1, None), (arr, 0, 1, None), (arr, -1, 1, C.byref(st)), (arr, 2, 1, None)):
        assert L.rt_accum_add_shares(*args) == E, args
        assert b"rt_accum_add_shares" in L.rt_last_error(), args
