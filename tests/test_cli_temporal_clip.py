"""rtbench -temporal-clip (DESIGN.md "Clamping the history") from the command line (child processes
with a time limit), against the same sequence through Temporal(moments=True, clip=True).push in
Python, in the manner of tests/test_cli_temporal_moments.py.  The usage errors need no GPU."""
import json

import pytest

from tests.cli import orbit, run
from tests.test_cli_temporal import SHAPE

EMIT = ["-accum-features", "-split-emitters", "-denoise-var"]
MOMENTS = ["-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments"]


def test_help_lists_the_flags():
    r = run("-h")
    assert r.returncode == 0 and all(f in r.stderr for f in ("-temporal-clip", "-clip-gamma float"))


@pytest.mark.parametrize("extra,word", [
    # a modifier of -temporal-moments: without it there is no window to clamp to
    (["-passes", "2", *EMIT, "-temporal-emit", "-temporal-clip"], "-temporal-clip needs -temporal-moments"),
    (["-temporal-clip"], "-temporal-clip needs -temporal-moments"),
    (["-passes", "1", *EMIT, "-temporal-moments", "-temporal-clip"], "-temporal-moments needs -temporal"),
    # its option without it
    ([*MOMENTS, "-clip-gamma", "1.5"], "-clip-gamma needs -temporal-clip"),
    # the library's ranges, refused before anything is rendered
    ([*MOMENTS, "-temporal-clip", "-clip-gamma", "-1"], "-clip-gamma"),
    ([*MOMENTS, "-temporal-clip", "-clip-gamma", "nan"], "-clip-gamma"),
    ([*MOMENTS, "-temporal-clip", "-clip-gamma", "inf"], "-clip-gamma"),
    ([*MOMENTS, "-temporal-clip", "-clip-gamma", "wide"], "-clip-gamma"),
    ([*MOMENTS, "-temporal-clip", "-clip-gamma", "1e-60"], "-clip-gamma"),   # 0 as a float: not the default in disguise
    ([*MOMENTS, "-temporal-clip", "-moments-radius", "-1"], "-temporal-clip needs the window"),
])
def test_usage_refusals_exit_2_before_any_file(tmp_path, extra, word):
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, *extra, "-o", str(out))
    assert r.returncode == 2 and "Usage of" in r.stderr and word in r.stderr, r.stderr[:400]
    assert list(tmp_path.iterdir()) == []


def _python_path(rt, tmp_path, name, **kw):
    """the three frames through Temporal(**kw).push and the split filter -> the PPMs' bytes match"""
    import torch
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    temporal = rt.Temporal(split_emitters=True, moments=True, **kw)
    same = []
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with sc.accumulator(orbit(cam, 1.5 * k), max_passes=1, features="emit") as acc:
                acc.add(1)
                rgb, var, count = temporal.push(acc)
                img = rt.denoise_var_device(rgb, var, acc.resolve_aov_device(), split_emitters=True, demodulate=True)
                torch.cuda.synchronize()
                same.append((tmp_path / f"{name}_{k:03d}.ppm").read_bytes() == rt.format_ppm(img.cpu().numpy()))
    assert float(count.max()) > 1.0  # the last frame found history
    return same


@pytest.mark.gpu
def test_one_pass_frames_match_the_python_path(rt, gpu, tmp_path):
    """3 frames of 32 x 32, ONE pass x 4 spp each, a 1.5 degree orbit: three PPMs, each the bytes
    of the same sequence through Temporal(split_emitters=True, moments=True, clip=True).push and the
    split variance-guided filter; -clip-gamma reaches the library (the Python path with the same
    gamma gives the same bytes, and another gamma does not); without the flag no temporal_clip key"""
    r = run(*SHAPE, *MOMENTS, "-temporal-clip", "-frames", "3", "-orbit", "1.5", "-o", str(tmp_path / "t.ppm"))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["t_000.ppm", "t_001.ppm", "t_002.ppm"]
    lines = [json.loads(ln) for ln in r.stderr.strip().splitlines()]
    assert [js["frame"] for js in lines] == [0, 1, 2]
    assert all(js["temporal_emit"] == 1 and js["temporal_moments"] == 1 and js["temporal_clip"] == 1 and js["passes"] == 1
               for js in lines)
    assert _python_path(rt, tmp_path, "t", clip=True) == [True, True, True]
    assert _python_path(rt, tmp_path, "t")[1:] != [True, True]          # the clamp is in the bytes
    r = run(*SHAPE, *MOMENTS, "-temporal-clip", "-clip-gamma", "0.25", "-frames", "3", "-orbit", "1.5", "-o",
            str(tmp_path / "g.ppm"))
    assert r.returncode == 0 and r.stderr.count('"temporal_clip": 1') == 3, r.stderr
    assert _python_path(rt, tmp_path, "g", clip=True, clip_gamma=0.25) == [True, True, True]
    assert _python_path(rt, tmp_path, "g", clip=True)[1:] != [True, True]   # the default gamma is another
    r = run(*SHAPE, *MOMENTS, "-o", str(tmp_path / "m.ppm"))
    assert r.returncode == 0 and "temporal_clip" not in r.stderr and '"temporal_moments": 1' in r.stderr
