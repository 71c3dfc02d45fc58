"""rtbench -temporal-moments (DESIGN.md "Luminance moments") from the command line (child processes
with a time limit), against the same sequence through Temporal(moments=True).push in Python, in
the manner of tests/test_cli_temporal_emit.py.  The usage errors need no GPU."""
import json

import pytest

from tests.cli import orbit, run
from tests.test_cli_temporal import SHAPE

EMIT = ["-accum-features", "-split-emitters", "-denoise-var"]


def test_help_lists_the_flags_and_an_example():
    r = run("-h")
    assert r.returncode == 0
    assert all(f in r.stderr for f in ("-temporal-moments", "-moments-frames", "-moments-radius"))
    assert "-passes 1 -accum-features -split-emitters -denoise-var -temporal-emit -temporal-moments" in r.stderr


@pytest.mark.parametrize("extra,word", [
    # a modifier of -temporal, -temporal-emit or -temporal-light: alone it modifies nothing
    (["-passes", "1", *EMIT, "-temporal-moments"], "-temporal-moments needs -temporal"),
    (["-passes", "2", *EMIT, "-temporal-moments"], "-temporal-moments needs -temporal"),
    (["-temporal-moments"], "-temporal-moments needs -temporal"),
    # its options without it
    (["-passes", "2", *EMIT, "-temporal-emit", "-moments-frames", "3"], "need -temporal-moments"),
    (["-passes", "2", *EMIT, "-temporal-emit", "-moments-radius", "2"], "need -temporal-moments"),
    # the library's ranges, refused before anything is rendered
    (["-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments", "-moments-radius", "9"], "-moments-radius"),
    (["-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments", "-moments-radius", "-2"], "-moments-radius"),
    (["-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments", "-moments-frames", "1.5"], "-moments-frames"),
    (["-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments", "-moments-frames", "-4"], "-moments-frames"),
    # one pass still has no variance without the moments
    (["-passes", "1", *EMIT, "-temporal-emit"], "-denoise-var needs -passes N with N >= 2"),
    # the stage's own needs stand
    (["-passes", "1", "-split-emitters", "-denoise-var", "-temporal-emit", "-temporal-moments"], "-temporal-emit needs"),
])
def test_usage_refusals_exit_2_before_any_file(tmp_path, extra, word):
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, *extra, "-o", str(out))
    assert r.returncode == 2 and "Usage of" in r.stderr and word in r.stderr, r.stderr[:400]
    assert list(tmp_path.iterdir()) == []


@pytest.mark.gpu
def test_one_pass_frames_match_the_python_path(rt, gpu, tmp_path):
    """3 frames of 32 x 32, ONE pass x 4 spp each, a 1.5 degree orbit: three PPMs, each the bytes
    of the same sequence through Temporal(split_emitters=True, moments=True).push and the split
    variance-guided filter"""
    import torch
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, "-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments", "-frames", "3", "-orbit", "1.5", "-o",
            str(out))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["t_000.ppm", "t_001.ppm", "t_002.ppm"]
    lines = [json.loads(ln) for ln in r.stderr.strip().splitlines()]
    assert [js["frame"] for js in lines] == [0, 1, 2]
    assert all(js["temporal"] == 1 and js["temporal_emit"] == 1 and js["temporal_moments"] == 1 and js["passes"] == 1
               and js["denoise_var"] == 1 for js in lines)
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    temporal = rt.Temporal(split_emitters=True, moments=True)
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with sc.accumulator(orbit(cam, 1.5 * k), max_passes=1, features="emit") as acc:
                acc.add(1)
                rgb, var, count = temporal.push(acc)
                assert float((var > 0).float().mean()) > 0.5   # frame 0 included: the filter has something to go by
                img = rt.denoise_var_device(rgb, var, acc.resolve_aov_device(), split_emitters=True, demodulate=True)
                torch.cuda.synchronize()
                assert (tmp_path / f"t_{k:03d}.ppm").read_bytes() == rt.format_ppm(img.cpu().numpy()), k
    assert float(count.max()) > 1.0  # the last frame found history


@pytest.mark.gpu
def test_options_and_the_other_stages(rt, gpu, tmp_path):
    """-moments-frames and -moments-radius reach the library (the Python path with the same
    options gives the same bytes), -temporal and -temporal-light take the modifier too, and
    without it no temporal_moments key appears"""
    import torch
    r = run(*SHAPE, "-passes", "1", "-accum-features", "-denoise-var", "-temporal", "-temporal-moments",
            "-moments-frames", "2", "-moments-radius", "1", "-frames", "3", "-orbit", "1.5", "-o", str(tmp_path / "p.ppm"))
    assert r.returncode == 0 and r.stderr.count('"temporal_moments": 1') == 3 and "temporal_emit" not in r.stderr, r.stderr
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    temporal = rt.Temporal(moments=True, min_frames=2.0, var_radius=1)
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with sc.accumulator(orbit(cam, 1.5 * k), max_passes=1, features="guides") as acc:
                acc.add(1)
                rgb, var, count = temporal.push(acc)
                img = rt.denoise_var_device(rgb, var, acc.resolve_aov_device(), demodulate=True)
                torch.cuda.synchronize()
                assert (tmp_path / f"p_{k:03d}.ppm").read_bytes() == rt.format_ppm(img.cpu().numpy()), k
    r = run(*SHAPE, "-passes", "1", *EMIT, "-temporal-light", "-temporal-moments", "-frames", "2", "-orbit", "1.5", "-o",
            str(tmp_path / "l.ppm"))
    assert r.returncode == 0 and r.stderr.count('"temporal_moments": 1') == 2 and '"temporal_light": 1' in r.stderr
    r = run(*SHAPE, "-passes", "2", *EMIT, "-temporal-emit", "-o", str(tmp_path / "e.ppm"))
    assert r.returncode == 0 and "temporal_moments" not in r.stderr and '"temporal_emit": 1' in r.stderr
