"""rtbench -temporal-specular (DESIGN.md "Temporal history for mirrors") from the command line (child
processes with a time limit), against the same sequence through Temporal(moments=True,
specular=True).push in Python, in the manner of tests/test_cli_temporal_clip.py.  The usage errors
need no GPU."""
import json

import pytest

from tests.cli import orbit, run

SHAPE = ["-S", "5", "-width", "48", "-spp", "4"]      # quads: the fuzz-0 metal quad
EMIT = ["-accum-features", "-split-emitters", "-denoise-var"]
MOMENTS = ["-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments"]


def test_help_lists_the_flag():
    r = run("-h")
    assert r.returncode == 0 and "-temporal-specular" in r.stderr


@pytest.mark.parametrize("extra,word", [
    # a modifier of -temporal-moments
    (["-passes", "2", *EMIT, "-temporal-emit", "-temporal-specular"], "-temporal-specular needs -temporal-moments"),
    (["-temporal-specular"], "-temporal-specular needs -temporal-moments"),
    # its planes are the accumulator's (the first check that fails is reported: without -accum-features
    # -temporal-emit has no planes either, so the stage is spelled through a feature pass's flags)
    (["-passes", "1", "-denoise", "-temporal-moments", "-temporal-specular", "-temporal"], "-temporal-specular needs -accum-features"),
    # a chain traces no media
    ([*MOMENTS, "-temporal-specular", "-aov-media"], "-temporal-specular does not combine with -aov-media"),
    # the limits: the library's ranges, and not without the flag
    ([*MOMENTS, "-temporal-specular", "-spec-bounces", "65"], "-spec-bounces"),
    ([*MOMENTS, "-temporal-specular", "-spec-bounces", "-1"], "-spec-bounces"),
    ([*MOMENTS, "-temporal-specular", "-spec-fuzz", "-0.5"], "-spec-fuzz"),
    ([*MOMENTS, "-temporal-specular", "-spec-fuzz", "nan"], "-spec-fuzz"),
    ([*MOMENTS, "-spec-bounces", "2"], "-spec-bounces and -spec-fuzz need"),
])
def test_usage_refusals_exit_2_before_any_file(tmp_path, extra, word):
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, *extra, "-o", str(out))
    assert r.returncode == 2 and "Usage of" in r.stderr and word in r.stderr, r.stderr[:400]
    assert list(tmp_path.iterdir()) == []


def _python_path(rt, tmp_path, name, features="emit+spec", step=3.0, acc_kw={}, **kw):
    import torch
    t, cam, w, l = rt.demo_scene("quads")
    cam.Width, cam.SamplesPerPixel = 48, 4
    temporal = rt.Temporal(split_emitters=True, moments=True, **kw)
    same = []
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with sc.accumulator(orbit(cam, step * k), max_passes=1, features=features, **acc_kw) as acc:
                acc.add(1)
                rgb, var, count = temporal.push(acc)
                img = rt.denoise_var_device(rgb, var, acc.resolve_aov_device(), split_emitters=True, demodulate=True)
                torch.cuda.synchronize()
                same.append((tmp_path / f"{name}_{k:03d}.ppm").read_bytes() == rt.format_ppm(img.cpu().numpy()))
    assert float(count.max()) > 1.0  # the last frame found history
    return same


@pytest.mark.gpu
def test_one_pass_frames_match_the_python_path(rt, gpu, tmp_path):
    """the issue's command: 3 frames of quads at 48 x 48, ONE pass x 4 spp each, a 3 degree orbit: three
    PPMs, each the bytes of the same sequence through Temporal(split_emitters=True, moments=True,
    specular=True).push and the split variance-guided filter; the flag is in the bytes (the
    non-specular Python path differs) and in the statistics line; -temporal-clip combines"""
    r = run(*SHAPE, *MOMENTS, "-temporal-specular", "-frames", "3", "-orbit", "3", "-o", str(tmp_path / "t.ppm"))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["t_000.ppm", "t_001.ppm", "t_002.ppm"]
    lines = [json.loads(ln) for ln in r.stderr.strip().splitlines()]
    assert [js["frame"] for js in lines] == [0, 1, 2]
    assert all(js["temporal_moments"] == 1 and js["temporal_specular"] == 1 and js["passes"] == 1 for js in lines)
    assert _python_path(rt, tmp_path, "t", specular=True) == [True, True, True]
    assert _python_path(rt, tmp_path, "t", features="emit")[1:] != [True, True]
    r = run(*SHAPE, *MOMENTS, "-temporal-specular", "-temporal-clip", "-spec-bounces", "1", "-spec-fuzz", "0.3",
            "-frames", "3", "-orbit", "3", "-o", str(tmp_path / "c.ppm"))
    assert r.returncode == 0 and r.stderr.count('"temporal_specular": 1') == 3, r.stderr
    assert _python_path(rt, tmp_path, "c", specular=True, clip=True,
                        acc_kw=dict(spec_bounces=1, spec_fuzz=0.3)) == [True, True, True]
    r = run(*SHAPE, *MOMENTS, "-o", str(tmp_path / "m.ppm"))
    assert r.returncode == 0 and "temporal_specular" not in r.stderr
