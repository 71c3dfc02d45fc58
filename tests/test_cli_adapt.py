"""rtbench -adaptive / -counts: adaptive passes from the command line (child processes with a
time limit).  The argument errors need no GPU."""
import json

import numpy as np
import pytest

from tests.cli import run

COMMON = ["-S", "6", "-width", "40", "-spp", "4"]


def test_help_lists_the_flags():
    r = run("-h")
    assert r.returncode == 0 and "-adaptive float" in r.stderr and "-counts string" in r.stderr


def test_bad_values_are_usage_errors(tmp_path):
    for bad, msg in ((["-adaptive", "0"], "the error threshold must be > 0"),
                     (["-adaptive", "-0.5"], "the error threshold must be > 0"),
                     (["-adaptive=nan"], "the error threshold must be > 0"),
                     (["-adaptive", "x"], 'invalid value "x" for flag -adaptive'),
                     (["-adaptive"], "flag needs an argument: -adaptive"),
                     (["-counts", str(tmp_path / "c.ppm")], "-counts needs -adaptive")):
        r = run(*COMMON, "-o", str(tmp_path / "x.ppm"), *bad)
        assert r.returncode == 2 and msg in r.stderr and "Usage of" in r.stderr, bad
    assert not (tmp_path / "c.ppm").exists()


@pytest.mark.gpu
def test_same_bytes_as_python(rt, gpu, tmp_path):
    E = 0.05
    out, cnt_file = tmp_path / "a.ppm", tmp_path / "c.ppm"
    r = run(*COMMON, "-passes", "16", "-adaptive", str(E), "-counts", str(cnt_file), "-stats", "-o", str(out))
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 40, 4
    with rt.Scene(t, w, l) as sc, sc.accumulator(cam, max_passes=16) as acc:
        a = acc.render_adaptive(E, 16, seed=1)  # rtbench's default -seed is 1
        rgb, _ = acc.resolve()
        cnt = acc.counts()
    assert out.read_bytes() == rt.format_ppm(rgb)
    assert js["passes"] == a["passes"] and js["samples_total"] == a["total_samples"] == int(cnt.sum()) * 4
    assert js["samples_full"] == a["passes"] * 4 * cnt.size and js["active_last"] == a["active_pixels"]
    assert js["samples"] == js["samples_total"]  # the passes' own sample counts add up to it
    grey = np.repeat((cnt / cnt.max()).astype(np.float32)[..., None], 3, axis=2)
    assert cnt_file.read_bytes() == rt.format_ppm(grey)
