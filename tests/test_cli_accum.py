"""rtbench -passes / -until: the image as the pass accumulator's mean, from the command line
(child processes with a time limit)."""
import json

import pytest

from tests.cli import run

COMMON = ["-S", "6", "-width", "32", "-spp", "4"]


def test_help_lists_the_flags():
    r = run("-h")
    assert r.returncode == 0 and "-passes int" in r.stderr and "-until float" in r.stderr


def test_bad_values_are_usage_errors(tmp_path):
    for bad in (["-passes", "x"], ["-until", "soon"], ["-until"]):
        r = run(*COMMON, "-o", str(tmp_path / "x.ppm"), *bad)
        assert r.returncode == 2 and "Usage of" in r.stderr, bad


@pytest.mark.gpu
def test_same_bytes_as_python(rt, gpu, tmp_path):
    out = tmp_path / "f.ppm"
    r = run(*COMMON, "-passes", "3", "-stats", "-o", str(out))
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])
    assert js["passes"] == 3 and js["rel_error"] > 0 and js["ms_accum"] > 0
    assert js["samples"] == 3 * 32 * 32 * 4
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    with rt.Scene(t, w, l) as sc, sc.accumulator(cam, max_passes=3) as acc:
        for s in (1, 2, 3):  # rtbench's default -seed is 1
            acc.add(s)
        rgb, _ = acc.resolve()
        assert js["rel_error"] == pytest.approx(acc.info()["rel_error"], rel=1e-5)  # printed with %.6g
    assert out.read_bytes() == rt.format_ppm(rgb)


@pytest.mark.gpu
def test_unchanged_when_off_and_until_stops_early(gpu, tmp_path):
    plain, one, until = tmp_path / "plain.ppm", tmp_path / "one.ppm", tmp_path / "until.ppm"
    assert run(*COMMON, "-seed", "7", "-o", str(plain)).returncode == 0
    assert run(*COMMON, "-seed", "7", "-passes", "1", "-o", str(one)).returncode == 0
    assert plain.read_bytes() == one.read_bytes() and len(plain.read_bytes()) > 32 * 32 * 6
    # a target any image meets: stops at the first check, after the second pass
    r = run(*COMMON, "-seed", "7", "-until", "1e9", "-stats", "-o", str(until))
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stderr.strip().splitlines()[-1])["passes"] == 2
    assert until.read_bytes() != plain.read_bytes()
