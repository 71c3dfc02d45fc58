"""rtbench -split-emitters: the split feature pass and the split filter from the command line
(child processes with a time limit), against the same pipeline through the Python wrappers."""
import json

import numpy as np
import pytest

from tests.cli import run
from tests.test_cli_denoise_var import read_p3

pytestmark = pytest.mark.gpu

COMMON = ["-S", "6", "-width", "40", "-spp", "4", "-passes", "4", "-denoise-var"]


_py = {}


def python_path(rt):
    """(split ppm, unsplit ppm, aov): Cornell 40 wide, 4 passes x 4 spp of seeds 1 .. 4, the
    feature pass at 4 samples of seed 1, the variance-guided filter demodulated; computed once"""
    if not _py:
        t, cam, w, l = rt.demo_scene("cornell")
        cam.Width, cam.SamplesPerPixel = 40, 4
        with rt.Scene(t, w, l) as sc:
            with sc.accumulator(cam, max_passes=4) as acc:
                for seed in (1, 2, 3, 4):
                    acc.add(seed)
                rgb, var = acc.resolve()
            aov = sc.render_aov(cam, n_samples=4, seed=1, emit=True)
        split = rt.denoise_var(rgb, var, aov, split_emitters=True, demodulate=True)
        plain = rt.denoise_var(rgb, var, aov, demodulate=True)
        _py.update(split=rt.format_ppm(split), plain=rt.format_ppm(plain), aov=aov)
    return _py


def test_split_emitters_matches_the_python_path(rt, gpu, tmp_path):
    out, prefix = tmp_path / "s.ppm", tmp_path / "P"
    r = run(*COMMON, "-split-emitters", "-aov", str(prefix), "-o", str(out))
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])
    assert js["split_emitters"] == 1 and js["denoise_var"] == 1 and js["passes"] == 4 and js["aov_samples"] == 4
    py = python_path(rt)
    assert out.read_bytes() == py["split"]
    assert py["split"] != py["plain"]
    aov = py["aov"]
    cov = np.repeat(aov["coverage"][..., None], 3, -1)
    assert (tmp_path / "P_emission.ppm").read_bytes() == rt.format_ppm(aov["emission"])
    assert (tmp_path / "P_coverage.ppm").read_bytes() == rt.format_ppm(cov)
    assert read_p3(tmp_path / "P_coverage.ppm").max() > 0  # the light is in view
    assert (tmp_path / "P_albedo.ppm").read_bytes() == rt.format_ppm(aov["albedo"])


def test_without_the_flag_nothing_changes(rt, gpu, tmp_path):
    out, prefix = tmp_path / "p.ppm", tmp_path / "Q"
    r = run(*COMMON, "-aov", str(prefix), "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert "split_emitters" not in r.stderr
    assert out.read_bytes() == python_path(rt)["plain"]
    assert not (tmp_path / "Q_emission.ppm").exists() and not (tmp_path / "Q_coverage.ppm").exists()
    assert (tmp_path / "Q_albedo.ppm").exists()
