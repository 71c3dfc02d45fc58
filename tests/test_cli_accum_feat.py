"""rtbench -accum-features: the denoiser's and -aov's feature buffers from the accumulator's own
passes, from the command line (child processes with a time limit), against the
same pipeline through the Python wrappers.  The usage error needs no GPU."""
import json

import numpy as np
import pytest

from tests.cli import run
from tests.test_cli_denoise_var import read_p3

SHAPE = ["-S", "6", "-width", "40", "-spp", "4"]


def test_help_lists_the_flag():
    r = run("-h")
    assert r.returncode == 0 and "-accum-features" in r.stderr


@pytest.mark.parametrize("extra", [[], ["-denoise"], ["-denoise", "-split-emitters", "-aov", "P"]])
def test_the_flag_needs_an_accumulator(tmp_path, extra):
    """without -passes / -until / -adaptive there is no accumulator to keep the sums: a usage
    error before anything is rendered or written"""
    out = tmp_path / "f.ppm"
    r = run(*SHAPE, *extra, "-accum-features", "-o", str(out))
    assert r.returncode != 0 and "-accum-features needs -passes" in r.stderr and "Usage of" in r.stderr
    assert not out.exists()


@pytest.mark.gpu
def test_composes_with_adaptive_passes(gpu, tmp_path):
    """active-pixel passes keep the guides too; without -split-emitters only the guides group"""
    out, prefix = tmp_path / "a.ppm", tmp_path / "A"
    r = run(*SHAPE, "-adaptive", "0.05", "-passes", "6", "-denoise-var", "-accum-features", "-aov", str(prefix),
            "-o", str(out))
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])
    assert js["accum_features"] == 1 and "split_emitters" not in js and 4 <= js["passes"] <= 6
    image = read_p3(out)
    assert all(read_p3(tmp_path / f"A_{k}.ppm").shape == image.shape for k in ("albedo", "normal", "depth"))
    assert read_p3(tmp_path / "A_albedo.ppm").max() > 0
    assert not (tmp_path / "A_coverage.ppm").exists()


@pytest.mark.gpu
def test_accum_features_match_the_python_path(rt, gpu, tmp_path):
    out, prefix = tmp_path / "s.ppm", tmp_path / "P"
    r = run(*SHAPE, "-passes", "4", "-denoise-var", "-split-emitters", "-accum-features", "-aov", str(prefix),
            "-o", str(out))
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])
    assert js["accum_features"] == 1 and js["split_emitters"] == 1 and js["denoise_var"] == 1 and js["passes"] == 4
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 40, 4
    with rt.Scene(t, w, l) as sc:
        with sc.accumulator(cam, max_passes=4, features="emit") as acc:
            for seed in (1, 2, 3, 4):
                acc.add(seed)
            rgb, var = acc.resolve()
            aov = acc.resolve_aov()
        separate = sc.render_aov(cam, n_samples=4, seed=1, emit=True)
    image = read_p3(out)
    names = ("albedo", "normal", "depth", "emission", "coverage")
    assert all(read_p3(tmp_path / f"P_{k}.ppm").shape == image.shape for k in names)  # the five feature PPMs
    cov = np.repeat(aov["coverage"][..., None], 3, -1)
    assert (tmp_path / "P_coverage.ppm").read_bytes() == rt.format_ppm(cov)
    assert read_p3(tmp_path / "P_coverage.ppm").max() > 0  # the light is in view
    assert (tmp_path / "P_albedo.ppm").read_bytes() == rt.format_ppm(aov["albedo"])
    assert (tmp_path / "P_emission.ppm").read_bytes() == rt.format_ppm(aov["emission"])
    # four seeds' samples, not one seed's: the rim differs from the separate feature pass
    assert not np.array_equal(aov["coverage"], separate["coverage"])
    assert out.read_bytes() == rt.format_ppm(rt.denoise_var(rgb, var, aov, split_emitters=True, demodulate=True))
