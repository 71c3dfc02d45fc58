"""rtbench -denoise / -aov: render -> feature pass -> denoise -> PPM from the command line,
in a child process with a time limit."""
import functools
import json
import subprocess

import numpy as np
import pytest

from tests import cli
from tests.cli import CLI

read_p3 = functools.partial(cli.read_p3, w=32)


def test_help_lists_the_flags():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-denoise" in r.stderr and "-aov string" in r.stderr


@pytest.mark.gpu
def test_denoise_and_aov_write_four_ppms(rt, gpu, tmp_path):
    img, pre = tmp_path / "img.ppm", tmp_path / "X"
    common = ["-S", "6", "-width", "32", "-spp", "4", "-seed", "3"]
    r = subprocess.run([CLI, *common, "-denoise", "-aov", str(pre), "-o", str(img)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])  # -denoise prints the statistics line
    assert js["aov_samples"] == 4 and js["ms_aov"] > 0 and js["ms_denoise"] > 0
    den = read_p3(img)
    alb, nrm, dep = (read_p3(tmp_path / f"X_{k}.ppm") for k in ("albedo", "normal", "depth"))
    assert den.shape == alb.shape == nrm.shape == dep.shape
    assert dep.max() == 255 and (dep[..., 0] == dep[..., 1]).all()  # normalised to the maximum
    assert len(np.unique(alb.reshape(-1, 3), axis=0)) >= 3  # white, red, green walls at least
    # the same image as the harness's render -> render_aov -> denoise
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    with rt.Scene(t, w, l) as sc:
        rgb, _ = sc.render(cam, seed=3)
        aov = sc.render_aov(cam, n_samples=4, seed=3)
    assert img.read_bytes() == rt.format_ppm(rt.denoise(rgb, aov))
    assert (tmp_path / "X_albedo.ppm").read_bytes() == rt.format_ppm(aov["albedo"])
    # without -denoise the image is the plain render
    plain = tmp_path / "plain.ppm"
    r = subprocess.run([CLI, *common, "-o", str(plain)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and plain.read_bytes() == rt.format_ppm(rgb)
    assert plain.read_bytes() != img.read_bytes()
