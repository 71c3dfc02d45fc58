"""rtbench -denoise-var: the accumulator's mean through the variance-guided filter, from the
command line (child processes with a time limit)."""
import functools
import json
import os

import pytest

from tests import cli
from tests.cli import REPO, run

GOLDEN = os.path.join(REPO, "tests", "golden", "cli_passes3_denoise_cornell40.ppm")
COMMON = ["-S", "6", "-width", "40", "-spp", "4"]

read_p3 = functools.partial(cli.read_p3, w=40)


def test_help_lists_the_flag():
    r = run("-h")
    assert r.returncode == 0 and "-denoise-var" in r.stderr


@pytest.mark.parametrize("extra", [[], ["-passes", "1"], ["-passes", "1", "-until", "0.5"], ["-denoise"]])
def test_needs_passes(tmp_path, extra):
    """no variance without a second pass: a usage error before anything is rendered or written"""
    out = tmp_path / "f.ppm"
    r = run(*COMMON, *extra, "-denoise-var", "-o", str(out))
    assert r.returncode != 0 and "-denoise-var needs -passes" in r.stderr
    assert not out.exists()


@pytest.mark.gpu
def test_writes_a_filtered_image_and_the_statistics(gpu, tmp_path):
    plain, var, until = tmp_path / "plain.ppm", tmp_path / "var.ppm", tmp_path / "until.ppm"
    assert run(*COMMON, "-passes", "3", "-o", str(plain)).returncode == 0
    r = run(*COMMON, "-passes", "3", "-denoise-var", "-o", str(var))
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])  # -denoise-var prints the statistics line
    assert js["denoise_var"] == 1 and js["passes"] == 3 and js["aov_samples"] == 4
    assert js["ms_aov"] > 0 and js["ms_denoise"] > 0
    a, b = read_p3(plain), read_p3(var)
    assert a.shape == b.shape and (a != b).any()
    # composes with -until, -aov, -progress and -stats
    r = run(*COMMON, "-until", "1e9", "-denoise-var", "-aov", str(tmp_path / "X"), "-progress", "-stats",
            "-o", str(until))
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stderr.strip().splitlines()[-1])
    assert js["denoise_var"] == 1 and js["passes"] == 2 and "2 passes" in r.stderr
    assert read_p3(until).shape == a.shape
    assert all(read_p3(tmp_path / f"X_{k}.ppm").shape == a.shape for k in ("albedo", "normal", "depth"))


@pytest.mark.gpu
def test_plain_denoise_is_unchanged(gpu, tmp_path):
    """-passes 3 -denoise writes the bytes the build before -denoise-var wrote (recorded from
    that build on an MI355X); its statistics line has no denoise_var"""
    out = tmp_path / "f.ppm"
    r = run(*COMMON, "-passes", "3", "-denoise", "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert "denoise_var" not in r.stderr
    with open(GOLDEN, "rb") as f:
        assert out.read_bytes() == f.read()
