"""rtbench -aov-specular [-spec-bounces N] [-spec-fuzz F]: the -aov planes and the
-denoise guides come from rt_render_aov_spec, the bytes are the Python path's, PREFIX_bounces.ppm
is written over the image maximum, the statistics line says so, and the combinations the entry
does not take are usage errors (exit 2) before any file exists."""
import numpy as np
import pytest

from tests.cli import last_json, run


def test_help_lists_the_flags():
    r = run("-h")
    assert r.returncode == 0 and all(f in r.stderr for f in ("-aov-specular", "-spec-bounces int", "-spec-fuzz float"))


@pytest.mark.parametrize("extra,msg", [
    (["-aov", "feat", "-aov-media"], "-aov-specular does not combine with -aov-media"),
    (["-denoise", "-split-emitters"], "-aov-specular does not combine with -split-emitters"),
    (["-denoise", "-passes", "2", "-accum-features"], "-aov-specular does not combine with -accum-features"),
    (["-denoise-var", "-until", "0.1", "-accum-features"], "-aov-specular does not combine with -accum-features"),
    ([], "-aov-specular needs -aov, -denoise or -denoise-var"),
    (["-aov", "feat", "-spec-bounces", "65"], "invalid value for flag -spec-bounces"),
    (["-aov", "feat", "-spec-bounces", "-1"], "invalid value for flag -spec-bounces"),
    (["-aov", "feat", "-spec-fuzz", "-0.5"], "invalid value for flag -spec-bounces"),
])
def test_refused_combinations_exit_2_and_leave_no_file(tmp_path, extra, msg):
    r = run("-S", "5", "-spp", "4", "-aov-specular", *extra, "-o", "o.ppm", cwd=str(tmp_path))
    assert r.returncode == 2 and "Usage of" in r.stderr, r.stderr
    assert msg in r.stderr
    assert list(tmp_path.iterdir()) == []


def test_spec_limits_need_the_mode(tmp_path):
    for extra in (["-spec-bounces", "3"], ["-spec-fuzz", "0.5"]):
        r = run("-S", "5", "-spp", "4", "-aov", "feat", *extra, "-o", "o.ppm", cwd=str(tmp_path))
        assert r.returncode == 2 and "need -aov-specular" in r.stderr
        assert list(tmp_path.iterdir()) == []


@pytest.mark.gpu
def test_cli_writes_the_python_paths_bytes(rt, gpu, tmp_path):
    """rtbench -S 5 -spp 4 -denoise -aov-specular -aov feat: the image and all five planes"""
    r = run("-S", "5", "-spp", "4", "-denoise", "-aov-specular", "-aov", "feat", "-o", "o.ppm", cwd=str(tmp_path),
            timeout=120)
    assert r.returncode == 0, r.stderr
    js = last_json(r)
    assert js["aov_specular"] == 1 and js["aov_samples"] == 4 and js["scene"] == "quads"
    t, cam, wd, l = rt.demo_scene("quads")
    cam.SamplesPerPixel = 4
    with rt.Scene(t, wd, l) as sc:
        rgb, _ = sc.render(cam, seed=1)
        a = sc.render_aov(cam, n_samples=4, seed=1, specular=True)
        first = sc.render_aov(cam, n_samples=4, seed=1)
    assert a["bounces"].max() > 0 and not np.array_equal(a["depth"], first["depth"])
    grey = lambda p: np.repeat((p / p.max())[..., None], 3, -1)  # noqa: E731
    want = {"albedo": a["albedo"], "normal": a["normal"] * np.float32(0.5) + np.float32(0.5),
            "depth": grey(a["depth"]), "bounces": grey(a["bounces"])}
    for k, img in want.items():
        assert (tmp_path / f"feat_{k}.ppm").read_bytes() == rt.format_ppm(img), k
    assert (tmp_path / "o.ppm").read_bytes() == rt.format_ppm(rt.denoise(rgb, a))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["feat_albedo.ppm", "feat_bounces.ppm", "feat_depth.ppm",
                                                          "feat_normal.ppm", "o.ppm"]
    # the limits are taken at their ends
    r = run("-S", "5", "-spp", "4", "-aov-specular", "-spec-bounces", "64", "-spec-fuzz", "1", "-aov", "g", "-o", "p.ppm",
            cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "g_bounces.ppm").exists()
