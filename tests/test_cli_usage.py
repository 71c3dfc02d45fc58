"""rtbench's argument checks and its statistics line, pinned by the text.

The "flag X needs flag Y" checks run in one order and the first that fails is reported, with the
usage and exit 2, before any file exists; a bad -mode or -passes / -until is found after the
output file was created and prints no usage.  Child processes with a time limit; only the last
test needs a GPU."""
import json

import pytest

from tests.cli import last_json, run

SHAPE = ["-S", "6", "-width", "32", "-spp", "4"]
ADAPTIVE = "invalid value for flag -adaptive: the error threshold must be > 0"
COUNTS = "-counts needs -adaptive"
DENOISE_VAR = "-denoise-var needs -passes N with N >= 2, or -until / -adaptive"
SPLIT = "-split-emitters needs -denoise or -denoise-var"
ACCUM_FEATURES = "-accum-features needs -passes, -until or -adaptive"
TEMPORAL = "-temporal needs -accum-features and -passes, -until or -adaptive"
TEMPORAL_EMIT = "-temporal-emit needs -split-emitters, -accum-features and -passes, -until or -adaptive"
AOV_MEDIA = "-aov-media needs -aov, -denoise, -denoise-var or -accum-features"
FRAMES = "invalid value for flag -frames (0..999) / -orbit"


@pytest.mark.parametrize("args,message", [
    # one per check, in precedence order
    (["-adaptive", "0"], ADAPTIVE),
    (["-counts", "c.ppm"], COUNTS),
    (["-passes", "1", "-denoise-var"], DENOISE_VAR),
    (["-split-emitters"], SPLIT),
    (["-denoise", "-accum-features"], ACCUM_FEATURES),
    (["-passes", "2", "-temporal"], TEMPORAL),
    (["-passes", "2", "-accum-features", "-denoise-var", "-temporal-emit"], TEMPORAL_EMIT),
    (["-aov-media"], AOV_MEDIA),
    (["-frames", "1000"], FRAMES),
    (["-frames", "2", "-orbit", "nan"], FRAMES),
    # two checks violated: the earlier one is reported
    (["-split-emitters", "-accum-features"], SPLIT),
    (["-accum-features", "-temporal"], ACCUM_FEATURES),
    (["-adaptive", "-1", "-counts", "c.ppm", "-frames", "-1"], ADAPTIVE),
])
def test_usage_errors_in_precedence_order(tmp_path, args, message):
    r = run(*SHAPE, *args, "-o", "f.ppm", cwd=tmp_path, timeout=20)
    lines = r.stderr.splitlines()
    assert r.returncode == 2, r
    assert lines[0] == message
    assert lines[1].startswith("Usage of ")
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("args,message", [
    (["-S", "6", "-mode", "bogus"], 'invalid value "bogus" for flag -mode'),
    (["-S", "6", "-width", "8", "-spp", "1", "-passes", "-1"], "invalid value for flag -passes / -until"),
    (["-S", "6", "-width", "8", "-spp", "1", "-until", "nan"], "invalid value for flag -passes / -until"),  # strtod takes nan
])
def test_late_errors_leave_an_empty_file_and_print_no_usage(tmp_path, args, message):
    r = run(*args, "-o", "f", cwd=tmp_path, timeout=20)
    assert r.returncode == 2, r
    assert message in r.stderr and "Usage of" not in r.stderr
    assert [p.name for p in tmp_path.iterdir()] == ["f"] and (tmp_path / "f").stat().st_size == 0


RENDER = ["scene", "width", "height", "spp", "max_depth", "samples", "segments", "ms_render", "samples_per_s", "mode",
          "tree_width", "chunk_samples", "aov_samples", "ms_aov", "ms_denoise"]
ACCUM = ["passes", "rel_error", "ms_accum"]


@pytest.mark.gpu
def test_statistics_line_key_order(gpu, tmp_path):
    """the key order tools and tests parse, recorded from the build before rtbench was split into
    stages: a two-frame accumulating -temporal-emit -denoise-var sequence, and an -adaptive
    -counts -aov -aov-media run"""
    r = run(*SHAPE, "-passes", "2", "-accum-features", "-split-emitters", "-temporal-emit", "-frames", "2", "-orbit", "1.5",
            "-denoise-var", "-stats", "-o", "t.ppm", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(ln, object_pairs_hook=list) for ln in r.stderr.strip().splitlines()]
    assert len(lines) == 2
    for js in lines:
        assert [k for k, _ in js] == RENDER + ACCUM + ["denoise_var", "split_emitters", "accum_features", "frame", "temporal",
                                                       "ms_reproject", "temporal_emit", "wall_s"]
    r = run("-S", "7", "-width", "32", "-spp", "4", "-passes", "16", "-adaptive", "0.05", "-counts", "c.ppm", "-aov", "P",
            "-aov-media", "-stats", "-o", "a.ppm", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert [k for k, _ in last_json(r, object_pairs_hook=list)] == RENDER + ACCUM + [
        "active_last", "samples_total", "samples_full", "aov_media", "wall_s"]
    assert sorted(p.name for p in tmp_path.iterdir()) == [
        "P_albedo.ppm", "P_depth.ppm", "P_normal.ppm", "P_scatter.ppm", "a.ppm", "c.ppm", "t_000.ppm", "t_001.ppm"]
