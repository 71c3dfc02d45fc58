"""rtbench -on-device: the temporal stage, the filter and the image's text through one rt_pipeline
instead of the host entries.  The files are the same bytes as without the flag, the statistics line
says so, and the flag without an accumulator's feature planes is a usage error before any file
exists."""
import json

import pytest

from tests.cli import run

SHAPE = ["-S", "6", "-width", "37", "-spp", "4"]
EMIT = ["-accum-features", "-split-emitters", "-denoise-var"]
SETS = {
    "temporal": ["-passes", "2", "-accum-features", "-denoise-var", "-temporal"],
    "emit+moments": ["-passes", "1", *EMIT, "-temporal-emit", "-temporal-moments"],
    "light+moments+clip": ["-passes", "1", *EMIT, "-temporal-light", "-temporal-moments", "-temporal-clip"],
}


def test_help_lists_the_flag():
    r = run("-h")
    assert r.returncode == 0 and "-on-device" in r.stderr and "rt_pipeline" in r.stderr


@pytest.mark.parametrize("extra,word", [
    ([], "-on-device needs -accum-features"),
    (["-passes", "2"], "-on-device needs -accum-features"),
    (["-denoise"], "-on-device needs -accum-features"),
    (["-passes", "2", "-denoise", "-aov", "P"], "-on-device needs -accum-features"),
    (["-passes", "2", "-accum-features", "-aov-media"], "-on-device does not combine with -aov-media"),
    # the other flags' own needs stand, and come first
    (["-accum-features"], "-accum-features needs -passes"),
    (["-passes", "1", "-accum-features", "-denoise-var"], "-denoise-var needs -passes N with N >= 2"),
])
def test_a_bad_combination_exits_2_before_any_file(tmp_path, extra, word):
    r = run(*SHAPE, *extra, "-on-device", "-frames", "2", "-o", str(tmp_path / "t.ppm"))
    assert r.returncode == 2 and "Usage of" in r.stderr and r.stderr.startswith(word), r.stderr[:300]
    assert list(tmp_path.iterdir()) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETS))
def test_the_frames_are_the_host_paths_bytes(gpu, tmp_path, name):
    """3 frames of 37 x 37, a 1-degree orbit, with and without the flag"""
    frames = ["-frames", "3", "-orbit", "1"]
    host = run(*SHAPE, *SETS[name], *frames, "-o", str(tmp_path / "h.ppm"))
    dev = run(*SHAPE, *SETS[name], *frames, "-on-device", "-o", str(tmp_path / "d.ppm"))
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr, dev.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"{p}_{k:03d}.ppm" for p in "dh" for k in range(3)]
    for k in range(3):
        h, d = ((tmp_path / f"{p}_{k:03d}.ppm").read_bytes() for p in "hd")
        assert h == d and h.startswith(b"P3\n37 37\n255\n"), k
    assert (tmp_path / "h_000.ppm").read_bytes() != (tmp_path / "h_002.ppm").read_bytes()
    hs, ds = ([json.loads(ln, object_pairs_hook=list) for ln in r.stderr.strip().splitlines()] for r in (host, dev))
    assert len(hs) == len(ds) == 3
    for h, d in zip(hs, ds):
        # the same keys in the same order, with the two new ones in front of wall_s
        assert [k for k, _ in d] == [k for k, _ in h][:-1] + ["on_device", "ms_pipeline", "wall_s"]
        d, h = dict(d), dict(h)
        assert d["on_device"] == 1 and d["ms_pipeline"] > 0 and d["ms_reproject"] == 0 and d["ms_denoise"] == 0
        assert "on_device" not in h and h["ms_reproject"] > 0 and h["ms_denoise"] > 0
        assert all(d[k] == h[k] for k in ("frame", "passes", "samples", "segments", "rel_error", "temporal"))


@pytest.mark.gpu
def test_aov_and_the_unfiltered_run_keep_working(gpu, tmp_path):
    """-aov still goes through the host resolves; without a filter or a history the flag still
    writes the accumulator's mean"""
    common = [*SHAPE, "-passes", "2", "-accum-features", "-split-emitters", "-denoise-var", "-temporal-emit"]
    host = run(*common, "-aov", str(tmp_path / "H"), "-o", str(tmp_path / "h.ppm"))
    dev = run(*common, "-aov", str(tmp_path / "D"), "-on-device", "-o", str(tmp_path / "d.ppm"))
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr, dev.stderr)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted(["h.ppm", "d.ppm"] + [f"{p}_{s}.ppm" for p in "HD" for s in
                                                 ("albedo", "normal", "depth", "emission", "coverage")])
    assert (tmp_path / "h.ppm").read_bytes() == (tmp_path / "d.ppm").read_bytes()
    for s in ("albedo", "normal", "depth", "emission", "coverage"):
        assert (tmp_path / f"H_{s}.ppm").read_bytes() == (tmp_path / f"D_{s}.ppm").read_bytes(), s
    bare = [*SHAPE, "-passes", "2", "-accum-features"]
    host = run(*bare, "-o", str(tmp_path / "b.ppm"))
    dev = run(*bare, "-on-device", "-o", str(tmp_path / "c.ppm"))
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr, dev.stderr)
    assert (tmp_path / "b.ppm").read_bytes() == (tmp_path / "c.ppm").read_bytes()
    assert '"on_device": 1' in dev.stderr
