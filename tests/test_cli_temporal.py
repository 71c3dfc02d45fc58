"""rtbench -frames / -orbit / -temporal (DESIGN.md "Temporal reprojection") from the command line
(child processes with a time limit), against the same sequence through Temporal.push in Python.
The usage errors need no GPU."""
import json

import pytest

from tests.cli import orbit, run

SHAPE = ["-S", "6", "-width", "32", "-spp", "4"]


def test_help_lists_the_flags():
    r = run("-h")
    assert r.returncode == 0 and all(f in r.stderr for f in ("-temporal", "-frames int", "-orbit float"))


@pytest.mark.parametrize("extra", [[], ["-passes", "2"], ["-accum-features"], ["-denoise", "-frames", "2"],
                                   ["-until", "0.1", "-denoise-var"]])
def test_temporal_needs_accumulated_features(tmp_path, extra):
    """without -accum-features there are no guides, without an accumulating flag no accumulator:
    a usage error with exit 2 before any file is created"""
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, *extra, "-temporal", "-o", str(out))
    assert r.returncode == 2 and "Usage of" in r.stderr
    assert "-temporal needs -accum-features" in r.stderr or "-accum-features needs -passes" in r.stderr
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("bad", [["-frames", "-1"], ["-frames", "1000"], ["-frames", "x"], ["-orbit", "deg"]])
def test_bad_frame_arguments(tmp_path, bad):
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, *bad, "-o", str(out))
    assert r.returncode == 2 and "Usage of" in r.stderr and list(tmp_path.iterdir()) == []


@pytest.mark.gpu
def test_frames_without_temporal_are_independent(rt, gpu, tmp_path):
    """-frames 2 -orbit 2: two numbered files, frame k the plain render of the turned camera;
    without -frames the -o name is used as it is (covered by the older CLI tests)"""
    out = tmp_path / "f.ppm"
    r = run(*SHAPE, "-frames", "2", "-orbit", "2", "-stats", "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["f_000.ppm", "f_001.ppm"]
    lines = [json.loads(ln) for ln in r.stderr.strip().splitlines()]
    assert [js["frame"] for js in lines] == [0, 1] and "temporal" not in lines[0]
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    with rt.Scene(t, w, l) as sc:
        for k in (0, 1):
            img, _ = sc.render(orbit(cam, 2.0 * k), seed=1)
            assert (tmp_path / f"f_{k:03d}.ppm").read_bytes() == rt.format_ppm(img), k


@pytest.mark.gpu
@pytest.mark.parametrize("denoise", [False, True])
def test_temporal_matches_the_python_path(rt, gpu, tmp_path, denoise):
    """3 frames of 32 x 32, 2 passes x 4 spp each, a 1.5 degree orbit: three PPMs, the last one the
    bytes of the same sequence through Temporal.push (and denoise_var_device)"""
    import torch
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, "-passes", "2", "-accum-features", "-temporal", "-frames", "3", "-orbit", "1.5",
            *(["-denoise-var"] if denoise else []), "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["t_000.ppm", "t_001.ppm", "t_002.ppm"]
    lines = [json.loads(ln) for ln in r.stderr.strip().splitlines()]
    assert [js["frame"] for js in lines] == [0, 1, 2]
    assert all(js["temporal"] == 1 and js["accum_features"] == 1 and js["ms_reproject"] >= 0 for js in lines)
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    temporal = rt.Temporal()
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with sc.accumulator(orbit(cam, 1.5 * k), max_passes=2, features="guides") as acc:
                acc.add(1)
                acc.add(2)
                rgb, var, count = temporal.push(acc)
                img = rgb
                if denoise:  # a new tensor: the history is what was pushed, not what was filtered
                    img = rt.denoise_var_device(rgb, var, acc.resolve_aov_device(), demodulate=True)
                torch.cuda.synchronize()
                assert (tmp_path / f"t_{k:03d}.ppm").read_bytes() == rt.format_ppm(img.cpu().numpy()), k
    assert float(count.max()) > 2.0  # the last frame found history
