"""rtbench -temporal-light (DESIGN.md "Light history") from the command line (child processes with a
time limit), against the same sequence through Temporal(split_emitters=True, light_history=True)
.push in Python, in the manner of tests/test_cli_temporal_emit.py.  The usage errors need no GPU."""
import json

import pytest

from tests.cli import orbit, run
from tests.test_cli_temporal import SHAPE

NEEDS = "-temporal-light needs -split-emitters, -accum-features and -passes, -until or -adaptive, and neither"
FULL = ["-passes", "2", "-accum-features", "-split-emitters", "-denoise-var"]


def test_help_lists_the_flag():
    r = run("-h")
    assert r.returncode == 0 and "-temporal-light" in r.stderr


@pytest.mark.parametrize("extra", [[], ["-passes", "2"], ["-passes", "2", "-accum-features"],
                                   ["-passes", "2", "-accum-features", "-denoise-var"],
                                   ["-passes", "2", "-split-emitters", "-denoise-var"],
                                   ["-accum-features", "-split-emitters", "-denoise"]])
def test_temporal_light_needs_the_accumulated_emit_planes(tmp_path, extra):
    """what -temporal-emit needs: a usage error with exit 2 before any file is created"""
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, *extra, "-temporal-light", "-o", str(out))
    assert r.returncode == 2 and "Usage of" in r.stderr
    assert (NEEDS in r.stderr or "-accum-features needs -passes" in r.stderr
            or "-split-emitters needs -denoise" in r.stderr)
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("other", [["-temporal"], ["-temporal-emit"], ["-temporal", "-temporal-emit"]])
def test_temporal_light_excludes_the_other_temporal_stages(tmp_path, other):
    r = run(*SHAPE, *FULL, *other, "-temporal-light", "-o", str(tmp_path / "t.ppm"))
    assert r.returncode == 2 and "Usage of" in r.stderr and NEEDS in r.stderr
    assert list(tmp_path.iterdir()) == []


@pytest.mark.gpu
@pytest.mark.parametrize("filt", ["-denoise-var", "-denoise"])
def test_temporal_light_matches_the_python_path(rt, gpu, tmp_path, filt):
    """3 frames of 32 x 32, 2 passes x 4 spp each, a 1.5 degree orbit: three PPMs, each the bytes
    of the same sequence through Temporal(split_emitters=True, light_history=True).push and the
    split filter given temporal.light's planes"""
    import torch
    out = tmp_path / "t.ppm"
    r = run(*SHAPE, "-passes", "2", "-accum-features", "-split-emitters", "-temporal-light", "-frames", "3", "-orbit",
            "1.5", filt, "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["t_000.ppm", "t_001.ppm", "t_002.ppm"]
    lines = [json.loads(ln) for ln in r.stderr.strip().splitlines()]
    assert [js["frame"] for js in lines] == [0, 1, 2]
    assert all(js["temporal"] == 1 and js["temporal_light"] == 1 and "temporal_emit" not in js
               and js["split_emitters"] == 1 and js["accum_features"] == 1 and js["ms_reproject"] >= 0 for js in lines)
    keys = list(lines[-1])
    assert keys[keys.index("ms_reproject") + 1] == "temporal_light" and keys[-1] == "wall_s"
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 32, 4
    temporal = rt.Temporal(split_emitters=True, light_history=True)
    moved = False
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with sc.accumulator(orbit(cam, 1.5 * k), max_passes=2, features="emit") as acc:
                acc.add(1)
                acc.add(2)
                rgb, var, count = temporal.push(acc)
                own = acc.resolve_aov_device()
                aov = dict(own, **temporal.light)
                moved = moved or not torch.equal(own["coverage"], temporal.light["coverage"])
                # a new tensor: the history is what was pushed, not what was filtered
                img = (rt.denoise_var_device(rgb, var, aov, split_emitters=True, demodulate=True) if filt == "-denoise-var"
                       else rt.denoise_device(rgb, aov, split_emitters=True))
                torch.cuda.synchronize()
                assert (tmp_path / f"t_{k:03d}.ppm").read_bytes() == rt.format_ppm(img.cpu().numpy()), k
    assert float(count.max()) > 2.0 and moved  # the last frame found history, and the rim's coverage was blended
    # the other stages are unchanged: no temporal_light key
    r = run(*SHAPE, "-passes", "2", "-accum-features", "-split-emitters", "-denoise-var", "-temporal-emit", "-o",
            str(tmp_path / "p.ppm"))
    assert r.returncode == 0 and "temporal_light" not in r.stderr and '"temporal_emit": 1' in r.stderr
