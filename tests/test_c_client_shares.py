"""examples/orbit_shares_c99.c, orbit_c99.c's moving camera with every frame held as three row shares
(DESIGN.md §25), built as strict C99 against include/rt_abi.h and librt_amd.so: the header's shares
section is valid C, rt_accum_add_shares and rt_pipeline_push_shares link from C, and (GPU) the three
PPMs the client writes are the bytes rt.Pipeline gives for whole accumulators of the harness's Cornell
scene, the same cameras and the same seeds."""
import json
import os
import shutil
import subprocess

import pytest

from tests.cli import orbit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "go_raytracer_amd")
SRC = os.path.join(REPO, "examples", "orbit_shares_c99.c")
W, SEED, DEGREES = 37, 5, 1.0


@pytest.fixture(scope="module")
def client(rt, tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    exe = str(tmp_path_factory.mktemp("cshares") / "orbit_shares_c99")
    subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-L", LIBDIR, "-lrt_amd", "-lm",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def test_the_client_is_strict_c99_and_checks_its_arguments(client, tmp_path):
    p = subprocess.run([client], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 2 and "usage:" in p.stderr and list(tmp_path.iterdir()) == []


@pytest.mark.gpu
def test_the_clients_frames_are_the_whole_accumulators(rt, gpu, client, tmp_path):
    p = subprocess.run([client, str(W), str(SEED), str(DEGREES), str(tmp_path / "f")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [json.loads(ln) for ln in p.stdout.strip().splitlines()]
    assert [ln["frame"] for ln in lines] == [0, 1, 2] and [ln["had_history"] for ln in lines] == [0, 1, 1]
    assert [ln["shares"] for ln in lines] == [3, 3, 3] and [ln["rows"] for ln in lines] == [lines[0]["height"]] * 3
    assert lines[2]["allocations"] == lines[1]["allocations"] > lines[0]["allocations"]
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    with rt.Scene(t, w, l) as sc, rt.Pipeline(split_emitters=True, moments=True) as pipe:
        for k in range(3):
            with sc.accumulator(orbit(cam, DEGREES * k), max_passes=1, features="emit") as acc:
                acc.add(SEED + k)
                want = pipe.push(acc).ppm()
            got = (tmp_path / f"f_{k:03d}.ppm").read_bytes()
            assert got == want and len(got) == lines[k]["ppm_bytes"], k
            assert got.startswith(b"P3\n%d %d\n255\n" % (lines[k]["width"], lines[k]["height"]))
