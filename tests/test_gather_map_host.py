"""rt_gather_map.h, the plane table and row map of rt_pipeline_push_shares' gather, checked
on the host: tests/gather_map_check.cpp built with the address and undefined-behaviour sanitizers and
run as a program of its own.  For every H in 1..40 and n in 1..min(H, 9) it shows that every image row
is mapped exactly once and every offset is inside the buffer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_map_and_offsets(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.fail("no C++ compiler for the host check")
    exe = tmp_path / "gather_map_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "go_raytracer_amd", "csrc"),
                    os.path.join(REPO, "tests", "gather_map_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("gather map ok:"), r.stdout
