"""bench.py's contract line, in both multi-GPU drivers' shapes (small workloads).

The single-process mode (--devices, rt_render_multi: the north_star's Go-host path) is
rehearsed on one GPU with two shares on device 0; torchrun's one-process-per-GPU mode
needs distinct GPUs (RCCL) and is covered by tests/test_distributed.py with gloo.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--scene", "cornell", "--width", "160", "--spp", "64", "--steps", "2", "--warmup", "1",
         "--no-cpu-baseline", "--no-extra-configs"]


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *SMALL, *args],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    return p


def test_devices_mode_rejects_mismatched_count():
    p = _bench("--gpus", "3", "--devices", "0,0")
    assert p.returncode != 0 and "--devices must list --gpus devices" in p.stderr


@pytest.mark.gpu
def test_devices_mode_line(gpu):
    p = _bench("--gpus", "2", "--devices", "0,0")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1  # distinct devices: both shares ran on device 0
    assert "rt_render_multi" in line["config"]["parallelism"]
    assert line["value"] > 0 and line["steps"] == 2
    assert line["roofline"]["launches"] == 2


@pytest.mark.gpu
def test_devices_mode_rccl_gather_line(gpu):
    """--gather rccl: the shares collected by one ncclGather (RT_FLAG_GATHER_RCCL); on a
    one-GPU box the device list is [0] (RCCL needs distinct devices)."""
    p = _bench("--gpus", "1", "--devices", "0", "--gather", "rccl")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert "rccl gather" in line["config"]["parallelism"]
    assert line["value"] > 0 and line["steps"] == 2


def test_steps_must_be_positive():
    p = _bench("--steps", "0")
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(rt, gpu, tmp_path):
    """A plain run prints the headline only (nothing of --full) and --dump-outputs writes
    what the last timed step returned: the image equals the harness render of the same
    scene, camera and seed bit for bit, and stats.npy holds that render's counters."""
    import numpy as np
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                        "--scene", "cornell", "--width", "160", "--spp", "64", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 3 and line["roofline"]["launches"] == 3
    assert line["ms_per_step"] > 0 and line["unit"] == "Msamples/s" and line["dtype"] == "f32"
    samples = 160 * 160 * 64
    assert line["value"] == pytest.approx(samples / line["ms_per_step"] / 1e3, rel=1e-3)
    for k in ("extra_configs", "cpu_baseline", "speedup_vs_cpu", "checks"):
        assert k not in line
    assert "ppm_on_device_s" not in line["wall_clock"]
    assert sorted(f.name for f in out.iterdir()) == ["image.npy", "stats.npy"]
    img, st = np.load(out / "image.npy"), np.load(out / "stats.npy")
    assert img.dtype == np.float32 and img.shape == (160, 160, 3) and st.dtype == np.float64
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = 160, 64
    with rt.Scene(t, w, l) as sc:
        ref, rst = sc.render(cam, seed=1)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert list(st) == [rst["samples"], rst["segments"], rst["rows"]] and st[0] == samples


@pytest.mark.gpu
def test_full_line_keeps_the_moved_fields(gpu):
    """--full runs what a plain run leaves out (here with the long legs switched off: the
    on-device PPM timing stays, and the CPU baseline's slot is in the line)."""
    p = _bench("--gpus", "1", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["wall_clock"]["ppm_bytes"] > 0 and line["wall_clock"]["ppm_on_device_s"] >= 0
    assert "cpu_baseline" in line and line["cpu_baseline"] is None
    assert line["value"] > 0 and line["steps"] == 2


def test_gather_option_rejects_unknown():
    p = _bench("--gather", "nccl-allgather")
    assert p.returncode != 0 and "invalid choice" in p.stderr


@pytest.mark.gpu
def test_multi_device_check_child_mode(gpu):
    """bench.py's distinct-device check (run by rank 0 of a torchrun job on a multi-GPU
    node) in its child-process mode; on one GPU the device list is [0]."""
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--multi-device-check",
                        "1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["devices"] == [0]
    for k in ("peer", "peer_reversed", "rccl"):
        assert res[k]["bitwise"], res
