"""What the rtbench tests share: the binary's path, a child process with a time limit, the
statistics line, a P3 reader and the -orbit camera.  A plain module, like tests/scenes.py."""
import json
import math
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "go_raytracer_amd", "rtbench")


def run(*args, cwd=None, timeout=60):
    return subprocess.run([CLI, *args], capture_output=True, text=True, cwd=cwd, timeout=timeout)


def last_json(r, **kw):
    """the statistics line: the last line of a finished run's stderr"""
    return json.loads(r.stderr.strip().splitlines()[-1], **kw)


def read_p3(path, w):
    lines = path.read_text().split("\n")
    assert lines[0] == "P3" and lines[2] == "255" and lines[-1] == ""
    pw, ph = map(int, lines[1].split())
    body = np.array([list(map(int, ln.split())) for ln in lines[3:-1]])
    assert pw == w and body.shape == (pw * ph, 3) and body.min() >= 0 and body.max() <= 255
    return body.reshape(ph, pw, 3)


def orbit(cam, degrees):
    """rtbench's -orbit, operation for operation: look_from turned about the vup axis through
    look_at (Rodrigues' formula) -> a positioned copy of cam"""
    frm, at, up = cam._pos
    th = degrees * math.pi / 180.0
    co, si = math.cos(th), math.sin(th)
    ul = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    k = [up[0] / ul, up[1] / ul, up[2] / ul]
    v = [frm[0] - at[0], frm[1] - at[1], frm[2] - at[2]]
    kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2]
    kxv = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
    out = type(cam).from_c(cam.to_c())
    out.PositionCamera([at[i] + (v[i] * co + kxv[i] * si + k[i] * kv * (1.0 - co)) for i in range(3)], at, up)
    return out
