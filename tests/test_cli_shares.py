"""rtbench -shares N [-devices a,b,...]: each frame accumulated as N row shares
(rt_accum_add_shares) and pushed with rt_pipeline_push_shares.  The files are the bytes of the same
line without -shares; the flag is valid only with -on-device, and not with -adaptive, -until, -aov or
-counts: those and a malformed -devices exit with status 2 before any file exists."""
import pytest

from tests.cli import last_json, run

LINE = ["-S", "6", "-width", "24", "-spp", "2", "-passes", "1", "-accum-features", "-split-emitters", "-denoise-var",
        "-temporal-emit", "-temporal-moments", "-frames", "3", "-orbit", "1", "-on-device"]
ON_DEVICE = ["-S", "6", "-width", "24", "-spp", "2", "-passes", "1", "-accum-features", "-on-device"]
NEEDS = "-shares needs -on-device"
DEVICES = "invalid value for flag -devices: one non-negative device number per share, a,b,..."


@pytest.mark.parametrize("args,message", [
    (["-S", "6", "-width", "24", "-shares", "3"], NEEDS),
    (["-S", "6", "-width", "24", "-passes", "1", "-accum-features", "-shares", "3"], NEEDS),
    ([*ON_DEVICE, "-shares", "-1"], "invalid value for flag -shares (1..4096)"),
    ([*ON_DEVICE, "-devices", "0,0"], "-devices needs -shares"),
    (["-S", "6", "-width", "24", "-spp", "2", "-accum-features", "-on-device", "-adaptive", "0.1", "-shares", "2"],
     "-shares does not combine with -adaptive or -until"),
    (["-S", "6", "-width", "24", "-spp", "2", "-accum-features", "-on-device", "-until", "0.1", "-shares", "2"],
     "-shares does not combine with -adaptive or -until"),
    ([*ON_DEVICE, "-shares", "2", "-aov", "p"], "-shares does not combine with -aov or -counts"),
    ([*ON_DEVICE, "-shares", "3", "-devices", "0,0"], DEVICES),
    ([*ON_DEVICE, "-shares", "2", "-devices", "0,x"], DEVICES),
    ([*ON_DEVICE, "-shares", "2", "-devices", "0,,1"], DEVICES),
    ([*ON_DEVICE, "-shares", "2", "-devices", "0,-1"], DEVICES),
    ([*ON_DEVICE, "-shares", "2", "-devices", "0,1,"], DEVICES),
])
def test_usage_errors(tmp_path, args, message):
    r = run(*args, "-o", "f.ppm", cwd=tmp_path, timeout=20)
    lines = r.stderr.splitlines()
    assert r.returncode == 2, r
    assert lines[0] == message
    assert lines[1].startswith("Usage of ")
    assert list(tmp_path.iterdir()) == []


@pytest.mark.gpu
def test_the_files_are_the_bytes_of_the_line_without_shares(gpu, tmp_path):
    whole = run(*LINE, "-o", "w.ppm", cwd=tmp_path)
    assert whole.returncode == 0, whole.stderr
    names = [f"_{k:03d}.ppm" for k in range(3)]
    want = [(tmp_path / ("w" + n)).read_bytes() for n in names]
    assert len(set(want)) == 3 and "shares" not in last_json(whole)
    for tag, extra in (("s", ["-shares", "3"]), ("d", ["-shares", "3", "-devices", "0,0,0"]), ("one", ["-shares", "1"])):
        r = run(*LINE, *extra, "-o", tag + ".ppm", cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        assert [(tmp_path / (tag + n)).read_bytes() for n in names] == want, tag
        st = last_json(r)
        assert st["shares"] == int(extra[1]) and st["on_device"] == 1 and st["frame"] == 2
        assert st["samples"] == last_json(whole)["samples"]
        keys = list(st)
        assert keys.index("shares") == keys.index("ms_pipeline") + 1 and keys[-1] == "wall_s"
