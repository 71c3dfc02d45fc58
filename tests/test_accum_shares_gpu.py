"""Row shares of the accumulator: the ground rt_pipeline_push_shares' bit claim stands
on, and rt_accum_add_shares.

The precondition: share i of n, given the same seeds, resolves to rows i::n of the whole accumulator
bit for bit, in every plane the pipeline asks for: resolve(), resolve_aov() and resolve_aov_spec().
24 x 17 with n = 3 has a short last share; 131 x 5 with n = 2 and n = 5 has shares of 3 + 2 rows and of
one row each.  Two passes of 4 spp, so the variance is not zero."""
import numpy as np
import pytest
import torch  # noqa: F401  before the library's HIP runtime initialises (one runtime per process)

pytestmark = pytest.mark.gpu
SEEDS = (3, 104)
CASES = [("cornell", "emit"), ("quads", "emit+spec")]
SHAPES = [((24, 17), 3), ((131, 5), 2), ((131, 5), 5)]


def camera(rt, scene, size):
    t, cam, w, l = rt.demo_scene(scene)
    cam.Width, cam.SamplesPerPixel, cam.AspectRatio = size[0], 4, size[0] / size[1]
    d = cam.derived()
    assert (d.width, d.height) == size
    return t, cam, w, l


def planes(acc):
    """every plane the accumulator resolves, by name"""
    rgb, var = acc.resolve()
    out = {"rgb": rgb, "var": var}
    out.update({"aov." + k: v for k, v in acc.resolve_aov().items()})
    if str(acc.features).endswith("+spec"):
        out.update({"spec." + k: v for k, v in acc.resolve_aov_spec().items()})
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


_WHOLE = {}


def whole(rt, scene, features, size):
    """the whole accumulator's planes and its passes' summed samples, computed once"""
    if (scene, size) not in _WHOLE:
        t, cam, w, l = camera(rt, scene, size)
        with rt.Scene(t, w, l) as sc, sc.accumulator(cam, max_passes=2, features=features) as acc:
            samples = sum(acc.add(s)["samples"] for s in SEEDS)
            _WHOLE[scene, size] = planes(acc), samples
    return _WHOLE[scene, size]


@pytest.mark.parametrize("size,n", SHAPES)
@pytest.mark.parametrize("scene,features", CASES)
def test_a_share_resolves_to_its_rows_of_the_whole(rt, gpu, scene, features, size, n):
    want, _ = whole(rt, scene, features, size)
    t, cam, w, l = camera(rt, scene, size)
    with rt.Scene(t, w, l) as sc:
        for i in range(n):
            with sc.accumulator(cam, max_passes=2, rank=i, nranks=n, features=features) as acc:
                for s in SEEDS:
                    acc.add(s)
                got = planes(acc)
            assert got.keys() == want.keys()
            for k in want:
                assert same_bits(got[k], want[k][i::n]), f"{scene} {size} share {i} of {n}: {k}"
    assert want["var"].max() > 0 and want["aov.depth"].max() > 0


@pytest.mark.parametrize("scene,features", CASES)
def test_add_shares_is_the_sequential_adds(rt, gpu, scene, features):
    size, n = (24, 17), 3
    want, samples = whole(rt, scene, features, size)
    t, cam, w, l = camera(rt, scene, size)
    with rt.Scene(t, w, l) as sc, sc.accumulator_shares(cam, [0] * n, max_passes=2, features=features) as sh:
        assert len(sh.shares) == n and sh.passes == 0
        stats = [sh.add(s) for s in SEEDS]
        assert sh.passes == 2 and [a.passes for a in sh.shares] == [2] * n
        # combined stats: the samples and rows of the whole render
        assert sum(st["samples"] for st in stats) == samples and stats[0]["rows"] == size[1]
        for i, a in enumerate(sh.shares):
            assert (a.shape, a.nranks) == ((len(range(i, size[1], n)), size[0]), n)
            with sc.accumulator(cam, max_passes=2, rank=i, nranks=n, features=features) as seq:
                for s in SEEDS:
                    seq.add(s)
                one, two = planes(a), planes(seq)
            assert all(same_bits(one[k], two[k]) for k in two), (scene, i)
        rgb, var = sh.resolve()
        assert same_bits(rgb, want["rgb"]) and same_bits(var, want["var"])


def test_add_shares_reports_the_lowest_failing_share(rt, gpu):
    t, cam, w, l = camera(rt, "cornell", (24, 17))
    with rt.Scene(t, w, l) as sc, sc.accumulator_shares(cam, [0, 0, 0], max_passes=1, features="emit") as sh:
        sh.shares[0].add(1)  # share 0 is full: the next pass fails there, and the others take it
        with pytest.raises(rt.RtError, match=r"rt_accum_add_shares share 0: .*holds its 1 passes") as e:
            sh.add(1)
        assert e.value.code == rt._lib.RT_ERR_INVALID
        assert [a.passes for a in sh.shares] == [1, 1, 1]
