"""rt.Temporal(split_emitters=True, moments=True, specular=True) on rendered frames, the feature's
end-to-end claim, on tests/test_temporal_clip_gpu.py's set-up: `quads` 48 x 48, a 6-frame orbit, ONE
pass x 4 spp per frame (features="emit+spec"), mean squared error against a 1024-spp render of the last
camera over the pixels whose first hit is the metal quad.

Asserted, both sides computed here: at 3 degrees per frame the metal set's error with specular=True
(no clip) is below the error with clip=True alone.  Printed, not asserted: whether the specular
history beats the frame itself there, the share of metal pixels with history, the "rest" rows, the
tables at 1 and 2 degrees, `cornell` (no chain: asserted to have specular=False's bits) and `book1` at
48 x 27 (curved mirrors and glass).

The first push: rgb, count and lum2 have the non-specular object's bits everywhere.  Its variance is
the window's, and the window gates on the planes it is handed, so var has those bits wherever the
window holds no pixel with a chain (there the chain planes ARE the first hit's); on and next to a
mirror the window is gated by the chain's depth and normal, as the definition says.  There the first
push is pinned another way (test_the_first_push_next_to_a_mirror): every plane, var included, has the
bits of the moments entry without a history called on the same frame with the chain's normal and depth
in the first hit's place, which is what "the window gates on the planes it is handed" means."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_temporal_gpu import W, frame, host, orbit

pytestmark = pytest.mark.gpu
FRAMES = 6


def _table(rt, scene, step, width=W, height=None):
    t, cam, w, l = rt.demo_scene(scene)
    cam.Width, cam.SamplesPerPixel = width, 4
    if height:
        cam.AspectRatio = width / height
    cam.DefocusAngle = 0.0  # (book1's camera has a lens: reprojection takes pinhole cameras only)
    kw = dict(split_emitters=True, moments=True)
    objs = {"history": rt.Temporal(**kw), "history + clip": rt.Temporal(clip=True, **kw),
            "history + specular": rt.Temporal(specular=True, **kw),
            "history + specular + clip": rt.Temporal(specular=True, clip=True, **kw)}
    with rt.Scene(t, w, l) as sc:
        for k in range(FRAMES):
            camk = orbit(cam, step * k)
            with frame(sc, camk, (10 * k + 1,), features="emit+spec") as acc:
                res = {name: host(*o.push(acc)) for name, o in objs.items()}
                if k == 0:
                    first = res
                    bounces0 = acc.resolve_aov_spec()["bounces"]
                if k == FRAMES - 1:
                    mean, _ = acc.resolve()
                    aov = acc.resolve_aov_device()
                    filt = {name + ", filtered": rt.denoise_var_device(
                        torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[1]).cuda(), aov,
                        split_emitters=True).cpu().numpy() for name, x in res.items()}
        material = sc.render_aov(camk)["material"]
        camk.SamplesPerPixel = 1024
        ref, _ = sc.render(camk, seed=977)
    fin = np.isfinite(mean).all(-1) & np.isfinite(ref).all(-1)
    metal = material == rt._lib.RT_MAT_METAL
    sets = {"all": fin, "metal": fin & metal, "rest": fin & ~metal}
    cols = dict({"frame": mean}, **{n: x[0] for n, x in res.items()}, **filt)
    rows = {r: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) if m.any() else float("nan")
                for c, x in cols.items()} for r, m in sets.items()}
    hw = mean.shape[:2]
    print(f"{scene} {hw[1]}x{hw[0]}, {FRAMES}-frame orbit of {step} degrees, 1 x 4 spp per frame, mse against 1024 spp")
    for r, m in sets.items():
        print(f"  {r}, {int(m.sum())} pixels: " + ", ".join(f"{c} {v:.5f}" for c, v in rows[r].items()))
    if sets["metal"].any():
        m = sets["metal"]
        share = {n: float((res[n][2][m] > 1.5).mean()) for n in res}
        print("  metal pixels with history: " + ", ".join(f"{n} {v:.3f}" for n, v in share.items()))
        print(f"  the specular history {'beats' if rows['metal']['history + specular'] < rows['metal']['frame'] else 'does not beat'} "
              "the frame on the metal set")
    return rows, first, res, sets, bounces0


def _no_chain_in_window(bounces, radius=3):
    h, w = bounces.shape
    pad = np.pad(bounces != 0, radius, mode="constant")
    near = np.zeros((h, w), bool)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            near |= pad[dy:dy + h, dx:dx + w]
    return ~near


def _check_first(first, bounces0):
    a, b = first["history"], first["history + specular"]
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)
    clear = _no_chain_in_window(bounces0)
    assert np.array_equal(a[1][clear], b[1][clear], equal_nan=True)
    c, d = first["history + clip"], first["history + specular + clip"]
    assert np.array_equal(c[0], d[0], equal_nan=True) and np.array_equal(c[1][clear], d[1][clear], equal_nan=True)
    return clear


def test_the_specular_history_beats_the_clipped_one_on_the_metal_quad(rt, gpu):
    rows, first, last, sets, bounces0 = _table(rt, "quads", 3.0)
    assert sets["metal"].sum() > 50
    clear = _check_first(first, bounces0)
    assert clear.sum() > 100 and (~clear).sum() > 50
    m = sets["metal"]
    assert (last["history"][0][m] != last["history + specular"][0][m]).any(-1).mean() > 0.5
    for n in ("history + specular", "history + specular + clip"):
        assert np.isfinite(last[n][0][sets["all"]]).all() and (last[n][1][sets["all"]] >= 0).all()
    row = rows["metal"]
    assert row["history + specular"] < row["history + clip"], row


@pytest.mark.parametrize("scene,step,size", [("quads", 1.0, (W, None)), ("quads", 2.0, (W, None)),
                                             ("book1", 3.0, (48, 27))])
def test_the_other_tables_are_printed(rt, gpu, scene, step, size):
    """figures only; DESIGN.md section 23 holds the 128 x 128 tables (tools/accum_spec_bench.py,
    profiles/accum_spec.json)"""
    rows, first, last, sets, bounces0 = _table(rt, scene, step, *size)
    _check_first(first, bounces0)
    assert np.isfinite(last["history + specular"][0][sets["all"]]).all()


def test_the_first_push_next_to_a_mirror(rt, gpu):
    """the first push of the specular object, everywhere, the metal quad and its surroundings
    included: rgb, var, count are reproject_moments_device's without a previous frame, fed the chain's
    normal and depth; with clip=True reproject_clip_device's.  And the variance does differ from the
    non-specular object's somewhere on or next to the quad, or this test would say nothing"""
    t, cam, w, l = rt.demo_scene("quads")
    cam.Width, cam.SamplesPerPixel = W, 4
    kw = dict(split_emitters=True, moments=True)
    with rt.Scene(t, w, l) as sc, frame(sc, cam, (1,), features="emit+spec") as acc:
        h, wd = acc.shape
        rgb, var = torch.empty((h, wd, 3), device="cuda"), torch.empty((h, wd), device="cuda")
        acc.resolve_device(rgb, var)
        first, chain = acc.resolve_aov_device(), acc.resolve_aov_spec_device()
        cur = {"rgb": rgb, "var": var, "count": 1.0, "emission": first["emission"], "coverage": first["coverage"],
               "normal": chain["normal"], "depth": chain["depth"]}
        want = host(*rt.reproject_moments_device("emit", None, None, acc.camera, cur)[:3])
        want_clip = host(*rt.reproject_clip_device("emit", None, None, acc.camera, cur)[:3])
        got = host(*rt.Temporal(specular=True, **kw).push(acc))
        got_clip = host(*rt.Temporal(specular=True, clip=True, **kw).push(acc))
        plain = host(*rt.Temporal(**kw).push(acc))
        bounces = chain["bounces"].cpu().numpy()
    for a, b in ((got, want), (got_clip, want_clip)):
        assert all(np.array_equal(i, j, equal_nan=True) for i, j in zip(a, b))
    near = ~_no_chain_in_window(bounces)
    differs = got[1] != plain[1]
    print(f"first push: var differs from the non-specular object's at {int(differs.sum())} pixels, all of them among "
          f"the {int(near.sum())} with a chain pixel in their window: {not differs[~near].any()}")
    assert differs.any() and not differs[~near].any()


def test_without_a_chain_it_is_the_non_specular_object(rt, gpu):
    """cornell has no specular surface: every bounces value is 0, the chain planes are the first hit's,
    and every push has specular=False's bits, with and without the clamp"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    kw = dict(split_emitters=True, moments=True)
    pairs = [(rt.Temporal(**kw), rt.Temporal(specular=True, **kw)),
             (rt.Temporal(clip=True, **kw), rt.Temporal(specular=True, clip=True, **kw))]
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with frame(sc, orbit(cam, 1.0 * k), (10 * k + 1,), features="emit+spec") as acc:
                assert not acc.resolve_aov_spec()["bounces"].any()
                for x, y in pairs:
                    p, q = host(*x.push(acc)), host(*y.push(acc))
                    assert all(np.array_equal(i, j, equal_nan=True) for i, j in zip(p, q)), k
    assert float(q[2].max()) > 1.0


def test_specular_off_is_what_it_was(rt, gpu):
    """specular=False spelled out, on an accumulator with the chain planes and on one without: the
    bits of Temporal(moments=True) on a plain "emit" accumulator"""
    t, cam, w, l = rt.demo_scene("quads")
    cam.Width, cam.SamplesPerPixel = W, 4
    kw = dict(split_emitters=True, moments=True, clip=True)
    x, y = rt.Temporal(**kw), rt.Temporal(specular=False, **kw)
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            camk = orbit(cam, 3.0 * k)
            with frame(sc, camk, (10 * k + 1,)) as a, frame(sc, camk, (10 * k + 1,), features="emit+spec") as b:
                p, q = host(*x.push(a)), host(*y.push(b))
    assert all(np.array_equal(i, j, equal_nan=True) for i, j in zip(p, q))
    with pytest.raises(ValueError, match="emit\\+spec"):
        with rt.Scene(t, w, l) as sc, frame(sc, cam, (1,)) as a:
            rt.Temporal(split_emitters=True, moments=True, specular=True).push(a)
