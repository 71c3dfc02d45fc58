"""rt.Temporal(split_emitters=True, moments=True, clip=True) on rendered frames, the feature's claim:
`quads` 48 x 48, a 6-frame orbit, ONE pass x 4 spp per frame (features="emit").

The history is accepted on the first hit's depth and normal, which on the metal quad agree from
frame to frame while the reflection moves under them.  Clamping the reprojected colour to the
current frame's neighbourhood overrules such a history.  Asserted: over the pixels whose first hit
is the metal quad (render_aov's material plane), the last frame's mean squared error against a
1024-spp render of the last camera is lower with clip=True than without, at an orbit step of 3
degrees.  Both are computed here: an ordering, not a figure.  The table (all pixels, the metal quad,
the rest; per-frame mean, history, history + clip, each with and without the filter) is printed for
steps of 1, 2 and 3 degrees, and for `cornell`, where nothing is stale and nothing is asserted."""
import numpy as np
import pytest
import torch  # before the library's HIP runtime initialises (one runtime per process)

from tests.test_temporal_gpu import W, frame, host, orbit

pytestmark = pytest.mark.gpu
FRAMES = 6


def _table(rt, scene, step):
    """-> (rows: {set name: {column: mse}}, the first frame's (plain, clip) tuples, the last frame's)"""
    t, cam, w, l = rt.demo_scene(scene)
    cam.Width, cam.SamplesPerPixel = W, 4
    kw = dict(split_emitters=True, moments=True)
    plain, clip = rt.Temporal(**kw), rt.Temporal(clip=True, **kw)
    with rt.Scene(t, w, l) as sc:
        for k in range(FRAMES):
            camk = orbit(cam, step * k)
            with frame(sc, camk, (10 * k + 1,)) as acc:
                a, b = host(*plain.push(acc)), host(*clip.push(acc))
                if k == 0:
                    first = (a, b)
                if k == FRAMES - 1:
                    mean, _ = acc.resolve()
                    aov = acc.resolve_aov_device()
                    a_f, b_f = (rt.denoise_var_device(torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[1]).cuda(), aov,
                                                      split_emitters=True).cpu().numpy() for x in (a, b))
        material = sc.render_aov(camk)["material"]
        camk.SamplesPerPixel = 1024
        ref, _ = sc.render(camk, seed=977)
    fin = np.isfinite(mean).all(-1) & np.isfinite(ref).all(-1)
    metal = material == rt._lib.RT_MAT_METAL
    sets = {"all": fin, "metal": fin & metal, "rest": fin & ~metal}
    cols = {"frame": mean, "history": a[0], "history + clip": b[0], "history, filtered": a_f,
            "history + clip, filtered": b_f}
    rows = {r: {c: float(((x[m].astype(np.float64) - ref[m]) ** 2).mean()) if m.any() else float("nan")
                for c, x in cols.items()} for r, m in sets.items()}
    print(f"{scene} {W}x{W}, {FRAMES}-frame orbit of {step} degrees, 1 x 4 spp per frame, mse against 1024 spp")
    for r, m in sets.items():
        print(f"  {r}, {int(m.sum())} pixels: " + ", ".join(f"{c} {v:.5f}" for c, v in rows[r].items()))
    return rows, first, (a, b), sets


def test_clipping_overrules_the_stale_reflection_on_the_metal_quad(rt, gpu):
    rows, first, last, sets = _table(rt, "quads", 3.0)
    assert sets["metal"].sum() > 50
    # the first push has no history: nothing to clamp, the same bits
    assert all(np.array_equal(i, j, equal_nan=True) for i, j in zip(*first))
    # clipping changes the metal quad's pixels
    m = sets["metal"]
    assert (last[0][0][m] != last[1][0][m]).any(-1).mean() > 0.5
    assert np.isfinite(last[1][0][sets["all"]]).all() and (last[1][1][sets["all"]] >= 0).all()
    row = rows["metal"]
    assert row["history + clip"] < row["history"], row


@pytest.mark.parametrize("scene,step", [("quads", 1.0), ("quads", 2.0), ("cornell", 1.0)])
def test_the_other_tables_are_printed(rt, gpu, scene, step):
    """the smaller orbit steps, and Cornell, where no history is stale: what clipping costs there.
    Figures only; DESIGN.md section 22 holds the 128 x 128 tables"""
    rows, first, last, sets = _table(rt, scene, step)
    assert all(np.array_equal(i, j, equal_nan=True) for i, j in zip(*first))
    assert np.isfinite(last[1][0][sets["all"]]).all()


def test_clip_off_is_what_it_was(rt, gpu):
    """Temporal with moments, and with clip=False spelled out, give identical bits"""
    t, cam, w, l = rt.demo_scene("cornell")
    cam.Width, cam.SamplesPerPixel = W, 4
    x, y = rt.Temporal(split_emitters=True, moments=True), rt.Temporal(split_emitters=True, moments=True, clip=False)
    with rt.Scene(t, w, l) as sc:
        for k in range(3):
            with frame(sc, orbit(cam, 1.0 * k), (10 * k + 1,)) as acc:
                p, q = host(*x.push(acc)), host(*y.push(acc))
    assert all(np.array_equal(i, j, equal_nan=True) for i, j in zip(p, q))
