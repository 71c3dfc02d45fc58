"""A numpy restatement of rt_reproject, written from the definition pinned in include/rt_abi.h
(not from the kernel), with the dtype of every operation as an argument, as tests/
test_denoise_var_gpu.py's svgf() has it: dt=np.float64 is the reference, dt=np.float32 measures
what fp32 arithmetic alone costs.  Both start from what the kernel is handed: the camera vectors
and the options rounded to fp32.

It also returns a per-pixel `fragile` flag: set when a yes/no decision of the pixel sits within a
relative 1e-3 of its threshold, where fp32 may legitimately decide the other way.  The decisions:
  s > 0               |den| <= 1e-3 |r| |Wp|  (the threshold is 0: relative to the product's scale)
  u, v near integers  |u - round(u)| <= 1e-3 or |v - round(v)| <= 1e-3 while a tap can be inside;
                      "a tap inside the image" changes only when floor(u) or floor(v) does, so this
                      is that decision's flag too
  depth tolerance     | |depth_q - d'| - depth_tol d' | <= 1e-3 depth_tol d'
  normal tolerance    | |n_p - n_q|^2 - normal_tol | <= 1e-3 normal_tol
                      (both for the taps inside the image that pass the tests without a threshold)
  S >= min_weight     |S - min_weight| <= 1e-3 min_weight
  n against the cap   |sum beta n_q / S - max_history| <= 1e-3 max_history
Fragile pixels are left out of value comparisons.

The fixtures of the tests are built here too (fixture()): two fronto-parallel planes meeting in a
step edge, seen by two cameras, with the depths evaluated analytically."""
import numpy as np

FRAGILE_REL = 1e-3
FRAGILE_CAP = 0.02   # a fixture may have at most this share of fragile pixels
DEFAULTS = dict(max_history=0.0, depth_tol=0.05, normal_tol=0.1, min_weight=0.01)


def geometry(cam):
    """rt_camera_derive's fp64 vectors of a go_raytracer_amd.Camera"""
    d = cam.derived()
    g = {k: np.array(getattr(d, n), np.float64) for k, n in
         (("C", "center"), ("P00", "pixel00"), ("U", "delta_u"), ("V", "delta_v"))}
    g["w"], g["h"] = d.width, d.height
    return g


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def reproject(gp, prev, gc, cur, max_history=0.0, depth_tol=0.0, normal_tol=0.0, min_weight=0.0,
              dt=np.float64):
    """gp, gc: geometry() of the previous / current camera.  prev, cur: dicts of "rgb", "normal",
    "depth" and optionally "var" (missing: 0) and "count" (an array or one number).
    -> {"rgb", "var", "count" (arrays of dtype dt), "history" (bool: n_h > 0), "fragile" (bool)}"""
    h, w = np.shape(cur["rgb"])[:2]

    def vec(a):  # what the kernel is handed: fp32
        return np.asarray(a, np.float64).astype(np.float32).astype(dt)

    def opt(value, default):
        return np.float32(value if value > 0 else default).astype(dt)

    D, Ac, Uc, Vc = vec(gc["C"] - gp["C"]), vec(gc["P00"] - gc["C"]), vec(gc["U"]), vec(gc["V"])
    Ap, Up, Vp = vec(gp["P00"] - gp["C"]), vec(gp["U"]), vec(gp["V"])
    depth_tol, normal_tol = opt(depth_tol, 0.05), opt(normal_tol, 0.1)
    min_weight = opt(min_weight, 0.01)

    def planes(f):
        rgb = np.asarray(f["rgb"], np.float32).astype(dt)
        var = np.zeros((h, w), dt) if f.get("var") is None else np.asarray(f["var"], np.float32).astype(dt)
        cnt = f.get("count")
        cnt = (np.full((h, w), np.float32(0.0 if cnt is None else cnt)).astype(dt) if cnt is None or np.ndim(cnt) == 0
               else np.asarray(cnt, np.float32).astype(dt))
        return rgb, var, cnt, np.asarray(f["normal"], np.float32).astype(dt), np.asarray(f["depth"], np.float32).astype(dt)

    c, v, nc, n_p, d_p = planes(cur)
    cq_all, vq_all, nq_all, nrm_q_all, dq_all = planes(prev)
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.astype(dt), ys.astype(dt)
    with np.errstate(all="ignore"):
        valid = np.isfinite(c).all(-1) & np.isfinite(v) & np.isfinite(nc) & (nc > 0)
        hist = valid & np.isfinite(d_p) & (d_p > 0) & np.isfinite(n_p).all(-1)
        dirv = Ac + fx[..., None] * Uc + fy[..., None] * Vc
        r = D + (d_p / np.sqrt(_dot(dirv, dirv)))[..., None] * dirv
        d1 = np.sqrt(_dot(r, r))
        Wp = np.cross(Up, Vp).astype(dt)
        num, den = _dot(Ap, Wp), _dot(r, Wp)
        s = num / den
        fragile = hist & (np.abs(den) <= dt(FRAGILE_REL) * d1 * np.sqrt(_dot(Wp, Wp)))
        hist = hist & np.isfinite(s) & (s > 0)
        q = s[..., None] * r - Ap
        u, vv = _dot(q, Up) / _dot(Up, Up), _dot(q, Vp) / _dot(Vp, Vp)
        # beyond [-1, w) x [-1, h) no tap is inside; clamped so that the conversion to int is defined
        u = np.where(hist, np.clip(np.nan_to_num(u, nan=-2.0), -2, w + 1), -2).astype(dt)
        vv = np.where(hist, np.clip(np.nan_to_num(vv, nan=-2.0), -2, h + 1), -2).astype(dt)
        near = ((np.abs(u - np.round(u)) <= FRAGILE_REL) | (np.abs(vv - np.round(vv)) <= FRAGILE_REL))
        reach = (u >= -1 - FRAGILE_REL) & (u <= w + FRAGILE_REL) & (vv >= -1 - FRAGILE_REL) & (vv <= h + FRAGILE_REL)
        fragile |= hist & near & reach
        u0, v0 = np.floor(u), np.floor(vv)
        x0, y0 = u0.astype(np.int64), v0.astype(np.int64)
        bu, bv = (dt(1) - (u - u0), u - u0), (dt(1) - (vv - v0), vv - v0)
        S, sn, sv = np.zeros((h, w), dt), np.zeros((h, w), dt), np.zeros((h, w), dt)
        sc = np.zeros((h, w, 3), dt)
        for b in (0, 1):
            for a in (0, 1):
                qx, qy = x0 + a, y0 + b
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                cq, vq, nq, dq = cq_all[cy, cx], vq_all[cy, cx], nq_all[cy, cx], dq_all[cy, cx]
                plain = (hist & inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & np.isfinite(nq) & (nq > 0)
                         & (dq > 0))
                dd = np.abs(dq - d1)
                dn = n_p - nrm_q_all[cy, cx]
                dn2 = _dot(dn, dn)
                ok = plain & (dd <= depth_tol * d1) & (dn2 <= normal_tol)
                fragile |= plain & (np.abs(dd - depth_tol * d1) <= FRAGILE_REL * depth_tol * d1)
                fragile |= plain & (np.abs(dn2 - normal_tol) <= FRAGILE_REL * normal_tol)
                beta = np.where(ok, bu[a] * bv[b], dt(0)).astype(dt)
                S += beta
                sc += beta[..., None] * np.where(ok[..., None], cq, dt(0))
                sv += beta * beta * np.where(ok, vq, dt(0))
                sn += beta * np.where(ok, nq, dt(0))
        fragile |= hist & (np.abs(S - min_weight) <= FRAGILE_REL * min_weight)
        hist = hist & (S >= min_weight)
        cap = (np.float32(max_history).astype(dt) if max_history > 0 else dt(8) * nc) + np.zeros((h, w), dt)
        n_raw = sn / S
        fragile |= hist & (np.abs(n_raw - cap) <= FRAGILE_REL * cap)
        nh = np.minimum(n_raw, cap)
        ch, vh = sc / S[..., None], sv / (S * S)
        n = nh + nc
        o_rgb = (nh[..., None] * ch + nc[..., None] * c) / n[..., None]
        o_var = (nh * nh * vh + nc * nc * v) / (n * n)
    return {"rgb": np.where(hist[..., None], o_rgb, c), "var": np.where(hist, o_var, v),
            "count": np.where(hist, n, nc), "history": hist, "fragile": fragile}


# ---- fixtures -----------------------------------------------------------------------------------

EDGE_X = 0.0371   # the near plane covers world x < EDGE_X (off every pixel centre's ray)
N_NEAR, N_FAR = (0.0, 0.0, 1.0), (0.6, 0.0, 0.8)   # |dn|^2 = 0.4 against the tolerance 0.1
Z_NEAR, Z_FAR = -4.0, -6.0
# previous camera's offset per fixture size where the issue's (0.13, 0.07, 0) would put a plane's
# near-constant u - x or v - y within 1e-3 of an integer (see test_reproject_ref.py)
OFFSETS = {}
OFFSET = (0.13, 0.07, 0.0)
YAW_DEG = 1.5


def cameras(rt, w, h, offset=None, yaw_deg=YAW_DEG):
    """(previous, current): the current camera at the origin looking down -z, 40 degrees across
    the longer side; the previous one translated by `offset` and yawed about +y"""
    offset = OFFSETS.get((w, h), OFFSET) if offset is None else offset
    vfov = 40.0 if h >= w else float(np.degrees(2 * np.arctan(np.tan(np.radians(20.0)) * h / w)))
    cams = []
    for frm, yaw in ((offset, yaw_deg), ((0.0, 0.0, 0.0), 0.0)):
        cam = rt.Camera(Width=w, AspectRatio=w / (h + 0.25), VerticalFOV=vfov, SamplesPerPixel=1)
        a = np.radians(yaw)
        at = (frm[0] - np.sin(a), frm[1], frm[2] - np.cos(a))
        cam.PositionCamera(frm, at, (0.0, 1.0, 0.0))
        assert cam.image_size()[:2] == (w, h)
        cams.append(cam)
    return cams[0], cams[1]


def surfaces(g):
    """(normal float32 [h, w, 3], depth float32 [h, w]) of the two planes at the pixel centres of
    a camera with geometry g, analytically in fp64: the distance along the ray, as rt_aov's depth"""
    ys, xs = np.mgrid[0:g["h"], 0:g["w"]]
    d = g["P00"] + xs[..., None] * g["U"] + ys[..., None] * g["V"] - g["C"]
    d /= np.sqrt((d * d).sum(-1))[..., None]
    t_near, t_far = (Z_NEAR - g["C"][2]) / d[..., 2], (Z_FAR - g["C"][2]) / d[..., 2]
    near = g["C"][0] + t_near * d[..., 0] < EDGE_X
    depth = np.where(near, t_near, t_far)
    normal = np.where(near[..., None], N_NEAR, N_FAR)
    return normal.astype(np.float32), depth.astype(np.float32)


_fixtures = {}


def fixture(rt, w, h):
    """{"cams": (prev, cur), "gp", "gc", "prev", "cur"} for a w x h image, built once per size and
    read-only.  Colours and variances are test_denoise_var_gpu.py's synthetic() / variance()
    (their NaN / Inf pixels and the block of zero variance included), counts are 1 .. 40, prev has
    a block of count 0, both frames a block of misses (depth 0, normal 0)."""
    if (w, h) in _fixtures:
        return _fixtures[(w, h)]
    from tests.test_denoise_var_gpu import synthetic, variance
    cam_p, cam_c = cameras(rt, w, h)
    gp, gc = geometry(cam_p), geometry(cam_c)
    frames = []
    ys, xs = np.mgrid[0:h, 0:w]
    for k, g in enumerate((gp, gc)):
        rng = np.random.default_rng(1000 * k + 10 * h + w)
        rgb = synthetic(h, w, seed=31 + k + h * 100 + w)[0]
        var = variance(h, w, seed=41 + k)
        normal, depth = surfaces(g)
        count = rng.integers(1, 41, (h, w)).astype(np.float32)
        miss = (ys >= h - max(h // 5, 1)) & (xs >= w - max(w // 6, 1)) & (h > 2)
        depth[miss] = 0.0
        normal[miss] = 0.0
        if k == 0 and w > 4:
            count[(ys < max(h // 4, 1)) & (xs >= w // 2) & (xs < w // 2 + max(w // 8, 1))] = 0.0
        f = {"rgb": rgb, "var": var, "count": count, "normal": normal, "depth": depth}
        for a in f.values():
            a.setflags(write=False)
        frames.append(f)
    _fixtures[(w, h)] = {"cams": (cam_p, cam_c), "gp": gp, "gc": gc, "prev": frames[0], "cur": frames[1]}
    return _fixtures[(w, h)]
