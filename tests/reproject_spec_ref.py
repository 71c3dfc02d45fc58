"""A numpy restatement of rt_reproject_spec, written from the definition pinned in include/rt_abi.h
(not from the kernel): rt_reproject_clip in its three modes (PLAIN, EMIT, LIGHT), with or without the
clamp, fed the specular chains' normal and depth, and gated on the chains' length.  dt=np.float64 is
the reference, dt=np.float32 measures what fp32 arithmetic alone costs.

It is written out in full, as tests/reproject_clip_ref.py is and for its reason: the two deltas sit in
the middle of the body.  Every frame may hold "bounces" [h, w]:
  current pixel   b_c is WHOLE when finite, >= 0 and equal to its floor; a pixel whose b_c is not
                  whole has no history and takes the mode's no-history path
  tap             the mode's rule, and b_q == b_c exactly (a NaN fails); the tap's value is compared
                  only, never used in arithmetic
With bounces=False (spec = NULL) the two statements are skipped and the values are
reproject_clip_ref's bit for bit (tests/test_reproject_spec_ref.py).

The fragile set is reproject_clip_ref's: the gate compares caller-supplied values exactly, so no
decision of it can turn with the arithmetic's precision, and it adds no fragile pixel.

fixture(): the clip fixture of the mode and size with bounces planes: zero over most of the image, a
block of 1.0 in both frames, a block where prev is 2.0 against cur 1.0, a block of cur 0.5, and one
NaN in each plane."""
import numpy as np

from tests import reproject_clip_ref as K
from tests import reproject_moments_ref as M
from tests import reproject_ref as R

FRAGILE_REL, FRAGILE_CAP = M.FRAGILE_REL, M.FRAGILE_CAP
PLAIN, EMIT, LIGHT, MODES, NAMES, keys, lum = M.PLAIN, M.EMIT, M.LIGHT, M.MODES, M.NAMES, M.keys, M.lum
DEFAULT_GAMMA = K.DEFAULT_GAMMA


def reproject_spec(mode, gp, prev, gc, cur, max_history=0.0, depth_tol=0.0, normal_tol=0.0, min_weight=0.0,
                   min_frames=0.0, radius=0, gamma=0.0, bounces=True, dt=np.float64):
    """arguments as reproject_clip_ref.reproject_clip's; bounces False: spec = NULL, the frames'
    "bounces" are not read.  -> its dict, and "whole" (bool: b_c is whole; all True without bounces)
    and "S" (the surface taps' weight sum)"""
    h, w = np.shape(cur["rgb"])[:2]
    _dot = R._dot
    emit, light = mode != PLAIN, mode == LIGHT
    clip = gamma is not None
    no_prev = prev is None
    if no_prev:
        gp, prev = gc, dict(cur, count=0.0, lum2=np.zeros((h, w), np.float32))

    def vec(a):  # what the kernel is handed: fp32
        return np.asarray(a, np.float64).astype(np.float32).astype(dt)

    def opt(value, default):
        return np.float32(value if value > 0 else default).astype(dt)

    D, Ac, Uc, Vc = vec(gc["C"] - gp["C"]), vec(gc["P00"] - gc["C"]), vec(gc["U"]), vec(gc["V"])
    Ap, Up, Vp = vec(gp["P00"] - gp["C"]), vec(gp["U"]), vec(gp["V"])
    depth_tol, normal_tol = opt(depth_tol, 0.05), opt(normal_tol, 0.1)
    min_weight, min_frames = opt(min_weight, 0.01), opt(min_frames, 4.0)
    radius = 3 if radius == 0 else radius
    if clip:
        assert radius >= 0, "the library refuses copts with radius -1"
        gamma = opt(gamma, DEFAULT_GAMMA)

    def planes(f):
        def a(x):
            return np.asarray(x, np.float32).astype(dt)
        var = np.zeros((h, w), dt) if f.get("var") is None else a(f["var"])
        cnt = f.get("count")
        cnt = (np.full((h, w), np.float32(0.0 if cnt is None else cnt)).astype(dt) if cnt is None or np.ndim(cnt) == 0
               else a(cnt))
        em = a(f["emission"]) if emit else np.zeros((h, w, 3), dt)
        cov = a(f["coverage"]) if emit else np.zeros((h, w), dt)
        return a(f["rgb"]), var, cnt, a(f["normal"]), a(f["depth"]), em, cov

    c, v, nc, n_p, d_p, e_c, cov_c = planes(cur)
    cq_all, vq_all, nq_all, nrm_q_all, dq_all, eq_all, covq_all = planes(prev)
    lq_all = np.asarray(prev["lum2"], np.float32).astype(dt)
    if bounces:  # compared, never computed with: kept as the float32 the caller handed over
        b_c = np.asarray(cur["bounces"], np.float32)
        b_q_all = b_c if no_prev else np.asarray(prev["bounces"], np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.astype(dt), ys.astype(dt)
    with np.errstate(all="ignore"):
        valid = np.isfinite(c).all(-1) & np.isfinite(v) & np.isfinite(nc) & (nc > 0)
        if emit:  # a fully covered pixel is valid in LIGHT only
            valid &= np.isfinite(e_c).all(-1) & (cov_c >= 0) & ((cov_c <= 1) if light else (cov_c < 1))
        surf = valid & (cov_c < 1)                      # the current pixel has a surface sample: w_c > 0
        w_c = np.where(cov_c < 1, nc, dt(0)).astype(dt)
        k_c = np.where(surf, dt(1) - cov_c, dt(1)).astype(dt)
        z_c = (c - e_c) / k_c[..., None] if emit else c
        vz_c = v / (k_c * k_c) if emit else v
        y_c = lum(z_c)
        q_c = y_c * y_c                                 # q before the blend
        hist = valid & np.isfinite(d_p) & (d_p > 0) & np.isfinite(n_p).all(-1) & (not no_prev)
        whole = np.ones((h, w), bool)
        if bounces:
            whole = np.isfinite(b_c) & (b_c >= 0) & (b_c == np.floor(b_c))
            hist = hist & whole
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
        u = np.where(hist, np.clip(np.nan_to_num(u, nan=-2.0), -2, w + 1), -2).astype(dt)
        vv = np.where(hist, np.clip(np.nan_to_num(vv, nan=-2.0), -2, h + 1), -2).astype(dt)
        near = ((np.abs(u - np.round(u)) <= FRAGILE_REL) | (np.abs(vv - np.round(vv)) <= FRAGILE_REL))
        reach = (u >= -1 - FRAGILE_REL) & (u <= w + FRAGILE_REL) & (vv >= -1 - FRAGILE_REL) & (vv <= h + FRAGILE_REL)
        fragile |= hist & near & reach
        u0, v0 = np.floor(u), np.floor(vv)
        x0, y0 = u0.astype(np.int64), v0.astype(np.int64)
        bu, bv = (dt(1) - (u - u0), u - u0), (dt(1) - (vv - v0), vv - v0)
        zero = lambda: np.zeros((h, w), dt)  # noqa: E731
        S, sn, sv, sq, sc = zero(), zero(), zero(), zero(), np.zeros((h, w, 3), dt)   # the surface taps
        Sl, sm, sk, se = zero(), zero(), zero(), np.zeros((h, w, 3), dt)              # the light taps
        for b in (0, 1):
            for a in (0, 1):
                qx, qy = x0 + a, y0 + b
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                cq, vq, nq, dq = cq_all[cy, cx], vq_all[cy, cx], nq_all[cy, cx], dq_all[cy, cx]
                eq, covq, lq = eq_all[cy, cx], covq_all[cy, cx], lq_all[cy, cx]
                plain = (hist & inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & np.isfinite(nq) & (nq > 0)
                         & (dq > 0) & np.isfinite(lq))
                if emit:
                    plain &= np.isfinite(eq).all(-1) & (covq >= 0) & ((covq <= 1) if light else (covq < 1))
                if bounces:
                    plain &= b_q_all[cy, cx] == b_c
                dd = np.abs(dq - d1)
                dn = n_p - nrm_q_all[cy, cx]
                dn2 = _dot(dn, dn)
                okl = plain & (dd <= depth_tol * d1) & (dn2 <= normal_tol)   # a light tap
                ok = okl & (covq < 1)                                        # a surface tap
                fragile |= plain & (np.abs(dd - depth_tol * d1) <= FRAGILE_REL * depth_tol * d1)
                fragile |= plain & (np.abs(dn2 - normal_tol) <= FRAGILE_REL * normal_tol)
                beta = np.where(ok, bu[a] * bv[b], dt(0)).astype(dt)
                cq0 = np.where(ok[..., None], cq, dt(0))
                if emit:
                    k_q = np.where(ok, dt(1) - covq, dt(1)).astype(dt)
                    z_q = (cq0 - np.where(ok[..., None], eq, dt(0))) / k_q[..., None]
                    vz_q = np.where(ok, vq, dt(0)) / (k_q * k_q)
                else:
                    z_q, vz_q = cq0, np.where(ok, vq, dt(0))
                S += beta
                sc += beta[..., None] * z_q
                sv += beta * beta * vz_q
                sn += beta * np.where(ok, nq, dt(0))
                sq += beta * np.where(ok, lq, dt(0))
                bl = np.where(okl, bu[a] * bv[b], dt(0)).astype(dt)
                Sl += bl
                se += bl[..., None] * np.where(okl[..., None], eq, dt(0))
                sk += bl * np.where(okl, covq, dt(0))
                sm += bl * np.where(okl, nq, dt(0))
        fragile |= hist & (np.abs(S - min_weight) <= FRAGILE_REL * min_weight)
        hs = hist & (S >= min_weight)
        hl = hs
        if light:
            fragile |= hist & (np.abs(Sl - min_weight) <= FRAGILE_REL * min_weight)
            hl = hist & (Sl >= min_weight)
        cap = (np.float32(max_history).astype(dt) if max_history > 0 else dt(8) * nc) + np.zeros((h, w), dt)
        n_raw, m_raw = sn / S, sm / Sl
        fragile |= hs & (np.abs(n_raw - cap) <= FRAGILE_REL * cap)
        if light:
            fragile |= hl & (np.abs(m_raw - cap) <= FRAGILE_REL * cap)
        nh = np.where(hs, np.minimum(n_raw, cap), dt(0)).astype(dt)
        mh = np.where(hl, np.minimum(m_raw, cap), dt(0)).astype(dt)
        zh = np.where(hs[..., None], sc / S[..., None], dt(0))
        vh = np.where(hs, sv / (S * S), dt(0))
        qh = np.where(hs, sq / S, dt(0))
        eh = np.where(hl[..., None], se / Sl[..., None], dt(0))
        kh = np.where(hl, sk / Sl, dt(0))
        blend = (hs | hl) & (hs | (w_c > 0))
        n = nh + w_c
        # the window of the current frame, rows then columns: the spatial estimate's luminance sums and,
        # with clipping, the shifted colour sums of the box
        ok_t = surf                                          # valid by the mode's rule, kappa < 1
        y_t = np.where(ok_t, y_c, dt(0))
        z_t = np.where(ok_t[..., None], z_c, dt(0))
        a_s, b_s, T = zero(), zero(), zero()
        A, B = np.zeros((h, w, 3), dt), np.zeros((h, w, 3), dt)
        near_gate = np.zeros((h, w), bool)                   # a window pixel sits on a tolerance
        tol_d = depth_tol * d_p
        for dy in range(-max(radius, 0), max(radius, 0) + 1):
            for dx in range(-max(radius, 0), max(radius, 0) + 1):
                tx, ty = xs + dx, ys + dy
                inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                cx, cy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
                base = inside & ok_t[cy, cx]
                dd = np.abs(d_p[cy, cx] - d_p)
                dn = n_p - n_p[cy, cx]
                dn2 = _dot(dn, dn)
                if dx == 0 and dy == 0:
                    okw = base                               # p itself always counts
                else:
                    okw = base & (dd <= tol_d) & (dn2 <= normal_tol)
                    on_d = surf & base & (tol_d > 0) & (np.abs(dd - tol_d) <= FRAGILE_REL * tol_d) & (radius >= 0)
                    on_n = surf & base & (np.abs(dn2 - normal_tol) <= FRAGILE_REL * normal_tol) & (radius >= 0)
                    fragile |= on_d | on_n
                    near_gate |= on_d | on_n
                yt = np.where(okw, y_t[cy, cx], dt(0))
                a_s += yt
                b_s += yt * yt
                T += np.where(okw, dt(1), dt(0))
                if clip:
                    d = np.where(okw[..., None], z_t[cy, cx] - z_c, dt(0))   # the deviation from x_p
                    A += d
                    B += d * d
        # the box and the clamp: x_h' stands in for the history colour
        clampable = hs & surf & (T >= 2) & clip
        x_h = zh
        lo, hi = np.full((h, w, 3), -np.inf, dt), np.full((h, w, 3), np.inf, dt)
        clamped = np.zeros((h, w), bool)
        if clip:
            fragile |= hs & surf & (T <= 2) & near_gate      # the decision T >= 2
            Tn = T[..., None]
            mA = A / Tn
            m_box = z_c + mA
            s_box = gamma * np.sqrt(np.maximum(B / Tn - mA * mA, dt(0)))
            lo = np.where(clampable[..., None], m_box - s_box, lo).astype(dt)
            hi = np.where(clampable[..., None], m_box + s_box, hi).astype(dt)
            edge = dt(FRAGILE_REL) * (np.abs(m_box) + s_box)
            fragile |= clampable & ((np.abs(x_h - lo) <= edge) | (np.abs(x_h - hi) <= edge)).any(-1)
            zh = np.minimum(np.maximum(x_h, lo), hi).astype(dt)
            clamped = clampable & (zh != x_h).any(-1)
        z_blend = (nh[..., None] * zh + w_c[..., None] * z_c) / n[..., None]
        v_blend = (nh * nh * vh + w_c * w_c * vz_c) / (n * n)
        q_out = (nh * qh + w_c * q_c) / n
        y_out = lum(z_blend.astype(dt))
        K = np.where(hs & surf, n / w_c, dt(1)).astype(dt)   # the history length in frames
        fragile |= hs & surf & (np.abs(K - min_frames) <= FRAGILE_REL * min_frames)
        v_t = np.maximum(q_out - y_out * y_out, dt(0)) / (K - dt(1))
        took_t = hs & surf & (K >= min_frames) & (radius >= 0)
        took_s = surf & ~took_t & (radius >= 0)
        am, bm = a_s / T, b_s / T
        v_s = np.where(T >= 2, np.maximum(bm - am * am, dt(0)) * (T / (T - dt(1))), dt(0)) / K
        v_carry = np.where(took_t, v_t, np.where(took_s, v_s, v_blend))
        m = mh + nc
        if light:
            k_out = (mh * kh + nc * cov_c) / m
            e_out = (mh[..., None] * eh + nc[..., None] * e_c) / m[..., None]
            o_cnt = np.maximum(nh, mh) + nc
        else:
            k_out, e_out, o_cnt = cov_c, e_c, n
        if emit:
            o_rgb = (dt(1) - k_out)[..., None] * z_blend + e_out if light else k_c[..., None] * z_blend + e_c
            relit = (dt(1) - k_out) if light else k_c
            o_var = relit * relit * v_carry
        else:
            o_rgb, o_var = z_blend, v_carry
        # no blend: the mode passes the pixel through; with a surface sample its var is the re-lit v_s
        p_var = np.where(took_s, k_c * k_c * v_s, v)
        lum2 = np.where(blend, q_out, np.where(surf, q_c, dt(0)))
    b3 = blend[..., None]
    return {"rgb": np.where(b3, o_rgb, c), "var": np.where(blend, o_var, p_var), "count": np.where(blend, o_cnt, nc),
            "emission": np.where(b3, e_out, e_c), "coverage": np.where(blend, k_out, cov_c), "lum2": lum2,
            "history": hs, "light_history": hl, "blend": blend, "took_t": took_t & blend, "took_s": took_s,
            "zero": ~blend & ~surf, "fragile": fragile, "K": K, "clampable": clampable, "clamped": clamped, "T": T,
            "box_lo": lo, "box_hi": hi, "x_h": x_h, "whole": whole, "S": S}


# ---- fixtures -----------------------------------------------------------------------------------

_fixtures = {}


def bounces_planes(w, h):
    """(prev, cur) bounces of the module docstring: zero; rows [h/4, h/2) x columns [w/8, w/2) 1.0 in
    both; rows [h/2, 3h/4) x columns [w/8, w/2) prev 2.0 against cur 1.0; rows [h/4, 3h/4) x columns
    [5w/8, 7w/8) cur 0.5; one NaN in each plane (images under 4 x 4: the NaNs only where they fit)"""
    ys, xs = np.mgrid[0:h, 0:w]
    big = (w >= 4) & (h >= 4)
    left = (xs >= w // 8) & (xs < w // 2) & big
    prev, cur = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    both = left & (ys >= h // 4) & (ys < h // 2)
    differ = left & (ys >= h // 2) & (ys < 3 * h // 4)
    half = (xs >= 5 * w // 8) & (xs < 7 * w // 8) & (ys >= h // 4) & (ys < 3 * h // 4) & big
    prev[both], cur[both] = 1.0, 1.0
    prev[differ], cur[differ] = 2.0, 1.0
    cur[half] = 0.5
    prev[h - 1, w - 1] = np.nan
    cur[0, w // 2] = np.nan
    return prev, cur


def fixture(rt, mode, w, h):
    """the clip fixture with the bounces planes.  Built once per mode and size, read-only."""
    if (mode, w, h) in _fixtures:
        return _fixtures[(mode, w, h)]
    fx = K.fixture(rt, mode, w, h)
    bp, bc = bounces_planes(w, h)
    bp.setflags(write=False), bc.setflags(write=False)
    _fixtures[(mode, w, h)] = dict(fx, prev=dict(fx["prev"], bounces=bp), cur=dict(fx["cur"], bounces=bc))
    return _fixtures[(mode, w, h)]


# ---- the planar-mirror scene, analytic and noise-free -------------------------

MIRROR_W, MIRROR_H = 24, 17


def mirror_cameras(rt):
    """cam_prev looks from (0, 1, 0) at (0, 0, -0.6), cam_cur from (0.3, 1, 0.1) at (0.25, 0, -0.6);
    vfov 40, 24 x 17"""
    cams = []
    for frm, at in (((0.0, 1.0, 0.0), (0.0, 0.0, -0.6)), ((0.3, 1.0, 0.1), (0.25, 0.0, -0.6))):
        cam = rt.Camera(Width=MIRROR_W, AspectRatio=MIRROR_W / (MIRROR_H + 0.25), VerticalFOV=40.0, SamplesPerPixel=1)
        cam.PositionCamera(frm, at, (0.0, 1.0, 0.0))
        assert cam.image_size()[:2] == (MIRROR_W, MIRROR_H)
        cams.append(cam)
    return cams


def mirror_frame(g, w, h):
    """the frame a camera of geometry g sees of a mirror floor y = 0 (albedo 0.8) under a diffuse
    ceiling y = 2 of colour (0.5 + 0.2 X_x, 0.5 + 0.2 X_z, 0.5), through the pixel centres: the
    first-hit planes and the chain planes, float32"""
    ys, xs = np.mgrid[0:h, 0:w]
    d = g["P00"] + xs[..., None] * g["U"] + ys[..., None] * g["V"] - g["C"]
    d = d / np.sqrt((d * d).sum(-1))[..., None]
    Cy = g["C"][1]
    assert (d[..., 1] < 0).all(), "every pixel looks down at the floor"
    first = Cy / -d[..., 1]
    D = (Cy + 2.0) / -d[..., 1]
    X = g["C"] + D[..., None] * d          # the terminal's mirror image; its x and z are the terminal's
    rgb = 0.8 * np.stack([0.5 + 0.2 * X[..., 0], 0.5 + 0.2 * X[..., 2], np.full((h, w), 0.5)], -1)
    rgb = rgb.astype(np.float32)
    up = np.broadcast_to(np.float32((0, 1, 0)), (h, w, 3)).copy()
    base = {"rgb": rgb, "var": np.zeros((h, w), np.float32), "count": 1.0,
            "lum2": (lum(rgb.astype(np.float64)) ** 2).astype(np.float32)}
    return (dict(base, normal=up, depth=first.astype(np.float32)),
            dict(base, normal=-up, depth=D.astype(np.float32), bounces=np.ones((h, w), np.float32)))
