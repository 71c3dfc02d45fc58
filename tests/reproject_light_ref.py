"""A numpy restatement of rt_reproject_light, written from the definition pinned in include/rt_abi.h
(not from the kernel) as a delta on tests/reproject_emit_ref.py's: the same geometry and tap
weights, with a second weight sum over the light taps (the surface taps and the fully covered
previous pixels) that blends emission and coverage as history planes of their own, and the pixel
re-lit from the blended planes.  dt=np.float64 is the reference, dt=np.float32 measures what fp32
arithmetic alone costs.

One case of the issue's text was settled here, before the header was written.  It made a light
tap of every geometrically valid previous pixel with finite emission and 0 <= coverage <= 1,
whatever its rgb and var.  A previous pixel of NaN colour with zero emission and coverage would
then be a light tap and no surface tap: m_h > n_h, out.count = max(n_h, m_h) + n_c is no longer
rt_reproject's n_h + n_c, and the zero-split identity the same text demands fails on the parent's
own fixtures (which hold NaN and Inf colours).  So a light tap also needs finite rgb_q and var_q:
it is rt_reproject's tap with finite emission and coverage in [0, 1], and a surface tap is a light
tap with coverage < 1, exactly rt_reproject_emit's.  A poisoned previous pixel gives no history of
either kind.

The fragile flags are reproject_emit_ref.py's (the parent's decisions) plus
  S_l >= min_weight   |S_l - min_weight| <= 1e-3 min_weight
  m against the cap   |sum beta n_q / S_l - cap| <= 1e-3 cap
Coverage takes eighths only in the fixtures, so coverage < 1 and <= 1 have no fragile side.

fixture() is reproject_emit_ref.fixture: a block of coverage 1, a rim in eighths, a NaN emission
per frame."""
import numpy as np

from tests import reproject_emit_ref as E
from tests import reproject_ref as R

FRAGILE_REL, FRAGILE_CAP = R.FRAGILE_REL, R.FRAGILE_CAP
LIGHT = E.LIGHT
KEYS = ("rgb", "var", "count", "emission", "coverage")
fixture = E.fixture


def reproject_light(gp, prev, gc, cur, max_history=0.0, depth_tol=0.0, normal_tol=0.0, min_weight=0.0,
                    dt=np.float64):
    """gp, gc, prev, cur as reproject_emit_ref.reproject_emit's.  -> {"rgb", "var", "count",
    "emission", "coverage" (dtype dt), "history" (bool: n_h > 0, surface history found),
    "light_history" (bool: m_h > 0), "blend" (bool: the pixel is not passed through), "fragile"}"""
    h, w = np.shape(cur["rgb"])[:2]
    _dot = R._dot

    def vec(a):  # what the kernel is handed: fp32
        return np.asarray(a, np.float64).astype(np.float32).astype(dt)

    def opt(value, default):
        return np.float32(value if value > 0 else default).astype(dt)

    D, Ac, Uc, Vc = vec(gc["C"] - gp["C"]), vec(gc["P00"] - gc["C"]), vec(gc["U"]), vec(gc["V"])
    Ap, Up, Vp = vec(gp["P00"] - gp["C"]), vec(gp["U"]), vec(gp["V"])
    depth_tol, normal_tol = opt(depth_tol, 0.05), opt(normal_tol, 0.1)
    min_weight = opt(min_weight, 0.01)

    def planes(f):
        def a(x):
            return np.asarray(x, np.float32).astype(dt)
        var = np.zeros((h, w), dt) if f.get("var") is None else a(f["var"])
        cnt = f.get("count")
        cnt = (np.full((h, w), np.float32(0.0 if cnt is None else cnt)).astype(dt) if cnt is None or np.ndim(cnt) == 0
               else a(cnt))
        return a(f["rgb"]), var, cnt, a(f["normal"]), a(f["depth"]), a(f["emission"]), a(f["coverage"])

    c, v, nc, n_p, d_p, e_c, cov_c = planes(cur)
    cq_all, vq_all, nq_all, nrm_q_all, dq_all, eq_all, covq_all = planes(prev)
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.astype(dt), ys.astype(dt)
    with np.errstate(all="ignore"):
        valid = (np.isfinite(c).all(-1) & np.isfinite(v) & np.isfinite(nc) & (nc > 0)
                 & np.isfinite(e_c).all(-1) & (cov_c >= 0) & (cov_c <= 1))
        surf_c = valid & (cov_c < 1)                      # the current pixel has a surface sample
        w_c = np.where(cov_c < 1, nc, dt(0)).astype(dt)
        k_c = np.where(surf_c, dt(1) - cov_c, dt(1)).astype(dt)
        z_c = (c - e_c) / k_c[..., None]                  # subtract, then divide
        vz_c = v / (k_c * k_c)
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
        u = np.where(hist, np.clip(np.nan_to_num(u, nan=-2.0), -2, w + 1), -2).astype(dt)
        vv = np.where(hist, np.clip(np.nan_to_num(vv, nan=-2.0), -2, h + 1), -2).astype(dt)
        near = ((np.abs(u - np.round(u)) <= FRAGILE_REL) | (np.abs(vv - np.round(vv)) <= FRAGILE_REL))
        reach = (u >= -1 - FRAGILE_REL) & (u <= w + FRAGILE_REL) & (vv >= -1 - FRAGILE_REL) & (vv <= h + FRAGILE_REL)
        fragile |= hist & near & reach
        u0, v0 = np.floor(u), np.floor(vv)
        x0, y0 = u0.astype(np.int64), v0.astype(np.int64)
        bu, bv = (dt(1) - (u - u0), u - u0), (dt(1) - (vv - v0), vv - v0)
        zero = lambda: np.zeros((h, w), dt)  # noqa: E731
        S, sn, sv, sc = zero(), zero(), zero(), np.zeros((h, w, 3), dt)     # the surface taps
        Sl, sm, sk, se = zero(), zero(), zero(), np.zeros((h, w, 3), dt)    # the light taps
        for b in (0, 1):
            for a in (0, 1):
                qx, qy = x0 + a, y0 + b
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                cq, vq, nq, dq = cq_all[cy, cx], vq_all[cy, cx], nq_all[cy, cx], dq_all[cy, cx]
                eq, covq = eq_all[cy, cx], covq_all[cy, cx]
                plain = (hist & inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & np.isfinite(nq) & (nq > 0)
                         & (dq > 0) & np.isfinite(eq).all(-1) & (covq >= 0) & (covq <= 1))
                dd = np.abs(dq - d1)
                dn = n_p - nrm_q_all[cy, cx]
                dn2 = _dot(dn, dn)
                okl = plain & (dd <= depth_tol * d1) & (dn2 <= normal_tol)   # a light tap
                ok = okl & (covq < 1)                                        # a surface tap
                fragile |= plain & (np.abs(dd - depth_tol * d1) <= FRAGILE_REL * depth_tol * d1)
                fragile |= plain & (np.abs(dn2 - normal_tol) <= FRAGILE_REL * normal_tol)
                beta = np.where(ok, bu[a] * bv[b], dt(0)).astype(dt)
                k_q = np.where(ok, dt(1) - covq, dt(1)).astype(dt)
                z_q = (np.where(ok[..., None], cq, dt(0)) - np.where(ok[..., None], eq, dt(0))) / k_q[..., None]
                vz_q = np.where(ok, vq, dt(0)) / (k_q * k_q)
                S += beta
                sc += beta[..., None] * z_q
                sv += beta * beta * vz_q
                sn += beta * np.where(ok, nq, dt(0))
                bl = np.where(okl, bu[a] * bv[b], dt(0)).astype(dt)
                Sl += bl
                se += bl[..., None] * np.where(okl[..., None], eq, dt(0))
                sk += bl * np.where(okl, covq, dt(0))
                sm += bl * np.where(okl, nq, dt(0))
        fragile |= hist & (np.abs(S - min_weight) <= FRAGILE_REL * min_weight)
        fragile |= hist & (np.abs(Sl - min_weight) <= FRAGILE_REL * min_weight)
        hs, hl = hist & (S >= min_weight), hist & (Sl >= min_weight)
        cap = (np.float32(max_history).astype(dt) if max_history > 0 else dt(8) * nc) + np.zeros((h, w), dt)
        n_raw, m_raw = sn / S, sm / Sl
        fragile |= hs & (np.abs(n_raw - cap) <= FRAGILE_REL * cap)
        fragile |= hl & (np.abs(m_raw - cap) <= FRAGILE_REL * cap)
        nh = np.where(hs, np.minimum(n_raw, cap), dt(0)).astype(dt)
        mh = np.where(hl, np.minimum(m_raw, cap), dt(0)).astype(dt)
        zh = np.where(hs[..., None], sc / S[..., None], dt(0))
        vh = np.where(hs, sv / (S * S), dt(0))
        eh = np.where(hl[..., None], se / Sl[..., None], dt(0))
        kh = np.where(hl, sk / Sl, dt(0))
        blend = (hs | hl) & (hs | (w_c > 0))
        n = nh + w_c
        z_blend = (nh[..., None] * zh + w_c[..., None] * z_c) / n[..., None]
        v_blend = (nh * nh * vh + w_c * w_c * vz_c) / (n * n)
        m = mh + nc
        k_out = (mh * kh + nc * cov_c) / m
        e_out = (mh[..., None] * eh + nc[..., None] * e_c) / m[..., None]
        o_rgb = (dt(1) - k_out)[..., None] * z_blend + e_out     # multiply-add: re-lit from the blended planes
        o_var = (dt(1) - k_out) * (dt(1) - k_out) * v_blend
        o_cnt = np.maximum(nh, mh) + nc
    b3 = blend[..., None]
    return {"rgb": np.where(b3, o_rgb, c), "var": np.where(blend, o_var, v), "count": np.where(blend, o_cnt, nc),
            "emission": np.where(b3, e_out, e_c), "coverage": np.where(blend, k_out, cov_c),
            "history": hs, "light_history": hl, "blend": blend, "fragile": fragile}
