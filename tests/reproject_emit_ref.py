"""A numpy restatement of rt_reproject_emit, written from the definition pinned in include/rt_abi.h
(not from the kernel) as a delta on tests/reproject_ref.py's: the same geometry, decisions and
fragile flags, with every frame's pixel entering as z = (rgb - emission) / (1 - coverage) and
v_z = var / (1 - coverage)^2, a pixel of coverage 1 or of non-finite emission neither a tap nor a
taker of history, and the current frame's emission added back to the blend.  dt=np.float64 is the
reference, dt=np.float32 measures what fp32 arithmetic alone costs.

It is written out in full rather than as a call of reproject_ref.reproject on transformed planes:
that function rounds its input planes to fp32 on entry, which would put an fp32 rounding of z into
the fp64 reference.  With zero emission and coverage it must return reproject_ref.reproject's
values exactly (tests/test_reproject_emit_ref.py), which holds the shared part to the parent's.

fixture() builds the tests' frames from reproject_ref.fixture(): see there."""
import numpy as np

from tests import reproject_ref as R

FRAGILE_REL, FRAGILE_CAP = R.FRAGILE_REL, R.FRAGILE_CAP
LIGHT = (15.0, 12.0, 9.0)   # emission of a fully covered pixel


def reproject_emit(gp, prev, gc, cur, max_history=0.0, depth_tol=0.0, normal_tol=0.0, min_weight=0.0,
                   dt=np.float64):
    """gp, gc, prev, cur as reproject_ref.reproject's, both frames also with "emission" [h, w, 3]
    and "coverage" [h, w].  -> {"rgb", "var", "count" (dtype dt), "history", "fragile" (bool)}"""
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
                 & np.isfinite(e_c).all(-1) & np.isfinite(cov_c) & (cov_c >= 0) & (cov_c < 1))
        k_c = np.where(valid, dt(1) - cov_c, dt(1)).astype(dt)
        z_c = (c - e_c) / k_c[..., None]          # subtract, then divide
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
        S, sn, sv = np.zeros((h, w), dt), np.zeros((h, w), dt), np.zeros((h, w), dt)
        sc = np.zeros((h, w, 3), dt)
        for b in (0, 1):
            for a in (0, 1):
                qx, qy = x0 + a, y0 + b
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                cq, vq, nq, dq = cq_all[cy, cx], vq_all[cy, cx], nq_all[cy, cx], dq_all[cy, cx]
                eq, covq = eq_all[cy, cx], covq_all[cy, cx]
                plain = (hist & inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & np.isfinite(nq) & (nq > 0)
                         & (dq > 0) & np.isfinite(eq).all(-1) & (covq >= 0) & (covq < 1))
                dd = np.abs(dq - d1)
                dn = n_p - nrm_q_all[cy, cx]
                dn2 = _dot(dn, dn)
                ok = plain & (dd <= depth_tol * d1) & (dn2 <= normal_tol)
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
        fragile |= hist & (np.abs(S - min_weight) <= FRAGILE_REL * min_weight)
        hist = hist & (S >= min_weight)
        cap = (np.float32(max_history).astype(dt) if max_history > 0 else dt(8) * nc) + np.zeros((h, w), dt)
        n_raw = sn / S
        fragile |= hist & (np.abs(n_raw - cap) <= FRAGILE_REL * cap)
        nh = np.minimum(n_raw, cap)
        zh, vh = sc / S[..., None], sv / (S * S)
        n = nh + nc
        z_blend = (nh[..., None] * zh + nc[..., None] * z_c) / n[..., None]
        v_blend = (nh * nh * vh + nc * nc * vz_c) / (n * n)
        o_rgb = k_c[..., None] * z_blend + e_c     # multiply-add: re-lit by the current emission
        o_var = k_c * k_c * v_blend
    return {"rgb": np.where(hist[..., None], o_rgb, c), "var": np.where(hist, o_var, v),
            "count": np.where(hist, n, nc), "history": hist, "fragile": fragile}


# ---- fixtures -----------------------------------------------------------------------------------

_fixtures = {}


def light_block(w, h):
    """(block, rim) masks: a block of fully covered pixels on the far plane and the one-pixel rim
    around it, the rim one or two columns right of the step edge (which falls at about w / 2);
    empty below 8 x 5"""
    ys, xs = np.mgrid[0:h, 0:w]
    if w < 8 or h < 5:
        return np.zeros((h, w), bool), np.zeros((h, w), bool)
    x0, y0 = w // 2 + 3, h // 3 + 1
    x1, y1 = x0 + max(w // 8, 1), y0 + max(h // 5, 1)
    block = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    grown = (xs >= x0 - 1) & (xs < x1 + 1) & (ys >= y0 - 1) & (ys < y1 + 1)
    return block, grown & ~block


def fixture(rt, w, h):
    """reproject_ref.fixture(rt, w, h) with the emission split's planes, built once per size and
    read-only.  Coverage takes values in {0, 1/8, .., 7/8, 1} only (exact in fp32, so coverage < 1
    has no fragile side): 0 on three pixels in four and a random eighth elsewhere, 1 in
    light_block()'s block, a random 1/8 .. 7/8 on its rim.  emission = coverage x LIGHT and
    rgb' = (1 - coverage) rgb + emission, so the surface radiance z of a partly covered pixel is
    the parent fixture's colour.  From 8 x 5 up one pixel of prev (far plane) and one of cur (near
    plane) have NaN emission."""
    if (w, h) in _fixtures:
        return _fixtures[(w, h)]
    fx = R.fixture(rt, w, h)
    block, rim = light_block(w, h)
    frames = []
    for k, name in enumerate(("prev", "cur")):
        rng = np.random.default_rng(7000 + 1000 * k + 10 * h + w)
        cov = np.where(rng.random((h, w)) < 0.25, rng.integers(1, 8, (h, w)), 0) / 8.0
        cov[rim] = rng.integers(1, 8, (h, w))[rim] / 8.0
        cov[block] = 1.0
        emission = cov[..., None] * np.array(LIGHT)
        with np.errstate(invalid="ignore"):
            rgb = (1.0 - cov)[..., None] * fx[name]["rgb"].astype(np.float64) + emission
        if w >= 8 and h >= 5:
            emission[(h // 2, w - 3) if k == 0 else (h // 2, w // 4)] = np.nan
        f = dict(fx[name], rgb=rgb.astype(np.float32), emission=emission.astype(np.float32),
                 coverage=cov.astype(np.float32))
        for a in f.values():
            a.setflags(write=False)
        frames.append(f)
    _fixtures[(w, h)] = dict(fx, prev=frames[0], cur=frames[1], block=block, rim=rim)
    return _fixtures[(w, h)]
