// rt_aov_kernel.inc — the feature kernel's text, included twice by rt_aov.hip: RT_AOV_EMIT 0 is
// k_aov, token for token what it was before the emission split existed (so its code
// generation cannot move); RT_AOV_EMIT 1 is its sibling k_aov_emit, which also counts the
// samples whose first hit is a front-facing light (L_j of rt_abi.h), sums their emission
// apart and sums the albedo of the other samples as surface_albedo.
//
// TREE: 0 record loop (quad-only scenes: the media set's code, which covers the lean one),
// 2 BVH2, 4 BVH4, 5 compressed BVH4 (any feature)
template <int TREE>
#if RT_AOV_EMIT
__global__ __launch_bounds__(256) void k_aov_emit(Params P, AovOut out, AovEmit em) {
#else
__global__ __launch_bounds__(256) void k_aov(Params P, AovOut out) {
#endif
  constexpr uint32_t FT = TREE == 0 ? (uint32_t)FT_MEDIA : (uint32_t)FT_ALL;
  __shared__ uint32_t lstack[kShortStack * 256];
  if constexpr (HAS(FT_NOISE)) stage_perlin(P.sc);
  __syncthreads();
  const DevScene& sc = P.sc;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const TravStack ts = {&lstack[threadIdx.x], P.ostack + gtid, P.stack_cols, kShortStack};
  (void)ts;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t lp = gtid; lp < P.npix; lp += stride) {
    Ids id;
    const uint32_t row_l = fdiv(lp, P.fd_width);
    id.lpix = lp;
    id.col = lp - row_l * (uint32_t)P.width;
    id.row = row_l * (uint32_t)P.nranks + (uint32_t)P.rank;
    id.gpix = id.row * (uint32_t)P.width + id.col;
    id.sample0 = 0;
    id.count = out.n;
    f3 asum = mk3(0, 0, 0), nsum = mk3(0, 0, 0);
    float dsum = 0.0f;
    int32_t kind0 = -1;
#if RT_AOV_EMIT
    f3 esum = mk3(0, 0, 0), ssum = mk3(0, 0, 0);
    uint32_t nlight = 0;
#endif
    for (uint32_t j = 0; j < out.n; ++j) {
      const rt_u32x4 r = rt_rng_draw(P.seed, id.gpix, j, RT_STREAM_CAMERA);
      f3 o, d;
      float time;
      camera_ray_r<0>(P, id, j, r, o, d, time);
      Trav tr;
      trav_init<FT>(sc, o, d, time, tr);
      if constexpr (TREE == 0) {
        trav_brute<FT, true>(sc, nullptr, o, d, time, 0.001f, tr);
      } else {
        do {  // a near-edge rejection ends a round early (retest_near), as trace_world
          trav_steps<false, FT, TREE != 2, TREE == 5>(sc, nullptr, false, ts, o, d, time, 0.001f, tr,
                                                      0x7FFFFFFF);
          retest_near<FT>(sc, o, d, 0.001f, tr);
        } while (tr.cur != TRAV_DONE);
      }
      Hit h = tr.best;
      const uint32_t ref = h.ref;
      f3 alb = mk3(P.bg[0], P.bg[1], P.bg[2]), n = mk3(0, 0, 0);  // a miss: camera.go:300-302
      float depth = 0.0f;
      int32_t kind = -1;
#if RT_AOV_EMIT
      bool lit = false;  // L_j
#endif
      if (ref != PRIM_NONE) {
        // finish_hit's refinements of the winning hit (no media, no trace)
#ifndef RT_NO_TRI_REFINE
        if (HAS(FT_TRI) && (ref >> 30) == PRIM_TRI)
          refine_tri_hit(sc, ref & 0x3FFFFFFFu, o, d, h.t, h.u, h.v);
#endif
#ifdef RT_SPHERE32_LEAVES
        if (HAS(FT_SPHERE) && (ref >> 30) == PRIM_SPHERE && h.v >= 0.0f)
          refine_sphere_hit(sc, ref & 0x3FFFFFFFu, o, d, time, h.t);
#endif
        // shade_core's hit record: r.At(t) snapped onto the surface, the outward normal,
        // setFaceNormal (hittable.go:27-34), and the texture coordinates
        const float t = h.t;
        float u = h.u, v = h.v;
        f3 p = o + d * t;
        const uint32_t type = ref >> 30, idx = ref & 0x3FFFFFFFu;
        f3 nout;
        int mat;
        if (HAS(FT_SPHERE) && type == PRIM_SPHERE) {
          const F4 cr = sc.sph_cr[idx], mv = sc.sph_mv[idx];
          const f3 cc = xyz(cr) + xyz(mv) * time;
          const double cx = (double)cr.x + (double)time * (double)mv.x;
          const double cy = (double)cr.y + (double)time * (double)mv.y;
          const double cz = (double)cr.z + (double)time * (double)mv.z;
          const double ex = (double)p.x - cx, ey = (double)p.y - cy, ez = (double)p.z - cz;
          const double rr = (double)cr.w;
          const float dn = (float)(rr * rr - (ex * ex + ey * ey + ez * ez));
          const f3 e = p - cc;
          const float le = length(e);
          const f3 nu = e * rcp(le);
          p = p + nu * (dn * rcp(fabsf(cr.w) + le));
          nout = cr.w < 0.0f ? -nu : nu;  // (p - c) / r objects.go:102
          mat = (int)fbits(mv.w);
          if (sc.mats[mat]._pad != 0.0f) {  // calculateSphereUV objects.go:44-50
            const F2 rs = sc.sph_uv[idx];
            const f3 no = mk3(rs.x * nout.x - rs.y * nout.z, nout.y, rs.y * nout.x + rs.x * nout.z);
            const float theta = acosf(-no.y);
            const float phi = atan2f(-no.z, no.x) + kPi;
            u = phi * (0.5f * kInvPi);
            v = theta * kInvPi;
          }
        } else if (!HAS(FT_TRI) || type == PRIM_QUAD) {
          const F4* q = sc.quad + 5 * (size_t)idx;
          nout = xyz(q[3]);
          p = p - nout * (dot(nout, p) - q[0].w);  // onto the plane n.p = D
          mat = (int)fbits(q[2].w);
          if (HAS(FT_BOX) && u < 0.0f) {  // a box leaf's face: alpha, beta at this p
            if (sc.mats[mat]._pad != 0.0f) {
              const f3 pp = p - xyz(q[0]), w = xyz(q[4]);
              u = dot(w, cross(pp, xyz(q[2])));
              v = dot(w, cross(xyz(q[1]), pp));
            } else {
              u = v = 0.0f;
            }
          }
        } else {
          nout = tri_normal(sc, idx, u, v);
          mat = (int)fbits(sc.tri[3 * (size_t)idx].w);
          const uint32_t tf = fbits(sc.tri[3 * (size_t)idx + 2].w);
          if (tf & TRI_HAS_UV) {  // objects.go:437-446
            const F4* at = sc.tri_attr + 6 * (size_t)idx;
            const float w = 1.0f - u - v;
            const float tu = w * at[4].x + u * at[4].z + v * at[5].x;
            const float tv = w * at[4].y + u * at[4].w + v * at[5].y;
            u = tu;
            v = tv;
          }
        }
        const bool ff = dot(d, nout) < 0;
        n = ff ? nout : -nout;
        const DevMaterial M = sc.mats[mat];
        kind = M.kind;
        if (M.kind == RT_MAT_METAL) alb = xyz(M.albedo);
        else if (M.kind == RT_MAT_DIELECTRIC) alb = mk3(1, 1, 1);
        else if (M.kind == RT_MAT_DIFFUSE_LIGHT && !ff) alb = mk3(0, 0, 0);  // materials.go:150-155
        else alb = tex_value<FT>(sc, M.tex, u, v, p);
        depth = t * length(d);
#if RT_AOV_EMIT
        lit = M.kind == RT_MAT_DIFFUSE_LIGHT && ff;
#endif
      }
#if RT_AOV_EMIT
      if (lit) {
        // what the render adds for this sample: a light does not scatter, so rayColor returns
        // its emission (camera.go:312-314) before the clampContribution of camera.go:330
        esum = esum + alb;
        ++nlight;
      } else {
        ssum = ssum + alb;
      }
#endif
      asum = asum + alb;
      nsum = nsum + n;
      dsum += depth;
      if (j == 0) kind0 = kind;
    }
    const float inv = 1.0f / (float)out.n;
    if (out.albedo) {
      out.albedo[3 * (size_t)lp + 0] = asum.x * inv;
      out.albedo[3 * (size_t)lp + 1] = asum.y * inv;
      out.albedo[3 * (size_t)lp + 2] = asum.z * inv;
    }
    if (out.normal) {
      out.normal[3 * (size_t)lp + 0] = nsum.x * inv;
      out.normal[3 * (size_t)lp + 1] = nsum.y * inv;
      out.normal[3 * (size_t)lp + 2] = nsum.z * inv;
    }
    if (out.depth) out.depth[lp] = dsum * inv;
    if (out.material) out.material[lp] = kind0;
#if RT_AOV_EMIT
    if (em.emission) {
      em.emission[3 * (size_t)lp + 0] = esum.x * inv;
      em.emission[3 * (size_t)lp + 1] = esum.y * inv;
      em.emission[3 * (size_t)lp + 2] = esum.z * inv;
    }
    if (em.surface_albedo) {
      em.surface_albedo[3 * (size_t)lp + 0] = ssum.x * inv;
      em.surface_albedo[3 * (size_t)lp + 1] = ssum.y * inv;
      em.surface_albedo[3 * (size_t)lp + 2] = ssum.z * inv;
    }
    // a true division (the build's fp32 divide is not correctly rounded): through fp64, whose
    // 53 bits >= 2 * 24 + 2 make the second rounding innocuous, so nlight == n gives 1.0f
    if (em.coverage) em.coverage[lp] = (float)((double)nlight / (double)out.n);
#endif
  }
}
