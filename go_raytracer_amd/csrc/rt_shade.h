// rt_shade.h — what a vertex evaluates besides geometry: textures (with the Perlin tables
// in LDS), interpolated triangle normals, light sampling and light pdfs over the light
// table, and the lean light kinds' single quad light (LeanLightRegs; its pdf is the record
// loop's axis form, rt_records.h).
#pragma once
#include "rt_records.h"

namespace rt {

// ---------------------------------------------------------------- shading --
// Texture.Value texture.go:10-125 (checker chains resolved iteratively)
// Perlin tables of perlin 0 in LDS (kernels with FT_NOISE stage them at start,
// stage_perlin): ranvec as float4 and the three byte permutations, the same layout
// as DevPerlin.  The noise evaluation is 7 octaves x 8 lattice corners of dependent
// table reads (book2's marble sphere, C4): from HBM/L2 they were latency-bound (C4
// -23 % with texture evaluation ablated).  One code path serves both copies: the
// tables are reached through a generic pointer (LDS for perlin 0, global for the
// others), so the hardware routes each flat load (a second, address-space-specific
// copy of the noise code doubled the kernel's spills).
__shared__ DevPerlin g_perlin;

// before the kernel's first __syncthreads (stage_nodes), every thread of the block
RT_D void stage_perlin(const DevScene& sc) {
  if (sc.n_perlins <= 0) return;
  const F4* src = (const F4*)sc.perlins;
  F4* dst = (F4*)&g_perlin;
  for (int i = threadIdx.x; i < (int)(sizeof(DevPerlin) / 16); i += blockDim.x) dst[i] = src[i];
}

// PL: const DevPerlin* (global or LDS, the all-features kernel: flat loads) or
// LdsPerlin (table 0 in LDS, the feature-set kernels: ds_read, 3 % faster on C4
// than flat loads and fewer spills)
typedef __attribute__((address_space(3))) const DevPerlin* LdsPerlin;
template <typename PL>
RT_D float perlin_noise(PL pl, f3 p) {  // perlin.go:34-54
  float fx = floorf(p.x), fy = floorf(p.y), fz = floorf(p.z);
  float u = p.x - fx, v = p.y - fy, w = p.z - fz;
  int i = (int)fx, j = (int)fy, k = (int)fz;
  float uu = u * u * (3 - 2 * u), vv = v * v * (3 - 2 * v), ww = w * w * (3 - 2 * w);
  const int pi[2] = {pl->perm[0][i & 255], pl->perm[0][(i + 1) & 255]},
            pj[2] = {pl->perm[1][j & 255], pl->perm[1][(j + 1) & 255]},
            pk[2] = {pl->perm[2][k & 255], pl->perm[2][(k + 1) & 255]};
  // the corner weights i*uu + (1-i)*(1-uu) of perlin.go:49-51 for i = 0, 1: since uu is in
  // [0, 1], 0*uu + (1-uu) and uu + 0*(1-uu) are exactly 1-uu and uu (hipcc kept the 0*x
  // terms, which it may not drop for a NaN x: 12 fma per noise call, 84 per turbulence)
  const float wx[2] = {1 - uu, uu}, wy[2] = {1 - vv, vv}, wz[2] = {1 - ww, ww};
  float accum = 0.0f;
  for (int di = 0; di < 2; ++di)
    for (int dj = 0; dj < 2; ++dj)
      for (int dk = 0; dk < 2; ++dk) {
        const int gi = pi[di] ^ pj[dj] ^ pk[dk];
        const F4 g = {pl->ranvec[gi].x, pl->ranvec[gi].y, pl->ranvec[gi].z, 0.0f};
        f3 wt = mk3(u - (float)di, v - (float)dj, w - (float)dk);
        accum += wx[di] * wy[dj] * wz[dk] * dot(xyz(g), wt);
      }
  return accum;
}
template <typename PL>
RT_D float perlin_turb(PL pl, f3 p, int depth) {  // perlin.go:57-69
  float accum = 0.0f, weight = 1.0f;
#pragma unroll 1  // unrolled, the scheduler hoists every octave's table reads
  for (int i = 0; i < depth; ++i) {
    accum += weight * perlin_noise(pl, p);
    weight *= 0.5f;
    p = p * 2.0f;
  }
  return fabsf(accum);
}

template <uint32_t FT>
RT_D f3 tex_value(const DevScene& sc, int tex, float u, float v, f3 p) {
  for (int guard = 0; guard < 64; ++guard) {
    const DevTexture T = sc.texs[tex];
    if (!HAS(FT_CHECKER | FT_IMAGE | FT_NOISE) || T.kind == RT_TEX_SOLID) return xyz(T.color);
    if (HAS(FT_CHECKER) && T.kind == RT_TEX_CHECKER) {  // texture.go:50-60
      float inv = T.color.w;
      int x = (int)floorf(inv * p.x), y = (int)floorf(inv * p.y), z = (int)floorf(inv * p.z);
      tex = ((x + y + z) % 2 == 0) ? T.a : T.b;
      continue;
    }
    if (HAS(FT_IMAGE) && (!HAS(FT_NOISE) || T.kind == RT_TEX_IMAGE)) {  // texture.go:70-86 + PixelData imageLoader.go:52-62
      const DevImage im = sc.images[T.a];
      if (im.h <= 0) return mk3(0, 1, 1);
      // fmod(u, 1) is u - trunc(u) exactly (no rounding for any finite u; inf and NaN give
      // NaN either way), without the library fmodf's loop and selects
      float uu = fabsf(u - truncf(u));
      float vv = 1.0f - fabsf(v - truncf(v));
      float fi = uu * (float)(im.w - 1), fj = vv * (float)(im.h - 1);
      int i = isnan(fi) ? 0 : (int)fi, j = isnan(fj) ? 0 : (int)fj;
      i = min(max(i, 0), im.w);
      j = min(max(j, 0), im.h);
      long idx = (long)j * im.w + i;
      if (idx >= (long)im.w * im.h) return mk3(1.0f, 0.0f, 1.0f);  // magenta
      const uint8_t* px = sc.texels + im.offset + 3 * idx;
      const float s = 1.0f / 255.0f;
      return mk3((float)px[0] * s, (float)px[1] * s, (float)px[2] * s);
    }
    if (!HAS(FT_NOISE)) return mk3(0, 0, 0);
    // noise, texture.go:112-125 (perlin 0 from its LDS copy when staged)
    const float scale = T.color.w;
    float s;
    auto eval = [&](auto pl) {
      if (T.variant == RT_NOISE_MARBLE) return 0.5f * (1.0f + sinf(scale * p.z + 10.0f * perlin_turb(pl, p, 7)));
      if (T.variant == RT_NOISE_TURBULENT) return perlin_turb(pl, p, 7);
      return 0.5f * (1.0f + perlin_noise(pl, p * scale));
    };
    if constexpr (FT == FT_ALL)
      s = eval((T.a == 0 && sc.n_perlins > 0) ? (const DevPerlin*)&g_perlin : sc.perlins + T.a);
    else
      s = eval((LdsPerlin)&g_perlin);  // table 0 (render_impl picks FT_ALL otherwise)
    return mk3(s, s, s);
  }
  return mk3(0, 0, 0);
}

// Triangle.interpolateNormal objects.go:389-405
RT_D f3 tri_normal(const DevScene& sc, uint32_t idx, float bu, float bv) {
  const F4* at = sc.tri_attr + 6 * (size_t)idx;
  uint32_t flags = fbits(sc.tri[3 * (size_t)idx + 2].w);
  if (!(flags & TRI_HAS_NORMALS)) return xyz(at[0]);
  float w = 1.0f - bu - bv;
  f3 n = xyz(at[1]) * w + xyz(at[2]) * bu + xyz(at[3]) * bv;
  return unit(n);
}

// light PdfValue: sphere objects.go:52-62, quad :152-160, triangle :356-367
template <uint32_t FT>
RT_D float prim_pdf(const DevScene& sc, uint32_t ref, int li, f3 origin, f3 dir) {
  uint32_t type = ref >> 30, idx = ref & 0x3FFFFFFFu;
  if (HAS(FT_SPHERE) && type == PRIM_SPHERE) {
    float t;
    if (!hit_sphere(sc, idx, origin, dir, 0.0f, 0.0001f, kInf, t)) return 0.0f;
    const F4 cr = sc.sph_cr[idx];
    f3 oc = xyz(cr) - origin;
    float dist2 = dot(oc, oc);
    float cmax = fsqrt(1.0f - cr.w * cr.w * rcp(dist2));
    return rcp(2.0f * kPi * (1.0f - cmax));
  }
  float t, u, v, area;
  f3 n;
  uint32_t miss = 0u;  // quad lights: the reject mask of the branch-free test
  if (!HAS(FT_TRI) || type == PRIM_QUAD) {
    // the light's leaf-record copy (uniform index: scalar loads) and the traversal's quad test
    F4 rec[4];
    if (FT != FT_ALL) {
      const F4* lr = kparams()->sc.light_recs + 8 * (size_t)__builtin_amdgcn_readfirstlane(li);
      rec[0] = ld_cst(lr), rec[1] = ld_cst(lr + 1), rec[2] = ld_cst(lr + 2), rec[3] = ld_cst(lr + 3);
    } else {
      const F4* lr = sc.light_recs + 8 * (size_t)li;
      rec[0] = lr[0], rec[1] = lr[1], rec[2] = lr[2], rec[3] = lr[3];
    }
    miss = hit_quad_rec_m(rec, origin, dir, 0.001f, kInf, t, u, v);
    n = xyz(rec[1]);
    area = rec[2].w;
  } else {
    if (!hit_tri(sc, idx, origin, dir, 0.001f, kInf, t, u, v)) return 0.0f;
    n = tri_normal(sc, idx, u, v);
    area = sc.tri[3 * (size_t)idx + 1].w;
  }
  // dist2 / (cosine * area) with dist2 = t^2 |dir|^2, cosine = |dir.n| / |dir|; +0 on a
  // miss (the mask clears every bit of whatever the missed test's t gave)
  const float dd = dot(dir, dir);
  return bitsf(and_not(fbits((t * t * dd) * fsqrt(dd) * rcp(fabsf(dot(dir, n)) * area)), miss));
}

// HittableList.PdfValue hittable.go:89-97 over the flattened light table
// (the light table's size and address re-read from the kernel-argument segment, kparams:
// held in SGPRs across the fused loop they were spilled to VGPR lanes, one v_readlane each
// per scattering vertex)
template <uint32_t FT>
RT_D float lights_pdf(const DevScene& sc, f3 origin, f3 dir) {
  float sum = 0.0f;
  const cst_params* kp = kparams();
  const int n_lights = kp->sc.n_lights;
  const DevLight* lights = kp->sc.lights;
  for (int i = 0; i < n_lights; ++i) {  // uniform loop: the table entry is a scalar load
    const F4 e = FT != FT_ALL ? ld_cst((const F4*)lights + __builtin_amdgcn_readfirstlane(i))
                              : ((const F4*)lights)[i];
    const uint32_t ref = fbits(e.x);
    if (ref == PRIM_NONE) continue;
    sum += e.z * prim_pdf<FT>(sc, ref, i, origin, dir);
  }
  return sum;
}

// HittableList.Random hittable.go:98-103 + sphere/quad/Triangle.Random
template <uint32_t FT>
RT_D f3 lights_random(const DevScene& sc, f3 origin, const rt_u32x4& r) {
  const float s0 = rt_unit_f(r.v[2]), s1 = rt_unit_f(r.v[3]);
  const cst_params* kp = kparams();  // (as lights_pdf)
  const int n_lights = kp->sc.n_lights;
  const DevLight* lights = kp->sc.lights;
  const F4* light_recs = kp->sc.light_recs;
  int lo = 0, hi = n_lights - 1;
  if (n_lights <= 0) return mk3(rt_unit_f(r.v[1]), s0, s1);  // vec.Random()
  const uint32_t u24 = rt_u24(r.v[1]);
  while (lo < hi) {  // last entry with lo24 <= u24
    int mid = (lo + hi + 1) >> 1;
    if (lights[mid].lo24 <= u24) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t ref =
      FT != FT_ALL && n_lights == 1 ? fbits(ld_cst((const F4*)lights).x) : lights[lo].ref;
  if (ref == PRIM_NONE) return mk3(rt_unit_f(r.v[1]), s0, s1);
  uint32_t type = ref >> 30, idx = ref & 0x3FFFFFFFu;
  if (HAS(FT_SPHERE) && type == PRIM_SPHERE) {  // sphere.Random + randomToSphere objects.go:63-80
    const F4 cr = sc.sph_cr[idx];
    f3 dir = xyz(cr) - origin;
    float dist2 = dot(dir, dir);
    Onb b = make_onb(dir);
    float z = 1.0f + s1 * (fsqrt(1.0f - cr.w * cr.w * rcp(dist2)) - 1.0f);
    float tt = fsqrt(1.0f - z * z);  // phi = 2*pi*s0
    return onb_transform(b, mk3(cos2pi(s0) * tt, sin2pi(s0) * tt, z));
  }
  if (!HAS(FT_TRI) || type == PRIM_QUAD) {  // quad.Random objects.go:161-165
    // the light record's Q, u, v; one light: a uniform index, so scalar loads
    F4 Q, U, V;
    if (FT != FT_ALL && n_lights == 1) {
      const F4* lr = light_recs + 4;
      Q = ld_cst(lr), U = ld_cst(lr + 1), V = ld_cst(lr + 2);
    } else {
      const F4* lr = light_recs + 8 * (size_t)lo + 4;
      Q = lr[0], U = lr[1], V = lr[2];
    }
    return (xyz(Q) + xyz(U) * s0 + xyz(V) * s1) - origin;
  }
  // Triangle.Random objects.go:369-385 (non-uniform barycentrics kept)
  const F4* tr = sc.tri + 3 * (size_t)idx;
  float r1 = s0, r2 = s1 * (1.0f - r1);
  f3 v0 = xyz(tr[0]), v1 = v0 + xyz(tr[1]), v2 = v0 + xyz(tr[2]);
  f3 p = v0 * (1.0f - r1 - r2) + v1 * r1 + v2 * r2;
  return p - origin;
}

// The light of a lean light kind (rt_device.h; KIND >= 1: one quad light on axis
// lean_light_axis(KIND), weight 1), read with 16-B scalar loads from the launch parameters --
// one address, no table entry, no record pointer -- where lights_random and lights_pdf chase
// kparams -> lights[i] -> light_recs.  The host matcher (host_records.cpp lean_light_of)
// guarantees what is left out here is an exact no-op.
// Two loads: the pdf's part (every vertex) first, before the vertex's basis and direction are
// worked out, and u, v in the half of the vertices that sample the light.
struct LeanLightRegs {
  F4 q, a, b;  // f[0..11]: Q | D', A | area, B | 0
};
RT_D LeanLightRegs lean_light_load() {
  const F4* lb = (const F4*)&kparams()->ll;
  return {ld_cst(lb), ld_cst(lb + 1), ld_cst(lb + 2)};
}
// lights_random for the kind: quad.Random objects.go:161-165 (the same expression)
RT_D f3 lean_light_random(const LeanLightRegs& L, f3 origin, const rt_u32x4& r) {
  const float s0 = rt_unit_f(r.v[2]), s1 = rt_unit_f(r.v[3]);
  const F4* lb = (const F4*)&kparams()->ll;
  const F4 U = ld_cst(lb + 3), V = ld_cst(lb + 4);
  return (xyz(L.q) + xyz(U) * s0 + xyz(V) * s1) - origin;
}
// lights_pdf for the kind: prim_pdf's quad test (hit_quad_rec_m), interval [0.001, +inf).
// With n = +-e_A the general test's n.d is +-d_A and n.o is +-o_A exactly, so t is the record
// loop's axis form (brute_half: D' = D / n_A, and |d_A| < 1e-8 makes t NaN, which the alpha /
// beta test rejects), and dot(dir, n) is +-d_A.  alpha and beta keep hit_quad_rec_m's three
// terms: the A_A = B_A = 0 term adds an exact zero, but a ray sampled at the light's edge
// (s0 or s1 = 0, one light sample in 2^23) lands on alpha or beta = +-0, whose sign decides
// the test (unit_ab_rej), and the zero term takes part in that sign: with the in-plane terms
// alone the 800 x 800 x 1024 Cornell image was not the general code's.
// The entry's weight is 1.
template <int KIND>
RT_D float lean_light_pdf(const LeanLightRegs& L, f3 o, f3 d) {
  constexpr int A = lean_light_axis(KIND);
  static_assert(A >= 0 && A < 3, "lean light: a kind with an axis");
  const float da = comp<A>(d);
  const float ia = bitsf(pick_by(fbits(rcp(da)), 0x7FC00000u, neg_mask(fabsf(da) - 1e-8f)));
  const float t = (L.q.w - comp<A>(o)) * ia;
  const f3 pp = (o + d * t) - xyz(L.q);
  const float alpha = dot(pp, xyz(L.a)), beta = dot(pp, xyz(L.b));
  const uint32_t miss = rec_reject_t(t, 0.001f, kInf, alpha, beta);
  const float dd = dot(d, d);
  return bitsf(and_not(fbits((t * t * dd) * fsqrt(dd) * rcp(fabsf(da) * L.a.w)), miss));
}

}  // namespace rt
