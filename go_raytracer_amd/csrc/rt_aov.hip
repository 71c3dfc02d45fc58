// rt_aov.hip — the feature pass: per-pixel albedo, shading normal, depth and material kind
// of the first hit of the render's own camera rays (rt_abi.h rt_render_aov), the guide
// buffers of the denoiser (rt_denoise.hip) and of any compositor or preview tool.
//
// k_aov: one lane per pixel, looping over the pixel's samples 0 .. n-1 in order and
// summing in registers (no atomics: the means are the same bits on every call).  The ray
// of sample j is start_sample's: rt_rng_draw(seed, gpix, j, RT_STREAM_CAMERA) through
// camera_ray_r.  The closest world hit is found in the structure the scene's fused render
// traverses (rt_render.hip aov_view): the record loop, the BVH2, the BVH4 or the compressed
// BVH4, all read through L1/L2 here (a feature ray per sample is ~1/10 of a path: no LDS
// scene cache).  The hit -> (p, n, material, u, v) evaluation restates shade_core's
// (rt_path.h) without touching it: the fused kernels are sensitive to code generation
// (DESIGN.md §9).  Constant media are not traced: they are transparent to this pass, unless the
// media mode is asked for (below).
//
// k_aov<TREE, true> (rt_render_aov_emit): the emission split of DESIGN.md §15.  It also counts
// the samples whose first hit is a front-facing light (L_j of rt_abi.h), sums their emission
// apart and sums the albedo of the other samples as surface_albedo.  One template: the EMIT
// instances are the instructions a separate kernel compiled to, the others differ from a
// kernel without the AovEmit argument in kernel-argument offsets only.
//
// k_aov<TREE, EMIT, true> (rt_render_aov_media): the first EVENT of the sample.  The
// media are laid over the closest world hit exactly as the render's vertex 0 lays them
// (trace_media with the camera draw's spare word: the render's own free-flight draws); a sample
// whose winner is a medium takes the phase material's albedo at the scatter point, no normal and
// the scatter's depth, and is counted into the `scatter` plane.  The MEDIA = false instances are
// the instructions they were (profiles/aov_media_device_code.txt); the dispatcher takes a MEDIA
// instance only for a scene that has media.
//
// k_aov<TREE, false, false, true> (rt_render_aov_spec): the first DIFFUSE hit of the
// sample.  While the hit is a dielectric or a metal of fuzz <= max_fuzz the lane scatters as the
// render's vertex k does (the same rt_rng_draw(seed, gpix, j, RT_STREAM(k, 0)), shade_core's
// expressions restated) and traces the next segment, a per-lane loop around the one
// trace-and-evaluate block; the planes are of the chain's terminal vertex, the albedo times the
// metals' on the way, the depth summed along the chain, and `bounces` counts the specular vertices
// passed.  SPEC only with EMIT = MEDIA = false; the SPEC = false instances are the instructions
// they were (profiles/aov_specular_device_code.txt).
//
// k_aov_fold<TREE, EMIT, PX, MEDIA>: the pass accumulator's feature fold (rt_accum.hip),
// the same samples (aov_sample is the one text of both kernels) summed into the accumulator's
// fp64 planes for all spp_sqrt^2 samples of a pass's seed, over a whole pass or its active pixels.
//
// The host half (DESIGN.md §11 "Host path"): the eight entries fill an AovRequest and aov_impl
// runs aov_check -> aov_plan -> aov_bind -> aov_launch -> aov_collect; aov_launch and
// aov_fold_enqueue choose the kernel instance through with_tree and with_flag.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <type_traits>
#include <vector>

#include "rt_hip_util.h"
#include "rt_host_units.h"
// the render's camera rays, traversal, record loop and textures: not its path state or
// shading core (rt_path.h)
#include "rt_camera.h"
#include "rt_trav.h"
#include "rt_records.h"
#include "rt_shade.h"

namespace rt {

struct AovOut {
  float* albedo;
  float* normal;
  float* depth;
  int32_t* material;
  uint32_t n;  // samples per pixel
};

// grid-stride above this many blocks: the tree kernels keep an overflow-stack column per
// launched lane (52 x 4 B: 27 MB at 512 blocks), the record loop has no stack
constexpr int kAovMaxBlocks = 1024, kAovMaxTreeBlocks = 512;

// the emission split's buffers (rt_abi.h rt_aov_emit), device pointers
struct AovEmit {
  float* emission;
  float* surface_albedo;
  float* coverage;
};

// The media mode's buffer (rt_abi.h rt_aov_media), a device pointer, and the accumulator's scatter
// counts (rt_accum.hip keeps them beside FeatPlanes).  They ride behind an argument the kernels
// already take, so that the MEDIA = false kernels take exactly the arguments they took: a
// trailing argument of an empty struct still occupies 8 bytes of the kernel-argument segment
// and moves the hidden arguments (blockDim, which these kernels read) behind it.
struct AovEmitMedia : AovEmit {
  float* scatter;
};
struct FeatPlanesMedia : FeatPlanes {
  uint32_t* nscatter;  // [npix], as nlight
};
// The specular mode's plane, its chain limits and the count of the chain segments traced (one
// device word, added to once by each wave that traced any), behind the same argument for the same reason
struct AovEmitSpec : AovEmit {
  float* bounces;                      // may be null
  unsigned long long* chain_segments;  // never null
  int32_t max_k;   // the last vertex a chain may reach: min(max_bounces, MaxDepth - 1)
  float max_fuzz;  // a metal is specular up to this fuzz
};
template <bool MEDIA, bool SPEC = false>
using AovEmitArg = std::conditional_t<SPEC, AovEmitSpec, std::conditional_t<MEDIA, AovEmitMedia, AovEmit>>;
template <bool MEDIA>
using FeatPlanesArg = std::conditional_t<MEDIA, FeatPlanesMedia, FeatPlanes>;

// A pixel's sums over its samples, in fp32 registers in sample order
struct AovSums {
  f3 asum, nsum;
  float dsum;
  int32_t kind0;  // the material kind of sample 0's hit, -1 on a miss
  f3 esum, ssum;  // EMIT only, as nlight
  uint32_t nlight;
  uint32_t nscatter;  // MEDIA only: the samples whose first event is a scatter in a medium
  uint32_t nspec;     // SPEC only: the specular vertices the samples' chains passed
};
RT_D AovSums aov_sums_zero() {
  return {mk3(0, 0, 0), mk3(0, 0, 0), 0.0f, -1, mk3(0, 0, 0), mk3(0, 0, 0), 0u, 0u, 0u};
}

// The camera ids of local pixel lp of the share, for `count` samples from sample 0
RT_D Ids aov_ids(const Params& P, uint32_t lp, uint32_t count) {
  Ids id;
  const uint32_t row_l = fdiv(lp, P.fd_width);
  id.lpix = lp;
  id.col = lp - row_l * (uint32_t)P.width;
  id.row = row_l * (uint32_t)P.nranks + (uint32_t)P.rank;
  id.gpix = id.row * (uint32_t)P.width + id.col;
  id.sample0 = 0;
  id.count = count;
  return id;
}

// Sample j of pixel id, added to s: the one text of the feature pass (k_aov) and of the
// accumulator's feature fold (k_aov_fold).
// TREE: 0 record loop (quad-only scenes: the media set's code, which covers the lean one),
// 2 BVH2, 4 BVH4, 5 compressed BVH4 (any feature)
// MEDIA: the first event, not the first surface: the render's vertex-0 trace_media on top of
// the world hit (finish_hit's order: the triangle refinement, then the media)
// SPEC (rt_abi.h rt_render_aov_spec): the loop below goes round again while the vertex is
// specular: vertex k < max_k, a dielectric or a metal of fuzz <= max_fuzz that does not scatter
// into its own surface.  The next ray is shade_core's for that vertex: the same draw, the same
// expressions, the snapped point (eta off a sphere) as the origin.  Only a hit is evaluated, and
// its material is the surface's own (MEDIA = false: no medium wins), so a chain lane reads no
// record of a PRIM_NONE hit and no material through a medium's id.  The evaluation stays in the
// loop's body, one text for the first hit and for every chain vertex, and is not a function of
// its own: as a callee with reference results it changed the register allocation of every
// existing instance; in place they are the instructions they were.
template <int TREE, bool EMIT, bool MEDIA, bool SPEC = false>
RT_D void aov_sample(const Params& P, const Ids& id, uint32_t j, const TravStack& ts, AovSums& s,
                     int32_t max_k = 0, float max_fuzz = 0.0f) {
  static_assert(!SPEC || (!EMIT && !MEDIA), "the specular mode: neither the emission split nor media");
  constexpr uint32_t FT = TREE == 0 ? (uint32_t)FT_MEDIA : (uint32_t)FT_ALL;
  const DevScene& sc = P.sc;
  (void)ts;
  const rt_u32x4 r = rt_rng_draw(P.seed, id.gpix, j, RT_STREAM_CAMERA);
  f3 o, d;
  float time;
  camera_ray_r<0>(P, id, j, r, o, d, time);
  // SPEC: the chain so far: the specular vertices passed, their attenuations' product T and the
  // length of their segments
  uint32_t k = 0u;
  f3 T = mk3(1, 1, 1);
  float dpre = 0.0f;
  for (;;) {  // (SPEC: once per segment of the chain; else once)
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
    if constexpr (MEDIA) {
      if (HAS(FT_TRI) && h.ref != PRIM_NONE && (h.ref >> 30) == PRIM_TRI)
        refine_tri_hit(sc, h.ref & 0x3FFFFFFFu, o, d, h.t, h.u, h.v);
      trace_media(P, o, d, time, 0.001f, id.gpix, j, 0u, rt_spare24(r), h);
    }
    const uint32_t ref = h.ref;
    f3 alb = mk3(P.bg[0], P.bg[1], P.bg[2]), n = mk3(0, 0, 0);  // a miss: camera.go:300-302
    float depth = 0.0f;
    int32_t kind = -1;
    bool lit = false;  // L_j
    if (ref != PRIM_NONE) {
      // finish_hit's refinements of the winning hit (no media, no trace)
      if constexpr (!MEDIA)
        if (HAS(FT_TRI) && (ref >> 30) == PRIM_TRI)
          refine_tri_hit(sc, ref & 0x3FFFFFFFu, o, d, h.t, h.u, h.v);
      // shade_core's hit record: r.At(t) snapped onto the surface, the outward normal,
      // setFaceNormal (hittable.go:27-34), and the texture coordinates
      const float t = h.t;
      float eta = 0.0f;  // SPEC, spheres: shade_core's offset of the next origin off the surface
      float u = h.u, v = h.v;
      f3 p = o + d * t;
      const uint32_t type = ref >> 30, idx = ref & 0x3FFFFFFFu;
      f3 nout;
      int mat;
      const bool medium = MEDIA && type == PRIM_MEDIUM;
      if (medium) {
        // a scatter inside a volume, as shade_core takes a medium hit: p = r.At(t) as it is, the
        // phase material at u = v = 0.  The reference's (1,0,0) normal (medium.go:162-166) is a
        // placeholder: a volume has no shading normal, the guide gets none
        nout = mk3(0, 0, 0);
        mat = sc.media[idx].phase_mat;
        u = v = 0.0f;
      } else if (HAS(FT_SPHERE) && type == PRIM_SPHERE) {
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
        if constexpr (SPEC) eta = 0x1p-22f * (fabsf(p.x * nu.x) + fabsf(p.y * nu.y) + fabsf(p.z * nu.z));
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
      if (medium) n = mk3(0, 0, 0);
      const DevMaterial M = sc.mats[mat];
      kind = M.kind;
      if (M.kind == RT_MAT_METAL) alb = xyz(M.albedo);
      else if (M.kind == RT_MAT_DIELECTRIC) alb = mk3(1, 1, 1);
      else if (M.kind == RT_MAT_DIFFUSE_LIGHT && !ff) alb = mk3(0, 0, 0);  // materials.go:150-155
      else alb = tex_value<FT>(sc, M.tex, u, v, p);
      depth = t * length(d);
      if constexpr (EMIT) lit = M.kind == RT_MAT_DIFFUSE_LIGHT && ff;
      if constexpr (MEDIA) s.nscatter += medium ? 1u : 0u;
      if constexpr (SPEC) {
        const bool metal = kind == RT_MAT_METAL;
        if ((int32_t)k < max_k && (kind == RT_MAT_DIELECTRIC || (metal && M.param <= max_fuzz))) {
          const rt_u32x4 rk = rt_rng_draw(P.seed, id.gpix, j, RT_STREAM(k, 0));
          f3 ndir;
          if (metal) {  // materials.go:70-79
            const f3 refl = unit(reflect(d, n));
            ndir = refl + uniform_sphere(rt_unit_f(rk.v[2]), rt_unit_f(rk.v[3])) * M.param;
          } else {  // materials.go:94-130, Schlick's fifth power as shade_core's three multiplies
            const float ior = M.param;
            const float ri = ff ? rcp(ior) : ior;
            const f3 ud = unit(d);
            const float cs = fminf(dot(-ud, n), 1.0f);
            const float sn = fsqrt(1.0f - cs * cs);
            bool refl = ri * sn > 1.0f;
            if (!refl) {
              float r0 = (1.0f - ior) * rcp(1.0f + ior);
              r0 = r0 * r0;
              const float x = 1.0f - cs, x2 = x * x;
              refl = r0 + (1.0f - r0) * (x2 * x2 * x) > rt_unit_f(rk.v[0]);
            }
            ndir = refl ? reflect(ud, n) : refract(ud, n, ri);
          }
          const float side = dot(ndir, n);
          if (!metal || side > 0.0f) {  // (a metal that scatters into itself absorbs: a terminal)
            T = T * alb;  // the metal's albedo; 1 for glass
            dpre += depth;
            ++k;
            o = p + n * copysignf(eta, side);
            d = ndir;
            continue;  // the next segment
          }
        }
      }
    }
    if constexpr (SPEC) {
      if (k > 0u) {  // (k == 0: the first hit's values as they are)
        alb = T * alb;
        depth = kind < 0 ? 0.0f : dpre + depth;
        s.nspec += k;
      }
    }
    if constexpr (EMIT) {
      if (lit) {
        // what the render adds for this sample: a light does not scatter, so rayColor returns
        // its emission (camera.go:312-314) before the clampContribution of camera.go:330
        s.esum = s.esum + alb;
        ++s.nlight;
      } else {
        s.ssum = s.ssum + alb;
      }
    }
    s.asum = s.asum + alb;
    s.nsum = s.nsum + n;
    s.dsum += depth;
    if (j == 0) s.kind0 = kind;
    break;
  }
}

template <int TREE, bool EMIT, bool MEDIA, bool SPEC>
__global__ __launch_bounds__(256) void k_aov(Params P, AovOut out, AovEmitArg<MEDIA, SPEC> em) {
  constexpr uint32_t FT = TREE == 0 ? (uint32_t)FT_MEDIA : (uint32_t)FT_ALL;
  __shared__ uint32_t lstack[kShortStack * 256];
  if constexpr (HAS(FT_NOISE)) stage_perlin(P.sc);
  __syncthreads();
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const TravStack ts = {&lstack[threadIdx.x], P.ostack + gtid, P.stack_cols, kShortStack};
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t chain_total = 0u;  // SPEC: the chain segments this lane traced
  for (uint32_t lp = gtid; lp < P.npix; lp += stride) {
    const Ids id = aov_ids(P, lp, out.n);
    AovSums s = aov_sums_zero();
    if constexpr (SPEC) {
      for (uint32_t j = 0; j < out.n; ++j) aov_sample<TREE, EMIT, MEDIA, true>(P, id, j, ts, s, em.max_k, em.max_fuzz);
    } else {
      for (uint32_t j = 0; j < out.n; ++j) aov_sample<TREE, EMIT, MEDIA>(P, id, j, ts, s);
    }
    const float inv = 1.0f / (float)out.n;
    if (out.albedo) {
      out.albedo[3 * (size_t)lp + 0] = s.asum.x * inv;
      out.albedo[3 * (size_t)lp + 1] = s.asum.y * inv;
      out.albedo[3 * (size_t)lp + 2] = s.asum.z * inv;
    }
    if (out.normal) {
      out.normal[3 * (size_t)lp + 0] = s.nsum.x * inv;
      out.normal[3 * (size_t)lp + 1] = s.nsum.y * inv;
      out.normal[3 * (size_t)lp + 2] = s.nsum.z * inv;
    }
    if (out.depth) out.depth[lp] = s.dsum * inv;
    if (out.material) out.material[lp] = s.kind0;
    if constexpr (EMIT) {
      if (em.emission) {
        em.emission[3 * (size_t)lp + 0] = s.esum.x * inv;
        em.emission[3 * (size_t)lp + 1] = s.esum.y * inv;
        em.emission[3 * (size_t)lp + 2] = s.esum.z * inv;
      }
      if (em.surface_albedo) {
        em.surface_albedo[3 * (size_t)lp + 0] = s.ssum.x * inv;
        em.surface_albedo[3 * (size_t)lp + 1] = s.ssum.y * inv;
        em.surface_albedo[3 * (size_t)lp + 2] = s.ssum.z * inv;
      }
      // a true division (the build's fp32 divide is not correctly rounded): through fp64, whose
      // 53 bits >= 2 * 24 + 2 make the second rounding innocuous, so nlight == n gives 1.0f
      if (em.coverage) em.coverage[lp] = (float)((double)s.nlight / (double)out.n);
    }
    if constexpr (MEDIA) {  // as coverage: exactly 0 and exactly 1 at the ends
      if (em.scatter) em.scatter[lp] = (float)((double)s.nscatter / (double)out.n);
    }
    if constexpr (SPEC) {  // the same division: exactly 0 where no chain left the first hit
      if (em.bounces) em.bounces[lp] = (float)((double)s.nspec / (double)out.n);
      chain_total += s.nspec;
    }
  }
  if constexpr (SPEC) {  // one atomic per wave that traced any, not one per pixel
    for (int off = 32; off > 0; off >>= 1) chain_total += __shfl_down(chain_total, off);
    if ((threadIdx.x & 63u) == 0u && chain_total) atomicAdd(em.chain_segments, (unsigned long long)chain_total);
  }
  (void)chain_total;
}

// The accumulator's feature fold: k_aov's loop over the P.npix pixels of one
// pass, all P.ss samples of P.seed each, the per-pass fp32 sums added to the fp64 planes F
// instead of being averaged.  PX, as k_accum_fold's: the pass's pixel v is local pixel
// p = map[v] of the share (map null: p = v), and every camera id comes from p, so an active
// pass casts the rays rt_accum_add(seed) casts for that pixel.  One writer per pixel, no
// atomics; count[] is k_accum_fold's.  v < P.npix <= F.npix and map[v] < F.npix (the
// compaction's sorted list of local pixels), so every store is inside its plane.
template <int TREE, bool EMIT, bool PX, bool MEDIA>
__global__ __launch_bounds__(256) void k_aov_fold(Params P, FeatPlanesArg<MEDIA> F, const uint32_t* map) {
  constexpr uint32_t FT = TREE == 0 ? (uint32_t)FT_MEDIA : (uint32_t)FT_ALL;
  __shared__ uint32_t lstack[kShortStack * 256];
  if constexpr (HAS(FT_NOISE)) stage_perlin(P.sc);
  __syncthreads();
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const TravStack ts = {&lstack[threadIdx.x], P.ostack + gtid, P.stack_cols, kShortStack};
  const uint32_t stride = gridDim.x * blockDim.x;
  const size_t n = F.npix;
  for (uint32_t v = gtid; v < P.npix; v += stride) {
    uint32_t p = v;
    if constexpr (PX) p = map ? map[v] : v;
    const Ids id = aov_ids(P, p, P.ss);
    AovSums s = aov_sums_zero();
    for (uint32_t j = 0; j < P.ss; ++j) aov_sample<TREE, EMIT, MEDIA>(P, id, j, ts, s);
    if (F.albedo) {  // the guides group
      F.albedo[p] += (double)s.asum.x;
      F.albedo[n + p] += (double)s.asum.y;
      F.albedo[2 * n + p] += (double)s.asum.z;
      F.normal[p] += (double)s.nsum.x;
      F.normal[n + p] += (double)s.nsum.y;
      F.normal[2 * n + p] += (double)s.nsum.z;
      F.depth[p] += (double)s.dsum;
    }
    if constexpr (EMIT) {
      F.emission[p] += (double)s.esum.x;
      F.emission[n + p] += (double)s.esum.y;
      F.emission[2 * n + p] += (double)s.esum.z;
      F.surface_albedo[p] += (double)s.ssum.x;
      F.surface_albedo[n + p] += (double)s.ssum.y;
      F.surface_albedo[2 * n + p] += (double)s.ssum.z;
      F.nlight[p] += s.nlight;
    }
    if constexpr (MEDIA) F.nscatter[p] += s.nscatter;
  }
}

// The accumulator's chain fold (RT_ACCUM_FEAT_SPEC): k_aov_fold's loop with the
// specular mode's samples (aov_sample<TREE, false, false, true>, rt_render_aov_spec's), the pass's
// fp32 normal and depth sums added to the fp64 planes S and its specular vertices to an exact 64-bit
// count.  No albedo is kept.  A kernel of its own, so that k_aov_fold's instances stay what they
// were (profiles/accum_spec_device_code.txt).  v < P.npix <= S.npix and map[v] < S.npix, as there.
template <int TREE, bool PX>
__global__ __launch_bounds__(256) void k_aov_spec_fold(Params P, SpecPlanes S, const uint32_t* map) {
  constexpr uint32_t FT = TREE == 0 ? (uint32_t)FT_MEDIA : (uint32_t)FT_ALL;
  __shared__ uint32_t lstack[kShortStack * 256];
  if constexpr (HAS(FT_NOISE)) stage_perlin(P.sc);
  __syncthreads();
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const TravStack ts = {&lstack[threadIdx.x], P.ostack + gtid, P.stack_cols, kShortStack};
  const uint32_t stride = gridDim.x * blockDim.x;
  const size_t n = S.npix;
  for (uint32_t v = gtid; v < P.npix; v += stride) {
    uint32_t p = v;
    if constexpr (PX) p = map ? map[v] : v;
    const Ids id = aov_ids(P, p, P.ss);
    AovSums s = aov_sums_zero();
    for (uint32_t j = 0; j < P.ss; ++j) aov_sample<TREE, false, false, true>(P, id, j, ts, s, S.max_k, S.max_fuzz);
    S.normal[p] += (double)s.nsum.x;
    S.normal[n + p] += (double)s.nsum.y;
    S.normal[2 * n + p] += (double)s.nsum.z;
    S.depth[p] += (double)s.dsum;
    S.nspec[p] += (unsigned long long)s.nspec;
  }
}

namespace {

// one feature pass at a time: the scratch buffers (overflow stacks, host staging) and the
// library stream are shared
std::mutex g_mu;
DeviceScratch g_stacks, g_stage, g_count;  // (g_count: the specular mode's chain-segment word)
// the library stream of each device ordinal.  Process lifetime: the list is never destroyed, so
// no stream is released while the runtime unloads.
std::vector<Stream>& g_streams = *new std::vector<Stream>();

// A runtime tree id (0 record loop, 2 BVH2, 5 compressed BVH4, anything else BVH4) as a compile-time
// constant, f(std::integral_constant<..>{}): every kernel choice below goes through this and
// rt_hip_util.h's with_flag
template <class F>
void with_tree(int tree, F&& f) {
  switch (tree) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 5: return f(std::integral_constant<int, 5>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// What a launch of k_aov or k_aov_fold over npix pixels of a view needs beside its planes: the grid,
// the Params with an overflow-stack column per launched thread, and what chooses the kernel instance
struct AovLaunch {
  Params p;
  int blocks, tree;
  bool has_media;
};
// (g_mu held: the stacks are shared; *L is written once nothing can fail any more)
int aov_setup(const AovView& view, const rt_camera_derived& cd, const rt_render_opts& o, uint32_t npix,
              const char* who, AovLaunch* L) {
  const uint32_t blocks = std::min<uint32_t>((npix + 255u) / 256u, view.tree == 0 ? kAovMaxBlocks : kAovMaxTreeBlocks);
  const uint32_t cols = blocks * 256u;
  void* ost = nullptr;
  const size_t depth = view.tree == 0 ? 1 : kStack - kShortStack;
  if (int rc = g_stacks.get(o.device, depth * cols * sizeof(uint32_t), &ost, who)) return rc;
  L->blocks = (int)blocks;
  L->tree = view.tree;
  L->has_media = view.sc.n_media > 0;
  L->p = Params{};
  L->p.sc = view.sc;
  set_camera_params(L->p, cd, o, npix);
  L->p.ostack = (uint32_t*)ost;
  L->p.stack_cols = cols;
  return RT_OK;
}

enum class AovMode { First, Emit, Media, Spec };

// What an entry asks for: the mode, whether its buffers are host memory, its name for the mode's
// own messages, and its arguments as they came in (null: a struct the entry does not take)
struct AovRequest {
  AovMode mode;
  bool host;
  const char* name;
  rt_scene* scene;
  const rt_camera* cam;
  const rt_render_opts* opts;
  int32_t n_samples;
  rt_stats* stats;
  const rt_aov* out;
  const rt_aov_emit* emit;
  const rt_aov_media* media;
  const rt_aov_spec* spec;
  const rt_aov_spec_opts* spec_opts;
};

struct AovPlane {
  void* user;  // the caller's pointer, null: not wanted
  size_t bpp;  // bytes per pixel: 3 or 1 floats or ints
  void* dev;   // where the kernel writes it (aov_bind)
};

struct AovJob {
  rt_render_opts o;  // the defaults resolved
  rt_camera_derived cd;
  rt_aov_spec_opts spec{8, 0.0f};
  uint32_t n;    // samples per pixel
  bool emit;     // the EMIT kernels: the emit entries, and the media entries given an emit struct
  int n_planes;  // the slots the mode stages: 4, 7 or 8
  AovPlane planes[8];  // in staging order: AovOut's pointers, AovEmit's, the mode's own plane
  std::chrono::steady_clock::time_point t_start;  // the checks done
  uint32_t rows, npix;                            // this rank's share
  hipStream_t stream;
  AovLaunch l;
  unsigned long long chain_segments;  // the specular mode: those behind the camera rays'
};

// Every argument test, in the entries' fixed order; no device is touched
int aov_check(const AovRequest& rq, AovJob* j) {
  if (!rq.scene || !rq.cam) return set_error(RT_ERR_INVALID, "rt_render_aov: null scene/camera");
  // per mode: the slots it stages and the struct that selects it (required; `out` may be null beside it)
  const char* missing = nullptr;
  switch (rq.mode) {
    case AovMode::First: j->n_planes = 4, missing = rq.out ? nullptr : "output"; break;
    case AovMode::Emit: j->n_planes = 7, missing = rq.emit ? nullptr : "emit"; break;
    case AovMode::Media: j->n_planes = 8, missing = rq.media ? nullptr : "media"; break;
    case AovMode::Spec: j->n_planes = 8, missing = rq.spec ? nullptr : "spec"; break;
  }
  if (missing) return set_error(RT_ERR_INVALID, "%s: null %s", rq.name, missing);
  void* own = nullptr;  // the mode's own plane, in the last slot
  if (rq.mode == AovMode::Media) own = rq.media->scatter;
  if (rq.mode == AovMode::Spec) own = rq.spec->bounces;
  j->emit = rq.mode == AovMode::Emit || (rq.mode == AovMode::Media && rq.emit);
  const rt_aov out = rq.out ? *rq.out : rt_aov{};
  const rt_aov_emit em = j->emit ? *rq.emit : rt_aov_emit{};
  const AovPlane planes[8] = {{out.albedo, 12},  {out.normal, 12},        {out.depth, 4},   {out.material, 4},
                              {em.emission, 12}, {em.surface_albedo, 12}, {em.coverage, 4}, {own, 4}};
  std::copy(planes, planes + 8, j->planes);
  // (rt_render_aov itself has always taken an `out` without a buffer)
  if (rq.mode != AovMode::First && std::none_of(planes, planes + 8, [](const AovPlane& p) { return p.user; }))
    return set_error(RT_ERR_INVALID, "%s: no buffer wanted", rq.name);
  if (const rt_aov_spec_opts* so = rq.mode == AovMode::Spec ? rq.spec_opts : nullptr) {
    if (so->max_bounces < 0 || so->max_bounces > 64)
      return set_error(RT_ERR_INVALID, "%s: max_bounces %d not in 0 .. 64", rq.name, so->max_bounces);
    if (!(so->max_fuzz >= 0.0f) || !std::isfinite(so->max_fuzz))
      return set_error(RT_ERR_INVALID, "%s: max_fuzz must be finite and >= 0", rq.name);
    if (so->max_bounces > 0) j->spec.max_bounces = so->max_bounces;
    j->spec.max_fuzz = so->max_fuzz;
  }
  j->o = rq.opts ? *rq.opts : rt_render_opts{};
  if (j->o.nranks <= 0) j->o.nranks = 1;
  if (j->o.rank < 0 || j->o.rank >= j->o.nranks) return set_error(RT_ERR_INVALID, "rt_render_aov: bad rank");
  if (int rc = rt_camera_derive(rq.cam, &j->cd)) return rc;
  const uint32_t ss = (uint32_t)j->cd.spp_sqrt * (uint32_t)j->cd.spp_sqrt;
  if (rq.n_samples < 0 || (uint32_t)rq.n_samples > ss)
    return set_error(RT_ERR_INVALID, "rt_render_aov: %d samples of %u", rq.n_samples, ss);
  j->n = rq.n_samples == 0 ? 1u : (uint32_t)rq.n_samples;
  j->t_start = std::chrono::steady_clock::now();
  return RT_OK;
}

int aov_plan(const AovView& view, AovJob* j) {
  j->rows = rank_rows((uint32_t)j->cd.height, j->o.rank, j->o.nranks);
  const uint64_t npix64 = (uint64_t)j->rows * (uint32_t)j->cd.width;
  if (npix64 >= 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_render_aov: image too large");
  j->npix = (uint32_t)npix64;
  if ((int)g_streams.size() <= j->o.device) g_streams.resize(j->o.device + 1);
  if (int rc = g_streams[j->o.device].pick(j->o.stream, &j->stream)) return rc;
  return aov_setup(view, j->cd, j->o, j->npix, "rt_render_aov", &j->l);  // (no pixels: no blocks, nothing allocated)
}

// A device entry's planes are written in place, a host entry's in their slots of one staging buffer
// (an absent plane keeps its slot)
int aov_bind(bool host, AovJob* j) {
  for (AovPlane& p : j->planes) p.dev = host ? nullptr : p.user;
  if (!host) return RT_OK;
  size_t total = 0;
  for (int i = 0; i < j->n_planes; ++i) total += j->planes[i].bpp * j->npix;
  void* stg = nullptr;
  if (int rc = g_stage.get(j->o.device, total, &stg, "rt_render_aov")) return rc;
  size_t off = 0;
  for (int i = 0; i < j->n_planes; off += j->planes[i++].bpp * j->npix)
    if (j->planes[i].user) j->planes[i].dev = (char*)stg + off;
  return RT_OK;
}

// The mode's kernel on the job's stream: k_aov of (emit x media | spec) x tree, its 20 instances
int aov_launch(AovMode mode, AovJob* j) {
  const AovPlane* pl = j->planes;
  const AovOut ao{(float*)pl[0].dev, (float*)pl[1].dev, (float*)pl[2].dev, (int32_t*)pl[3].dev, j->n};
  const AovEmitMedia md{{(float*)pl[4].dev, (float*)pl[5].dev, (float*)pl[6].dev}, (float*)pl[7].dev};
  const dim3 g((unsigned)j->l.blocks), b(256);
  if (mode == AovMode::Spec) {  // (with neither flag)
    // the chain segments are counted on the device; max_k: the last vertex a chain may reach
    void* cnt = nullptr;
    if (int rc = g_count.get(j->o.device, sizeof j->chain_segments, &cnt, "rt_render_aov_spec")) return rc;
    HIP_OK(hipMemsetAsync(cnt, 0, sizeof j->chain_segments, j->stream));
    const int32_t max_k = std::max(0, std::min(j->spec.max_bounces, j->cd.max_depth - 1));
    const AovEmitSpec sp{md, md.scatter, (unsigned long long*)cnt, max_k, j->spec.max_fuzz};
    with_tree(j->l.tree, [&](auto t) {
      hipLaunchKernelGGL((k_aov<decltype(t)::value, false, false, true>), g, b, 0, j->stream, j->l.p, ao, sp);
    });
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&j->chain_segments, cnt, sizeof j->chain_segments, hipMemcpyDeviceToHost, j->stream));
    return RT_OK;
  }
  // a scene without media: the kernels without the mode (rt_render_aov_emit's bits), scatter = 0
  const bool media = mode == AovMode::Media && j->l.has_media;
  if (mode == AovMode::Media && !media && md.scatter)
    HIP_OK(hipMemsetAsync(md.scatter, 0, pl[7].bpp * j->npix, j->stream));
  with_tree(j->l.tree, [&](auto t) {
    constexpr int T = decltype(t)::value;
    with_flag(j->emit, [&](auto e) {
      with_flag(media, [&](auto m) {
        constexpr bool E = decltype(e)::value, M = decltype(m)::value;
        hipLaunchKernelGGL((k_aov<T, E, M, false>), g, b, 0, j->stream, j->l.p, ao, (const AovEmitArg<M>&)md);
      });
    });
  });
  HIP_OK(hipGetLastError());
  return RT_OK;
}

int aov_collect(const AovRequest& rq, const AovJob& j) {
  for (int i = 0; rq.host && j.npix > 0 && i < j.n_planes; ++i)
    if (const AovPlane& p = j.planes[i]; p.user)
      HIP_OK(hipMemcpyAsync(p.user, p.dev, p.bpp * j.npix, hipMemcpyDeviceToHost, j.stream));
  if (j.npix > 0) HIP_OK(hipStreamSynchronize(j.stream));
  if (rt_stats* stats = rq.stats) {
    memset(stats, 0, sizeof *stats);
    stats->samples = (uint64_t)j.npix * j.n;
    // one closest-hit query per feature ray, and per specular vertex passed in the specular mode
    stats->segments = (uint64_t)j.npix * j.n + j.chain_segments;
    stats->rows = (int32_t)j.rows;
    stats->tree_width = j.l.tree;
    stats->scene_features = (int32_t)rq.scene->s.h.features;
    stats->kernel_features = j.l.tree == 0 ? (int32_t)FT_MEDIA : (int32_t)FT_ALL;
    stats->path_slots = j.l.blocks * 256;
    stats->tuned = tune_count();
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j.t_start).count();
  }
  return RT_OK;
}

int aov_impl(const AovRequest& rq) {
  AovJob j{};
  int rc;
  if ((rc = aov_check(rq, &j)) || (rc = device_ok("rt_render_aov", j.o.device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(j.o.device));
  AovView view;
  if ((rc = aov_view(&rq.scene->s, j.o.device, &view))) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = aov_plan(view, &j))) return rc;
  if (j.npix > 0 && ((rc = aov_bind(rq.host, &j)) || (rc = aov_launch(rq.mode, &j)))) return rc;
  return aov_collect(rq, j);
}

// the pass aov_fold_begin prepared, valid while it holds g_mu
AovLaunch g_fold;

}  // namespace

int aov_fold_begin(rt_scene* scene, const rt_camera_derived& cd, const rt_render_opts& o, uint32_t n_pass) {
  if (int rc = device_ok("rt_accum_add", o.device)) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(o.device));
  AovView view;
  if (int rc = aov_view(&scene->s, o.device, &view)) return rc;
  std::unique_lock<std::mutex> lk(g_mu);
  if (int rc = aov_setup(view, cd, o, n_pass, "rt_accum_add", &g_fold)) return rc;
  lk.release();  // held until aov_fold_end
  return RT_OK;
}

// k_aov_fold of emit x px x media x tree, its 32 instances
int aov_fold_enqueue(const FeatPlanes& F, uint32_t* nscatter, bool px, const uint32_t* map, hipStream_t stream) {
  // a scene without media: the kernels without the mode, the counts stay 0
  const FeatPlanesMedia fm{F, g_fold.has_media ? nscatter : nullptr};
  const dim3 g((unsigned)g_fold.blocks), b(256);
  with_tree(g_fold.tree, [&](auto t) {
    with_flag(F.emission != nullptr, [&](auto e) {
      with_flag(px, [&](auto x) {
        with_flag(fm.nscatter != nullptr, [&](auto m) {
          constexpr bool M = decltype(m)::value;
          hipLaunchKernelGGL((k_aov_fold<decltype(t)::value, decltype(e)::value, decltype(x)::value, M>), g, b, 0,
                             stream, g_fold.p, (const FeatPlanesArg<M>&)fm, map);
        });
      });
    });
  });
  HIP_OK(hipGetLastError());
  return RT_OK;
}

// k_aov_spec_fold of px x tree, its 8 instances
int aov_spec_fold_enqueue(const SpecPlanes& S, bool px, const uint32_t* map, hipStream_t stream) {
  const dim3 g((unsigned)g_fold.blocks), b(256);
  with_tree(g_fold.tree, [&](auto t) {
    with_flag(px, [&](auto x) {
      hipLaunchKernelGGL((k_aov_spec_fold<decltype(t)::value, decltype(x)::value>), g, b, 0, stream, g_fold.p, S, map);
    });
  });
  HIP_OK(hipGetLastError());
  return RT_OK;
}

void aov_fold_end() { g_mu.unlock(); }

}  // namespace rt

extern "C" {

int rt_render_aov(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
                  const rt_aov* out_host, rt_stats* stats) {
  return rt::aov_impl({rt::AovMode::First, /*host=*/true, "rt_render_aov", s, cam, opts, n_samples, stats, out_host});
}

int rt_render_aov_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                         int32_t n_samples, const rt_aov* out_device, rt_stats* stats) {
  return rt::aov_impl(
      {rt::AovMode::First, /*host=*/false, "rt_render_aov", s, cam, opts, n_samples, stats, out_device});
}

int rt_render_aov_emit(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
                       const rt_aov* out_host, const rt_aov_emit* emit_host, rt_stats* stats) {
  return rt::aov_impl({rt::AovMode::Emit, /*host=*/true, "rt_render_aov_emit", s, cam, opts, n_samples, stats,
                       out_host, emit_host});
}

int rt_render_aov_emit_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                              int32_t n_samples, const rt_aov* out_device,
                              const rt_aov_emit* emit_device, rt_stats* stats) {
  return rt::aov_impl({rt::AovMode::Emit, /*host=*/false, "rt_render_aov_emit", s, cam, opts, n_samples, stats,
                       out_device, emit_device});
}

int rt_render_aov_media(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
                        const rt_aov* out_host, const rt_aov_emit* emit_host, const rt_aov_media* media_host,
                        rt_stats* stats) {
  return rt::aov_impl({rt::AovMode::Media, /*host=*/true, "rt_render_aov_media", s, cam, opts, n_samples, stats,
                       out_host, emit_host, media_host});
}

int rt_render_aov_media_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                               int32_t n_samples, const rt_aov* out_device, const rt_aov_emit* emit_device,
                               const rt_aov_media* media_device, rt_stats* stats) {
  return rt::aov_impl({rt::AovMode::Media, /*host=*/false, "rt_render_aov_media", s, cam, opts, n_samples, stats,
                       out_device, emit_device, media_device});
}

int rt_render_aov_spec(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
                       const rt_aov_spec_opts* spec_opts, const rt_aov* out_host, const rt_aov_spec* spec_host,
                       rt_stats* stats) {
  return rt::aov_impl({rt::AovMode::Spec, /*host=*/true, "rt_render_aov_spec", s, cam, opts, n_samples, stats,
                       out_host, nullptr, nullptr, spec_host, spec_opts});
}

int rt_render_aov_spec_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
                              const rt_aov_spec_opts* spec_opts, const rt_aov* out_device,
                              const rt_aov_spec* spec_device, rt_stats* stats) {
  return rt::aov_impl({rt::AovMode::Spec, /*host=*/false, "rt_render_aov_spec", s, cam, opts, n_samples, stats,
                       out_device, nullptr, nullptr, spec_device, spec_opts});
}

}  // extern "C"
