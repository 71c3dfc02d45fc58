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
// (DESIGN.md §9).  Constant media are not traced: they are transparent to this pass.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <vector>

#include "rt_hip_util.h"
#include "rt_path.h"

namespace rt {

#ifdef RT_QTOP
#error "rt_aov.hip: k_aov<5> stages no top items in LDS; the RT_QTOP experiment build does not cover the feature pass"
#endif

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

// TREE: 0 record loop (quad-only scenes: the media set's code, which covers the lean one),
// 2 BVH2, 4 BVH4, 5 compressed BVH4 (any feature)
template <int TREE>
__global__ __launch_bounds__(256) void k_aov(Params P, AovOut out) {
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
      }
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
  }
}

namespace {

// one feature pass at a time: the scratch buffers (overflow stacks, host staging) and the
// library stream are shared
std::mutex g_mu;
DeviceScratch g_stacks, g_stage;
std::vector<hipStream_t> g_streams;

int aov_impl(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
             const rt_aov* outp, bool host, rt_stats* stats) {
  if (!scene || !cam) return set_error(RT_ERR_INVALID, "rt_render_aov: null scene/camera");
  if (!outp) return set_error(RT_ERR_INVALID, "rt_render_aov: null output");
  rt_render_opts o{};
  if (opts) o = *opts;
  if (o.nranks <= 0) o.nranks = 1;
  if (o.rank < 0 || o.rank >= o.nranks) return set_error(RT_ERR_INVALID, "rt_render_aov: bad rank");
  rt_camera_derived cd;
  int rc = rt_camera_derive(cam, &cd);
  if (rc) return rc;
  const uint32_t ss = (uint32_t)cd.spp_sqrt * (uint32_t)cd.spp_sqrt;
  if (n_samples < 0 || (uint32_t)n_samples > ss)
    return set_error(RT_ERR_INVALID, "rt_render_aov: %d samples of %u", n_samples, ss);
  const uint32_t n = n_samples == 0 ? 1u : (uint32_t)n_samples;
  const auto t_start = std::chrono::steady_clock::now();
  if ((rc = device_ok("rt_render_aov", o.device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(o.device));
  AovView view;
  if ((rc = aov_view(&scene->s, o.device, &view))) return rc;
  std::lock_guard<std::mutex> lk(g_mu);

  const uint32_t W = (uint32_t)cd.width, H = (uint32_t)cd.height;
  const uint32_t rows = rank_rows(H, o.rank, o.nranks);
  const uint64_t npix64 = (uint64_t)rows * W;
  if (npix64 >= 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_render_aov: image too large");
  const uint32_t npix = (uint32_t)npix64;

  hipStream_t stream = (hipStream_t)o.stream;
  if (!stream) {
    if ((int)g_streams.size() <= o.device) g_streams.resize(o.device + 1, nullptr);
    if (!g_streams[o.device])
      HIP_OK(hipStreamCreateWithFlags(&g_streams[o.device], hipStreamNonBlocking));
    stream = g_streams[o.device];
  }

  const int blocks = (int)std::min<uint32_t>((npix + 255u) / 256u,
                                             (uint32_t)(view.tree == 0 ? kAovMaxBlocks : kAovMaxTreeBlocks));
  if (npix > 0) {
    Params p{};
    p.sc = view.sc;
    set_camera_params(p, cd, o, npix);
    // traversal-stack overflow columns, one per launched thread
    const uint32_t cols = (uint32_t)blocks * 256u;
    void* ost = nullptr;
    if ((rc = g_stacks.get(o.device, (size_t)(view.tree == 0 ? 1 : kStack - kShortStack) * cols * sizeof(uint32_t), &ost,
                           "rt_render_aov")))
      return rc;
    p.ostack = (uint32_t*)ost;
    p.stack_cols = cols;

    AovOut ao{outp->albedo, outp->normal, outp->depth, outp->material, n};
    size_t off_n = 0, off_d = 0, off_m = 0, total = 0;
    if (host) {  // stage: albedo | normal | depth | material in one scratch buffer
      off_n = 3 * (size_t)npix * 4;
      off_d = off_n + 3 * (size_t)npix * 4;
      off_m = off_d + (size_t)npix * 4;
      total = off_m + (size_t)npix * 4;
      void* stg = nullptr;
      if ((rc = g_stage.get(o.device, total, &stg, "rt_render_aov"))) return rc;
      char* b = (char*)stg;
      ao.albedo = outp->albedo ? (float*)b : nullptr;
      ao.normal = outp->normal ? (float*)(b + off_n) : nullptr;
      ao.depth = outp->depth ? (float*)(b + off_d) : nullptr;
      ao.material = outp->material ? (int32_t*)(b + off_m) : nullptr;
    }
    const dim3 g((unsigned)blocks), b(256);
    switch (view.tree) {
      case 0: hipLaunchKernelGGL(k_aov<0>, g, b, 0, stream, p, ao); break;
      case 2: hipLaunchKernelGGL(k_aov<2>, g, b, 0, stream, p, ao); break;
      case 5: hipLaunchKernelGGL(k_aov<5>, g, b, 0, stream, p, ao); break;
      default: hipLaunchKernelGGL(k_aov<4>, g, b, 0, stream, p, ao); break;
    }
    HIP_OK(hipGetLastError());
    if (host) {
      if (outp->albedo)
        HIP_OK(hipMemcpyAsync(outp->albedo, ao.albedo, 3 * (size_t)npix * 4, hipMemcpyDeviceToHost, stream));
      if (outp->normal)
        HIP_OK(hipMemcpyAsync(outp->normal, ao.normal, 3 * (size_t)npix * 4, hipMemcpyDeviceToHost, stream));
      if (outp->depth)
        HIP_OK(hipMemcpyAsync(outp->depth, ao.depth, (size_t)npix * 4, hipMemcpyDeviceToHost, stream));
      if (outp->material)
        HIP_OK(hipMemcpyAsync(outp->material, ao.material, (size_t)npix * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP_OK(hipStreamSynchronize(stream));
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->samples = (uint64_t)npix * n;
    stats->segments = (uint64_t)npix * n;  // one closest-hit query per feature ray
    stats->rows = (int32_t)rows;
    stats->tree_width = view.tree;
    stats->scene_features = (int32_t)scene->s.h.features;
    stats->kernel_features = view.tree == 0 ? (int32_t)FT_MEDIA : (int32_t)FT_ALL;
    stats->path_slots = blocks * 256;
    stats->tuned = tune_count();
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  }
  return RT_OK;
}

}  // namespace
}  // namespace rt

extern "C" {

int rt_render_aov(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
                  const rt_aov* out_host, rt_stats* stats) {
  return rt::aov_impl(s, cam, opts, n_samples, out_host, true, stats);
}

int rt_render_aov_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                         int32_t n_samples, const rt_aov* out_device, rt_stats* stats) {
  return rt::aov_impl(s, cam, opts, n_samples, out_device, false, stats);
}

}  // extern "C"
