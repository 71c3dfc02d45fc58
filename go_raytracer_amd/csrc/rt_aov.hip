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
//
// k_aov_emit (rt_render_aov_emit): the same kernel text (rt_aov_kernel.inc) with the emission
// split of DESIGN.md §15: per pixel also the mean emission of the samples that see a light's
// front face, the mean albedo of the others and the fraction of the former.
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

// the emission split's buffers (rt_abi.h rt_aov_emit), device pointers
struct AovEmit {
  float* emission;
  float* surface_albedo;
  float* coverage;
};

#define RT_AOV_EMIT 0
#include "rt_aov_kernel.inc"  // k_aov
#undef RT_AOV_EMIT
#define RT_AOV_EMIT 1
#include "rt_aov_kernel.inc"  // k_aov_emit
#undef RT_AOV_EMIT

namespace {

// one feature pass at a time: the scratch buffers (overflow stacks, host staging) and the
// library stream are shared
std::mutex g_mu;
DeviceScratch g_stacks, g_stage;
std::vector<hipStream_t> g_streams;

// split: the rt_render_aov_emit entries (outp may be null, emitp is required); else emitp is null
int aov_impl(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
             const rt_aov* outp, const rt_aov_emit* emitp, bool split, bool host, rt_stats* stats) {
  if (!scene || !cam) return set_error(RT_ERR_INVALID, "rt_render_aov: null scene/camera");
  const rt_aov no_out{nullptr, nullptr, nullptr, nullptr};
  if (split) {
    if (!emitp) return set_error(RT_ERR_INVALID, "rt_render_aov_emit: null emit");
    if (!outp) outp = &no_out;
    if (!outp->albedo && !outp->normal && !outp->depth && !outp->material && !emitp->emission &&
        !emitp->surface_albedo && !emitp->coverage)
      return set_error(RT_ERR_INVALID, "rt_render_aov_emit: no buffer wanted");
  }
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
    AovEmit ae{nullptr, nullptr, nullptr};
    if (split) ae = AovEmit{emitp->emission, emitp->surface_albedo, emitp->coverage};
    size_t off_n = 0, off_d = 0, off_m = 0, total = 0;
    if (host) {  // stage: albedo | normal | depth | material in one scratch buffer
      off_n = 3 * (size_t)npix * 4;
      off_d = off_n + 3 * (size_t)npix * 4;
      off_m = off_d + (size_t)npix * 4;
      total = off_m + (size_t)npix * 4;
      const size_t off_e = total;  // split: | emission | surface_albedo | coverage
      if (split) total += 7 * (size_t)npix * 4;
      void* stg = nullptr;
      if ((rc = g_stage.get(o.device, total, &stg, "rt_render_aov"))) return rc;
      char* b = (char*)stg;
      ao.albedo = outp->albedo ? (float*)b : nullptr;
      ao.normal = outp->normal ? (float*)(b + off_n) : nullptr;
      ao.depth = outp->depth ? (float*)(b + off_d) : nullptr;
      ao.material = outp->material ? (int32_t*)(b + off_m) : nullptr;
      if (split) {
        ae.emission = emitp->emission ? (float*)(b + off_e) : nullptr;
        ae.surface_albedo = emitp->surface_albedo ? (float*)(b + off_e + 3 * (size_t)npix * 4) : nullptr;
        ae.coverage = emitp->coverage ? (float*)(b + off_e + 6 * (size_t)npix * 4) : nullptr;
      }
    }
    const dim3 g((unsigned)blocks), b(256);
    if (split) {
      switch (view.tree) {
        case 0: hipLaunchKernelGGL(k_aov_emit<0>, g, b, 0, stream, p, ao, ae); break;
        case 2: hipLaunchKernelGGL(k_aov_emit<2>, g, b, 0, stream, p, ao, ae); break;
        case 5: hipLaunchKernelGGL(k_aov_emit<5>, g, b, 0, stream, p, ao, ae); break;
        default: hipLaunchKernelGGL(k_aov_emit<4>, g, b, 0, stream, p, ao, ae); break;
      }
    } else {
      switch (view.tree) {
        case 0: hipLaunchKernelGGL(k_aov<0>, g, b, 0, stream, p, ao); break;
        case 2: hipLaunchKernelGGL(k_aov<2>, g, b, 0, stream, p, ao); break;
        case 5: hipLaunchKernelGGL(k_aov<5>, g, b, 0, stream, p, ao); break;
        default: hipLaunchKernelGGL(k_aov<4>, g, b, 0, stream, p, ao); break;
      }
    }
    HIP_OK(hipGetLastError());
    if (host && split) {
      if (emitp->emission)
        HIP_OK(hipMemcpyAsync(emitp->emission, ae.emission, 3 * (size_t)npix * 4, hipMemcpyDeviceToHost, stream));
      if (emitp->surface_albedo)
        HIP_OK(hipMemcpyAsync(emitp->surface_albedo, ae.surface_albedo, 3 * (size_t)npix * 4,
                              hipMemcpyDeviceToHost, stream));
      if (emitp->coverage)
        HIP_OK(hipMemcpyAsync(emitp->coverage, ae.coverage, (size_t)npix * 4, hipMemcpyDeviceToHost, stream));
    }
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
  return rt::aov_impl(s, cam, opts, n_samples, out_host, nullptr, false, true, stats);
}

int rt_render_aov_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                         int32_t n_samples, const rt_aov* out_device, rt_stats* stats) {
  return rt::aov_impl(s, cam, opts, n_samples, out_device, nullptr, false, false, stats);
}

int rt_render_aov_emit(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t n_samples,
                       const rt_aov* out_host, const rt_aov_emit* emit_host, rt_stats* stats) {
  return rt::aov_impl(s, cam, opts, n_samples, out_host, emit_host, true, true, stats);
}

int rt_render_aov_emit_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                              int32_t n_samples, const rt_aov* out_device,
                              const rt_aov_emit* emit_device, rt_stats* stats) {
  return rt::aov_impl(s, cam, opts, n_samples, out_device, emit_device, true, false, stats);
}

}  // extern "C"
