// rt_accum.hip — the progressive pass accumulator (rt_abi.h rt_accum_*).
//
// An accumulator keeps, for one (scene, camera, row share) on one device, the exact sum of
// every render pass added to it, and a Welford pair of the passes' luminance per pixel.  A
// pass is an ordinary render (rt_render.hip render_impl: the same plans, launches and buffers,
// under the same per-(device, slot) mutex) that ends in k_accum_fold instead of k_resolve.
//
// State, structure of planes, one entry per pixel of the share (68 B per pixel):
//   sum[3]   u64  the passes' 2^-32 fixed-point pixel sums, added with plain 64-bit adds
//                 (a pass's samples are limited to 2^31 / (spp * max_passes), so the total
//                 stays inside int64; read back as int64)
//   side[3]  f64  the passes' fp64 side sums (samples above that limit)
//   mean, m2 f64  Welford's running mean and sum of squared deviations of the pass luminance
//   flags    u32  the passes' NaN / +Inf / -Inf flag words, OR-ed
// k_accum_fold     one pass -> state          (one pixel per lane, 256-thread blocks)
// k_accum_resolve  state -> mean RGB and the variance of the mean luminance
// k_accum_info1/2  state -> {sum of variances, sum of means, finite pixels, other pixels}:
//                  a two-stage block reduction in fp64, fixed tree order, no atomics
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "rt_hip_util.h"
#include "rt_resolve.h"

namespace rt {

struct AccumPlanes {
  unsigned long long* sum;  // [3][npix]
  double* side;             // [3][npix]
  double* mean;             // [npix]
  double* m2;               // [npix]
  uint32_t* flags;          // [npix]
};

// Rec. 709 luminance of linear RGB
RT_D double luminance(double r, double g, double b) { return 0.2126 * r + 0.7152 * g + 0.0722 * b; }

// variance of the mean of n passes from Welford's M2 (0 while there is no second pass)
RT_D double var_of_mean(double m2, uint32_t n) {
  return n >= 2u ? m2 / ((double)(n - 1u) * (double)n) : 0.0;
}

// One finished pass (P's accum / csum records / side / pflags, as k_resolve reads them)
// into the accumulator; n = passes including this one, scale = pixel_samples_scale.
__global__ __launch_bounds__(256) void k_accum_fold(Params P, AccumPlanes A, double scale, uint32_t n) {
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= P.npix) return;
  const uint32_t f = P.pflags[lp];
  unsigned long long cs[3] = {0ull, 0ull, 0ull};
  chunk_record_sums(P, lp, cs);
  double c[3];
  for (int ch = 0; ch < 3; ++ch) {
    const size_t i = (size_t)ch * P.npix + lp;
    const unsigned long long sum = P.accum[i] + cs[ch];
    const double side = P.side[i];
    A.sum[i] += sum;
    A.side[i] += side;
    c[ch] = flagged_channel(f, ch, (long long)sum, side, scale);
  }
  A.flags[lp] |= f;
  const double y = luminance(c[0], c[1], c[2]);
  double mean = A.mean[lp];
  const double d = y - mean;
  mean += d / (double)n;
  A.m2[lp] += d * (y - mean);
  A.mean[lp] = mean;
}

// scale_n = pixel_samples_scale / passes (0 with no pass: the image is zeros)
__global__ __launch_bounds__(256) void k_accum_resolve(AccumPlanes A, uint32_t npix, double scale_n,
                                                       uint32_t n, float* rgb, float* var) {
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= npix) return;
  if (rgb) {
    const uint32_t f = A.flags[lp];
    for (int ch = 0; ch < 3; ++ch) {
      const size_t i = (size_t)ch * npix + lp;
      rgb[3 * (size_t)lp + ch] = (float)flagged_channel(f, ch, (long long)A.sum[i], A.side[i], scale_n);
    }
  }
  if (var) var[lp] = (float)var_of_mean(A.m2[lp], n);
}

constexpr int kInfoBlocks = 256;  // at most: stage 2 is one block over the partials

// the block's four sums by a fixed tree over its 256 threads -> lane 0's v
RT_D void block_sum4(double v[4], double (*red)[256]) {
  const uint32_t t = threadIdx.x;
  for (int k = 0; k < 4; ++k) red[k][t] = v[k];
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + s];
    __syncthreads();
  }
  for (int k = 0; k < 4; ++k) v[k] = red[k][0];
}

// stage 1: thread t of block b sums pixels b * 256 + t, + gridDim.x * 256, ... in order
__global__ __launch_bounds__(256) void k_accum_info1(AccumPlanes A, uint32_t npix, uint32_t n, double* part) {
  __shared__ double red[4][256];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x; lp < npix; lp += stride) {
    const double var = var_of_mean(A.m2[lp], n), mean = A.mean[lp];
    if (isfinite(var) && isfinite(mean)) {
      v[0] += var;
      v[1] += mean;
      v[2] += 1.0;
    } else {
      v[3] += 1.0;
    }
  }
  block_sum4(v, red);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) part[4 * blockIdx.x + k] = v[k];
}

// stage 2: one block over stage 1's nb <= 256 partials -> out[4]
__global__ __launch_bounds__(256) void k_accum_info2(const double* part, uint32_t nb, double* out) {
  __shared__ double red[4][256];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (threadIdx.x < nb)
    for (int k = 0; k < 4; ++k) v[k] = part[4 * threadIdx.x + k];
  block_sum4(v, red);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) out[k] = v[k];
}

}  // namespace rt

// ==================================================================== host ==
struct rt_accum {
  rt_scene* scene = nullptr;
  rt_camera cam{};
  rt_render_opts opts{};  // the fields rt_accum_create keeps; seed set per pass
  rt_camera_derived cd{};
  int32_t max_passes = 0, passes = 0;
  uint32_t npix = 0, ss = 0;
  std::mutex mu;  // one call per accumulator at a time
  void* buf = nullptr;  // planes | info partials and result | resolve staging
  size_t state_bytes = 0;
  rt::AccumPlanes A{};
  double* part = nullptr;  // [kInfoBlocks][4], then the result [4]
  float *stage_rgb = nullptr, *stage_var = nullptr;
  hipStream_t own_stream = nullptr;
};

namespace rt {
namespace {

int accum_stream(rt_accum* a, hipStream_t* out) {
  *out = (hipStream_t)a->opts.stream;
  if (*out) return RT_OK;
  if (!a->own_stream) HIP_OK(hipStreamCreateWithFlags(&a->own_stream, hipStreamNonBlocking));
  *out = a->own_stream;
  return RT_OK;
}

// render_impl's sink: the pass is complete on `stream` up to the resolve
int fold_pass(void* ctx, const Params& p, double scale, hipStream_t stream) {
  rt_accum* a = (rt_accum*)ctx;
  if (p.npix != a->npix) return set_error(RT_ERR_INVALID, "rt_accum_add: the pass has %u pixels, the accumulator %u", p.npix, a->npix);
  hipLaunchKernelGGL(k_accum_fold, dim3((a->npix + 255) / 256), dim3(256), 0, stream, p, a->A, scale,
                     (uint32_t)a->passes + 1u);
  HIP_OK(hipGetLastError());
  return RT_OK;
}

void free_accum(rt_accum* a) {
  DeviceGuard dg;
  if (a->buf || a->own_stream) (void)hipSetDevice(a->opts.device);
  if (a->buf) (void)hipFree(a->buf);
  if (a->own_stream) (void)hipStreamDestroy(a->own_stream);
  delete a;
}

int accum_resolve(rt_accum* a, float* rgb, float* var, bool host) {
  if (!a) return set_error(RT_ERR_INVALID, "rt_accum_resolve: null accumulator");
  std::lock_guard<std::mutex> lk(a->mu);
  if (a->npix == 0 || (!rgb && !var)) return RT_OK;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(a->opts.device));
  hipStream_t stream;
  int rc;
  if ((rc = accum_stream(a, &stream))) return rc;
  float* drgb = !rgb ? nullptr : host ? a->stage_rgb : rgb;
  float* dvar = !var ? nullptr : host ? a->stage_var : var;
  const double scale_n = a->passes > 0 ? a->cd.pixel_samples_scale / (double)a->passes : 0.0;
  hipLaunchKernelGGL(k_accum_resolve, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->A, a->npix,
                     scale_n, (uint32_t)a->passes, drgb, dvar);
  HIP_OK(hipGetLastError());
  if (host && rgb)
    HIP_OK(hipMemcpyAsync(rgb, drgb, 3 * (size_t)a->npix * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (host && var)
    HIP_OK(hipMemcpyAsync(var, dvar, (size_t)a->npix * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}

}  // namespace

// rt_scene_destroy: the accumulators the scene still owns
void release_accums(Scene* s) {
  std::vector<rt_accum*> own;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    own.swap(s->accums);
  }
  for (rt_accum* a : own) free_accum(a);
}

}  // namespace rt

extern "C" {

int rt_accum_create(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, int32_t max_passes,
                    rt_accum** out) {
  using namespace rt;
  if (!s || !cam || !out) return set_error(RT_ERR_INVALID, "rt_accum_create: null scene/camera/out");
  *out = nullptr;
  rt_render_opts o{};
  if (opts) {  // the fields a pass keeps; the seed comes with each pass
    o.device = opts->device;
    o.rank = opts->rank;
    o.nranks = opts->nranks;
    o.mode = opts->mode;
    o.chunk = opts->chunk;
    o.path_slots = opts->path_slots;
    o.flags = opts->flags & RT_FLAG_PROFILE;
    o.stream = opts->stream;
    o.progress_slices = opts->progress_slices;
    if (opts->trace_out) return set_error(RT_ERR_INVALID, "rt_accum_create: a pass records no path trace (trace_out)");
  }
  o.trace_pixel = -1;
  if (o.nranks <= 0) o.nranks = 1;
  if (o.rank < 0 || o.rank >= o.nranks) return set_error(RT_ERR_INVALID, "rt_accum_create: bad rank");
  if (max_passes < 0) return set_error(RT_ERR_INVALID, "rt_accum_create: max_passes %d", max_passes);
  if (max_passes == 0) max_passes = 1024;
  rt_camera_derived cd;
  int rc = rt_camera_derive(cam, &cd);
  if (rc) return rc;
  const uint64_t ss = (uint64_t)cd.spp_sqrt * (uint64_t)cd.spp_sqrt;
  if (ss * (uint64_t)max_passes >= ((uint64_t)1 << 31))
    return set_error(RT_ERR_INVALID, "rt_accum_create: %llu samples x %d passes: the exact sum holds fewer than 2^31 samples per pixel",
                     (unsigned long long)ss, max_passes);
  const uint64_t npix64 = (uint64_t)rank_rows((uint32_t)cd.height, o.rank, o.nranks) * (uint32_t)cd.width;
  if (npix64 >= 0x7FFFFFFFull) return set_error(RT_ERR_UNSUPPORTED, "rt_accum_create: image too large");
  if ((rc = device_ok("rt_accum_create", o.device))) return rc;

  rt_accum* a = new rt_accum();
  a->scene = s;
  a->cam = *cam;
  a->opts = o;
  a->cd = cd;
  a->max_passes = max_passes;
  a->npix = (uint32_t)npix64;
  a->ss = (uint32_t)ss;
  const size_t n = std::max<size_t>(a->npix, 1);
  // sum | side | mean | m2 (f64 / u64), the info partials, then flags and the staging (4 B)
  a->state_bytes = n * (3 * 8 + 3 * 8 + 8 + 8);
  const size_t part_bytes = (size_t)(kInfoBlocks + 1) * 4 * sizeof(double);
  const size_t total = a->state_bytes + part_bytes + n * 4 + n * 16;
  DeviceGuard dg;
  hipError_t e = hipSetDevice(o.device);
  if (e == hipSuccess) e = hipMalloc(&a->buf, total);
  if (e == hipSuccess) e = hipMemset(a->buf, 0, total);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    free_accum(a);
    return set_error(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_DEVICE, "rt_accum_create: %zu bytes: %s", total,
                     hipGetErrorString(e));
  }
  char* b = (char*)a->buf;
  a->A.sum = (unsigned long long*)b;
  a->A.side = (double*)(b + n * 24);
  a->A.mean = (double*)(b + n * 48);
  a->A.m2 = (double*)(b + n * 56);
  a->part = (double*)(b + a->state_bytes);
  a->A.flags = (uint32_t*)(b + a->state_bytes + part_bytes);
  a->stage_rgb = (float*)(b + a->state_bytes + part_bytes + n * 4);
  a->stage_var = a->stage_rgb + 3 * n;
  {
    std::lock_guard<std::mutex> lk(s->s.mu);
    s->s.accums.push_back(a);
  }
  *out = a;
  return RT_OK;
}

int rt_accum_destroy(rt_accum* a) {
  if (!a) return RT_OK;
  {
    rt::Scene& s = a->scene->s;
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = std::find(s.accums.begin(), s.accums.end(), a);
    if (it != s.accums.end()) s.accums.erase(it);
  }
  {
    std::lock_guard<std::mutex> lk(a->mu);  // a call in flight on another thread ends first
  }
  rt::free_accum(a);
  return RT_OK;
}

int rt_accum_reset(rt_accum* a) {
  using namespace rt;
  if (!a) return set_error(RT_ERR_INVALID, "rt_accum_reset: null accumulator");
  std::lock_guard<std::mutex> lk(a->mu);
  DeviceGuard dg;
  HIP_OK(hipSetDevice(a->opts.device));
  hipStream_t stream;
  int rc;
  if ((rc = accum_stream(a, &stream))) return rc;
  HIP_OK(hipMemsetAsync(a->buf, 0, a->state_bytes, stream));
  HIP_OK(hipMemsetAsync(a->A.flags, 0, std::max<size_t>(a->npix, 1) * sizeof(uint32_t), stream));
  HIP_OK(hipStreamSynchronize(stream));
  a->passes = 0;
  return RT_OK;
}

int rt_accum_add(rt_accum* a, uint64_t seed, rt_stats* stats) {
  using namespace rt;
  if (!a) return set_error(RT_ERR_INVALID, "rt_accum_add: null accumulator");
  std::lock_guard<std::mutex> lk(a->mu);
  if (a->passes >= a->max_passes)
    return set_error(RT_ERR_INVALID, "rt_accum_add: the accumulator holds its %d passes", a->max_passes);
  rt_render_opts o = a->opts;
  o.seed = seed;
  const PassSink sink = {(uint32_t)a->max_passes, fold_pass, a};
  const int rc = render_pass(a->scene, &a->cam, &o, stats, &sink);
  if (rc == RT_OK) ++a->passes;
  return rc;
}

int rt_accum_resolve(rt_accum* a, float* rgb_host, float* var_host) {
  return rt::accum_resolve(a, rgb_host, var_host, true);
}

int rt_accum_resolve_device(rt_accum* a, float* rgb_dev, float* var_dev) {
  return rt::accum_resolve(a, rgb_dev, var_dev, false);
}

int rt_accum_info_get(rt_accum* a, rt_accum_info* out) {
  using namespace rt;
  if (!a || !out) return set_error(RT_ERR_INVALID, "rt_accum_info_get: null");
  std::lock_guard<std::mutex> lk(a->mu);
  memset(out, 0, sizeof *out);
  out->passes = a->passes;
  out->max_passes = a->max_passes;
  out->samples_per_pixel = (uint64_t)a->ss * (uint64_t)a->passes;
  if (a->npix == 0) return RT_OK;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(a->opts.device));
  hipStream_t stream;
  int rc;
  if ((rc = accum_stream(a, &stream))) return rc;
  const uint32_t nb = std::min<uint32_t>((a->npix + 255u) / 256u, (uint32_t)kInfoBlocks);
  double* res = a->part + 4 * (size_t)kInfoBlocks;
  hipLaunchKernelGGL(k_accum_info1, dim3(nb), dim3(256), 0, stream, a->A, a->npix, (uint32_t)a->passes, a->part);
  hipLaunchKernelGGL(k_accum_info2, dim3(1), dim3(256), 0, stream, a->part, nb, res);
  HIP_OK(hipGetLastError());
  double h[4];
  HIP_OK(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  out->nonfinite_pixels = (uint64_t)h[3];
  if (h[2] > 0.0) {
    out->rms_std_error = sqrt(h[0] / h[2]);
    out->mean_luminance = h[1] / h[2];
  }
  out->rel_error = out->rms_std_error / (out->mean_luminance + 1e-6);
  return RT_OK;
}

}  // extern "C"
