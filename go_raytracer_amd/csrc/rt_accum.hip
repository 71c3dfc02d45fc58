// rt_accum.hip — the progressive pass accumulator (rt_abi.h rt_accum_*).
//
// An accumulator keeps, for one (scene, camera, row share) on one device, the exact sum of
// every render pass added to it, and a Welford pair of the passes' luminance per pixel.  A
// pass is an ordinary render (rt_render.hip render_impl: the same plans, launches and buffers,
// under the same per-(device, slot) mutex) that ends in k_accum_fold instead of k_resolve.
//
// State, structure of planes, one entry per pixel of the share (76 B per pixel):
//   sum[3]   u64  the passes' 2^-32 fixed-point pixel sums, added with plain 64-bit adds
//                 (a pass's samples are limited to 2^31 / (spp * max_passes), so the total
//                 stays inside int64; read back as int64)
//   side[3]  f64  the passes' fp64 side sums (samples above that limit)
//   mean, m2 f64  Welford's running mean and sum of squared deviations of the pass luminance
//   flags    u32  the passes' NaN / +Inf / -Inf flag words, OR-ed
//   count    u32  passes the pixel took; written from the first active-pixel pass on (§14): an
//                 accumulator that took whole passes only is *uniform* and never touches it
//   map      u32  the current selection: the active local pixels, ascending
// Each of the next three is one text in two instances.  PX = false, the uniform accumulator:
// every pixel has the pass count the launch carries, and count and map are not even arguments.
// PX = true, once a pass covered a part of the pixels: count[p] passes.
// k_accum_fold<PX>     one pass -> state (one pixel per lane, 256-thread blocks); PX: the
//                      pass's pixel v updates pixel map[v] of the share
// k_accum_resolve<PX>  state -> mean RGB and the variance of the mean luminance
// k_accum_info1<PX>/2  state -> {sum of variances, sum of means, finite pixels, other pixels}:
//                      a two-stage block reduction in fp64, fixed tree order, no atomics
// k_accum_tiles    state -> per tile: the error figure e_T and the active flag (one tile per lane)
// k_active_count / k_active_scan / k_active_scatter  active pixels -> the sorted map: ballot
//                  counts per block, an exclusive scan by one block, a scatter; no atomics
// k_count_stats    min, max and sum of a u32 array by one block (counts, tile flags)
//
// Feature buffers (rt_accum_set_features): a second allocation, alive only while
// features are on, of the FeatPlanes sums (rt_host_units.h; 56 B per pixel for the guides group,
// 52 B for the emit group, 4 B of scatter counts for RT_ACCUM_FEAT_MEDIA) and 56 B per pixel (60 B
// with the scatter plane) of staging for rt_accum_resolve_aov.  A pass then
// also runs rt_aov.hip's k_aov_fold for the same seed and pixels on the same stream;
// k_feat_resolve<PX> maps the sums to the rt_aov / rt_aov_emit planes.
// RT_ACCUM_FEAT_SPEC adds the chain sums (SpecPlanes: 40 B per pixel, fp64 normal and
// depth and a 64-bit count of specular vertices) and 20 B of staging; a pass then also runs
// k_aov_spec_fold, and k_spec_resolve<PX> maps the sums to rt_accum_resolve_aov_spec's planes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <type_traits>

#include "rt_hip_util.h"
#include "rt_host_units.h"
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

// Where a kernel's pass counts come from: the launch's n for every pixel, or per pixel
template <bool PX>
struct Passes {
  uint32_t n;  // k_accum_fold: including the pass being folded
};
template <>
struct Passes<true> {
  uint32_t npix;        // pixels of the share
  uint32_t* count;      // [npix]
  const uint32_t* map;  // k_accum_fold: the pass's pixels (null: a whole pass, the identity)
};
template <bool PX>
RT_D uint32_t passes_of(const Passes<PX>& c, uint32_t p) {
  if constexpr (PX) return c.count[p];
  else return c.n;
}

// Welford's update of pixel p with the luminance y of its n-th pass
RT_D void welford_add(const AccumPlanes& A, uint32_t p, double y, uint32_t n) {
  double mean = A.mean[p];
  const double d = y - mean;
  mean += d / (double)n;
  A.m2[p] += d * (y - mean);
  A.mean[p] = mean;
}

// Pixel p of n passes into {sum of variances, sum of means, pixels} if its variance of the mean
// and its Welford mean are finite; else false, and nothing is added
RT_D bool add_finite(const AccumPlanes& A, uint32_t p, uint32_t n, double& sv, double& sm, double& k) {
  const double var = var_of_mean(A.m2[p], n), mean = A.mean[p];
  if (!(isfinite(var) && isfinite(mean))) return false;
  sv += var;
  sm += mean;
  k += 1.0;
  return true;
}

// One finished pass (P's accum / csum records / side / pflags, as k_resolve reads them) into the
// accumulator; scale = pixel_samples_scale.  The pass's sums are read at the pass's own pixel v;
// PX: the state is updated at p = map[v] with the pixel's own pass count
template <bool PX>
__global__ __launch_bounds__(256) void k_accum_fold(Params P, AccumPlanes A, double scale, Passes<PX> c) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= P.npix) return;
  uint32_t p = v, npix = P.npix;
  if constexpr (PX) {
    p = c.map ? c.map[v] : v;
    npix = c.npix;
  }
  const uint32_t f = P.pflags[v];
  unsigned long long cs[3] = {0ull, 0ull, 0ull};
  chunk_record_sums(P, v, cs);
  double y[3];
  for (int ch = 0; ch < 3; ++ch) {
    const size_t i = (size_t)ch * P.npix + v, k = (size_t)ch * npix + p;
    const unsigned long long sum = P.accum[i] + cs[ch];
    const double side = P.side[i];
    A.sum[k] += sum;
    A.side[k] += side;
    y[ch] = flagged_channel(f, ch, (long long)sum, side, scale);
  }
  A.flags[p] |= f;
  uint32_t n;
  if constexpr (PX) c.count[p] = n = c.count[p] + 1u;
  else n = c.n;
  welford_add(A, p, luminance(y[0], y[1], y[2]), n);
}

// PX: scale = pixel_samples_scale, and a pixel without a pass resolves to zeros; else scale is
// that over the passes, divided on the host (0 with no pass: the image is zeros)
template <bool PX>
__global__ __launch_bounds__(256) void k_accum_resolve(AccumPlanes A, uint32_t npix, double scale, Passes<PX> c,
                                                       float* rgb, float* var) {
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= npix) return;
  const uint32_t n = passes_of(c, lp);
  if (rgb) {
    const uint32_t f = A.flags[lp];
    double scale_n = scale;
    if constexpr (PX) scale_n = n ? scale / (double)n : 0.0;
    for (int ch = 0; ch < 3; ++ch) {
      const size_t i = (size_t)ch * npix + lp;
      rgb[3 * (size_t)lp + ch] = (float)flagged_channel(f, ch, (long long)A.sum[i], A.side[i], scale_n);
    }
  }
  if (var) var[lp] = (float)var_of_mean(A.m2[lp], n);
}

// The float planes of rt_accum_resolve_aov (rt_aov's without the material, rt_aov_emit's), any null
struct FeatOut {
  float *albedo, *normal, *depth, *emission, *surface_albedo, *coverage;
};

// Feature sums -> their means over the n_p * ss camera samples of pixel lp: each fp64 sum
// divided in fp64 and rounded once to fp32; a pixel without a pass resolves to zeros.  An
// output whose group is not enabled is null (checked on the host).
template <bool PX>
__global__ __launch_bounds__(256) void k_feat_resolve(FeatPlanes F, uint32_t ss, Passes<PX> c, FeatOut out) {
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= F.npix) return;
  const double den = (double)passes_of(c, lp) * (double)ss;
  const size_t n = F.npix;
  auto mean3 = [&](const double* sum, float* o) {
    for (int ch = 0; ch < 3; ++ch) o[3 * (size_t)lp + ch] = den > 0.0 ? (float)(sum[ch * n + lp] / den) : 0.0f;
  };
  if (out.albedo) mean3(F.albedo, out.albedo);
  if (out.normal) mean3(F.normal, out.normal);
  if (out.depth) out.depth[lp] = den > 0.0 ? (float)(F.depth[lp] / den) : 0.0f;
  if (out.emission) mean3(F.emission, out.emission);
  if (out.surface_albedo) mean3(F.surface_albedo, out.surface_albedo);
  if (out.coverage) out.coverage[lp] = den > 0.0 ? (float)((double)F.nlight[lp] / den) : 0.0f;
}

// The media mode's plane (RT_ACCUM_FEAT_MEDIA), a kernel of its own so that k_feat_resolve stays
// the code it was: scatter = the pixel's scatter samples over its n_p * ss camera samples, as
// coverage above; 0 without a pass.
template <bool PX>
__global__ __launch_bounds__(256) void k_scatter_resolve(const uint32_t* nscatter, uint32_t npix, uint32_t ss,
                                                         Passes<PX> c, float* scatter) {
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= npix) return;
  const double den = (double)passes_of(c, lp) * (double)ss;
  scatter[lp] = den > 0.0 ? (float)((double)nscatter[lp] / den) : 0.0f;
}

// The chain planes (RT_ACCUM_FEAT_SPEC), a kernel of its own as k_scatter_resolve: the normal and
// depth sums over the pixel's n_p * ss samples, divided in fp64 and rounded once, and bounces = the
// specular vertices passed over the same number (a pixel whose samples all passed k: exactly k).
template <bool PX>
__global__ __launch_bounds__(256) void k_spec_resolve(SpecPlanes S, uint32_t ss, Passes<PX> c, float* normal,
                                                      float* depth, float* bounces) {
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= S.npix) return;
  const double den = (double)passes_of(c, lp) * (double)ss;
  const size_t n = S.npix;
  if (normal)
    for (int ch = 0; ch < 3; ++ch) normal[3 * (size_t)lp + ch] = den > 0.0 ? (float)(S.normal[ch * n + lp] / den) : 0.0f;
  if (depth) depth[lp] = den > 0.0 ? (float)(S.depth[lp] / den) : 0.0f;
  if (bounces) bounces[lp] = den > 0.0 ? (float)((double)S.nspec[lp] / den) : 0.0f;
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
template <bool PX>
__global__ __launch_bounds__(256) void k_accum_info1(AccumPlanes A, uint32_t npix, Passes<PX> c, double* part) {
  __shared__ double red[4][256];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x; lp < npix; lp += stride)
    if (!add_finite(A, lp, passes_of(c, lp), v[0], v[1], v[2])) v[3] += 1.0;
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

// ------------------------------------------- per-pixel pass counts --
__global__ __launch_bounds__(256) void k_accum_fill(uint32_t* v, uint32_t n, uint32_t x) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = x;
}

// {min, max, sum} of v[0 .. n) by one block: thread t takes t, t + 256, ..., then a fixed tree
// (block_sum4's tree with one operator per row: a shared form would be longer than the two)
__global__ __launch_bounds__(256) void k_count_stats(const uint32_t* v, uint32_t n, unsigned long long* out) {
  __shared__ unsigned long long red[3][256];
  unsigned long long lo = ~0ull, hi = 0ull, sum = 0ull;
  for (uint32_t i = threadIdx.x; i < n; i += 256u) {
    const unsigned long long x = v[i];
    lo = x < lo ? x : lo;
    hi = x > hi ? x : hi;
    sum += x;
  }
  const uint32_t t = threadIdx.x;
  red[0][t] = lo;
  red[1][t] = hi;
  red[2][t] = sum;
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] = red[0][t + s] < red[0][t] ? red[0][t + s] : red[0][t];
      red[1][t] = red[1][t + s] > red[1][t] ? red[1][t + s] : red[1][t];
      red[2][t] += red[2][t + s];
    }
    __syncthreads();
  }
  if (t == 0)
    for (int k = 0; k < 3; ++k) out[k] = red[k][0];
}

// ----------------------------------------------------- selection --
// The share's local image in tiles of tile x tile pixels (edge tiles smaller), tx x ty of them
struct TileGrid {
  uint32_t W, rows, tile, tx, ty;
};

// e_T = sqrt(mean var_p) / (max(mean mean_p, 0) + lum_floor) over the tile's pixels whose
// variance and Welford mean are finite, summed row by row in fp64 (0 without such a pixel),
// rounded to fp32: the figure rt_accum_tile_error reports is the one rt_accum_select compares.
// *young: some pixel of the tile has fewer than min_passes passes.  count null: every pixel
// has `passes` (a uniform accumulator).
RT_D float tile_error(const AccumPlanes& A, const uint32_t* count, uint32_t passes, const TileGrid& g,
                      uint32_t T, double lum_floor, uint32_t min_passes, bool* young) {
  const uint32_t tr = T / g.tx, tc = T - tr * g.tx;
  const uint32_t r1 = min((tr + 1u) * g.tile, g.rows), c1 = min((tc + 1u) * g.tile, g.W);
  double sv = 0.0, sm = 0.0, k = 0.0;
  bool yg = false;
  for (uint32_t r = tr * g.tile; r < r1; ++r)
    for (uint32_t c = tc * g.tile; c < c1; ++c) {
      const uint32_t lp = r * g.W + c;
      const uint32_t n = count ? count[lp] : passes;
      yg |= n < min_passes;
      add_finite(A, lp, n, sv, sm, k);
    }
  *young = yg;
  return k > 0.0 ? (float)(sqrt(sv / k) / (fmax(sm / k, 0.0) + lum_floor)) : 0.0f;
}

// one tile per lane -> err[T] (if asked) and flag[T] = young or e_T > rel_error (if asked)
__global__ __launch_bounds__(256) void k_accum_tiles(AccumPlanes A, const uint32_t* count, uint32_t passes,
                                                     TileGrid g, double lum_floor, uint32_t min_passes,
                                                     double rel_error, float* err, uint32_t* flag) {
  const uint32_t T = blockIdx.x * blockDim.x + threadIdx.x;
  if (T >= g.tx * g.ty) return;
  bool young;
  const float e = tile_error(A, count, passes, g, T, lum_floor, min_passes, &young);
  if (err) err[T] = e;
  if (flag) flag[T] = (young || (double)e > rel_error) ? 1u : 0u;
}

// A pixel is active when its tile is (flag, by rt_accum_select) or its mask byte is set (mask,
// by rt_accum_set_active)
struct ActiveSrc {
  const uint32_t* flag;
  const uint8_t* mask;
  TileGrid g;
};
RT_D bool pixel_active(const ActiveSrc& a, uint32_t lp) {
  if (a.mask) return a.mask[lp] != 0;
  const uint32_t r = lp / a.g.W, c = lp - r * a.g.W;
  return a.flag[(r / a.g.tile) * a.g.tx + c / a.g.tile] != 0u;
}
// The compaction: cnt[b] = active pixels of block b's 256 pixels (four ballots) ...
__global__ __launch_bounds__(256) void k_active_count(ActiveSrc a, uint32_t npix, uint32_t* cnt) {
  __shared__ uint32_t wsum[4];
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = lp < npix && pixel_active(a, lp);
  const unsigned long long m = __ballot(act);
  if (lane_id() == 0u) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// ... cnt[0 .. nb) -> its exclusive prefix sums in place, cnt[nb] = the total: one block, 256
// entries per step, a carry between the steps ...
__global__ __launch_bounds__(256) void k_active_scan(uint32_t* cnt, uint32_t nb) {
  __shared__ uint32_t buf[256];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = 0u;
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += 256u) {
    const uint32_t i = base + t;
    const uint32_t x = i < nb ? cnt[i] : 0u;
    buf[t] = x;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {  // inclusive (Hillis-Steele)
      const uint32_t y = t >= off ? buf[t - off] : 0u;
      __syncthreads();
      buf[t] += y;
      __syncthreads();
    }
    const uint32_t c0 = carry;
    if (i < nb) cnt[i] = c0 + buf[t] - x;
    __syncthreads();
    if (t == 255u) carry = c0 + buf[255];
    __syncthreads();
  }
  if (t == 0) cnt[nb] = carry;
}
// ... and block b's active pixels to map[off[b] ..), in ascending order: a lane's place is
// the active lanes below it in its wave plus the waves below its wave
__global__ __launch_bounds__(256) void k_active_scatter(ActiveSrc a, uint32_t npix, const uint32_t* off,
                                                        uint32_t* map) {
  __shared__ uint32_t wsum[4];
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = lp < npix && pixel_active(a, lp);
  const unsigned long long m = __ballot(act);
  const uint32_t w = threadIdx.x >> 6;
  if (lane_id() == 0u) wsum[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = off[blockIdx.x];
  for (uint32_t i = 0; i < w; ++i) base += wsum[i];
  if (act) map[base + prefix_count(m)] = lp;  // base + place < the total <= npix
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
  rt::DeviceBuffer buf;  // planes | info partials and result | resolve staging
  size_t state_bytes = 0;
  rt::AccumPlanes A{};
  double* part = nullptr;  // [kInfoBlocks][4], then the result [4]
  float *stage_rgb = nullptr, *stage_var = nullptr;
  rt::Stream own_stream;  // for an accumulator without opts.stream
  // per-pixel pass counts and the selection
  uint32_t W = 0, rows = 0;
  uint32_t* count = nullptr;  // [npix], valid while per_pixel
  uint32_t* map = nullptr;    // [npix], the selection's sel_n active pixels
  uint32_t* scan = nullptr;   // [ceil(npix / 256) + 1] block counts, then their prefix sums and the total
  unsigned long long* red = nullptr;  // k_count_stats' results: [0..3) of count, [4..7) of the tile flags
  bool per_pixel = false;     // a pass covered a part of the pixels: count holds, the PX instances run
  bool sel_valid = false;     // a selection was made since the last pass or reset
  bool sel_tiles = false;     // ... by rt_accum_select (red[4..7) describes its tiles)
  uint32_t sel_n = 0;         // active pixels of the last selection
  int32_t n_tiles = 0;
  const uint32_t* pass_map = nullptr;  // the map of the pass being folded (null: a whole pass)
  // feature buffers: off until rt_accum_set_features
  uint32_t features = 0;     // RT_ACCUM_FEAT_* enabled
  rt::DeviceBuffer feat_buf;  // the enabled groups' planes | resolve staging
  size_t feat_state_bytes = 0;
  rt::FeatPlanes F{};
  uint32_t* nscatter = nullptr;  // [npix] RT_ACCUM_FEAT_MEDIA: samples whose first event is a scatter (exact)
  float* feat_stage = nullptr;  // [14][npix] floats: rt_accum_resolve_aov's planes in FeatOut's order, then scatter's
  rt::SpecPlanes S{};           // RT_ACCUM_FEAT_SPEC: the chain sums and the chain limits
  float* spec_stage = nullptr;  // [5][npix] floats: rt_accum_resolve_aov_spec's normal, depth, bounces
};

namespace rt {
namespace {

// Every entry's prologue once a->mu is held (DeviceGuard in the caller's scope): makes the
// accumulator's device current, -> the caller's stream or the accumulator's own
int accum_device(rt_accum* a, hipStream_t* out) {
  HIP_OK(hipSetDevice(a->opts.device));
  return a->own_stream.pick(a->opts.stream, out);
}

// the PX instances' counts (a->per_pixel); uniform launches carry Passes<false>{passes}
Passes<true> px_counts(const rt_accum* a, const uint32_t* map = nullptr) { return {a->npix, a->count, map}; }

// render_impl's sink: the pass is complete on `stream` up to the resolve
int fold_pass(void* ctx, const Params& p, double scale, hipStream_t stream) {
  rt_accum* a = (rt_accum*)ctx;
  const uint32_t want = a->pass_map ? a->sel_n : a->npix;
  if (p.npix != want) return set_error(RT_ERR_INVALID, "rt_accum_add: the pass has %u pixels, the accumulator expects %u", p.npix, want);
  if (!a->per_pixel && !a->pass_map) {  // uniform: every pixel has taken every pass
    hipLaunchKernelGGL(k_accum_fold<false>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, p, a->A, scale,
                       Passes<false>{(uint32_t)a->passes + 1u});
  } else {
    if (!a->per_pixel)  // the first active pass: every pixel has `passes` so far
      hipLaunchKernelGGL(k_accum_fill, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->count, a->npix,
                         (uint32_t)a->passes);
    hipLaunchKernelGGL(k_accum_fold<true>, dim3((p.npix + 255) / 256), dim3(256), 0, stream, p, a->A, scale,
                       px_counts(a, a->pass_map));
  }
  HIP_OK(hipGetLastError());
  if (a->features) {
    if (int rc = aov_fold_enqueue(a->F, a->nscatter, a->per_pixel || a->pass_map, a->pass_map, stream)) return rc;
    if (a->features & RT_ACCUM_FEAT_SPEC)  // the chain fold: the same seed and pixels, after the first-hit fold
      return aov_spec_fold_enqueue(a->S, a->per_pixel || a->pass_map, a->pass_map, stream);
  }
  return RT_OK;
}

// rt_adapt_opts with its defaults filled in, or RT_ERR_INVALID: needs no accumulator
int adapt_opts_ok(const char* who, const rt_adapt_opts* in, rt_adapt_opts* o) {
  if (!in) return set_error(RT_ERR_INVALID, "%s: null options", who);
  *o = *in;
  if (!(o->rel_error > 0.0)) return set_error(RT_ERR_INVALID, "%s: rel_error %g must be > 0", who, o->rel_error);
  if (!(o->lum_floor >= 0.0) || !std::isfinite(o->lum_floor))
    return set_error(RT_ERR_INVALID, "%s: lum_floor %g", who, o->lum_floor);
  if (o->lum_floor == 0.0) o->lum_floor = 1e-2;
  if (o->tile == 0) o->tile = 8;
  if (o->tile < 1 || o->tile > 64) return set_error(RT_ERR_INVALID, "%s: tile %d is not in 1..64", who, o->tile);
  if (o->min_passes == 0) o->min_passes = 4;
  if (o->min_passes < 2) return set_error(RT_ERR_INVALID, "%s: min_passes %d must be >= 2", who, o->min_passes);
  return RT_OK;
}

TileGrid tile_grid(const rt_accum* a, int32_t tile) {
  TileGrid g;
  g.W = a->W;
  g.rows = a->rows;
  g.tile = (uint32_t)tile;
  g.tx = (a->W + g.tile - 1u) / g.tile;
  g.ty = (a->rows + g.tile - 1u) / g.tile;
  return g;
}

// a selection of n pixels stands
int selected(rt_accum* a, uint32_t n, uint64_t* n_active_pixels) {
  a->sel_n = n;
  a->sel_valid = true;
  if (n_active_pixels) *n_active_pixels = n;
  return RT_OK;
}

// the active pixels of `src` -> a->map, ascending; their number -> a->sel_n (one 4-byte read-back)
int compact_active(rt_accum* a, const ActiveSrc& src, hipStream_t stream, uint64_t* n_active_pixels) {
  const uint32_t nb = (a->npix + 255u) / 256u;
  hipLaunchKernelGGL(k_active_count, dim3(nb), dim3(256), 0, stream, src, a->npix, a->scan);
  hipLaunchKernelGGL(k_active_scan, dim3(1), dim3(256), 0, stream, a->scan, nb);
  hipLaunchKernelGGL(k_active_scatter, dim3(nb), dim3(256), 0, stream, src, a->npix, a->scan, a->map);
  HIP_OK(hipGetLastError());
  uint32_t n = 0;
  HIP_OK(hipMemcpyAsync(&n, a->scan + nb, sizeof n, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  if (n > a->npix) return set_error(RT_ERR_DEVICE, "internal: %u active pixels of %u", n, a->npix);
  return selected(a, n, n_active_pixels);
}

// {min, max, sum} of the per-pixel counts -> h (a->per_pixel)
int count_stats(rt_accum* a, hipStream_t stream, unsigned long long h[3]) {
  hipLaunchKernelGGL(k_count_stats, dim3(1), dim3(256), 0, stream, a->count, a->npix, a->red);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(h, a->red, 3 * sizeof h[0], hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}

int accum_counts(rt_accum* a, int32_t* out, bool host) {
  if (!a || !out) return set_error(RT_ERR_INVALID, "rt_accum_counts: null");
  std::lock_guard<std::mutex> lk(a->mu);
  if (a->npix == 0) return RT_OK;
  if (host && !a->per_pixel) {
    std::fill(out, out + a->npix, a->passes);
    return RT_OK;
  }
  DeviceGuard dg;
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  if (!a->per_pixel) {
    hipLaunchKernelGGL(k_accum_fill, dim3((a->npix + 255) / 256), dim3(256), 0, stream, (uint32_t*)out, a->npix,
                       (uint32_t)a->passes);
    HIP_OK(hipGetLastError());
  } else {
    HIP_OK(hipMemcpyAsync(out, a->count, (size_t)a->npix * sizeof(uint32_t),
                          host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
  }
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}

// The accumulator's one allocation, in order: a's pointers into the buffer at `base` and
// state_bytes -> the buffer's size (base null: only the size is meant)
size_t carve(rt_accum* a, void* base) {
  const size_t n = std::max<size_t>(a->npix, 1);
  size_t off = 0;
  auto take = [&](auto*& p, size_t count) {  // the next `count` elements of p's type
    p = (std::remove_reference_t<decltype(p)>)((uintptr_t)base + off);
    off += count * sizeof *p;
  };
  take(a->A.sum, 3 * n);
  take(a->A.side, 3 * n);
  take(a->A.mean, n);
  take(a->A.m2, n);
  a->state_bytes = off;  // what rt_accum_reset clears, with the flags
  take(a->part, (size_t)(kInfoBlocks + 1) * 4);
  take(a->red, 8);
  take(a->A.flags, n);
  take(a->stage_rgb, 3 * n);  // the selection's tile flags or mask bytes pass through it too
  take(a->stage_var, n);      // ... and the tile errors
  take(a->count, n);
  take(a->map, n);
  take(a->scan, (n + 255) / 256 + 1);
  return off;
}

// The feature allocation, in order: the enabled groups of a->F and the staging at `base`
// (null: only the size is meant), feat_state_bytes -> what rt_accum_reset clears
size_t carve_features(rt_accum* a, uint32_t planes, void* base) {
  const size_t n = std::max<size_t>(a->npix, 1);
  size_t off = 0;
  auto take = [&](auto*& p, size_t count) {
    p = (std::remove_reference_t<decltype(p)>)((uintptr_t)base + off);
    off += count * sizeof *p;
  };
  a->F = FeatPlanes{};
  a->F.npix = a->npix;
  const SpecPlanes lim = a->S;  // (the chain limits are accum_set_features', not this function's)
  a->S = SpecPlanes{};
  a->S.npix = a->npix, a->S.max_k = lim.max_k, a->S.max_fuzz = lim.max_fuzz;
  if (planes & RT_ACCUM_FEAT_SPEC) {  // first: 8-byte elements, before the groups' 4-byte counts
    take(a->S.normal, 3 * n);
    take(a->S.depth, n);
    take(a->S.nspec, n);
  }
  if (planes & RT_ACCUM_FEAT_GUIDES) {
    take(a->F.albedo, 3 * n);
    take(a->F.normal, 3 * n);
    take(a->F.depth, n);
  }
  if (planes & RT_ACCUM_FEAT_EMIT) {
    take(a->F.emission, 3 * n);
    take(a->F.surface_albedo, 3 * n);
    take(a->F.nlight, n);
  }
  a->nscatter = nullptr;
  if (planes & RT_ACCUM_FEAT_MEDIA) take(a->nscatter, n);
  a->feat_state_bytes = off;
  take(a->feat_stage, (planes & RT_ACCUM_FEAT_MEDIA ? 15 : 14) * n);
  a->spec_stage = nullptr;
  if (planes & RT_ACCUM_FEAT_SPEC) take(a->spec_stage, 5 * n);
  return off;
}

// features off: the feature allocation freed (the accumulator's device is current)
void drop_features(rt_accum* a) {
  a->feat_buf.reset();
  a->features = 0;
  a->F = FeatPlanes{};
  a->nscatter = nullptr;
  a->feat_stage = nullptr;
  a->S = SpecPlanes{};
  a->spec_stage = nullptr;
}

void free_accum(rt_accum* a) {
  DeviceGuard dg;
  if (a->buf.p || a->feat_buf.p || a->own_stream.s) (void)hipSetDevice(a->opts.device);
  delete a;
}

int accum_resolve(rt_accum* a, float* rgb, float* var, bool host) {
  if (!a) return set_error(RT_ERR_INVALID, "rt_accum_resolve: null accumulator");
  std::lock_guard<std::mutex> lk(a->mu);
  if (a->npix == 0 || (!rgb && !var)) return RT_OK;
  DeviceGuard dg;
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  float* drgb = !rgb ? nullptr : host ? a->stage_rgb : rgb;
  float* dvar = !var ? nullptr : host ? a->stage_var : var;
  const double scale_n = a->passes > 0 ? a->cd.pixel_samples_scale / (double)a->passes : 0.0;
  if (a->per_pixel)
    hipLaunchKernelGGL(k_accum_resolve<true>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->A, a->npix,
                       a->cd.pixel_samples_scale, px_counts(a), drgb, dvar);
  else
    hipLaunchKernelGGL(k_accum_resolve<false>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->A, a->npix,
                       scale_n, Passes<false>{(uint32_t)a->passes}, drgb, dvar);
  HIP_OK(hipGetLastError());
  if (host && rgb)
    HIP_OK(hipMemcpyAsync(rgb, drgb, 3 * (size_t)a->npix * sizeof(float), hipMemcpyDeviceToHost, stream));
  if (host && var)
    HIP_OK(hipMemcpyAsync(var, dvar, (size_t)a->npix * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}

// media: the rt_accum_resolve_aov_media entries (mediap is required there)
int accum_resolve_aov(rt_accum* a, const rt_aov* outp, const rt_aov_emit* emitp, const rt_aov_media* mediap,
                      bool media, bool host) {
  const char* who = media ? (host ? "rt_accum_resolve_aov_media" : "rt_accum_resolve_aov_media_device")
                          : (host ? "rt_accum_resolve_aov" : "rt_accum_resolve_aov_device");
  if (!a) return set_error(RT_ERR_INVALID, "%s: null accumulator", who);
  if (media && !mediap) return set_error(RT_ERR_INVALID, "%s: null media", who);
  float* const uscat = media ? mediap->scatter : nullptr;
  const rt_aov no_out{nullptr, nullptr, nullptr, nullptr};
  const rt_aov_emit no_emit{nullptr, nullptr, nullptr};
  const rt_aov& o = outp ? *outp : no_out;
  const rt_aov_emit& e = emitp ? *emitp : no_emit;
  if (o.material) return set_error(RT_ERR_INVALID, "%s: the accumulator keeps no material plane", who);
  void* const user[6] = {o.albedo, o.normal, o.depth, e.emission, e.surface_albedo, e.coverage};
  const bool guides = user[0] || user[1] || user[2], emit = user[3] || user[4] || user[5];
  if (!guides && !emit && !uscat) return set_error(RT_ERR_INVALID, "%s: no buffer wanted", who);
  std::lock_guard<std::mutex> lk(a->mu);
  if (uscat && !(a->features & RT_ACCUM_FEAT_MEDIA))
    return set_error(RT_ERR_INVALID, "%s: the scatter plane is not enabled (rt_accum_set_features)", who);
  if ((guides && !(a->features & RT_ACCUM_FEAT_GUIDES)) || (emit && !(a->features & RT_ACCUM_FEAT_EMIT)))
    return set_error(RT_ERR_INVALID, "%s: the %s planes are not enabled (rt_accum_set_features)", who,
                     guides && !(a->features & RT_ACCUM_FEAT_GUIDES) ? "guide" : "emit");
  if (a->npix == 0) return RT_OK;
  DeviceGuard dg;
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  const size_t n = a->npix;
  const size_t floats[6] = {3 * n, 3 * n, n, 3 * n, 3 * n, n};
  float* dev[6];  // where the kernel writes: the caller's device buffer or the plane's staging slot
  size_t off = 0;
  for (int i = 0; i < 6; off += floats[i++]) dev[i] = !user[i] ? nullptr : host ? a->feat_stage + off : (float*)user[i];
  const FeatOut fo{dev[0], dev[1], dev[2], dev[3], dev[4], dev[5]};
  const bool planes = guides || emit;  // else: the scatter plane alone
  if (planes && a->per_pixel)
    hipLaunchKernelGGL(k_feat_resolve<true>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->F, a->ss,
                       px_counts(a), fo);
  else if (planes)
    hipLaunchKernelGGL(k_feat_resolve<false>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->F, a->ss,
                       Passes<false>{(uint32_t)a->passes}, fo);
  float* const dscat = !uscat ? nullptr : host ? a->feat_stage + 14 * n : uscat;
  if (dscat && a->per_pixel)
    hipLaunchKernelGGL(k_scatter_resolve<true>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->nscatter,
                       a->npix, a->ss, px_counts(a), dscat);
  else if (dscat)
    hipLaunchKernelGGL(k_scatter_resolve<false>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->nscatter,
                       a->npix, a->ss, Passes<false>{(uint32_t)a->passes}, dscat);
  HIP_OK(hipGetLastError());
  if (host && uscat) HIP_OK(hipMemcpyAsync(uscat, dscat, n * sizeof(float), hipMemcpyDeviceToHost, stream));
  for (int i = 0; host && i < 6; ++i)
    if (user[i]) HIP_OK(hipMemcpyAsync(user[i], dev[i], floats[i] * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}

// One pass as `who`: rt_accum_add's whole pass, or (active) rt_accum_add_active's over the selection
int accum_add(rt_accum* a, const char* who, bool active, uint64_t seed, rt_stats* stats) {
  if (!a) return set_error(RT_ERR_INVALID, "%s: null accumulator", who);
  std::lock_guard<std::mutex> lk(a->mu);
  if (active && !a->sel_valid)
    return set_error(RT_ERR_INVALID, "%s: no selection since the last pass or reset", who);
  if (active && a->sel_n == 0) {  // nothing to render: no pass is counted
    if (stats) memset(stats, 0, sizeof *stats);
    return RT_OK;
  }
  if (a->passes >= a->max_passes)
    return set_error(RT_ERR_INVALID, "%s: the accumulator holds its %d passes", who, a->max_passes);
  rt_render_opts o = a->opts;
  o.seed = seed;
  const PassSink sink = {(uint32_t)a->max_passes, fold_pass, a};
  // every pixel active: the plain whole pass (the same bits, the grouped chunk order)
  const bool part = active && a->sel_n < a->npix;
  const PixelMap pm = {a->map, a->sel_n};
  // the feature fold's view and scratch before the render starts; its mutex until the pass ends
  const bool fold = a->features && a->npix > 0;
  int rc = fold ? aov_fold_begin(a->scene, a->cd, o, part ? a->sel_n : a->npix) : RT_OK;
  if (rc) return rc;
  a->pass_map = part ? a->map : nullptr;
  rc = render_pass(a->scene, &a->cam, &o, stats, &sink, part ? &pm : nullptr);
  a->pass_map = nullptr;
  if (fold) aov_fold_end();
  if (rc == RT_OK) {
    ++a->passes;
    if (part) a->per_pixel = true;
    a->sel_valid = false;  // a selection describes the state it was made from
  }
  return rc;
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

// rt_pipeline_push: a copy of what it needs (rt_host_units.h)
int accum_view(rt_accum* a, AccumView* out) {
  std::lock_guard<std::mutex> lk(a->mu);
  *out = {a->cam,   (int32_t)a->W, (int32_t)a->rows, a->opts.device, a->opts.nranks, a->passes, a->features,
          a->opts.stream ? a->opts.stream : (void*)a->own_stream.s,
          a->opts.rank, (int32_t)a->cd.height, a->scene,
          (a->features & RT_ACCUM_FEAT_SPEC) ? a->S.max_k : 0, (a->features & RT_ACCUM_FEAT_SPEC) ? a->S.max_fuzz : 0.0f};
  return RT_OK;
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
  a->W = (uint32_t)cd.width;
  a->rows = a->W ? a->npix / a->W : 0u;
  const size_t total = carve(a, nullptr);
  DeviceGuard dg;
  auto zeroed = [&]() -> int {  // the one allocation, on the accumulator's device
    HIP_OK(hipSetDevice(o.device));
    if ((rc = a->buf.grow(total, "rt_accum_create"))) return rc;
    HIP_OK(hipMemset(a->buf.p, 0, total));
    return RT_OK;
  };
  if ((rc = zeroed())) {
    free_accum(a);
    return rc;
  }
  carve(a, a->buf.p);
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
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  HIP_OK(hipMemsetAsync(a->buf.p, 0, a->state_bytes, stream));
  HIP_OK(hipMemsetAsync(a->A.flags, 0, std::max<size_t>(a->npix, 1) * sizeof(uint32_t), stream));
  if (a->feat_buf.p) HIP_OK(hipMemsetAsync(a->feat_buf.p, 0, a->feat_state_bytes, stream));
  HIP_OK(hipStreamSynchronize(stream));
  a->passes = 0;
  a->per_pixel = a->sel_valid = a->sel_tiles = false;  // uniform again, no selection
  a->sel_n = 0;
  a->n_tiles = 0;
  return RT_OK;
}

}  // extern "C"

namespace rt {
namespace {
// rt_accum_set_features and rt_accum_set_features_spec (spec: that entry, which alone knows
// RT_ACCUM_FEAT_SPEC; spec_opts: the chain limits, null: the defaults)
int accum_set_features(const char* who, bool spec, rt_accum* a, uint32_t planes, const rt_aov_spec_opts* spec_opts) {
  if (!a) return set_error(RT_ERR_INVALID, "%s: null accumulator", who);
  // rt_accum_set_features takes the planes it always took: to it the chain group is an unknown bit
  if (planes & ~(RT_ACCUM_FEAT_GUIDES | RT_ACCUM_FEAT_EMIT | RT_ACCUM_FEAT_MEDIA | (spec ? RT_ACCUM_FEAT_SPEC : 0u)))
    return set_error(RT_ERR_INVALID, "%s: unknown planes 0x%x%s", who, planes,
                     planes & RT_ACCUM_FEAT_SPEC ? " (RT_ACCUM_FEAT_SPEC: rt_accum_set_features_spec)" : "");
  if (planes == RT_ACCUM_FEAT_MEDIA)
    return set_error(RT_ERR_INVALID, "%s: RT_ACCUM_FEAT_MEDIA modifies GUIDES / EMIT, it needs one", who);
  if (planes == RT_ACCUM_FEAT_SPEC)
    return set_error(RT_ERR_INVALID, "%s: RT_ACCUM_FEAT_SPEC goes with GUIDES / EMIT, it needs one", who);
  if ((planes & RT_ACCUM_FEAT_SPEC) && (planes & RT_ACCUM_FEAT_MEDIA))
    return set_error(RT_ERR_INVALID, "%s: RT_ACCUM_FEAT_SPEC does not combine with RT_ACCUM_FEAT_MEDIA (a chain traces no media)", who);
  rt_aov_spec_opts so{8, 0.0f};  // rt_render_aov_spec's defaults and range checks
  if (spec_opts) {
    if (spec_opts->max_bounces < 0 || spec_opts->max_bounces > 64)
      return set_error(RT_ERR_INVALID, "%s: max_bounces %d not in 0 .. 64", who, spec_opts->max_bounces);
    if (!(spec_opts->max_fuzz >= 0.0f) || !std::isfinite(spec_opts->max_fuzz))
      return set_error(RT_ERR_INVALID, "%s: max_fuzz must be finite and >= 0", who);
    if (spec_opts->max_bounces > 0) so.max_bounces = spec_opts->max_bounces;
    so.max_fuzz = spec_opts->max_fuzz;
  }
  std::lock_guard<std::mutex> lk(a->mu);
  if (a->passes > 0)
    return set_error(RT_ERR_INVALID, "%s: the accumulator holds %d passes (rt_accum_reset first)", who, a->passes);
  const int32_t max_k = std::max(0, std::min(so.max_bounces, a->cd.max_depth - 1));
  if (planes == a->features) {  // the same planes: only the chain limits may change
    if (planes & RT_ACCUM_FEAT_SPEC) a->S.max_k = max_k, a->S.max_fuzz = so.max_fuzz;
    return RT_OK;
  }
  DeviceGuard dg;
  HIP_OK(hipSetDevice(a->opts.device));
  drop_features(a);
  if (planes == 0) return RT_OK;
  const size_t total = carve_features(a, planes, nullptr);
  int rc = a->feat_buf.grow(total, who);
  if (rc == RT_OK && hipMemset(a->feat_buf.p, 0, total) != hipSuccess)
    rc = set_error(RT_ERR_DEVICE, "%s: clearing %zu bytes", who, total);
  if (rc) {
    drop_features(a);
    return rc;
  }
  if (planes & RT_ACCUM_FEAT_SPEC) a->S.max_k = max_k, a->S.max_fuzz = so.max_fuzz;
  carve_features(a, planes, a->feat_buf.p);
  a->features = planes;
  return RT_OK;
}

int accum_resolve_aov_spec(rt_accum* a, const rt_aov* outp, const rt_aov_spec* specp, bool host) {
  const char* who = host ? "rt_accum_resolve_aov_spec" : "rt_accum_resolve_aov_spec_device";
  if (!a) return set_error(RT_ERR_INVALID, "%s: null accumulator", who);
  if (outp && (outp->albedo || outp->material))
    return set_error(RT_ERR_INVALID, "%s: the accumulator keeps no albedo or material plane of the chain", who);
  float* const user[3] = {outp ? outp->normal : nullptr, outp ? outp->depth : nullptr, specp ? specp->bounces : nullptr};
  if (!user[0] && !user[1] && !user[2]) return set_error(RT_ERR_INVALID, "%s: no buffer wanted", who);
  std::lock_guard<std::mutex> lk(a->mu);
  if (!(a->features & RT_ACCUM_FEAT_SPEC))
    return set_error(RT_ERR_INVALID, "%s: the chain planes are not enabled (rt_accum_set_features_spec)", who);
  if (a->npix == 0) return RT_OK;
  DeviceGuard dg;
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  const size_t n = a->npix;
  const size_t floats[3] = {3 * n, n, n};
  float* dev[3];
  size_t off = 0;
  for (int i = 0; i < 3; off += floats[i++]) dev[i] = !user[i] ? nullptr : host ? a->spec_stage + off : user[i];
  if (a->per_pixel)
    hipLaunchKernelGGL(k_spec_resolve<true>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->S, a->ss,
                       px_counts(a), dev[0], dev[1], dev[2]);
  else
    hipLaunchKernelGGL(k_spec_resolve<false>, dim3((a->npix + 255) / 256), dim3(256), 0, stream, a->S, a->ss,
                       Passes<false>{(uint32_t)a->passes}, dev[0], dev[1], dev[2]);
  HIP_OK(hipGetLastError());
  for (int i = 0; host && i < 3; ++i)
    if (user[i]) HIP_OK(hipMemcpyAsync(user[i], dev[i], floats[i] * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}
}  // namespace
}  // namespace rt

extern "C" {

int rt_accum_set_features(rt_accum* a, uint32_t planes) {
  return rt::accum_set_features("rt_accum_set_features", false, a, planes, nullptr);
}

int rt_accum_set_features_spec(rt_accum* a, uint32_t planes, const rt_aov_spec_opts* spec_opts) {
  return rt::accum_set_features("rt_accum_set_features_spec", true, a, planes, spec_opts);
}

int rt_accum_resolve_aov_spec(rt_accum* a, const rt_aov* out_host, const rt_aov_spec* spec_host) {
  return rt::accum_resolve_aov_spec(a, out_host, spec_host, true);
}

int rt_accum_resolve_aov_spec_device(rt_accum* a, const rt_aov* out_dev, const rt_aov_spec* spec_dev) {
  return rt::accum_resolve_aov_spec(a, out_dev, spec_dev, false);
}

int rt_accum_get_features(rt_accum* a, uint32_t* planes) {
  if (!a || !planes) return rt::set_error(RT_ERR_INVALID, "rt_accum_get_features: null");
  std::lock_guard<std::mutex> lk(a->mu);
  *planes = a->features;
  return RT_OK;
}

int rt_accum_resolve_aov(rt_accum* a, const rt_aov* out_host, const rt_aov_emit* emit_host) {
  return rt::accum_resolve_aov(a, out_host, emit_host, nullptr, false, true);
}

int rt_accum_resolve_aov_device(rt_accum* a, const rt_aov* out_dev, const rt_aov_emit* emit_dev) {
  return rt::accum_resolve_aov(a, out_dev, emit_dev, nullptr, false, false);
}

int rt_accum_resolve_aov_media(rt_accum* a, const rt_aov* out_host, const rt_aov_emit* emit_host,
                               const rt_aov_media* media_host) {
  return rt::accum_resolve_aov(a, out_host, emit_host, media_host, true, true);
}

int rt_accum_resolve_aov_media_device(rt_accum* a, const rt_aov* out_dev, const rt_aov_emit* emit_dev,
                                      const rt_aov_media* media_dev) {
  return rt::accum_resolve_aov(a, out_dev, emit_dev, media_dev, true, false);
}

int rt_accum_add(rt_accum* a, uint64_t seed, rt_stats* stats) {
  return rt::accum_add(a, "rt_accum_add", false, seed, stats);
}

int rt_accum_add_active(rt_accum* a, uint64_t seed, rt_stats* stats) {
  return rt::accum_add(a, "rt_accum_add_active", true, seed, stats);
}

int rt_accum_select(rt_accum* a, const rt_adapt_opts* opts, uint64_t* n_active_pixels) {
  using namespace rt;
  rt_adapt_opts o;
  int rc;
  if ((rc = adapt_opts_ok("rt_accum_select", opts, &o))) return rc;
  if (!a) return set_error(RT_ERR_INVALID, "rt_accum_select: null accumulator");
  std::lock_guard<std::mutex> lk(a->mu);
  const TileGrid g = tile_grid(a, o.tile);
  if (a->npix == 0) {
    a->sel_tiles = true;
    a->n_tiles = 0;
    return selected(a, 0, n_active_pixels);
  }
  DeviceGuard dg;
  hipStream_t stream;
  if ((rc = accum_device(a, &stream))) return rc;
  a->sel_valid = a->sel_tiles = false;  // until the new selection stands
  a->n_tiles = 0;
  a->sel_n = 0;
  uint32_t* flag = (uint32_t*)a->stage_rgb;  // tiles <= pixels
  const uint32_t nt = g.tx * g.ty;
  hipLaunchKernelGGL(k_accum_tiles, dim3((nt + 255) / 256), dim3(256), 0, stream, a->A,
                     a->per_pixel ? a->count : nullptr, (uint32_t)a->passes, g, o.lum_floor, (uint32_t)o.min_passes,
                     o.rel_error, (float*)nullptr, flag);
  hipLaunchKernelGGL(k_count_stats, dim3(1), dim3(256), 0, stream, flag, nt, a->red + 4);
  HIP_OK(hipGetLastError());
  const ActiveSrc src = {flag, nullptr, g};
  if ((rc = compact_active(a, src, stream, n_active_pixels))) return rc;
  a->sel_tiles = true;
  a->n_tiles = (int32_t)nt;
  return RT_OK;
}

int rt_accum_set_active(rt_accum* a, const uint8_t* mask_host, uint64_t* n_active_pixels) {
  using namespace rt;
  if (!mask_host) return set_error(RT_ERR_INVALID, "rt_accum_set_active: null mask");
  if (!a) return set_error(RT_ERR_INVALID, "rt_accum_set_active: null accumulator");
  std::lock_guard<std::mutex> lk(a->mu);
  a->sel_tiles = false;
  a->n_tiles = 0;
  if (a->npix == 0) return selected(a, 0, n_active_pixels);
  DeviceGuard dg;
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  a->sel_valid = false;
  a->sel_n = 0;
  uint8_t* mask = (uint8_t*)a->stage_rgb;
  HIP_OK(hipMemcpyAsync(mask, mask_host, a->npix, hipMemcpyHostToDevice, stream));
  const ActiveSrc src = {nullptr, mask, tile_grid(a, 1)};
  return compact_active(a, src, stream, n_active_pixels);
}

int rt_accum_counts(rt_accum* a, int32_t* counts_host) { return rt::accum_counts(a, counts_host, true); }
int rt_accum_counts_device(rt_accum* a, int32_t* counts_dev) { return rt::accum_counts(a, counts_dev, false); }

int rt_accum_tile_error(rt_accum* a, const rt_adapt_opts* opts, float* err_host, int32_t* tiles_x,
                        int32_t* tiles_y) {
  using namespace rt;
  rt_adapt_opts o;
  int rc;
  if ((rc = adapt_opts_ok("rt_accum_tile_error", opts, &o))) return rc;
  if (!a) return set_error(RT_ERR_INVALID, "rt_accum_tile_error: null accumulator");
  std::lock_guard<std::mutex> lk(a->mu);
  const TileGrid g = tile_grid(a, o.tile);
  if (tiles_x) *tiles_x = (int32_t)g.tx;
  if (tiles_y) *tiles_y = (int32_t)g.ty;
  const uint32_t nt = g.tx * g.ty;
  if (!err_host || nt == 0) return RT_OK;
  DeviceGuard dg;
  hipStream_t stream;
  if ((rc = accum_device(a, &stream))) return rc;
  hipLaunchKernelGGL(k_accum_tiles, dim3((nt + 255) / 256), dim3(256), 0, stream, a->A,
                     a->per_pixel ? a->count : nullptr, (uint32_t)a->passes, g, o.lum_floor, (uint32_t)o.min_passes,
                     o.rel_error, a->stage_var, (uint32_t*)nullptr);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(err_host, a->stage_var, (size_t)nt * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}

int rt_accum_adapt_info(rt_accum* a, rt_adapt_info* out) {
  using namespace rt;
  if (!a || !out) return set_error(RT_ERR_INVALID, "rt_accum_adapt_info: null");
  std::lock_guard<std::mutex> lk(a->mu);
  memset(out, 0, sizeof *out);
  out->active_pixels = a->sel_n;
  out->n_tiles = a->n_tiles;
  out->min_count = out->max_count = a->passes;
  out->total_samples = (uint64_t)a->ss * (uint64_t)a->passes * a->npix;
  const bool tiles = a->sel_tiles && a->n_tiles > 0 && a->npix > 0;
  if (a->npix == 0 || (!a->per_pixel && !tiles)) return RT_OK;
  DeviceGuard dg;
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  if (a->per_pixel) {
    unsigned long long h[3];
    if ((rc = count_stats(a, stream, h))) return rc;
    out->min_count = (int32_t)h[0];
    out->max_count = (int32_t)h[1];
    out->total_samples = (uint64_t)a->ss * h[2];
  }
  if (tiles) {  // the last rt_accum_select's tile flags, summed when it ran
    unsigned long long h[3];
    HIP_OK(hipMemcpyAsync(h, a->red + 4, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    out->active_tiles = (int32_t)h[2];
  }
  return RT_OK;
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
  hipStream_t stream;
  int rc;
  if ((rc = accum_device(a, &stream))) return rc;
  const uint32_t nb = std::min<uint32_t>((a->npix + 255u) / 256u, (uint32_t)kInfoBlocks);
  double* res = a->part + 4 * (size_t)kInfoBlocks;
  if (a->per_pixel)
    hipLaunchKernelGGL(k_accum_info1<true>, dim3(nb), dim3(256), 0, stream, a->A, a->npix, px_counts(a), a->part);
  else
    hipLaunchKernelGGL(k_accum_info1<false>, dim3(nb), dim3(256), 0, stream, a->A, a->npix,
                       Passes<false>{(uint32_t)a->passes}, a->part);
  hipLaunchKernelGGL(k_accum_info2, dim3(1), dim3(256), 0, stream, a->part, nb, res);
  HIP_OK(hipGetLastError());
  double h[4];
  HIP_OK(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  if (a->per_pixel) {  // the most any pixel has
    unsigned long long c[3];
    if ((rc = count_stats(a, stream, c))) return rc;
    out->samples_per_pixel = (uint64_t)a->ss * c[1];
  }
  out->nonfinite_pixels = (uint64_t)h[3];
  if (h[2] > 0.0) {
    out->rms_std_error = sqrt(h[0] / h[2]);
    out->mean_luminance = h[1] / h[2];
  }
  out->rel_error = out->rms_std_error / (out->mean_luminance + 1e-6);
  return RT_OK;
}

}  // extern "C"
