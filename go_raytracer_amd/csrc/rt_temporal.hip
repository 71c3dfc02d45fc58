// rt_temporal.hip — temporal reprojection (rt_reproject, include/rt_abi.h): the previous frame's
// colour, variance and history length carried into the current camera through the depth and
// normal buffers, the stage Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017,
// put in front of the spatial filter (rt_denoise.hip's Var mode).  A pure image operation beside
// the denoiser: accumulate -> resolve -> reproject -> denoise -> quantize -> PPM in HBM.
//
//   k_reproject : one lane per pixel of the current frame, a wave = one 64-pixel row segment of a
//                 64 x 4 tile (every read and write of the current frame is a coalesced row
//                 segment).  The lane rebuilds the hit point from its depth, projects it into the
//                 previous camera and gathers the four bilinear taps of the previous frame, each
//                 tested against the reprojected depth and the current normal.  Both cameras
//                 travel as kernel arguments: they are wave-uniform, so they live in SGPRs and
//                 cost no memory traffic.  No LDS, no atomics: neighbouring lanes reproject to
//                 neighbouring pixels, so the taps are near-coherent gathers served by L1/L2, and
//                 the 12-byte pixels are read as three dword loads.  The tap loop is branch-free:
//                 coordinates clamped, an invalid tap's weight and values zeroed by selects (so a
//                 NaN in the previous frame never meets a multiply).
//
//   k_reproject<Emit> : the template twin of rt_reproject_emit.  Emit = true keeps the directly
//                 seen emission out of the history: every frame's pixel enters as z = (rgb -
//                 emission) / (1 - coverage), the surface radiance of the samples that saw no light,
//                 and the current frame's own emission is added back to the blend.  A tap whose
//                 emission is not finite or whose coverage is not in [0, 1) is invalid like any
//                 other: its values are selected to 0 and its divisor to 1 before the subtraction
//                 and the division.  Emit = false is rt_reproject's kernel, instruction for
//                 instruction (profiles/temporal_emit_device_code.txt).
//
//   k_reproject<true, Light> : the third instance, rt_reproject_light's.  Emission and coverage
//                 are history planes of their own: a second weight sum runs over the light taps
//                 (the surface taps and the fully covered ones), which blends the taps' emission
//                 and coverage by the same bilinear weights, and the pixel is re-lit from the
//                 blended planes, which are written out as the next history's.  It gathers no
//                 byte that <true, false> does not gather and writes 16 more per pixel.  The two
//                 other instances are what they were, instruction for instruction
//                 (profiles/temporal_light_device_code.txt).
//
//   k_reproject<Emit, Light, true> : rt_reproject_moments' three instances.  The second raw moment of
//                 luminance is one more history plane, gathered and blended with the colour's taps
//                 and weights; the variance comes from the moments (q - y^2) / (K - 1) once the
//                 history is min_frames long, and before that from an unweighted, depth- and
//                 normal-gated window of the current frame.  The window loop runs only in the lanes
//                 that need it (a first frame: all; a steady orbit: disocclusions), over clamped
//                 addresses, as L1/L2 gathers like the taps: lanes of a row read one row segment
//                 per step, shifted by one pixel from step to step.  LDS would need every lane of
//                 the tile, halo included, to stage Y, depth, normal and validity before a barrier,
//                 whether or not any lane needs the window.  out never aliases cur here.  The three
//                 Mom = false instances are what they were, instruction for instruction
//                 (profiles/temporal_moments_device_code.txt).
//
//   k_reproject<Emit, Light, true, true> : rt_reproject_clip's three instances.  Before the blend the
//                 history colour is clamped per channel to mean +- gamma sigma of the current frame's
//                 gated window (variance clipping; Salvi, GDC 2016).  One window pass per pixel
//                 (window_sums): the luminance sums of the spatial estimate and the six shifted
//                 colour sums come from the same loads, in every lane with a surface sample, so in
//                 a steady orbit nearly all of them.  That turns section 21's choice round: the
//                 block stages its 64 x 4 tile plus a halo of radius in LDS (the window's colour,
//                 depth, normal and a validity flag, from clamped addresses, all 256 lanes, one
//                 barrier) and the window reads LDS.  Measured against the gather loop it is 0.04 to
//                 0.09 ms faster at radius 3 and up to 2 x at radius 8.
//                 The clamp is fminf(fmaxf()) between the tap loop and the blend, on sums formed
//                 from selected values only.  The six other instances are what they were,
//                 instruction for instruction (profiles/temporal_clip_device_code.txt).
//
//   k_reproject<Emit, Light, true, Clip, true> : rt_reproject_spec's six instances.  The caller hands
//                 the specular chain's depth and normal for both frames (rt_accum_resolve_aov_spec), so
//                 the hit point rebuilt above is the virtual point behind the mirror, and one more
//                 plane, the chain's length: a pixel whose bounces value is not a whole number has no
//                 history, and a tap is taken only where its bounces value equals the pixel's, one
//                 more term of the tap rule and one more gathered dword per tap.  The tap loop stays
//                 branch-free and the Clip instances' LDS tile is what it was.  The nine other
//                 instances are what they were, instruction for instruction
//                 (profiles/temporal_spec_device_code.txt).
//
// Bytes per pixel: 36 read of the current frame (28 without var and count planes), up to 4 x 36
// gathered from the previous one (L1/L2-resident: adjacent lanes share three of four taps), 20
// written.  Emit: 16 more of the current pixel, 4 x 16 more gathered.  Light: 16 more written.
#include <hip/hip_runtime.h>
#include <math.h>

#include <mutex>

#include "rt_hip_util.h"
#include "rt_host_units.h"

namespace rt {
namespace {

constexpr int kTW = 64, kTH = 4;  // tile: one wave per row of 64 pixels

struct V3 {
  float x, y, z;
};

// everything wave-uniform: the two cameras relative to their centres (rt_abi.h's D, Ac, Uc, Vc,
// Ap, Up, Vp) and the resolved options
struct TpParams {
  int w, h, tiles_x;
  V3 d, ac, uc, vc, ap, up, vp;
  float max_history;  // 0: 8 x the current pixel's count
  float depth_tol, normal_tol, min_weight;
  float prev_count, cur_count;  // the frames' count_scalar
};

struct Planes {  // an rt_frame's buffers
  float* rgb;
  float* var;
  float* count;
  float* normal;
  float* depth;
};

// the emission split's planes of both frames (rt_aov_emit's emission and coverage); no member
// without it, so that k_reproject<false, false> takes rt_reproject's arguments.  Light: the two
// planes of the new history (either may be NULL)
template <bool Emit, bool Light>
struct EmitPlanes {};
template <>
struct EmitPlanes<true, false> {
  const float* prev_emission;
  const float* prev_coverage;
  const float* cur_emission;
  const float* cur_coverage;
};
template <>
struct EmitPlanes<true, true> {
  const float* prev_emission;
  const float* prev_coverage;
  const float* cur_emission;
  const float* cur_coverage;
  float* out_emission;
  float* out_coverage;
};

__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 load3(const float* p, size_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// rt_reproject_moments' own arguments (the moment planes and the resolved rt_moments_opts); no
// member without it, as EmitPlanes
template <bool Mom>
struct MomPlanes {};
template <>
struct MomPlanes<true> {
  const float* prev_lum2;  // NULL: no history at all (prev = NULL; the kernel's prev is then cur, never a tap)
  float* out_lum2;
  float min_frames;
  int radius;  // < 0: no spatial estimate
};

// rt_reproject_clip's own argument (the resolved rt_clip_opts); no member without it
template <bool Clip>
struct ClipArgs {};
template <>
struct ClipArgs<true> {
  float gamma;
};

// rt_reproject_spec's own arguments (rt_spec_planes); no member without it.  prev_bounces is the
// current plane when there is no previous frame (read through clamped addresses, never a tap)
template <bool Spec>
struct SpecArgs {};
template <>
struct SpecArgs<true> {
  const float* prev_bounces;
  const float* cur_bounces;
};

// a kernel's last argument: the sets as bases, so that an empty one takes no kernel argument space
template <bool Emit, bool Light, bool Mom, bool Clip, bool Spec = false>
struct Extra : EmitPlanes<Emit, Light>, MomPlanes<Mom>, ClipArgs<Clip>, SpecArgs<Spec> {};

__device__ __forceinline__ float lum(V3 a) { return 0.2126f * a.x + 0.7152f * a.y + 0.0722f * a.z; }

// the spatial estimate's b - a^2 with Bessel's factor, max(b - a^2, 0) T / (T - 1) (0 when T < 2),
// over the current frame's window around (x, y): rows then columns in ascending order, addresses
// clamped, a pixel outside the image or the rules selected to 0 before any arithmetic.  Called by
// the lanes that need it only: neighbouring lanes read neighbouring addresses, L1/L2 gathers as
// the taps'
template <bool Emit, bool Light>
__device__ __forceinline__ float window_var(const TpParams& P, const Planes& cur, const EmitPlanes<Emit, Light>& em,
                                            int x, int y, V3 np, float dp, int R) {
  const float tol_d = P.depth_tol * dp;
  float a = 0.0f, b = 0.0f, T = 0.0f;
  for (int dy = -R; dy <= R; ++dy) {
    const int ty = y + dy, cy = min(max(ty, 0), P.h - 1);
    for (int dx = -R; dx <= R; ++dx) {
      const int tx = x + dx, cx = min(max(tx, 0), P.w - 1);
      const size_t ti = (size_t)cy * P.w + cx;
      const V3 ct = load3(cur.rgb, ti), nt = load3(cur.normal, ti);
      const float vt = cur.var ? cur.var[ti] : 0.0f;
      const float cntt = cur.count ? cur.count[ti] : P.cur_count;
      const float dt = cur.depth[ti];
      const float nx = np.x - nt.x, ny = np.y - nt.y, nz = np.z - nt.z;
      bool ok = cx == tx && cy == ty && finite3(ct) && isfinite(vt) && isfinite(cntt) && cntt > 0.0f &&
                ((dx == 0 && dy == 0) ||
                 (fabsf(dt - dp) <= tol_d && nx * nx + ny * ny + nz * nz <= P.normal_tol));
      V3 xt = {ok ? ct.x : 0.0f, ok ? ct.y : 0.0f, ok ? ct.z : 0.0f};
      if constexpr (Emit) {
        const V3 et = load3(em.cur_emission, ti);
        const float covt = em.cur_coverage[ti];
        ok = ok && finite3(et) && covt >= 0.0f && covt < 1.0f;
        const float kt = ok ? 1.0f - covt : 1.0f;
        xt = {((ok ? ct.x : 0.0f) - (ok ? et.x : 0.0f)) / kt, ((ok ? ct.y : 0.0f) - (ok ? et.y : 0.0f)) / kt,
              ((ok ? ct.z : 0.0f) - (ok ? et.z : 0.0f)) / kt};
      }
      const float yt = lum(xt);
      a += yt;
      b += yt * yt;
      T += ok ? 1.0f : 0.0f;
    }
  }
  if (T < 2.0f) return 0.0f;
  const float am = a / T, bm = b / T;
  return fmaxf(bm - am * am, 0.0f) * (T / (T - 1.0f));
}

// rt_reproject_clip's window sums: window_var's luminance sums (the same statements in the same
// order, so v_s has window_var's bits) and, per channel, the sums of the deviations d = x_t - x_p
// from the current pixel's colour and of their squares.  An excluded pixel's d is selected to 0
struct WindowSums {
  float a, b, T;
  V3 A, B;
};

// over the tile k_reproject<.., true, true> stages in LDS: eight planes of npx = tw x th floats (x,
// depth, normal, validity without the gates), the lane at (lx, ly) of the tile.  A plane's row is
// read by the lanes of a wave at consecutive dwords: no bank conflict
__device__ __forceinline__ WindowSums window_sums(const TpParams& P, const float* s, int tw, int npx, int lx,
                                                      int ly, V3 np, float dp, V3 xp, int R) {
  const float tol_d = P.depth_tol * dp;
  float a = 0.0f, b = 0.0f, T = 0.0f;
  V3 A = {0.0f, 0.0f, 0.0f}, B = {0.0f, 0.0f, 0.0f};
  for (int dy = -R; dy <= R; ++dy) {
    for (int dx = -R; dx <= R; ++dx) {
      const int i = (ly + dy) * tw + lx + dx;
      const V3 st = {s[i], s[npx + i], s[2 * npx + i]}, nt = {s[4 * npx + i], s[5 * npx + i], s[6 * npx + i]};
      const float dt = s[3 * npx + i];
      const float nx = np.x - nt.x, ny = np.y - nt.y, nz = np.z - nt.z;
      const bool ok = s[7 * npx + i] > 0.0f &&
                      ((dx == 0 && dy == 0) ||
                       (fabsf(dt - dp) <= tol_d && nx * nx + ny * ny + nz * nz <= P.normal_tol));
      const V3 xt = {ok ? st.x : 0.0f, ok ? st.y : 0.0f, ok ? st.z : 0.0f};
      const float yt = lum(xt);
      a += yt;
      b += yt * yt;
      T += ok ? 1.0f : 0.0f;
      const V3 d = {ok ? xt.x - xp.x : 0.0f, ok ? xt.y - xp.y : 0.0f, ok ? xt.z - xp.z : 0.0f};
      A.x += d.x, A.y += d.y, A.z += d.z;
      B.x += d.x * d.x, B.y += d.y * d.y, B.z += d.z * d.z;
    }
  }
  return {a, b, T, A, B};
}

template <bool Emit, bool Light, bool Mom, bool Clip, bool Spec = false>
__global__ __launch_bounds__(256) void k_reproject(TpParams P, Planes prev, Planes cur, Planes out,
                                                   Extra<Emit, Light, Mom, Clip, Spec> ex) {
  const EmitPlanes<Emit, Light>& em = ex;
  const MomPlanes<Mom>& mo = ex;
  [[maybe_unused]] const float* tile = nullptr;
  [[maybe_unused]] int tile_w = 0, tile_n = 0;
  if constexpr (Clip) {
    // stage the 64 x 4 tile plus a halo of radius: the window's colour, depth, normal and validity
    // without the gates, from clamped addresses; every lane of the block takes part, one barrier
    extern __shared__ float s_tile[];
    const int R = mo.radius, tw = kTW + 2 * R, npx = tw * (kTH + 2 * R);
    const int ty0 = blockIdx.x / P.tiles_x, tx0 = blockIdx.x - ty0 * P.tiles_x;
    for (int i = threadIdx.x; i < npx; i += 256) {
      const int ly = i / tw, lx = i - ly * tw;
      const int gx = tx0 * kTW + lx - R, gy = ty0 * kTH + ly - R;
      const int cx = min(max(gx, 0), P.w - 1), cy = min(max(gy, 0), P.h - 1);
      const size_t ti = (size_t)cy * P.w + cx;
      const V3 ct = load3(cur.rgb, ti), nt = load3(cur.normal, ti);
      const float vt = cur.var ? cur.var[ti] : 0.0f;
      const float cntt = cur.count ? cur.count[ti] : P.cur_count;
      bool ok = cx == gx && cy == gy && finite3(ct) && isfinite(vt) && isfinite(cntt) && cntt > 0.0f;
      V3 xt = {ok ? ct.x : 0.0f, ok ? ct.y : 0.0f, ok ? ct.z : 0.0f};
      if constexpr (Emit) {
        const V3 et = load3(em.cur_emission, ti);
        const float covt = em.cur_coverage[ti];
        ok = ok && finite3(et) && covt >= 0.0f && covt < 1.0f;
        const float kt = ok ? 1.0f - covt : 1.0f;
        xt = {((ok ? ct.x : 0.0f) - (ok ? et.x : 0.0f)) / kt, ((ok ? ct.y : 0.0f) - (ok ? et.y : 0.0f)) / kt,
              ((ok ? ct.z : 0.0f) - (ok ? et.z : 0.0f)) / kt};
      }
      s_tile[i] = xt.x, s_tile[npx + i] = xt.y, s_tile[2 * npx + i] = xt.z;
      s_tile[3 * npx + i] = cur.depth[ti];
      s_tile[4 * npx + i] = nt.x, s_tile[5 * npx + i] = nt.y, s_tile[6 * npx + i] = nt.z;
      s_tile[7 * npx + i] = ok ? 1.0f : 0.0f;
    }
    __syncthreads();
    tile = s_tile, tile_w = tw, tile_n = npx;
  }
  static_assert(Emit || !Light, "the light history is a history of the emission split's planes");
  static_assert(Mom || !Clip, "the clip entries are the moments entries with one more step");
  static_assert(Mom || !Spec, "the specular entries are the clip entries with one more plane");
  const int tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
  const int x = tile_x * kTW + (threadIdx.x & (kTW - 1)), y = tile_y * kTH + (threadIdx.x >> 6);
  if (x >= P.w || y >= P.h) return;
  const size_t pi = (size_t)y * P.w + x;
  // the current pixel, read whole before any write: out may alias cur
  const V3 c = load3(cur.rgb, pi), np = load3(cur.normal, pi);
  const float v = cur.var ? cur.var[pi] : 0.0f;
  const float nc = cur.count ? cur.count[pi] : P.cur_count;
  const float dp = cur.depth[pi];
  bool valid = finite3(c) && isfinite(v) && isfinite(nc) && nc > 0.0f;
  // Emit: z = (c - e) / k and v_z = v / k^2 stand in for c and v up to the blend; a pixel whose
  // samples all saw the light (k = 0) carries no surface radiance and is not valid
  V3 e = {0.0f, 0.0f, 0.0f}, z = c;
  float kc = 1.0f, vz = v;
  float covc = 0.0f, wc = nc;  // Light: the current coverage, and the weight of the current z
  if constexpr (Emit) {
    e = load3(em.cur_emission, pi);
    const float cov = em.cur_coverage[pi];
    if constexpr (Light) {  // a fully covered pixel is valid: no surface sample (w_c = 0, divisor 1)
      valid = valid && finite3(e) && cov >= 0.0f && cov <= 1.0f;
      covc = cov;
      wc = cov < 1.0f ? nc : 0.0f;
      kc = valid && cov < 1.0f ? 1.0f - cov : 1.0f;
    } else {
      valid = valid && finite3(e) && cov >= 0.0f && cov < 1.0f;
      kc = valid ? 1.0f - cov : 1.0f;
    }
    z = {(c.x - e.x) / kc, (c.y - e.y) / kc, (c.z - e.z) / kc};
    vz = v / (kc * kc);
  }
  bool hist = valid && isfinite(dp) && dp > 0.0f && finite3(np);
  float qc = 0.0f, sq = 0.0f;  // Mom: the current pixel's second moment Y(z)^2, and the taps' sum
  if constexpr (Mom) {
    hist = hist && mo.prev_lum2 != nullptr;
    const float yc = lum(z);
    qc = yc * yc;
  }
  [[maybe_unused]] float bc = 0.0f;  // Spec: the chain length of the current pixel
  if constexpr (Spec) {  // no history unless every sample of the pixel took a chain of the same length
    const SpecArgs<true>& sp = ex;
    bc = sp.cur_bounces[pi];
    hist = hist && isfinite(bc) && bc >= 0.0f && bc == floorf(bc);
  }

  // the hit point relative to the previous centre, and its pixel in the previous camera
  const float fx = (float)x, fy = (float)y;
  const V3 dir = {P.ac.x + fx * P.uc.x + fy * P.vc.x, P.ac.y + fx * P.uc.y + fy * P.vc.y,
                  P.ac.z + fx * P.uc.z + fy * P.vc.z};
  const float t = dp / sqrtf(dot(dir, dir));
  const V3 r = {P.d.x + t * dir.x, P.d.y + t * dir.y, P.d.z + t * dir.z};
  const float d1 = sqrtf(dot(r, r));
  const V3 wp = {P.up.y * P.vp.z - P.up.z * P.vp.y, P.up.z * P.vp.x - P.up.x * P.vp.z,
                 P.up.x * P.vp.y - P.up.y * P.vp.x};
  const float s = dot(P.ap, wp) / dot(r, wp);
  hist = hist && isfinite(s) && s > 0.0f;
  const V3 q = {s * r.x - P.ap.x, s * r.y - P.ap.y, s * r.z - P.ap.z};
  float u = dot(q, P.up) / dot(P.up, P.up), vv = dot(q, P.vp) / dot(P.vp, P.vp);
  // beyond [-1, w) x [-1, h) no tap is inside: clamped there (NaN included) so that the
  // conversion to int is defined; such a pixel ends with S = 0
  u = hist ? fminf(fmaxf(u, -2.0f), (float)P.w + 1.0f) : -2.0f;
  vv = hist ? fminf(fmaxf(vv, -2.0f), (float)P.h + 1.0f) : -2.0f;
  const float u0 = floorf(u), v0 = floorf(vv);
  const int x0 = (int)u0, y0 = (int)v0;
  const float bu[2] = {1.0f - (u - u0), u - u0}, bv[2] = {1.0f - (vv - v0), vv - v0};
  const float tol_d = P.depth_tol * d1;

  float S = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, sn = 0.0f;
  float Sl = 0.0f, ser = 0.0f, seg = 0.0f, seb = 0.0f, sk = 0.0f, sm = 0.0f;  // Light: the light taps' sums
#pragma unroll
  for (int b = 0; b < 2; ++b) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int qx = x0 + a, qy = y0 + b;
      const int cx = min(max(qx, 0), P.w - 1), cy = min(max(qy, 0), P.h - 1);
      const size_t qi = (size_t)cy * P.w + cx;
      const V3 cq = load3(prev.rgb, qi), nq = load3(prev.normal, qi);
      const float vq = prev.var ? prev.var[qi] : 0.0f;
      const float cntq = prev.count ? prev.count[qi] : P.prev_count;
      const float dq = prev.depth[qi];
      const float nx = np.x - nq.x, ny = np.y - nq.y, nz = np.z - nq.z;
      bool ok = hist && cx == qx && cy == qy && finite3(cq) && isfinite(vq) && isfinite(cntq) &&
                cntq > 0.0f && dq > 0.0f && fabsf(dq - d1) <= tol_d &&
                nx * nx + ny * ny + nz * nz <= P.normal_tol;
      float lq = 0.0f;
      if constexpr (Mom) {  // one more term of the tap rule: a finite second moment
        lq = mo.prev_lum2 ? mo.prev_lum2[qi] : 0.0f;
        ok = ok && isfinite(lq);
      }
      if constexpr (Spec) {  // one more: the tap's chain is as long as the pixel's (a NaN fails)
        const SpecArgs<true>& sp = ex;
        ok = ok && sp.prev_bounces[qi] == bc;
      }
      V3 eq = {0.0f, 0.0f, 0.0f};
      float covq = 0.0f;
      bool okl = false;  // Light: a light tap (a surface tap, or a fully covered one)
      if constexpr (Emit) {
        eq = load3(em.prev_emission, qi);
        covq = em.prev_coverage[qi];
        if constexpr (Light) {
          okl = ok && finite3(eq) && covq >= 0.0f && covq <= 1.0f;
          ok = okl && covq < 1.0f;
        } else {
          ok = ok && finite3(eq) && covq >= 0.0f && covq < 1.0f;  // a NaN coverage fails both
        }
      }
      const float beta = ok ? bu[a] * bv[b] : 0.0f;
      V3 tq = {ok ? cq.x : 0.0f, ok ? cq.y : 0.0f, ok ? cq.z : 0.0f};
      float tv = ok ? vq : 0.0f;
      if constexpr (Emit) {  // the tap's z and v_z, from selected values only
        const float kq = ok ? 1.0f - covq : 1.0f;
        tq = {(tq.x - (ok ? eq.x : 0.0f)) / kq, (tq.y - (ok ? eq.y : 0.0f)) / kq,
              (tq.z - (ok ? eq.z : 0.0f)) / kq};
        tv = tv / (kq * kq);
      }
      S += beta;
      sr += beta * tq.x;
      sg += beta * tq.y;
      sb += beta * tq.z;
      sv += beta * beta * tv;
      sn += beta * (ok ? cntq : 0.0f);
      if constexpr (Mom) sq += beta * (ok ? lq : 0.0f);
      if constexpr (Light) {
        const float bl = okl ? bu[a] * bv[b] : 0.0f;
        Sl += bl;
        ser += bl * (okl ? eq.x : 0.0f);
        seg += bl * (okl ? eq.y : 0.0f);
        seb += bl * (okl ? eq.z : 0.0f);
        sk += bl * (okl ? covq : 0.0f);
        sm += bl * (okl ? cntq : 0.0f);
      }
    }
  }
  if constexpr (Mom) {
    // the three modes' blend in k_reproject<true, true>'s form (for the two others h_l = h_s and
    // w_c = n_c, and the written-out multiply-add is theirs), with the second moment blended by the
    // colour's weights and the variance taken from the moments or from the window
    const bool hs = hist && S >= P.min_weight;
    bool hl = hs;
    if constexpr (Light) hl = hist && Sl >= P.min_weight;
    const bool blend = (hs || hl) && (hs || wc > 0.0f);
    const bool surf = valid && wc > 0.0f;  // the current pixel has a surface sample
    const float inv = 1.0f / fmaxf(S, P.min_weight);
    const float cap = P.max_history > 0.0f ? P.max_history : 8.0f * nc;
    const float nh = hs ? fminf(sn * inv, cap) : 0.0f;
    const float n = nh + wc;
    const float K = hs && surf ? n / wc : 1.0f;  // the history length in frames
    const bool use_t = hs && surf && K >= mo.min_frames;
    float vs = 0.0f;
    [[maybe_unused]] V3 lo = {-INFINITY, -INFINITY, -INFINITY}, hi = {INFINITY, INFINITY, INFINITY};  // Clip: the box
    if constexpr (Clip) {
      // one window pass in every lane with a surface sample (radius >= 0: resolve_moments): v_s where
      // the pixel takes it, and the box mean +- gamma sigma, which overrules the history colour of a
      // pixel with surface history and at least two window pixels.  Any other pixel's box is the
      // whole line, which leaves xh's bits alone
      const ClipArgs<true>& cl = ex;
      if (surf) {
        const WindowSums ws = window_sums(P, tile, tile_w, tile_n, (int)(threadIdx.x & (kTW - 1)) + mo.radius,
                                          (int)(threadIdx.x >> 6) + mo.radius, np, dp, z, mo.radius);
        if (ws.T >= 2.0f) {
          const float am = ws.a / ws.T, bm = ws.b / ws.T;
          if (!use_t) vs = fmaxf(bm - am * am, 0.0f) * (ws.T / (ws.T - 1.0f)) / K;
          if (hs) {
            const V3 mA = {ws.A.x / ws.T, ws.A.y / ws.T, ws.A.z / ws.T};
            const V3 sd = {cl.gamma * sqrtf(fmaxf(ws.B.x / ws.T - mA.x * mA.x, 0.0f)),
                           cl.gamma * sqrtf(fmaxf(ws.B.y / ws.T - mA.y * mA.y, 0.0f)),
                           cl.gamma * sqrtf(fmaxf(ws.B.z / ws.T - mA.z * mA.z, 0.0f))};
            const V3 m = {z.x + mA.x, z.y + mA.y, z.z + mA.z};
            lo = {m.x - sd.x, m.y - sd.y, m.z - sd.z};
            hi = {m.x + sd.x, m.y + sd.y, m.z + sd.z};
          }
        }
      }
    } else {
      if (mo.radius >= 0 && surf && !use_t) vs = window_var<Emit, Light>(P, cur, em, x, y, np, dp, mo.radius) / K;
    }
    V3 o = c, oe = e;
    float ov = v, on = nc, oc = covc, oq = 0.0f;
    if (blend) {
      const float in = 1.0f / n, vh = sv * (inv * inv);
      if constexpr (Clip) {  // the history colour, clamped to the box; the blend is the one below
        o.x = fmaf(wc, z.x, nh * fminf(fmaxf(sr * inv, lo.x), hi.x)) * in;
        o.y = fmaf(wc, z.y, nh * fminf(fmaxf(sg * inv, lo.y), hi.y)) * in;
        o.z = fmaf(wc, z.z, nh * fminf(fmaxf(sb * inv, lo.z), hi.z)) * in;
      } else {
        o.x = fmaf(wc, z.x, nh * (sr * inv)) * in;
        o.y = fmaf(wc, z.y, nh * (sg * inv)) * in;
        o.z = fmaf(wc, z.z, nh * (sb * inv)) * in;
      }
      ov = fmaf(wc * wc, vz, nh * nh * vh) * (in * in);
      oq = (nh * (sq * inv) + wc * qc) * in;  // q before the blend, then the colour's weights
      if (mo.radius >= 0 && surf) {
        float yo = lum(o);
        // Clip: Y with its contraction written out as the moments instances have it (the 0.7152 g
        // product rounded, the two others fused), so that an unclamped pixel keeps their bits
        if constexpr (Clip) yo = fmaf(0.0722f, o.z, fmaf(0.2126f, o.x, 0.7152f * o.y));
        ov = use_t ? fmaxf(oq - yo * yo, 0.0f) / (K - 1.0f) : vs;
      }
      float ko = kc;
      if constexpr (Light) {
        const float invl = 1.0f / fmaxf(Sl, P.min_weight);
        const float mh = hl ? fminf(sm * invl, cap) : 0.0f;
        on = fmaxf(nh, mh) + nc;
        const float im = 1.0f / (mh + nc);
        oc = (mh * (sk * invl) + nc * covc) * im;
        oe = {(mh * (ser * invl) + nc * e.x) * im, (mh * (seg * invl) + nc * e.y) * im,
              (mh * (seb * invl) + nc * e.z) * im};
        ko = 1.0f - oc;
        o = {ko * o.x + oe.x, ko * o.y + oe.y, ko * o.z + oe.z};
        ov = ko * ko * ov;
      } else {
        on = n;
        if constexpr (Emit) {
          o = {kc * o.x + e.x, kc * o.y + e.y, kc * o.z + e.z};
          ov = kc * kc * ov;
        }
      }
    } else if (surf) {  // no history: the pixel's own colour, its own moment, the window's variance
      oq = qc;
      if (mo.radius >= 0) ov = kc * kc * vs;
    }
    if (out.rgb) out.rgb[3 * pi] = o.x, out.rgb[3 * pi + 1] = o.y, out.rgb[3 * pi + 2] = o.z;
    if (out.var) out.var[pi] = ov;
    if (out.count) out.count[pi] = on;
    if constexpr (Light) {
      if (em.out_emission)
        em.out_emission[3 * pi] = oe.x, em.out_emission[3 * pi + 1] = oe.y, em.out_emission[3 * pi + 2] = oe.z;
      if (em.out_coverage) em.out_coverage[pi] = oc;
    }
    mo.out_lum2[pi] = oq;
    return;
  }
  if constexpr (Light) {
    // n_h from the surface taps, m_h from the light taps; a sum below min_weight is no history of
    // its kind.  Nothing to blend: neither history, or a pixel covered now (w_c = 0) without
    // surface history: the inside of a light
    const bool hs = hist && S >= P.min_weight, hl = hist && Sl >= P.min_weight;
    V3 o = c, oe = e;
    float ov = v, on = nc, oc = covc;
    if ((hs || hl) && (hs || wc > 0.0f)) {
      // a sum that is no history divides by min_weight (> 0: resolve()) and its weight below is 0;
      // the maximum leaves a sum that is one untouched, and the division is the other instances'
      const float inv = 1.0f / fmaxf(S, P.min_weight), invl = 1.0f / fmaxf(Sl, P.min_weight);
      const float cap = P.max_history > 0.0f ? P.max_history : 8.0f * nc;
      const float nh = hs ? fminf(sn * inv, cap) : 0.0f, vh = sv * (inv * inv);
      const float mh = hl ? fminf(sm * invl, cap) : 0.0f;
      const float n = nh + wc, in = 1.0f / n;
      // (restated in the Mom branch above: a change here goes there too)
      // the blend below, with its one fused multiply-add written out as the compiler contracts it in
      // the two other instances: zero emission and coverage must give rt_reproject's bits
      o.x = fmaf(wc, z.x, nh * (sr * inv)) * in;
      o.y = fmaf(wc, z.y, nh * (sg * inv)) * in;
      o.z = fmaf(wc, z.z, nh * (sb * inv)) * in;
      ov = fmaf(wc * wc, vz, nh * nh * vh) * (in * in);
      on = fmaxf(nh, mh) + nc;
      const float im = 1.0f / (mh + nc);
      oc = (mh * (sk * invl) + nc * covc) * im;
      oe = {(mh * (ser * invl) + nc * e.x) * im, (mh * (seg * invl) + nc * e.y) * im,
            (mh * (seb * invl) + nc * e.z) * im};
      const float ko = 1.0f - oc;  // re-lit from the blended planes; the light adds no variance
      o = {ko * o.x + oe.x, ko * o.y + oe.y, ko * o.z + oe.z};
      ov = ko * ko * ov;
    }
    if (out.rgb) out.rgb[3 * pi] = o.x, out.rgb[3 * pi + 1] = o.y, out.rgb[3 * pi + 2] = o.z;
    if (out.var) out.var[pi] = ov;
    if (out.count) out.count[pi] = on;
    if (em.out_emission)
      em.out_emission[3 * pi] = oe.x, em.out_emission[3 * pi + 1] = oe.y, em.out_emission[3 * pi + 2] = oe.z;
    if (em.out_coverage) em.out_coverage[pi] = oc;
    return;
  }
  hist = hist && S >= P.min_weight;

  V3 o = c;
  float ov = v, on = nc;
  if (hist) {
    const float inv = 1.0f / S;
    const float cap = P.max_history > 0.0f ? P.max_history : 8.0f * nc;
    const float nh = fminf(sn * inv, cap), vh = sv * (inv * inv);
    const float n = nh + nc, in = 1.0f / n;
    // (the Mom branch above restates this blend and the Light one: a change here goes there too, or
    // tests/test_reproject_moments_gpu.py's bit identity with these instances fails)
    o.x = (nh * (sr * inv) + nc * z.x) * in;
    o.y = (nh * (sg * inv) + nc * z.y) * in;
    o.z = (nh * (sb * inv) + nc * z.z) * in;
    ov = (nh * nh * vh + nc * nc * vz) * (in * in);
    on = n;
    if constexpr (Emit) {  // re-lit by the current frame's own emission, which adds no variance
      o = {kc * o.x + e.x, kc * o.y + e.y, kc * o.z + e.z};
      ov = kc * kc * ov;
    }
  }
  if (out.rgb) out.rgb[3 * pi] = o.x, out.rgb[3 * pi + 1] = o.y, out.rgb[3 * pi + 2] = o.z;
  if (out.var) out.var[pi] = ov;
  if (out.count) out.count[pi] = on;
}

// ---- host -------------------------------------------------------------------------------------
// The twelve entries fill a ReprojectRequest (rt_host_units.h) and reproject_impl runs the stages
// reproject_check -> reproject_bind -> reproject_launch -> reproject_collect over one ReprojectJob,
// as rt_aov.hip's entries do (DESIGN.md section 17 "Host path").

std::mutex g_mu;        // one host-staged call at a time: the staging buffer is shared
DeviceScratch g_stage;  // the host entries' staged frames (72 B per pixel, 104 with the emit planes;
                        // rt_reproject_moments: 100, 132 and in the light mode 148)

V3 v3(const double* a) { return {(float)a[0], (float)a[1], (float)a[2]}; }
V3 v3_diff(const double* a, const double* b) {  // the difference in fp64, then rounded
  return {(float)(a[0] - b[0]), (float)(a[1] - b[1]), (float)(a[2] - b[2])};
}

constexpr float kClipGamma = 0.75f;  // rt_clip_opts' default gamma (DESIGN.md section 22's sweep)

// a frame's planes in staging order, rt_frame's five and the emit struct's emission and coverage,
// and the floats per pixel of each
constexpr int kFloats[7] = {3, 1, 1, 3, 1, 3, 1};
struct UserFrame {
  float* p[7];
};
UserFrame user_frame(const rt_frame* f, const rt_aov_emit* e) {
  UserFrame u = {{f->rgb, f->var, f->count, f->normal, f->depth}};
  if (e) u.p[5] = e->emission, u.p[6] = e->coverage;
  return u;
}

// One plane of a call: the caller's pointer and the kernel's pointer to the plane, as read (src,
// in) and as written (dst, out); cur's rgb is both when out goes over it.  A device entry's planes
// are used in place.  A host entry's take `floats` per pixel of the staging buffer each, in the
// order listed: dev is the slot, which an absent plane keeps, filled from src and copied back to dst
struct TpPlane {
  int floats;
  const float* src;
  const float** in;
  float* dst;
  float** out;
  float* dev;
};

// What the stages derive from a request
struct ReprojectJob {
  bool emit, light;      // the mode: the _emit and _light kernels
  bool mom, clip, spec;  // the moments family, and its copts and spec given
  bool no_prev;          // the moments family's prev == NULL: no history at all
  // the request's structs the mode takes (NULL: dropped), and the history the kernel reads: the
  // current frame's when there is none (clamped addresses need memory behind them; never a tap)
  const rt_camera* cam_prev;
  const rt_frame* prev;
  const rt_aov_emit *prev_emit, *cur_emit, *out_emit;
  TpParams P;
  MomPlanes<true> mo;
  ClipArgs<true> cl;
  SpecArgs<true> sp;
  hipStream_t stream;
  const float *d_prev[7], *d_cur[7];  // the kernel's planes, in UserFrame's order (reproject_bind)
  float* d_out[7];
  TpPlane planes[24];  // 14 of the frames, 7 of the moments family, 2 of spec
  int n_planes;
};

// argument checks of every entry point (before any device is touched) -> the kernel's parameters;
// emit: the _emit and _light entries, which need both rt_aov_emit with emission and coverage;
// light: the _light entries, which need out_emit (NULL for the others)
int resolve(const ReprojectRequest& rq, ReprojectJob* j) {
  const char* who = rq.name;
  const bool emit = j->emit, light = j->light;
  const rt_frame *prev = j->prev, *cur = rq.cur, *out = rq.out;
  const rt_aov_emit *prev_emit = j->prev_emit, *cur_emit = j->cur_emit, *out_emit = j->out_emit;
  const int w = rq.w, h = rq.h;
  if (!j->cam_prev || !rq.cam_cur) return set_error(RT_ERR_INVALID, "%s: null camera", who);
  if (!prev || !cur || !out) return set_error(RT_ERR_INVALID, "%s: null frame", who);
  if (emit && (!prev_emit || !cur_emit)) return set_error(RT_ERR_INVALID, "%s: null emit", who);
  if (light && !out_emit) return set_error(RT_ERR_INVALID, "%s: null out_emit", who);
  if (!prev->rgb || !prev->normal || !prev->depth || !cur->rgb || !cur->normal || !cur->depth)
    return set_error(RT_ERR_INVALID, "%s: prev and cur need rgb, normal and depth", who);
  if (emit && (!prev_emit->emission || !prev_emit->coverage || !cur_emit->emission || !cur_emit->coverage))
    return set_error(RT_ERR_INVALID, "%s: prev_emit and cur_emit need emission and coverage", who);
  if (!out->rgb && !out->var && !out->count) return set_error(RT_ERR_INVALID, "%s: out has no buffer", who);
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31) / 3)
    return set_error(RT_ERR_INVALID, "%s: %d x %d image", who, w, h);
  const rt_reproject_opts o = rq.opts ? *rq.opts : rt_reproject_opts{};
  for (float f : {o.max_history, o.depth_tol, o.normal_tol, o.min_weight})
    if (!(f >= 0.0f) || !isfinite(f)) return set_error(RT_ERR_INVALID, "%s: negative or non-finite option", who);
  const float* const prev_bufs[5] = {prev->rgb, prev->var, prev->count, prev->normal, prev->depth};
  for (const float* ob : {out->rgb, out->var, out->count})
    for (const float* pb : prev_bufs)
      if (ob && ob == pb)
        return set_error(RT_ERR_INVALID, "%s: out aliases a buffer of prev (the taps gather from prev)", who);
  if (emit)
    for (const float* ob : {out->rgb, out->var, out->count})
      for (const float* pb : {prev_emit->emission, prev_emit->surface_albedo, prev_emit->coverage})
        if (ob && ob == pb)
          return set_error(RT_ERR_INVALID, "%s: out aliases a buffer of prev_emit (the taps gather from prev)", who);
  if (light)
    for (const float* ob : {out_emit->emission, out_emit->coverage}) {
      for (const float* pb : prev_bufs)
        if (ob && ob == pb)
          return set_error(RT_ERR_INVALID, "%s: out_emit aliases a buffer of prev (the taps gather from prev)", who);
      for (const float* pb : {prev_emit->emission, prev_emit->surface_albedo, prev_emit->coverage})
        if (ob && ob == pb)
          return set_error(RT_ERR_INVALID, "%s: out_emit aliases a buffer of prev_emit (the taps gather from prev)",
                           who);
    }
  rt_camera_derived dp, dc;
  int rc = rt_camera_derive(j->cam_prev, &dp);
  if (rc == RT_OK) rc = rt_camera_derive(rq.cam_cur, &dc);
  if (rc != RT_OK) return rc;
  if (dp.width != w || dp.height != h || dc.width != w || dc.height != h)
    return set_error(RT_ERR_INVALID, "%s: cameras of %d x %d and %d x %d for a %d x %d image", who, dp.width,
                     dp.height, dc.width, dc.height, w, h);
  if (dp.defocus_angle > 0.0 || dc.defocus_angle > 0.0)
    return set_error(RT_ERR_UNSUPPORTED, "%s: a defocus camera measures depth from the lens sample", who);
  TpParams* P = &j->P;
  P->w = w;
  P->h = h;
  P->tiles_x = (w + kTW - 1) / kTW;
  P->d = v3_diff(dc.center, dp.center);
  P->ac = v3_diff(dc.pixel00, dc.center);
  P->uc = v3(dc.delta_u);
  P->vc = v3(dc.delta_v);
  P->ap = v3_diff(dp.pixel00, dp.center);
  P->up = v3(dp.delta_u);
  P->vp = v3(dp.delta_v);
  P->max_history = o.max_history;
  P->depth_tol = o.depth_tol > 0.0f ? o.depth_tol : 0.05f;
  P->normal_tol = o.normal_tol > 0.0f ? o.normal_tol : 0.1f;
  P->min_weight = o.min_weight > 0.0f ? o.min_weight : 0.01f;
  P->prev_count = prev->count_scalar;
  P->cur_count = cur->count_scalar;
  return RT_OK;
}

// the moments entries' own checks, ahead of the mode's (resolve).  prev == NULL is no history at
// all: the job's history becomes the current frame, which the kernel reads and never takes a tap from
int resolve_moments(const ReprojectRequest& rq, ReprojectJob* j) {
  const char* who = rq.name;
  const rt_frame *prev = rq.prev, *cur = rq.cur, *out = rq.out;
  if (!rq.out_lum2) return set_error(RT_ERR_INVALID, "%s: null out_lum2", who);
  const bool no_prev = !prev;
  if (!no_prev && !rq.prev_lum2) return set_error(RT_ERR_INVALID, "%s: prev without prev_lum2", who);
  const float* ob[5] = {out ? out->rgb : nullptr, out ? out->var : nullptr, out ? out->count : nullptr,
                        j->out_emit ? j->out_emit->emission : nullptr, j->out_emit ? j->out_emit->coverage : nullptr};
  if (j->spec) {  // the specular entries' own: the chain lengths of both frames, inputs only
    if (!rq.spec->cur_bounces) return set_error(RT_ERR_INVALID, "%s: spec without cur_bounces", who);
    if (!no_prev && !rq.spec->prev_bounces) return set_error(RT_ERR_INVALID, "%s: prev without spec's prev_bounces", who);
    for (const float* o : {ob[0], ob[1], ob[2], ob[3], ob[4], (const float*)rq.out_lum2})
      if (o && (o == rq.spec->cur_bounces || (!no_prev && o == rq.spec->prev_bounces)))
        return set_error(RT_ERR_INVALID, "%s: a bounces plane is an out buffer", who);
  }
  const rt_moments_opts mop = rq.mopts ? *rq.mopts : rt_moments_opts{};
  if (mop.radius < -1 || mop.radius > 8)
    return set_error(RT_ERR_INVALID, "%s: radius %d (-1: no spatial estimate; at most 8)", who, mop.radius);
  if (!(mop.min_frames >= 0.0f) || !isfinite(mop.min_frames) || (mop.min_frames > 0.0f && mop.min_frames < 2.0f))
    return set_error(RT_ERR_INVALID, "%s: min_frames must be 0 (the default) or a finite number >= 2", who);
  if (j->clip) {  // the clip entries' own: the box is the window's
    if (mop.radius == -1)
      return set_error(RT_ERR_INVALID, "%s: clipping needs the window (radius -1 has none)", who);
    if (!(rq.copts->gamma >= 0.0f) || !isfinite(rq.copts->gamma))
      return set_error(RT_ERR_INVALID, "%s: gamma must be 0 (the default) or a finite positive number", who);
  }
  const float* in[17] = {};  // every input plane
  int ni = 0;
  if (!no_prev) {
    for (const float* b : {(const float*)prev->rgb, (const float*)prev->var, (const float*)prev->count,
                           (const float*)prev->normal, (const float*)prev->depth, rq.prev_lum2})
      in[ni++] = b;
    if (j->prev_emit)
      for (const float* b : {j->prev_emit->emission, j->prev_emit->surface_albedo, j->prev_emit->coverage}) in[ni++] = b;
  }
  const int first_cur = ni;
  if (cur)
    for (const float* b : {cur->rgb, cur->var, cur->count, cur->normal, cur->depth}) in[ni++] = b;
  if (j->cur_emit)
    for (const float* b : {j->cur_emit->emission, j->cur_emit->surface_albedo, j->cur_emit->coverage}) in[ni++] = b;
  for (int i = 0; i < ni; ++i)
    if (in[i] == rq.out_lum2) return set_error(RT_ERR_INVALID, "%s: out_lum2 aliases an input plane", who);
  for (const float* o : ob) {
    if (o && o == rq.out_lum2) return set_error(RT_ERR_INVALID, "%s: out_lum2 aliases a buffer of out", who);
    if (o && !no_prev && o == rq.prev_lum2)
      return set_error(RT_ERR_INVALID, "%s: out aliases prev_lum2 (the taps gather from prev)", who);
  }
  for (const float* o : ob)
    for (int i = first_cur; i < ni; ++i)
      if (o && o == in[i])
        return set_error(RT_ERR_INVALID,
                         "%s: out aliases a buffer of cur (the window reads the current frame's neighbours)", who);
  j->no_prev = no_prev;
  if (no_prev) j->cam_prev = rq.cam_cur, j->prev = cur, j->prev_emit = j->cur_emit;
  j->mo.min_frames = mop.min_frames > 0.0f ? mop.min_frames : 4.0f;
  j->mo.radius = mop.radius == 0 ? 3 : mop.radius;
  if (j->clip) j->cl.gamma = rq.copts->gamma > 0.0f ? rq.copts->gamma : kClipGamma;
  return RT_OK;
}

// Every argument test, in the entries' fixed order; no device is touched.  The mode decides which
// of the request's emit structs are read: the others are dropped here, once
int reproject_check(const ReprojectRequest& rq, ReprojectJob* j) {
  if (rq.mode < RT_REPROJECT_PLAIN || rq.mode > RT_REPROJECT_LIGHT)
    return set_error(RT_ERR_INVALID, "%s: mode %d", rq.name, rq.mode);
  j->emit = rq.mode != RT_REPROJECT_PLAIN, j->light = rq.mode == RT_REPROJECT_LIGHT;
  j->mom = rq.moments, j->clip = rq.moments && rq.copts, j->spec = rq.moments && rq.spec;
  j->cam_prev = rq.cam_prev, j->prev = rq.prev;
  j->prev_emit = j->emit ? rq.prev_emit : nullptr;
  j->cur_emit = j->emit ? rq.cur_emit : nullptr;
  j->out_emit = j->light ? rq.out_emit : nullptr;
  if (int rc = j->mom ? resolve_moments(rq, j) : RT_OK) return rc;
  return resolve(rq, j);
}

// The call's planes, listed in the host entries' staging order (the results depend on which slots
// alias), then bound: device pointers in place, host pointers to their slots and copied in
int reproject_bind(const ReprojectRequest& rq, ReprojectJob* j) {
  const size_t n = (size_t)rq.w * rq.h;
  const UserFrame pv = j->no_prev ? UserFrame{} : user_frame(j->prev, j->prev_emit);  // not copied without history
  const UserFrame cu = user_frame(rq.cur, j->cur_emit);
  UserFrame ou = user_frame(rq.out, j->out_emit);
  ou.p[3] = ou.p[4] = nullptr;  // no normal or depth is written
  const int nf = j->emit ? 7 : 5;
  TpPlane* p = j->planes;
  for (int k = 0; k < nf; ++k) *p++ = {kFloats[k], pv.p[k], &j->d_prev[k]};
  // without moments out is written over cur's copy (out may alias cur), into the var and count slots
  // also when cur has neither, and out_emit over cur_emit's copy
  for (int k = 0; k < nf; ++k)
    *p++ = {kFloats[k], cu.p[k], &j->d_cur[k], j->mom ? nullptr : ou.p[k], j->mom ? nullptr : &j->d_out[k]};
  if (j->mom) {  // beside the frames instead (the window reads cur's copy): prev's lum2, then out
    *p++ = {1, j->no_prev ? nullptr : rq.prev_lum2, &j->mo.prev_lum2};
    for (int k : {0, 1, 2}) *p++ = {kFloats[k], nullptr, nullptr, ou.p[k], &j->d_out[k]};
    *p++ = {1, nullptr, nullptr, rq.out_lum2, &j->mo.out_lum2};
    if (j->light)
      for (int k : {5, 6}) *p++ = {kFloats[k], nullptr, nullptr, ou.p[k], &j->d_out[k]};
  }
  if (j->spec) {  // last: the two bounces planes
    *p++ = {1, j->no_prev ? nullptr : rq.spec->prev_bounces, &j->sp.prev_bounces};
    *p++ = {1, rq.spec->cur_bounces, &j->sp.cur_bounces};
  }
  j->n_planes = (int)(p - j->planes);
  float* slot = nullptr;
  if (rq.host) {
    size_t floats = 0;
    for (int i = 0; i < j->n_planes; ++i) floats += j->planes[i].floats;
    void* stg = nullptr;
    if (int rc = g_stage.get(0, n * 4 * floats, &stg, rq.name)) return rc;
    slot = (float*)stg;
  }
  for (p = j->planes; p != j->planes + j->n_planes; ++p) {
    if (rq.host) p->dev = p->src || p->dst ? slot : nullptr, slot += p->floats * n;
    if (p->in) *p->in = rq.host && p->src ? p->dev : p->src;
    if (p->out) *p->out = rq.host && p->dst ? p->dev : p->dst;
    if (rq.host && p->src) HIP_OK(hipMemcpyAsync(p->dev, p->src, n * 4 * p->floats, hipMemcpyHostToDevice, j->stream));
  }
  if (j->no_prev) {  // read through clamped addresses, never a tap
    std::copy(j->d_cur, j->d_cur + 7, j->d_prev);
    j->sp.prev_bounces = j->sp.cur_bounces;
  }
  return RT_OK;
}

Planes planes_of(const float* const* p) {
  return {(float*)p[0], (float*)p[1], (float*)p[2], (float*)p[3], (float*)p[4]};
}
template <bool Emit, bool Light>
EmitPlanes<Emit, Light> emit_planes_of(const ReprojectJob& j) {
  if constexpr (Light)
    return {j.d_prev[5], j.d_prev[6], j.d_cur[5], j.d_cur[6], j.d_out[5], j.d_out[6]};
  else if constexpr (Emit)
    return {j.d_prev[5], j.d_prev[6], j.d_cur[5], j.d_cur[6]};
  else
    return {};
}
// an argument set of Extra: the job's when the instance takes it, else the empty one
template <template <bool> class Set, bool On>
Set<On> set_if(const Set<true>& v) {
  if constexpr (On)
    return v;
  else
    return {};
}

// The kernel table: k_reproject<Emit, Light, Mom, Clip, Spec> by the job's five flags.  Light needs
// Emit, Clip and Spec need Mom: 3 plain + 3 moments + 3 clip + 6 spec = 15 instances and no other
int reproject_launch(const ReprojectJob& j) {
  const unsigned tiles = (unsigned)((int64_t)j.P.tiles_x * ((j.P.h + kTH - 1) / kTH));  // < 2^31 / 3: w h is
  const Planes prev = planes_of(j.d_prev), cur = planes_of(j.d_cur), out = planes_of(j.d_out);
  // Clip: the tile and its halo in LDS, 8 floats a pixel, 22 KB at radius 3, 51 KB at radius 8
  const size_t lds = j.clip ? (size_t)(kTW + 2 * j.mo.radius) * (kTH + 2 * j.mo.radius) * 32 : 0;
  with_flag(j.emit, [&](auto e) {
    with_flag(j.light, [&](auto l) {
      with_flag(j.mom, [&](auto m) {
        with_flag(j.clip, [&](auto c) {
          with_flag(j.spec, [&](auto s) {
            constexpr bool E = decltype(e)::value, L = decltype(l)::value, M = decltype(m)::value,
                           C = decltype(c)::value, S = decltype(s)::value;
            if constexpr ((E || !L) && (M || (!C && !S)))
              hipLaunchKernelGGL((k_reproject<E, L, M, C, S>), dim3(tiles), dim3(256), lds, j.stream, j.P, prev, cur, out,
                                 Extra<E, L, M, C, S>{emit_planes_of<E, L>(j), set_if<MomPlanes, M>(j.mo),
                                                      set_if<ClipArgs, C>(j.cl), set_if<SpecArgs, S>(j.sp)});
          });
        });
      });
    });
  });
  HIP_OK(hipGetLastError());
  return RT_OK;
}

// rc: the launch's.  A host entry's results are copied back; the one synchronise also runs after an
// error, so that nothing is in flight on the staging buffer
int reproject_collect(const ReprojectRequest& rq, const ReprojectJob& j, int rc) {
  const size_t n = (size_t)rq.w * rq.h;
  for (int i = 0; rq.host && !rc && i < j.n_planes; ++i)
    if (const TpPlane& p = j.planes[i];
        p.dst && hipMemcpyAsync(p.dst, p.dev, n * 4 * p.floats, hipMemcpyDeviceToHost, j.stream) != hipSuccess)
      rc = set_error(RT_ERR_DEVICE, "%s: copy to host failed", rq.name);
  HIP_OK(hipStreamSynchronize(j.stream));
  return rc;
}

}  // namespace

// host entries: staged through device 0 on the null stream, one at a time
int reproject_impl(const ReprojectRequest& rq) {
  ReprojectJob j{};
  const int device = rq.host ? 0 : rq.device;
  int rc;
  if ((rc = reproject_check(rq, &j)) || (rc = device_ok(rq.name, device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::unique_lock<std::mutex> lk(g_mu, std::defer_lock);
  if (rq.host) lk.lock();
  j.stream = rq.host ? nullptr : (hipStream_t)rq.stream;
  if ((rc = reproject_bind(rq, &j))) return rc;
  return reproject_collect(rq, j, reproject_launch(j));
}

}  // namespace rt

using namespace rt;

// a request's fields: name, host, moments, mode; cam_prev, prev, prev_emit, prev_lum2; cam_cur, cur,
// cur_emit; w, h; opts, mopts, copts, spec; out, out_emit, out_lum2; device, stream
extern "C" {

int rt_reproject_device(const rt_camera* cam_prev, const rt_frame* prev_dev, const rt_camera* cam_cur,
                        const rt_frame* cur_dev, int w, int h, const rt_reproject_opts* opts,
                        const rt_frame* out_dev, int device, void* stream) {
  return reproject_impl({"rt_reproject_device", false, false, RT_REPROJECT_PLAIN, cam_prev, prev_dev, nullptr, nullptr,
                         cam_cur, cur_dev, nullptr, w, h, opts, nullptr, nullptr, nullptr, out_dev, nullptr, nullptr,
                         device, stream});
}

int rt_reproject(const rt_camera* cam_prev, const rt_frame* prev, const rt_camera* cam_cur,
                 const rt_frame* cur, int w, int h, const rt_reproject_opts* opts, const rt_frame* out) {
  return reproject_impl({"rt_reproject", true, false, RT_REPROJECT_PLAIN, cam_prev, prev, nullptr, nullptr, cam_cur, cur,
                         nullptr, w, h, opts, nullptr, nullptr, nullptr, out});
}

int rt_reproject_emit_device(const rt_camera* cam_prev, const rt_frame* prev_dev, const rt_aov_emit* prev_emit_dev,
                             const rt_camera* cam_cur, const rt_frame* cur_dev, const rt_aov_emit* cur_emit_dev,
                             int w, int h, const rt_reproject_opts* opts, const rt_frame* out_dev, int device,
                             void* stream) {
  return reproject_impl({"rt_reproject_emit_device", false, false, RT_REPROJECT_EMIT, cam_prev, prev_dev, prev_emit_dev,
                         nullptr, cam_cur, cur_dev, cur_emit_dev, w, h, opts, nullptr, nullptr, nullptr, out_dev,
                         nullptr, nullptr, device, stream});
}

int rt_reproject_emit(const rt_camera* cam_prev, const rt_frame* prev, const rt_aov_emit* prev_emit,
                      const rt_camera* cam_cur, const rt_frame* cur, const rt_aov_emit* cur_emit, int w, int h,
                      const rt_reproject_opts* opts, const rt_frame* out) {
  return reproject_impl({"rt_reproject_emit", true, false, RT_REPROJECT_EMIT, cam_prev, prev, prev_emit, nullptr,
                         cam_cur, cur, cur_emit, w, h, opts, nullptr, nullptr, nullptr, out});
}

int rt_reproject_light_device(const rt_camera* cam_prev, const rt_frame* prev_dev, const rt_aov_emit* prev_emit_dev,
                              const rt_camera* cam_cur, const rt_frame* cur_dev, const rt_aov_emit* cur_emit_dev,
                              int w, int h, const rt_reproject_opts* opts, const rt_frame* out_dev,
                              const rt_aov_emit* out_emit_dev, int device, void* stream) {
  return reproject_impl({"rt_reproject_light_device", false, false, RT_REPROJECT_LIGHT, cam_prev, prev_dev,
                         prev_emit_dev, nullptr, cam_cur, cur_dev, cur_emit_dev, w, h, opts, nullptr, nullptr, nullptr,
                         out_dev, out_emit_dev, nullptr, device, stream});
}

int rt_reproject_light(const rt_camera* cam_prev, const rt_frame* prev, const rt_aov_emit* prev_emit,
                       const rt_camera* cam_cur, const rt_frame* cur, const rt_aov_emit* cur_emit, int w, int h,
                       const rt_reproject_opts* opts, const rt_frame* out, const rt_aov_emit* out_emit) {
  return reproject_impl({"rt_reproject_light", true, false, RT_REPROJECT_LIGHT, cam_prev, prev, prev_emit, nullptr,
                         cam_cur, cur, cur_emit, w, h, opts, nullptr, nullptr, nullptr, out, out_emit});
}

int rt_reproject_moments_device(int mode, const rt_camera* cam_prev, const rt_frame* prev_dev,
                                const rt_aov_emit* prev_emit_dev, const float* prev_lum2_dev,
                                const rt_camera* cam_cur, const rt_frame* cur_dev, const rt_aov_emit* cur_emit_dev,
                                int w, int h, const rt_reproject_opts* opts, const rt_moments_opts* mopts,
                                const rt_frame* out_dev, const rt_aov_emit* out_emit_dev, float* out_lum2_dev,
                                int device, void* stream) {
  return reproject_impl({"rt_reproject_moments_device", false, true, mode, cam_prev, prev_dev, prev_emit_dev,
                         prev_lum2_dev, cam_cur, cur_dev, cur_emit_dev, w, h, opts, mopts, nullptr, nullptr, out_dev,
                         out_emit_dev, out_lum2_dev, device, stream});
}

int rt_reproject_moments(int mode, const rt_camera* cam_prev, const rt_frame* prev, const rt_aov_emit* prev_emit,
                         const float* prev_lum2, const rt_camera* cam_cur, const rt_frame* cur,
                         const rt_aov_emit* cur_emit, int w, int h, const rt_reproject_opts* opts,
                         const rt_moments_opts* mopts, const rt_frame* out, const rt_aov_emit* out_emit,
                         float* out_lum2) {
  return reproject_impl({"rt_reproject_moments", true, true, mode, cam_prev, prev, prev_emit, prev_lum2, cam_cur, cur,
                         cur_emit, w, h, opts, mopts, nullptr, nullptr, out, out_emit, out_lum2});
}

int rt_reproject_clip_device(int mode, const rt_camera* cam_prev, const rt_frame* prev_dev,
                             const rt_aov_emit* prev_emit_dev, const float* prev_lum2_dev, const rt_camera* cam_cur,
                             const rt_frame* cur_dev, const rt_aov_emit* cur_emit_dev, int w, int h,
                             const rt_reproject_opts* opts, const rt_moments_opts* mopts, const rt_clip_opts* copts,
                             const rt_frame* out_dev, const rt_aov_emit* out_emit_dev, float* out_lum2_dev,
                             int device, void* stream) {
  return reproject_impl({"rt_reproject_clip_device", false, true, mode, cam_prev, prev_dev, prev_emit_dev,
                         prev_lum2_dev, cam_cur, cur_dev, cur_emit_dev, w, h, opts, mopts, copts, nullptr, out_dev,
                         out_emit_dev, out_lum2_dev, device, stream});
}

int rt_reproject_clip(int mode, const rt_camera* cam_prev, const rt_frame* prev, const rt_aov_emit* prev_emit,
                      const float* prev_lum2, const rt_camera* cam_cur, const rt_frame* cur,
                      const rt_aov_emit* cur_emit, int w, int h, const rt_reproject_opts* opts,
                      const rt_moments_opts* mopts, const rt_clip_opts* copts, const rt_frame* out,
                      const rt_aov_emit* out_emit, float* out_lum2) {
  return reproject_impl({"rt_reproject_clip", true, true, mode, cam_prev, prev, prev_emit, prev_lum2, cam_cur, cur,
                         cur_emit, w, h, opts, mopts, copts, nullptr, out, out_emit, out_lum2});
}

int rt_reproject_spec_device(int mode, const rt_camera* cam_prev, const rt_frame* prev_dev,
                             const rt_aov_emit* prev_emit_dev, const float* prev_lum2_dev, const rt_camera* cam_cur,
                             const rt_frame* cur_dev, const rt_aov_emit* cur_emit_dev, int w, int h,
                             const rt_reproject_opts* opts, const rt_moments_opts* mopts, const rt_clip_opts* copts,
                             const rt_spec_planes* spec_dev, const rt_frame* out_dev, const rt_aov_emit* out_emit_dev,
                             float* out_lum2_dev, int device, void* stream) {
  return reproject_impl({"rt_reproject_spec_device", false, true, mode, cam_prev, prev_dev, prev_emit_dev,
                         prev_lum2_dev, cam_cur, cur_dev, cur_emit_dev, w, h, opts, mopts, copts, spec_dev, out_dev,
                         out_emit_dev, out_lum2_dev, device, stream});
}

int rt_reproject_spec(int mode, const rt_camera* cam_prev, const rt_frame* prev, const rt_aov_emit* prev_emit,
                      const float* prev_lum2, const rt_camera* cam_cur, const rt_frame* cur,
                      const rt_aov_emit* cur_emit, int w, int h, const rt_reproject_opts* opts,
                      const rt_moments_opts* mopts, const rt_clip_opts* copts, const rt_spec_planes* spec,
                      const rt_frame* out, const rt_aov_emit* out_emit, float* out_lum2) {
  return reproject_impl({"rt_reproject_spec", true, true, mode, cam_prev, prev, prev_emit, prev_lum2, cam_cur, cur,
                         cur_emit, w, h, opts, mopts, copts, spec, out, out_emit, out_lum2});
}

}  // extern "C"
