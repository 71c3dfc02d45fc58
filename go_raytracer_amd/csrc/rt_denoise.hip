// rt_denoise.hip — edge-avoiding a-trous wavelet denoiser (Dammertz, Sewtz, Hanika, Lensch,
// "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG
// 2010), guided by the feature buffers of rt_aov.hip.  A filter stage beside the output
// kernels (rt_output.hip): a low-spp image goes render -> denoise -> quantize -> PPM in HBM.
//
// Two modes share every kernel below; a mode is a policy struct (Plain, Var) that supplies
// what differs, and each kernel is written once as a template over it:
//
//   Plain (rt_denoise)    : records colour {c.rgb, depth} (ping-pong) and guide {n.xyz, valid}
//                           (read-only); the colour term of the weight is |dc|^2 / sc_i^2,
//                           sc_i = sigma_color 2^-i
//   Var (rt_denoise_var)  : the edge-stopping function of Schied et al., "Spatiotemporal
//                           Variance-Guided Filtering", HPG 2017.  Records {c.rgb, v} and
//                           {n.xyz, depth}; v is the variance of the luminance of c, >= 0, and
//                           v = -1 marks an invalid pixel, so validity travels with the record
//                           that every tap reads anyway and depth keeps its own bits.  The colour
//                           term is |Y(c_p) - Y(c_q)| / (sigma_lum sqrt(g(p)) + 1e-6), g the 3 x 3
//                           (offsets of 1 whatever the step) [1/4, 1/2, 1/4]^2 prefilter of v
//                           over valid pixels; v' = sum w^2 v_q / (sum w)^2
//
//   k_dn_prep<VAR, EMIT> : writes the two records of a pixel; c = rgb / max(albedo, 1e-3) when
//                          demodulating (v / Y(albedo)^2); a pixel with a non-finite input gets
//                          c = 0 and is marked invalid (so a zero weight times its colour is 0,
//                          not NaN).  EMIT (the split entries): c = (rgb - emission) /
//                          max(surface_albedo, 1e-3), and a pixel is also invalid when its
//                          emission is not finite or its coverage is not below 1
//   k_dn_atrous<Mode, TILE, FINAL>
//                        : iteration i, step 2^i: 25 taps (dx, dy) in {-2..2}^2 * step, B3 kernel
//                          h (x) h, weight h_x h_y exp(-(colour term + |dn|^2 / sn^2 + dd^2 /
//                          (sd max(d_p, 1e-6))^2)) * valid_q * inside, renormalised.  Steps 1 and
//                          2 (TILE) stage the tile and its halo in LDS (one wave = one 64-pixel
//                          row segment, so every tap is 64 consecutive 16-B records:
//                          conflict-free ds_read_b128); for larger steps the halo exceeds the
//                          tile and the taps are read through L1/L2, each one a coalesced row
//                          segment.  The tap loop is branch-free: coordinates clamped, the
//                          weight zeroed by a multiply.  The last iteration (FINAL) multiplies
//                          the albedo back and writes `out` (and `var_out`); invalid pixels are
//                          copied through from rgb (var)
//   k_dn_emit_add        : the split entries' epilogue, out += emission on the valid pixels.  It
//                          takes the validity from the records, not from rgb, which an aliased
//                          out has overwritten
//
// Bytes per pixel: prep 40 to 60 read and 32 written; an iteration 50 x 16 read (L1/L2-resident
// stencil; Var 9 x 16 (tiled) or 9 x 4 (global) more) and 16 written; epilogue 28 read, 12 written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "rt_hip_util.h"

namespace rt {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4f lds_v4;
typedef __attribute__((address_space(1))) v4f glb_v4;

constexpr int kTW = 64, kTH = 4;       // tile: one wave per row of 64 pixels
constexpr int kMaxHalo = 4;            // 2 * step for the LDS steps 1 and 2
constexpr int kLW = kTW + 2 * kMaxHalo, kLH = kTH + 2 * kMaxHalo;  // 72 x 12 records
constexpr float kMaxInv = 1e30f;       // 1 / sigma^2 clamp: sigma -> 0+ keeps 0 * inv = 0
constexpr float kLumEps = 1e-6f;

struct DnParams {
  int w, h;
  float sc;      // Plain: 1 / sigma_color_i^2; Var: sigma_lum (the variance shrinks by itself)
  float inv_n;   // 1 / sigma_normal^2, 0 = off
  float sd;      // sigma_depth, 0 = depth weight off
  int step;
  int demod;
};

// The input planes, null = absent, in the order the host entries stage them: plane k starts at
// float kOff[k] * n of the staging buffer.  kAlbedo is the surface albedo in the split mode.
enum { kRgb, kAlbedo, kNormal, kDepth, kVar, kEmission, kCoverage, kPlanes };
constexpr int kOff[kPlanes + 1] = {0, 3, 6, 9, 10, 11, 14, 15};
struct Planes {
  const float* p[kPlanes];
};

__device__ __forceinline__ float lum(float r, float g, float b) {
  return 0.2126f * r + 0.7152f * g + 0.0722f * b;  // the accumulator's weights
}

float inv_sq(double sigma) {
  const double v = 1.0 / (sigma * sigma);
  return (float)std::min(v, (double)kMaxInv);
}

// Img: the images of the FINAL write, each mode's own (pointer types and all)
template <class Mode, bool TILE, bool FINAL, class... Img>
__global__ void k_dn_atrous(DnParams P, const v4f* __restrict__ cin, const v4f* __restrict__ gd,
                            v4f* __restrict__ cout, Img... img);

// ---- the modes: what differs between rt_denoise and rt_denoise_var ----------------------------

struct Plain {
  static constexpr bool kHasVar = false;
  static constexpr const char* kWho = "rt_denoise";
  static constexpr float kSigma = 0.5f;    // sigma_color's default
  static float sigma(float sc, int i) { return inv_sq((double)sc * ldexp(1.0, -i)); }  // DnParams::sc
  template <bool TILE, bool FINAL>
  static void launch(dim3 grid, hipStream_t s, const DnParams& p, const v4f* cin, const v4f* gd, v4f* cout,
                     const Planes& in, float* out, float*) {
    hipLaunchKernelGGL((k_dn_atrous<Plain, TILE, FINAL, const float*, const float* __restrict__, float*>), grid,
                       dim3(256), 0, s, p, cin, gd, cout, in.p[kRgb], in.p[kAlbedo], out);
  }

  struct Px {};  // per-pixel setup: none
  static constexpr float kOutsideW = 0.0f;  // a colour record outside the image (the guide's valid = 0)
  static __device__ bool valid(v4f, v4f g) { return g.w != 0.0f; }
  static __device__ float tap_valid(v4f, v4f g) { return g.w; }  // 0 or 1
  static __device__ float depth(v4f c, v4f) { return c.w; }
  template <class WAt>
  static __device__ Px setup(const DnParams&, v4f, WAt) {
    return {};
  }
  struct Diff {
    float r, g, b;
  };
  static __device__ Diff diff(const Px&, v4f cp, v4f cq) { return {cp.x - cq.x, cp.y - cq.y, cp.z - cq.z}; }
  static __device__ float colour(const Px&, const DnParams& P, Diff d) {
    return (d.r * d.r + d.g * d.g + d.b * d.b) * P.sc;
  }
  static __device__ float moment(float, v4f) { return 0.0f; }
  static __device__ float carry(bool, float, float, v4f cp) { return cp.w; }  // depth
  static __device__ void write(int demod, size_t pi, bool valid, float r, float g, float b, float,
                               const float* rgb,  // may alias out
                               const float* __restrict__ albedo, float* out) {
    float o0, o1, o2;
    if (valid) {
      o0 = r, o1 = g, o2 = b;
      if (demod) {
        o0 *= fmaxf(albedo[3 * pi], 1e-3f);
        o1 *= fmaxf(albedo[3 * pi + 1], 1e-3f);
        o2 *= fmaxf(albedo[3 * pi + 2], 1e-3f);
      }
    } else {  // a non-finite pixel passes through (read before the write: out may alias rgb)
      o0 = rgb[3 * pi], o1 = rgb[3 * pi + 1], o2 = rgb[3 * pi + 2];
    }
    out[3 * pi] = o0;
    out[3 * pi + 1] = o1;
    out[3 * pi + 2] = o2;
  }
};

struct Var {
  static constexpr bool kHasVar = true;
  static constexpr const char* kWho = "rt_denoise_var";
  static constexpr float kSigma = 1.0f;    // sigma_lum's default (the sweep)
  static float sigma(float sl, int) { return sl; }  // not shrunk per iteration
  template <bool TILE, bool FINAL>
  static void launch(dim3 grid, hipStream_t s, const DnParams& p, const v4f* cin, const v4f* gd, v4f* cout,
                     const Planes& in, float* out, float* var_out) {
    hipLaunchKernelGGL((k_dn_atrous<Var, TILE, FINAL, const float*, const float*, const float* __restrict__,
                                    float*, float*>),
                       grid, dim3(256), 0, s, p, cin, gd, cout, in.p[kRgb], in.p[kVar], in.p[kAlbedo], out,
                       var_out);
  }

  struct Px {
    float inv_l, yp;
  };
  static constexpr float kOutsideW = -1.0f;  // a colour record outside the image: v = -1, not valid
  static __device__ bool valid(v4f c, v4f) { return c.w >= 0.0f; }
  static __device__ float tap_valid(v4f c, v4f) { return c.w >= 0.0f ? 1.0f : 0.0f; }
  static __device__ float depth(v4f, v4f g) { return g.w; }
  // the 3 x 3 prefilter of the variance at p, over the adjacent pixels whatever the step
  template <class WAt>
  static __device__ Px setup(const DnParams& P, v4f cp, WAt w_at) {
    const float k3[2] = {0.5f, 0.25f};
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        float inside = 1.0f;
        const float vq = w_at(dx, dy, inside);
        const float k = k3[dx < 0 ? -dx : dx] * k3[dy < 0 ? -dy : dy] * (vq >= 0.0f ? 1.0f : 0.0f) * inside;
        gs += k * fmaxf(vq, 0.0f);
        gw += k;
      }
    }
    const float gvar = gw > 0.0f ? gs / gw : 0.0f;
    return {1.0f / (P.sc * sqrtf(gvar) + kLumEps), lum(cp.x, cp.y, cp.z)};
  }
  typedef float Diff;
  static __device__ Diff diff(const Px& px, v4f, v4f cq) { return fabsf(px.yp - lum(cq.x, cq.y, cq.z)); }
  static __device__ float colour(const Px& px, const DnParams&, Diff dl) { return dl * px.inv_l; }
  static __device__ float moment(float wgt, v4f cq) { return wgt * wgt * fmaxf(cq.w, 0.0f); }
  static __device__ float carry(bool valid, float sv, float inv, v4f cp) {
    return valid ? sv * (inv * inv) : cp.w;
  }
  static __device__ void write(int demod, size_t pi, bool valid, float r, float g, float b, float v,
                               const float* rgb,  // may alias out
                               const float* var,  // may alias var_out
                               const float* __restrict__ albedo, float* out, float* var_out) {
    float o0, o1, o2, ov;
    if (valid) {
      o0 = r, o1 = g, o2 = b, ov = v;
      if (demod) {
        const float a0 = fmaxf(albedo[3 * pi], 1e-3f), a1 = fmaxf(albedo[3 * pi + 1], 1e-3f),
                    a2 = fmaxf(albedo[3 * pi + 2], 1e-3f);
        const float ya = lum(a0, a1, a2);
        o0 *= a0;
        o1 *= a1;
        o2 *= a2;
        ov *= ya * ya;
      }
    } else {  // passes through (read before the write: out may alias rgb, var_out var)
      o0 = rgb[3 * pi], o1 = rgb[3 * pi + 1], o2 = rgb[3 * pi + 2], ov = var[pi];
    }
    out[3 * pi] = o0;
    out[3 * pi + 1] = o1;
    out[3 * pi + 2] = o2;
    if (var_out) var_out[pi] = ov;
  }
};

// ---- kernels ----------------------------------------------------------------------------------

// VAR: the records of Var, from in.p[kVar] too; EMIT: the split inputs (header comment).  One
// lane per pixel, coalesced.
template <bool VAR, bool EMIT>
__global__ __launch_bounds__(256) void k_dn_prep(Planes in, int64_t n, int demod, v4f* __restrict__ col,
                                                 v4f* __restrict__ gd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ rgb = in.p[kRgb];
  const float* __restrict__ albedo = in.p[kAlbedo];
  const float* __restrict__ normal = in.p[kNormal];
  const float* __restrict__ depth = in.p[kDepth];
  float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2], v = 0.0f;
  if constexpr (VAR) v = in.p[kVar][i];
  bool valid = isfinite(r) && isfinite(g) && isfinite(b);
  if constexpr (VAR) valid = valid && isfinite(v);
  if constexpr (EMIT) {
    const float* __restrict__ emission = in.p[kEmission];
    const float e0 = emission[3 * i], e1 = emission[3 * i + 1], e2 = emission[3 * i + 2];
    valid = valid && isfinite(e0) && isfinite(e1) && isfinite(e2) && in.p[kCoverage][i] < 1.0f;
    r -= e0;
    g -= e1;
    b -= e2;
  }
  if (demod) {
    const float a0 = fmaxf(albedo[3 * i], 1e-3f), a1 = fmaxf(albedo[3 * i + 1], 1e-3f),
                a2 = fmaxf(albedo[3 * i + 2], 1e-3f);
    const float ya = VAR ? lum(a0, a1, a2) : 1.0f;
    r = r / a0;
    g = g / a1;
    b = b / a2;
    if constexpr (VAR) v = v / (ya * ya);
  }
  v = fmaxf(v, 0.0f);
  if (!valid) r = g = b = 0.0f, v = -1.0f;
  const float d = depth ? depth[i] : 0.0f;
  v4f nv = {0.0f, 0.0f, 0.0f, VAR ? d : valid ? 1.0f : 0.0f};
  if (normal) nv.x = normal[3 * i], nv.y = normal[3 * i + 1], nv.z = normal[3 * i + 2];
  *(glb_v4*)(col + i) = v4f{r, g, b, VAR ? v : d};
  *(glb_v4*)(gd + i) = nv;
}

// TILE: taps from the LDS tile (step <= 2); FINAL: the last iteration writes the mode's images
template <class Mode, bool TILE, bool FINAL, class... Img>
__global__ __launch_bounds__(256) void k_dn_atrous(DnParams P, const v4f* __restrict__ cin,
                                                   const v4f* __restrict__ gd,
                                                   v4f* __restrict__ cout, Img... img) {
  __shared__ v4f lcol[TILE ? kLW * kLH : 1];
  __shared__ v4f lgd[TILE ? kLW * kLH : 1];
  const int tx = threadIdx.x & (kTW - 1), ty = threadIdx.x >> 6;
  const int x = blockIdx.x * kTW + tx, y = blockIdx.y * kTH + ty;
  const int step = P.step;
  const int halo = 2 * step;       // <= kMaxHalo when TILE
  const int lw = kTW + 2 * halo;   // LDS row length of this launch
  if constexpr (TILE) {
    const int lh = kTH + 2 * halo;
    const int x0 = blockIdx.x * kTW - halo, y0 = blockIdx.y * kTH - halo;
    for (int i = threadIdx.x; i < lw * lh; i += 256) {
      const int ly = i / lw, lx = i - ly * lw;
      const int gx = x0 + lx, gy = y0 + ly;
      const bool in = gx >= 0 && gx < P.w && gy >= 0 && gy < P.h;
      v4f c = {0.0f, 0.0f, 0.0f, Mode::kOutsideW}, g = {0.0f, 0.0f, 0.0f, 0.0f};
      if (in) {
        const size_t q = (size_t)gy * P.w + gx;
        c = *(const glb_v4*)(cin + q);
        g = *(const glb_v4*)(gd + q);
      }
      *(lds_v4*)&lcol[i] = c;
      *(lds_v4*)&lgd[i] = g;
    }
    __syncthreads();
  }
  if (x >= P.w || y >= P.h) return;
  const size_t pi = (size_t)y * P.w + x;
  v4f cp, gp;
  if constexpr (TILE) {
    const int li = (ty + halo) * lw + tx + halo;
    cp = *(const lds_v4*)&lcol[li];
    gp = *(const lds_v4*)&lgd[li];
  } else {
    cp = *(const glb_v4*)(cin + pi);
    gp = *(const glb_v4*)(gd + pi);
  }
  // the w of the colour record of the adjacent pixel (x + ox, y + oy), for Var's prefilter
  auto w_at = [&](int ox, int oy, float& inside) -> float {
    if constexpr (TILE) {  // the whole record: 64 consecutive 16-B reads, conflict-free
      const v4f cq = *(const lds_v4*)&lcol[(ty + halo + oy) * lw + tx + halo + ox];
      return cq.w;
    } else {
      const int qx = x + ox, qy = y + oy;
      const int cx = min(max(qx, 0), P.w - 1), cy = min(max(qy, 0), P.h - 1);
      inside = (cx == qx && cy == qy) ? 1.0f : 0.0f;
      return ((const float*)(cin + ((size_t)cy * P.w + cx)))[3];
    }
  };
  const typename Mode::Px px = Mode::setup(P, cp, w_at);
  const float sdp = P.sd * fmaxf(Mode::depth(cp, gp), 1e-6f);
  const float inv_d = P.sd > 0.0f ? fminf(1.0f / (sdp * sdp), kMaxInv) : 0.0f;
  const float hk[3] = {0.375f, 0.25f, 0.0625f};
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      v4f cq, gq;
      float inside = 1.0f;
      if constexpr (TILE) {
        const int li = (ty + halo + dy * step) * lw + tx + halo + dx * step;
        cq = *(const lds_v4*)&lcol[li];
        gq = *(const lds_v4*)&lgd[li];
      } else {
        const int qx = x + dx * step, qy = y + dy * step;
        const int cx = min(max(qx, 0), P.w - 1), cy = min(max(qy, 0), P.h - 1);
        inside = (cx == qx && cy == qy) ? 1.0f : 0.0f;
        const size_t q = (size_t)cy * P.w + cx;
        cq = *(const glb_v4*)(cin + q);
        gq = *(const glb_v4*)(gd + q);
      }
      const typename Mode::Diff dc = Mode::diff(px, cp, cq);
      const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
      const float dd = Mode::depth(cp, gp) - Mode::depth(cq, gq);
      const float arg = Mode::colour(px, P, dc) + (nx * nx + ny * ny + nz * nz) * P.inv_n + dd * dd * inv_d;
      const float wgt = hk[dx < 0 ? -dx : dx] * hk[dy < 0 ? -dy : dy] * __expf(-arg) *
                        Mode::tap_valid(cq, gq) * inside;
      sw += wgt;
      sr += wgt * cq.x;
      sg += wgt * cq.y;
      sb += wgt * cq.z;
      sv += Mode::moment(wgt, cq);
    }
  }
  const bool valid = Mode::valid(cp, gp);
  const float inv = 1.0f / sw;
  const float r = valid ? sr * inv : cp.x, g = valid ? sg * inv : cp.y, b = valid ? sb * inv : cp.z;
  const float v = Mode::carry(valid, sv, inv, cp);
  if constexpr (FINAL) {
    Mode::write(P.demod, pi, valid, r, g, b, v, img...);
  } else {
    *(glb_v4*)(cout + pi) = v4f{r, g, b, v};
  }
}

// out += emission on the valid pixels.  rec: the guide records (valid: w != 0) or, with var_mode,
// the colour records the last iteration read (valid: w >= 0).
__global__ __launch_bounds__(256) void k_dn_emit_add(const v4f* __restrict__ rec, int var_mode,
                                                     const float* __restrict__ emission, int64_t n,
                                                     float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float w = ((const float*)(rec + i))[3];
  if (var_mode ? !(w >= 0.0f) : w == 0.0f) return;
  out[3 * i] += emission[3 * i];
  out[3 * i + 1] += emission[3 * i + 1];
  out[3 * i + 2] += emission[3 * i + 2];
}

// ---- host -------------------------------------------------------------------------------------

std::mutex g_mu;                 // one denoise at a time: the scratch buffers are shared
DeviceScratch g_work, g_stage;   // records (48 B per pixel); the host entries' staged planes

struct Resolved {
  int iterations;
  int demod;
  float sc, sn, sd;
};

// argument checks of every entry point (before any device is touched).  o: sigma_lum travels in
// sigma_color; split: the emit buffers are required and replace feat->albedo
template <class Mode>
int resolve(const char* who, const float* rgb, const float* var, const rt_aov* feat, bool split,
            const rt_aov_emit* emit, int w, int h, const rt_denoise_opts& o, const float* out,
            Resolved* r) {
  if (w <= 0 || h <= 0) return set_error(RT_ERR_INVALID, "%s: %d x %d image", who, w, h);
  if ((int64_t)w * h >= ((int64_t)1 << 31) / 3)
    return set_error(RT_ERR_INVALID, "%s: %d x %d image", who, w, h);
  if ((h + kTH - 1) / kTH > 65535)  // one block row per kTH image rows: the grid's y limit
    return set_error(RT_ERR_INVALID, "%s: height %d above %d", who, h, 65535 * kTH);
  if (!rgb || !out) return set_error(RT_ERR_INVALID, "%s: null image", who);
  if (o.iterations < 0 || o.iterations > 8)
    return set_error(RT_ERR_INVALID, "%s: %d iterations (1..8)", who, o.iterations);
  if (split) {
    if (!emit || !emit->emission || !emit->surface_albedo || !emit->coverage)
      return set_error(RT_ERR_INVALID, "%s: needs the emission, surface_albedo and coverage buffers", who);
  } else if (o.demodulate && (!feat || !feat->albedo)) {
    return set_error(RT_ERR_INVALID, "%s: demodulate needs the albedo buffer", who);
  }
  if (!(o.sigma_color >= 0.0f) || !(o.sigma_normal >= 0.0f) || !(o.sigma_depth >= 0.0f))
    return set_error(RT_ERR_INVALID, "%s: negative or NaN sigma", who);
  if (Mode::kHasVar && !var) return set_error(RT_ERR_INVALID, "%s: null variance", who);
  r->iterations = o.iterations == 0 ? 5 : o.iterations;
  r->demod = o.demodulate ? 1 : 0;
  r->sc = o.sigma_color > 0.0f ? o.sigma_color : Mode::kSigma;
  r->sn = o.sigma_normal > 0.0f ? o.sigma_normal : 0.3f;
  r->sd = o.sigma_depth > 0.0f ? o.sigma_depth : 0.02f;
  return RT_OK;
}

// the filter; every plane of `in`, out and var_out (Var only; may be null) on the current device;
// g_mu held
template <class Mode>
int run(const Planes& in, bool split, int w, int h, const Resolved& r, float* out, float* var_out,
        int device, hipStream_t s) {
  const int64_t n = (int64_t)w * h;
  void* wk = nullptr;
  int rc = g_work.get(device, (size_t)n * 48, &wk, Mode::kWho);
  if (rc) return rc;
  v4f* gd = (v4f*)wk;
  v4f* col[2] = {gd + n, gd + 2 * n};
  const dim3 lin((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL((split ? k_dn_prep<Mode::kHasVar, true> : k_dn_prep<Mode::kHasVar, false>), lin, dim3(256), 0, s,
                     in, n, r.demod, col[0], gd);
  HIP_OK(hipGetLastError());
  const dim3 grid((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kTH - 1) / kTH));
  decltype(&Mode::template launch<false, false>) const launch[2][2] = {  // [TILE][FINAL]
      {Mode::template launch<false, false>, Mode::template launch<false, true>},
      {Mode::template launch<true, false>, Mode::template launch<true, true>}};
  for (int i = 0; i < r.iterations; ++i) {
    DnParams p;
    p.w = w;
    p.h = h;
    p.sc = Mode::sigma(r.sc, i);
    p.inv_n = in.p[kNormal] ? inv_sq(r.sn) : 0.0f;
    p.sd = in.p[kDepth] ? r.sd : 0.0f;
    p.step = 1 << i;
    p.demod = r.demod;
    const bool tile = 2 * p.step <= kMaxHalo, fin = i == r.iterations - 1;
    launch[tile][fin](grid, s, p, col[i & 1], gd, col[(i & 1) ^ 1], in, out, var_out);
    HIP_OK(hipGetLastError());
  }
  if (split) {  // validity from the records: the guide's w, or the v the last iteration read
    hipLaunchKernelGGL(k_dn_emit_add, lin, dim3(256), 0, s, Mode::kHasVar ? col[(r.iterations - 1) & 1] : gd,
                       (int)Mode::kHasVar, in.p[kEmission], n, out);
    HIP_OK(hipGetLastError());
  }
  return RT_OK;
}

// The body of every entry point.  host: the pointers are host memory, staged through `device`
// (rgb and var in place: they are also the outputs); else they are on `device` already.
template <class Mode>
int denoise(const char* who, bool host, const float* rgb, const float* var, const rt_aov* feat, bool split,
            const rt_aov_emit* emit, int w, int h, const rt_denoise_opts& o, float* out, float* var_out,
            int device, void* stream) {
  Resolved r;
  int rc = resolve<Mode>(who, rgb, var, feat, split, emit, w, h, o, out, &r);
  if (rc) return rc;
  if ((rc = device_ok(who, device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  hipStream_t s = (hipStream_t)stream;
  Planes in{};
  in.p[kRgb] = rgb;
  in.p[kAlbedo] = split ? emit->surface_albedo : feat ? feat->albedo : nullptr;
  in.p[kNormal] = feat ? feat->normal : nullptr;
  in.p[kDepth] = feat ? feat->depth : nullptr;
  in.p[kVar] = Mode::kHasVar ? var : nullptr;
  in.p[kEmission] = split ? emit->emission : nullptr;
  in.p[kCoverage] = split ? emit->coverage : nullptr;
  if (!Mode::kHasVar) var_out = nullptr;
  float *d_out = out, *d_var_out = var_out;
  const size_t n = (size_t)w * h;
  if (host) {  // n * 40, 44 or 60 bytes: the planes up to the last one the mode can have
    const int last = split ? kCoverage : Mode::kHasVar ? kVar : kDepth;
    void* stg = nullptr;
    if ((rc = g_stage.get(device, n * 4 * kOff[last + 1], &stg, who))) return rc;
    for (int k = 0; k <= last; ++k) {
      if (!in.p[k]) continue;
      float* d = (float*)stg + kOff[k] * n;
      HIP_OK(hipMemcpyAsync(d, in.p[k], n * 4 * (kOff[k + 1] - kOff[k]), hipMemcpyHostToDevice, s));
      in.p[k] = d;
    }
    d_out = (float*)stg;
    if (var_out) d_var_out = (float*)stg + kOff[kVar] * n;
  }
  rc = run<Mode>(in, split, w, h, r, d_out, d_var_out, device, s);
  if (host && !rc &&
      (hipMemcpyAsync(out, d_out, n * 12, hipMemcpyDeviceToHost, s) != hipSuccess ||
       (var_out && hipMemcpyAsync(var_out, d_var_out, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = set_error(RT_ERR_DEVICE, "%s: copy to host failed", who);
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  return rc;
}

rt_denoise_opts opts_of(const rt_denoise_opts* o) { return o ? *o : rt_denoise_opts{}; }

rt_denoise_opts opts_of(const rt_denoise_var_opts* o) {  // sigma_lum in sigma_color's place
  rt_denoise_opts r{};
  if (o) {
    r.iterations = o->iterations;
    r.demodulate = o->demodulate;
    r.sigma_color = o->sigma_lum;
    r.sigma_normal = o->sigma_normal;
    r.sigma_depth = o->sigma_depth;
  }
  return r;
}

}  // namespace
}  // namespace rt

using namespace rt;

extern "C" {

int rt_denoise(const float* rgb, const rt_aov* feat, int w, int h, const rt_denoise_opts* opts,
               float* out) {
  return denoise<Plain>("rt_denoise", true, rgb, nullptr, feat, false, nullptr, w, h, opts_of(opts), out,
                        nullptr, 0, nullptr);
}

int rt_denoise_device(const float* rgb_dev, const rt_aov* feat_dev, int w, int h,
                      const rt_denoise_opts* opts, float* out_dev, int device, void* stream) {
  return denoise<Plain>("rt_denoise_device", false, rgb_dev, nullptr, feat_dev, false, nullptr, w, h,
                        opts_of(opts), out_dev, nullptr, device, stream);
}

int rt_denoise_var(const float* rgb, const float* var, const rt_aov* feat, int w, int h,
                   const rt_denoise_var_opts* opts, float* out, float* var_out) {
  return denoise<Var>("rt_denoise_var", true, rgb, var, feat, false, nullptr, w, h, opts_of(opts), out,
                      var_out, 0, nullptr);
}

int rt_denoise_var_device(const float* rgb_dev, const float* var_dev, const rt_aov* feat_dev, int w,
                          int h, const rt_denoise_var_opts* opts, float* out_dev, float* var_out_dev,
                          int device, void* stream) {
  return denoise<Var>("rt_denoise_var_device", false, rgb_dev, var_dev, feat_dev, false, nullptr, w, h,
                      opts_of(opts), out_dev, var_out_dev, device, stream);
}

// the emission split: the entries above with an rt_aov_emit after feat

int rt_denoise_emit(const float* rgb, const rt_aov* feat, const rt_aov_emit* emit, int w, int h,
                    const rt_denoise_opts* opts, float* out) {
  return denoise<Plain>("rt_denoise_emit", true, rgb, nullptr, feat, true, emit, w, h, opts_of(opts), out,
                        nullptr, 0, nullptr);
}

int rt_denoise_emit_device(const float* rgb_dev, const rt_aov* feat_dev, const rt_aov_emit* emit_dev,
                           int w, int h, const rt_denoise_opts* opts, float* out_dev, int device,
                           void* stream) {
  return denoise<Plain>("rt_denoise_emit_device", false, rgb_dev, nullptr, feat_dev, true, emit_dev, w, h,
                        opts_of(opts), out_dev, nullptr, device, stream);
}

int rt_denoise_var_emit(const float* rgb, const float* var, const rt_aov* feat, const rt_aov_emit* emit,
                        int w, int h, const rt_denoise_var_opts* opts, float* out, float* var_out) {
  return denoise<Var>("rt_denoise_var_emit", true, rgb, var, feat, true, emit, w, h, opts_of(opts), out,
                      var_out, 0, nullptr);
}

int rt_denoise_var_emit_device(const float* rgb_dev, const float* var_dev, const rt_aov* feat_dev,
                               const rt_aov_emit* emit_dev, int w, int h,
                               const rt_denoise_var_opts* opts, float* out_dev, float* var_out_dev,
                               int device, void* stream) {
  return denoise<Var>("rt_denoise_var_emit_device", false, rgb_dev, var_dev, feat_dev, true, emit_dev, w, h,
                      opts_of(opts), out_dev, var_out_dev, device, stream);
}

}  // extern "C"
