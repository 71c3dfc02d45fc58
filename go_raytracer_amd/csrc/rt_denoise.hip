// rt_denoise.hip — edge-avoiding a-trous wavelet denoiser (Dammertz, Sewtz, Hanika, Lensch,
// "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG
// 2010), guided by the feature buffers of rt_aov.hip.  A filter stage beside the output
// kernels (rt_output.hip): a low-spp image goes render -> denoise -> quantize -> PPM in HBM.
//
//   k_dn_prep  : per pixel two 16-B records, colour {c.rgb, depth} and guide {n.xyz, valid};
//                c = rgb / max(albedo, 1e-3) when demodulating; a pixel with a non-finite
//                colour channel gets valid = 0 and c = 0 (so a zero weight times its colour
//                is 0, not NaN)
//   k_dn_atrous: iteration i, step 2^i: 25 taps (dx, dy) in {-2..2}^2 * step, B3 kernel
//                h (x) h, weight h_x h_y exp(-(|dc|^2 / sc_i^2 + |dn|^2 / sn^2 + dd^2 /
//                (sd max(d_p, 1e-6))^2)) * valid_q * inside, renormalised; the colour
//                records ping-pong, the guide records are read-only.  Steps 1 and 2 stage the
//                tile and its halo in LDS (one wave = one 64-pixel row segment, so every tap
//                is 64 consecutive 16-B records: conflict-free ds_read_b128); for larger steps
//                the halo exceeds the tile and the taps are read through L1/L2, each one a
//                coalesced row segment.  The tap loop is branch-free: coordinates clamped,
//                the weight zeroed by a multiply.  The last iteration multiplies the albedo
//                back and writes `out`; pixels with valid = 0 are copied through from rgb.
//
// Bytes per pixel and iteration: 50 x 16 read (L1/L2-resident stencil) + 16 written.
//
// The variance-guided mode (rt_denoise_var, the edge-stopping function of Schied et al.,
// "Spatiotemporal Variance-Guided Filtering", HPG 2017) has kernels of its own beside these,
// so the code generation of the ones above does not move:
//
//   k_dnv_prep  : records {c.rgb, v} (ping-pong) and {n.xyz, depth} (read-only); v is the
//                 variance of the luminance of c, >= 0; v = -1 marks a pixel whose colour or
//                 variance is not finite (c = 0), so validity travels with the record that
//                 every tap reads anyway and depth keeps its own bits
//   k_dnv_atrous: the same tile, halo, tap loop and clamping; the colour term of the weight is
//                 |Y(c_p) - Y(c_q)| / (sigma_lum sqrt(g(p)) + 1e-6), g the 3 x 3 (offsets of 1,
//                 inside the halo of the tiled steps; nine clamped loads for the others)
//                 [1/4, 1/2, 1/4]^2 prefilter of v over valid pixels; v' = sum w^2 v_q / (sum w)^2
//
// Bytes per pixel and iteration: 50 x 16 + 9 x 16 (tiled) or 9 x 4 (global) read, 16 written.
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

struct DnParams {
  int w, h;
  float inv_c;   // 1 / sigma_color_i^2
  float inv_n;   // 1 / sigma_normal^2, 0 = off
  float sd;      // sigma_depth, 0 = depth weight off
  int step;
  int demod;
};

__global__ __launch_bounds__(256) void k_dn_prep(const float* __restrict__ rgb,
                                                 const float* __restrict__ albedo,
                                                 const float* __restrict__ normal,
                                                 const float* __restrict__ depth, int64_t n,
                                                 int demod, v4f* __restrict__ col,
                                                 v4f* __restrict__ gd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
  const bool valid = isfinite(r) && isfinite(g) && isfinite(b);
  if (demod) {
    r = r / fmaxf(albedo[3 * i], 1e-3f);
    g = g / fmaxf(albedo[3 * i + 1], 1e-3f);
    b = b / fmaxf(albedo[3 * i + 2], 1e-3f);
  }
  if (!valid) r = g = b = 0.0f;
  const float d = depth ? depth[i] : 0.0f;
  v4f nv = {0.0f, 0.0f, 0.0f, valid ? 1.0f : 0.0f};
  if (normal) nv.x = normal[3 * i], nv.y = normal[3 * i + 1], nv.z = normal[3 * i + 2];
  *(glb_v4*)(col + i) = v4f{r, g, b, d};
  *(glb_v4*)(gd + i) = nv;
}

// TILE: taps from the LDS tile (step <= 2); FINAL: the last iteration writes `out`
template <bool TILE, bool FINAL>
__global__ __launch_bounds__(256) void k_dn_atrous(DnParams P, const v4f* __restrict__ cin,
                                                   const v4f* __restrict__ gd,
                                                   v4f* __restrict__ cout,
                                                   const float* rgb,  // may alias out
                                                   const float* __restrict__ albedo,
                                                   float* out) {
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
      v4f c = {0.0f, 0.0f, 0.0f, 0.0f}, g = {0.0f, 0.0f, 0.0f, 0.0f};  // outside: valid = 0
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
  const float sdp = P.sd * fmaxf(cp.w, 1e-6f);
  const float inv_d = P.sd > 0.0f ? fminf(1.0f / (sdp * sdp), kMaxInv) : 0.0f;
  const float hk[3] = {0.375f, 0.25f, 0.0625f};
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
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
      const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
      const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
      const float dd = cp.w - cq.w;
      const float arg = (dr * dr + dg * dg + db * db) * P.inv_c + (nx * nx + ny * ny + nz * nz) * P.inv_n +
                        dd * dd * inv_d;
      const float wgt = hk[dx < 0 ? -dx : dx] * hk[dy < 0 ? -dy : dy] * __expf(-arg) * gq.w * inside;
      sw += wgt;
      sr += wgt * cq.x;
      sg += wgt * cq.y;
      sb += wgt * cq.z;
    }
  }
  const bool valid = gp.w != 0.0f;
  const float inv = 1.0f / sw;
  const float r = valid ? sr * inv : cp.x, g = valid ? sg * inv : cp.y, b = valid ? sb * inv : cp.z;
  if constexpr (FINAL) {
    float o0, o1, o2;
    if (valid) {
      o0 = r, o1 = g, o2 = b;
      if (P.demod) {
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
  } else {
    *(glb_v4*)(cout + pi) = v4f{r, g, b, cp.w};
  }
}

// ---- variance-guided mode -------------------------------------------------------------------

struct DvParams {
  int w, h;
  float sl;      // sigma_lum (not shrunk per iteration: the variance shrinks by itself)
  float inv_n;   // 1 / sigma_normal^2, 0 = off
  float sd;      // sigma_depth, 0 = depth weight off
  int step;
  int demod;
};

constexpr float kLumEps = 1e-6f;

__device__ __forceinline__ float lum(float r, float g, float b) {
  return 0.2126f * r + 0.7152f * g + 0.0722f * b;  // the accumulator's weights
}

__global__ __launch_bounds__(256) void k_dnv_prep(const float* __restrict__ rgb,
                                                  const float* __restrict__ var,
                                                  const float* __restrict__ albedo,
                                                  const float* __restrict__ normal,
                                                  const float* __restrict__ depth, int64_t n,
                                                  int demod, v4f* __restrict__ col,
                                                  v4f* __restrict__ gd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2], v = var[i];
  const bool valid = isfinite(r) && isfinite(g) && isfinite(b) && isfinite(v);
  if (demod) {
    const float a0 = fmaxf(albedo[3 * i], 1e-3f), a1 = fmaxf(albedo[3 * i + 1], 1e-3f),
                a2 = fmaxf(albedo[3 * i + 2], 1e-3f);
    const float ya = lum(a0, a1, a2);
    r = r / a0;
    g = g / a1;
    b = b / a2;
    v = v / (ya * ya);
  }
  v = fmaxf(v, 0.0f);
  if (!valid) r = g = b = 0.0f, v = -1.0f;
  v4f nv = {0.0f, 0.0f, 0.0f, depth ? depth[i] : 0.0f};
  if (normal) nv.x = normal[3 * i], nv.y = normal[3 * i + 1], nv.z = normal[3 * i + 2];
  *(glb_v4*)(col + i) = v4f{r, g, b, v};
  *(glb_v4*)(gd + i) = nv;
}

// TILE: taps from the LDS tile (step <= 2); FINAL: the last iteration writes `out` / `var_out`
template <bool TILE, bool FINAL>
__global__ __launch_bounds__(256) void k_dnv_atrous(DvParams P, const v4f* __restrict__ cin,
                                                    const v4f* __restrict__ gd,
                                                    v4f* __restrict__ cout,
                                                    const float* rgb,  // may alias out
                                                    const float* var,  // may alias var_out
                                                    const float* __restrict__ albedo,
                                                    float* out, float* var_out) {
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
      v4f c = {0.0f, 0.0f, 0.0f, -1.0f}, g = {0.0f, 0.0f, 0.0f, 0.0f};  // outside: not valid
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
  // the 3 x 3 prefilter of the variance at p, over the adjacent pixels whatever the step
  const float k3[2] = {0.5f, 0.25f};
  float gs = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      float vq, inside = 1.0f;
      if constexpr (TILE) {  // the whole record: 64 consecutive 16-B reads, conflict-free
        const v4f cq = *(const lds_v4*)&lcol[(ty + halo + dy) * lw + tx + halo + dx];
        vq = cq.w;
      } else {
        const int qx = x + dx, qy = y + dy;
        const int cx = min(max(qx, 0), P.w - 1), cy = min(max(qy, 0), P.h - 1);
        inside = (cx == qx && cy == qy) ? 1.0f : 0.0f;
        vq = ((const float*)(cin + ((size_t)cy * P.w + cx)))[3];
      }
      const float k = k3[dx < 0 ? -dx : dx] * k3[dy < 0 ? -dy : dy] * (vq >= 0.0f ? 1.0f : 0.0f) * inside;
      gs += k * fmaxf(vq, 0.0f);
      gw += k;
    }
  }
  const float gvar = gw > 0.0f ? gs / gw : 0.0f;
  const float inv_l = 1.0f / (P.sl * sqrtf(gvar) + kLumEps);
  const float yp = lum(cp.x, cp.y, cp.z);
  const float sdp = P.sd * fmaxf(gp.w, 1e-6f);
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
      const float dl = fabsf(yp - lum(cq.x, cq.y, cq.z));
      const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
      const float dd = gp.w - gq.w;
      const float arg = dl * inv_l + (nx * nx + ny * ny + nz * nz) * P.inv_n + dd * dd * inv_d;
      const float wgt = hk[dx < 0 ? -dx : dx] * hk[dy < 0 ? -dy : dy] * __expf(-arg) *
                        (cq.w >= 0.0f ? 1.0f : 0.0f) * inside;
      sw += wgt;
      sr += wgt * cq.x;
      sg += wgt * cq.y;
      sb += wgt * cq.z;
      sv += wgt * wgt * fmaxf(cq.w, 0.0f);
    }
  }
  const bool valid = cp.w >= 0.0f;
  const float inv = 1.0f / sw;
  const float r = valid ? sr * inv : cp.x, g = valid ? sg * inv : cp.y, b = valid ? sb * inv : cp.z;
  const float v = valid ? sv * (inv * inv) : cp.w;
  if constexpr (FINAL) {
    float o0, o1, o2, ov;
    if (valid) {
      o0 = r, o1 = g, o2 = b, ov = v;
      if (P.demod) {
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
  } else {
    *(glb_v4*)(cout + pi) = v4f{r, g, b, v};
  }
}

// ---- emission split (rt_denoise_emit, rt_denoise_var_emit) ------------------------------------
//
// The iteration kernels above run unchanged on records written by a prep of the split inputs:
// c = (rgb - emission) / max(surface_albedo, 1e-3), and a pixel is also invalid when its
// emission is not finite or its coverage is not below 1.  The final iteration multiplies the
// surface albedo back and passes invalid pixels through; k_dn_emit_add then adds the emission
// to the valid ones.  It takes the validity from the records (the guide record's w, or the
// sign of the v the last iteration read), not from rgb, which an aliased out has overwritten.
// One lane per pixel, coalesced: 16 B + 40 B read and 32 B written by the prep, 4 B + 24 B read
// and 12 B written by the epilogue.

__global__ __launch_bounds__(256) void k_dn_prep_emit(const float* __restrict__ rgb,
                                                      const float* __restrict__ emission,
                                                      const float* __restrict__ salbedo,
                                                      const float* __restrict__ coverage,
                                                      const float* __restrict__ normal,
                                                      const float* __restrict__ depth, int64_t n,
                                                      int demod, v4f* __restrict__ col,
                                                      v4f* __restrict__ gd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
  const float e0 = emission[3 * i], e1 = emission[3 * i + 1], e2 = emission[3 * i + 2];
  const bool valid = isfinite(r) && isfinite(g) && isfinite(b) && isfinite(e0) && isfinite(e1) &&
                     isfinite(e2) && coverage[i] < 1.0f;
  r -= e0;
  g -= e1;
  b -= e2;
  if (demod) {
    r = r / fmaxf(salbedo[3 * i], 1e-3f);
    g = g / fmaxf(salbedo[3 * i + 1], 1e-3f);
    b = b / fmaxf(salbedo[3 * i + 2], 1e-3f);
  }
  if (!valid) r = g = b = 0.0f;
  const float d = depth ? depth[i] : 0.0f;
  v4f nv = {0.0f, 0.0f, 0.0f, valid ? 1.0f : 0.0f};
  if (normal) nv.x = normal[3 * i], nv.y = normal[3 * i + 1], nv.z = normal[3 * i + 2];
  *(glb_v4*)(col + i) = v4f{r, g, b, d};
  *(glb_v4*)(gd + i) = nv;
}

__global__ __launch_bounds__(256) void k_dnv_prep_emit(const float* __restrict__ rgb,
                                                       const float* __restrict__ var,
                                                       const float* __restrict__ emission,
                                                       const float* __restrict__ salbedo,
                                                       const float* __restrict__ coverage,
                                                       const float* __restrict__ normal,
                                                       const float* __restrict__ depth, int64_t n,
                                                       int demod, v4f* __restrict__ col,
                                                       v4f* __restrict__ gd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2], v = var[i];
  const float e0 = emission[3 * i], e1 = emission[3 * i + 1], e2 = emission[3 * i + 2];
  const bool valid = isfinite(r) && isfinite(g) && isfinite(b) && isfinite(v) && isfinite(e0) &&
                     isfinite(e1) && isfinite(e2) && coverage[i] < 1.0f;
  r -= e0;
  g -= e1;
  b -= e2;
  if (demod) {
    const float a0 = fmaxf(salbedo[3 * i], 1e-3f), a1 = fmaxf(salbedo[3 * i + 1], 1e-3f),
                a2 = fmaxf(salbedo[3 * i + 2], 1e-3f);
    const float ya = lum(a0, a1, a2);
    r = r / a0;
    g = g / a1;
    b = b / a2;
    v = v / (ya * ya);
  }
  v = fmaxf(v, 0.0f);
  if (!valid) r = g = b = 0.0f, v = -1.0f;
  v4f nv = {0.0f, 0.0f, 0.0f, depth ? depth[i] : 0.0f};
  if (normal) nv.x = normal[3 * i], nv.y = normal[3 * i + 1], nv.z = normal[3 * i + 2];
  *(glb_v4*)(col + i) = v4f{r, g, b, v};
  *(glb_v4*)(gd + i) = nv;
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

std::mutex g_mu;                 // one denoise at a time: the scratch buffers are shared
DeviceScratch g_work, g_stage;   // records (48 B per pixel); rt_denoise's staged host buffers

struct Resolved {
  int iterations;
  int demod;
  float sc, sn, sd;
};

// argument checks shared by both entry points (before any device is touched)
// emit: null for the parents; the split entries pass theirs, which replaces feat->albedo
int resolve(const char* who, const float* rgb, const rt_aov* feat, int w, int h,
            const rt_denoise_opts* opts, const float* out, Resolved* r,
            const rt_aov_emit* const* emit = nullptr) {
  if (w <= 0 || h <= 0) return set_error(RT_ERR_INVALID, "%s: %d x %d image", who, w, h);
  if ((int64_t)w * h >= ((int64_t)1 << 31) / 3)
    return set_error(RT_ERR_INVALID, "%s: %d x %d image", who, w, h);
  if ((h + kTH - 1) / kTH > 65535)  // one block row per kTH image rows: the grid's y limit
    return set_error(RT_ERR_INVALID, "%s: height %d above %d", who, h, 65535 * kTH);
  if (!rgb || !out) return set_error(RT_ERR_INVALID, "%s: null image", who);
  rt_denoise_opts o{};
  if (opts) o = *opts;
  if (o.iterations < 0 || o.iterations > 8)
    return set_error(RT_ERR_INVALID, "%s: %d iterations (1..8)", who, o.iterations);
  if (emit) {
    if (!*emit || !(*emit)->emission || !(*emit)->surface_albedo || !(*emit)->coverage)
      return set_error(RT_ERR_INVALID, "%s: needs the emission, surface_albedo and coverage buffers", who);
  } else if (o.demodulate && (!feat || !feat->albedo)) {
    return set_error(RT_ERR_INVALID, "%s: demodulate needs the albedo buffer", who);
  }
  if (!(o.sigma_color >= 0.0f) || !(o.sigma_normal >= 0.0f) || !(o.sigma_depth >= 0.0f))
    return set_error(RT_ERR_INVALID, "%s: negative or NaN sigma", who);
  r->iterations = o.iterations == 0 ? 5 : o.iterations;
  r->demod = o.demodulate ? 1 : 0;
  r->sc = o.sigma_color > 0.0f ? o.sigma_color : 0.5f;
  r->sn = o.sigma_normal > 0.0f ? o.sigma_normal : 0.3f;
  r->sd = o.sigma_depth > 0.0f ? o.sigma_depth : 0.02f;
  return RT_OK;
}

// rt_denoise_var's checks: rt_denoise's own (sigma_lum in sigma_color's place) and the variance
int resolve_var(const char* who, const float* rgb, const float* var, const rt_aov* feat, int w, int h,
                const rt_denoise_var_opts* opts, const float* out, Resolved* r,
                const rt_aov_emit* const* emit = nullptr) {
  rt_denoise_opts o{};
  if (opts) {
    o.iterations = opts->iterations;
    o.demodulate = opts->demodulate;
    o.sigma_color = opts->sigma_lum;
    o.sigma_normal = opts->sigma_normal;
    o.sigma_depth = opts->sigma_depth;
  }
  int rc = resolve(who, rgb, feat, w, h, &o, out, r, emit);
  if (rc) return rc;
  if (!var) return set_error(RT_ERR_INVALID, "%s: null variance", who);
  r->sc = o.sigma_color > 0.0f ? o.sigma_color : 1.0f;  // sigma_lum (the sweep)
  return RT_OK;
}

float inv_sq(double sigma) {
  const double v = 1.0 / (sigma * sigma);
  return (float)std::min(v, (double)kMaxInv);
}

// all pointers on the current device; g_mu held.  emit: the split mode (null: the parent)
int run(const float* rgb, const rt_aov* feat, const rt_aov_emit* emit, int w, int h, const Resolved& r,
        float* out, int device, hipStream_t s) {
  const int64_t n = (int64_t)w * h;
  void* wk = nullptr;
  int rc = g_work.get(device, (size_t)n * 48, &wk, "rt_denoise");
  if (rc) return rc;
  v4f* gd = (v4f*)wk;
  v4f* col[2] = {gd + n, gd + 2 * n};
  const float* albedo = emit ? emit->surface_albedo : feat ? feat->albedo : nullptr;
  const float* normal = feat ? feat->normal : nullptr;
  const float* depth = feat ? feat->depth : nullptr;
  const dim3 lin((unsigned)((n + 255) / 256));
  if (emit)
    hipLaunchKernelGGL(k_dn_prep_emit, lin, dim3(256), 0, s, rgb, emit->emission, albedo, emit->coverage,
                       normal, depth, n, r.demod, col[0], gd);
  else
    hipLaunchKernelGGL(k_dn_prep, lin, dim3(256), 0, s, rgb, albedo, normal, depth, n, r.demod, col[0], gd);
  HIP_OK(hipGetLastError());
  const dim3 grid((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kTH - 1) / kTH));
  for (int i = 0; i < r.iterations; ++i) {
    DnParams p;
    p.w = w;
    p.h = h;
    p.inv_c = inv_sq((double)r.sc * ldexp(1.0, -i));
    p.inv_n = normal ? inv_sq(r.sn) : 0.0f;
    p.sd = depth ? r.sd : 0.0f;
    p.step = 1 << i;
    p.demod = r.demod;
    const bool tile = 2 * p.step <= kMaxHalo, fin = i == r.iterations - 1;
    const v4f* in = col[i & 1];
    v4f* o = col[(i & 1) ^ 1];
    if (tile && fin) hipLaunchKernelGGL((k_dn_atrous<true, true>), grid, dim3(256), 0, s, p, in, gd, o, rgb, albedo, out);
    else if (tile) hipLaunchKernelGGL((k_dn_atrous<true, false>), grid, dim3(256), 0, s, p, in, gd, o, rgb, albedo, out);
    else if (fin) hipLaunchKernelGGL((k_dn_atrous<false, true>), grid, dim3(256), 0, s, p, in, gd, o, rgb, albedo, out);
    else hipLaunchKernelGGL((k_dn_atrous<false, false>), grid, dim3(256), 0, s, p, in, gd, o, rgb, albedo, out);
    HIP_OK(hipGetLastError());
  }
  if (emit) {  // the guide records keep the validity an aliased out has overwritten in rgb
    hipLaunchKernelGGL(k_dn_emit_add, lin, dim3(256), 0, s, gd, 0, emit->emission, n, out);
    HIP_OK(hipGetLastError());
  }
  return RT_OK;
}

// the variance-guided filter; all pointers on the current device (var_out may be null); g_mu held
int run_var(const float* rgb, const float* var, const rt_aov* feat, const rt_aov_emit* emit, int w, int h,
            const Resolved& r, float* out, float* var_out, int device, hipStream_t s) {
  const int64_t n = (int64_t)w * h;
  void* wk = nullptr;
  int rc = g_work.get(device, (size_t)n * 48, &wk, "rt_denoise_var");
  if (rc) return rc;
  v4f* gd = (v4f*)wk;
  v4f* col[2] = {gd + n, gd + 2 * n};
  const float* albedo = emit ? emit->surface_albedo : feat ? feat->albedo : nullptr;
  const float* normal = feat ? feat->normal : nullptr;
  const float* depth = feat ? feat->depth : nullptr;
  const dim3 lin((unsigned)((n + 255) / 256));
  if (emit)
    hipLaunchKernelGGL(k_dnv_prep_emit, lin, dim3(256), 0, s, rgb, var, emit->emission, albedo,
                       emit->coverage, normal, depth, n, r.demod, col[0], gd);
  else
    hipLaunchKernelGGL(k_dnv_prep, lin, dim3(256), 0, s, rgb, var, albedo, normal, depth, n, r.demod,
                       col[0], gd);
  HIP_OK(hipGetLastError());
  const dim3 grid((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kTH - 1) / kTH));
  for (int i = 0; i < r.iterations; ++i) {
    DvParams p;
    p.w = w;
    p.h = h;
    p.sl = r.sc;
    p.inv_n = normal ? inv_sq(r.sn) : 0.0f;
    p.sd = depth ? r.sd : 0.0f;
    p.step = 1 << i;
    p.demod = r.demod;
    const bool tile = 2 * p.step <= kMaxHalo, fin = i == r.iterations - 1;
    const v4f* in = col[i & 1];
    v4f* o = col[(i & 1) ^ 1];
    if (tile && fin) hipLaunchKernelGGL((k_dnv_atrous<true, true>), grid, dim3(256), 0, s, p, in, gd, o, rgb, var, albedo, out, var_out);
    else if (tile) hipLaunchKernelGGL((k_dnv_atrous<true, false>), grid, dim3(256), 0, s, p, in, gd, o, rgb, var, albedo, out, var_out);
    else if (fin) hipLaunchKernelGGL((k_dnv_atrous<false, true>), grid, dim3(256), 0, s, p, in, gd, o, rgb, var, albedo, out, var_out);
    else hipLaunchKernelGGL((k_dnv_atrous<false, false>), grid, dim3(256), 0, s, p, in, gd, o, rgb, var, albedo, out, var_out);
    HIP_OK(hipGetLastError());
  }
  if (emit) {  // the records the last iteration read keep the validity (v >= 0)
    hipLaunchKernelGGL(k_dn_emit_add, lin, dim3(256), 0, s, col[(r.iterations - 1) & 1], 1, emit->emission, n,
                       out);
    HIP_OK(hipGetLastError());
  }
  return RT_OK;
}

}  // namespace
}  // namespace rt

extern "C" {

int rt_denoise_device(const float* rgb_dev, const rt_aov* feat_dev, int w, int h,
                      const rt_denoise_opts* opts, float* out_dev, int device, void* stream) {
  using namespace rt;
  Resolved r;
  int rc = resolve("rt_denoise_device", rgb_dev, feat_dev, w, h, opts, out_dev, &r);
  if (rc) return rc;
  if ((rc = device_ok("rt_denoise_device", device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  hipStream_t s = (hipStream_t)stream;
  rc = run(rgb_dev, feat_dev, nullptr, w, h, r, out_dev, device, s);
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  if (rc) return rc;
  return RT_OK;
}

int rt_denoise(const float* rgb, const rt_aov* feat, int w, int h, const rt_denoise_opts* opts,
               float* out) {
  using namespace rt;
  Resolved r;
  int rc = resolve("rt_denoise", rgb, feat, w, h, opts, out, &r);
  if (rc) return rc;
  const int device = 0;
  if ((rc = device_ok("rt_denoise", device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  // staged: rgb (also the output) | albedo | normal | depth
  const size_t n = (size_t)w * h;
  void* stg = nullptr;
  if ((rc = g_stage.get(device, n * 40, &stg, "rt_denoise"))) return rc;
  float* d_rgb = (float*)stg;
  rt_aov f{nullptr, nullptr, nullptr, nullptr};
  hipStream_t s = nullptr;
  HIP_OK(hipMemcpyAsync(d_rgb, rgb, n * 12, hipMemcpyHostToDevice, s));
  if (feat && feat->albedo) {
    f.albedo = d_rgb + 3 * n;
    HIP_OK(hipMemcpyAsync(f.albedo, feat->albedo, n * 12, hipMemcpyHostToDevice, s));
  }
  if (feat && feat->normal) {
    f.normal = d_rgb + 6 * n;
    HIP_OK(hipMemcpyAsync(f.normal, feat->normal, n * 12, hipMemcpyHostToDevice, s));
  }
  if (feat && feat->depth) {
    f.depth = d_rgb + 9 * n;
    HIP_OK(hipMemcpyAsync(f.depth, feat->depth, n * 4, hipMemcpyHostToDevice, s));
  }
  rc = run(d_rgb, &f, nullptr, w, h, r, d_rgb, device, s);
  if (!rc && hipMemcpyAsync(out, d_rgb, n * 12, hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = set_error(RT_ERR_DEVICE, "rt_denoise: copy to host failed");
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  if (rc) return rc;
  return RT_OK;
}

int rt_denoise_var_device(const float* rgb_dev, const float* var_dev, const rt_aov* feat_dev, int w,
                          int h, const rt_denoise_var_opts* opts, float* out_dev, float* var_out_dev,
                          int device, void* stream) {
  using namespace rt;
  Resolved r;
  int rc = resolve_var("rt_denoise_var_device", rgb_dev, var_dev, feat_dev, w, h, opts, out_dev, &r);
  if (rc) return rc;
  if ((rc = device_ok("rt_denoise_var_device", device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  hipStream_t s = (hipStream_t)stream;
  rc = run_var(rgb_dev, var_dev, feat_dev, nullptr, w, h, r, out_dev, var_out_dev, device, s);
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  if (rc) return rc;
  return RT_OK;
}

int rt_denoise_var(const float* rgb, const float* var, const rt_aov* feat, int w, int h,
                   const rt_denoise_var_opts* opts, float* out, float* var_out) {
  using namespace rt;
  Resolved r;
  int rc = resolve_var("rt_denoise_var", rgb, var, feat, w, h, opts, out, &r);
  if (rc) return rc;
  const int device = 0;
  if ((rc = device_ok("rt_denoise_var", device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  // staged: rgb (also the output) | albedo | normal | depth | var (also the output)
  const size_t n = (size_t)w * h;
  void* stg = nullptr;
  if ((rc = g_stage.get(device, n * 44, &stg, "rt_denoise_var"))) return rc;
  float* d_rgb = (float*)stg;
  float* d_var = d_rgb + 10 * n;
  rt_aov f{nullptr, nullptr, nullptr, nullptr};
  hipStream_t s = nullptr;
  HIP_OK(hipMemcpyAsync(d_rgb, rgb, n * 12, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(d_var, var, n * 4, hipMemcpyHostToDevice, s));
  if (feat && feat->albedo) {
    f.albedo = d_rgb + 3 * n;
    HIP_OK(hipMemcpyAsync(f.albedo, feat->albedo, n * 12, hipMemcpyHostToDevice, s));
  }
  if (feat && feat->normal) {
    f.normal = d_rgb + 6 * n;
    HIP_OK(hipMemcpyAsync(f.normal, feat->normal, n * 12, hipMemcpyHostToDevice, s));
  }
  if (feat && feat->depth) {
    f.depth = d_rgb + 9 * n;
    HIP_OK(hipMemcpyAsync(f.depth, feat->depth, n * 4, hipMemcpyHostToDevice, s));
  }
  rc = run_var(d_rgb, d_var, &f, nullptr, w, h, r, d_rgb, var_out ? d_var : nullptr, device, s);
  if (!rc && (hipMemcpyAsync(out, d_rgb, n * 12, hipMemcpyDeviceToHost, s) != hipSuccess ||
              (var_out && hipMemcpyAsync(var_out, d_var, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = set_error(RT_ERR_DEVICE, "rt_denoise_var: copy to host failed");
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  if (rc) return rc;
  return RT_OK;
}

// ---- emission split: the parents' entries with an rt_aov_emit after feat ----

int rt_denoise_emit_device(const float* rgb_dev, const rt_aov* feat_dev, const rt_aov_emit* emit_dev,
                           int w, int h, const rt_denoise_opts* opts, float* out_dev, int device,
                           void* stream) {
  using namespace rt;
  Resolved r;
  int rc = resolve("rt_denoise_emit_device", rgb_dev, feat_dev, w, h, opts, out_dev, &r, &emit_dev);
  if (rc) return rc;
  if ((rc = device_ok("rt_denoise_emit_device", device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  hipStream_t s = (hipStream_t)stream;
  rc = run(rgb_dev, feat_dev, emit_dev, w, h, r, out_dev, device, s);
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  if (rc) return rc;
  return RT_OK;
}

int rt_denoise_var_emit_device(const float* rgb_dev, const float* var_dev, const rt_aov* feat_dev,
                               const rt_aov_emit* emit_dev, int w, int h,
                               const rt_denoise_var_opts* opts, float* out_dev, float* var_out_dev,
                               int device, void* stream) {
  using namespace rt;
  Resolved r;
  int rc = resolve_var("rt_denoise_var_emit_device", rgb_dev, var_dev, feat_dev, w, h, opts, out_dev, &r,
                       &emit_dev);
  if (rc) return rc;
  if ((rc = device_ok("rt_denoise_var_emit_device", device))) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  hipStream_t s = (hipStream_t)stream;
  rc = run_var(rgb_dev, var_dev, feat_dev, emit_dev, w, h, r, out_dev, var_out_dev, device, s);
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  if (rc) return rc;
  return RT_OK;
}

}  // extern "C"

namespace rt {
namespace {

// the two host entries of the split mode (var null: rt_denoise_emit); arguments already checked.
// staged: rgb (also the output) | surface_albedo | normal | depth | var (also the output) |
// emission | coverage
int host_emit(const char* who, const float* rgb, const float* var, const rt_aov* feat,
              const rt_aov_emit* emit, int w, int h, const Resolved& r, float* out, float* var_out) {
  const int device = 0;
  int rc = device_ok(who, device);
  if (rc) return rc;
  DeviceGuard dg;
  HIP_OK(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  const size_t n = (size_t)w * h;
  void* stg = nullptr;
  if ((rc = g_stage.get(device, n * 60, &stg, who))) return rc;
  float* d_rgb = (float*)stg;
  float* d_var = d_rgb + 10 * n;
  rt_aov f{nullptr, nullptr, nullptr, nullptr};
  rt_aov_emit e{d_rgb + 11 * n, d_rgb + 3 * n, d_rgb + 14 * n};
  hipStream_t s = nullptr;
  HIP_OK(hipMemcpyAsync(d_rgb, rgb, n * 12, hipMemcpyHostToDevice, s));
  if (var) HIP_OK(hipMemcpyAsync(d_var, var, n * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(e.emission, emit->emission, n * 12, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(e.surface_albedo, emit->surface_albedo, n * 12, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(e.coverage, emit->coverage, n * 4, hipMemcpyHostToDevice, s));
  if (feat && feat->normal) {
    f.normal = d_rgb + 6 * n;
    HIP_OK(hipMemcpyAsync(f.normal, feat->normal, n * 12, hipMemcpyHostToDevice, s));
  }
  if (feat && feat->depth) {
    f.depth = d_rgb + 9 * n;
    HIP_OK(hipMemcpyAsync(f.depth, feat->depth, n * 4, hipMemcpyHostToDevice, s));
  }
  rc = var ? run_var(d_rgb, d_var, &f, &e, w, h, r, d_rgb, var_out ? d_var : nullptr, device, s)
           : run(d_rgb, &f, &e, w, h, r, d_rgb, device, s);
  if (!rc && (hipMemcpyAsync(out, d_rgb, n * 12, hipMemcpyDeviceToHost, s) != hipSuccess ||
              (var_out && hipMemcpyAsync(var_out, d_var, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = set_error(RT_ERR_DEVICE, "%s: copy to host failed", who);
  HIP_OK(hipStreamSynchronize(s));  // also after an error: nothing in flight on the scratch
  return rc;
}

}  // namespace
}  // namespace rt

extern "C" {

int rt_denoise_emit(const float* rgb, const rt_aov* feat, const rt_aov_emit* emit, int w, int h,
                    const rt_denoise_opts* opts, float* out) {
  using namespace rt;
  Resolved r;
  int rc = resolve("rt_denoise_emit", rgb, feat, w, h, opts, out, &r, &emit);
  if (rc) return rc;
  return host_emit("rt_denoise_emit", rgb, nullptr, feat, emit, w, h, r, out, nullptr);
}

int rt_denoise_var_emit(const float* rgb, const float* var, const rt_aov* feat, const rt_aov_emit* emit,
                        int w, int h, const rt_denoise_var_opts* opts, float* out, float* var_out) {
  using namespace rt;
  Resolved r;
  int rc = resolve_var("rt_denoise_var_emit", rgb, var, feat, w, h, opts, out, &r, &emit);
  if (rc) return rc;
  return host_emit("rt_denoise_var_emit", rgb, var, feat, emit, w, h, r, out, var_out);
}

}  // extern "C"
