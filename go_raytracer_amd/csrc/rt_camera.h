// rt_camera.h — from a chunk id to a camera ray: the chunk -> pixel / sample mapping
// (Ids, chunk_pixel, chunk_ids), the camera constants in LDS (g_cam, stage_camera; the
// fused kernels' dynamic LDS is declared beside them) and getRay (camera_ray_r).
#pragma once
#include "rt_params.h"

namespace rt {

// chunk c -> (local pixel, global pixel, first sample).  The rank's pixels are
// taken in groups of G = fd_gpix.d consecutive pixels (G divides npix); a group's
// chunks are pixel-fastest over all its sample blocks, so a wave's consecutive
// chunks are adjacent pixels (coherent camera rays, different accumulators) and the
// chunks in flight cover only a few groups of the image (a small working set of the
// scene for the camera rays and their first bounces) instead of the whole image.
// G = npix is the image-wide pixel-fastest order.
struct Ids {
  uint32_t lpix, gpix, row, col, sample0, count;
};

// Two phases (render_impl): chunk ids [0, n1) cover samples [0, S1) of every pixel in
// chunks of K, ids [n1, n_chunks) the rest in chunks of K2 <= K, both in row-group order.
// The partitioned grab hands out the first phase before the tail, so the render's last
// chunks are short (the tail that idles lanes) while most samples pay the per-chunk cost of
// the large K.  `sub` is the sample block in its phase's units.
// (the tail's parameters are read from the kernel-argument segment where used, kparams:
// held in SGPRs for the whole kernel they cost the mesh and book1 kernels ~45 SGPR spills)
RT_D uint32_t chunk_pixel(const Params& P, uint32_t chunk, uint32_t& sub) {
  const cst_params* kp = kparams();
  const uint32_t n1 = kp->n1;
  const bool tail = chunk >= n1;
  const uint32_t c = tail ? chunk - n1 : chunk;
  const FastDiv fg = tail ? FastDiv{kp->fd_gchunks2.m, kp->fd_gchunks2.s1, kp->fd_gchunks2.s2,
                                    kp->fd_gchunks2.d}
                          : P.fd_gchunks;
  const uint32_t qs = fdiv(c, fg);
  const uint32_t r = c - qs * fg.d;
#ifdef RT_SWEEP_ORDER  // (opt-in build: RT_SWEEP=reverse, DESIGN.md §8 "Sweep order")
  const uint32_t q = (qs ^ kp->gflip) + kp->gbase;  // the group at this sweep position
#else
  const uint32_t q = qs;
#endif
  sub = fdiv(r, P.fd_gpix);
  return q * P.fd_gpix.d + (r - sub * P.fd_gpix.d);
}
// ONE: a launch without a tail phase (S1 = ss), with the launch parameters held in SGPRs:
// the record-loop kernel, whose chunk starts lost 3 % to the tail mapping's kernel-argument
// loads (profiles/r4_tail_code_ab.jsonl); render_impl never gives it a tail
// MAP: an active-pixel pass.  lpix, the chunk records and the pass's sums stay
// in the pass's own (virtual) pixels, P.npix of them; row, col and gpix, which key the random
// stream and aim the camera ray, are those of the share's pixel pixmap[lpix].  The table's
// address is read from the kernel-argument segment where a chunk starts (kparams), not held
// in SGPRs across the loop.
template <bool MAP>
RT_D uint32_t mapped_pixel(uint32_t lpix) {
  if constexpr (MAP) return *(const glb_u32*)(kparams()->pixmap + lpix);
  return lpix;
}
template <bool ONE = false, bool MAP = false>
RT_D Ids chunk_ids(const Params& P, uint32_t chunk) {
  Ids r;
  uint32_t sub;
  if (ONE) {
    const uint32_t q = fdiv(chunk, P.fd_gchunks);
    const uint32_t rr = chunk - q * P.fd_gchunks.d;
    sub = fdiv(rr, P.fd_gpix);
    r.lpix = q * P.fd_gpix.d + (rr - sub * P.fd_gpix.d);
    const uint32_t rp = mapped_pixel<MAP>(r.lpix);
    const uint32_t row_l = fdiv(rp, P.fd_width);
    r.col = rp - row_l * (uint32_t)P.width;
    r.row = row_l * (uint32_t)P.nranks + (uint32_t)P.rank;
    r.gpix = r.row * (uint32_t)P.width + r.col;
    r.sample0 = sub * P.K;
    r.count = min(P.K, P.ss - r.sample0);
    return r;
  }
  r.lpix = chunk_pixel(P, chunk, sub);
  const uint32_t rp = mapped_pixel<MAP>(r.lpix);
  uint32_t row_l = fdiv(rp, P.fd_width);
  r.col = rp - row_l * (uint32_t)P.width;
  r.row = row_l * (uint32_t)P.nranks + (uint32_t)P.rank;
  r.gpix = r.row * (uint32_t)P.width + r.col;
  const cst_params* kp = kparams();
  const bool tail = chunk >= kp->n1;
  const uint32_t S1 = kp->S1, K2 = kp->K2;
  r.sample0 = tail ? S1 + sub * K2 : sub * P.K;
  r.count = tail ? min(K2, P.ss - r.sample0) : min(P.K, S1 - r.sample0);
  return r;
}

// The camera constants in LDS (every kernel that starts samples stages them once,
// stage_camera): read with broadcast ds_reads where a ray starts instead of held in
// SGPRs for the whole kernel (the fused kernels run out of SGPRs and spill them to
// VGPR lanes, one v_readlane per use).  [0] pixel00 - center | 1/s, [1] du | fd_s.m,
// [2] dv | fd_s shifts, [3] center | s, [4] defocus u | defocus flag, [5] defocus v.
__shared__ F4 g_cam[6];
// the dynamic LDS of the fused kernels (k_fused's lnodes: tree, records, shade table)
extern __shared__ F4 g_dyn_lds[];
// Where a fused kernel reads the camera constants: 1 = g_cam (book2 set: round 2, against
// SGPR-resident constants, C4 -3.6 %, fewer SGPR and VGPR spills), 2 = scalar loads from the
// kernel-argument segment where a ray starts (kparams: SGPRs live only there).  Mode 0, the
// SGPRs the compiler holds P in for the whole kernel, is the wavefront kernels'.  Measured
// against 0, mode 2 took C2's SGPR spills to VGPR lanes from 78 to 34 and C3's from 101 to
// 32: C2 -1.9 / -4.6 %, C3 -2.1 / -2.5 % (two boxes); against 1, C5 -2.0 / -2.2 % but C4
// +1.1 % (profiles/r3_cam_kernarg_ab.jsonl); images bit-identical.
constexpr int cam_mode(uint32_t ft) { return ft == FT_SET_BOOK2 ? 1 : 2; }
RT_D void stage_camera(const Params& P) {  // before a __syncthreads of every thread
  if (threadIdx.x == 0) {
    g_cam[0] = {P.p00r[0], P.p00r[1], P.p00r[2], P.recip_s};
    g_cam[1] = {P.du[0], P.du[1], P.du[2], bitsf(P.fd_s.m)};
    g_cam[2] = {P.dv[0], P.dv[1], P.dv[2], bitsf(P.fd_s.s1 | (P.fd_s.s2 << 8))};
    g_cam[3] = {P.cc[0], P.cc[1], P.cc[2], bitsf((uint32_t)P.s)};
    g_cam[4] = {P.dku[0], P.dku[1], P.dku[2], bitsf((uint32_t)P.defocus)};
    g_cam[5] = {P.dkv[0], P.dkv[1], P.dkv[2], 0.0f};
  }
}

// getRay camera.go:256-270 + sampleSquareStratified :277-282 + defocusDiskSample :285-290;
// r = rt_rng_draw(seed, gpix, sample, RT_STREAM_CAMERA), drawn by the caller.
// CAM: where the constants come from (cam_mode): P (0), g_cam (1) or the kernarg segment (2).
template <int CAM>
RT_D void camera_ray_r(const Params& P, const Ids& id, uint32_t sample, const rt_u32x4& r, f3& o,
                       f3& d, float& time) {
  F4 c0, c1, c2, c3;
  FastDiv fd_s;
  uint32_t s;
  bool defocus;
  if constexpr (CAM == 1) {
    c0 = ld_lds(&g_cam[0]), c1 = ld_lds(&g_cam[1]), c2 = ld_lds(&g_cam[2]), c3 = ld_lds(&g_cam[3]);
    const uint32_t sh = fbits(c2.w);
    s = fbits(c3.w);
    fd_s = {fbits(c1.w), sh & 0xFFu, sh >> 8, s};
    defocus = fbits(ld_lds(&g_cam[4]).w) != 0u;
  } else if constexpr (CAM == 2) {
    const cst_params* kp = kparams();
    c0 = {kp->p00r[0], kp->p00r[1], kp->p00r[2], kp->recip_s};
    c1 = {kp->du[0], kp->du[1], kp->du[2], 0.0f};
    c2 = {kp->dv[0], kp->dv[1], kp->dv[2], 0.0f};
    c3 = {kp->cc[0], kp->cc[1], kp->cc[2], 0.0f};
    fd_s = {kp->fd_s.m, kp->fd_s.s1, kp->fd_s.s2, kp->fd_s.d};
    s = (uint32_t)kp->s;
    defocus = kp->defocus != 0;
  } else {
    c0 = {P.p00r[0], P.p00r[1], P.p00r[2], P.recip_s};
    c1 = {P.du[0], P.du[1], P.du[2], 0.0f};
    c2 = {P.dv[0], P.dv[1], P.dv[2], 0.0f};
    c3 = {P.cc[0], P.cc[1], P.cc[2], 0.0f};
    fd_s = P.fd_s;
    s = (uint32_t)P.s;
    defocus = P.defocus != 0;
  }
  uint32_t si = fdiv(sample, fd_s), sj = sample - si * s;
  float px = (((float)sj + rt_unit_f(r.v[0])) * c0.w) - 0.5f;
  float py = (((float)si + rt_unit_f(r.v[1])) * c0.w) - 0.5f;
  float fx = (float)id.col + px, fy = (float)id.row + py;
  // pixelSample - rayOrigin rearranged as (pixel00 - center) + du*fx + dv*fy - disk:
  // the same vector without fp32 cancellation against large camera coordinates
  d = mk3(c0.x + c1.x * fx + c2.x * fy, c0.y + c1.y * fx + c2.y * fy, c0.z + c1.z * fx + c2.z * fy);
  o = mk3(c3.x, c3.y, c3.z);
  if (defocus) {
    F4 c4, c5;
    if constexpr (CAM == 1) {
      c4 = ld_lds(&g_cam[4]), c5 = ld_lds(&g_cam[5]);
    } else if constexpr (CAM == 2) {
      const cst_params* kp = kparams();
      c4 = {kp->dku[0], kp->dku[1], kp->dku[2], 0.0f};
      c5 = {kp->dkv[0], kp->dkv[1], kp->dkv[2], 0.0f};
    } else {
      c4 = {P.dku[0], P.dku[1], P.dku[2], 0.0f};
      c5 = {P.dkv[0], P.dkv[1], P.dkv[2], 0.0f};
    }
    // the disk's two uniforms are the halves of camera word [3] (rt_rng.h): no second
    // Philox call per defocused camera ray (C3, C5)
    f3 dk = uniform_disk(rt_unit16_hi_f(r.v[3]), rt_unit16_lo_f(r.v[3]));
    f3 off = mk3(c4.x, c4.y, c4.z) * dk.x + mk3(c5.x, c5.y, c5.z) * dk.y;
    o = o + off;
    d = d - off;
  }
  time = rt_unit_f(r.v[2]);
}

}  // namespace rt
