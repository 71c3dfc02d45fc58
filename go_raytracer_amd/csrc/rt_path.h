// rt_path.h — per-path device logic shared by the wavefront and fused kernels, on top of
// the layers it includes (rt_params.h, rt_camera.h, rt_trav.h, rt_records.h, rt_shade.h):
// the exact fixed-point pixel sums (SampleAcc), the path state (Path), the clamp-weight
// stack (WStack), the shading core (shade_core: one rayColor vertex, camera.go:293-331),
// the drain's sample split and the wave-batched chunk grab (WaveBatch).
// The shading core is templated on where path state lives: HBM structure-of-
// arrays (wavefront kernels) or registers (fused persistent kernel).
#pragma once
#include "rt_camera.h"
#include "rt_shade.h"

namespace rt {

// ---------------------------------------------------------- pixel sums -----
// pixelColor += rayColor(...) (camera.go:97-101) for every sample, in fixed point:
// each sample's channel becomes floor(v * 2^32) and the pixel sums are int64, so
// the sum is exact and independent of how samples are grouped into chunks, which
// lane or kernel renders them, and how rows are split over ranks (bitwise the same
// image for any chunk size, schedule, strategy and GPU count).  |v| < vlim = 2^31/ss
// keeps the ss-sample sum inside int64; a finite sample outside that range (never
// in the BASELINE scenes) is added in fp64 to a side plane and counted
// (Counters::overflow, rt_stats.overflow_samples); NaN and +-Inf set pixel flags
// with the reference's sum semantics (NaN, or +Inf and -Inf, give NaN).
RT_D uint32_t local_pixel(const Params& P, uint32_t chunk) {
  uint32_t sub;
  return chunk_pixel(P, chunk, sub);
}
// floor(v * 2^32) for |v| < 2^31: the integer part in the high word, the fraction
// in the low.  v - floor(v) is exact except for v in (-2^-24, 0), where it rounds
// to 1.0f; the fraction is capped at 1 - 2^-24 so its conversion stays in range
// (those samples count as -2^-24: error below 2^-24, still a fixed function of v,
// so the sums stay order-independent); * 2^32 only moves the exponent.
RT_D unsigned long long to_fixed(float v) {
  const float hi = floorf(v);
  const uint32_t lo = (uint32_t)(fminf(v - hi, 0x1.fffffep-1f) * 4294967296.0f);
  return ((unsigned long long)(uint32_t)(int32_t)hi << 32) | lo;
}
// a sample with a channel outside the fixed-point range or non-finite (rare): every
// channel goes straight to the pixel (fixed-point channels included: the integer sum
// does not care where it is added)
// (the buffers' addresses re-read from the kernel-argument segment: held across the fused
// loop for these rare branches they cost the record-loop kernel spilled VGPRs)
RT_D void add_sample_rare(const Params& P, uint32_t lp, float x, float y, float z) {
  const cst_params* kp = kparams();
  const float c[3] = {x, y, z};
  for (int ch = 0; ch < 3; ++ch) {
    const float v = c[ch];
    if (fabsf(v) < kp->vlim) {
      atomicAdd(&kp->accum[(size_t)ch * kp->npix + lp], to_fixed(v));
    } else if (isnan(v)) {
      atomicOr(&kp->pflags[lp], 1u << ch);
    } else if (isinf(v)) {
      atomicOr(&kp->pflags[lp], (v > 0.0f ? 8u : 64u) << ch);
    } else {
      atomicAdd(&kp->side[(size_t)ch * kp->npix + lp], (double)v);
      atomicAdd(&kp->ctr->overflow, 1ull);
    }
  }
}
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
// Per-lane chunk sums: the fused kernel keeps them in an LDS column (3 x u64 per
// lane, [channel][thread]; ds_add_u64, no registers held across the path) and
// flushes them to the pixel with one global atomic per channel when the chunk
// ends; the wavefront kernels (lds == null) add every sample to the pixel.
struct SampleAcc {
  unsigned long long* lds;  // &lacc[0][threadIdx.x], stride 256, or null
  RT_D void add(const Params& P, uint32_t chunk, f3 L) const {
    const bool fixed = fabsf(L.x) < P.vlim && fabsf(L.y) < P.vlim && fabsf(L.z) < P.vlim;
    if (!fixed) {
      add_sample_rare(P, local_pixel(P, chunk), L.x, L.y, L.z);
      return;
    }
    const unsigned long long fx = to_fixed(L.x), fy = to_fixed(L.y), fz = to_fixed(L.z);
    if (lds) {
      __atomic_fetch_add((lds_u64*)lds, fx, __ATOMIC_RELAXED);
      __atomic_fetch_add((lds_u64*)lds + 256, fy, __ATOMIC_RELAXED);
      __atomic_fetch_add((lds_u64*)lds + 512, fz, __ATOMIC_RELAXED);
    } else {
      const uint32_t lp = local_pixel(P, chunk);
      atomicAdd(&P.accum[lp], fx);
      atomicAdd(&P.accum[(size_t)P.npix + lp], fy);
      atomicAdd(&P.accum[2 * (size_t)P.npix + lp], fz);
    }
  }
  RT_D void flush(const Params& P, uint32_t chunk, bool split = false) const {
    if (!lds) return;
    if (P.csum && !split) {
      // the chunk's own 32-B record, two plain 16-B stores.  A pixel atomic is performed
      // beyond L2 and completes late, and every later s_waitcnt vmcnt of the wave (the
      // traversal's node loads, the shading's) waited for it: C3 -4.4 %, C2 -2.5 %, C4
      // -1.5 % without them (profiles/r4_flush_*); stores retire at L2
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      typedef __attribute__((address_space(1))) u64x2 glb_u64x2;
      const unsigned long long s0 = ((lds_u64*)lds)[0], s1 = ((lds_u64*)lds)[256],
                               s2 = ((lds_u64*)lds)[512];
      ((lds_u64*)lds)[0] = 0ull;
      ((lds_u64*)lds)[256] = 0ull;
      ((lds_u64*)lds)[512] = 0ull;
      glb_u64x2* rec = (glb_u64x2*)(P.csum + 4 * (size_t)chunk);
      rec[0] = u64x2{s0, s1};
      rec[1] = u64x2{s2, 0ull};
      return;
    }
    const uint32_t lp = local_pixel(P, chunk);
    const cst_params* kp = kparams();  // (as add_sample_rare: a rare branch)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      lds_u64* q = (lds_u64*)lds + ch * 256;
      const unsigned long long s = *q;
      *q = 0ull;
      if (s) atomicAdd(&kp->accum[(size_t)ch * kp->npix + lp], s);
    }
  }
};

// ------------------------------------------------------------- path state --
// One path.  In the fused kernel every field lives in registers; in the
// wavefront kernels ray/key fields are loaded from SoA and pend/pre/acc are
// touched in HBM only when a vertex needs them (SOA = true).
struct Path {
  f3 o, d;
  float time;
  uint32_t chunk, j, k, nst, flags;
  uint32_t gpix, s0;  // global pixel and first sample of the chunk (chunk_ids, cached)
  uint32_t spare;     // rt_spare24 of the call that generated the ray (trace_media)
  f3 pend, pre;
  uint32_t segs;    // world.Hit calls of this lane (statistics)
  uint32_t pushes;  // clamp weights stored (statistics, RT_COUNT_PUSHES builds only)
};

template <bool SOA>
RT_D f3 get_pend(const Params& P, uint32_t slot, const Path& s) {
  return SOA ? xyz(P.pend[slot]) : s.pend;
}
template <bool SOA>
RT_D void set_pend(const Params& P, uint32_t slot, Path& s, f3 v) {
  if (SOA) P.pend[slot] = {v.x, v.y, v.z, 0.0f};
  else s.pend = v;
}
template <bool SOA>
RT_D f3 get_pre(const Params& P, uint32_t slot, const Path& s) {
  return SOA ? xyz(P.pre[slot]) : s.pre;
}
template <bool SOA>
RT_D void set_pre(const Params& P, uint32_t slot, Path& s, f3 v) {
  if (SOA) P.pre[slot] = {v.x, v.y, v.z, 0.0f};
  else s.pre = v;
}

// Clamp-weight stack: entries below nlds in an LDS column (fused kernel, one
// per thread), the rest in HBM [entry - nlds][slot].  LDS keeps the common
// shallow pushes off the vector-memory counter (a store holds vmcnt for
// hundreds of cycles and every later load waits behind it).
struct WStack {
  float* lds;  // &lds_w[0][0][threadIdx.x]: [channel][entry][thread] planes, 12 B per entry
  int nlds;
  RT_D void put(const Params& P, uint32_t slot, uint32_t k, F4 v) const {
    if ((int)k < nlds) {
      lds_f32* q = (lds_f32*)lds + k * 256;
      q[0] = v.x;
      q[nlds * 256] = v.y;
      q[2 * nlds * 256] = v.z;
    } else {
      st_glb(hbm_entry(P, slot, k), v);
    }
  }
  // entry k (the top) *= w: a dominated clamp vertex merged into it (shade_core);
  // returns the new entry
  RT_D f3 mul(const Params& P, uint32_t slot, uint32_t k, f3 w) const {
    f3 r;
    if ((int)k < nlds) {
      lds_f32* q = (lds_f32*)lds + k * 256;
      r = mk3(q[0] * w.x, q[nlds * 256] * w.y, q[2 * nlds * 256] * w.z);
      q[0] = r.x;
      q[nlds * 256] = r.y;
      q[2 * nlds * 256] = r.z;
    } else {
      F4* e = hbm_entry(P, slot, k);
      const F4 v = ld_glb(e);
      r = mk3(v.x * w.x, v.y * w.y, v.z * w.z);
      st_glb(e, {r.x, r.y, r.z, 0.0f});
    }
    return r;
  }
  // HBM entries: [entry][slot] (a wave's lanes at one depth coalesce; [slot][entry], one
  // lane's pushes sharing cache lines, measured slower).
  // The entry's address, with the stack base and column count re-read from the
  // kernel-argument segment (kparams): these rare HBM branches otherwise kept a 64-bit base
  // live across the fused loop (2 spilled VGPRs in the record-loop kernel)
  RT_D F4* hbm_entry(const Params& P, uint32_t slot, uint32_t k) const {
    const cst_params* kp = kparams();
    return kp->stack + ((size_t)(k - nlds) * kp->P + slot);
  }
  // The backward clamp fold (camera.go:328-330) as one scale.  A clamp only scales its
  // vector, by s_k = min(1, M / I(w_k (.) v_k+1)) with I the channel sum, so the folded
  // value is (prod s_k) times the plain product P_0 = w_0 (.) ... (.) w_n (.) L, and the
  // scales telescope: prod s_k = min(1, min_k M / I(P_k)) over the suffix products
  // P_k = w_k (.) ... (.) L.  So the walk from the last weight back multiplies and
  // keeps the largest channel sum; one scale by M / max I at the end (if max I > M)
  // replaces a compare, reciprocal and select per clamp vertex.  Same value as the
  // step-by-step clamps up to fp32 rounding (weights and radiance are non-negative).
  // `v` is pend (.) L with maxI = I(v) on entry; entries nst-1 .. 0: HBM ones (rare)
  // one by one, then the LDS ones, unrolled.
  RT_D void fold_max(const Params& P, uint32_t slot, uint32_t nst, f3& v, float& maxI) const {
    int k = (int)nst - 1;
    // HBM entries two at a time: both loads in flight before the products need them
    for (; k - 1 >= nlds; k -= 2) {
      const F4 a = ld_glb(hbm_entry(P, slot, (uint32_t)k));
      const F4 b = ld_glb(hbm_entry(P, slot, (uint32_t)(k - 1)));
      v = xyz(a) * v;
      maxI = fmaxf(maxI, v.x + v.y + v.z);
      v = xyz(b) * v;
      maxI = fmaxf(maxI, v.x + v.y + v.z);
    }
    for (; k >= nlds; --k) {
      v = xyz(ld_glb(hbm_entry(P, slot, (uint32_t)k))) * v;
      maxI = fmaxf(maxI, v.x + v.y + v.z);
    }
    if (nlds > 0 && nst > 0) {
      const lds_f32* q = (const lds_f32*)lds;
      f3 e[kLdsWMax];
#pragma unroll
      for (int i = 0; i < kLdsWMax; ++i)
        if (i < nlds)  // entries >= nst are garbage, unused
          e[i] = mk3(q[i * 256], q[(nlds + i) * 256], q[(2 * nlds + i) * 256]);
#pragma unroll
      for (int i = kLdsWMax - 1; i >= 0; --i)
        if (i < nlds && i < (int)nst) {
          v = e[i] * v;
          maxI = fmaxf(maxI, v.x + v.y + v.z);
        }
    }
  }
};

template <bool SOA>
RT_D void store_ray(const Params& P, uint32_t slot, const Path& s) {
  if (SOA) {
    P.ray_o[slot] = {s.o.x, s.o.y, s.o.z, s.time};
    P.ray_d[slot] = {s.d.x, s.d.y, s.d.z, bitsf(s.spare)};
    P.path[slot] = make_uint2(s.chunk, pack_path(s.j, s.k, s.nst, s.flags));
  }
}

RT_D void load_path(const Params& P, uint32_t slot, Path& s) {
  const F4 ro = P.ray_o[slot], rd = P.ray_d[slot];
  const uint2 ps = P.path[slot];
  s.o = xyz(ro);
  s.time = ro.w;
  s.d = xyz(rd);
  s.spare = fbits(rd.w);
  s.chunk = ps.x;
  const Ids id = chunk_ids(P, s.chunk);
  s.gpix = id.gpix;
  s.s0 = id.sample0;
  s.j = ps.y & 0xFFFu;
  s.k = (ps.y >> 12) & 0xFFu;
  s.nst = (ps.y >> 20) & 0xFFu;
  s.flags = (ps.y >> 28) | (id.count << kCountShift);
}

// the next sample of the same chunk, its camera draw already made: the path
// state (pixel ids cached in s) is reset for sample j
template <bool SOA, int CAM = 0>
RT_D void next_sample(const Params& P, uint32_t slot, Path& s, uint32_t j, const rt_u32x4& r) {
  Ids id;
  id.gpix = s.gpix;
  id.row = fdiv(s.gpix, P.fd_width);
  id.col = s.gpix - id.row * (uint32_t)P.width;
  camera_ray_r<CAM>(P, id, s.s0 + j, r, s.o, s.d, s.time);
  s.spare = rt_spare24(r);
  s.j = j;
  s.k = 0;
  s.nst = 0;
  s.flags &= ~(F_SPLIT - 1u);  // the chunk's sample count and F_SPLIT stay
  store_ray<SOA>(P, slot, s);
}

// camera ray for sample j of `chunk` (path state reset)
template <bool SOA, int CAM = 0, bool ONE = false, bool MAP = false>
RT_D void start_sample(const Params& P, uint32_t slot, Path& s, uint32_t chunk, uint32_t j) {
  Ids id = chunk_ids<ONE, MAP>(P, chunk);
  const rt_u32x4 r = rt_rng_draw(P.seed, id.gpix, id.sample0 + j, RT_STREAM_CAMERA);
  camera_ray_r<CAM>(P, id, id.sample0 + j, r, s.o, s.d, s.time);
  s.spare = rt_spare24(r);
  s.chunk = chunk;
  s.gpix = id.gpix;
  s.s0 = id.sample0;
  s.j = j;
  s.k = 0;
  s.nst = 0;
  s.flags = id.count << kCountShift;
  store_ray<SOA>(P, slot, s);
}

// debug path trace (Params::trace): one world.Hit of the traced sample
RT_D void record_trace(const Params& P, const Path& s, const Hit& best) {
  if (s.gpix == P.trace_gpix && s.s0 + s.j == P.trace_sample && (int)s.k < P.trace_cap) {
    P.trace[3 * s.k + 0] = {s.o.x, s.o.y, s.o.z, s.time};
    P.trace[3 * s.k + 1] = {s.d.x, s.d.y, s.d.z, (float)s.k};
    P.trace[3 * s.k + 2] = {best.t, best.u, best.v, bitsf(best.ref)};
  }
}

// One vertex of rayColor (camera.go:293-331) given its closest hit.
// Returns OUT_ALIVE (continue with s.o/s.d), or OUT_NEED_CHUNK (chunk flushed).
// LIGHT: the lean light kind the light sampling and light pdf are compiled for (rt_device.h;
// the lean LDS record-loop kernel only, k_fused), 0 = any light list
// EARLY_SHAPE (that kernel with a lean light kind only: the listed record layout the
// early-draw variant is compiled for, k_fused's SHAPE; 0 = no early draw): h is
// trav_brute<.., EARLY>'s {t, -, -, bk}, the winner still unresolved.  "The hit
// scatters" is then known from bk alone -- a winner that is not the emitter slot, by the host
// matcher (host_records.cpp emitter_slot_of) the shade table's M.kind != RT_MAT_DIFFUSE_LIGHT --
// so the vertex's Philox call is issued first and the winner's dependent LDS reads (box
// fields, face slot, ref, shade table; all unconditional, lrec = the records in LDS) follow
// in the same block, for the scheduler to start them ahead of the ten Philox rounds.  The
// same draws and the same hit as resolving first.
template <bool SOA, uint32_t FT, int LIGHT = 0, int EARLY_SHAPE = 0>
RT_D int shade_core(const Params& P, uint32_t slot, Path& s, const Hit& h, const WStack& ws,
                    const SampleAcc& sa, const F4* lrec = nullptr) {
  static_assert(EARLY_SHAPE == 0 || (FT == 0u && LIGHT != 0 && !SOA), "early draw: the lean light kernels only");
  const DevScene& sc = P.sc;
  const f3 o = s.o, d = s.d;
  const float time = s.time;
  rt_u32x4 r;
  bool scat = false;
  uint32_t ref = h.ref;
  F4 etab_a = {0, 0, 0, 0}, etab_b = {0, 0, 0, 0};  // early draw: the winner's shade-table rows
  if constexpr (EARLY_SHAPE != 0) {
    const uint32_t bk = h.ref;
    scat = bk != 0xFFFFFFFFu && bk != fbits(kparams()->ll.f[11]);
    r = rt_rng_draw(P.seed, s.gpix, s.s0 + s.j + (scat ? 0u : 1u),
                    scat ? RT_STREAM(s.k, 0) : RT_STREAM_CAMERA);
    uint32_t ref_raw;
    const uint32_t wslot = brute_resolve_early<EARLY_SHAPE>(sc, lrec, bk, o, d, h.t, ref_raw);
    const F4* tab = g_dyn_lds + sc.shade_lds + 2 * (ref_raw & 0x3FFFFFFFu);
    etab_a = ld_lds(tab), etab_b = ld_lds(tab + 1);
    ref = bk != 0xFFFFFFFFu ? ref_raw : PRIM_NONE;
    if (P.trace) {  // debug trace (finish_hit): the hit as trav_brute resolves it
      Hit th = {h.t, h.u, h.v, ref};
      if (ref != PRIM_NONE) brute_slot_uv(lrec, wslot, o, d, h.t, th.u, th.v);
      record_trace(P, s, th);
    }
  }
  f3 lterm = mk3(0, 0, 0);
  bool term = false;
  rt_u32x4 rcam;  // camera draw of the next sample, when this vertex made it
  bool have_rcam = false;
  f3 p = mk3(0, 0, 0), n = mk3(0, 0, 0);
  float u = h.u, v = h.v;
  bool ff = true;
  DevMaterial M;
  // lean record-loop kernel: the quad's normal, material kind and solid colour from the
  // shade table in LDS (rt_render.hip), no global loads
  bool ltab = false;
  f3 lcol = mk3(0, 0, 0);
  // The hit point goes back onto the surface it was found on.  r.At(t) in fp32 carries
  // the rounding of t along the ray (~|p - o| * 2^-22: up to ~1e-4 off the surface for the
  // long rays of the 555- and 1000-unit scenes), and from a point that far on the wrong
  // side a next ray leaving at a grazing angle re-hits the same quad or sphere at t >=
  // 0.001 -- a vertex the fp64 reference (point on the surface to ~1e-13) never makes.
  // That self-hit was 98 % of C2's and ~40 % of C4's forked samples
  // (tools/fork_census.py).  Quads: projected onto their plane, p - n (n.p - D), exact for
  // axis-aligned quads (every term is an exact zero or a Sterbenz difference, so p lands
  // ON the plane and the next test's t is exactly 0).  Spheres: onto the sphere, and then
  // `eta` (4x the rounding left) to the side the next ray leaves on (below).
  float eta = 0.0f;
  if (ref != PRIM_NONE) {
    const float t = h.t;
    p = o + d * t;  // r.At(t)
    const uint32_t type = ref >> 30, idx = ref & 0x3FFFFFFFu;
    f3 nout;
    int mat;
    if (HAS(FT_SPHERE) && type == PRIM_SPHERE) {
      const F4 cr = sc.sph_cr[idx], mv = sc.sph_mv[idx];
      f3 cc = xyz(cr) + xyz(mv) * time;
      // p moved along the unit normal by r - |p - c|, that offset from r^2 - |p - c|^2
      // formed in fp64 (the sphere test's centre; every fp32 square is exact there), so the
      // point is on the sphere to its coordinates' rounding, ~2^-24 sum|p_i n_i|, even for
      // the R=1000 ground where p - c cancels in fp32.  eta, 4x that bound, then puts it
      // on the right side (below).  nout = (p - c) / r objects.go:102 (a negative radius
      // keeps its inward normal).
      {
        const double cx = (double)cr.x + (double)time * (double)mv.x;
        const double cy = (double)cr.y + (double)time * (double)mv.y;
        const double cz = (double)cr.z + (double)time * (double)mv.z;
        const double ex = (double)p.x - cx, ey = (double)p.y - cy, ez = (double)p.z - cz;
        const double rr = (double)cr.w;
        const float dn = (float)(rr * rr - (ex * ex + ey * ey + ez * ez));  // (r - |e|)(r + |e|)
        const f3 e = p - cc;
        const float le = length(e);
        const f3 nu = e * rcp(le);
        p = p + nu * (dn * rcp(fabsf(cr.w) + le));
        nout = cr.w < 0.0f ? -nu : nu;
        eta = 0x1p-22f * (fabsf(p.x * nu.x) + fabsf(p.y * nu.y) + fabsf(p.z * nu.z));
      }
      mat = (int)fbits(mv.w);
      ff = dot(d, nout) < 0;  // setFaceNormal hittable.go:27-34
      n = ff ? nout : -nout;
      if (HAS(FT_IMAGE) && sc.mats[mat]._pad != 0.0f) {  // texture reads u,v: calculateSphereUV objects.go:44-50
        const F2 rs = sc.sph_uv[idx];
        f3 no = mk3(rs.x * nout.x - rs.y * nout.z, nout.y, rs.y * nout.x + rs.x * nout.z);
        float theta = acosf(-no.y);
        float phi = atan2f(-no.z, no.x) + kPi;
        u = phi * (0.5f * kInvPi);
        v = theta * kInvPi;
      }
    } else if (FT == 0u && (EARLY_SHAPE != 0 || sc.shade_lds >= 0)) {
      const F4* tab = g_dyn_lds + sc.shade_lds + 2 * idx;
      const F4 a = EARLY_SHAPE != 0 ? etab_a : ld_lds(tab), b = EARLY_SHAPE != 0 ? etab_b : ld_lds(tab + 1);
      lcol = xyz(b);
      nout = xyz(a);
      p = p - nout * (dot(nout, p) - b.w);  // onto the plane n.p = D (b.w, rt_render.hip)
      mat = (int)fbits(a.w);  // the material KIND here
      ltab = true;
      ff = dot(d, nout) < 0;
      n = ff ? nout : -nout;
    } else if (!HAS(FT_TRI | FT_MEDIA) || type == PRIM_QUAD) {
      const F4* q = sc.quad + 5 * (size_t)idx;
      nout = xyz(q[3]);
      p = p - nout * (dot(nout, p) - q[0].w);  // onto the plane n.p = D
      mat = (int)fbits(q[2].w);
      ff = dot(d, nout) < 0;
      n = ff ? nout : -nout;
      if (HAS(FT_BOX) && u < 0.0f) {
        // a box leaf's face (hit_box_rec): quad.Hit's alpha, beta (objects.go:186-187) at
        // this p, computed only when the material reads them (image textures)
        if (HAS(FT_IMAGE) && sc.mats[mat]._pad != 0.0f) {
          const f3 pp = p - xyz(q[0]), w = xyz(q[4]);
          u = dot(w, cross(pp, xyz(q[2])));
          v = dot(w, cross(xyz(q[1]), pp));
        } else {
          u = v = 0.0f;
        }
      }
    } else if (HAS(FT_TRI) && (!HAS(FT_MEDIA) || type == PRIM_TRI)) {
      nout = tri_normal(sc, idx, u, v);
      mat = (int)fbits(sc.tri[3 * (size_t)idx].w);
      ff = dot(d, nout) < 0;
      n = ff ? nout : -nout;
      uint32_t tf = fbits(sc.tri[3 * (size_t)idx + 2].w);
      if (tf & TRI_HAS_UV) {  // objects.go:437-446
        const F4* at = sc.tri_attr + 6 * (size_t)idx;
        float w = 1.0f - u - v;
        float tu = w * at[4].x + u * at[4].z + v * at[5].x;
        float tv = w * at[4].y + u * at[4].w + v * at[5].y;
        u = tu;
        v = tv;
      }
    } else {  // medium hit medium.go:162-166: normal (1,0,0), front face
      mat = sc.media[idx].phase_mat;
      n = mk3(1, 0, 0);
      ff = true;
      u = v = 0.0f;
    }
    if (ltab)
      M.kind = mat;
    else
      M = sc.mats[mat];
    if constexpr (EARLY_SHAPE == 0) scat = M.kind != RT_MAT_DIFFUSE_LIGHT;  // (early draw: the same, from bk)
  }
  // ONE Philox call per vertex for the whole wave: a scattering vertex draws its
  // own numbers; a path ending here (miss or light) draws the camera numbers of
  // the chunk's next sample (otherwise two divergent calls per iteration):
  // C2 +3 %, C3 +2 %.  The all-features kernel (3 waves/SIMD, register-bound)
  // keeps the two draws in their branches (merged there: C4 -3 %).
  constexpr bool kMergeDraws = FT != FT_ALL;
  static_assert(EARLY_SHAPE == 0 || kMergeDraws, "early draw: the vertex's one merged draw");
  if (kMergeDraws && EARLY_SHAPE == 0)
    r = rt_rng_draw(P.seed, s.gpix, s.s0 + s.j + (scat ? 0u : 1u),
                    scat ? RT_STREAM(s.k, 0) : RT_STREAM_CAMERA);
  if (!scat) {
    if (ref == PRIM_NONE)
      lterm = mk3(P.bg[0], P.bg[1], P.bg[2]);  // camera.go:300-302
    else  // Emitted materials.go:150-155; Scatter false
      lterm = ff ? (ltab ? lcol : tex_value<FT>(sc, M.tex, u, v, p)) : mk3(0, 0, 0);
    term = true;
    if (kMergeDraws) {
      rcam = r;
      have_rcam = true;
    }
  } else {
    if (!kMergeDraws) r = rt_rng_draw(P.seed, s.gpix, s.s0 + s.j, RT_STREAM(s.k, 0));
    {
      f3 ndir;
      bool clamp_vertex = false;
      f3 weight;
      if (HAS(FT_METAL) && M.kind == RT_MAT_METAL) {  // materials.go:70-79
        f3 refl = unit(reflect(d, n));
        ndir = refl + uniform_sphere(rt_unit_f(r.v[2]), rt_unit_f(r.v[3])) * M.param;
        weight = xyz(M.albedo);
      } else if (HAS(FT_DIEL) && M.kind == RT_MAT_DIELECTRIC) {  // materials.go:94-130
        float ior = M.param;
        float ri = ff ? rcp(ior) : ior;
        f3 ud = unit(d);
        float cs = fminf(dot(-ud, n), 1.0f);
        float sn = fsqrt(1.0f - cs * cs);
        bool cannot = ri * sn > 1.0f;
        bool refl = cannot;
        if (!cannot) {
          float r0 = (1.0f - ior) * rcp(1.0f + ior);
          r0 = r0 * r0;
          // Schlick's (1 - cos)^5 (materials.go:132-136, math.Pow) as three multiplies: the
          // library powf is ~40 instructions with its special-case selects; the product is
          // within a few ulp of it for the base in [0, 1]
          const float x = 1.0f - cs, x2 = x * x;
          float refl_p = r0 + (1.0f - r0) * (x2 * x2 * x);
          refl = refl_p > rt_unit_f(r.v[0]);
        }
        ndir = refl ? reflect(ud, n) : refract(ud, n, ri);
        weight = mk3(1, 1, 1);
      } else {  // lambertian materials.go:45-57 / isotropic :157-177 + mixture pdf.go:58-74
        const bool iso = HAS(FT_MEDIA) && M.kind == RT_MAT_ISOTROPIC;
        PH_T(t_tex);
        f3 att = ltab ? lcol : tex_value<FT>(sc, M.tex, u, v, p);
        PH_ADD(PH_TEX, t_tex);
        PH_T(t_light);
        // a lean light kind: the pdf part of the light block is asked for first
        LeanLightRegs lean;
        if constexpr (LIGHT != 0) lean = lean_light_load();
        Onb b;
        if (!iso) b = make_onb_unit(n);
        if (rt_unit_f(r.v[0]) < 0.5f) {
          if constexpr (LIGHT != 0) ndir = lean_light_random(lean, p, r);
          else ndir = lights_random<FT>(sc, p, r);
        } else if (iso) {
          ndir = uniform_sphere(rt_unit_f(r.v[2]), rt_unit_f(r.v[3]));
        } else {
          ndir = onb_transform(b, cosine_direction(rt_unit_f(r.v[2]), rt_unit_f(r.v[3])));
        }
        float bsdf_pdf, spdf;
        if (iso) {
          bsdf_pdf = 1.0f / (4.0f * kPi);
          spdf = 1.0f / (4.0f * kPi);
        } else {
          f3 ud = unit(ndir);
          bsdf_pdf = fmaxf(0.0f, dot(ud, b.w) * kInvPi);  // 1 ulp of /pi, no division sequence
          float ct = dot(n, ud);
          spdf = fmaxf(0.0f, ct * kInvPi);  // (kInvPi > 0: zero exactly when ct < 0)
        }
        float lpdf;
        if constexpr (LIGHT != 0) lpdf = lean_light_pdf<LIGHT>(lean, p, ndir);
        else lpdf = lights_pdf<FT>(sc, p, ndir);
        float pdf = 0.5f * lpdf + 0.5f * bsdf_pdf;
        PH_ADD(PH_LIGHT, t_light);
        // pdf >= 1e-30 when every light entry is a prim (sc.pdf_floor): a direction below
        // the surface (spdf = 0) whose light pdf test just misses the light's edge in fp32
        // (pdf = 0) weighs 0, not 0 * inf = NaN (camera.go:321-328 divides by the mixture
        // pdf; one sample in ~1e9 of C2 met this).  Any pdf > 1e-30 is untouched.  An empty
        // lights list's pdf is 0 by the reference's rules (hittable.go:89-103): its 0/0 NaNs
        // are the reference's own and stay (floor 0, test_world_without_lights_list).
        // (a lean light kind: the floor is 1e-30 by the host matcher)
        weight = (att * spdf) * rcp(fmaxf(pdf, LIGHT != 0 ? 1e-30f : sc.pdf_floor));
        clamp_vertex = true;
      }
      // vertex bookkeeping (H1: the clamp is folded backwards at termination)
      if (clamp_vertex) {
        if (s.flags & F_PEND) {
          const f3 pv = get_pend<SOA>(P, slot, s);
          // Dominated clamp vertices are merged, not pushed.  The fold needs
          // max_k I(P_k) over the suffix products P_k = w_k (.) P_k+1 (WStack::fold_max);
          // with 0 <= w_k <= 1 in every channel, I(P_k) <= I(P_k+1) whatever follows,
          // so vertex k never sets the scale and only its product matters: w_k is
          // multiplied into the entry below instead of taking a stack entry (the
          // bottom entry is still pushed: merging it into the camera-side prefix
          // `pre`, which the book2 kernel keeps in scratch, cost more than it saved).
          // Same folded value up to fp32 rounding; paths through the water orb and
          // the fog (book2, up to 40 isotropic vertices) keep most of their stack in LDS.
          // Needs P_k+1 >= 0 in every channel: scenes with a negative colour, albedo or
          // background (sc.merge_ok = 0) push every vertex, which the fold handles exactly
          // for any sign.
          // (the flag is re-read from the kernel-argument segment here, kparams(): held in
          // an SGPR across the loop it added SGPR spills)
          // (a lean light kind: set by the host matcher and kept by the launch, plan_kernel)
          const bool merge = (LIGHT != 0 || kparams()->sc.merge_ok) && s.nst > 0 && pv.x >= 0.0f && pv.y >= 0.0f &&
                             pv.z >= 0.0f && pv.x <= 1.0f && pv.y <= 1.0f && pv.z <= 1.0f;
          if (merge) {
            f3 top = ws.mul(P, slot, s.nst - 1, pv);
            // Kernels with media also cascade: the merged top may itself now be
            // dominated by the new clamp vertex (0 <= top <= 1), so it folds into the
            // entry below, and so on.  Book2's HBM pushes: 309 M -> 126 M (merge) ->
            // 19 M (cascade) at 400 x 400 x 1024; C4 -1.7 %, while the lean and mesh
            // kernels, whose stacks stay shallow, lost 0.6-1.4 % to the loop
            // (profiles/r3_weight_cascade_ab.jsonl).
            if (HAS(FT_MEDIA))
              while (s.nst >= 2 && top.x >= 0.0f && top.y >= 0.0f && top.z >= 0.0f &&
                     top.x <= 1.0f && top.y <= 1.0f && top.z <= 1.0f) {
                top = ws.mul(P, slot, s.nst - 2, top);
                --s.nst;
              }
          } else {
            ws.put(P, slot, s.nst, {pv.x, pv.y, pv.z, 0.0f});
            ++s.nst;
#ifdef RT_COUNT_PUSHES
            ++s.pushes;  // a per-lane counter costs the fused kernels a VGPR: opt-in
#endif
          }
        }
        set_pend<SOA>(P, slot, s, weight);
        s.flags |= F_PEND;
      } else if (s.flags & F_PEND) {
        set_pend<SOA>(P, slot, s, get_pend<SOA>(P, slot, s) * weight);
      } else {
        f3 w = (s.flags & F_PRE) ? get_pre<SOA>(P, slot, s) : mk3(1, 1, 1);
        set_pre<SOA>(P, slot, s, w * weight);
        s.flags |= F_PRE;
      }
      if (!finite3(weight)) s.flags |= F_NONFINITE;
      ++s.k;
      if ((int)s.k > P.max_depth) {  // rayColor(depth-1 < 0) == black, camera.go:294-296
        term = true;
        lterm = mk3(0, 0, 0);
      } else {
        // spheres: the new origin eta off the surface on the side the ray leaves to, so
        // the fp64 sphere test (exact for this fp32 point) sees it where the reference's
        // point is: outside for a ray leaving outward (no root ahead), inside for one
        // refracted or fuzz-reflected inward (the far root only).  eta = 0 elsewhere.
        if (HAS(FT_SPHERE)) p = p + n * copysignf(eta, dot(ndir, n));
        s.o = p;
        s.d = ndir;
        s.spare = rt_spare24(r);
        store_ray<SOA>(P, slot, s);
        return OUT_ALIVE;
      }
    }
  }
  // ---- termination: backward clamp fold (camera.go:316, :328-330)
  PH_T(t_term);
  f3 L = lterm;
  const bool zero = lterm.x == 0.0f && lterm.y == 0.0f && lterm.z == 0.0f;
  if (!(zero && !(s.flags & F_NONFINITE))) {
    float maxI = 0.0f;  // no clamp vertex: no scale
    if (s.flags & F_PEND) {
      L = get_pend<SOA>(P, slot, s) * L;
      maxI = L.x + L.y + L.z;
      ws.fold_max(P, slot, s.nst, L, maxI);
    }
    // min(1, M / maxI) as one v_min: no compare and three v_cndmask_b32_e32 (and_not); the
    // scale is exactly 1 whenever M * rcp(maxI) >= 1 (maxI below M by more than an ulp)
    L = L * fminf(1.0f, P.maxc * rcp(maxI));
    if (s.flags & F_PRE) L = get_pre<SOA>(P, slot, s) * L;
  } else {
    L = mk3(0, 0, 0);
  }
#ifdef RT_NAN_DEBUG
  if (isnan(L.x) || isnan(L.y) || isnan(L.z)) printf("NAN gpix %u sample %u\n", s.gpix, s.s0 + s.j);
#endif
  sa.add(P, s.chunk, L);
  const uint32_t count = s.flags >> kCountShift;  // chunk_ids().count, or a drain split's
  if (s.j + 1 < count) {
    if (!have_rcam)  // a miss, or the depth limit: the camera draw is made here
      rcam = rt_rng_draw(P.seed, s.gpix, s.s0 + s.j + 1, RT_STREAM_CAMERA);
    next_sample<SOA, cam_mode(FT)>(P, slot, s, s.j + 1, rcam);
    PH_ADD(PH_TERM, t_term);
    return OUT_ALIVE;
  }
  sa.flush(P, s.chunk, (s.flags & F_SPLIT) != 0u);
  PH_ADD(PH_TERM, t_term);
  return OUT_NEED_CHUNK;
}

// the n-th (from 0) set bit of m, n < popcount(m)
RT_D uint32_t nth_set_bit(unsigned long long m, uint32_t n) {
  uint32_t pos = 0u;
#pragma unroll
  for (uint32_t w = 32u; w > 0u; w >>= 1) {
    const uint32_t lo = (uint32_t)__popcll(m & ((1ull << w) - 1ull));
    if (n >= lo) {
      n -= lo;
      m >>= w;
      pos += w;
    }
  }
  return pos;
}

// Drain of the fused kernel (every chunk handed out, wave-uniform call): the k-th lane
// without work takes the upper half of the samples left in the k-th lane that has at least
// P.split_min left after its current one.  Samples are keyed by (pixel, sample) and summed
// exactly, so who traces them does not change the image; the taker's sums go to the pixel
// with atomics (F_SPLIT), the giver's chunk record covers the samples it kept.  A taker gets
// the giver's chunk in `c`, its samples [j0, n0) of it (j0 >= 1), for start_sample.  A giver
// may be a taker or have given before: the count it passes on is its current one.
RT_D void split_samples(const Params& P, Path& s, bool has, uint32_t& c, uint32_t& j0,
                        uint32_t& n0) {
  const uint32_t cnt = s.flags >> kCountShift;
  const uint32_t left = has ? cnt - 1u - s.j : 0u;
  const bool giver = left >= kparams()->split_min;
  const unsigned long long need = __ballot(!has && c == 0xFFFFFFFFu), give = __ballot(giver);
  if (!need || !give) return;
  const uint32_t n_need = (uint32_t)__popcll(need), n_give = (uint32_t)__popcll(give);
  const bool needs = ((need >> lane_id()) & 1ull) != 0ull;
  const uint32_t rank = prefix_count(needs ? need : give);
  const bool taker = needs && rank < n_give;
  const uint32_t keep = cnt - ((left + 1u) >> 1);  // the giver's new sample count
  const uint32_t src = taker ? nth_set_bit(give, rank) : lane_id();
  const uint32_t t_chunk = __shfl(s.chunk, (int)src), t_keep = __shfl(keep, (int)src),
                 t_cnt = __shfl(cnt, (int)src);
  if (giver && rank < n_need) s.flags = (s.flags & ((1u << kCountShift) - 1u)) | (keep << kCountShift);
  if (taker) {
    c = t_chunk;
    j0 = t_keep;
    n0 = t_cnt;
  }
}

// Wave-batched work distribution over partitioned counters.  The chunk range is split
// into NP = 2^parts_log2 partitions, interleaved in granules of G = 2^gran_log2 chunks
// (granule j belongs to partition j % NP), each with its own counter of positions
// (Counters::part, 256 B apart).  Every partition therefore sweeps the image in the same
// order as one counter would (the row-group locality of chunk_pixel is kept), while the
// returning atomics are spread over NP addresses: one address saturates near 88
// returning atomics per µs on MI355X, which is what forced large batches (and the long
// tail they leave when the range runs out) on a single counter.  A wave starts on
// partition (wave id % NP); when its partition is used up it probes every counter with
// one load per lane and moves to the next one with work left.  Partitions whose atomic
// came back exhausted are remembered (`dead`), so the search ends after at most NP + 1
// atomics even on stale probes.  Lanes that need a chunk take consecutive positions from
// the wave's batch; the batch is refilled with ONE returning atomic per >= grab_min
// positions.  parts_log2 = 0 is the single counter (progress slices use it).
struct WaveBatch {
  uint32_t next, end;   // wave-uniform: positions [next, end) of partition `part`
  uint32_t part;        // the wave's partition; kMaxParts once every partition is used up
  unsigned long long dead;  // partitions known exhausted
};
RT_D uint32_t part_end(const Params& P, uint32_t p) {
  const uint32_t gl = P.gran_log2, lg = P.parts_log2;
  const uint32_t granules = (P.n_chunks + (1u << gl) - 1u) >> gl;
  return granules > p ? (((granules - p - 1u) >> lg) + 1u) << gl : 0u;
}
RT_D uint32_t part_chunk(const Params& P, uint32_t p, uint32_t pos) {
  const uint32_t gl = P.gran_log2;
  return ((((pos >> gl) << P.parts_log2) + p) << gl) | (pos & ((1u << gl) - 1u));
}
RT_D WaveBatch batch_init(const Params& P) {
  // wave-uniform (readfirstlane): the batch lives in SGPRs, not in VGPRs of every lane
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  return {0u, 0u, wave & ((1u << P.parts_log2) - 1u), 0ull};
}
RT_D uint32_t grab_chunk(const Params& P, WaveBatch& b, bool need) {
  const unsigned long long m = __ballot(need);
  if (!m) return 0xFFFFFFFFu;
  const uint32_t n = (uint32_t)__popcll(m);
  const uint32_t r = prefix_count(m);
  const uint32_t avail = b.end - b.next;
  // per lane only the chunk id: positions are mapped with the (uniform) partition of
  // the batch they come from, so no per-lane partition or position stays live
  uint32_t c = r < avail && b.part < (uint32_t)kMaxParts ? part_chunk(P, b.part, b.next + r)
                                                         : 0xFFFFFFFFu;
  if (n <= avail) {
    b.next = __builtin_amdgcn_readfirstlane(b.next + n);
  } else {
    const uint32_t leader = (uint32_t)(__ffsll((long long)m) - 1);
    const uint32_t np = 1u << P.parts_log2;
    uint32_t g = 0u, gend = 0u;
    // a wave-uniform loop: each pass either takes a batch, finds every partition used
    // up, or marks one more partition dead (at most NP + 1 passes)
    while (b.part < (uint32_t)kMaxParts) {
      const uint32_t endp = part_end(P, b.part);
      const uint32_t want = max(P.grab_min, n - avail);
      uint32_t v = 0u;
      if (lane_id() == leader) v = atomicAdd(&P.ctr->part[b.part * kPartStride], want);
      g = __builtin_amdgcn_readlane(v, leader);
      if (g < endp) {
        gend = min(g + want, endp);
        break;
      }
      b.dead |= 1ull << b.part;
      // probe: lane i reads partition i's counter (stale values only read low)
      const uint32_t li = lane_id();
      bool left = false;
      if (li < np)
        left = __hip_atomic_load(&P.ctr->part[li * kPartStride], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) < part_end(P, li);
      const unsigned long long live = __ballot(left) & ~b.dead;
      if (!live) {
        b.part = (uint32_t)kMaxParts;
        break;
      }
      // the next live partition after this one, cyclically
      const uint32_t sh = b.part + 1u;
      const unsigned long long rot = sh >= 64u ? live : ((live >> sh) | (live << (64u - sh)));
      b.part = __builtin_amdgcn_readfirstlane((sh + (uint32_t)(__ffsll((long long)rot) - 1)) & 63u);
    }
    const uint32_t take = r - avail;  // this lane's offset in the new batch (r >= avail)
    if (r >= avail)
      c = b.part < (uint32_t)kMaxParts && g + take < gend ? part_chunk(P, b.part, g + take)
                                                          : 0xFFFFFFFFu;
    b.next = __builtin_amdgcn_readfirstlane(min(g + (n - avail), gend));
    b.end = __builtin_amdgcn_readfirstlane(gend);
  }
  if (!need) return 0xFFFFFFFFu;
  return c < P.n_chunks ? c : 0xFFFFFFFFu;
}

}  // namespace rt
