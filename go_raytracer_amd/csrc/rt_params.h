// rt_params.h — what every device layer of the path tracer starts from: the kernels'
// constants and path flags, the queue counters, the launch parameters (Params) and their
// re-read through the scalar cache (kparams), the address-space-typed loads and stores,
// the bit and lane helpers, and the phase probes of the RT_PHASES debug build.
#pragma once
#include "rt_kernels.h"

namespace rt {

constexpr int kLdsNodes = 384;   // 64-B slots staged in LDS per workgroup (24 KB): BVH nodes,
                                 // then the leaf records when both fit (LDS instantiation)
constexpr int kLdsWMax = 6;      // clamp-weight stack entries per lane kept in LDS (fused, max)
constexpr int kStack = 64;       // traversal stack entries per lane (LDS short stack + HBM overflow)
constexpr int kShortStack = 12;  // LDS entries per lane (column layout: [entry][thread])
constexpr int kShortStackMin = 6;  // smallest short stack of any kernel (fused lean set)
constexpr int kMaxIt = 1 << 16;  // per-iteration counter slots (no per-iteration memsets)
constexpr int kXcd = 8;          // queue counters are sharded per XCD (blockIdx % 8)
constexpr int kMaxParts = 64;    // chunk-range partitions of the fused kernel (one counter each)
constexpr int kPartStride = 64;  // u32 between partition counters (256 B: own cache lines)

enum : uint32_t { F_PEND = 1u, F_PRE = 2u, F_NONFINITE = 4u };
// Path::flags above this bit: the sample count of the path's chunk (chunk_ids().count, set
// when the chunk starts), so the per-sample "last sample?" test needs no launch parameter
constexpr uint32_t kCountShift = 8;
// Path::flags bit 7 (kept by next_sample): the path runs samples split off another lane's
// chunk (k_fused's drain, split_samples); its sums go to the pixel with atomics, not to the
// chunk's record
constexpr uint32_t F_SPLIT = 0x80u;

enum { OUT_DEAD = 0, OUT_ALIVE = 1, OUT_NEED_CHUNK = 2 };

struct Counters {
  unsigned long long segments;
  unsigned long long pushes;
  unsigned long long overflow;  // samples whose channel left the fixed-point range (add_sample)
  uint32_t chunk_head;
  uint32_t _pad[11];
  uint32_t part[kMaxParts * kPartStride];  // fused kernel: next position of partition p at [p * stride]
  uint32_t cnt[kMaxIt][kXcd];  // per-XCD queue lengths entering iteration i
};

// Division by a launch-invariant divisor: q = (t + ((n - t) >> s1)) >> s2 with
// t = mulhi(m, n) (round-up magic, exact for all 32-bit n and d >= 1; host side
// make_fastdiv in rt_render.hip; Hacker's Delight 10-8 with the add fix-up).
struct FastDiv {
  uint32_t m, s1, s2, d;
};
RT_D uint32_t fdiv(uint32_t n, const FastDiv& f) {
  const uint32_t t = __umulhi(f.m, n);
  return (t + ((n - t) >> f.s1)) >> f.s2;
}

struct Params {
  DevScene sc;
  FastDiv fd_width, fd_s;
  FastDiv fd_gchunks, fd_gpix;  // chunk order: groups of fd_gpix.d pixels x all sample blocks
  FastDiv fd_gchunks2;          // the tail phase's chunks per group (gpix x its blocks)
#ifdef RT_SWEEP_ORDER
  uint32_t gflip, gbase;        // group at sweep position q: (q ^ gflip) + gbase (0, 0: image
                                // order; ~0, groups: reversed, RT_SWEEP) -- and back (k_resolve)
#endif
  // camera (initialize camera.go:179-253, converted to fp32)
  float p00r[3], du[3], dv[3], cc[3], dku[3], dkv[3];  // p00r = pixel00 - center
  float bg[3];
  float recip_s, maxc;
  int s, defocus, max_depth;
  int width, rank, nranks;
  uint32_t npix;       // pixels of this rank
  uint32_t K;          // samples per chunk (first phase)
  uint32_t K2;         // samples per chunk of the tail phase (chunk ids >= n1)
  uint32_t S1;         // samples [0, S1) of every pixel in the first phase, [S1, ss) in the tail
  uint32_t n1;         // chunks of the first phase (npix * S1 / K)
  uint32_t n_chunks;
  uint32_t P;          // path slots (stack column count)
  uint32_t ss;         // s*s
  int step_budget;     // fused: traversal steps per scheduling round
  uint32_t shade_min;  // fused: lanes that must be waiting before a wave shades
  uint32_t grab_min;   // fused: chunks a wave takes per refill of its batch (>= 1)
  uint32_t parts_log2; // fused: the chunk range is split over 2^parts_log2 partitions ...
  uint32_t gran_log2;  // ... interleaved in granules of 2^gran_log2 chunks (grab_chunk)
  uint32_t split_min;  // fused drain: a lane with >= split_min samples left shares them (0: off)
  unsigned long long* wave_times;  // debug (RT_WAVE_TIMES): per wave {start, end, segments}
  uint32_t recs_lds;   // leaf records cached in LDS after the nodes (stage_nodes)
  uint64_t seed;
  // wavefront state (SoA, slot-indexed)
  F4* ray_o;   // origin | time
  F4* ray_d;   // direction | 0
  F4* hit;     // t, u, v, prim ref bits
  uint2* path; // chunk, packed(j:12 | vertex:8 | nstack:8 | flags:4)
  F4* pend;    // pending clamp-vertex weight (top of the weight stack)
  F4* pre;     // camera-side product of specular attenuations
  F4* stack;   // [vertex][slot] clamp-vertex weights spilled to HBM
  uint32_t* queue[2];  // each kXcd segments of P entries
  Counters* ctr;
  unsigned long long* accum;  // 3 planes x npix: per-sample fixed point 2^-32, summed exactly
  unsigned long long* csum;   // fused: per-chunk sums, 4 x u64 per chunk id (x, y, z, 0), each
                              // stored once by the lane that ran the chunk (SampleAcc::flush);
                              // k_resolve adds a pixel's chunks.  Null: atomics into accum
  double* side;               // 3 planes x npix: samples outside the fixed-point range (fp64)
  float vlim;                 // fixed-point range per sample: |v| < 2^31 / ss (no int64 wrap)
  uint32_t* pflags;           // per pixel NaN (bits 0-2) / +Inf (bits 3-5) / -Inf (bits 6-8)
  uint32_t* ostack;            // traversal-stack overflow [kStack - kShortStackMin][stack_cols]
  uint32_t stack_cols;         // = launched threads of the traversal kernel
  F4* trace;                  // debug path trace (3 F4 per vertex) or null
  uint32_t trace_gpix, trace_sample;
  int trace_cap;
  LeanLight ll;               // the light of a lean light kind's kernel (rt_device.h; set only
                              // for a launch of such a kernel, read by it alone)
  const uint32_t* pixmap;     // an active-pixel pass (k_fused<.., MAP>): local pixel
                              // lv of the pass stands for the share's local pixel pixmap[lv]
                              // (sorted, npix entries); null otherwise, read by MAP kernels alone
};

RT_D uint32_t pack_path(uint32_t j, uint32_t k, uint32_t nst, uint32_t flags) {
  return (j & 0xFFFu) | ((k & 0xFFu) << 12) | ((nst & 0xFFu) << 20) | ((flags & 0xFu) << 28);
}

// address-space-typed loads and stores (see trace_world's note)
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(1))) uint32_t glb_u32;
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4f lds_v4;
typedef __attribute__((address_space(1))) v4f glb_v4;
typedef float v2f __attribute__((ext_vector_type(2)));
// 16 B from a wave-uniform address through the scalar cache (s_load into SGPRs):
// for tables indexed by a loop counter or a broadcast index
RT_D F4 ld_cst(const F4* p) {
  typedef __attribute__((address_space(4))) const v4f cst_v4;
  const v4f v = *(const cst_v4*)p;
  return {v.x, v.y, v.z, v.w};
}
RT_D F4 ld_lds(const F4* p) {
  const v4f v = *(const lds_v4*)p;
  return {v.x, v.y, v.z, v.w};
}
RT_D F4 ld_glb(const F4* p) {
  const v4f v = *(const glb_v4*)p;
  return {v.x, v.y, v.z, v.w};
}
RT_D void st_lds(F4* p, F4 v) { *(lds_v4*)p = v4f{v.x, v.y, v.z, v.w}; }
// s_waitcnt vmcnt(0) (gfx9 encoding: expcnt/lgkmcnt left unconstrained).  Placed
// at the end of a RARE global-memory branch whose result merges with an LDS
// branch: without it the compiler's wait lands after the merge, on the common
// LDS path too, where it drains every outstanding store and atomic.
RT_D void wait_vm() { __builtin_amdgcn_s_waitcnt(0x0F70); }
RT_D void st_glb(F4* p, F4 v) { *(glb_v4*)p = v4f{v.x, v.y, v.z, v.w}; }

// m ? b : a, bitwise (v_bitop3_b32, truth table 0xD8 over (a, b, m)).  With m a sign mask
// this is a select in one full-rate instruction: hipcc turns the same C expression into
// v_cmp + v_cndmask, both of which issue at half rate or less on gfx950
// (profiles/r4_instr_rate.jsonl)
RT_D uint32_t pick_by(uint32_t a, uint32_t b, uint32_t m) { return __builtin_amdgcn_bitop3_b32(a, b, m, 0xD8); }
// a & ~m as one v_bitop3 (written as `a & ~m` with m a spread sign, LLVM turns it into a
// compare and a v_cndmask_b32_e32 on vcc, which issues at ~23 cycles per wave64 on gfx950
// whatever the occupancy: tools/instr_rate.hip, profiles/r6_instr_rate.jsonl)
RT_D uint32_t and_not(uint32_t a, uint32_t m) { return __builtin_amdgcn_bitop3_b32(a, m, 0u, 0x30); }
// all ones when x < 0 (sign bit set), else 0: -0 and negative NaNs count as negative
RT_D uint32_t neg_mask(float x) { return (uint32_t)((int32_t)__float_as_uint(x) >> 31); }
RT_D uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// Debug build (-DRT_PHASES, tools/phase_probe.py): shader-clock cycles each wave
// spends per phase of the fused loop, accumulated by lane 0 in LDS and written with
// the RT_WAVE_TIMES record.  Timing perturbs the kernel (s_memtime waits): use the
// shares, not the absolute cycles.
enum { PH_GRAB, PH_TRAV, PH_MEDIA, PH_SHADE, PH_TEX, PH_LIGHT, PH_TERM, PH_LOOP,
       PH_TRAV_LANES, PH_TRAV_ROUNDS, PH_SHADE_LANES, PH_SHADE_ROUNDS, PH_STEP_LANES,
       PH_STEP_WAVE, PH_QNODE_LANES, PH_QLEAF_LANES, PH_QMIXED, PH_QITERS,
       // compressed-BVH steps: lanes on the first active lane's item, distinct items per
       // iteration, and lanes on items of BFS levels 0-3 (item < 85) / 4-5 (item < 1365)
       PH_QSAME, PH_QUNIQ, PH_QTOP, PH_QMID, PH_N = 22 };
constexpr int kWaveRec = 4 + PH_N;  // {start, end, segments, pad, phases...} per wave
#ifdef RT_PHASES
__shared__ unsigned long long g_ph[4][PH_N];
RT_D unsigned long long ph_now() { return __builtin_readcyclecounter(); }
RT_D void ph_acc(int i, unsigned long long v) {  // first active lane (divergent code too)
  if (lane_id() == (uint32_t)(__ffsll((long long)__ballot(1)) - 1)) g_ph[threadIdx.x >> 6][i] += v;
}
#define PH_T(v) const unsigned long long v = ::rt::ph_now()
#define PH_ADD(i, v) ::rt::ph_acc(i, ::rt::ph_now() - (v))
#define PH_CNT(i, n) ::rt::ph_acc(i, (unsigned long long)(n))
// traversal steps: summed over the lanes, and the wave's maximum (loop trips)
RT_D void ph_steps(int n) {
  atomicAdd(&g_ph[threadIdx.x >> 6][PH_STEP_LANES], (unsigned long long)n);
  int m = n;
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
  ph_acc(PH_STEP_WAVE, (unsigned long long)m);
}
#else
#define PH_T(v)
#define PH_ADD(i, v)
#define PH_CNT(i, n)
#endif
RT_D uint32_t prefix_count(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
RT_D uint32_t wave_uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

typedef __attribute__((address_space(4))) const Params cst_params;
// The launch parameters re-read through the scalar cache where they are used: the asm
// barrier hides that the pointer is the kernel-argument segment's, so the compiler
// cannot hoist the loads to the kernel entry and hold the values in SGPRs across the
// whole loop (where they spill to VGPR lanes).
RT_D const cst_params* kparams() {
  const cst_params* p = (const cst_params*)__builtin_amdgcn_kernarg_segment_ptr();
  __asm__ volatile("" : "+s"(p));
  return p;
}

}  // namespace rt
