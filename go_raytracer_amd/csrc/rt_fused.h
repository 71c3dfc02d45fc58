// rt_fused.h — the fused persistent kernel k_fused and the device helpers it shares with
// the wavefront kernels (stage_nodes, finish_hit).  A header so that kernel instantiations
// can be compiled in their own translation units with their own code-generation flags
// (rt_fused_sets.hip: the scheduler strategy per kernel); rt_render.hip holds the rest.
#pragma once
#include "rt_device.h"
// (RT_FUSED_TABLE_ONLY: the kernel table at the end alone, for tools/fused_dispatch.cpp, which
// runs the dispatcher over stand-in kernels on the host)
#ifndef RT_FUSED_TABLE_ONLY
#include "rt_path.h"

namespace rt {

// the whole node array (W F4 per node) -> LDS (only used when it fits in
// kLdsNodes 64-B slots), then the leaf records when they fit too
RT_D bool stage_nodes(const Params& P, F4* lnodes, int W) {
  const int nl = min(P.sc.n_nodes, 4 * kLdsNodes / W);
  for (int i = threadIdx.x; i < W * nl; i += blockDim.x) lnodes[i] = P.sc.nodes[i];
  const bool recs = P.recs_lds != 0u;
  if (recs) {
    // + the lean set's shade table after the record pairs (rt_render.hip)
    const int n = 4 * P.sc.n_refs + (P.sc.shade_lds >= 0 ? P.sc.shade_n : 0);
    for (int i = threadIdx.x; i < n; i += blockDim.x) lnodes[W * nl + i] = P.sc.leafprims[i];
  }
  __syncthreads();
  return recs;
}

// media + debug trace on top of the world closest hit, camera.go:300
template <uint32_t FT>
RT_D void finish_hit(const Params& P, const Path& s, Hit& best) {
  if (HAS(FT_TRI) && best.ref != PRIM_NONE && (best.ref >> 30) == PRIM_TRI)
    refine_tri_hit(P.sc, best.ref & 0x3FFFFFFFu, s.o, s.d, best.t, best.u, best.v);
  if (HAS(FT_MEDIA) && P.sc.n_media > 0)
    trace_media(P, s.o, s.d, s.time, 0.001f, s.gpix, s.s0 + s.j, s.k, s.spare, best);
  if (P.trace) record_trace(P, s, best);
}

// ----------------------------------------------------------------- fused ---
// FT = compiled-in scene features (rt_device.h), chosen per scene by pick_fused (rt_fused_pick.h).
// Waves per SIMD by feature set: the lean sets fit more waves in the register
// file (VGPRs <= 512 / waves) and in LDS (24 KB static + the scene cache).
#ifndef MESH_WAVES
#define MESH_WAVES 4
#endif
#ifndef TRI_WAVES
#define TRI_WAVES 4
#endif
#ifndef TRI_QWAVES
// the {sphere, triangle, metal} set (C5) on the compressed BVH4 at 5 waves per SIMD (round
// 5): that kernel needs 113 VGPRs at 4, and 5 waves (96 VGPRs, 1 spilled with the default
// scheduler; 13 LDS stack entries, TRI_QSHORT, so five blocks fit the CU's LDS) measured C5 -3.8 %
// (profiles/r5_c4_c5_isolation_ab.jsonl); round 2's 5-wave try of the 128-B-node kernel
// spilled 32 VGPRs in the traversal loop and lost 24 %
#define TRI_QWAVES 5
#endif
#ifndef TRI_QSHORT
// 13 LDS traversal-stack entries fill five blocks' LDS (5 x 31,776 B of 160 KiB): C5 -1.5 %,
// C3 -0.3 % against 12, 10 +4.5 % (profiles/r5_qshort_ab.jsonl)
#define TRI_QSHORT 13
#endif
#ifndef MESH_QWAVES
// book1's set (C3) on the compressed BVH4 at 5 waves too (96 VGPRs, 1 spilled with the default
// scheduler, 13 LDS stack entries): C3 -1.2 % with the ILP scheduler's 26 spills
// (profiles/r5_waves5_ab.jsonl), -5.5 % more without them; book2's set at 5 waves lost 3 %
// (31 spilled), it stays at 4
#define MESH_QWAVES 5
#endif
#ifndef MESH_QSHORT
#define MESH_QSHORT 13
#endif
#ifndef FT_TEX_WAVES
#define FT_TEX_WAVES 4
#endif
#ifndef BRUTE_WAVES
#define BRUTE_WAVES 6
#endif
// The record-loop kernels (TREE 0) need no traversal stack: kBruteWaves.
constexpr int kBruteWaves = BRUTE_WAVES;
constexpr int fused_waves(uint32_t ft, int tree = 4) {
  return (tree == 0 && ft == 0u) ? kBruteWaves  // 7 measured within noise of 6, 8 -3 %
         : ft == 0u ? 6
         : ft == FT_MEDIA ? 4
         : ft == (FT_SPHERE | FT_TRI | FT_METAL) ? (tree == 5 ? TRI_QWAVES : TRI_WAVES)
         : ft == (FT_SPHERE | FT_TRI | FT_METAL | FT_DIEL | FT_CHECKER) ? (tree == 5 ? MESH_QWAVES : MESH_WAVES)
         : ft == FT_SET_BOOK2 ? FT_TEX_WAVES
                                                                                  : 3;
}
// LDS clamp-weight entries (12 B each): 6 (C2 +1 %, C3 +2.5 % over 3-4), 4 for the
// mesh set, whose specular paths rarely push weights (C5 -1.5 % with 6), and 4 for
// the lean set's tree kernels (their stack + sums must fit 6 waves/SIMD)
#ifndef MESH_WLDS
#define MESH_WLDS 4
#endif
#ifndef MESH_SHORT
#define MESH_SHORT 16  // C5's 1M-triangle tree: -1.3 % against 12 (r2_mesh_short_ab.jsonl)
#endif
#ifndef TRI_SHORT
#define TRI_SHORT MESH_SHORT  // the {sphere, triangle, metal} set (C5)
#endif
#ifndef TRI_WLDS
#define TRI_WLDS MESH_WLDS
#endif
#ifndef TEX_SHORT
// book2's set: 10 traversal-stack and 5 weight entries fill its 4-wave LDS budget with the
// staged perlin tables (C4 -0.8 % against 13 x 4, +2 % at 7 x 6 on the compressed BVH4,
// profiles/r5_c4_stack_split_ab.jsonl; round 3 on the 128-B nodes: 16 x 3 / 18 x 2 / 21 x 1
// +0.6 to +1.7 % against 13 x 4, r3_tex_stack_ab.jsonl)
#define TEX_SHORT 10
#endif
#ifndef TEX_WLDS
#define TEX_WLDS 5
#endif
#ifndef ALL_WLDS
#define ALL_WLDS 4  // 6 pushed the C3-size trees out of the 3-wave LDS budget
#endif
#ifndef BRUTE_WLDS
#define BRUTE_WLDS kLdsWMax
#endif
constexpr int fused_wlds(uint32_t ft, int tree = 4) {
  return ft == (FT_SPHERE | FT_TRI | FT_METAL | FT_DIEL | FT_CHECKER) ? MESH_WLDS
         : ft == (FT_SPHERE | FT_TRI | FT_METAL)                    ? TRI_WLDS
         : (ft == 0u && tree != 0)                                  ? 4
         : (ft == 0u && tree == 0)                                  ? BRUTE_WLDS
         : ft == FT_ALL                                             ? ALL_WLDS
         : ft == FT_SET_BOOK2 ? TEX_WLDS
                                                                    : kLdsWMax;
}
// short traversal stack: none for the record loop, 6 entries for the lean set
// (tiny trees; its LDS budget at 6 waves/SIMD), 12 elsewhere; deeper ones in HBM
constexpr int fused_short(uint32_t ft, int tree = 4) {
  return tree == 0                                                    ? 0
         : ft == 0u                                                   ? kShortStackMin
         : ft == (FT_SPHERE | FT_TRI | FT_METAL | FT_DIEL | FT_CHECKER) ? (tree == 5 ? MESH_QSHORT : MESH_SHORT)
         : ft == (FT_SPHERE | FT_TRI | FT_METAL)                      ? (tree == 5 ? TRI_QSHORT : TRI_SHORT)
         : ft == FT_SET_BOOK2 ? TEX_SHORT
                                                                      : kShortStack;
}
// + 24 B per lane of chunk sums (SampleAcc) + the perlin tables of noise kernels
constexpr unsigned fused_static_lds(uint32_t ft, int tree = 4) {
  return (unsigned)(fused_short(ft, tree) * 4 + fused_wlds(ft, tree) * 12 + 24) * 256u +
         ((ft & FT_NOISE) ? 256u * 16u + 768u : 0u);
}
__shared__ unsigned long long g_tstart[4];  // per wave: k_fused's start time (RT_WAVE_TIMES)
#ifdef RT_DRAIN_TIMES
__shared__ unsigned long long g_tdrain[4];  // debug builds: when the wave's grab came back empty
__shared__ unsigned long long g_dinfo[4][3];  // ... and then: samples left, busy lanes, segments
#endif
// TREE: 4 = BVH4, 5 = compressed BVH4 (64-B nodes, global only), 2 = BVH2, 0 = no tree
// (every record tested, tiny scenes).  SHAPE (TREE 0, FT 0, LDS only): the record layout the
// loop is compiled for (rt_device.h brute_shape), 0 = any.  LIGHT (the same kernels only): the
// lean light kind the light sampling and light pdf are compiled for (rt_device.h), 0 = any list.
// MAP: an active-pixel pass over the pixels listed in P.pixmap (chunk_ids; rt_fused_map.hip)
// EARLY (a listed SHAPE with a lean light kind only; the kernel table has it for shape 1): the vertex's
// Philox draw is issued before the record loop's winner is resolved (rt_path.h shade_core);
// P.ll.f[11] is the emitter slot (rt_device.h LeanLight)
// COST (the early-draw kernel only; RT_LEAN_COST=0 takes its COST = false twin): the per-round
// path without the tree scheduler's state (below), DESIGN.md §4 "The round without the tree
// scheduler's state".  The same operations on the same operands: the same image, segments and
// samples bit for bit.
template <bool LDS, uint32_t FT, int TREE, int SHAPE = 0, int LIGHT = 0, bool MAP = false, bool EARLY = false,
          bool COST = false>
__global__ __launch_bounds__(256, fused_waves(FT, TREE)) void k_fused(Params P) {
  static_assert(!EARLY || (SHAPE != 0 && LIGHT != 0 && !MAP), "early draw: a listed shape with a lean light kind");
  static_assert(!COST || (EARLY && TREE == 0), "lean cost cuts: the early-draw record-loop kernel only");
  static_assert(SHAPE == 0 || (LDS && FT == 0u && TREE == 0), "shapes: the lean LDS record loop only");
  static_assert(LIGHT == 0 || (LDS && FT == 0u && TREE == 0), "light kinds: the lean LDS record loop only");
  static_assert(LIGHT >= 0 && LIGHT < kLeanLightCount, "light kinds: unlisted kind");
  extern __shared__ F4 lnodes[];  // LDS scene cache, sized at launch (scene_lds_bytes)
  __shared__ uint32_t lstack[(fused_short(FT, TREE) > 0 ? fused_short(FT, TREE) : 1) * 256];
  __shared__ float lw[3 * fused_wlds(FT, TREE) * 256];
  __shared__ unsigned long long lacc[3 * 256];  // per-lane chunk sums (SampleAcc)
  for (int ch = 0; ch < 3; ++ch) lacc[ch * 256 + threadIdx.x] = 0ull;
  if constexpr (HAS(FT_NOISE)) stage_perlin(P.sc);  // before stage_nodes' barrier
  if constexpr (cam_mode(FT) == 1) stage_camera(P);
  const bool recs_lds = LDS && TREE != 8 && stage_nodes(P, lnodes, TREE == 4 ? 8 : 4);
  if (!LDS) __syncthreads();  // staged tables visible to every wave (stage_nodes ends with one)
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;  // weight-stack column
  const TravStack ts = {&lstack[threadIdx.x], P.ostack + slot, P.stack_cols, fused_short(FT, TREE)};
  const WStack ws = {&lw[threadIdx.x], fused_wlds(FT, TREE)};
  const SampleAcc sa = {&lacc[threadIdx.x]};
  Path s;
  s.pushes = 0;
  s.chunk = s.j = 0u;  // read by split_samples before a lane's first chunk
  s.flags = 0u;
  s.segs = 0;
  Trav tr;
  tr.cur = TRAV_DONE;
  bool has = false;
  WaveBatch b = batch_init(P);
  // debug (RT_WAVE_TIMES): the wave's start time parks in LDS (a register held across the
  // loop for this was the record-loop kernel's one spilled VGPR)
  // (the record-loop kernel keeps the wave's index in an SGPR: threadIdx.x >> 6 kept to the
  // end took its one spilled VGPR; the compressed-BVH kernels spill two more VGPRs that way)
  const uint32_t wave_in_group = (FT == 0u && TREE == 0) ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)
                                                         : threadIdx.x >> 6;
  if (P.wave_times && lane_id() == 0u) g_tstart[wave_in_group] = wall_clock64();
#ifdef RT_DRAIN_TIMES
  if (lane_id() == 0u) g_tdrain[wave_in_group] = 0ull;
#endif
  // Scheduling round: lanes without work take a chunk; traversing lanes run up
  // to step_budget traversal steps; lanes whose traversal is done are shaded
  // together once at least shade_min of them wait (or nothing else traverses),
  // so traversal divergence costs idle lanes only until the next round.
#ifdef RT_PHASES
  if (threadIdx.x < 4 * PH_N) (&g_ph[0][0])[threadIdx.x] = 0ull;
  __syncthreads();
#endif
  PH_T(t_loop);
  for (;;) {
    PH_T(t_grab);
    uint32_t c = grab_chunk(P, b, !has), j0 = 0u, n0 = 0u;
    // lanes share samples in the drain (split_samples), in every kernel: measured against
    // the record-loop kernel alone, profiles/r4_split_trees_ab.jsonl
    if (b.part >= (uint32_t)kMaxParts) split_samples(P, s, has, c, j0, n0);
    if (c != 0xFFFFFFFFu) {
      start_sample<false, cam_mode(FT), FT == 0u && TREE == 0, MAP>(P, slot, s, c, j0);
      if (j0) s.flags = F_SPLIT | (n0 << kCountShift);
      if constexpr (!COST) trav_init<FT>(P.sc, s.o, s.d, s.time, tr);
      has = true;
    }
    PH_ADD(PH_GRAB, t_grab);
#ifdef RT_DRAIN_TIMES
    if (b.part >= (uint32_t)kMaxParts && __builtin_amdgcn_readfirstlane((uint32_t)(g_tdrain[wave_in_group] != 0ull)) == 0u) {
      uint32_t rem = has ? (s.flags >> kCountShift) - s.j : 0u, act = has ? 1u : 0u;
      uint32_t sg = s.segs;
      for (int off = 32; off > 0; off >>= 1) {
        rem += __shfl_xor(rem, off);
        act += __shfl_xor(act, off);
        sg += __shfl_xor(sg, off);
      }
      if (lane_id() == 0u) {
        g_tdrain[wave_in_group] = wall_clock64();
        g_dinfo[wave_in_group][0] = rem;
        g_dinfo[wave_in_group][1] = act;
        g_dinfo[wave_in_group][2] = sg;
      }
    }
#endif
    if (!__any(has)) break;
    if constexpr (COST) {
      // The record loop always finishes in its one call, so a lane with a path is traversing
      // and ready in the same round: no tr.cur to carry and test, no ready ballot, count or
      // busy vote, no shade_min compare, no copy of tr.best, and no trav_init after a vertex
      // (its reciprocals and stack resets feed the tree steps only; trav_brute takes its own
      // rcp(d.y) and starts from the {inf, 0, 0, none} hit set here).
      if (has) {
        tr.best = {kInf, 0.0f, 0.0f, PRIM_NONE};
        trav_brute<FT, !LDS, SHAPE, EARLY>(P.sc, lnodes, s.o, s.d, s.time, 0.001f, tr);
      }
      // (nothing scheduled across: with the loop's tail and the vertex's head interleaved the
      // kernel took 77 VGPRs and 11 SGPR spills, with the barrier 75 and 8)
      __builtin_amdgcn_sched_barrier(0);
      if (has) {
        ++s.segs;
        if (shade_core<false, FT, LIGHT, SHAPE>(P, slot, s, tr.best, ws, sa, lnodes) == OUT_NEED_CHUNK) has = false;
      }
      continue;
    }
    PH_T(t_trav);
    if (has && tr.cur != TRAV_DONE)
    {
      PH_CNT(PH_TRAV_LANES, __popcll(__ballot(1)));
      PH_CNT(PH_TRAV_ROUNDS, 1);
      if constexpr (TREE == 0)
        trav_brute<FT, !LDS, SHAPE, EARLY>(P.sc, lnodes, s.o, s.d, s.time, 0.001f, tr);
      else if constexpr (TREE == 8)
      {
        const int nsteps = trav_steps8<FT>(P.sc, ts, s.o, s.d, s.time, 0.001f, tr, P.step_budget);
#ifdef RT_PHASES
        ph_steps(nsteps);
#endif
        (void)nsteps;
      }
      else
      {
        // TREE 5: the compressed BVH4 (64-B items, host_qbvh.cpp), read through L1/L2
        const int nsteps = trav_steps<LDS, FT, TREE == 4 || TREE == 5, TREE == 5>(
            P.sc, lnodes, recs_lds, ts, s.o, s.d, s.time, 0.001f, tr, P.step_budget);
        retest_near<FT>(P.sc, s.o, s.d, 0.001f, tr);
#ifdef RT_PHASES
        ph_steps(nsteps);
#endif
        (void)nsteps;
      }
    }
    PH_ADD(PH_TRAV, t_trav);
    const bool ready = has && tr.cur == TRAV_DONE;
    const uint32_t n_ready = (uint32_t)__popcll(__ballot(ready));
    const bool busy = __any(has && !ready);
    if (n_ready >= P.shade_min || !busy) {
      if (ready) {
        PH_CNT(PH_SHADE_LANES, n_ready);
        PH_CNT(PH_SHADE_ROUNDS, 1);
        PH_T(t_media);
        Hit best = tr.best;
        if constexpr (!EARLY) finish_hit<FT>(P, s, best);  // (EARLY: the trace is shade_core's)
        PH_ADD(PH_MEDIA, t_media);
        ++s.segs;
        PH_T(t_shade);
        if (shade_core<false, FT, LIGHT, EARLY ? SHAPE : 0>(P, slot, s, best, ws, sa, lnodes) == OUT_NEED_CHUNK) has = false;
        else trav_init<FT>(P.sc, s.o, s.d, s.time, tr);
        PH_ADD(PH_SHADE, t_shade);
      }
    }
  }
  PH_ADD(PH_LOOP, t_loop);
  uint32_t segs = s.segs;
  for (int off = 32; off > 0; off >>= 1) segs += __shfl_xor(segs, off);
  uint32_t pushes = s.pushes;
  for (int off = 32; off > 0; off >>= 1) pushes += __shfl_xor(pushes, off);
  if (lane_id() == 0) {
    atomicAdd(&P.ctr->segments, (unsigned long long)segs);
    atomicAdd(&P.ctr->pushes, (unsigned long long)pushes);
    if (P.wave_times) {
      const size_t w = (size_t)blockIdx.x * 4 + wave_in_group;
      unsigned long long* rec = P.wave_times + kWaveRec * w;
      rec[0] = g_tstart[wave_in_group];
      rec[1] = wall_clock64();
      rec[2] = segs;
#ifdef RT_DRAIN_TIMES
      rec[3] = g_tdrain[wave_in_group];
#else
      rec[3] = 0ull;
#endif
#ifdef RT_PHASES
      for (int i = 0; i < PH_N; ++i) rec[4 + i] = g_ph[wave_in_group][i];
#else
      for (int i = 0; i < PH_N; ++i) rec[4 + i] = 0ull;
#ifdef RT_DRAIN_TIMES
      for (int i = 0; i < 3; ++i) rec[4 + i] = g_dinfo[wave_in_group][i];
#endif
#endif
    }
  }
}

}  // namespace rt
#endif  // RT_FUSED_TABLE_ONLY

// ------------------------------------------------------------ the kernel table ---
// Every k_fused instance the library compiles, once: X(LDS, FT, TREE, SHAPE, LIGHT, MAP, EARLY,
// COST, unit).  `unit` is the translation unit that compiles the row: DEF rt_render.hip (instantiated
// by the dispatcher), ILP rt_fused_sets.hip (LLVM's iterative-ILP machine scheduler, Makefile),
// MAP rt_fused_map.hip (the default scheduler; a unit of its own so the build stays parallel).
// The explicit instantiations of the ILP and MAP units, rt_render.hip's `extern template`
// declarations of them and the dispatcher (rt_fused_pick.h) all expand from this table, so a
// row is compiled once, with its unit's flags, and can be chosen.  The sets are rt_device.h
// kFtSets ([5] is FT_ALL).
//
// The record loop (TREE 0) and its lean LDS kernels: per listed layout (SHAPE, rt_device.h
// brute_shape), per lean light kind (LIGHT), and the early-draw variant (EARLY) for shape 1 with
// light kind 1 only, and that kernel's lean-cost twin (COST, the default).  Shape 2 has no
// early-draw kernel: it compiled to 9 SGPR spills against the 8 of its (2, 1) kernel and was not
// measured, DESIGN.md §9.  The generic loop has no light-kind kernel: the dispatcher returns
// nullptr and the planner takes kind 0.
#define RT_FUSED_ROWS_RECORD_LOOP(X)                                  \
  X(true, kFtSets[0], 0, 1, 1, false, true, true, DEF)                \
  X(true, kFtSets[0], 0, 1, 1, false, true, false, DEF)               \
  X(true, kFtSets[0], 0, 1, 1, false, false, false, DEF)              \
  X(true, kFtSets[0], 0, 2, 1, false, false, false, DEF)              \
  X(true, kFtSets[0], 0, 1, 0, false, false, false, DEF)              \
  X(true, kFtSets[0], 0, 2, 0, false, false, false, DEF)              \
  X(true, kFtSets[0], 0, 0, 0, false, false, false, DEF)              \
  X(true, kFtSets[1], 0, 0, 0, false, false, false, DEF)              \
  X(false, kFtSets[0], 0, 0, 0, false, false, false, DEF)             \
  X(false, kFtSets[1], 0, 0, 0, false, false, false, DEF)
// BVH2 kernels exist for the two smallest sets with the tree in LDS (tiny scenes)
#define RT_FUSED_ROWS_BVH2(X)                                         \
  X(true, kFtSets[0], 2, 0, 0, false, false, false, DEF)              \
  X(true, kFtSets[1], 2, 0, 0, false, false, false, DEF)
// The BVH4, every set.  The C5 mesh set ([2]) and the C3 sphere set ([3]) take the ILP
// scheduler: C5 -0.6 / -1.0 %, C3 -0.8 %, images bit-identical; the same strategy costs the C2
// kernel 3.5 % (profiles/r3_sched_strategy_ab.jsonl, r3_split_ilp_ab.jsonl).
#define RT_FUSED_ROWS_BVH4(X)                                         \
  X(true, kFtSets[0], 4, 0, 0, false, false, false, DEF)              \
  X(false, kFtSets[0], 4, 0, 0, false, false, false, DEF)             \
  X(true, kFtSets[1], 4, 0, 0, false, false, false, DEF)              \
  X(false, kFtSets[1], 4, 0, 0, false, false, false, DEF)             \
  X(true, kFtSets[2], 4, 0, 0, false, false, false, ILP)              \
  X(false, kFtSets[2], 4, 0, 0, false, false, false, ILP)             \
  X(true, kFtSets[3], 4, 0, 0, false, false, false, ILP)              \
  X(false, kFtSets[3], 4, 0, 0, false, false, false, ILP)             \
  X(true, kFtSets[4], 4, 0, 0, false, false, false, DEF)              \
  X(false, kFtSets[4], 4, 0, 0, false, false, false, DEF)             \
  X(true, FT_ALL, 4, 0, 0, false, false, false, DEF)                  \
  X(false, FT_ALL, 4, 0, 0, false, false, false, DEF)
// The compressed BVH4 (TREE 5): trees read through L1/L2 only.  Not in the ILP unit: at 5 waves
// per SIMD the ILP scheduler spilled 6 / 26 VGPRs in the [2] / [3] kernels against 1 / 2 with the
// default one, and the default one renders C3 5.5 % and C5 0.3 % faster (bit-identical,
// profiles/r5_q_sched_ab.jsonl).  (book2's kernel with the ILP scheduler: C4 +0.7 %,
// r5_book2_sched_ab.jsonl)
#define RT_FUSED_ROWS_QBVH(X)                                         \
  X(false, kFtSets[2], 5, 0, 0, false, false, false, DEF)             \
  X(false, kFtSets[3], 5, 0, 0, false, false, false, DEF)             \
  X(false, kFtSets[4], 5, 0, 0, false, false, false, DEF)             \
  X(false, FT_ALL, 5, 0, 0, false, false, false, DEF)
// The BVH8 (measured slower than the BVH4): A/B builds only.  Large trees read
// through L1/L2, the three tree sets.
#ifdef RT_BVH8_KERNELS
#define RT_FUSED_ROWS_BVH8(X)                                         \
  X(false, kFtSets[2], 8, 0, 0, false, false, false, DEF)             \
  X(false, kFtSets[3], 8, 0, 0, false, false, false, DEF)             \
  X(false, kFtSets[4], 8, 0, 0, false, false, false, DEF)
#else
#define RT_FUSED_ROWS_BVH8(X)
#endif
// The MAP twins (active-pixel passes): one for every kernel the dispatcher
// selects with no knob set, but the record loop's SHAPE / LIGHT kernels (the generic record
// loop renders the same bits).  None for the opt-in trees 2 and 8.
#define RT_FUSED_ROWS_MAP(X)                                          \
  X(true, kFtSets[0], 0, 0, 0, true, false, false, MAP)               \
  X(false, kFtSets[0], 0, 0, 0, true, false, false, MAP)              \
  X(true, kFtSets[1], 0, 0, 0, true, false, false, MAP)               \
  X(false, kFtSets[1], 0, 0, 0, true, false, false, MAP)              \
  X(true, kFtSets[0], 4, 0, 0, true, false, false, MAP)               \
  X(false, kFtSets[0], 4, 0, 0, true, false, false, MAP)              \
  X(true, kFtSets[1], 4, 0, 0, true, false, false, MAP)               \
  X(false, kFtSets[1], 4, 0, 0, true, false, false, MAP)              \
  X(true, kFtSets[2], 4, 0, 0, true, false, false, MAP)               \
  X(false, kFtSets[2], 4, 0, 0, true, false, false, MAP)              \
  X(true, kFtSets[3], 4, 0, 0, true, false, false, MAP)               \
  X(false, kFtSets[3], 4, 0, 0, true, false, false, MAP)              \
  X(true, kFtSets[4], 4, 0, 0, true, false, false, MAP)               \
  X(false, kFtSets[4], 4, 0, 0, true, false, false, MAP)              \
  X(true, FT_ALL, 4, 0, 0, true, false, false, MAP)                   \
  X(false, FT_ALL, 4, 0, 0, true, false, false, MAP)                  \
  X(false, kFtSets[2], 5, 0, 0, true, false, false, MAP)              \
  X(false, kFtSets[3], 5, 0, 0, true, false, false, MAP)              \
  X(false, kFtSets[4], 5, 0, 0, true, false, false, MAP)              \
  X(false, FT_ALL, 5, 0, 0, true, false, false, MAP)
#define RT_FUSED_KERNELS(X)                                                                  \
  RT_FUSED_ROWS_RECORD_LOOP(X) RT_FUSED_ROWS_BVH2(X) RT_FUSED_ROWS_BVH4(X) RT_FUSED_ROWS_QBVH(X) \
  RT_FUSED_ROWS_BVH8(X) RT_FUSED_ROWS_MAP(X)
// A unit picks its rows by defining RT_FUSED_IN_DEF / _ILP / _MAP (L, F, T, S, G, M, E, C) and
// expanding RT_FUSED_KERNELS(RT_FUSED_BY_UNIT); the units it leaves out expand to nothing.
#define RT_FUSED_BY_UNIT(L, F, T, S, G, M, E, C, U) RT_FUSED_IN_##U(L, F, T, S, G, M, E, C)
#define RT_FUSED_SKIP(L, F, T, S, G, M, E, C)
#define RT_FUSED_INSTANTIATE(L, F, T, S, G, M, E, C) template __global__ void k_fused<L, F, T, S, G, M, E, C>(Params);
