// rt_trav.h — closest-hit traversal: Hit, the LDS / HBM traversal stack (TravStack), the
// resumable traversal state (Trav) and its steps over the BVH2, the BVH4, the compressed
// BVH4 (trav_steps) and the BVH8 (trav_steps8), the whole traversal at once (trace_world)
// and the constant media on top of the world hit (trace_media).
#pragma once
#include "rt_params.h"

namespace rt {

// ------------------------------------------------------------- traversal ---
struct Hit {
  float t, u, v;
  uint32_t ref;
};

RT_D void slab(const F4& lo, const F4& hi, f3 o, f3 inv, float tmin, float tmax, bool& hit,
               float& tnear) {
  float tx0 = (lo.x - o.x) * inv.x, tx1 = (hi.x - o.x) * inv.x;
  float ty0 = (lo.y - o.y) * inv.y, ty1 = (hi.y - o.y) * inv.y;
  float tz0 = (lo.z - o.z) * inv.z, tz1 = (hi.z - o.z) * inv.z;
  float t0 = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tmin));
  float t1 = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), tmax));
  hit = t0 <= t1 * 1.00000024f;  // 2 ulp slack: conservative for flat boxes
  tnear = t0;
}

// Closest hit over the world BVH (replaces BVHNode.Hit bvh.go:69-82 +
// HittableList.Hit hittable.go:122-138 + AABB.Hit aabb.go:90-113).
// LDS = true: the whole node array is staged in LDS (ds_read_b128); false: nodes
// come from HBM/L2 (global_load_dwordx4).  The two are separate instantiations:
// mixing both sources in one loop makes hipcc merge them into flat loads.
// The traversal stack lives in LDS (kShortStack entries per lane, one column
// per thread: conflict-free ds_read/write_b32) and overflows to HBM.
// Explicit address spaces: with generic pointers hipcc selects between the two
// bases and emits a flat load (slower, counts against both vmcnt and lgkmcnt).
struct TravStack {
  uint32_t* lds;     // &lds_stack[0][threadIdx.x], stride blockDim.x
  uint32_t* ovf;     // &ostack[slot], stride cols
  uint32_t cols;
  int nshort;        // LDS entries (a compile-time constant of each kernel)
  RT_D void push(int sp, uint32_t v) const {
    if (sp < nshort) {
      ((lds_u32*)lds)[sp * 256] = v;
    } else {
      ((glb_u32*)ovf)[(size_t)(sp - nshort) * cols] = v;
    }
  }
  RT_D uint32_t pop(int sp) const {
    uint32_t v;
    if (sp < nshort) {
      v = ((lds_u32*)lds)[sp * 256];
    } else {
      v = ((glb_u32*)ovf)[(size_t)(sp - nshort) * cols];
      wait_vm();
    }
    return v;
  }
};

// Resumable closest-hit traversal (replaces BVHNode.Hit bvh.go:69-82 +
// HittableList.Hit hittable.go:122-138 + AABB.Hit aabb.go:90-113).  One step =
// one inner node or one leaf; the fused kernel runs a bounded number of steps
// per scheduling round so a lane that finishes early does not idle until the
// wave's slowest ray is done (see k_fused).
constexpr uint32_t TRAV_DONE = 0xFFFFFFFFu;  // never a node or leaf code (host_bvh.cpp)
struct Trav {
  f3 inv;
  uint32_t cur;
  int sp;        // stack depth; entry sp-1 lives in `top`, entries below in TravStack
  uint32_t top;  // register copy of the top entry: a pop uses it at once and refills it
                 // from LDS in the background (the refill lands while the popped
                 // subtree is traversed), taking the LDS latency off the pop
  Hit best;
  // a triangle the last round's fp32 test rejected within its rounding error of an edge
  // (hit_tri_rec_m `near`), for tri_hit64 after trav_steps; PRIM_NONE: none.  Set only by the
  // round that ends on it, consumed before the next one (retest_near)
  uint32_t pend;
};
// the fp64 re-test of a round's near-edge rejection (hit_tri_rec_m): taken when it hits
// within the closest hit so far, as the fp32 test would have taken it.  Divergent and rare.
template <uint32_t FT>
RT_D void retest_near(const DevScene& sc, f3 o, f3 d, float tmin, Trav& tr) {
  if constexpr (HAS(FT_TRI)) {
    if (tr.pend != PRIM_NONE) {
      float t, u, v;
      if (tri_hit64(sc, tr.pend & 0x3FFFFFFFu, o, d, tmin, tr.best.t, t, u, v)) tr.best = {t, u, v, tr.pend};
    }
  }
}
// A new ray: the traversal state, and the spheres kept out of the BVH (radius >=
// kBigSphereR: the ground spheres of book1 and the mesh scene) tested first, in fp64, by
// every lane at once (a uniform loop over scalar-loaded records), so the BVH's sphere
// leaves are all small.  Their hit carries v = -1, a big sphere's mark (it told the fp32
// sphere leaves' refinement, removed since, that t was already fp64-solved).
template <uint32_t FT>
RT_D void trav_init(const DevScene& sc, f3 o, f3 d, float time, Trav& tr) {
  tr.inv = mk3(rcp(d.x), rcp(d.y), rcp(d.z));
  tr.cur = sc.root == PRIM_NONE ? TRAV_DONE : sc.root;
  tr.sp = 0;
  tr.top = 0;
  tr.best = {kInf, 0.0f, 0.0f, PRIM_NONE};
  if (HAS(FT_SPHERE))
    for (int i = 0; i < sc.n_big; ++i) {
      const F4* q = sc.big_recs + 4 * (size_t)__builtin_amdgcn_readfirstlane(i);
      const F4 rec[4] = {ld_cst(q), ld_cst(q + 1), ld_cst(q + 2), ld_cst(q + 3)};
      float t;
      if (hit_sphere_rec64(rec, o, d, time, 0.001f, tr.best.t, t))
        tr.best = {t, 0.0f, -1.0f, fbits(rec[0].w)};
    }
}

// LDS instantiation: lnodes holds the node array and, when recs_lds, the leaf
// records right after it (uniform flag: both load forms exist, one runs)
// one fp16 half of a 32-bit word as fp32 (an fma on it compiles to v_fma_mix_f32)
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
template <int H> RT_D float half_of(uint32_t w) { return (float)__builtin_bit_cast(h2v, w)[H]; }

// The compressed BVH4 node test (trav_steps QN): the four children's entry distances
// (inf: missed) and codes, sorted front to back
RT_D void qnode_children(const F4 v[4], f3 o, f3 inv, float tmin, float tmax, float tn[4],
                         uint32_t ch[4]) {
  // t = off * inv + (corner - o) * inv per plane (v_fma_mix_f32 on the fp16 offset).
  // Planes come as (lo 0|1, lo 2|3, hi 0|1, hi 2|3) per axis; the near pair is lo when
  // inv >= 0 and hi otherwise (a sign-mask select per word), so no min/max per axis.
  const float bx = (v[0].x - o.x) * inv.x, by = (v[0].y - o.y) * inv.y,
              bz = (v[0].z - o.z) * inv.z;
  const uint32_t info = fbits(v[0].w);
  const uint32_t base = info & 0x0FFFFFFFu, lmask = info >> 28;
  const uint32_t mx = neg_mask(inv.x), my = neg_mask(inv.y), mz = neg_mask(inv.z);
  const uint32_t nx[2] = {pick_by(fbits(v[1].x), fbits(v[1].z), mx), pick_by(fbits(v[1].y), fbits(v[1].w), mx)};
  const uint32_t fx[2] = {pick_by(fbits(v[1].z), fbits(v[1].x), mx), pick_by(fbits(v[1].w), fbits(v[1].y), mx)};
  const uint32_t ny[2] = {pick_by(fbits(v[2].x), fbits(v[2].z), my), pick_by(fbits(v[2].y), fbits(v[2].w), my)};
  const uint32_t fy[2] = {pick_by(fbits(v[2].z), fbits(v[2].x), my), pick_by(fbits(v[2].w), fbits(v[2].y), my)};
  const uint32_t nz[2] = {pick_by(fbits(v[3].x), fbits(v[3].z), mz), pick_by(fbits(v[3].y), fbits(v[3].w), mz)};
  const uint32_t fz[2] = {pick_by(fbits(v[3].z), fbits(v[3].x), mz), pick_by(fbits(v[3].w), fbits(v[3].y), mz)};
  auto child = [&](auto hk, int k) {
    constexpr int H = decltype(hk)::value;
    const int w = k >> 1;
    const float tx0 = fmaf(half_of<H>(nx[w]), inv.x, bx), tx1 = fmaf(half_of<H>(fx[w]), inv.x, bx);
    const float ty0 = fmaf(half_of<H>(ny[w]), inv.y, by), ty1 = fmaf(half_of<H>(fy[w]), inv.y, by);
    const float tz0 = fmaf(half_of<H>(nz[w]), inv.z, bz), tz1 = fmaf(half_of<H>(fz[w]), inv.z, bz);
    const float t0 = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, tmin));
    const float t1 = fminf(fminf(tx1, ty1), fminf(tz1, tmax));
    tn[k] = bitsf(pick_by(fbits(t0), 0x7F800000u, neg_mask(t1 * 1.00000024f - t0)));
    ch[k] = (base + (uint32_t)k) | (((lmask >> k) & 1u) << 31);
  };
  child(std::integral_constant<int, 0>{}, 0);
  child(std::integral_constant<int, 1>{}, 1);
  child(std::integral_constant<int, 0>{}, 2);
  child(std::integral_constant<int, 1>{}, 3);
  auto cx = [&](int a, int b) {  // as the 128-B path's network
    const uint32_t m = neg_mask(tn[b] - tn[a]);
    const uint32_t ta = fbits(tn[a]), tb = fbits(tn[b]);
    const uint32_t ca = ch[a], cb = ch[b];
    tn[a] = bitsf(pick_by(ta, tb, m));
    tn[b] = bitsf(pick_by(tb, ta, m));
    ch[a] = pick_by(ca, cb, m);
    ch[b] = pick_by(cb, ca, m);
  };
  cx(0, 1);
  cx(2, 3);
  cx(0, 2);
  cx(1, 3);
  cx(1, 2);
}

// QN: the compressed BVH4 (host_qbvh.cpp, rt_device.h "compressed BVH4 node"), 64-B
// items read through L1/L2; cur = item index, LEAF_BIT set for a single-prim leaf record
template <bool LDS, uint32_t FT, bool W4 = true, bool QN = false>
RT_D int trav_steps(const DevScene& sc, const F4* lnodes, bool recs_lds, const TravStack& stack,
                     f3 o, f3 d, float time, float tmin, Trav& tr, int budget) {
  uint32_t cur = tr.cur;
  int sp = tr.sp;
  uint32_t top = tr.top;
  // The register top is used with the BVH2 only (tiny LDS scenes, +1.2 % on C2):
  // with the BVH4 its extra store per push cost C3-C5 1-2 %.
  constexpr bool kTopReg = !W4;
  // push v: with kTopReg the old top goes down to the stack proper (entry sp-1)
  auto push = [&](uint32_t v) {
    if (kTopReg) {
      if (sp > 0) stack.push(sp - 1, top);
      top = v;
      ++sp;
    } else {
      stack.push(sp++, v);
    }
  };
  const f3 inv = tr.inv;
  // a near-edge rejection of this round, re-tested in fp64 after it (retest_near); a second
  // one ends the round before its step, which the next round repeats
  uint32_t pend = PRIM_NONE;
  int n = 0;
  for (; n < budget && cur != TRAV_DONE; ++n) {
    if constexpr (QN) {
      // One 64-B item per step, node or leaf record alike (4 x 16 B, issued together).
      const bool leaf = (cur & LEAF_BIT) != 0u;
#ifdef RT_PHASES
      {  // node / leaf steps of this iteration, and whether both kinds ran in it
        const unsigned long long ml = __ballot(leaf), mn = __ballot(!leaf);
        PH_CNT(PH_QLEAF_LANES, __popcll(ml));
        PH_CNT(PH_QNODE_LANES, __popcll(mn));
        PH_CNT(PH_QMIXED, (ml && mn) ? 1 : 0);
        PH_CNT(PH_QITERS, 1);
        const uint32_t item = cur & 0x0FFFFFFFu;
        const uint32_t first_item = __builtin_amdgcn_readfirstlane(item);
        PH_CNT(PH_QSAME, __popcll(__ballot(item == first_item)));
        PH_CNT(PH_QTOP, __popcll(__ballot(item < 85u)));
        PH_CNT(PH_QMID, __popcll(__ballot(item >= 85u && item < 1365u)));
        unsigned long long left = __ballot(1);
        uint32_t uniq = 0;
        while (left) {  // distinct items among the active lanes (debug build only)
          const uint32_t lead = (uint32_t)(__ffsll((long long)left) - 1);
          const uint32_t vi = __builtin_amdgcn_readlane(item, lead);
          left &= ~__ballot(item == vi);
          ++uniq;
        }
        PH_CNT(PH_QUNIQ, uniq);
      }
#endif
      const F4* it = (const F4*)((const char*)sc.nodes + ((cur & 0x0FFFFFFFu) << 6));
      F4 v[4];
      // (all four unconditionally: a leaf lane skipping the fourth when the scene has no
      // quads made hipcc wait for the first loads before the predicated one, C5 +1.9 %)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ld_glb(it + e);
      if (!leaf) {
        float tn[4];
        uint32_t ch[4];
        qnode_children(v, o, inv, tmin, tr.best.t, tn, ch);
        if (tn[0] != kInf) {
          if (sp + 3 <= stack.nshort) {
            lds_u32* q = (lds_u32*)stack.lds;
            q[sp * 256] = ch[3];
            sp += tn[3] != kInf;
            q[sp * 256] = ch[2];
            sp += tn[2] != kInf;
            q[sp * 256] = ch[1];
            sp += tn[1] != kInf;
          } else {
            if (tn[3] != kInf && sp < kStack) push(ch[3]);
            if (tn[2] != kInf && sp < kStack) push(ch[2]);
            if (tn[1] != kInf && sp < kStack) push(ch[1]);
          }
          cur = ch[0];
          continue;
        }
      } else {
        float t, u, vv;
        uint32_t ref;
        bool near;
        const uint32_t rej = hit_record_m<FT>(v, o, d, inv.y, time, tmin, tr.best.t, t, u, vv, ref, near);
        tr.best.t = bitsf(pick_by(fbits(t), fbits(tr.best.t), rej));
        tr.best.u = bitsf(pick_by(fbits(u), fbits(tr.best.u), rej));
        tr.best.v = bitsf(pick_by(fbits(vv), fbits(tr.best.v), rej));
        tr.best.ref = pick_by(ref, tr.best.ref, rej);
        if (HAS(FT_TRI) && near) {
          if (pend != PRIM_NONE) {  // (rejected: nothing changed) this leaf again next round
            n = budget;
            continue;
          }
          pend = ref;
        }
      }
      if (sp == 0) cur = TRAV_DONE;
      else cur = stack.pop(--sp);
      continue;
    }
    if (W4 && !LDS) {
      // One fetch per step for node and leaf lanes alike: the node (nodes + 8 cur,
      // 7 x 16 B) or the leaf's first record (leafprims + 4 first, 4 x 16 B), issued
      // together before either is used.  With the loads inside each branch, a wave
      // whose lanes are split between nodes and leaves waited for two dependent
      // memory round trips per step; here it waits for one (measured against the split
      // fetch: C3 -1.7 %, C4 -4.9 %, C5 -2.8 %, profiles/r3_unified_fetch_ab.jsonl).
      // Node and leaf record share one allocation (rt_render.hip upload_scene): both are
      // addressed as 32-bit byte offsets from the node base (global_load with an SGPR
      // base).  A node's planes are fetched already ordered by the ray's direction signs:
      // the near x plane of the four children is lo.x (offset 0) when inv.x >= 0 and hi.x
      // (offset 16) when inv.x < 0, the far plane the other one, and likewise for y / z.
      // The slab test then needs no min/max per axis (v_min/v_max_f32 issue at half the
      // rate of v_sub/v_mul on gfx950, profiles/r4_instr_rate.jsonl): 16 min/max per node
      // instead of 40.  The same planes as min/max would pick, so the same t0, t1.
      const bool leaf = (cur & LEAF_BIT) != 0u;
      const uint32_t first = (cur >> 4) & 0x7FFFFFFu;
      const uint32_t rec0 = (uint32_t)((const char*)sc.leafprims - (const char*)sc.nodes);
      const uint32_t off = leaf ? rec0 + (first << 6) : cur << 7;
      const uint32_t nmask = leaf ? 0u : 16u;
      const uint32_t sx = (fbits(inv.x) >> 27) & nmask, sy = (fbits(inv.y) >> 27) & nmask;
      // (node: v[0] = the child codes, then near x, far x, near y; a leaf: its record)
      const char* nb = (const char*)sc.nodes;
      F4 v[7];
      v[0] = ld_glb((const F4*)(nb + off));
      v[1] = ld_glb((const F4*)(nb + (off + (16u + sx))));
      v[2] = ld_glb((const F4*)(nb + (off + (32u - sx))));
      v[3] = ld_glb((const F4*)(nb + (off + (48u + sy))));
      if (!leaf) {
        const uint32_t sz = (fbits(inv.z) >> 27) & 16u;
        v[4] = ld_glb((const F4*)(nb + (off + (64u - sy))));
        v[5] = ld_glb((const F4*)(nb + (off + (80u + sz))));
        v[6] = ld_glb((const F4*)(nb + (off + (96u - sz))));
        const float tmax = tr.best.t;
        float tn[4];
        uint32_t ch[4];
        const float Nx[4] = {v[1].x, v[1].y, v[1].z, v[1].w}, Fx[4] = {v[2].x, v[2].y, v[2].z, v[2].w};
        const float Ny[4] = {v[3].x, v[3].y, v[3].z, v[3].w}, Fy[4] = {v[4].x, v[4].y, v[4].z, v[4].w};
        const float Nz[4] = {v[5].x, v[5].y, v[5].z, v[5].w}, Fz[4] = {v[6].x, v[6].y, v[6].z, v[6].w};
        const uint32_t C[4] = {fbits(v[0].x), fbits(v[0].y), fbits(v[0].z), fbits(v[0].w)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float tx0 = (Nx[k] - o.x) * inv.x, tx1 = (Fx[k] - o.x) * inv.x;
          const float ty0 = (Ny[k] - o.y) * inv.y, ty1 = (Fy[k] - o.y) * inv.y;
          const float tz0 = (Nz[k] - o.z) * inv.z, tz1 = (Fz[k] - o.z) * inv.z;
          const float t0 = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, tmin));
          const float t1 = fminf(fminf(tx1, ty1), fminf(tz1, tmax));
          // hit when t0 <= t1 * (1 + 2 ulp) (slab() semantics), i.e. when that difference
          // is not negative: tn = hit ? t0 : inf as a sign-mask select.  (An empty slot's
          // inverted infinite box gives t1 = -inf: no code check.  t0 = t1 = inf gives a
          // NaN difference with the sign clear: a "hit" at inf, as with the comparison.)
          tn[k] = bitsf(pick_by(fbits(t0), 0x7F800000u, neg_mask(t1 * 1.00000024f - t0)));
          ch[k] = C[k];
        }
        // compare-exchange as sign-mask selects: swap when tn[b] - tn[a] < 0, i.e. when
        // tn[b] < tn[a] (the difference of two distinct floats is never +-0; inf - inf
        // gives a NaN with the sign clear: no swap, like the comparison)
        auto cx = [&](int a, int b) {
          const uint32_t m = neg_mask(tn[b] - tn[a]);
          const uint32_t ta = fbits(tn[a]), tb = fbits(tn[b]);
          const uint32_t ca = ch[a], cb = ch[b];
          tn[a] = bitsf(pick_by(ta, tb, m));
          tn[b] = bitsf(pick_by(tb, ta, m));
          ch[a] = pick_by(ca, cb, m);
          ch[b] = pick_by(cb, ca, m);
        };
        cx(0, 1);
        cx(2, 3);
        cx(0, 2);
        cx(1, 3);
        cx(1, 2);
        if (tn[0] != kInf) {
          // The sorted hits are a prefix (tn[1] <= tn[2] <= tn[3], misses at inf): all three
          // candidates are written to consecutive LDS entries, farthest first, and the stack
          // pointer advances past the valid ones — no exec-mask branch per push when the
          // short stack has room (C3 -0.5 %, C4 -1.0 %, C5 -0.5 %, bit-identical,
          // profiles/r3_push_nobranch_ab.jsonl)
          if (!kTopReg && sp + 3 <= stack.nshort) {
            lds_u32* q = (lds_u32*)stack.lds;
            q[sp * 256] = ch[3];
            sp += tn[3] != kInf;
            q[sp * 256] = ch[2];
            sp += tn[2] != kInf;
            q[sp * 256] = ch[1];
            sp += tn[1] != kInf;
          } else {
            if (tn[3] != kInf && sp < kStack) push(ch[3]);
            if (tn[2] != kInf && sp < kStack) push(ch[2]);
            if (tn[1] != kInf && sp < kStack) push(ch[1]);
          }
          cur = ch[0];
          continue;
        }
      } else {
        const uint32_t count = (cur & 15u) + 1u;
        F4 rec[4] = {v[0], v[1], v[2], v[3]};
        uint32_t k = 0;
        for (;;) {
          float t, u, vv;
          uint32_t ref;
          bool near;
          const uint32_t rej = hit_record_m<FT>(rec, o, d, inv.y, time, tmin, tr.best.t, t, u, vv, ref, near);
          tr.best.t = bitsf(pick_by(fbits(t), fbits(tr.best.t), rej));
          tr.best.u = bitsf(pick_by(fbits(u), fbits(tr.best.u), rej));
          tr.best.v = bitsf(pick_by(fbits(vv), fbits(tr.best.v), rej));
          tr.best.ref = pick_by(ref, tr.best.ref, rej);
          if (HAS(FT_TRI) && near) {
            if (pend != PRIM_NONE) {  // the round ends before this prim (repeated next round)
              n = budget;
              break;
            }
            pend = ref;
          }
          ++k;
          if (k >= count) break;
          const F4* q = sc.leafprims + 4 * (size_t)(first + k);
          for (int e = 0; e < 4; ++e) rec[e] = ld_glb(q + e);
        }
        if (HAS(FT_TRI) && k < count) {
          cur = LEAF_BIT | ((first + k) << 4) | (count - k - 1u);
          continue;
        }
      }
      if (sp == 0) cur = TRAV_DONE;
      else cur = stack.pop(--sp);
      continue;
    }
    if (!W4 && !(cur & LEAF_BIT)) {
      // BVH2 node (tiny scenes, see render_impl): both child boxes, nearer first
      const F4* g = LDS ? lnodes + 4 * cur : sc.nodes + 4 * (size_t)cur;
      const F4 a0 = g[0], a1 = g[1], b0 = g[2], b1 = g[3];
      bool h0, h1;
      float t0, t1;
      slab(a0, a1, o, inv, tmin, tr.best.t, h0, t0);
      slab(b0, b1, o, inv, tmin, tr.best.t, h1, t1);
      const uint32_t c0 = fbits(a0.w), c1 = fbits(a1.w);
      if (h0 && h1) {
        const uint32_t nearc = t0 <= t1 ? c0 : c1, farc = t0 <= t1 ? c1 : c0;
        if (sp < kStack) push(farc);
        cur = nearc;
        continue;
      }
      if (h0 || h1) {
        cur = h0 ? c0 : c1;
        continue;
      }
    } else if (W4 && !(cur & LEAF_BIT)) {
      // BVH4 node: four slab tests, children ordered front to back; the
      // nearest is visited next, the others pushed farthest first
      const F4* g = LDS ? lnodes + 8 * cur : sc.nodes + 8 * (size_t)cur;
      const F4 cc = g[0], lx = g[1], hx = g[2], ly = g[3], hy = g[4], lz = g[5], hz = g[6];
      const float tmax = tr.best.t;
      float tn[4];
      uint32_t ch[4];
      const float Lx[4] = {lx.x, lx.y, lx.z, lx.w}, Hx[4] = {hx.x, hx.y, hx.z, hx.w};
      const float Ly[4] = {ly.x, ly.y, ly.z, ly.w}, Hy[4] = {hy.x, hy.y, hy.z, hy.w};
      const float Lz[4] = {lz.x, lz.y, lz.z, lz.w}, Hz[4] = {hz.x, hz.y, hz.z, hz.w};
      const uint32_t C[4] = {fbits(cc.x), fbits(cc.y), fbits(cc.z), fbits(cc.w)};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float tx0 = (Lx[k] - o.x) * inv.x, tx1 = (Hx[k] - o.x) * inv.x;
        const float ty0 = (Ly[k] - o.y) * inv.y, ty1 = (Hy[k] - o.y) * inv.y;
        const float tz0 = (Lz[k] - o.z) * inv.z, tz1 = (Hz[k] - o.z) * inv.z;
        const float t0 = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tmin));
        const float t1 = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), tmax));
        const bool h = t0 <= t1 * 1.00000024f && C[k] != CHILD_EMPTY;  // slab() semantics
        tn[k] = h ? t0 : kInf;
        ch[k] = C[k];
      }
      // sorting network (0,1)(2,3)(0,2)(1,3)(1,2): ascending entry distance
      auto cx = [&](int a, int b) {
        const bool sw = tn[b] < tn[a];
        const float ta = tn[a], tb = tn[b];
        const uint32_t ca = ch[a], cb = ch[b];
        tn[a] = sw ? tb : ta;
        tn[b] = sw ? ta : tb;
        ch[a] = sw ? cb : ca;
        ch[b] = sw ? ca : cb;
      };
      cx(0, 1);
      cx(2, 3);
      cx(0, 2);
      cx(1, 3);
      cx(1, 2);
      if (tn[0] != kInf) {
        if (tn[3] != kInf && sp < kStack) push(ch[3]);
        if (tn[2] != kInf && sp < kStack) push(ch[2]);
        if (tn[1] != kInf && sp < kStack) push(ch[1]);
        cur = ch[0];
        continue;
      }
    } else {
      uint32_t first = (cur >> 4) & 0x7FFFFFFu, count = (cur & 15u) + 1u;
      // leaf records are contiguous: no ref indirection, all four loads issue at once
      uint32_t k = 0;
      for (; k < count;) {
        const uint32_t ri = 4 * (first + k);
        F4 rec[4];
        if (LDS && recs_lds) {
          const F4* q = lnodes + (W4 ? 8 : 4) * sc.n_nodes + ri;
          for (int e = 0; e < 4; ++e) rec[e] = ld_lds(q + e);
        } else {
          const F4* q = sc.leafprims + ri;
          for (int e = 0; e < 4; ++e) rec[e] = ld_glb(q + e);
          if (LDS) wait_vm();  // LDS kernel whose records did not fit: keep the wait here
        }
        float t, u, v;
        uint32_t ref;
        bool near;
        const uint32_t rej = hit_record_m<FT>(rec, o, d, inv.y, time, tmin, tr.best.t, t, u, v, ref, near);
        tr.best.t = bitsf(pick_by(fbits(t), fbits(tr.best.t), rej));
        tr.best.u = bitsf(pick_by(fbits(u), fbits(tr.best.u), rej));
        tr.best.v = bitsf(pick_by(fbits(v), fbits(tr.best.v), rej));
        tr.best.ref = pick_by(ref, tr.best.ref, rej);
        if (HAS(FT_TRI) && near) {
          if (pend != PRIM_NONE) {  // the round ends before this prim (repeated next round)
            n = budget;
            break;
          }
          pend = ref;
        }
        ++k;
      }
      if (HAS(FT_TRI) && k < count) {  // the leaf's other prims first, next round
        cur = LEAF_BIT | ((first + k) << 4) | (count - k - 1u);
        continue;
      }
    }
    if (sp == 0) {
      cur = TRAV_DONE;
    } else if (kTopReg) {
      cur = top;
      if (--sp > 0) top = stack.pop(sp - 1);
    } else {
      cur = stack.pop(--sp);
    }
  }
  tr.cur = cur;
  tr.sp = sp;
  tr.top = top;
  tr.pend = pend;
  return n;
}

// ---- BVH8 (large scenes, host_bvh8.cpp layout, rt_device.h "BVH8 node") ----
// A child slot's traversal code from its meta byte: inner node child_base + rank, or
// a leaf code over recs8 (the same LEAF_BIT format as the BVH4's leaves).
RT_D uint32_t bvh8_code(uint32_t m, uint32_t child_base, uint32_t leaf_base) {
  return (m & 0x80u) ? child_base + (m & 7u)
                     : LEAF_BIT | ((leaf_base + (m & 31u)) << 4) | ((m >> 5) & 3u);
}
RT_D uint32_t bvh8_meta(uint32_t m0, uint32_t m1, uint32_t k) {
  return (uint32_t)((((unsigned long long)m1 << 32) | m0) >> (8u * k)) & 0xFFu;
}
// Resumable closest-hit traversal of the BVH8 (same contract as trav_steps).  A
// node step fetches one 128-B line per lane and tests eight children: each plane
// is t = (origin + q * 2^e - o) * inv, evaluated as fma(q, 2^e * inv, (origin - o)
// * inv) (2^e * inv is exact); the boxes carry one quantum of padding and the hit
// test 4 ulp of slack on the exit distance, which cover this form's rounding.
// The hit children's entry distances are sorted as keys (t0 bits with the slot in
// the low 3 bits: t0 >= tmin > 0, so the bits order like the floats) by a
// 19-comparator network of integer min/max; the nearest is visited next, the rest
// pushed farthest first.  Leaf steps fetch the record (64 B) only.
template <uint32_t FT>
RT_D int trav_steps8(const DevScene& sc, const TravStack& stack, f3 o, f3 d, float time,
                     float tmin, Trav& tr, int budget) {
  uint32_t cur = tr.cur;
  int sp = tr.sp;
  const f3 inv = tr.inv;
  const bool negx = inv.x < 0.0f, negy = inv.y < 0.0f, negz = inv.z < 0.0f;
  int n = 0;
  for (; n < budget && cur != TRAV_DONE; ++n) {
    const bool leaf = (cur & LEAF_BIT) != 0u;
    const uint32_t first = (cur >> 4) & 0x7FFFFFFu;
    const F4* g = leaf ? sc.recs8 + 4 * (size_t)first : sc.nodes8 + 8 * (size_t)cur;
    F4 v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ld_glb(g + e);
    if (!leaf) {
#pragma unroll
      for (int e = 4; e < 8; ++e) v[e] = ld_glb(g + e);
      const uint32_t ex = fbits(v[0].w);
      const float scx = bitsf((ex & 0xFFu) << 23) * inv.x;
      const float scy = bitsf(((ex >> 8) & 0xFFu) << 23) * inv.y;
      const float scz = bitsf(((ex >> 16) & 0xFFu) << 23) * inv.z;
      const float bx = (v[0].x - o.x) * inv.x, by = (v[0].y - o.y) * inv.y,
                  bz = (v[0].z - o.z) * inv.z;
      const uint32_t child_base = fbits(v[1].x), leaf_base = fbits(v[1].y);
      const uint32_t m0 = fbits(v[1].z), m1 = fbits(v[1].w);
      const uint32_t LX[4] = {fbits(v[2].x), fbits(v[2].y), fbits(v[2].z), fbits(v[2].w)};
      const uint32_t HX[4] = {fbits(v[3].x), fbits(v[3].y), fbits(v[3].z), fbits(v[3].w)};
      const uint32_t LY[4] = {fbits(v[4].x), fbits(v[4].y), fbits(v[4].z), fbits(v[4].w)};
      const uint32_t HY[4] = {fbits(v[5].x), fbits(v[5].y), fbits(v[5].z), fbits(v[5].w)};
      const uint32_t LZ[4] = {fbits(v[6].x), fbits(v[6].y), fbits(v[6].z), fbits(v[6].w)};
      const uint32_t HZ[4] = {fbits(v[7].x), fbits(v[7].y), fbits(v[7].z), fbits(v[7].w)};
      // entry / exit planes by the ray's direction signs, selected as whole words
      uint32_t NX[4], FX[4], NY[4], FY[4], NZ[4], FZ[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        NX[j] = negx ? HX[j] : LX[j];
        FX[j] = negx ? LX[j] : HX[j];
        NY[j] = negy ? HY[j] : LY[j];
        FY[j] = negy ? LY[j] : HY[j];
        NZ[j] = negz ? HZ[j] : LZ[j];
        FZ[j] = negz ? LZ[j] : HZ[j];
      }
      const float tmax = tr.best.t;
      uint32_t key[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int j = k >> 1, sh = (k & 1) * 16;
        auto q = [&](uint32_t w) { return (float)((w >> sh) & 0xFFFFu); };
        const float t0 = fmaxf(fmaxf(fmaf(q(NX[j]), scx, bx), fmaf(q(NY[j]), scy, by)),
                               fmaxf(fmaf(q(NZ[j]), scz, bz), tmin));
        const float t1 = fminf(fminf(fmaf(q(FX[j]), scx, bx), fmaf(q(FY[j]), scy, by)),
                               fminf(fmaf(q(FZ[j]), scz, bz), tmax));
        const uint32_t m = ((k < 4 ? m0 : m1) >> (8 * (k & 3))) & 0xFFu;
        const bool h = t0 <= t1 * 1.0000005f && m != 0xFFu;
        key[k] = h ? (fbits(t0) & ~7u) | (uint32_t)k : 0xFFFFFFFFu;
      }
      auto cx = [&](int a, int b) {
        const uint32_t lo = min(key[a], key[b]), hi = max(key[a], key[b]);
        key[a] = lo;
        key[b] = hi;
      };
      cx(0, 1), cx(2, 3), cx(4, 5), cx(6, 7);
      cx(0, 2), cx(1, 3), cx(4, 6), cx(5, 7);
      cx(1, 2), cx(5, 6);
      cx(0, 4), cx(1, 5), cx(2, 6), cx(3, 7);
      cx(2, 4), cx(3, 5);
      cx(1, 2), cx(3, 4), cx(5, 6);
      if (key[0] != 0xFFFFFFFFu) {
#pragma unroll
        for (int i = 7; i >= 1; --i)
          if (key[i] != 0xFFFFFFFFu && sp < kStack)
            stack.push(sp++, bvh8_code(bvh8_meta(m0, m1, key[i] & 7u), child_base, leaf_base));
        cur = bvh8_code(bvh8_meta(m0, m1, key[0] & 7u), child_base, leaf_base);
        continue;
      }
    } else {
      const uint32_t count = (cur & 15u) + 1u;
      F4 rec[4] = {v[0], v[1], v[2], v[3]};
      for (uint32_t k = 0;;) {
        float t, u, vv;
        uint32_t ref;
        bool near;
        const uint32_t rej = hit_record_m<FT>(rec, o, d, inv.y, time, tmin, tr.best.t, t, u, vv, ref, near);
        tr.best.t = bitsf(pick_by(fbits(t), fbits(tr.best.t), rej));
        tr.best.u = bitsf(pick_by(fbits(u), fbits(tr.best.u), rej));
        tr.best.v = bitsf(pick_by(fbits(vv), fbits(tr.best.v), rej));
        tr.best.ref = pick_by(ref, tr.best.ref, rej);
        // (opt-in BVH8 kernels: the near-edge fp64 re-test applied at once, not deferred)
        if (HAS(FT_TRI) && near && tri_hit64(sc, ref & 0x3FFFFFFFu, o, d, tmin, tr.best.t, t, u, vv))
          tr.best = {t, u, vv, ref};
        if (++k >= count) break;
        const F4* q = sc.recs8 + 4 * (size_t)(first + k);
        for (int e = 0; e < 4; ++e) rec[e] = ld_glb(q + e);
      }
    }
    if (sp == 0) cur = TRAV_DONE;
    else cur = stack.pop(--sp);
  }
  tr.cur = cur;
  tr.sp = sp;
  return n;
}

// the whole traversal at once (wavefront extend kernel)
template <bool LDS, uint32_t FT>
RT_D void trace_world(const DevScene& sc, const F4* lnodes, bool recs_lds, const TravStack& stack,
                      f3 o, f3 d, float time, float tmin, Hit& best) {
  Trav tr;
  trav_init<FT>(sc, o, d, time, tr);
  do {  // a near-edge rejection ends a round early (retest_near)
    trav_steps<LDS, FT>(sc, lnodes, recs_lds, stack, o, d, time, tmin, tr, 0x7FFFFFFF);
    retest_near<FT>(sc, o, d, tmin, tr);
  } while (tr.cur != TRAV_DONE);
  best = tr.best;
}

// closest boundary hit over (lo, hi) with each prim's own interval semantics
RT_D bool boundary_hit(const DevScene& sc, const DevMedium& m, f3 o, f3 d, float time, double lo,
                       double hi, double& t_out) {
  bool any = false;
  double best = hi;
  for (uint32_t k = 0; k < m.bcount; ++k) {
    double t;
    if (hit_prim_d(sc, sc.medium_refs[m.bfirst + k], o, d, time, lo, best, t)) {
      any = true;
      best = t;
    }
  }
  t_out = best;
  return any;
}

// constantMedium.Hit medium.go:27-58, as a closest-hit candidate.  A medium
// occurrence with multiplicity m keeps the smallest of m free-flight draws.
// Interval arithmetic in fp64: the reference searches (t1 + 1e-4, inf) with
// |t1| up to ~1e4 (book2 fog, R = 5000), below fp32 resolution.
// `spare`: rt_spare24 of the call that generated this ray, the scene's last draw
// index (rt_rng.h), so the outermost medium needs no Philox call of its own.
RT_D void trace_media(const Params& P, f3 o, f3 d, float time, float tmin, uint32_t gpix,
                      uint32_t sample, uint32_t vertex, uint32_t spare, Hit& best) {
  const DevScene& sc = P.sc;
  rt_u32x4 r = {{0, 0, 0, 0}};
  int cached_group = -1;
  const float ray_len = length(d);
  for (int mi = 0; mi < sc.n_media; ++mi) {
    // the medium record and its boundary through the scalar cache (a uniform index: no
    // vector-memory load, and no s_waitcnt vmcnt on the traversal's outstanding loads)
    static_assert(sizeof(DevMedium) == 32, "DevMedium: two 16-B scalar loads");
    const F4* mr = (const F4*)(sc.media + __builtin_amdgcn_readfirstlane(mi));
    const F4 ma = ld_cst(mr), mb = ld_cst(mr + 1);
    DevMedium m;
    m.bfirst = fbits(ma.x);
    m.bcount = fbits(ma.y);
    m.neg_inv_density = ma.z;
    m.phase_mat = (int32_t)fbits(ma.w);
    m.draw_base = (int32_t)fbits(mb.x);
    m.mult = (int32_t)fbits(mb.y);
    // The free-flight distance first (its draws are a pure function of the path's
    // counters, rt_rng.h, so drawing them before the boundary test changes nothing).
    // The medium's hit lies at max(t1, tmin) + hd / |d| > hd / |d|: when that is already
    // past the closest hit, the medium cannot be the closest hit and its fp64 boundary
    // roots are not needed -- book2's R = 5000 fog (mean free path 10^4) skips them on
    // most segments.  Same result as computing them (tm < best.t fails either way).
    float hd = kInf;
    for (int k = 0; k < m.mult; ++k) {
      int draw = m.draw_base + k;
      float u;
      if (draw == sc.medium_draws - 1) {
        u = rt_unit_f(spare);
      } else {
        int group = 1 + (draw >> 2);
        if (group != cached_group) {
          r = rt_rng_draw(P.seed, gpix, sample, RT_STREAM(vertex, group));
          cached_group = group;
        }
        u = rt_unit_f(r.v[draw & 3]);
      }
      hd = fminf(hd, m.neg_inv_density * logf(u));
    }
    const float hd_t = hd / ray_len;  // the same quotient as tm's below
    if (!(hd_t < best.t)) continue;
    double t1, t2;
    typedef __attribute__((address_space(4))) const uint32_t cst_u32;
    const uint32_t b0 = m.bcount == 1 ? *(const cst_u32*)(sc.medium_refs + m.bfirst) : PRIM_NONE;
    if ((b0 >> 30) == PRIM_SPHERE && b0 != PRIM_NONE) {
      // a sphere boundary (book2's fog and glass-ball interior): one quadratic gives
      // both boundary.Hit calls of medium.go:33-42 — t1 = the smaller root (always
      // inside (-inf, inf)), t2 = the larger one if it exceeds t1 + 1e-4
      double r0, r1;
      const uint32_t bi = b0 & 0x3FFFFFFFu;
      if (!sphere_roots_cm(ld_cst(sc.sph_cr + bi), ld_cst(sc.sph_mv + bi), o, d, time, r0, r1))
        continue;
      t1 = r0;
      if (!(t1 + 0.0001 < r1 && r1 < (double)kInf)) continue;
      t2 = r1;
    } else {
      if (!boundary_hit(sc, m, o, d, time, -(double)kInf, (double)kInf, t1)) continue;
      if (!boundary_hit(sc, m, o, d, time, t1 + 0.0001, (double)kInf, t2)) continue;
    }
    t1 = fmax(t1, (double)tmin);
    if (t1 >= t2) continue;
    t1 = fmax(0.0, t1);
    double inside = (t2 - t1) * (double)ray_len;
    if ((double)hd > inside) continue;
    float tm = (float)(t1 + (double)hd_t);
    if (tm < best.t) {
      best.t = tm;
      best.u = 0.0f;
      best.v = 0.0f;
      best.ref = prim_ref(PRIM_MEDIUM, (uint32_t)mi);
    }
  }
}

}  // namespace rt
