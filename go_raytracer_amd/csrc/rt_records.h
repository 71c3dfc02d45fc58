// rt_records.h — the record loop (TREE 0, tiny quad-only scenes): every leaf record tested
// by every lane, two at a time in packed fp32, with its per-layout (SHAPE) and early-draw
// (EARLY) variants and the winner's resolve.
#pragma once
#include "rt_trav.h"

namespace rt {

// Tiny scenes: every leaf record, in order, from the LDS cache (or through the
// scalar cache).  All lanes test the same record at the same time (a broadcast
// read, no divergence, no stack), which on 64-wide SIMDs beats a divergent BVH
// walk when the scene has a few dozen prims (C2: 18 quads).  Closest hit over all
// records = BVHNode.Hit's result (hittable.go:122-138; quad.go Hit per record).
// The small feature sets hold quads only, so the loop is the quad test alone,
// two records at a time in packed fp32 (v_pk_fma_f32: one issue, two records)
// from the pair layout (rt_device.h), branch-free: the loop keeps the closest t
// and its record index; the winner's (alpha, beta) and ref are recomputed once
// after the loop with the same fma sequence, so they equal the loop's values.
// The record loop is VALU-issue bound (C2: ~55 % of the kernel), so every
// instruction per record counts: 11 packed/rcp ops + 5 checks + 2 selects
// (18 VALU per record test, was 36 with one record at a time and early exits).
RT_D v2f pfma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
// 0 <= a <= 1 && 0 <= b <= 1 as one unsigned max + compare: non-negative floats
// order like their bits, and negatives / NaN have the sign or exponent bits set
// above 1.0f's.  (-0.0f is rejected where the reference accepts it: exactly
// zero alpha with a negative sign; measure zero, within the parity tolerance.)
RT_D bool unit_ab(float a, float b) {
  return max(__float_as_uint(a), __float_as_uint(b)) <= 0x3F800000u;
}
// The record tests' acceptance as a sign mask (all ones = reject), from differences whose
// sign bit says the same as each comparison: |den| - 1e-8, t - tmin, best - t (>= 0 when
// the comparison holds; equal values give +0) and unit_ab_rej.  Then the closest-hit update
// is two v_bitop3 selects instead of v_cmp / v_cndmask (half rate and slower on gfx950,
// profiles/r4_instr_rate.jsonl): same choices.
RT_D uint32_t rec_reject(float den, float t, float tmin, float best, float a, float b) {
  const uint32_t ab = unit_ab_rej(a, b);
  const uint32_t any = __builtin_amdgcn_bitop3_b32(__float_as_uint(fabsf(den) - 1e-8f),
                                                   __float_as_uint(t - tmin),
                                                   __float_as_uint(best - t), 0xFE) | ab;
  return (uint32_t)((int32_t)any >> 31);
}
// the same without the denominator test (axis-aligned records: the inverse of the axis
// direction component is NaN when |d_a| < 1e-8; a NaN t makes alpha and beta NaN, whose
// bits exceed 1.0f's in either sign, so the alpha/beta term rejects it as t >= tmin did)
RT_D uint32_t rec_reject_t(float t, float tmin, float best, float a, float b) {
  const uint32_t ab = unit_ab_rej(a, b);
  const uint32_t any = __builtin_amdgcn_bitop3_b32(__float_as_uint(t - tmin),
                                                   __float_as_uint(best - t), ab, 0xFE);
  return (uint32_t)((int32_t)any >> 31);
}
// one record pair's loop fields (7 x 16 B) from the LDS cache or the scalar cache
template <bool SMEM>
RT_D void load_pair(const DevScene& sc, const F4* lrec, int p, v4f r[7]) {
  if (SMEM) {
    typedef __attribute__((address_space(4))) const v4f cst_v4;
    const cst_v4* q = (const cst_v4*)sc.leafprims + 8 * __builtin_amdgcn_readfirstlane(p);
#pragma unroll
    for (int e = 0; e < 7; ++e) r[e] = q[e];
  } else {
    const lds_v4* q = (const lds_v4*)lrec + 8 * p;
#pragma unroll
    for (int e = 0; e < 7; ++e) r[e] = q[e];
  }
}
// component I of Q, A, B for both records (floats 8-13, 14-19, 20-25 of the pair)
template <int I> RT_D v2f pair_q(const v4f* r) { return I == 0 ? r[2].xy : I == 1 ? r[2].zw : r[3].xy; }
template <int I> RT_D v2f pair_a(const v4f* r) { return I == 0 ? r[3].zw : I == 1 ? r[4].xy : r[4].zw; }
template <int I> RT_D v2f pair_b(const v4f* r) { return I == 0 ? r[5].xy : I == 1 ? r[5].zw : r[6].xy; }
// Axis-aligned pairs (unit normal +-e_AX, A_AX = B_AX = 0; grouped by the host after
// the general pairs).  With n = +-e_AX the general test's n.d is +-d_AX and n.o is
// +-o_AX, and the zero components of n, A and B add exact zeros, so t = (D' - o_AX)
// * rcp(d_AX) with D' = D / n_AX (stored by the host) and alpha, beta over the two
// in-plane axes are the general test's values bit for bit: 10 packed ops per pair
// instead of 20, and one rcp per ray and axis instead of two per pair.
template <int AX, bool SMEM>
RT_D void brute_axis(const DevScene& sc, const F4* lrec, int p0, int p1, const v2f* O,
                     const v2f* Dv, float tmin, float& best, uint32_t& bk) {
  constexpr int B0 = AX == 0 ? 1 : 0, B1 = AX == 2 ? 1 : 2;  // in-plane axes, ascending
  const float da = Dv[AX].x;
  // |n.d| < 1e-8: no hit (NaN), as a sign-mask select (a compare and v_cndmask_b32_e32 on
  // vcc cost ~23 cycles, and_not above)
  const float ia = bitsf(pick_by(fbits(rcp(da)), 0x7FC00000u, neg_mask(fabsf(da) - 1e-8f)));
  const v2f inv = {ia, ia};
  for (int p = p0; p < p1; ++p) {
    v4f r[7];
    load_pair<SMEM>(sc, lrec, p, r);
    const uint32_t k0 = __float_as_uint(r[6].z), k1 = __float_as_uint(r[6].w);
    const v2f t = (r[1].zw - O[AX]) * inv;
    const v2f pb = pfma(Dv[B0], t, O[B0]) - pair_q<B0>(r);
    const v2f pc = pfma(Dv[B1], t, O[B1]) - pair_q<B1>(r);
    const v2f a = pfma(pc, pair_a<B1>(r), pb * pair_a<B0>(r));
    const v2f b = pfma(pc, pair_b<B1>(r), pb * pair_b<B0>(r));
    const uint32_t m0 = rec_reject_t(t.x, tmin, best, a.x, b.x);
    best = bitsf(pick_by(fbits(t.x), fbits(best), m0));
    bk = pick_by(k0, bk, m0);
    const uint32_t m1 = rec_reject_t(t.y, tmin, best, a.y, b.y);
    best = bitsf(pick_by(fbits(t.y), fbits(best), m1));
    bk = pick_by(k1, bk, m1);
  }
}
// A mixed pair: record 2p axis-aligned on A0, record 2p+1 on A1 (A0 < A1; the odd records of
// two axis groups, host-paired; one pair per scene at most).  Each half runs brute_axis's
// arithmetic on its own axis in scalar form -- the same operations on the same operands
// (a packed op is two IEEE fp32 ops), so the same t, alpha, beta bit for bit -- reading the
// ray's components from o and d directly: a packed form gathered {o[A0], o[A1]}, ... into
// ten new registers, which spilled three VGPRs of the record-loop kernel.
template <int I> RT_D float comp(f3 v) { return I == 0 ? v.x : I == 1 ? v.y : v.z; }
template <int A, int H>
RT_D void brute_half(const v4f* r, f3 o, f3 d, float tmin, float& best, uint32_t& bk) {
  constexpr int B0 = A == 0 ? 1 : 0, B1 = A == 2 ? 1 : 2;  // in-plane axes, ascending
  const float da = comp<A>(d);
  // |n.d| < 1e-8: no hit (NaN), as a sign-mask select (a compare and v_cndmask_b32_e32 on
  // vcc cost ~23 cycles, and_not above)
  const float ia = bitsf(pick_by(fbits(rcp(da)), 0x7FC00000u, neg_mask(fabsf(da) - 1e-8f)));
  const float t = ((H ? r[1].w : r[1].z) - comp<A>(o)) * ia;
  const float pb = fmaf(comp<B0>(d), t, comp<B0>(o)) - (H ? pair_q<B0>(r).y : pair_q<B0>(r).x);
  const float pc = fmaf(comp<B1>(d), t, comp<B1>(o)) - (H ? pair_q<B1>(r).y : pair_q<B1>(r).x);
  const float a = fmaf(pc, H ? pair_a<B1>(r).y : pair_a<B1>(r).x, pb * (H ? pair_a<B0>(r).y : pair_a<B0>(r).x));
  const float b = fmaf(pc, H ? pair_b<B1>(r).y : pair_b<B1>(r).x, pb * (H ? pair_b<B0>(r).y : pair_b<B0>(r).x));
  const uint32_t m = rec_reject_t(t, tmin, best, a, b);
  best = bitsf(pick_by(fbits(t), fbits(best), m));
  bk = pick_by(__float_as_uint(H ? r[6].w : r[6].z), bk, m);
}
template <int A0, int A1, bool SMEM>
RT_D void brute_mixed(const DevScene& sc, const F4* lrec, int p, f3 o, f3 d, float tmin,
                      float& best, uint32_t& bk) {
  v4f r[7];
  load_pair<SMEM>(sc, lrec, p, r);
  brute_half<A0, 0>(r, o, d, tmin, best, bk);
  brute_half<A1, 1>(r, o, d, tmin, best, bk);
}
// Pairs parallel to axis AX (host-grouped): n_AX = 0 and A_AX = 0 exactly and B has only
// its AX component (NewBox's side faces after RotateY: v is the vertical edge).  Each
// dropped term of the general test is an exact zero, so den, num, alpha and beta are the
// general test's values (up to the sign of an exact zero): 15 packed ops per pair instead
// of 20.  (r: n.x 0, n.y 1, n.z 2 | Q 2-3 | A 3-4 | B 5-6, as pair_q/a/b)
template <int I> RT_D v2f pair_n(const v4f* r) { return I == 0 ? r[0].xy : I == 1 ? r[0].zw : r[1].xy; }
template <int AX, bool SMEM>
RT_D void brute_vert(const DevScene& sc, const F4* lrec, int p0, int p1, const v2f* O,
                     const v2f* Dv, float tmin, float& best, uint32_t& bk) {
  constexpr int B0 = AX == 0 ? 1 : 0, B1 = AX == 2 ? 1 : 2;  // the other axes, ascending
  for (int p = p0; p < p1; ++p) {
    v4f r[7];
    load_pair<SMEM>(sc, lrec, p, r);
    const uint32_t k0 = __float_as_uint(r[6].z), k1 = __float_as_uint(r[6].w);
    const v2f D = r[1].zw;
    const v2f den = pfma(pair_n<B1>(r), Dv[B1], pair_n<B0>(r) * Dv[B0]);
    const v2f num = D - pfma(pair_n<B1>(r), O[B1], pair_n<B0>(r) * O[B0]);
    const v2f t = num * v2f{rcp(den.x), rcp(den.y)};
    const v2f pa = pfma(Dv[AX], t, O[AX]) - pair_q<AX>(r);
    const v2f p0v = pfma(Dv[B0], t, O[B0]) - pair_q<B0>(r);
    const v2f p1v = pfma(Dv[B1], t, O[B1]) - pair_q<B1>(r);
    const v2f a = pfma(p1v, pair_a<B1>(r), p0v * pair_a<B0>(r));
    const v2f b = pa * pair_b<AX>(r);
    const uint32_t m0 = rec_reject(den.x, t.x, tmin, best, a.x, b.x);
    best = bitsf(pick_by(fbits(t.x), fbits(best), m0));
    bk = pick_by(k0, bk, m0);
    const uint32_t m1 = rec_reject(den.y, t.y, tmin, best, a.y, b.y);
    best = bitsf(pick_by(fbits(t.y), fbits(best), m1));
    bk = pick_by(k1, bk, m1);
  }
}
// Boxes rotated about y (host-detected: six records forming a box, rt_render.hip), two per
// descriptor pair: C.x | C.z | ax/|ax|^2 | az/|az|^2 (x, z) | y range | face slots.  In the
// box's frame (x' = (p - C).ax/|ax|^2, z' likewise, y unchanged) the faces are the planes
// x' = 0 / 1, y = ylo / yhi, z' = 0 / 1, and each face's quad test is t = (k - o'_a) / d'_a:
// the reference's own arithmetic in rotateY.Hit's object frame (transformation.go:94-107,
// objects.go:102-118).  The closest face with t in [tmin, best] is the entering one when
// t_near >= tmin, else the leaving one: one slab test instead of six record tests.  The
// winner is recorded as a box code (pair, half, leaving) and resolved to its face record
// after the loop (box_face).
constexpr uint32_t kBoxCode = 0x40000000u;
template <bool SMEM>
RT_D void brute_box(const DevScene& sc, const F4* lrec, int p0, int p1, const v2f* O,
                    const v2f* Dv, float iy1, float tmin, float& best, uint32_t& bk) {
  const v2f iy = {iy1, iy1};
  for (int p = p0; p < p1; ++p) {
    v4f r[4];
    if (SMEM) {
      typedef __attribute__((address_space(4))) const v4f cst_v4;
      const cst_v4* q = (const cst_v4*)sc.leafprims + 8 * __builtin_amdgcn_readfirstlane(p);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = q[e];
    } else {
      const lds_v4* q = (const lds_v4*)lrec + 8 * p;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = q[e];
    }
    const v2f ex = O[0] - r[0].xy, ez = O[2] - r[0].zw;
    const v2f lx = pfma(ez, r[1].zw, ex * r[1].xy), lz = pfma(ez, r[2].zw, ex * r[2].xy);
    const v2f vx = pfma(Dv[2], r[1].zw, Dv[0] * r[1].xy), vz = pfma(Dv[2], r[2].zw, Dv[0] * r[2].xy);
    const v2f ix = {rcp(vx.x), rcp(vx.y)}, iz = {rcp(vz.x), rcp(vz.y)};
    const v2f tx0 = -lx * ix, tx1 = pfma(-lx, ix, ix);
    const v2f tz0 = -lz * iz, tz1 = pfma(-lz, iz, iz);
    const v2f ty0 = (r[3].xy - O[1]) * iy, ty1 = (r[3].zw - O[1]) * iy;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float ax0 = h ? tx0.y : tx0.x, ax1 = h ? tx1.y : tx1.x;
      const float ay0 = h ? ty0.y : ty0.x, ay1 = h ? ty1.y : ty1.x;
      const float az0 = h ? tz0.y : tz0.x, az1 = h ? tz1.y : tz1.x;
      const float tn = fmaxf(fmaxf(fminf(ax0, ax1), fminf(ay0, ay1)), fminf(az0, az1));
      const float tf = fminf(fminf(fmaxf(ax0, ax1), fmaxf(ay0, ay1)), fmaxf(az0, az1));
      // enter = tn >= tmin; t = enter ? tn : tf; accept = tn <= tf && t >= tmin && t <= best,
      // all as sign masks and v_bitop3 selects (rec_reject)
      const uint32_t leave = neg_mask(tn - tmin);
      const float t = bitsf(pick_by(fbits(tn), fbits(tf), leave));
      const uint32_t rej = (uint32_t)((int32_t)__builtin_amdgcn_bitop3_b32(
                               fbits(tf - tn), fbits(t - tmin), fbits(best - t), 0xFE) >> 31);
      best = bitsf(pick_by(fbits(t), fbits(best), rej));
      bk = pick_by(kBoxCode | ((uint32_t)p << 2) | ((uint32_t)h << 1) | (leave & 1u), bk, rej);
    }
  }
}
// the face record slot of a box code: the plane (of the entering or leaving three) whose
// t is the loop's winning t, recomputed with the loop's operations
template <bool SMEM>
RT_D uint32_t box_face(const DevScene& sc, const F4* lrec, uint32_t code, f3 o, f3 d, float iy,
                       float best) {
  const uint32_t base = 32u * ((code & ~kBoxCode) >> 2) + ((code >> 1) & 1u);
  float f[8];  // C.x, C.z, a.x, a.z, b.x, b.z, ylo, yhi (then the six face slots)
  if (SMEM) {
    const float* g = (const float*)sc.leafprims + base;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = *(const __attribute__((address_space(1))) float*)(g + 2 * e);
  } else {
    const lds_f32* l = (const lds_f32*)lrec + base;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = l[2 * e];
  }
  const float ex = o.x - f[0], ez = o.z - f[1];
  const float lx = fmaf(ez, f[3], ex * f[2]), lz = fmaf(ez, f[5], ex * f[4]);
  const float ix = rcp(fmaf(d.z, f[3], d.x * f[2])), iz = rcp(fmaf(d.z, f[5], d.x * f[4]));
  const float t[6] = {-lx * ix, fmaf(-lx, ix, ix), (f[6] - o.y) * iy, (f[7] - o.y) * iy,
                      -lz * iz, fmaf(-lz, iz, iz)};
  // Entering plane of slab a: the smaller t (ties: the lo plane); leaving: the larger.  The
  // face is the first slab whose plane t is nearest the winning t.  As sign-mask selects and
  // ONE load of the face slot: written with dynamic indices (t[2a + side], f[8 + face]) hipcc
  // loaded all 14 fields and chained ~60 v_cmp / v_cndmask, about 100 VALU on every shading
  // round of the record-loop kernel (a wave almost always has a lane whose hit is a box).
  const uint32_t flip = (code & 1u) ? 0xFFFFFFFFu : 0u;  // leaving: take the larger
  uint32_t slot = 0u;
  float err = kInf;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint32_t m = neg_mask(t[2 * a + 1] - t[2 * a]) ^ flip;  // all ones: the hi plane
    // (fminf: a NaN distance reads as inf, so it never replaces, as with e < err)
    const float e = fminf(fabsf(bitsf(pick_by(fbits(t[2 * a]), fbits(t[2 * a + 1]), m)) - best), kInf);
    const uint32_t nearer = neg_mask(e - err);  // e < err
    slot = pick_by(slot, 2u * (uint32_t)a + (m & 1u), nearer);
    err = bitsf(pick_by(fbits(err), fbits(e), nearer));
  }
  if (SMEM)
    return *(const __attribute__((address_space(1))) uint32_t*)((const float*)sc.leafprims + base +
                                                                 2 * (8 + slot));
  return ((const lds_u32*)lrec)[base + 2 * (8 + slot)];
}
// SHAPE: 0 = any layout, the group bounds read from the scene's parameters; else the
// listed layout brute_shape(SHAPE) (rt_device.h), chosen by the host when the uploaded
// scene's counts equal it: every bound below is then a constant, so the group loops
// disappear, every record address is an immediate offset from the record base, and the
// pairs' loads and tests are one straight block that the scheduler interleaves ahead of
// the ordered best / bk selects.  Same operations on the same operands in the same record
// order either way: the same hits bit for bit.
// EARLY (a listed SHAPE in LDS only): the loop's winning t and bk are handed back as they are,
// tr.best = {t, -, -, bk}, and the caller resolves the winner (brute_resolve_early) beside its
// Philox draw.
template <uint32_t FT, bool SMEM, int SHAPE = 0, bool EARLY = false>
RT_D void trav_brute(const DevScene& sc, const F4* lrec, f3 o, f3 d, float time, float tmin,
                     Trav& tr) {
  static_assert(!HAS(FT_SPHERE | FT_TRI), "record loop: quad-only feature sets");
  static_assert(SHAPE >= 0 && SHAPE < kBruteShapeCount, "record loop: unlisted shape");
  // generic: the group bounds re-read from the kernel-argument segment on every call
  // (kparams): held in SGPRs across the kernel's loop they were spilled to VGPR lanes, ~15
  // v_readlane per segment in the loops' prologues
  const cst_params* kp = SHAPE == 0 ? kparams() : nullptr;
  BruteCounts bc = brute_shape(SHAPE);
  if constexpr (SHAPE == 0) {
    bc.ax[0] = kp->sc.brute_ax[0], bc.ax[1] = kp->sc.brute_ax[1], bc.ax[2] = kp->sc.brute_ax[2];
    bc.vy = kp->sc.brute_vt[1];
    bc.ng = kp->sc.brute_ng;
  }
  const int nax = bc.ax[0], nay = bc.ax[1], naz = bc.ax[2];
  const int nvy = bc.vy;  // y-parallel pairs only (RotateY is the only rotation)
  // general pairs first, then the y-parallel and the axis-aligned groups
  const int ng = bc.ng;
  const v2f ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
  const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z};
  float best = tr.best.t;
  uint32_t bk = 0xFFFFFFFFu;
  for (int p = 0; p < ng; ++p) {
    v4f r[7];
    load_pair<SMEM>(sc, lrec, p, r);
    // record indices 2p, 2p+1 as stored data: the select takes them from a VGPR
    // (a loop-counter SGPR would need a v_mov first: one constant-bus read per op)
    const uint32_t k0 = __float_as_uint(r[6].z), k1 = __float_as_uint(r[6].w);
    const v2f nx = r[0].xy, ny = r[0].zw, nz = r[1].xy, D = r[1].zw;
    const v2f den = pfma(nz, dz, pfma(ny, dy, nx * dx));
    const v2f num = D - pfma(nz, oz, pfma(ny, oy, nx * ox));
    const v2f t = num * v2f{rcp(den.x), rcp(den.y)};
    const v2f px = pfma(dx, t, ox) - r[2].xy;
    const v2f py = pfma(dy, t, oy) - r[2].zw;
    const v2f pz = pfma(dz, t, oz) - r[3].xy;
    const v2f a = pfma(pz, r[4].zw, pfma(py, r[4].xy, px * r[3].zw));
    const v2f b = pfma(pz, r[6].xy, pfma(py, r[5].zw, px * r[5].xy));
    const uint32_t m0 = rec_reject(den.x, t.x, tmin, best, a.x, b.x);
    best = bitsf(pick_by(fbits(t.x), fbits(best), m0));
    bk = pick_by(k0, bk, m0);
    const uint32_t m1 = rec_reject(den.y, t.y, tmin, best, a.y, b.y);
    best = bitsf(pick_by(fbits(t.y), fbits(best), m1));
    bk = pick_by(k1, bk, m1);
  }
  const v2f O[3] = {ox, oy, oz}, Dv[3] = {dx, dy, dz};
  const int q = ng + nvy;
  brute_vert<1, SMEM>(sc, lrec, ng, q, O, Dv, tmin, best, bk);
  brute_axis<0, SMEM>(sc, lrec, q, q + nax, O, Dv, tmin, best, bk);
  brute_axis<1, SMEM>(sc, lrec, q + nax, q + nax + nay, O, Dv, tmin, best, bk);
  brute_axis<2, SMEM>(sc, lrec, q + nax + nay, q + nax + nay + naz, O, Dv, tmin, best, bk);
  const int qm = q + nax + nay + naz, mx = SHAPE == 0 ? kp->sc.brute_mx : bc.mx;  // the mixed pair (0 or 1)
  if (mx == (1 | (2 << 2))) brute_mixed<0, 1, SMEM>(sc, lrec, qm, o, d, tmin, best, bk);
  else if (mx == (1 | (3 << 2))) brute_mixed<0, 2, SMEM>(sc, lrec, qm, o, d, tmin, best, bk);
  else if (mx == (2 | (3 << 2))) brute_mixed<1, 2, SMEM>(sc, lrec, qm, o, d, tmin, best, bk);
  const int qb = qm + (mx != 0 ? 1 : 0);
  const float iy = rcp(d.y);
  brute_box<SMEM>(sc, lrec, qb, qb + (SHAPE == 0 ? kp->sc.brute_box : bc.box), O, Dv, iy, tmin, best, bk);
  if constexpr (EARLY) {
    static_assert(SHAPE != 0 && !SMEM, "early draw: the listed shapes in LDS only");
    tr.best.t = best;  // (no winner: the t it came with)
    tr.best.ref = bk;
    tr.cur = TRAV_DONE;
    return;
  }
  if (bk != 0xFFFFFFFFu) {
    if (bk & kBoxCode) bk = box_face<SMEM>(sc, lrec, bk, o, d, iy, best);
    // the winner's fields (pair bk/2, half bk&1): Q at floats 8/10/12, A at
    // 14/16/18, B at 20/22/24, ref at 28 (+ half)
    const uint32_t base = 32u * (bk >> 1) + (bk & 1u);
    float f[10];
    if (SMEM) {
      const float* g = (const float*)sc.leafprims + base + 8;
#pragma unroll
      for (int e = 0; e < 10; ++e)
        f[e] = *(const __attribute__((address_space(1))) float*)(g + 2 * e + (e == 9 ? 2 : 0));
    } else {
      const lds_f32* l = (const lds_f32*)lrec + base + 8;
#pragma unroll
      for (int e = 0; e < 10; ++e) f[e] = l[2 * e + (e == 9 ? 2 : 0)];
    }
    const float px = fmaf(d.x, best, o.x) - f[0];
    const float py = fmaf(d.y, best, o.y) - f[1];
    const float pz = fmaf(d.z, best, o.z) - f[2];
    tr.best.t = best;
    tr.best.u = fmaf(pz, f[5], fmaf(py, f[4], px * f[3]));
    tr.best.v = fmaf(pz, f[8], fmaf(py, f[7], px * f[6]));
    tr.best.ref = __float_as_uint(f[9]);
  }
  tr.cur = TRAV_DONE;
}
// The winner of trav_brute<.., EARLY> resolved to its slot and ref without a branch: every
// lane reads, so the loads are one straight block that the scheduler can start ahead of the
// caller's Philox rounds.  A lane whose winner is no box reads the first box pair's half 0 (a
// valid address) and drops the face by a mask select; a lane without a winner reads slot 0 and
// the caller drops its ref.  For the lanes that keep them: trav_brute's operations on the same
// operands.  ref_raw is some quad's ref on every lane (a row of the shade table).
template <int SHAPE>
RT_D uint32_t brute_resolve_early(const DevScene& sc, const F4* lrec, uint32_t bk, f3 o, f3 d,
                                  float best, uint32_t& ref_raw) {
  constexpr BruteCounts bc = brute_shape(SHAPE);
  const uint32_t none = (uint32_t)((int32_t)bk >> 31);  // all ones: no winner (slots and box codes: bit 31 clear)
  uint32_t slot = and_not(bk, none);
  if constexpr (bc.box > 0) {
    constexpr uint32_t qb = (uint32_t)(bc.ng + bc.vy + bc.ax[0] + bc.ax[1] + bc.ax[2] + (bc.mx != 0 ? 1 : 0));
    const uint32_t box = and_not((uint32_t)((int32_t)(bk << 1) >> 31), none);  // all ones: a box code
    const uint32_t code = pick_by(kBoxCode | (qb << 2), bk, box);
    slot = pick_by(slot, box_face<false>(sc, lrec, code, o, d, rcp(d.y), best), box);
  }
  ref_raw = ((const lds_u32*)lrec)[32u * (slot >> 1) + (slot & 1u) + 28u];
  return slot;
}
// quad.Hit's alpha and beta of the winner in `slot` (trav_brute's resolve): the early-draw
// kernel needs them for the debug trace only
RT_D void brute_slot_uv(const F4* lrec, uint32_t slot, f3 o, f3 d, float best, float& u, float& v) {
  const lds_f32* l = (const lds_f32*)lrec + 32u * (slot >> 1) + (slot & 1u) + 8;
  float f[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) f[e] = l[2 * e];
  const float px = fmaf(d.x, best, o.x) - f[0];
  const float py = fmaf(d.y, best, o.y) - f[1];
  const float pz = fmaf(d.z, best, o.z) - f[2];
  u = fmaf(pz, f[5], fmaf(py, f[4], px * f[3]));
  v = fmaf(pz, f[8], fmaf(py, f[7], px * f[6]));
}

}  // namespace rt
