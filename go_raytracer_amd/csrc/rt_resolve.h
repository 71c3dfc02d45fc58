// rt_resolve.h — what one finished render pass left for a pixel, gathered the one way every
// kernel that ends a pass gathers it: k_resolve (rt_render.hip, right below its include) and
// the accumulator's fold kernel (rt_accum.hip).  The library is built without relocatable
// device code, so a device function two translation units call has to live in a header; this
// one holds nothing else, and rt_path.h / rt_fused.h do not see it.
#pragma once
#include "rt_path.h"

namespace rt {

// The fused kernel's per-chunk sums (SampleAcc::flush) of local pixel lp: its chunks are
// q * gchunks + sub * gpix + r for its group q, its place r in the group and every sample
// block sub (chunk_pixel), summed mod 2^64 like the atomics they replace.  cs is added to.
RT_D void chunk_record_sums(const Params& P, uint32_t lp, unsigned long long cs[3]) {
  if (!P.csum) return;
  const uint32_t gpix = P.fd_gpix.d, g = fdiv(lp, P.fd_gpix), r = lp - g * gpix;
#ifdef RT_SWEEP_ORDER
  const uint32_t q = (g ^ P.gflip) + P.gbase;  // the group's sweep position (an involution)
#else
  const uint32_t q = g;
#endif
  for (int ph = 0; ph < 2; ++ph) {  // the first phase's chunks, then the tail's (if any)
    const uint32_t gch = ph ? P.fd_gchunks2.d : P.fd_gchunks.d;
    const uint32_t cpp = ph && P.S1 >= P.ss ? 0u : gch / gpix;
    const unsigned long long* rec = P.csum + 4 * ((ph ? (size_t)P.n1 : 0) + (size_t)q * gch + r);
    // unrolled: eight records' loads in flight per thread before the adds wait (one at a
    // time, the 655 MB of C2's records were read at ~3.5 TB/s)
#pragma unroll 8
    for (uint32_t sb = 0; sb < cpp; ++sb, rec += 4 * (size_t)gpix) {
      cs[0] += rec[0];
      cs[1] += rec[1];
      cs[2] += rec[2];
    }
  }
}

// One channel of a pixel from its exact sum, fp64 side sum and NaN / +Inf / -Inf flag bits
// (f >> ch: bit 0 NaN, bit 3 +Inf, bit 6 -Inf), as the fp64 sum of the samples would give it
RT_D double flagged_channel(uint32_t f, int ch, long long sum, double side, double scale) {
  const bool nan = (f & (1u << ch)) != 0, pinf = (f & (8u << ch)) != 0, ninf = (f & (64u << ch)) != 0;
  if (nan || (pinf && ninf)) return __builtin_nan("");  // Inf + -Inf = NaN, as in the fp64 sum
  if (pinf || ninf) return pinf ? (double)kInf : -(double)kInf;
  return ((double)sum * 2.3283064365386963e-10 + side) * scale;
}

}  // namespace rt
