// rt_fused_map.hip — the fused kernel's MAP twins: the instantiations an active-pixel pass of
// the accumulator launches, in a translation unit of their own so the build
// stays parallel.  The list is in rt_fused.h (RT_FUSED_MAP_KERNELS); the default scheduler.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_fused.h"

namespace rt {
#define RT_FUSED_INST(L, F, T) template __global__ void k_fused<L, F, T, 0, 0, true>(Params);
RT_FUSED_MAP_KERNELS(RT_FUSED_INST)
#undef RT_FUSED_INST
}  // namespace rt
