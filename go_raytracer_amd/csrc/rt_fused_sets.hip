// rt_fused_sets.hip — fused-kernel instantiations compiled with their own code-generation
// flags (Makefile: LLVM's iterative-ILP machine scheduler): the ILP rows of rt_fused.h's kernel
// table, where the measurement is.  Everything else is in rt_render.hip.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_fused.h"

namespace rt {
#define RT_FUSED_IN_DEF RT_FUSED_SKIP
#define RT_FUSED_IN_ILP RT_FUSED_INSTANTIATE
#define RT_FUSED_IN_MAP RT_FUSED_SKIP
RT_FUSED_KERNELS(RT_FUSED_BY_UNIT)
}  // namespace rt
