// rt_fused_map.hip — the fused kernel's MAP twins: the instantiations an active-pixel pass of
// the accumulator launches, in a translation unit of their own so the build
// stays parallel: the MAP rows of rt_fused.h's kernel table; the default scheduler.
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_fused.h"

namespace rt {
#define RT_FUSED_IN_DEF RT_FUSED_SKIP
#define RT_FUSED_IN_ILP RT_FUSED_SKIP
#define RT_FUSED_IN_MAP RT_FUSED_INSTANTIATE
RT_FUSED_KERNELS(RT_FUSED_BY_UNIT)
}  // namespace rt
