// rt_gather.hip — k_gather_planes: the one kernel of rt_pipeline_push_shares.  The
// lead device's gather buffer holds every share's block of resolved planes (rt_gather_map.h); one
// launch writes each plane of the configuration, row-interleaved, where the pipeline's stages
// read it.  rt_render_multi's k_deinterleave (rt_multi.hip) does this for one [H][W][3] image; this
// one takes up to eleven planes of one or three floats per pixel in a table that is a kernel
// argument, so it lives in SGPRs and needs no buffer.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_gather_map.h"
#include "rt_hip_util.h"
#include "rt_host_units.h"

namespace rt {

// grid: x the 256-float segments of the widest row (3 W floats), y image rows (strided when H is
// past the grid's limit), z the table's rows.  One lane moves one dword; a block reads and writes
// 1 KiB of consecutive addresses.  No LDS, no atomics.  Every address comes from a clamped index:
// a lane past the row's end reads the row's last float and stores nothing.
__global__ __launch_bounds__(256) void k_gather_planes(const float* __restrict__ gather, const GatherTable t) {
  const GatherPlane pl = t.plane[min(blockIdx.z, t.n_planes - 1u)];
  const uint32_t row_floats = pl.fpp * t.W;
  if (blockIdx.x * 256u >= row_floats) return;  // a one-float plane's row is shorter: the whole block leaves
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  const bool live = x < row_floats;
  const uint32_t xc = min(x, row_floats - 1u);
  for (uint32_t r = blockIdx.y; r < t.H; r += gridDim.y) {
    const float v = gather[gather_src(t, pl, r, xc)];
    if (live) pl.dst[(uint64_t)r * row_floats + xc] = v;
  }
}

int gather_planes_launch(const char* who, const float* gather, const GatherTable& t, hipStream_t stream) {
  if (t.n_planes == 0 || t.W == 0 || t.H == 0 || t.n == 0) return RT_OK;
  if (t.n_planes > (uint32_t)kGatherMaxPlanes || t.n > t.H || t.used > t.stride)
    return set_error(RT_ERR_INVALID, "%s: gather table of %u planes, %u shares of %u rows", who, t.n_planes, t.n, t.H);
  const dim3 grid((3u * t.W + 255u) / 256u, std::min(t.H, 65535u), t.n_planes);
  hipLaunchKernelGGL(k_gather_planes, grid, dim3(256), 0, stream, gather, t);
  HIP_OK(hipGetLastError());
  return RT_OK;
}

}  // namespace rt
