// rt_fused_pick.h — the fused kernels' dispatcher over rt_fused.h's kernel table.  Included by
// rt_render.hip, after k_fused and the `extern template` declarations of the rows other units
// compile, and by tools/fused_dispatch.cpp, which runs it over stand-in kernels on the host.
#pragma once
#include "rt_fused.h"

namespace rt {

// the table's kernel of exactly these template arguments, nullptr when it has no such row
static const void* find_fused(bool lds, uint32_t set, int tree, int shape, int light, bool map, bool early,
                              bool cost = false) {
#define RT_FUSED_FIND(L, F, T, S, G, M, E, C, U)                                                 \
  if (lds == L && set == (F) && tree == T && shape == S && light == G && map == M && early == E && \
      cost == C)                                                                                 \
    return (const void*)k_fused<L, F, T, S, G, M, E, C>;
  RT_FUSED_KERNELS(RT_FUSED_FIND)
#undef RT_FUSED_FIND
  return nullptr;
}

// one record-loop kernel per listed shape, and one per listed shape and lean light kind
#define RT_FUSED_COUNT_SHAPES(L, F, T, S, G, M, E, C, U) +(T == 0 && L && (F) == kFtSets[0] && G == 0 && !M ? 1 : 0)
#define RT_FUSED_COUNT_LIGHTS(L, F, T, S, G, M, E, C, U) +(G != 0 && !E ? 1 : 0)
static_assert(0 RT_FUSED_KERNELS(RT_FUSED_COUNT_SHAPES) == kBruteShapeCount, "kernel table: one kernel per listed shape");
static_assert(0 RT_FUSED_KERNELS(RT_FUSED_COUNT_LIGHTS) == (kBruteShapeCount - 1) * (kLeanLightCount - 1),
              "kernel table: one kernel per listed shape and light kind");
#undef RT_FUSED_COUNT_SHAPES
#undef RT_FUSED_COUNT_LIGHTS

// The kernel of a render (not an active-pixel pass).
// (shape: the lean LDS record loop compiled for a listed record layout, rt_device.h brute_shape;
// a structure without shape kernels takes its generic one)
// (light: the lean LDS record loop's light code compiled for a lean light kind, rt_device.h; the
// listed shapes have such kernels, the generic loop does not: nullptr, the caller takes kind 0)
// (early: the lean light kind's kernel that draws a vertex's numbers before it resolves the
// winner, rt_path.h shade_core<.., EARLY_SHAPE>; nullptr without a light kind)
// (cost: the early-draw kernel's lean-cost twin, k_fused<.., COST>; nullptr without early)
// nullptr too for a tree without a kernel of the set: tree 5 in LDS, tree 2 outside the two
// small sets in LDS, tree 8 outside an RT_BVH8_KERNELS build.  At tree 4 a set without a kernel
// of its own runs the all-features one.
static const void* pick_fused(bool lds, uint32_t set, int tree, int shape = 0, int light = 0,
                              bool early = false, bool cost = false) {
  const void* k = find_fused(lds, set, tree, shape, light, false, early, cost);
  if (k || light != 0 || early || cost) return k;
  if (shape != 0) k = find_fused(lds, set, tree, 0, 0, false, false);
  if (!k && tree == 4) k = find_fused(lds, FT_ALL, 4, 0, 0, false, false);
  return k;
}

// The MAP twin (an active-pixel pass) of the kernel pick_fused(lds, set, tree) returns; nullptr
// where there is none (the opt-in trees 2 and 8)
static const void* pick_fused_map(bool lds, uint32_t set, int tree) {
  return find_fused(lds, set, tree, 0, 0, true, false);
}

}  // namespace rt
