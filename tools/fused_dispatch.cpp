// fused_dispatch.cpp — the fused kernels' dispatcher written out as a table, on the host (no
// GPU, no HIP): for every (lds, set, tree, shape, light, early) over the listed feature sets and
// FT_ALL, trees {0, 2, 4, 5, 8}, shapes 0-2, light kinds 0-1 and early {0, 1}, the kernel
// pick_fused returns, and per (lds, set, tree) the one pick_fused_map returns, named through
// rt_fused.h's kernel table ("-": nullptr).  The real dispatcher (rt_fused_pick.h) runs over
// stand-in kernels, one empty host function per template argument list.
//
//   g++ -std=c++17 -Igo_raytracer_amd/csrc -Iinclude tools/fused_dispatch.cpp -o fused_dispatch
//   ./fused_dispatch > profiles/render_host_stages_dispatch.txt
//
// (-DRT_BVH8_KERNELS: that build's table.)  A change to the table or the dispatcher shows as a
// diff of the recorded output.
#include <stdint.h>
#include <stdio.h>

#define RT_FUSED_TABLE_ONLY
namespace rt {
struct Params {};
template <bool LDS, uint32_t FT, int TREE, int SHAPE = 0, int LIGHT = 0, bool MAP = false, bool EARLY = false,
          bool COST = false>
void k_fused(Params) {}
}  // namespace rt
#include "rt_fused_pick.h"

using namespace rt;

static const char* name_of(const void* k) {
  if (!k) return "-";
#define ROW(L, F, T, S, G, M, E, C, U) \
  if (k == (const void*)k_fused<L, F, T, S, G, M, E, C>)   \
    return C ? "k_fused<" #L ", " #F ", " #T ", " #S ", " #G ", " #M ", " #E ", " #C "> " #U \
             : "k_fused<" #L ", " #F ", " #T ", " #S ", " #G ", " #M ", " #E "> " #U;
  RT_FUSED_KERNELS(ROW)
#undef ROW
  return "NOT IN THE TABLE";
}

int main() {
  const int trees[] = {0, 2, 4, 5, 8};
  for (int lds = 0; lds < 2; ++lds)
    for (uint32_t set : kFtSets)  // the listed sets; the last is FT_ALL
      for (int tree : trees) {
        for (int shape = 0; shape < 3; ++shape)
          for (int light = 0; light < 2; ++light)
            for (int early = 0; early < 2; ++early)
              printf("lds %d set %3u tree %d shape %d light %d early %d : %s\n", lds, set, tree, shape, light,
                     early, name_of(pick_fused(lds != 0, set, tree, shape, light, early != 0)));
        // the early-draw kernel's lean-cost twin (RT_LEAN_COST, the default where it exists)
        for (int shape = 1; shape < 3; ++shape)
          printf("lds %d set %3u tree %d shape %d light 1 early 1 cost 1 : %s\n", lds, set, tree, shape,
                 name_of(pick_fused(lds != 0, set, tree, shape, 1, true, true)));
        printf("lds %d set %3u tree %d map : %s\n", lds, set, tree, name_of(pick_fused_map(lds != 0, set, tree)));
      }
  return 0;
}
