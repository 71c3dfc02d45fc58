// The arithmetic of rt_pipeline_push_shares' gather (go_raytracer_amd/csrc/rt_gather_map.h) on the
// host: for every H in 1..40, n in 1..min(H, 9) and a few widths, with the widest table (eleven
// planes) and the narrowest (two), every image row of every plane is mapped exactly once, to a
// row its share holds, every offset lies inside the gather buffer and inside its own share's block,
// and no two planes overlap.  The "gather buffer" here is a real allocation written through the same
// index function the kernel uses, so an address sanitizer sees an offset that is out of bounds.
// tests/test_gather_map_host.py builds this with -fsanitize=address,undefined and runs it.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "rt_gather_map.h"

using namespace rt;

static int fail(const char* what, uint32_t W, uint32_t H, uint32_t n) {
  fprintf(stderr, "gather map: %s at W=%u H=%u n=%u\n", what, W, H, n);
  return 1;
}

static int check(uint32_t W, uint32_t H, uint32_t n, int n_planes) {
  static const uint32_t fpp[kGatherMaxPlanes] = {3, 1, 3, 3, 1, 3, 1, 1, 3, 3, 1};
  const uint32_t rows_per = gather_rows_per(H, n);
  uint64_t stride = 0;
  for (int j = 0; j < n_planes; ++j) stride += gather_plane_floats(fpp[j], W, rows_per);
  if (rows_per * n < H || (rows_per - 1) * n >= H) return fail("rows_per", W, H, n);
  uint32_t rows_sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t rows = gather_share_rows(H, i, n);
    if (rows < 1 || rows > rows_per) return fail("share rows", W, H, n);
    rows_sum += rows;
  }
  if (rows_sum != H) return fail("the shares' rows do not add up to H", W, H, n);

  GatherTable t;
  gather_begin(&t, W, H, n, stride);
  std::vector<std::vector<float>> dst(n_planes);
  float dummy;
  uint64_t none = 12345;
  if (!gather_add(&t, 3, nullptr, &none) || none != 12345 || t.n_planes != 0 || t.used != 0)
    return fail("a null destination took a row", W, H, n);
  for (int j = 0; j < n_planes; ++j) {
    dst[j].assign((size_t)fpp[j] * W * H, 0.0f);
    uint64_t off = ~0ull;
    if (!gather_add(&t, fpp[j], dst[j].data(), &off)) return fail("gather_add refused a plane that fits", W, H, n);
    if (off != t.plane[j].off || off % kGatherAlignFloats || t.plane[j].fpp != fpp[j])
      return fail("plane offset", W, H, n);
  }
  if (t.used != stride) return fail("the block is not the sum of its planes", W, H, n);
  if (gather_add(&t, 1, &dummy, &none)) return fail("gather_add took a plane past the block's end", W, H, n);

  // the gather buffer: how often each float is read
  std::vector<uint8_t> hits((size_t)n * stride, 0);
  for (int j = 0; j < n_planes; ++j) {
    const GatherPlane& pl = t.plane[j];
    const uint32_t row_floats = pl.fpp * W;
    for (uint32_t r = 0; r < H; ++r) {
      const uint32_t share = r % n, local = r / n;
      if (local >= gather_share_rows(H, share, n)) return fail("a row its share does not hold", W, H, n);
      for (uint32_t x = 0; x < row_floats; ++x) {
        const uint64_t src = gather_src(t, pl, r, x);
        if (src >= hits.size()) return fail("offset outside the gather buffer", W, H, n);
        if (src / stride != share) return fail("offset outside the share's block", W, H, n);
        const uint64_t in_block = src - (uint64_t)share * stride;
        if (in_block < pl.off || in_block >= pl.off + gather_plane_floats(pl.fpp, W, rows_per))
          return fail("offset outside the plane", W, H, n);
        if (hits[src]++) return fail("a float read twice", W, H, n);
        dst[j][(size_t)r * row_floats + x] += 1.0f;
      }
    }
  }
  // every image float written exactly once; exactly the shares' live floats read
  uint64_t live = 0;
  for (int j = 0; j < n_planes; ++j) {
    for (float v : dst[j])
      if (v != 1.0f) return fail("an image float not written exactly once", W, H, n);
    live += (uint64_t)fpp[j] * W * H;
  }
  uint64_t read = 0;
  for (uint8_t h : hits) read += h;
  if (read != live) return fail("floats read", W, H, n);
  return 0;
}

int main() {
  static const uint32_t widths[] = {1, 3, 24, 131};
  int cases = 0;
  for (uint32_t W : widths)
    for (uint32_t H = 1; H <= 40; ++H)
      for (uint32_t n = 1; n <= (H < 9 ? H : 9); ++n)
        for (int n_planes : {2, kGatherMaxPlanes}) {
          if (check(W, H, n, n_planes)) return 1;
          ++cases;
        }
  printf("gather map ok: %d cases\n", cases);
  return 0;
}
