// rt_gather_map.h — the arithmetic of rt_pipeline_push_shares' gather, free of HIP
// so that a host program can check it: the layout of a share's block, the plane table
// k_gather_planes takes, and the row map.  Image row r is local row r / n of share r % n
// (camera.go:119-122, rt_render_multi's map).  A share's block holds the configuration's planes one
// after the other, each padded to ceil(H / n) rows and to a 256-byte boundary, so every share's
// block has one layout and the blocks lie `stride` floats apart in the gather buffer; the padding
// rows of a short share are never read.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RT_GATHER_FN __host__ __device__ inline
#else
#define RT_GATHER_FN inline
#endif

namespace rt {

constexpr int kGatherMaxPlanes = 11;         // rgb, var, three emit planes, three chain planes, three first-hit guides
constexpr uint32_t kGatherAlignFloats = 64;  // 256 bytes

struct GatherPlane {
  float* dst;    // the whole image's plane on the lead device, [H][W][fpp]
  uint64_t off;  // of the plane inside a share's block, in floats
  uint32_t fpp;  // floats per pixel: 1 or 3
  uint32_t _pad;
};

struct GatherTable {
  GatherPlane plane[kGatherMaxPlanes];
  uint32_t n_planes;
  uint32_t W, H, n;
  uint32_t rows_per;  // ceil(H / n): the rows every share's planes are padded to
  uint32_t _pad;
  uint64_t used;      // floats of a block the planes added so far take
  uint64_t stride;    // floats from one share's block to the next: at least `used`
};

RT_GATHER_FN uint32_t gather_rows_per(uint32_t H, uint32_t n) { return (H + n - 1) / n; }

// the rows share i of n holds of an H-row image (0 for i >= H)
RT_GATHER_FN uint32_t gather_share_rows(uint32_t H, uint32_t i, uint32_t n) { return i < H ? (H - i + n - 1) / n : 0u; }

// a plane's place in a block: rows_per rows of W pixels, rounded up to the alignment
RT_GATHER_FN uint64_t gather_plane_floats(uint32_t fpp, uint32_t W, uint32_t rows_per) {
  const uint64_t raw = (uint64_t)fpp * W * rows_per;
  return (raw + kGatherAlignFloats - 1) / kGatherAlignFloats * kGatherAlignFloats;
}

RT_GATHER_FN void gather_begin(GatherTable* t, uint32_t W, uint32_t H, uint32_t n, uint64_t stride) {
  t->n_planes = 0;
  t->W = W, t->H = H, t->n = n;
  t->rows_per = gather_rows_per(H, n);
  t->_pad = 0;
  t->used = 0;
  t->stride = stride;
}

// The next plane of the block, gathered into dst; a null dst is no plane of the configuration and
// takes neither a row nor room.  *off: the plane's offset in a block.  False when the table or the
// block is full (the caller sized neither for this plane).
RT_GATHER_FN bool gather_add(GatherTable* t, uint32_t fpp, float* dst, uint64_t* off) {
  if (!dst) return true;
  const uint64_t floats = gather_plane_floats(fpp, t->W, t->rows_per);
  if (t->n_planes >= (uint32_t)kGatherMaxPlanes || t->used + floats > t->stride) return false;
  t->plane[t->n_planes++] = {dst, t->used, fpp, 0u};
  *off = t->used;
  t->used += floats;
  return true;
}

// where float x of image row r of plane `pl` lies in the gather buffer
RT_GATHER_FN uint64_t gather_src(const GatherTable& t, const GatherPlane& pl, uint32_t r, uint32_t x) {
  const uint32_t share = r % t.n, local = r / t.n;
  return (uint64_t)share * t.stride + pl.off + (uint64_t)local * ((uint64_t)pl.fpp * t.W) + x;
}

}  // namespace rt
