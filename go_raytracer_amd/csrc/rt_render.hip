// rt_render.hip — MI355X kernels and host orchestration of one render.
//
// Replaces the reference's per-pixel loop (camera.go:90-153) and recursive
// estimator rayColor (camera.go:293-331).  Two execution strategies run the
// same per-vertex code (rt_path.h):
//
//  WAVEFRONT — a queue-driven loop of
//   k_extend : closest hit for every queued ray (BVH top staged in LDS, static
//              work split, no atomics) -> SoA hit records
//   k_shade  : one rayColor vertex per queued path; paths that finish a sample
//              regenerate a camera ray in place; survivors are compacted into
//              the next queue by wave ballot + prefix with one atomic per
//              workgroup on a per-XCD counter
//  FUSED — k_fused: persistent threads, one path per lane kept in registers,
//          trace + shade in a loop, finished lanes refilled from a wave-batched
//          chunk counter (ballot + one atomic per >=64 chunks).
// Both end with k_resolve (fixed-point pixel sums -> linear mean RGB), or, for a pass of an
// accumulator, with rt_accum.hip's fold kernel over the same sums.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "rt_hip_util.h"
#include "rt_host_units.h"
#include "rt_path.h"
#include "rt_fused.h"
#include "rt_resolve.h"

namespace rt {

// ------------------------------------------------------------- wavefront ---
// The queue of iteration `it` is kXcd segments; segment x holds cnt[it][x]
// slots at queue[sel][x*P ...].
RT_D uint32_t queue_slot(const Params& P, const uint32_t* q, const uint32_t* cnt, uint32_t i) {
  uint32_t x = 0;
  while (x + 1 < (uint32_t)kXcd && i >= cnt[x]) {
    i -= cnt[x];
    ++x;
  }
  return q[(size_t)x * P.P + i];
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_extend(Params P, int it) {
  __shared__ F4 lnodes[LDS ? 4 * kLdsNodes : 4];
  __shared__ uint32_t lstack[kShortStack * 256];
  const bool recs_lds = LDS && stage_nodes(P, lnodes, 8);
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const TravStack ts = {&lstack[threadIdx.x], P.ostack + gtid, P.stack_cols, kShortStack};
  const uint32_t sel = (uint32_t)it & 1u;
  uint32_t cnt[kXcd];
  uint32_t n = 0;
  for (int x = 0; x < kXcd; ++x) {
    cnt[x] = P.ctr->cnt[it % kMaxIt][x];
    n += cnt[x];
  }
  const uint32_t* q = P.queue[sel];
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t slot = queue_slot(P, q, cnt, i);
    Path s;
    load_path(P, slot, s);
    Hit best;
    trace_world<LDS, FT_ALL>(P.sc, lnodes, recs_lds, ts, s.o, s.d, s.time, 0.001f, best);
    finish_hit<FT_ALL>(P, s, best);
    P.hit[slot] = {best.t, best.u, best.v, bitsf(best.ref)};
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&P.ctr->segments, (unsigned long long)n);
}

__global__ __launch_bounds__(256) void k_shade(Params P, int it) {
  __shared__ uint32_t wave_cnt[4], wave_base[4], block_base;
  stage_perlin(P.sc);
  __syncthreads();
  const uint32_t sel = (uint32_t)it & 1u;
  uint32_t cnt[kXcd];
  uint32_t n = 0;
  for (int x = 0; x < kXcd; ++x) {
    cnt[x] = P.ctr->cnt[it % kMaxIt][x];
    n += cnt[x];
  }
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const uint32_t slot = active ? queue_slot(P, P.queue[sel], cnt, i) : 0u;
  bool alive = false;
  if (active) {
    Path s;
    load_path(P, slot, s);
    const F4 hv = P.hit[slot];
    const Hit h = {hv.x, hv.y, hv.z, fbits(hv.w)};
    const WStack ws = {nullptr, 0};  // the weight stack outlives the launch: HBM only
    const SampleAcc sa = {nullptr};  // every sample straight to its pixel
    int out = shade_core<true, FT_ALL>(P, slot, s, h, ws, sa);
    if (out == OUT_NEED_CHUNK) {
      // static work split: slot s renders chunks s, s+P, s+2P, ... (no atomics)
      const uint32_t c = s.chunk + P.P;
      if (c < P.n_chunks) {
        start_sample<true>(P, slot, s, c, 0);
        out = OUT_ALIVE;
      }
    }
    alive = out == OUT_ALIVE;
  }
  // compaction: wave ballot + prefix, block-level sum, one atomic per block
  const unsigned long long am = __ballot(alive);
  const uint32_t w = threadIdx.x >> 6, lane = lane_id();
  if (lane == 0) wave_cnt[w] = (uint32_t)__popcll(am);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int k = 0; k < 4; ++k) {
      wave_base[k] = tot;
      tot += wave_cnt[k];
    }
    const uint32_t x = blockIdx.x % kXcd;
    block_base = tot ? atomicAdd(&P.ctr->cnt[(it + 1) % kMaxIt][x], tot) : 0u;
  }
  __syncthreads();
  if (alive) {
    const uint32_t x = blockIdx.x % kXcd;
    P.queue[sel ^ 1u][(size_t)x * P.P + block_base + wave_base[w] + prefix_count(am)] = slot;
  }
}

__global__ __launch_bounds__(256) void k_init(Params P) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= P.P) return;
  if (slot < P.n_chunks) {
    Path s;
    start_sample<true>(P, slot, s, slot, 0);
    P.queue[0][slot] = slot;  // segment 0 holds the whole first queue
  }
  if (slot == 0) {
    P.ctr->cnt[0][0] = min(P.P, P.n_chunks);
    P.ctr->chunk_head = P.P;
  }
}

// fixed-point sums -> linear mean RGB; Scale(pixelSamplesScale) camera.go:103
__global__ __launch_bounds__(256) void k_resolve(Params P, float* out, double scale) {
  const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
  if (lp >= P.npix) return;
  const uint32_t f = P.pflags[lp];
  // the fused kernel's per-chunk sums of this pixel (rt_resolve.h, shared with the
  // accumulator's fold kernel)
  unsigned long long cs[3] = {0ull, 0ull, 0ull};
  chunk_record_sums(P, lp, cs);
  for (int ch = 0; ch < 3; ++ch) {
    const bool nan = (f & (1u << ch)) != 0, pinf = (f & (8u << ch)) != 0,
               ninf = (f & (64u << ch)) != 0;
    float v;
    if (nan || (pinf && ninf)) {  // Inf + -Inf = NaN, as in the fp64 sum
      v = __builtin_nanf("");
    } else if (pinf || ninf) {
      v = pinf ? kInf : -kInf;
    } else {
      const size_t i = (size_t)ch * P.npix + lp;
      const long long sum = (long long)(P.accum[i] + cs[ch]);
      v = (float)(((double)sum * 2.3283064365386963e-10 + P.side[i]) * scale);
    }
    out[3 * (size_t)lp + ch] = v;
  }
}

// ==================================================================== host ==
struct DeviceScene {
  int device = -1;
  DevicePool pool;              // every array below, freed with the copy
  DevScene d{};                 // nodes = BVH4
  const F4* nodes2 = nullptr;   // BVH2 of the same leaves (tiny scenes)
  const F4* brute_pairs = nullptr;  // quad records in pairs, largest first (record loop)
  size_t brute_slots = 0;           // records in brute_pairs, pads included (even)
  int32_t shade_n = 0;              // F4s of the lean shade table after the pairs (0: none)
  int32_t brute_boxes = 0;          // boxes among them tested as slabs (rt_records.h brute_box)
  int brute_shape = 0;              // the listed layout the pair counts equal (rt_device.h), 0 = none
  int lean_light = 0;               // the light list's lean kind (rt_device.h), 0 = the general code
  LeanLight light_block{};          // ... and its light as the kernel of that kind reads it
  int32_t emitter_slot = -1;        // the early-draw kernel's emitter slot (host_records.cpp), -1 = none
  uint32_t root2 = PRIM_NONE;
  int32_t n_nodes2 = 0;
  const F4* qnodes = nullptr;       // compressed BVH4 (host_qbvh.cpp): 64-B items, root item 0
  size_t qitems = 0;
  std::mutex qmu;                   // ensure_qbvh: the first render that needs it uploads it
  bool q_done = false;
};

struct RenderState {
  int device = -1;
  uint32_t P = 0;
  int depth_cap = 0;
  uint32_t npix = 0;
  Stream own_stream;  // for renders without opts.stream
  DevicePool pool;    // every buffer below
  F4 *ray_o = nullptr, *ray_d = nullptr, *hit = nullptr, *pend = nullptr, *pre = nullptr,
     *stack = nullptr;
  uint2* path = nullptr;
  uint32_t* queue[2] = {nullptr, nullptr};
  Counters* ctr = nullptr;
  unsigned long long* accum = nullptr;
  unsigned long long* csum = nullptr;  // fused: per-chunk sums (4 x u64 per chunk)
  size_t csum_chunks = 0;
  double* side = nullptr;
  uint32_t* pflags = nullptr;
  uint32_t* ostack = nullptr;
  uint32_t ostack_cols = 0;
  float* out = nullptr;
  uint32_t out_cap = 0;
  Events events;       // RT_FLAG_PROFILE (ProfEvents)
  Events prog_events;  // one per progress slice (rt_progress)
  int resident_blocks = 0;
  // the launch parameters' pointers into these buffers (csum: the render has the chunk sums)
  void bind(Params& p, bool use_csum) const {
    p.ray_o = ray_o;
    p.ray_d = ray_d;
    p.hit = hit;
    p.path = path;
    p.pend = pend;
    p.pre = pre;
    p.stack = stack;
    p.queue[0] = queue[0];
    p.queue[1] = queue[1];
    p.ctr = ctr;
    p.accum = accum;
    p.csum = use_csum ? csum : nullptr;
    p.side = side;
    p.pflags = pflags;
    p.ostack = ostack;
    p.stack_cols = ostack_cols;
  }
};

void release_device(Scene* s) {
  DeviceGuard dg;
  release_accums(s);
  release_multi(s);
  std::lock_guard<std::mutex> lk(s->mu);
  for (auto& kv : s->slots) {
    if (kv.second->st) {
      (void)hipSetDevice(kv.first.first);
      delete kv.second->st;
    }
    delete kv.second;
  }
  s->slots.clear();
  for (auto& kv : s->devs) {
    if (kv.second->ds) {
      (void)hipSetDevice(kv.first);
      delete kv.second->ds;
    }
    delete kv.second;
  }
  s->devs.clear();
}

// (the scheduling knobs below, A/B experiments with measured defaults, are tune_int: rt_tune_set
// only, never the process environment, host_tune.cpp)
FastDiv make_fastdiv(uint32_t d) {
  FastDiv f{1u, 0u, 0u, d};
  if (d <= 1) return f;  // d == 1: t = 0, q = n
  const uint32_t l = 32u - (uint32_t)__builtin_clz(d - 1u);
  f.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1u);
  f.s1 = 1u;
  f.s2 = l - 1u;
  return f;
}

// the scene's device copy on `device` (uploaded on first use, then shared by every
// slot on that device; read-only while rendering).  The scene-wide lock covers the
// map lookup only; the upload holds its device's own lock, so first renders on
// different devices upload concurrently.  Called with `device` current.
static int upload_scene(const Scene* s, DeviceScene* ds);
static int ensure_scene(Scene* s, int device, DeviceScene** out) {
  DeviceSlot* slot;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceSlot*& sl = s->devs[device];
    if (!sl) sl = new DeviceSlot();
    slot = sl;
  }
  std::lock_guard<std::mutex> up(slot->mu);
  if (slot->ds) {
    *out = slot->ds;
    return RT_OK;
  }
  DeviceScene* ds = new DeviceScene();
  ds->device = device;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = upload_scene(s, ds);
  if (tune_int("RT_TIMING", 0))
    fprintf(stderr, "[rt] scene upload to device %d %.3f s\n", device,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if (rc != RT_OK) {
    delete ds;
    return rc;
  }
  slot->ds = ds;
  *out = ds;
  return RT_OK;
}
static int upload_scene(const Scene* s, DeviceScene* ds) {
  const HostScene& h = s->h;
  DevScene& d = ds->d;
  const std::vector<DevMaterial> mats = materials_with_uv_flag(h);
  int rc;
  auto upload = [ds](const auto& vec, auto* out) { return ds->pool.upload(vec, out, "scene upload"); };
#define UP(vec, field)                                  \
  if ((rc = upload(vec, &d.field)) != RT_OK) return rc;
  UP(h.sph_cr, sph_cr);
  UP(h.sph_mv, sph_mv);
  UP(h.sph_uv, sph_uv);
  UP(h.quad, quad);
  UP(h.tri, tri);
  UP(h.tri_attr, tri_attr);
  // the BVH4 nodes and the leaf records in ONE allocation (nodes first): the traversal
  // addresses both as 32-bit byte offsets from the node base (rt_trav.h trav_steps)
  std::vector<F4> recs;
  build_leaf_records(h, recs);
  {
    std::vector<F4> tree_buf(h.nodes4);
    tree_buf.resize((tree_buf.size() + 15) / 16 * 16, F4{0, 0, 0, 0});  // records 256-B aligned
    const size_t rec0 = tree_buf.size();
    if ((rec0 + recs.size()) * sizeof(F4) >= ((size_t)1 << 32))
      return set_error(RT_ERR_UNSUPPORTED, "scene: BVH nodes + leaf records exceed 4 GiB");
    tree_buf.insert(tree_buf.end(), recs.begin(), recs.end());
    const F4* base = nullptr;
    if ((rc = upload(tree_buf, &base)) != RT_OK) return rc;
    d.nodes = base;
    d.leafprims = base ? base + rec0 : nullptr;
  }
  // (the compressed BVH4 is built and uploaded on demand: ensure_qbvh)
  const bool small = tiny_scene(h);  // the BVH2 and the record-loop pairs: tiny scenes only
  if (small && (rc = upload(h.nodes, &ds->nodes2)) != RT_OK) return rc;
  ds->root2 = h.root;
  ds->n_nodes2 = small ? (int32_t)(h.nodes.size() / 4) : 0;
  UP(h.refs, refs);
  {
    std::vector<F4> lrecs;
    if (!h.refs8.empty()) {  // the BVH8's records, in its node order
      std::vector<F4> r8(4 * h.refs8.size());
      for (size_t i = 0; i < h.refs8.size(); ++i) make_record(h, h.refs8[i], &r8[4 * i]);
      UP(r8, recs8);
      UP(h.nodes8, nodes8);
    }
    build_light_records(h, lrecs);
    UP(lrecs, light_recs);
  }
  if (small) {  // the record loop's pairs (host_records.cpp), packed once per device upload
    const RecordPack rp = pack_records(h);
    d.brute_ng = rp.counts.ng;
    d.brute_vt[1] = rp.counts.vy;
    for (int a = 0; a < 3; ++a) d.brute_ax[a] = rp.counts.ax[a];
    d.brute_mx = rp.counts.mx;
    d.brute_box = rp.counts.box;
    ds->brute_slots = rp.n_slots;
    ds->shade_n = rp.shade_n;
    ds->brute_boxes = rp.n_boxes;
    ds->brute_shape = rp.shape;
    ds->emitter_slot = rp.emitter_slot;
    if ((rc = upload(rp.pairs, &ds->brute_pairs)) != RT_OK) return rc;
  }
  UP(h.media, media);
  UP(h.medium_refs, medium_refs);
  {  // spheres tested before the BVH (host_flatten: radius >= kBigSphereR), as leaf records
    std::vector<F4> br(4 * h.big_refs.size());
    for (size_t i = 0; i < h.big_refs.size(); ++i) make_record(h, h.big_refs[i], &br[4 * i]);
    UP(br, big_recs);
    d.n_big = (int32_t)h.big_refs.size();
  }
  UP(h.lights, lights);
  UP(mats, mats);
  UP(h.texs, texs);
  UP(h.texels, texels);
  UP(h.images, images);
  UP(h.perlins, perlins);
#undef UP
  d.root = h.root4;
  d.n_nodes = (int32_t)(h.nodes4.size() / 8);
  d.n_media = (int32_t)h.media.size();
  d.medium_draws = h.medium_draws;
  d.n_lights = (int32_t)h.lights.size();
  d.pdf_floor = scene_pdf_floor(h);  // (host_records.cpp)
  d.n_refs = (int32_t)h.refs.size();
  d.n_perlins = (int32_t)h.perlins.size();
  d.shade_lds = -1;  // set per launch (record-loop kernel with the records in LDS)
  d.shade_n = 0;
  d.merge_ok = scene_merge_ok(h);  // (host_records.cpp; the background is checked per render)
  // the lean kernel's light kind and its light block (host_records.cpp), fixed at upload
  ds->lean_light = lean_light_of(h, &ds->light_block);
  return RT_OK;
}

// slot-indexed wavefront buffers (only for WAVEFRONT) + the weight stack,
// counters and pixel accumulators (both modes)
static int ensure_state(SlotState* slot, int device, uint32_t P, int depth_cap, uint32_t npix,
                        bool soa) {
  RenderState* st = slot->st;
  if (st && (st->device != device || st->P < P || st->depth_cap < depth_cap || st->npix < npix ||
             (soa && !st->ray_o))) {
    delete st;
    st = slot->st = nullptr;
  }
  if (st) return RT_OK;
  st = slot->st = new RenderState();
  st->device = device;
  st->P = P;
  st->depth_cap = depth_cap;
  st->npix = npix;
  int rc;
  auto alloc = [st](auto** out, size_t count) { return st->pool.alloc(out, count, "rt_render"); };
  if ((rc = alloc(&st->stack, (size_t)P * depth_cap)) || (rc = alloc(&st->ctr, 1)) ||
      (rc = alloc(&st->accum, 3 * (size_t)npix)) || (rc = alloc(&st->side, 3 * (size_t)npix)) ||
      (rc = alloc(&st->pflags, npix)) ||
      (rc = alloc(&st->out, 3 * (size_t)npix)))
    return rc;
  if (soa &&
      ((rc = alloc(&st->ray_o, P)) || (rc = alloc(&st->ray_d, P)) ||
       (rc = alloc(&st->hit, P)) || (rc = alloc(&st->pend, P)) ||
       (rc = alloc(&st->pre, P)) ||
       (rc = alloc(&st->path, P)) || (rc = alloc(&st->queue[0], (size_t)kXcd * P)) ||
       (rc = alloc(&st->queue[1], (size_t)kXcd * P))))
    return rc;
  return RT_OK;
}

// traversal-stack overflow columns: one per launched traversal thread
static int ensure_ostack(RenderState* st, uint32_t cols) {
  if (st->ostack_cols >= cols) return RT_OK;
  int rc;
  if ((rc = st->pool.free(&st->ostack))) return rc;
  st->ostack_cols = 0;  // (a failed allocation below leaves no columns, not the old count)
  if ((rc = st->pool.alloc(&st->ostack, (size_t)(kStack - kShortStackMin) * cols, "rt_render"))) return rc;
  st->ostack_cols = cols;
  return RT_OK;
}

// *use_csum in: the render wants the chunk sums; out: it has them (st->csum)
// keep: an active-pixel pass neither allocates nor frees: it takes the buffer
// the whole passes left when its chunks fit (a smaller K can give it more chunks than they
// had), and pixel atomics otherwise
static int ensure_csum(RenderState* st, uint32_t n_chunks, bool* use_csum_io, bool keep = false) {
  int rc;
  bool use_csum = *use_csum_io;
  if (keep) {
    *use_csum_io = use_csum && st->csum && st->csum_chunks >= n_chunks;
    return RT_OK;
  }
  // fused: the per-chunk sums (32 B per chunk, every record stored once per render: no clear).
  // The buffer grows with the sample count, not the image: above its cap (RT_CSUM_MAX_MB,
  // default 16 GiB, and at most half of the device's free memory) or when it cannot be
  // allocated, the render falls back to pixel atomics (P.csum == nullptr: the same integer
  // sums, so the same image; rt_stats.chunk_records = 0).  A buffer more than 4x larger than
  // this render needs (and over 256 MiB) is released first.
  {
    const size_t need_b = 32 * (size_t)n_chunks;
    auto drop_csum = [&]() -> int {
      st->csum_chunks = 0;
      return st->pool.free(&st->csum);
    };
    if (st->csum && (!use_csum || (st->csum_chunks > 4 * (size_t)n_chunks &&
                                   32 * st->csum_chunks > ((size_t)256 << 20))))
      if ((rc = drop_csum())) return rc;
    if (use_csum && st->csum_chunks < n_chunks) {
      if ((rc = drop_csum())) return rc;
      size_t free_b = 0, total_b = 0;
      const size_t cap_b = (size_t)std::max(0, tune_int("RT_CSUM_MAX_MB", 16384)) << 20;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
      // (a failed allocation is not an error: pixel atomics instead)
      if (need_b <= cap_b && need_b <= free_b / 2 &&
          st->pool.try_alloc((void**)&st->csum, std::max<size_t>(need_b, 32)))
        st->csum_chunks = n_chunks;
      else
        use_csum = false;
    }
  }
  *use_csum_io = use_csum;
  return RT_OK;
}

static int occupancy_blocks(const void* kernel, int device, int* out, size_t dyn_lds = 0) {
  int per_cu = 0, cus = 0;
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, dyn_lds));
  HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  *out = std::max(1, per_cu) * std::max(1, cus);
  return RT_OK;
}

static_assert(FT_SPHERE == RT_FT_SPHERE && FT_TRI == RT_FT_TRI && FT_METAL == RT_FT_METAL &&
                  FT_DIEL == RT_FT_DIEL && FT_MEDIA == RT_FT_MEDIA && FT_CHECKER == RT_FT_CHECKER &&
                  FT_IMAGE == RT_FT_IMAGE && FT_NOISE == RT_FT_NOISE && FT_BOX == RT_FT_BOX,
              "feature bits: rt_device.h and rt_abi.h disagree");

// the table's rows other units compile (rt_fused_sets.hip, rt_fused_map.hip); this unit's are
// instantiated by the dispatcher
#define RT_FUSED_EXTERN(L, F, T, S, G, M, E, C) extern template __global__ void k_fused<L, F, T, S, G, M, E, C>(Params);
#define RT_FUSED_IN_DEF RT_FUSED_SKIP
#define RT_FUSED_IN_ILP RT_FUSED_EXTERN
#define RT_FUSED_IN_MAP RT_FUSED_EXTERN
RT_FUSED_KERNELS(RT_FUSED_BY_UNIT)

}  // namespace rt
#include "rt_fused_pick.h"
namespace rt {

// The compressed BVH4 of a tree read through L1/L2 (render_impl's tree 5), on `device`
// (current): built on the host once per scene and uploaded once per device, by the first
// render whose kernel can traverse it -- not for LDS-resident trees, record-loop scenes or
// RT_QBVH=0 renders (~85 MB of HBM per GPU for the 1M-triangle mesh otherwise).
static int ensure_qbvh(Scene* s, DeviceScene* ds) {
  std::lock_guard<std::mutex> lk(ds->qmu);
  if (ds->q_done) return RT_OK;
  {
    std::lock_guard<std::mutex> hk(s->qb_mu);
    if (!s->qb_built) {
      std::vector<F4> recs;
      build_leaf_records(s->h, recs);
      int rc = build_qbvh(s->h, recs, &s->qb, &s->qb_items);
      if (rc != RT_OK) return rc;
      s->qb_built = true;
    }
  }
  if (s->qb_items) {
    const int rc = ds->pool.upload(s->qb, &ds->qnodes, "scene upload");
    if (rc != RT_OK) return rc;
    ds->qitems = s->qb_items;
  }
  ds->q_done = true;
  return RT_OK;
}

// The fused kernels' LDS scene-cache budget in 64-B slots at the kernel's waves per SIMD
// (160 KB per CU, less the static stacks), and the structure a fused render of the scene
// traverses before the L1/L2-only refinements (BVH8, compressed BVH4): 0 record loop, 2 BVH2,
// 4 BVH4.  One place for render_impl and the feature pass (aov_view).
static size_t fused_lds_slots(uint32_t ft_set, int tr) {
  return std::min<size_t>(kLdsNodes, (160u * 1024u / (unsigned)fused_waves(ft_set, tr) -
                                      fused_static_lds(ft_set, tr) - 512u) / 64u);
}
static uint32_t scene_ft_set(const Scene* s) {
  // the feature-set kernels read perlin table 0 from LDS only: scenes whose noise
  // textures use other tables run the all-features kernel (generic table pointers)
  const uint32_t feats = s->h.features;
  return (feats & FT_NOISE) && !s->h.noise_table0 ? FT_ALL : pick_ft_set(feats);
}
static int fused_base_tree(const Scene* s, uint32_t ft_set) {
  const size_t n_refs = s->h.refs.size();
  const bool small_set = ft_set == kFtSets[0] || ft_set == kFtSets[1];
  const int env_tree = tune_int("RT_TREE", -1);
  const size_t brute_max = (size_t)tune_int("RT_BRUTE_MAX", kBruteMax);  // A/B override
  const bool fits2 = !s->h.nodes.empty() && s->h.nodes.size() / 4 + n_refs <= fused_lds_slots(ft_set, 2);
  int tree = 4;
  // Record loop vs tree, measured on the Cornell box plus 0-12 extra boxes
  // (tools/brute_sweep.py, profiles/r1_brute_sweep.jsonl): the lockstep loop wins
  // up to ~56 records (18: +33 %, 48: +16 %), reading the records from the LDS
  // cache when they fit (C2 +2 % over scalar loads), with scalar loads otherwise.
  if (small_set && n_refs > 0 && n_refs <= brute_max) tree = 0;
  else if (small_set && n_refs <= 64 && fits2) tree = 2;
  if (small_set && (env_tree == 4 || (env_tree == 2 && fits2))) tree = env_tree;  // A/B override
  return tree;
}
// a BVH4 read through L1/L2 with single-prim leaves takes its compressed form (64-B nodes,
// host_qbvh.cpp) when a kernel of the set exists; RT_QBVH=0: the 128-B nodes (A/B)
static bool wants_qbvh(uint32_t ft_set) {
  return tune_int("RT_QBVH", 1) != 0 && pick_fused(false, ft_set, 5) != nullptr;
}

// What a render of the scene traverses and the fused kernel that does it: one decision for
// render_impl and the feature pass (aov_view), which ignores what it does not need.
struct StructurePlan {
  int tree;          // 0 record loop, 2 BVH2, 4 BVH4, 8 BVH8 (5, the compressed BVH4: take_qbvh)
  bool f_lds;        // the tree's nodes (tree 0: the records) are staged in LDS
  bool f_recs;       // ... and the leaf records after them
  bool shade_tab;    // the lean kernel's shade table goes with the record pairs
  int shape;         // the record layout the kernel is compiled for (rt_device.h brute_shape), 0 = any
  int light;         // the lean light kind its light code is compiled for (rt_device.h), 0 = any list
  bool early;        // ... and that kernel's early-draw variant (the scene has an emitter slot)
  bool cost;         // ... and that variant's lean-cost twin (RT_LEAN_COST)
  const void* kernel;
  size_t lds_bytes;  // dynamic LDS of the kernel
  bool wants_qbvh;   // a BVH4 read through L1/L2 whose set has a compressed-BVH4 kernel
  bool merge_bg;     // plan_kernel: the render's background keeps DevScene::merge_ok (no channel < 0)
};
// no_default_bvh2: an active-pixel pass, whose kernels have no BVH2 twin, takes
// the BVH4 where the BVH2 is the default choice (49..64 leaf entries); RT_TREE=2 still asks for it
static int plan_structure(const Scene* s, const DeviceScene* ds, uint32_t ft_set, int mode,
                          StructurePlan* out, bool no_default_bvh2 = false) {
  // The fused kernel's LDS scene cache (stage_nodes): all BVH nodes, then the
  // leaf records when both fit, within the LDS a workgroup may take at the
  // kernel's target waves per SIMD (160 KB per CU, 24 KB of stacks per group).
  // A tree that does not fit runs the global-node instantiation: caching only
  // its top measured 3-6 % slower on C3-C5 than one node source per kernel.
  // Tree width: the fused kernel traverses the BVH4, except for tiny scenes
  // (<= 64 leaf entries, C2's 18 quads) where the BVH2 measured 3 % faster;
  // the wavefront extend kernel always takes the BVH4.
  // BVH2 kernels exist only for the two smallest feature sets with the tree and
  // its records in LDS (pick_fused): anything else takes the BVH4.
  const size_t n_refs = s->h.refs.size();
  auto slots_for = [&](int tr) { return fused_lds_slots(ft_set, tr); };
  // tree: 0 (no tree: every record tested, <= kBruteMax records in LDS), 2 or 4
  const int env_tree = tune_int("RT_TREE", -1);
  int tree = mode == RT_MODE_FUSED ? fused_base_tree(s, ft_set) : 4;
  if (tree == 0 && !ds->brute_pairs) tree = 4;  // (records not uploaded: RT_BRUTE_MAX raised since)
  if (tree == 2 && !ds->nodes2) tree = 4;
  if (tree == 2 && no_default_bvh2 && env_tree != 2) tree = 4;
  const size_t lds_slots = slots_for(tree);
  const size_t brute_slots = ds->brute_slots;  // record-loop pairs, 2 x 64 B each
  const int smem_env = tune_int("RT_BRUTE_SMEM", -1);
  const bool brute_smem =
      tree == 0 && (smem_env >= 0 ? smem_env != 0 : brute_slots > lds_slots);
  const bool w4 = tree == 4;
  const size_t n_nodes = tree == 4 ? s->h.nodes4.size() / 8 : tree == 2 ? s->h.nodes.size() / 4 : 0;
  const size_t node_slots = w4 ? 2 : 1;  // 64-B LDS slots per node
  const bool f_lds = node_slots * n_nodes <= lds_slots && !brute_smem;
  // the record loop's pairs, then (lean set) the quads' shade table, 4 F4 per 64-B slot
  // The record-loop LDS kernel reads its records from LDS only (trav_brute<.., SMEM = false>),
  // so with a tree 0 in LDS the records must be staged: brute_smem above guarantees they fit
  // alone, and a shade table that would push them over the budget is left out (the lean
  // kernel then shades from the quad table in HBM).  Found in round 6: a 7-wave build shrank
  // the budget below Cornell's records + table, and the kernel read unstaged LDS.
  bool shade_tab = tree == 0 && ft_set == 0u && ds->shade_n > 0;
  if (shade_tab && f_lds && brute_slots + (size_t)(ds->shade_n + 3) / 4 > lds_slots) shade_tab = false;
  const size_t rec_slots = tree == 0 ? brute_slots + (shade_tab ? (size_t)(ds->shade_n + 3) / 4 : 0) : n_refs;
  const bool f_recs = f_lds && node_slots * n_nodes + rec_slots <= lds_slots;
  if (tree == 0 && f_lds && !f_recs)
    return set_error(RT_ERR_UNSUPPORTED, "internal: record loop in LDS without its records");
  // Trees read through L1/L2 take the BVH8 (host_bvh8.cpp) when the scene has one (built
  // only with RT_BVH8=1) and a kernel exists for its feature set; RT_TREE=4 keeps the BVH4
  const bool through_l2 = mode == RT_MODE_FUSED && tree == 4 && !f_lds;
  out->wants_qbvh = through_l2 && wants_qbvh(ft_set);
  if (through_l2 && !s->h.nodes8.empty() && env_tree != 4 && pick_fused(false, ft_set, 8)) tree = 8;
  // The lean LDS record loop compiled for the scene's record layout, when it is a listed one
  // (fixed at upload: the same for every render of the scene).  RT_BRUTE_SHAPE=0: the generic
  // kernel (A/B; the same hits bit for bit).
  const int brute_shape_id = tree == 0 && f_lds && ft_set == kFtSets[0] && tune_int("RT_BRUTE_SHAPE", 1) != 0
                                 ? ds->brute_shape : 0;
  // ... and its light sampling and light pdf compiled for the scene's light list, when that is
  // a lean light kind (fixed at upload too) and the layout's kernel exists for it.  The block
  // is a launch parameter: no LDS, nothing to stage.  RT_LEAN_LIGHT=0: the general light code
  // (A/B; the same image bit for bit).  A render whose background clears merge_ok takes kind 0
  // (plan_kernel).
  int light = tree == 0 && f_lds && ft_set == kFtSets[0] && tune_int("RT_LEAN_LIGHT", 1) != 0
                  ? ds->lean_light : 0;
  if (light != 0 && !pick_fused(f_lds, ft_set, tree, brute_shape_id, light)) light = 0;
  // ... and, for a scene with an emitter slot (fixed at upload) whose shade table is staged, the
  // variant of that kernel that draws each vertex's numbers before it resolves the winner.
  // RT_LEAN_EARLY_DRAW=0: the kernel that draws after (A/B; the same image bit for bit).
  const bool early = light != 0 && ds->emitter_slot >= 0 && shade_tab && f_recs &&
                     tune_int("RT_LEAN_EARLY_DRAW", 1) != 0 &&
                     pick_fused(f_lds, ft_set, tree, brute_shape_id, light, true) != nullptr;
  // ... and that variant's lean-cost twin (DESIGN.md §4 "The cost-weighted census").
  // RT_LEAN_COST=0: the early-draw kernel as it was (A/B; the same image bit for bit).
  const bool cost = early && tune_int("RT_LEAN_COST", 1) != 0 &&
                    pick_fused(f_lds, ft_set, tree, brute_shape_id, light, true, true) != nullptr;
  const void* fused_kernel = pick_fused(f_lds, ft_set, tree, brute_shape_id, light, early, cost);
  if (!fused_kernel) return set_error(RT_ERR_UNSUPPORTED, "internal: no fused kernel for this scene");
  const size_t fused_lds = f_lds ? 64 * (node_slots * n_nodes + (f_recs ? rec_slots : 0)) : 0;
  out->tree = tree;
  out->f_lds = f_lds;
  out->f_recs = f_recs;
  out->shade_tab = shade_tab;
  out->shape = brute_shape_id;
  out->light = light;
  out->early = early;
  out->cost = cost;
  out->kernel = fused_kernel;
  out->lds_bytes = fused_lds;
  return RT_OK;
}
// Trees read through L1/L2 with single-prim leaves take the compressed BVH4 (64-B nodes,
// host_qbvh.cpp): the same closest hits, half the bytes per node step.  RT_QBVH=0: the
// 128-B nodes (A/B)
// The caller's step from "wants the compressed tree" (plan_structure, the tree still 4) to
// "has it" (tree 5): nothing the LDS decisions depend on changes across it, f_lds is false
// either way.
static int take_qbvh(Scene* s, DeviceScene* ds, uint32_t ft_set, StructurePlan* sp) {
  const int rc = ensure_qbvh(s, ds);
  if (rc || !ds->qnodes) return rc;
  sp->tree = 5;
  sp->kernel = pick_fused(false, ft_set, 5);
  return RT_OK;
}

// The kernel a render launches and what it traverses: the scene's structure plan
// (plan_structure) after the steps that depend on the render.  One decision for render_impl, the
// feature pass (aov_view) and the rt_scene_plan_* entries, which use what they need of it.
// background: the camera's (null: non-negative); map: an active-pixel pass.
static int plan_kernel(Scene* s, DeviceScene* ds, uint32_t ft_set, int mode, const double* background,
                       bool map, StructurePlan* sp) {
  int rc;
  if ((rc = plan_structure(s, ds, ft_set, mode, sp, map))) return rc;
  if (sp->tree == 4 && sp->wants_qbvh && (rc = take_qbvh(s, ds, ft_set, sp))) return rc;
  // A lean light kind's kernel holds merge_ok as the constant true: a render whose background
  // clears the flag (fill_params) launches the layout's kernel with the general light code instead
  sp->merge_bg = !background || ((float)background[0] >= 0.0f && (float)background[1] >= 0.0f &&
                                 (float)background[2] >= 0.0f);
  if (sp->light != 0 && !sp->merge_bg) {
    sp->light = 0;
    sp->early = sp->cost = false;
    sp->kernel = pick_fused(sp->f_lds, ft_set, sp->tree, sp->shape, 0);
  }
  if (map) {  // the structure's MAP twin; the record loop's is the generic one (the same bits)
    sp->shape = sp->light = 0;
    sp->early = sp->cost = false;
    sp->kernel = pick_fused_map(sp->f_lds, ft_set, sp->tree);
    if (!sp->kernel)
      return set_error(RT_ERR_UNSUPPORTED, "an active-pixel pass has no kernel for tree %d, chosen by RT_TREE / RT_BVH8", sp->tree);
  }
  return RT_OK;
}

// The DevScene a launch over `tree` reads: the scene's device copy with the tree's nodes and
// records in place (render_impl adds the shade-table fields).
static DevScene scene_for_tree(const DeviceScene* ds, int tree) {
  DevScene sc = ds->d;
  if (tree == 2) {
    sc.nodes = ds->nodes2;
    sc.root = ds->root2;
    sc.n_nodes = ds->n_nodes2;
  } else if (tree == 5) {
    sc.nodes = ds->qnodes;
    sc.root = 0;  // item 0: the root node (trav_init)
    sc.n_nodes = (int32_t)std::min<size_t>(ds->qitems, 0x7FFFFFFF);  // 64-B items
  } else if (tree == 8) {
    sc.root = 0;  // BVH8 node 0 (trav_init)
  } else if (tree == 0) {
    sc.n_nodes = 0;  // records only (stage_nodes puts them at the start of the cache)
    sc.leafprims = ds->brute_pairs;
    sc.n_refs = (int32_t)ds->brute_slots;  // even: whole pairs
  }
  return sc;
}

// The feature pass's view of the scene (rt_internal.h AovView, rt_aov.hip): the tree a fused
// render of it takes and the DevScene set up for it as render_impl sets up Params::sc.
// The BVH8 of RT_BVH8_KERNELS builds is not taken: those scenes' BVH4 (or its compressed
// form) finds the same hits.
int aov_view(Scene* s, int device, AovView* out) {
  DeviceScene* ds = nullptr;
  int rc = ensure_scene(s, device, &ds);
  if (rc) return rc;
  const uint32_t ft_set = scene_ft_set(s);
  StructurePlan sp;
  if ((rc = plan_kernel(s, ds, ft_set, RT_MODE_FUSED, nullptr, false, &sp))) return rc;
  if (sp.tree == 8) {
    sp.tree = 4;
    if (sp.wants_qbvh && (rc = take_qbvh(s, ds, ft_set, &sp))) return rc;
  }
  out->sc = scene_for_tree(ds, sp.tree);
  out->tree = sp.tree;
  return RT_OK;
}

// The camera part of Params (the render's and the feature pass's): the image plane, the
// sample grid, the rank's share of the rows and the seed.
void set_camera_params(Params& p, const rt_camera_derived& cd, const rt_render_opts& o, uint32_t npix) {
  for (int i = 0; i < 3; ++i) {
    p.p00r[i] = (float)(cd.pixel00[i] - cd.center[i]);
    p.du[i] = (float)cd.delta_u[i];
    p.dv[i] = (float)cd.delta_v[i];
    p.cc[i] = (float)cd.center[i];
    p.dku[i] = (float)cd.defocus_u[i];
    p.dkv[i] = (float)cd.defocus_v[i];
    p.bg[i] = (float)cd.background[i];
  }
  p.recip_s = (float)cd.recip_spp_sqrt;
  p.maxc = (float)cd.max_contribution;
  p.s = cd.spp_sqrt;
  p.defocus = cd.defocus_angle > 0 ? 1 : 0;  // camera.go:262
  p.max_depth = cd.max_depth;
  p.width = cd.width;
  p.rank = o.rank;
  p.nranks = o.nranks;
  p.npix = npix;
  p.ss = (uint32_t)cd.spp_sqrt * (uint32_t)cd.spp_sqrt;
  p.seed = o.seed;
  p.fd_width = make_fastdiv((uint32_t)cd.width);
  p.fd_s = make_fastdiv((uint32_t)cd.spp_sqrt);
}
// rows of an H-row image that rank `rank` of `nranks` renders (r % nranks == rank)
uint32_t rank_rows(uint32_t H, int rank, int nranks) {
  return H > (uint32_t)rank ? (H - (uint32_t)rank + nranks - 1) / nranks : 0;
}

// How a render's samples are cut into chunks (rt_camera.h chunk_pixel): K samples per chunk, a
// tail phase of K2-sample chunks after the first S1 samples of every pixel (S1 == ss: none),
// and the row groups the chunks sweep.  P: the fused kernel's lanes (unused otherwise).
struct ChunkPlan {
  uint32_t K, K2, S1;
  uint32_t cpp1;      // first-phase chunks per pixel
  uint32_t n_chunks;
  uint32_t n_groups;  // chunk-order groups of this rank
  FastDiv fd_gpix, fd_gchunks, fd_gchunks2;
};
static int plan_chunks(uint32_t npix, uint32_t rows, uint32_t W, uint32_t ss, uint32_t P, int chunk,
                       uint32_t ft_set, int tree, bool f_lds, int mode, ChunkPlan* out) {
  // Samples per chunk.  Fused: the largest K in {32, 16, 8} (64 for C2's record loop, below)
  // that still gives
  // every lane >= 12 chunks (tree in LDS) or >= 100 (tree through L1/L2, whose
  // per-pixel cost varies more), so the last chunks do not leave most lanes idle.
  // Round 4 (partitioned counters, chunk sums as plain stores): C2's 2-, 4- and 8-GPU
  // shares are fastest at K = 32 / 16 / 16 (16.9 / 8.67 / 4.68 ms; K = 8: 18.2 / 9.03 /
  // 4.91, profiles/r4_chunk_probe_csum.jsonl), which 12 chunks per lane picks; 48 picked
  // 16 / 8 / 8.
  // Measured with the row-group order (tools/chunk_probe.py,
  // profiles/r2_chunk_size_*.jsonl): 8-GPU shares of C2/C3/C4/C5 are fastest at
  // K = 8 (C5 -27 % against 32), whole images at K = 32 (C3 -3 % against 8); at 100
  // C3 takes K = 16 (1.5 % behind 32, which is 14 % behind 8 on C5's 8-GPU share).
  uint32_t K = 32u;
  if (chunk > 0) {
    K = (uint32_t)chunk;
  } else if (mode == RT_MODE_FUSED) {
    // (the mesh set asks 200: the 1M-triangle mesh's 2- / 4- / 8-GPU shares -0.6 / -1.6 /
    // -2.3 % with K halved, its whole image unchanged at K = 32; book1 and book2 gained
    // nothing from it, profiles/r5_model_chunk_share_ab.jsonl, r5_chunk_need200_ab.jsonl)
    // Round 6: book1's set asks 50 and may take K = 24.  Its bar of 100 had been met at K = 16
    // with 4 waves per SIMD; at 5 (round 5) the lanes outnumber it and the rule fell to K = 8:
    // the whole C3 image 72.2 ms at 8, 71.2 at 16, 70.6 at 24, 71.8 at 32; its 2- and 8-GPU
    // shares still get 8 and 4 (profiles/r6_chunk_sweep.jsonl)
    const bool book1_set = ft_set == (FT_SPHERE | FT_TRI | FT_METAL | FT_DIEL | FT_CHECKER);
    const int need_dflt = f_lds ? 12 : ft_set == (FT_SPHERE | FT_TRI | FT_METAL) ? 200 : book1_set ? 50 : 100;
    const uint64_t work = (uint64_t)npix * ss,
                   need = (uint64_t)std::max(1, tune_int("RT_CHUNK_NEED", need_dflt)) * P;
    K = f_lds ? 8u : 4u;  // the smallest: C3's 8-GPU share 6 % faster at 4 than 8 (C2's ±1 %)
    // Round 6: the lean record-loop kernel (C2) also takes K = 64 at the same bar (half as
    // many chunk starts and records; k_resolve reads half the bytes): C2 28.44 -> 27.81 ms
    // on the whole image, its 2-GPU share -0.6 %; its 4-GPU share, 6.5 chunks per lane at 64,
    // keeps 32 (7.56-7.65 against 7.81-7.83 ms at 64, profiles/r6_chunk64_share_ab.jsonl),
    // the 8-GPU share 16 (64: 4.62, 32: 4.39 ms against 4.03), and the tree kernels 32 (64:
    // book1 +4 %, C5 +1.9 %, book2 +0.5 %; profiles/r6_chunk64_probe.jsonl)
    if (tree == 0 && ft_set == 0u && work / 64u >= need) {
      K = 64u;
    } else {
      for (uint32_t k : {32u, 24u, 16u, 8u})
        if ((k != 24u || book1_set) && work / k >= need) {
          K = k;
          break;
        }
    }
  }
  K = std::max<uint32_t>(1u, std::min<uint32_t>(std::min(K, ss), 4096u));
  // Tail phase (fused, default chunk sizes): the last ~1/RT_TAIL_FRAC of every pixel's
  // samples in chunks of K / 4 (min 4), after all first-phase chunks (rt_camera.h chunk_pixel),
  // by default (1/4) when a lane gets fewer than 40 chunks: the multi-GPU shares.  C2's 2-,
  // 4- and 8-GPU shares -1.0 / -4.0 / -2.3 %, the whole image (52 chunks per lane, no tail)
  // +0.5 % with it (profiles/r4_tail_ab.jsonl)
  uint32_t S1 = ss, K2 = K;
  {
    // (not the record-loop kernel: its chunk starts use the one-phase mapping, chunk_ids<true>)
    const bool one_phase = tree == 0 && ft_set == 0u;
    const bool few = mode == RT_MODE_FUSED && !one_phase &&
                     (uint64_t)npix * ss / std::max<uint32_t>(K, 1u) < 40ull * P;
    // default: with the default chunk size only; an explicit RT_TAIL_FRAC also applies to
    // an explicit chunk size (A/B and tests)
    const int tf_env = tune_int("RT_TAIL_FRAC", -1);
    const int tf = tf_env >= 0 ? tf_env : (few && chunk <= 0 ? 4 : 0);
    if (mode == RT_MODE_FUSED && !one_phase && tf > 1 && K >= 8u) {
      K2 = std::max<uint32_t>(1u, (uint32_t)tune_int("RT_TAIL_K", (int)std::max<uint32_t>(4u, K / 4)));
      const uint32_t s1 = (uint32_t)((uint64_t)ss * (uint32_t)(tf - 1) / (uint32_t)tf) / K * K;
      if (s1 > 0 && s1 < ss && K2 < K) S1 = s1;
      else K2 = K;
    }
  }
  const uint32_t cpp1 = S1 / K + (S1 == ss && ss % K ? 1u : 0u);  // no tail: ceil(ss / K)
  const uint32_t cpp2 = S1 < ss ? (ss - S1 + K2 - 1) / K2 : 0u;
  const uint32_t cpp = cpp1 + cpp2;
  const uint64_t n_chunks64 = (uint64_t)npix * cpp;
  if (n_chunks64 >= 0xF0000000ull) return set_error(RT_ERR_UNSUPPORTED, "too many work chunks");
  const uint32_t n_chunks = (uint32_t)n_chunks64;
  {
    // chunk order (chunk_pixel): groups of `grows` of this rank's rows, so the paths in
    // flight start from a band of a few rows instead of the whole image (C5 -10 %,
    // C3 -5 %, C4 -3 %, C2 -1 % against image-wide pixel-fastest chunks; 1, 4 and 16
    // rows measured alike, profiles/r2_chunk_order_ab.jsonl)
    const int env_rows = tune_int("RT_CHUNK_ROWS", -1);
    uint32_t grows = env_rows > 0 ? (uint32_t)env_rows : 4u;
    grows = std::max<uint32_t>(1u, std::min<uint32_t>(grows, std::max<uint32_t>(rows, 1u)));
    while (rows % grows) --grows;  // a divisor of the rank's row count
    const uint32_t gpix = std::max<uint32_t>(1u, grows * W);
    out->fd_gpix = make_fastdiv(gpix);
    out->fd_gchunks = make_fastdiv(gpix * cpp1);
    out->fd_gchunks2 = make_fastdiv(std::max<uint32_t>(1u, gpix * cpp2));
    out->n_groups = rows / grows;
  }
  out->K = K;
  out->K2 = K2;
  out->S1 = S1;
  out->cpp1 = cpp1;
  out->n_chunks = n_chunks;
  return RT_OK;
}

// The fused kernel's scheduling knobs and their measured defaults.
struct SchedPlan {
  int step_budget;
  uint32_t shade_min, grab_min, split_min, parts_log2, gran_log2;
};
static SchedPlan plan_sched(uint32_t ft_set, int tree, bool f_lds, uint32_t K, size_t n_nodes4) {
  SchedPlan sd;
  // Scheduling rounds, measured on the full-size configs (tools/sched_sweep.py,
  // tools/sched_ab.sh, profiles/r1_sched_sweep*.jsonl, r2_sched_ab*.jsonl): trees read
  // through L1/L2 gain from bounded rounds so short rays do not idle behind long ones —
  // 8 steps for large trees (C5 +75 %, C4 +10 % over unbounded), 12 for small ones
  // (C3's 485 spheres: 7 % faster than 8); LDS-resident trees (C2) lose from any bound.
  // Kernels with long shading gain from waiting until enough lanes are ready: 32 for
  // the book2 and all-features sets (C4 -1.2 %), 16 for large trees otherwise (C5 -2 %).
  // Round 5, on the compressed BVH4 (cheaper node steps, 5 waves per SIMD): the mesh
  // scene is fastest at 5 steps and 32 ready lanes (C5 +4.6 % over 8 / 16 at 256 spp;
  // 64 ready lanes halves it), book2 unchanged at 8 / 32 (6 / 32 within 0.1 %), book1 at
  // 12 / 1 (profiles/r5_sched_sweep_q.jsonl) -- then 10 steps for book1: -0.7 % at full size
  // (r5_c3_step_ab.jsonl; 9 to 16 swept at 256 spp, r5_knob_sweeps_q.jsonl)
  const bool big_tree = n_nodes4 >= 1024;
  const bool long_shade = ft_set == FT_ALL || (ft_set & FT_NOISE);
  // (book2 at full size: 7 steps and 40 ready lanes -0.7 % against 8 / 32,
  // profiles/r5_c4_c5_knobs_full.jsonl)
  // (clamped where read, as every scheduling knob: a round without a traversal step would
  // never finish a traversal)
  // (round 6, with the mesh set's 256-chunk batches: 4 steps -0.5 % on C5's whole image, -0.4 /
  // -0.6 % on its 2- / 8-GPU shares against 5; 3 as 4 except the 8-GPU share, 2 +1.5 %; the
  // ready-lane bar 24 as 32, 16 +2.5 %, 40 +2 %; profiles/r6_c5_sched_sweep.jsonl)
  sd.step_budget = std::max(1, tune_int("RT_STEP_BUDGET", f_lds ? (1 << 30) : big_tree ? (long_shade ? 7 : 4) : 10));
  sd.shade_min = (uint32_t)std::max(1, tune_int("RT_SHADE_MIN", f_lds ? 1 : long_shade ? 40 : big_tree ? 32 : 1));
  // chunks per refill of a wave's batch (one returning atomic on the chunk
  // counter each): C2 grab sweep (profiles/r1_grab_sweep.jsonl) 64 -> 128:
  // -4 % at 1-2 ranks' shares; 256 for small chunks: -11 % on the 8-GPU share
  // Round 4, with the 64 partitioned counters below: batches of 32 chunks for the
  // LDS-resident scenes (C2 -1.7 % on the whole image, its 8-GPU share 5.13 ms against
  // 5.22 with 128; profiles/r4_share_probe_grab_v1.jsonl, r4_grab_ab.jsonl), while the
  // scenes that traverse a tree through L1/L2 keep 128 (32 measured C3 +3.7 %, C4 +2.2 %,
  // C5 +2 %: their waves refill more often and spread over more of the image)
  // (round 6: 16 for C2's record loop at any K: its whole image at K = 64 -0.4 % against 32
  // (64 +1 %, 128 +4 %), its 2- / 4-GPU shares -0.9 / -1.3 %, the 8-GPU share ±0;
  // profiles/r6_chunk_sweep.jsonl, r6_grab_sweep_c2_shares.jsonl)
  // (round 6: 256 for the mesh set at any K: C5 -1.0 % on the whole image, -0.5 % on its 2-GPU
  // share; 512 ±0, 1024 +5 %; book2 keeps 128: -0.4 % whole but +0.4 % on its 2-GPU share, and
  // book1 128: 64 +0.7 %, 256 +2 %; profiles/r6_grab_sweep.jsonl)
  const bool mesh_set = ft_set == (FT_SPHERE | FT_TRI | FT_METAL);
  sd.grab_min = (uint32_t)std::max(1, tune_int("RT_GRAB_MIN", f_lds ? (tree == 0 && ft_set == 0u ? 16 : 32) : (K <= 8u || mesh_set) ? 256 : 128));
  {  // drain splitting (k_fused's record-loop kernel): share when >= split_min samples are left
    const int sm = tune_int("RT_SPLIT_MIN", 1);
    sd.split_min = sm > 0 ? (uint32_t)sm : 0xFFFFFFFFu;  // 0: off (no lane has that many)
  }
  // partitioned chunk counters (rt_path.h grab_chunk): 64 partitions interleaved in
  // granules of 256 chunks; progress slices use one counter (their ranges are contiguous)
  sd.parts_log2 = (uint32_t)std::min(6, std::max(0, tune_int("RT_PARTS_LOG2", 6)));
  sd.gran_log2 = (uint32_t)std::min(20, std::max(0, tune_int("RT_GRAN_LOG2", 8)));
  return sd;
}

// RT_FLAG_PROFILE: events around every kernel, as index pairs into st->events
struct ProfEvents {
  RenderState* st;
  bool on;
  int used = 0;
  std::vector<std::pair<int, int>> ext, shade, fused;
  int next(hipEvent_t* e) {
    const int rc = st->events.ensure((size_t)used + 1, hipEventDefault);
    if (rc) return rc;
    *e = st->events.ev[used++];
    return RT_OK;
  }
  int sum_ms(const std::vector<std::pair<int, int>>& v, double* acc) const {
    for (auto& pr : v) {
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, st->events.ev[pr.first], st->events.ev[pr.second]));
      *acc += ms;
    }
    return RT_OK;
  }
};

// The fused strategy: the kernel once, or once per progress slice over consecutive chunk
// ranges with an event after each (the image does not depend on the split).
static int launch_fused(Params& p, RenderState* st, hipStream_t stream, const StructurePlan& sp,
                        int fused_blocks, int slices, ProfEvents& ev) {
  const uint32_t n_chunks = p.n_chunks;
  int rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ev.on) {
    if ((rc = ev.next(&e0)) || (rc = ev.next(&e1))) return rc;
    HIP_OK(hipEventRecord(e0, stream));
  }
  // debug: per-wave start/end clocks (100 MHz), segments and (RT_PHASES builds) phase
  // cycles -> binary file RT_WAVE_TIMES, kWaveRec u64 per wave
  std::string wt_file;
  const char* wt_path = tune_str("RT_WAVE_TIMES", &wt_file) ? wt_file.c_str() : nullptr;
  DeviceBuffer wt;
  const size_t n_waves = (size_t)fused_blocks * 4;
  if (wt_path && *wt_path) {
    if ((rc = wt.grow(kWaveRec * n_waves * sizeof(unsigned long long), "rt_render"))) return rc;
    p.wave_times = (unsigned long long*)wt.p;
  }
  void* args[] = {&p};
  for (int sl = 0; sl < slices; ++sl) {
    if (slices > 1) {  // chunks [n*sl/S, n*(sl+1)/S): the counter starts at the range
      p.n_chunks = (uint32_t)((uint64_t)n_chunks * (sl + 1) / slices);
      if (sl > 0)  // one partition (parts_log2 = 0 with slices): its counter is the head
        HIP_OK(hipMemsetD32Async((hipDeviceptr_t)&st->ctr->part[0],
                                 (int)((uint64_t)n_chunks * sl / slices), 1, stream));
    }
    HIP_OK(hipLaunchKernel(sp.kernel, dim3(fused_blocks), dim3(256), args, sp.lds_bytes, stream));
    HIP_OK(hipGetLastError());
    if (slices > 1) HIP_OK(hipEventRecord(st->prog_events.ev[sl], stream));
  }
  p.n_chunks = n_chunks;
  if (wt.p) {
    std::vector<unsigned long long> h(kWaveRec * n_waves);
    HIP_OK(hipMemcpyAsync(h.data(), wt.p, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    p.wave_times = nullptr;
    if (FILE* f = fopen(wt_path, "wb")) {
      fwrite(h.data(), sizeof(h[0]), h.size(), f);
      fclose(f);
    }
  }
  if (ev.on) {
    HIP_OK(hipEventRecord(e1, stream));
    ev.fused.push_back({ev.used - 2, ev.used - 1});
  }
  return RT_OK;
}

// The wavefront strategy: k_init, then extend + shade per iteration in batches, reading the
// queue lengths back after each batch.  *iterations: extend (= shade) launches.
static int launch_wavefront(Params& p, RenderState* st, hipStream_t stream, const void* extend_kernel,
                            ProfEvents& ev, int* iterations_out) {
  const uint32_t P = p.P, n_chunks = p.n_chunks;
  int rc, iterations = 0;
  hipLaunchKernelGGL(k_init, dim3((P + 255) / 256), dim3(256), 0, stream, p);
  HIP_OK(hipGetLastError());
  uint32_t n_est = std::min(P, n_chunks);
  const int kBatch = 4;
  while (n_est > 0) {
    for (int b = 0; b < kBatch; ++b) {
      if (iterations + 1 >= kMaxIt)
        return set_error(RT_ERR_UNSUPPORTED, "more than %d wavefront iterations", kMaxIt);
      const uint32_t ext_blocks = std::max<uint32_t>(
          1u, std::min<uint32_t>((n_est + 255) / 256, (uint32_t)st->resident_blocks));
      hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
      if (ev.on) {
        if ((rc = ev.next(&e0)) || (rc = ev.next(&e1)) || (rc = ev.next(&e2))) return rc;
        HIP_OK(hipEventRecord(e0, stream));
      }
      int it_arg = iterations;
      void* eargs[] = {&p, &it_arg};
      HIP_OK(hipLaunchKernel(extend_kernel, dim3(ext_blocks), dim3(256), eargs, 0, stream));
      if (ev.on) HIP_OK(hipEventRecord(e1, stream));
      hipLaunchKernelGGL(k_shade, dim3((n_est + 255) / 256), dim3(256), 0, stream, p,
                         iterations);
      if (ev.on) {
        HIP_OK(hipEventRecord(e2, stream));
        ev.ext.push_back({ev.used - 3, ev.used - 2});
        ev.shade.push_back({ev.used - 2, ev.used - 1});
      }
      HIP_OK(hipGetLastError());
      ++iterations;
    }
    uint32_t n_now[kXcd];
    HIP_OK(hipMemcpyAsync(n_now, &st->ctr->cnt[iterations % kMaxIt][0], sizeof n_now,
                          hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    n_est = 0;
    for (int x = 0; x < kXcd; ++x) n_est += n_now[x];
  }
  *iterations_out = iterations;
  return RT_OK;
}

// the wavefront extend kernel stages the BVH4's nodes in LDS
static bool extend_in_lds(const Scene* s) { return s->h.nodes4.size() / 8 <= (size_t)kLdsNodes / 2; }

// rt_stats of a finished render, but for ms_total and tuned (the caller's clock and knob count)
static int fill_stats(rt_stats* stats, const Scene* s, const DeviceScene* ds, const RenderState* st,
                      const Params& p, const StructurePlan& sp, int mode, uint32_t ft_set,
                      uint32_t rows, int iterations, const ProfEvents& ev) {
  const int tree = sp.tree;
  int rc;
  memset(stats, 0, sizeof *stats);
  Counters hc;
  HIP_OK(hipMemcpy(&hc, st->ctr, offsetof(Counters, cnt), hipMemcpyDeviceToHost));
  stats->samples = (uint64_t)p.npix * p.ss;
  stats->segments = hc.segments;
  stats->stack_pushes = hc.pushes;
  stats->overflow_samples = hc.overflow;
  stats->extend_rays = hc.segments;
  stats->shade_rays = hc.segments;
  stats->n_extend_launches = mode == RT_MODE_FUSED ? 0 : iterations;
  stats->n_shade_launches = stats->n_extend_launches;
  stats->iterations = iterations;
  stats->rows = (int32_t)rows;
  stats->mode = mode;
  stats->path_slots = (int32_t)p.P;
  stats->kernel_features = mode == RT_MODE_FUSED ? (int32_t)ft_set : (int32_t)FT_ALL;
  stats->scene_features = (int32_t)s->h.features;
  stats->tree_width = tree;
  stats->chunk_samples = (int32_t)p.K;
  stats->record_boxes = tree == 0 ? ds->brute_boxes : 0;
  stats->chunk_records = p.csum ? 1 : 0;
  stats->lds_scene = mode == RT_MODE_FUSED ? (sp.f_lds ? 1 : 0) : (extend_in_lds(s) ? 1 : 0);
  if (ev.on) {
    if ((rc = ev.sum_ms(ev.ext, &stats->ms_extend)) || (rc = ev.sum_ms(ev.shade, &stats->ms_shade)) ||
        (rc = ev.sum_ms(ev.fused, &stats->ms_fused)))
      return rc;
  }
  return RT_OK;
}


// the scene's render slot `slot_id` on `device`, created on first use
static SlotState* slot_of(Scene* s, int device, int slot_id) {
  std::lock_guard<std::mutex> lk(s->mu);
  SlotState*& sl = s->slots[{device, slot_id}];
  if (!sl) sl = new SlotState();
  return sl;
}

// Where a render's image goes and which of the scene's render slots it runs in.  A caller
// names what it sets.
struct RenderTarget {
  float* host = nullptr;           // the image, copied to host memory
  float* dev = nullptr;            // resolved into this device buffer instead of the slot's own
  int slot_id = 0;                 // 0: rt_render[_device] and passes; 1 + i: share i of rt_render_multi
  const Gather* gather = nullptr;  // the share's hand-off (rt_host_units.h)
  const PassSink* sink = nullptr;  // an accumulator's pass: folded into its sums, not resolved
  const PixelMap* map = nullptr;   // an active-pixel pass
};

// Path slots: the fused kernel's resident lanes, at most opts.path_slots (the chunk plan cuts
// the work by them) ...
static int fused_slots(const StructurePlan& sp, const rt_render_opts& o, int* blocks, uint32_t* P) {
  int rc;
  if ((rc = occupancy_blocks(sp.kernel, o.device, blocks, sp.lds_bytes))) return rc;
  if (o.path_slots > 0) *blocks = std::max(1, std::min(*blocks, (o.path_slots + 255) / 256));
  *P = (uint32_t)*blocks * 256u;
  return RT_OK;
}
// ... or the wavefront queue's length, at most the chunks there are
static uint32_t wavefront_slots(const rt_render_opts& o, uint32_t n_chunks) {
  uint32_t P = o.path_slots > 0 ? (uint32_t)o.path_slots : (1u << 20);
  P = std::max<uint32_t>(256u, std::min<uint32_t>(P, std::max<uint32_t>(n_chunks, 256u)));
  return (P + 255u) & ~255u;
}

// What the plans decide of the launch parameters: the scene as the plan's tree reads it, the
// chunk cut and the scheduling knobs.  After set_camera_params (p.npix).
static int fill_params(Params& p, const DeviceScene* ds, const StructurePlan& sp, const ChunkPlan& cp,
                       const SchedPlan& sd, uint32_t P) {
  p.sc = scene_for_tree(ds, sp.tree);
  if (sp.tree == 0 && sp.shade_tab && sp.f_recs) {  // the shade table follows the pairs, in LDS as in HBM
    p.sc.shade_lds = (int32_t)(4 * ds->brute_slots);
    p.sc.shade_n = ds->shade_n;
  }
  if (!sp.merge_bg) p.sc.merge_ok = 0;
  if (sp.light != 0) {
    if (!p.sc.merge_ok) return set_error(RT_ERR_UNSUPPORTED, "internal: lean light kernel without merge_ok");
    p.ll = ds->light_block;
    if (sp.early) {  // the emitter slot in the block's first spare word (rt_device.h LeanLight)
      const uint32_t es = (uint32_t)ds->emitter_slot;
      memcpy(&p.ll.f[11], &es, 4);
    }
  }
  p.K = cp.K;
  p.K2 = cp.K2;
  p.S1 = cp.S1;
  p.n1 = p.npix * cp.cpp1;
  p.n_chunks = cp.n_chunks;
  p.P = P;
  p.fd_gpix = cp.fd_gpix;
  p.fd_gchunks = cp.fd_gchunks;
  p.fd_gchunks2 = cp.fd_gchunks2;
  p.step_budget = sd.step_budget;
  p.shade_min = sd.shade_min;
  p.grab_min = sd.grab_min;
  p.split_min = sd.split_min;
  p.parts_log2 = sd.parts_log2;
  p.gran_log2 = sd.gran_log2;
  p.wave_times = nullptr;
  p.recs_lds = sp.f_recs ? 1u : 0u;
  return RT_OK;
}

// The order the sweep takes the row groups in (chunk_pixel, k_resolve; images do not
// depend on it): RT_SWEEP = forward (image order, the default) or reverse.  A render's tail
// is the paths still in flight when the chunk pool runs dry, so it depends on which rows
// the sweep ends on: book2's costly bottom rows (fog, the box ground) end its forward sweep,
// and its 2- / 8-GPU shares are 2.3 / 3.2 % faster reversed, while C5 and book1 are 1-6 %
// slower (the sky ends their reverse sweep right after the metal dragon / the sphere field,
// whose long specular paths are then still in flight); no probe of the rows' costs chose
// between them reliably, DESIGN.md §8.  Feature-set kernels only (the record loop maps
// chunks in one phase).  The group of sweep position q is (q ^ gflip) + gbase, compiled in
// only with -DRT_SWEEP_ORDER: even that form, two kernel-argument words and two VALU ops
// per chunk start, measured C4 +0.3 % and C5 +0.5 % in the default order at full size
// (profiles/r6_sweep_table_cost_ab.jsonl; a table lookup the same).
static int sweep_order(Params& p, int mode, uint32_t ft_set, const ChunkPlan& cp) {
#ifdef RT_SWEEP_ORDER
  p.gflip = p.gbase = 0u;
#endif
  std::string v;
  if (tune_str("RT_SWEEP", &v) && v == "reverse") {
#ifdef RT_SWEEP_ORDER
    if (mode == RT_MODE_FUSED && ft_set != 0u && cp.n_groups > 1 && p.npix > 0) {
      p.gflip = ~0u;  // (q ^ ~0) + ng = ng - 1 - q
      p.gbase = cp.n_groups;
    }
#else
    return set_error(RT_ERR_UNSUPPORTED, "RT_SWEEP=reverse needs a library built with -DRT_SWEEP_ORDER");
#endif
  }
  return RT_OK;
}

// opts.trace_out: the device buffer the traced sample's vertices are recorded in (t = -1: a
// vertex the path did not reach); the caller's buffer, freed when the render returns
static int start_trace(Params& p, const rt_render_opts& o, DeviceBuffer* dtrace) {
  if (!(o.trace_out && o.trace_cap > 0)) return RT_OK;
  const int rc = dtrace->grow((size_t)o.trace_cap * 3 * sizeof(F4), "rt_render");
  if (rc) return rc;
  std::vector<float> init((size_t)o.trace_cap * 12, 0.0f);
  for (int v = 0; v < o.trace_cap; ++v) init[12 * v + 7] = -1.0f;
  HIP_OK(hipMemcpy(dtrace->p, init.data(), init.size() * 4, hipMemcpyHostToDevice));
  p.trace = (F4*)dtrace->p;
  p.trace_gpix = (uint32_t)o.trace_pixel;
  p.trace_sample = (uint32_t)o.trace_sample;
  p.trace_cap = o.trace_cap;
  return RT_OK;
}

// ... copied to opts.trace_out after the render
static int read_trace(const rt_render_opts& o, const DeviceBuffer& dtrace) {
  if (!dtrace.p) return RT_OK;
  HIP_OK(hipMemcpy(o.trace_out, dtrace.p, (size_t)o.trace_cap * 3 * sizeof(F4), hipMemcpyDeviceToHost));
  return RT_OK;
}

// the overflow columns of the traversal stacks, one per traversal thread: the fused kernel's
// lanes, or the wavefront extend kernel's resident blocks (asked once per state)
static int ensure_trav_stacks(RenderState* st, int device, int mode, uint32_t P, const void* extend_kernel) {
  int rc;
  if (mode == RT_MODE_WAVEFRONT && st->resident_blocks == 0 &&
      (rc = occupancy_blocks(extend_kernel, device, &st->resident_blocks)))
    return rc;
  return ensure_ostack(st, mode == RT_MODE_FUSED ? P : (uint32_t)st->resident_blocks * 256u);
}

// |v| < 2^31 / ss: the ss-sample fixed-point sum of a pixel stays inside int64 (a pass of an
// accumulator: the sum of all its max_passes passes, ss * max_passes < 2^31)
static float sample_limit(uint32_t ss, const PassSink* sink) {
  return std::nextafter((float)(2147483648.0 / (double)((uint64_t)std::max<uint32_t>(ss, 1u) *
                                                        (sink ? std::max<uint32_t>(sink->max_passes, 1u) : 1u))),
                        0.0f);
}

// the counters and the npix pixels' sums and flags, cleared on the render's stream
static int clear_sums(const RenderState* st, uint32_t npix, hipStream_t stream) {
  HIP_OK(hipMemsetAsync(st->ctr, 0, sizeof(Counters), stream));
  if (npix > 0) {
    HIP_OK(hipMemsetAsync(st->accum, 0, 3 * (size_t)npix * sizeof(unsigned long long), stream));
    HIP_OK(hipMemsetAsync(st->side, 0, 3 * (size_t)npix * sizeof(double), stream));
    HIP_OK(hipMemsetAsync(st->pflags, 0, (size_t)npix * sizeof(uint32_t), stream));
  }
  return RT_OK;
}

// rt_progress of a render in `slices` launches: in the record of the render that claimed it, the
// slot's event per slice with the samples complete when each has fired
static void track_slices(Progress& pr, const RenderState* st, int slices, uint32_t n_chunks) {
  std::lock_guard<std::mutex> lk(pr.mu);
  for (int sl = 0; sl < slices; ++sl) {
    pr.events.push_back((void*)st->prog_events.ev[sl]);
    pr.cum.push_back((uint64_t)((double)pr.total * (double)((uint64_t)n_chunks * (sl + 1) / slices) /
                                (double)n_chunks));
  }
}

// After the launches: the sums resolved to the image (or folded into an accumulator's), the
// image copied where the target wants it, and the stream synchronised.
static int finish_render(const Params& p, const RenderState* st, hipStream_t stream, double scale,
                         int device, const RenderTarget& tg) {
  const uint32_t npix = p.npix;
  int rc;
  float* dst = tg.dev ? tg.dev : st->out;
  if (npix > 0 && tg.sink) {  // an accumulator's pass: folded into its sums, not resolved
    if ((rc = tg.sink->fold(tg.sink->ctx, p, scale, stream))) return rc;
  } else if (npix > 0) {
    hipLaunchKernelGGL(k_resolve, dim3((npix + 255) / 256), dim3(256), 0, stream, p, dst, scale);
    HIP_OK(hipGetLastError());
  }
  if (tg.host && npix > 0)
    HIP_OK(hipMemcpyAsync(tg.host, dst, 3 * (size_t)npix * sizeof(float), hipMemcpyDeviceToHost,
                          stream));
  if (tg.gather && npix > 0)
    HIP_OK(hipMemcpyPeerAsync(tg.gather->dst, tg.gather->dst_device, dst, device,
                              3 * (size_t)npix * sizeof(float), stream));
  HIP_OK(hipStreamSynchronize(stream));
  return RT_OK;
}

// One render on one device: plan (kernel, slots, chunks, scheduling), the slot's buffers, the
// launch parameters, the launches, the image.
static int render_impl(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                       rt_stats* stats, const RenderTarget& tg) {
  if (!scene || !cam) return set_error(RT_ERR_INVALID, "rt_render: null scene/camera");
  rt_render_opts o{};
  if (opts) o = *opts;
  if (o.nranks <= 0) o.nranks = 1;
  if (o.rank < 0 || o.rank >= o.nranks) return set_error(RT_ERR_INVALID, "rt_render: bad rank");
  rt_camera_derived cd;
  int rc = rt_camera_derive(cam, &cd);
  if (rc) return rc;
  auto t_start = std::chrono::steady_clock::now();
  const int32_t tuned = tune_count();  // rt_stats.tuned: knobs off their defaults

  if ((rc = device_ok("rt_render", o.device))) return rc;
  DeviceGuard dg;  // the caller's current device is restored on every return
  HIP_OK(hipSetDevice(o.device));
  Scene* s = &scene->s;
  DeviceScene* ds = nullptr;
  if ((rc = ensure_scene(s, o.device, &ds))) return rc;
  SlotState* slot = slot_of(s, o.device, tg.slot_id);
  std::lock_guard<std::mutex> inflight(slot->mu);  // one render per (scene, device, slot)

  const PixelMap* map = tg.map;
  const uint32_t W = (uint32_t)cd.width, H = (uint32_t)cd.height;
  const uint32_t rows = rank_rows(H, o.rank, o.nranks);
  const uint32_t npix_share = rows * W;
  // an active-pixel pass renders the map's n pixels as an image of its own
  if (map && (!map->pixels || map->n == 0 || map->n > npix_share))
    return set_error(RT_ERR_INVALID, "rt_render: a pixel map of %u of %u pixels", map->n, npix_share);
  const uint32_t npix = map ? map->n : npix_share;
  const uint32_t ss = (uint32_t)cd.spp_sqrt * (uint32_t)cd.spp_sqrt;
  int mode = o.mode;
  if (map && mode == RT_MODE_WAVEFRONT)
    return set_error(RT_ERR_UNSUPPORTED, "an active-pixel pass runs the fused kernel only (mode wavefront)");
  if (mode != RT_MODE_WAVEFRONT && mode != RT_MODE_FUSED) mode = RT_MODE_FUSED;
  const uint32_t ft_set = scene_ft_set(s);

  // the plans: kernel and structure (the feature pass takes the same: aov_view), path slots (the
  // fused kernel's lanes before the chunk cut, the wavefront queue after it), scheduling
  StructurePlan sp;
  if ((rc = plan_kernel(s, ds, ft_set, mode, cd.background, map != nullptr, &sp))) return rc;
  uint32_t P = 0;
  int fused_blocks = 0;
  if (mode == RT_MODE_FUSED && (rc = fused_slots(sp, o, &fused_blocks, &P))) return rc;
  ChunkPlan cp;
  // (a map: one chunk group, chunk_pixel's "G = npix" order over the sorted list)
  if ((rc = plan_chunks(npix, map ? 1u : rows, map ? npix : W, ss, P, o.chunk, ft_set, sp.tree, sp.f_lds, mode, &cp)))
    return rc;
  const uint32_t n_chunks = cp.n_chunks;
  if (mode != RT_MODE_FUSED) P = wavefront_slots(o, n_chunks);
  const SchedPlan sd = plan_sched(ft_set, sp.tree, sp.f_lds, cp.K, s->h.nodes4.size() / 8);

  // the slot's buffers (sized for the whole share with a map too: neither pass reallocates the
  // other's) and the stream
  if ((rc = ensure_state(slot, o.device, P, cd.max_depth + 1, std::max<uint32_t>(npix_share, 1),
                         mode == RT_MODE_WAVEFRONT)))
    return rc;
  RenderState* st = slot->st;
  const void* extend_kernel =
      extend_in_lds(s) ? (const void*)k_extend<true> : (const void*)k_extend<false>;
  if ((rc = ensure_trav_stacks(st, o.device, mode, P, extend_kernel))) return rc;
  bool use_csum = mode == RT_MODE_FUSED && tune_int("RT_CSUM", 1) != 0;
  if ((rc = ensure_csum(st, n_chunks, &use_csum, map != nullptr))) return rc;
  hipStream_t stream = nullptr;
  if ((rc = st->own_stream.pick(o.stream, &stream))) return rc;  // the caller's, or the slot's own

  Params p{};
  set_camera_params(p, cd, o, npix);
  if ((rc = fill_params(p, ds, sp, cp, sd, P)) || (rc = sweep_order(p, mode, ft_set, cp))) return rc;
  st->bind(p, use_csum);
  p.pixmap = map ? map->pixels : nullptr;
  p.vlim = sample_limit(ss, tg.sink);
  DeviceBuffer dtrace;
  if ((rc = start_trace(p, o, &dtrace))) return rc;
  ProfEvents ev{st, (o.flags & RT_FLAG_PROFILE) != 0};

  if ((rc = clear_sums(st, npix, stream))) return rc;
  // rt_progress: the fused render as `slices` launches over consecutive chunk
  // ranges, an event after each (the image does not depend on the split)
  const int slices = (mode == RT_MODE_FUSED && n_chunks > 0)
                         ? std::max(1, std::min(o.progress_slices, 1024))
                         : 1;
  if (slices > 1) p.parts_log2 = 0;
  if ((rc = st->prog_events.ensure((size_t)slices, hipEventDisableTiming))) return rc;
  // rt_progress: an rt_render call (slot 0) claims the record when no other render holds it
  // (rt_render_multi claims it for its shares); every return path below releases it
  ProgressDone prog_done{s->prog, tg.slot_id == 0 && claim_progress(s->prog, (uint64_t)npix * ss, o.device)};
  if (prog_done.track && slices > 1) track_slices(s->prog, st, slices, n_chunks);
  int iterations = 0;
  if (n_chunks > 0 && mode == RT_MODE_FUSED) {
    if ((rc = launch_fused(p, st, stream, sp, fused_blocks, slices, ev))) return rc;
    iterations = 1;
  } else if (n_chunks > 0) {
    if ((rc = launch_wavefront(p, st, stream, extend_kernel, ev, &iterations))) return rc;
  }
  if ((rc = finish_render(p, st, stream, cd.pixel_samples_scale, o.device, tg))) return rc;
  prog_done.ok = true;
  auto t_end = std::chrono::steady_clock::now();
  if ((rc = read_trace(o, dtrace))) return rc;
  if (stats) {
    if ((rc = fill_stats(stats, s, ds, st, p, sp, mode, ft_set, rows, iterations, ev))) return rc;
    stats->ms_total = std::chrono::duration<double, std::milli>(t_end - t_start).count();
    stats->tuned = tuned;
  }
  return RT_OK;
}

int render_pass(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts, rt_stats* stats,
                const PassSink* sink, const PixelMap* map) {
  RenderTarget tg;
  tg.sink = sink;
  tg.map = map;
  return render_impl(scene, cam, opts, stats, tg);
}

int render_share(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts, rt_stats* stats,
                 int share, float* out_dev, const Gather* gather) {
  RenderTarget tg;
  tg.slot_id = 1 + share;
  tg.dev = out_dev;
  tg.gather = gather;
  return render_impl(scene, cam, opts, stats, tg);
}

// the device, the scene's copy on it and the scene's structure plan, for the rt_scene_plan_*
// entries: what plan_structure fixes per scene, before a render's background or pixel map
static int scene_plan(const char* who, rt_scene* sc, int device, const void* out, StructurePlan* sp) {
  if (!sc || !out) return set_error(RT_ERR_INVALID, "%s: null", who);
  int rc = device_ok(who, device);
  if (rc) return rc;
  DeviceGuard dg;
  if (hipSetDevice(device) != hipSuccess) return set_error(RT_ERR_DEVICE, "%s", who);
  DeviceScene* ds = nullptr;
  if ((rc = ensure_scene(&sc->s, device, &ds))) return rc;
  return plan_structure(&sc->s, ds, scene_ft_set(&sc->s), RT_MODE_FUSED, sp);
}

}  // namespace rt

extern "C" {

int rt_render(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, float* out_rgb,
              rt_stats* stats) {
  if (!out_rgb) return rt::set_error(RT_ERR_INVALID, "rt_render: null output");
  rt::RenderTarget tg;
  tg.host = out_rgb;
  return rt::render_impl(s, cam, opts, stats, tg);
}

int rt_render_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                     float* out_rgb_device, rt_stats* stats) {
  if (!out_rgb_device) return rt::set_error(RT_ERR_INVALID, "rt_render_device: null output");
  rt::RenderTarget tg;
  tg.dev = out_rgb_device;
  return rt::render_impl(s, cam, opts, stats, tg);
}

int rt_progress(const rt_scene* sc, uint64_t* done, uint64_t* total) {
  if (!sc || !done || !total) return rt::set_error(RT_ERR_INVALID, "rt_progress: null");
  rt::Progress& p = const_cast<rt_scene*>(sc)->s.prog;
  std::lock_guard<std::mutex> lk(p.mu);
  *total = p.total;
  *done = p.done;  // 0 while a render without slices is in flight; multi shares add theirs
  if (!p.busy || p.events.empty()) return RT_OK;
  if (hipSetDevice(p.device) != hipSuccess) return rt::set_error(RT_ERR_DEVICE, "rt_progress");
  for (size_t i = 0; i < p.events.size(); ++i) {  // slices complete in stream order
    if (hipEventQuery((hipEvent_t)p.events[i]) != hipSuccess) break;
    *done = p.cum[i];
  }
  return RT_OK;
}

int rt_scene_plan_light(rt_scene* sc, int device, int32_t* kind) {
  rt::StructurePlan sp;
  const int rc = rt::scene_plan("rt_scene_plan_light", sc, device, kind, &sp);
  if (rc == RT_OK) *kind = sp.light;
  return rc;
}

int rt_scene_plan_early(rt_scene* sc, int device, int32_t* early) {
  rt::StructurePlan sp;
  const int rc = rt::scene_plan("rt_scene_plan_early", sc, device, early, &sp);
  if (rc == RT_OK) *early = sp.early ? 1 : 0;
  return rc;
}

int rt_scene_plan_cost(rt_scene* sc, int device, int32_t* cost) {
  rt::StructurePlan sp;
  const int rc = rt::scene_plan("rt_scene_plan_cost", sc, device, cost, &sp);
  if (rc == RT_OK) *cost = sp.cost ? 1 : 0;
  return rc;
}

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"
