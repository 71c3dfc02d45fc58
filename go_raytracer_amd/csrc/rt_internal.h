// rt_internal.h — host-side structures behind the opaque rt_tree / rt_scene handles.
#pragma once
#include <stdint.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "rt_device.h"

namespace rt {

// thread-local error slot (rt_last_error)
int set_error(int code, const char* fmt, ...);

// host_tune.cpp: tuning overrides set by the caller through rt_tune_set (the library never
// reads the process environment).  The value of knob `name`, or `dflt` when it is not set.
bool tune_str(const char* name, std::string* out);
double tune_num(const char* name, double dflt);
int tune_int(const char* name, int dflt);
int32_t tune_count();  // knobs currently set (rt_scene_info.tuned, rt_stats.tuned)

struct Tree {
  // nodes as created; LIST/BVH children live in lists[node.a]
  std::vector<rt_node> nodes;
  std::vector<std::vector<int32_t>> lists;
  std::vector<rt_tri> tris;
  std::vector<rt_material> materials;
  std::vector<rt_texture> textures;
  std::vector<std::vector<uint8_t>> image_data;
  std::vector<rt_image> images;
  std::vector<rt_perlin> perlins;
  uint64_t rng = 0x853c49e6748fea9bull;

  // packed view (rebuilt lazily when dirty)
  bool dirty = true;
  std::vector<rt_node> v_nodes;
  std::vector<int32_t> v_children;

  double rand01();
  int randn(int n);
  void pack();
};

// Host copy of the flattened scene plus its device mirror.
// World spheres this large stay out of the BVH and are tested in fp64 at the start of every
// ray (trav_init): the BVH's sphere leaves are then all small and tested in fp32
constexpr double kBigSphereR = 256.0;
struct HostScene {
  std::vector<F4> sph_cr, sph_mv;
  std::vector<F2> sph_uv;
  std::vector<F4> quad;      // 5 per quad
  std::vector<F4> tri;       // 3 per tri
  std::vector<F4> tri_attr;  // 6 per tri
  std::vector<F4> box_recs;  // 4 per box leaf: the leaf record (rt_device.h), ref in [0].w
  std::vector<F4> nodes;     // BVH2, 4 per node (export / structural tests)
  std::vector<F4> nodes4;    // BVH4 the kernels traverse, 8 per node (rt_device.h)
  uint32_t root4 = PRIM_NONE;
  std::vector<F4> nodes8;    // BVH8, 8 F4 per node, root = node 0 (large scenes, host_bvh8.cpp)
  std::vector<uint32_t> refs8;  // the BVH8's leaf records in node order (prim refs)
  std::vector<uint32_t> refs;
  uint32_t root = PRIM_NONE;
  std::vector<float> prim_bounds;  // 6 per world ref (export/tests)
  std::vector<DevMedium> media;
  std::vector<uint32_t> medium_refs;
  std::vector<uint32_t> big_refs;  // world spheres of radius >= kBigSphereR: tested in fp64
                                   // by every ray before the BVH (not BVH prims)
  int32_t medium_draws = 0;
  std::vector<DevLight> lights;
  std::vector<DevMaterial> mats;
  std::vector<DevTexture> texs;
  std::vector<uint8_t> texels;
  std::vector<DevImage> images;
  std::vector<DevPerlin> perlins;
  int32_t n_world_prims = 0;
  int32_t bvh_depth = 0;
  int32_t max_leaf = 0;
  int32_t bvh_builder = 0;  // 0 host binned SAH, 1 device PLOC
  uint32_t features = 0;    // scene_features(), computed once by rt_scene_create
  bool noise_table0 = true; // every reachable noise texture uses perlin table 0 (scene_features)
  int32_t tuned = 0;        // tuning knobs set when the scene was created (rt_scene_info.tuned)
};

struct DeviceScene;  // defined in the HIP translation units
struct RenderState;
struct MultiState;

// Progress of the tracked render (rt_progress): written by the rendering thread,
// read by any polling thread under `mu`.  One render is tracked at a time: the
// rt_render / rt_render_multi call that finds `busy` clear claims it, and
// only that render updates and clears it, so concurrent renders of one scene on
// other devices neither reset nor finish another render's record.
struct Progress {
  std::mutex mu;
  int busy = 0;                 // 1 while the tracked render is in flight
  int device = -1;
  uint64_t total = 0;           // samples of the current / last render
  uint64_t done = 0;            // samples of the last render once it returned
  std::vector<void*> events;    // hipEvent_t recorded after each slice
  std::vector<uint64_t> cum;    // samples complete when event i has fired
};

// rt_progress follows one render per scene: the rt_render call (slot 0) or rt_render_multi
// call that finds no other render holding the record claims it here, and ProgressDone
// releases it on every return path of the claimant.
inline bool claim_progress(Progress& pr, uint64_t total, int device) {
  std::lock_guard<std::mutex> lk(pr.mu);
  if (pr.busy) return false;
  pr.busy = 1;
  pr.total = total;
  pr.done = 0;
  pr.device = device;
  pr.events.clear();  // no slice events unless the claimant adds them
  pr.cum.clear();
  return true;
}
struct ProgressDone {
  Progress& p;
  bool track;
  bool ok = false;
  ~ProgressDone() {
    if (!track) return;
    std::lock_guard<std::mutex> lk(p.mu);
    if (ok) p.done = p.total;
    p.busy = 0;
  }
};

// Render buffers of one (device, slot): slot 0 serves rt_render / rt_render_device,
// slots 1..n the shares of rt_render_multi (so {0, 0, 0} gets three of them).  The
// mutex is held for the whole render: one render in flight per (scene, device, slot).
struct SlotState {
  std::mutex mu;
  RenderState* st = nullptr;
};

// A device's copy of the scene.  `mu` is held while it is uploaded, so uploads to
// different devices run concurrently (rt_render_multi's share threads), and a
// render on a device whose copy is being uploaded waits for that copy only.
struct DeviceSlot {
  std::mutex mu;
  DeviceScene* ds = nullptr;  // null until the upload succeeded
};

struct Scene {
  HostScene h;
  std::mutex mu;                                    // guards the maps (not the renders)
  std::map<int, DeviceSlot*> devs;                  // per device ordinal, uploaded lazily
  std::map<std::pair<int, int>, SlotState*> slots;  // per (device, slot)
  std::mutex multi_mu;                              // one rt_render_multi at a time
  MultiState* multi = nullptr;                      // its gather buffer and RCCL state (rt_multi.hip)
  Progress prog;
  std::vector<rt_accum*> accums;                    // accumulators alive (rt_accum.hip), under mu
  // the compressed BVH4 (host_qbvh.cpp), built on the host once, at the first render that
  // can traverse it (rt_render.hip ensure_qbvh), then uploaded per device
  std::mutex qb_mu;
  bool qb_built = false;
  std::vector<F4> qb;
  size_t qb_items = 0;
};

// host_flatten.cpp
int flatten_scene(const Tree& t, int world, int lights, HostScene& out);
// host_bvh.cpp
int build_bvh(HostScene& s, const std::vector<F4>& lo, const std::vector<F4>& hi,
              const std::vector<uint32_t>& prims);
// host_bvh8.cpp: the BVH8 of s.nodes (the binary tree) -> s.nodes8 / s.refs8
constexpr size_t kBvh8MinRefs = 1024;
int build_bvh8(HostScene& s);
// host_qbvh.cpp: s's BVH4 as 64-B compressed nodes with the single-prim leaf records inline
// (rt_device.h "compressed BVH4 node"); *n_items = 0 when the tree is not encodable
int build_qbvh(const HostScene& s, const std::vector<F4>& recs, std::vector<F4>* out,
               size_t* n_items);
// host_records.cpp: the traversal's leaf records (rt_device.h "leaf records") in refs order,
// one record, and the light table's entries
void make_record(const HostScene& h, uint32_t ref, F4* r);
void build_leaf_records(const HostScene& h, std::vector<F4>& recs);
void build_light_records(const HostScene& h, std::vector<F4>& recs);
// host_records.cpp: s.mats with the per-material "texture reads u,v" flag in the pad
std::vector<DevMaterial> materials_with_uv_flag(const HostScene& h);
// host_records.cpp: the scene is small enough for the BVH2 and the record-loop pairs to be
// uploaded (RT_BRUTE_MAX, at least 64 leaf entries)
bool tiny_scene(const HostScene& h);
// host_records.cpp: the record loop's pair array (rt_device.h "record-loop pair layout") of a
// tiny scene, as upload_scene copies it to the device; empty (n_slots = 0) for any other
struct RecordPack {
  std::vector<F4> pairs;  // 4 F4 per slot, then the lean kernel's shade table (shade_n F4)
  size_t n_slots = 0;     // records in pairs, pads included (even)
  int32_t shade_n = 0;    // F4s of the shade table after the pairs (0: none)
  int32_t n_boxes = 0;    // boxes among the records tested as slabs (rt_records.h brute_box)
  BruteCounts counts{};   // the layout's group counts (DevScene brute_*)
  int shape = 0;          // brute_shape_of(counts)
  int32_t emitter_slot = -1;  // the slot (the loop's bk) of the scene's one emissive record when
                              // "winner != this slot" is "the hit scatters" (host_records.cpp
                              // emitter_slot_of: a listed shape, lean light kind 1), else -1
};
RecordPack pack_records(const HostScene& h);
// host_records.cpp: DevScene::merge_ok before the render's background is looked at (every
// solid colour and metal albedo >= 0) and DevScene::pdf_floor (1e-30 when every light entry
// is a prim, else 0), fixed at upload
int32_t scene_merge_ok(const HostScene& h);
float scene_pdf_floor(const HostScene& h);
// host_records.cpp: the lean light kind of the scene's light list (rt_device.h "lean light
// kinds", 0 = the general code) and, for a kind >= 1, its light packed into *block (zeroed
// otherwise); computed once per upload, next to pack_records
int lean_light_of(const HostScene& h, LeanLight* block);
// rt_build.hip: the same outputs as build_bvh, built by PLOC on `device` (-1: the calling
// thread's current device; the current device is restored on return)
int build_bvh_device(HostScene& s, const std::vector<F4>& lo, const std::vector<F4>& hi,
                     const std::vector<uint32_t>& prims, int device);
bool bvh_device_available();
// box leaves only in scenes of more world prims than this (counting faces; host_flatten.cpp)
constexpr size_t kBoxLeafMinPrims = 256;
// host_scene.cpp: RT_FT_* features a flattened scene needs
uint32_t scene_features(const HostScene& h, bool* noise_table0 = nullptr);
// rt_render.hip
void release_device(Scene* s);
// rt_accum.hip: frees the accumulators the scene still owns (release_device calls it first)
void release_accums(Scene* s);
// rt_multi.hip: frees rt_render_multi's RCCL state and gather buffer (release_device calls it next)
void release_multi(Scene* s);
// rt_render.hip, for the feature pass (rt_aov.hip): the scene's copy on `device` (the
// calling thread's current device; uploaded on first use) set up for the structure the fused
// render of this scene traverses -- tree 0 record loop, 2 BVH2, 4 BVH4, 5 compressed BVH4
// (built and uploaded on demand), chosen by the render's rules (plan_kernel)
struct AovView {
  DevScene sc;
  int tree;
};
int aov_view(Scene* s, int device, AovView* out);

}  // namespace rt

struct rt_tree {
  rt::Tree t;
};
struct rt_scene {
  rt::Scene s;
};
