// rt_host_units.h — what the host sides of the render (rt_render.hip), the feature pass
// (rt_aov.hip), the accumulator (rt_accum.hip), rt_render_multi (rt_multi.hip), the temporal
// reprojection (rt_temporal.hip), the frame pipeline (rt_pipeline.hip) and its gather kernel
// (rt_gather.hip) declare for one another.  The generic HIP helpers and the resource owners are rt_hip_util.h.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_internal.h"

namespace rt {

// rt_render.hip, shared with the feature pass (rt_aov.hip): the camera part of the launch
// parameters (rt_params.h Params: image plane, sample grid, rank, seed, the width and
// spp_sqrt fast divisions), and the rows of an H-row image that `rank` of `nranks` renders
struct Params;
void set_camera_params(Params& p, const rt_camera_derived& cd, const rt_render_opts& o, uint32_t npix);
uint32_t rank_rows(uint32_t H, int rank, int nranks);

// rt_render.hip, for the accumulator (rt_accum.hip): one render pass of rt_render's own
// path (slot 0, the same plans, launches, buffers and mutex) that hands its sums to a sink
// instead of resolving them.  fold runs where k_resolve would: the pass's launches are
// enqueued on `stream`, p holds what k_resolve reads (accum, csum, side, pflags) and scale is
// pixel_samples_scale; render_pass synchronises the stream after it.  max_passes: a sample
// stays in the exact fixed-point sum below 2^31 / (spp_sqrt^2 * max_passes), so the sum over
// that many passes stays inside int64 (Params::vlim; 1 is rt_render's limit).
struct PassSink {
  uint32_t max_passes;
  int (*fold)(void* ctx, const Params& p, double scale, hipStream_t stream);
  void* ctx;
};
// map (optional): an active-pixel pass over the n sorted local pixels of the
// share listed in `pixels` (device memory).  The pass is then an image of n pixels of its own:
// p.npix = n, p's sums are indexed by the place in the list, the chunk plan is the one of an
// n x 1 image, and the fused kernel's MAP twin runs whatever the mode asks (RT_ERR_UNSUPPORTED
// before any launch for RT_MODE_WAVEFRONT, and for a structure without a twin).
struct PixelMap {
  const uint32_t* pixels;
  uint32_t n;
};
int render_pass(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts, rt_stats* stats,
                const PassSink* sink, const PixelMap* map = nullptr);

// rt_render.hip, for rt_render_multi (rt_multi.hip): share `share` of the image (opts.rank of
// opts.nranks on opts.device) rendered in the scene's slot 1 + share, resolved into out_dev (or
// the slot's own buffer when null) and then, with a gather, handed off: the share's image (rows
// of this rank, [rows][W][3]) is copied to `dst` on device `dst_device` (peer copy over xGMI when
// the devices differ) on the share's stream, before the render returns.
struct Gather {
  float* dst;
  int dst_device;
};
int render_share(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts, rt_stats* stats,
                 int share, float* out_dev, const Gather* gather);

// The accumulator's feature sums, a structure of planes over the npix pixels of
// the share: the per-pass fp32 sums of the feature rays (rt_aov.hip k_aov_fold), added in fp64.
// A group that is not enabled has null pointers.
struct FeatPlanes {
  double* albedo;          // [3][npix]  the RT_ACCUM_FEAT_GUIDES group
  double* normal;          // [3][npix]
  double* depth;           // [npix]
  double* emission;        // [3][npix]  the RT_ACCUM_FEAT_EMIT group
  double* surface_albedo;  // [3][npix]
  uint32_t* nlight;        // [npix]     samples whose first hit is a light's front face (exact)
  uint32_t npix;
};
// rt_aov.hip, for the accumulator (rt_accum.hip): the feature fold of one pass.  aov_fold_begin
// does what can fail without a launch, before the render starts: the scene's aov_view on
// o.device and the overflow-stack scratch for a pass of n_pass pixels; on RT_OK it holds the
// feature pass's mutex until aov_fold_end (after the pass's stream is synchronised).  Between
// the two, aov_fold_enqueue launches k_aov_fold on `stream` for o.seed: the pass's pixel v is
// pixel map[v] of the share (px), or v when map is null.  nscatter (null: off): the media mode
// (RT_ACCUM_FEAT_MEDIA), the sums become first-event sums and the pass's scatter samples are
// counted into nscatter[F.npix]; for a scene without media the plain kernels run.
int aov_fold_begin(rt_scene* scene, const rt_camera_derived& cd, const rt_render_opts& o, uint32_t n_pass);
int aov_fold_enqueue(const FeatPlanes& F, uint32_t* nscatter, bool px, const uint32_t* map, hipStream_t stream);
void aov_fold_end();

// The accumulator's chain sums (RT_ACCUM_FEAT_SPEC): the per-pass fp32 sums of the
// specular chains' terminal normal and summed depth (rt_render_aov_spec's samples), added in fp64,
// and the specular vertices passed as an exact integer (at most 64 a sample: 64 bits hold
// max_passes x spp_sqrt^2 x 64).  max_k and max_fuzz are the chain limits the kernel takes.
struct SpecPlanes {
  double* normal;             // [3][npix]
  double* depth;              // [npix]
  unsigned long long* nspec;  // [npix]
  uint32_t npix;
  int32_t max_k;
  float max_fuzz;
};
// The chain fold of the pass aov_fold_begin prepared, after aov_fold_enqueue on the same stream (the
// two share the overflow stacks): k_aov_spec_fold for the same seed and pixels.
int aov_spec_fold_enqueue(const SpecPlanes& S, bool px, const uint32_t* map, hipStream_t stream);

// rt_accum.hip, for the frame pipeline (rt_pipeline.hip): what a push has to know of the
// accumulator it is handed, copied under the accumulator's lock so that the pipeline keeps no
// pointer into it.  cam is the camera rt_accum_create took; width x rows the share's image;
// stream the one the accumulator's own entries enqueue on (the caller's, else its own, which
// exists once a pass ran; valid for the duration of the call that asked).  Touches no device.
struct AccumView {
  rt_camera cam;
  int32_t width, rows, device, nranks, passes;
  uint32_t features;  // RT_ACCUM_FEAT_*
  void* stream;
  // what rt_pipeline_push_shares compares between the shares of one frame: the share's rank, the
  // whole image's height, the scene, and the chain limits of RT_ACCUM_FEAT_SPEC (0, 0 without it)
  int32_t rank, height;
  const void* scene;
  int32_t spec_bounces;
  float spec_fuzz;
};
int accum_view(rt_accum* a, AccumView* out);

// rt_multi.hip, for the frame pipeline's shares (rt_pipeline.hip): xGMI peer access from -> to
// ("already enabled" is success), and between devices[0] and every other device of a list that
// reports a peer path, which leaves devices[0] current.  who: the entry's name for the message.
int enable_peer(const char* who, int from, int to);
int enable_peers(const char* who, const int32_t* devices, int n);

// rt_gather.hip, for the frame pipeline's shares: one launch of k_gather_planes on `stream` (the
// lead device is current), from the gather buffer into the table's destinations (rt_gather_map.h)
struct GatherTable;
int gather_planes_launch(const char* who, const float* gather, const GatherTable& t, hipStream_t stream);

// rt_temporal.hip, for the frame pipeline (rt_pipeline.hip): what one of the twelve rt_reproject
// entries asks for, as it came in, and the one path they all take.  name: the entry's, for the
// messages; host: the buffers are host memory, staged through device 0 (device and stream are
// not read); moments: an entry of the moments family (_moments, _clip, _spec), which has
// prev_lum2, mopts and out_lum2, clips when copts is given and gates on the chain length when
// spec is.  A struct the entry does not take is NULL, and so, for reproject_impl, is one the mode
// does not take.  The fields stand in the order of rt_reproject_spec_device's parameters.
struct ReprojectRequest {
  const char* name;
  bool host, moments;
  int mode;  // RT_REPROJECT_PLAIN, _EMIT or _LIGHT
  const rt_camera* cam_prev;
  const rt_frame* prev;
  const rt_aov_emit* prev_emit;
  const float* prev_lum2;
  const rt_camera* cam_cur;
  const rt_frame* cur;
  const rt_aov_emit* cur_emit;
  int w, h;
  const rt_reproject_opts* opts;
  const rt_moments_opts* mopts;
  const rt_clip_opts* copts;
  const rt_spec_planes* spec;
  const rt_frame* out;
  const rt_aov_emit* out_emit;
  float* out_lum2;
  int device;
  void* stream;
};
int reproject_impl(const ReprojectRequest& rq);

}  // namespace rt
