// rt_pipeline.hip — rt_pipeline (include/rt_abi.h; DESIGN.md "Frame pipeline"): the owner, on the
// device side of the C ABI, of what the low-sample pipeline keeps between frames.  A push is the
// sequence rt.Temporal.push + the guides' resolve + the spatial filter, restated buffer for buffer
// over the public _device entries and, for the reprojection, the one path they all take
// (rt_temporal.hip's reproject_impl): this unit launches no kernel and has no device code.  Its own
// work is the bookkeeping (which plane lives in which set), two runtime fills and the copies to
// the host.  Device memory comes from rt_hip_util.h's owners only.
// rt_pipeline_push_shares feeds the same stages from a frame held as row shares:
// the stages take a FrameSource, which for shares resolves into a staging block per share, copies
// the blocks to the lead device and has rt_gather.hip's kernel write the planes where the single
// accumulator's resolves would have.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "rt_gather_map.h"
#include "rt_hip_util.h"
#include "rt_host_units.h"

namespace rt {
namespace {

constexpr size_t kAlign = 256;  // every plane starts on a 256-byte boundary of its allocation

// a history set (DESIGN.md "Frame pipeline", the buffer plan): one allocation, carved
struct HistSet {
  DeviceBuffer buf;
  float *rgb = nullptr, *var = nullptr, *count = nullptr, *normal = nullptr, *depth = nullptr;
  float *emission = nullptr, *coverage = nullptr, *lum2 = nullptr, *bounces = nullptr;
  float* image = nullptr;  // the filter's output for the frame whose blend the set holds
};
// the current frame's planes the moments entries may not have as out (the window reads them)
struct CurSet {
  DeviceBuffer buf;
  float *rgb = nullptr, *var = nullptr, *emission = nullptr, *coverage = nullptr;
};
// the filter's guides that are no history plane, and rt_pipeline_ppm's text
struct GuideSet {
  DeviceBuffer buf;
  float *albedo = nullptr, *surface_albedo = nullptr, *normal = nullptr, *depth = nullptr;
  char* ppm = nullptr;
  int64_t ppm_cap = 0;
};

// a share's resolve staging on the share's own device: one block in rt_gather_map.h's layout, and
// the event that follows the block's copy to the lead device (created on the share's device)
struct ShareStage {
  DeviceBuffer buf;
  Events ev;
  int device = -1;
};

// planes of `floats` floats each, one after the other from `base` (null: sizing only)
struct Carver {
  char* base;
  size_t off = 0;
  float* take(size_t floats) { return (float*)take_bytes(floats * sizeof(float)); }
  char* take_bytes(size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + kAlign - 1) / kAlign * kAlign;
    return p;
  }
};

}  // namespace
}  // namespace rt

struct rt_pipeline {
  rt_pipeline_opts o{};
  std::mutex mu;  // one call per pipeline at a time
  // what the flags mean for the buffer plan
  bool emit = false;      // the sets hold emission and coverage (a non-plain mode, or the split filter)
  bool light = false;     // mode == RT_REPROJECT_LIGHT
  bool filtered = false;  // filter != RT_PIPE_FILTER_NONE
  bool split = false;     // the filter's _emit entry
  // the buffers: all of one size on one device, dropped together when either changes
  int32_t w = 0, h = 0, device = -1;
  rt::HistSet set[2];
  rt::CurSet cur;
  rt::GuideSet guide;
  rt::Stream own_stream;  // rt_pipeline_image's and rt_pipeline_ppm's
  uint64_t allocations = 0;
  // rt_pipeline_push_shares: the shares' blocks on the lead device and their staging on their own,
  // kept while the size, the share count and the shares' devices stay the same
  rt::DeviceBuffer gather;
  std::vector<std::unique_ptr<rt::ShareStage>> stage;
  uint64_t share_stride = 0;  // floats of a share's block
  // the history: which set holds it and the camera that saw it
  int prev = -1;  // -1: none
  rt_camera cam_prev{};
  int last = -1;  // the set of the last successful push (rt_pipeline_image, _ppm, _planes_device)
  int32_t frames = 0, had_history = 0;
  int64_t ppm_len = -1;  // the length of the text in guide.ppm when it is `last`'s, else -1
};

namespace rt {
namespace {

size_t npix(const rt_pipeline* p) { return (size_t)p->w * (size_t)p->h; }

size_t carve(const rt_pipeline* p, HistSet* s, char* base) {
  const size_t n = npix(p);
  Carver c{base};
  s->rgb = c.take(3 * n), s->var = c.take(n), s->count = c.take(n), s->normal = c.take(3 * n), s->depth = c.take(n);
  s->emission = p->emit ? c.take(3 * n) : nullptr;
  s->coverage = p->emit ? c.take(n) : nullptr;
  s->lum2 = p->o.moments ? c.take(n) : nullptr;
  s->bounces = p->o.specular ? c.take(n) : nullptr;
  s->image = p->filtered ? c.take(3 * n) : s->rgb;
  return c.off;
}
size_t carve(const rt_pipeline* p, CurSet* s, char* base) {
  const size_t n = npix(p);
  Carver c{base};
  s->rgb = c.take(3 * n), s->var = c.take(n);
  s->emission = p->light ? c.take(3 * n) : nullptr;
  s->coverage = p->light ? c.take(n) : nullptr;
  return c.off;
}
// rt_format_ppm_device's text is at most the header and "255 255 255\n" per pixel
int64_t ppm_bound(const rt_pipeline* p) { return 64 + 12 * (int64_t)npix(p); }
size_t carve(const rt_pipeline* p, GuideSet* s, char* base) {
  const size_t n = npix(p);
  Carver c{base};
  s->albedo = p->filtered ? c.take(3 * n) : nullptr;
  s->surface_albedo = p->split ? c.take(3 * n) : nullptr;
  s->normal = p->filtered && p->o.specular ? c.take(3 * n) : nullptr;
  s->depth = p->filtered && p->o.specular ? c.take(n) : nullptr;
  s->ppm_cap = ppm_bound(p);
  s->ppm = c.take_bytes((size_t)s->ppm_cap);
  return c.off;
}

// the group's allocation for the current size, made once (the pipeline's device is current)
template <class Set>
int ensure(rt_pipeline* p, Set* s) {
  if (s->buf.p) return RT_OK;
  const int rc = s->buf.grow(carve(p, s, nullptr), "rt_pipeline_push");
  if (rc) return rc;
  ++p->allocations;
  carve(p, s, (char*)s->buf.p);
  return RT_OK;
}

// the gather buffer and the shares' staging, each freed with its device current
void drop_shares(rt_pipeline* p) {
  if (p->gather.p || !p->stage.empty()) {
    DeviceGuard dg;
    for (auto& st : p->stage) {
      (void)hipSetDevice(st->device);
      st.reset();
    }
    p->stage.clear();
    (void)hipSetDevice(p->device);
    p->gather.reset();
  }
  p->share_stride = 0;
}

// frees everything with the owners' device current; the history goes with the buffers
void drop_buffers(rt_pipeline* p) {
  drop_shares(p);
  const bool any = p->set[0].buf.p || p->set[1].buf.p || p->cur.buf.p || p->guide.buf.p || p->own_stream.s;
  if (any) {  // a pipeline that never pushed touches no device here either
    DeviceGuard dg;
    (void)hipSetDevice(p->device);
    for (HistSet& s : p->set) s.buf.reset();
    p->cur.buf.reset();
    p->guide.buf.reset();
    p->own_stream.reset();
  }
  p->prev = p->last = -1;
  p->frames = p->had_history = 0;
  p->ppm_len = -1;
}

bool bad(float f) { return !(f >= 0.0f) || !std::isfinite(f); }

int check_opts(const rt_pipeline_opts& o) {
  const char* who = "rt_pipeline_create";
  if (o.mode < RT_REPROJECT_PLAIN || o.mode > RT_REPROJECT_LIGHT)
    return set_error(RT_ERR_INVALID, "%s: mode %d (RT_REPROJECT_PLAIN, _EMIT or _LIGHT)", who, o.mode);
  if (o.filter < RT_PIPE_FILTER_NONE || o.filter > RT_PIPE_FILTER_VAR)
    return set_error(RT_ERR_INVALID, "%s: filter %d (RT_PIPE_FILTER_NONE, _PLAIN or _VAR)", who, o.filter);
  if (o.clip && !o.moments)
    return set_error(RT_ERR_INVALID, "%s: clip needs moments = 1 (the clamp is a step of rt_reproject_moments)", who);
  if (o.specular && !o.moments)
    return set_error(RT_ERR_INVALID, "%s: specular needs moments = 1 (the chain gate is a step of rt_reproject_moments)", who);
  if (!o.temporal && (o.moments || o.clip || o.specular || o.mode != RT_REPROJECT_PLAIN))
    return set_error(RT_ERR_INVALID,
                     "%s: moments, clip, specular and a non-plain mode are the temporal stage's: set temporal = 1", who);
  const rt_reproject_opts& r = o.reproject;
  if (bad(r.max_history) || bad(r.depth_tol) || bad(r.normal_tol) || bad(r.min_weight))
    return set_error(RT_ERR_INVALID, "%s: negative or non-finite reproject option (0 selects the default)", who);
  if (o.mopts.radius < -1 || o.mopts.radius > 8)
    return set_error(RT_ERR_INVALID, "%s: mopts.radius %d (-1: no spatial estimate; at most 8)", who, o.mopts.radius);
  if (bad(o.mopts.min_frames) || (o.mopts.min_frames > 0.0f && o.mopts.min_frames < 2.0f))
    return set_error(RT_ERR_INVALID, "%s: mopts.min_frames must be 0 (the default) or a finite number >= 2", who);
  if (o.clip && o.mopts.radius == -1)
    return set_error(RT_ERR_INVALID, "%s: clip needs the window: mopts.radius >= 0, not -1", who);
  if (bad(o.copts.gamma))
    return set_error(RT_ERR_INVALID, "%s: copts.gamma must be 0 (the default) or a finite positive number", who);
  if (o.dopts.iterations < 0 || o.dopts.iterations > 8 || o.vopts.iterations < 0 || o.vopts.iterations > 8)
    return set_error(RT_ERR_INVALID, "%s: filter iterations must be 0 (the default) or 1..8", who);
  // the filters refuse a negative or NaN sigma (+Inf is theirs to take); so does the object
  for (float f : {o.dopts.sigma_color, o.dopts.sigma_normal, o.dopts.sigma_depth, o.vopts.sigma_lum,
                  o.vopts.sigma_normal, o.vopts.sigma_depth})
    if (!(f >= 0.0f)) return set_error(RT_ERR_INVALID, "%s: negative or NaN filter sigma (0 selects the default)", who);
  return RT_OK;
}

// set k as an rt_frame; count: the plane, or null with `scalar` for every pixel
rt_frame frame_of(const float* rgb, const float* var, const float* count, const HistSet& nd, float scalar) {
  return {(float*)rgb, (float*)var, (float*)count, nd.normal, nd.depth, scalar, 0};
}

// a frame without history: set k's count filled with the accumulator's pass count
int fill_count(rt_pipeline* p, const AccumView& v, int k) {
  const float passes = (float)v.passes;
  uint32_t bits;
  memcpy(&bits, &passes, sizeof bits);
  HIP_OK(hipMemsetD32Async((hipDeviceptr_t)p->set[k].count, (int)bits, npix(p), (hipStream_t)v.stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)v.stream));
  return RT_OK;
}

// Where a push's frame comes from: one whole accumulator, whose _device resolves write the
// pipeline's planes directly, or n row shares (accs[i] rank i of n, views their AccumViews), whose
// same resolves write the share's staging block; gather() then brings the planes to where the
// whole accumulator's would be.  The stages below ask a source and never an accumulator.
struct FrameSource {
  rt_pipeline* p;
  rt_accum* acc;           // the whole accumulator, or null: shares
  rt_accum* const* accs;
  const AccumView* views;
  int n;
  GatherTable t;

  // the plane's address in share i's staging block (null stays null: no plane of the configuration)
  float* staged(int i, float* dst, uint64_t off) const { return dst ? (float*)p->stage[i]->buf.p + off : nullptr; }
  int full() const {
    return set_error(RT_ERR_INVALID, "rt_pipeline_push_shares: the configuration's planes do not fit the share block");
  }
  int resolve(float* rgb, float* var) {
    if (acc) return rt_accum_resolve_device(acc, rgb, var);
    uint64_t o[2] = {0, 0};
    if (!gather_add(&t, 3, rgb, &o[0]) || !gather_add(&t, 1, var, &o[1])) return full();
    int rc;
    for (int i = 0; i < n; ++i)
      if ((rc = rt_accum_resolve_device(accs[i], staged(i, rgb, o[0]), staged(i, var, o[1])))) return rc;
    return RT_OK;
  }
  int resolve_aov(const rt_aov* out, const rt_aov_emit* emit) {
    if (acc) return rt_accum_resolve_aov_device(acc, out, emit);
    uint64_t o[6] = {0, 0, 0, 0, 0, 0};
    if (out && (!gather_add(&t, 3, out->albedo, &o[0]) || !gather_add(&t, 3, out->normal, &o[1]) ||
                !gather_add(&t, 1, out->depth, &o[2])))
      return full();
    if (emit && (!gather_add(&t, 3, emit->emission, &o[3]) || !gather_add(&t, 3, emit->surface_albedo, &o[4]) ||
                 !gather_add(&t, 1, emit->coverage, &o[5])))
      return full();
    int rc;
    for (int i = 0; i < n; ++i) {
      rt_aov so{};
      rt_aov_emit se{};
      if (out) so = {staged(i, out->albedo, o[0]), staged(i, out->normal, o[1]), staged(i, out->depth, o[2]), nullptr};
      if (emit)
        se = {staged(i, emit->emission, o[3]), staged(i, emit->surface_albedo, o[4]), staged(i, emit->coverage, o[5])};
      if ((rc = rt_accum_resolve_aov_device(accs[i], out ? &so : nullptr, emit ? &se : nullptr))) return rc;
    }
    return RT_OK;
  }
  int resolve_aov_spec(const rt_aov* out, const rt_aov_spec* spec) {
    if (acc) return rt_accum_resolve_aov_spec_device(acc, out, spec);
    uint64_t o[3] = {0, 0, 0};
    if (!gather_add(&t, 3, out->normal, &o[0]) || !gather_add(&t, 1, out->depth, &o[1]) ||
        !gather_add(&t, 1, spec->bounces, &o[2]))
      return full();
    int rc;
    for (int i = 0; i < n; ++i) {
      const rt_aov so = {nullptr, staged(i, out->normal, o[0]), staged(i, out->depth, o[1]), nullptr};
      const rt_aov_spec ss = {staged(i, spec->bounces, o[2])};
      if ((rc = rt_accum_resolve_aov_spec_device(accs[i], &so, &ss))) return rc;
    }
    return RT_OK;
  }

  // After the last resolve (each blocks: the staging blocks are complete).  Every share's block is
  // copied to the lead device on the share's own stream and followed by the share's event; the
  // lead stream waits for the events, runs k_gather_planes and is synchronised.  `issued` shares
  // have work in flight: whatever fails, their streams are drained before the call returns.
  int gather() {
    if (acc) return RT_OK;
    int issued = 0;
    const int rc = gather_enqueue(&issued);
    if (rc) {
      for (int i = 0; i < issued; ++i)
        if (hipSetDevice(views[i].device) == hipSuccess) (void)hipStreamSynchronize((hipStream_t)views[i].stream);
      (void)hipSetDevice(p->device);
      (void)hipStreamSynchronize((hipStream_t)views[0].stream);
    }
    return rc;
  }
  int gather_enqueue(int* issued) {
    const char* who = "rt_pipeline_push_shares";
    const size_t bytes = (size_t)t.used * sizeof(float);
    float* const gbuf = (float*)p->gather.p;
    for (int i = 0; i < n; ++i) {
      const int d = views[i].device;
      const hipStream_t s = (hipStream_t)views[i].stream;
      float* const dst = gbuf + (size_t)i * t.stride;
      HIP_OK(hipSetDevice(d));
      *issued = i + 1;
      if (d == p->device)
        HIP_OK(hipMemcpyAsync(dst, p->stage[i]->buf.p, bytes, hipMemcpyDeviceToDevice, s));
      else
        HIP_OK(hipMemcpyPeerAsync(dst, p->device, p->stage[i]->buf.p, d, bytes, s));
      HIP_OK(hipEventRecord(p->stage[i]->ev.ev[0], s));
    }
    HIP_OK(hipSetDevice(p->device));
    const hipStream_t lead = (hipStream_t)views[0].stream;
    for (int i = 0; i < n; ++i) HIP_OK(hipStreamWaitEvent(lead, p->stage[i]->ev.ev[0], 0));
    const int rc = gather_planes_launch(who, gbuf, t, lead);
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(lead));
    return RT_OK;
  }
};

// the floats of a share's block: the planes the configuration's resolves write (push_temporal and
// push_frame below), each padded as rt_gather_map.h pads it
uint64_t share_block_floats(const rt_pipeline* p, uint32_t W, uint32_t rows_per) {
  const rt_pipeline_opts& o = p->o;
  int threes = 1, ones = 1;                                   // rgb, var
  if (p->emit) threes += 1 + (p->split ? 1 : 0), ones += 1;   // emission, surface_albedo, coverage
  threes += 1, ones += 1;                                     // the history's normal and depth
  if (o.temporal && o.specular) ones += 1;                    // bounces
  if (p->filtered) threes += 1;                               // albedo
  if (o.temporal && o.specular && p->filtered) threes += 1, ones += 1;  // the first hit's normal and depth
  return threes * gather_plane_floats(3, W, rows_per) + ones * gather_plane_floats(1, W, rows_per);
}

// the gather buffer and the staging for these shares, made once per size, share count and devices
int ensure_shares(rt_pipeline* p, const AccumView* views, int n) {
  const char* who = "rt_pipeline_push_shares";
  const uint32_t rows_per = gather_rows_per((uint32_t)p->h, (uint32_t)n);
  const uint64_t stride = share_block_floats(p, (uint32_t)p->w, rows_per);
  bool same = p->gather.p && (int)p->stage.size() == n && p->share_stride == stride;
  for (int i = 0; same && i < n; ++i) same = p->stage[i]->device == views[i].device;
  if (same) return RT_OK;
  drop_shares(p);
  std::vector<int32_t> devs(n);
  for (int i = 0; i < n; ++i) devs[i] = views[i].device;
  int rc = enable_peers(who, devs.data(), n);  // leaves the lead device current
  if (rc == RT_OK && (rc = p->gather.grow((size_t)n * stride * sizeof(float), who)) == RT_OK) ++p->allocations;
  for (int i = 0; rc == RT_OK && i < n; ++i) {
    if (hipSetDevice(devs[i]) != hipSuccess) {
      rc = set_error(RT_ERR_DEVICE, "%s: device %d", who, devs[i]);
      break;
    }
    p->stage.emplace_back(new ShareStage());
    p->stage[i]->device = devs[i];
    if ((rc = p->stage[i]->buf.grow((size_t)stride * sizeof(float), who))) break;
    rc = p->stage[i]->ev.ensure(1, hipEventDisableTiming);
  }
  if (rc) {
    drop_shares(p);
    return rc;
  }
  p->share_stride = stride;
  HIP_OK(hipSetDevice(p->device));
  return RT_OK;
}

// the temporal half: Temporal.push / Temporal._push_moments.  k: the set the history is not in
int push_temporal(rt_pipeline* p, FrameSource& src, const AccumView& v, int k, bool has_prev) {
  const rt_pipeline_opts& o = p->o;
  HistSet& s = p->set[k];
  GuideSet& g = p->guide;
  const bool mom = o.moments != 0;
  int rc;
  // the frame: without moments straight into the new history's set (out aliases cur); with them
  // into the third set, since no out buffer of the moments entries may be one of cur's
  float* frgb = mom ? p->cur.rgb : s.rgb;
  float* fvar = mom ? p->cur.var : s.var;
  if ((rc = src.resolve(frgb, fvar))) return rc;
  // the frame's emission and coverage: the kernel writes them only with the light history
  float* femi = !p->emit ? nullptr : (mom && p->light) ? p->cur.emission : s.emission;
  float* fcov = !p->emit ? nullptr : (mom && p->light) ? p->cur.coverage : s.coverage;
  const rt_aov_emit emit_out = {femi, g.surface_albedo, fcov};
  const rt_aov_emit* ep = p->emit ? &emit_out : nullptr;
  if (o.specular) {  // the chain's normal, depth and bounces in the first hit's place
    const rt_aov chain = {nullptr, s.normal, s.depth, nullptr};
    const rt_aov_spec sp = {s.bounces};
    if ((rc = src.resolve_aov_spec(&chain, &sp))) return rc;
    const rt_aov first = {g.albedo, g.normal, g.depth, nullptr};  // the filter's guides stay the first hit's
    if (p->filtered || ep)
      if ((rc = src.resolve_aov(p->filtered ? &first : nullptr, ep))) return rc;
  } else {
    const rt_aov first = {g.albedo, s.normal, s.depth, nullptr};
    if ((rc = src.resolve_aov(&first, ep))) return rc;
  }
  if ((rc = src.gather())) return rc;  // shares: the planes are where the lines above name them
  if (!mom && !has_prev) return fill_count(p, v, k);  // the frame itself
  // the entry the configuration stands for: its name is in every message the call can raise
  const char* name = o.specular ? "rt_reproject_spec_device"
                     : o.clip   ? "rt_reproject_clip_device"
                     : mom      ? "rt_reproject_moments_device"
                     : o.mode == RT_REPROJECT_LIGHT ? "rt_reproject_light_device"
                     : o.mode == RT_REPROJECT_EMIT  ? "rt_reproject_emit_device"
                                                    : "rt_reproject_device";
  const HistSet& q = p->set[has_prev ? p->prev : k];
  const rt_frame prev = frame_of(q.rgb, q.var, q.count, q, 0.0f);
  const rt_aov_emit prev_emit = {q.emission, nullptr, q.coverage};
  const rt_frame cur = frame_of(frgb, fvar, nullptr, s, (float)v.passes);
  const rt_aov_emit cur_emit = {femi, nullptr, fcov};
  const rt_frame out = {s.rgb, s.var, s.count, nullptr, nullptr, 0.0f, 0};
  const rt_aov_emit out_emit = {s.emission, nullptr, s.coverage};
  const rt_spec_planes sp = {has_prev ? q.bounces : nullptr, s.bounces};
  // moments: a first frame goes through the entry too, with prev = NULL.  reproject_impl drops the
  // emit structs the mode does not take
  ReprojectRequest rq = {name, /*host=*/false, mom, o.mode};
  if (has_prev) rq.cam_prev = &p->cam_prev, rq.prev = &prev, rq.prev_emit = &prev_emit, rq.prev_lum2 = q.lum2;
  rq.cam_cur = &v.cam, rq.cur = &cur, rq.cur_emit = &cur_emit;
  rq.w = p->w, rq.h = p->h;
  rq.opts = &o.reproject;
  rq.mopts = &o.mopts, rq.copts = o.clip ? &o.copts : nullptr, rq.spec = o.specular ? &sp : nullptr;
  rq.out = &out, rq.out_emit = &out_emit, rq.out_lum2 = s.lum2;
  rq.device = p->device, rq.stream = v.stream;
  return reproject_impl(rq);
}

// temporal = 0: the frame is the accumulator's resolve and count the pass count
int push_frame(rt_pipeline* p, FrameSource& src, const AccumView& v, int k) {
  HistSet& s = p->set[k];
  GuideSet& g = p->guide;
  int rc;
  if ((rc = src.resolve(s.rgb, s.var))) return rc;
  const rt_aov first = {g.albedo, s.normal, s.depth, nullptr};
  const rt_aov_emit emit_out = {s.emission, g.surface_albedo, s.coverage};
  if ((rc = src.resolve_aov(&first, p->emit ? &emit_out : nullptr))) return rc;
  if ((rc = src.gather())) return rc;
  return fill_count(p, v, k);
}

// the filter half: set k's blend into set k's image.  In the light mode the set's emission and
// coverage are the blended ones; in every other they are the frame's own
int push_filter(rt_pipeline* p, const AccumView& v, int k) {
  const rt_pipeline_opts& o = p->o;
  HistSet& s = p->set[k];
  GuideSet& g = p->guide;
  const bool own_guides = o.specular != 0;  // the set's normal and depth are the chain's then
  const rt_aov feat = {g.albedo, own_guides ? g.normal : s.normal, own_guides ? g.depth : s.depth, nullptr};
  const rt_aov_emit emit = {s.emission, g.surface_albedo, s.coverage};
  if (o.filter == RT_PIPE_FILTER_VAR)
    return p->split ? rt_denoise_var_emit_device(s.rgb, s.var, &feat, &emit, p->w, p->h, &o.vopts, s.image, nullptr,
                                                 p->device, v.stream)
                    : rt_denoise_var_device(s.rgb, s.var, &feat, p->w, p->h, &o.vopts, s.image, nullptr, p->device,
                                            v.stream);
  return p->split
             ? rt_denoise_emit_device(s.rgb, &feat, &emit, p->w, p->h, &o.dopts, s.image, p->device, v.stream)
             : rt_denoise_device(s.rgb, &feat, p->w, p->h, &o.dopts, s.image, p->device, v.stream);
}

// what both push entries ask of an accumulator (a share's or the whole image's), in this order
int check_accum(const char* who, const rt_pipeline* p, const AccumView& v) {
  if (v.passes < 1) return set_error(RT_ERR_INVALID, "%s: the accumulator holds no pass (rt_accum_add first)", who);
  if (!v.features)
    return set_error(RT_ERR_INVALID, "%s: needs an accumulator with features (rt_accum_set_features: the normal and "
                     "depth guides)", who);
  if (!(v.features & RT_ACCUM_FEAT_GUIDES))
    return set_error(RT_ERR_INVALID, "%s: needs RT_ACCUM_FEAT_GUIDES (the normal and depth guides), the accumulator "
                     "has planes 0x%x", who, v.features);
  if (p->emit && !(v.features & RT_ACCUM_FEAT_EMIT))
    return set_error(RT_ERR_INVALID, "%s: a non-plain mode and split_emitters need an accumulator with "
                     "RT_ACCUM_FEAT_EMIT (rt_accum_set_features), this one has planes 0x%x", who, v.features);
  if (p->o.specular && !(v.features & RT_ACCUM_FEAT_SPEC))
    return set_error(RT_ERR_INVALID, "%s: specular needs an accumulator with RT_ACCUM_FEAT_SPEC "
                     "(rt_accum_set_features_spec), this one has planes 0x%x", who, v.features);
  return RT_OK;
}
int check_image(const char* who, int32_t w, int32_t h) {
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31) / 3)
    return set_error(RT_ERR_INVALID, "%s: %d x %d image", who, w, h);
  return RT_OK;
}

// A checked push (p->mu held): v is the frame as the stages see it, the whole image on the lead
// device and stream, whichever source it comes from
int push_source(rt_pipeline* p, FrameSource& src, const AccumView& v) {
  const rt_pipeline_opts& o = p->o;
  int rc;
  DeviceGuard dg;
  if (v.width != p->w || v.rows != p->h || v.device != p->device) {  // another size or device: no history
    drop_buffers(p);
    p->w = v.width, p->h = v.rows, p->device = v.device;
  }
  HIP_OK(hipSetDevice(p->device));
  const int k = p->last == 0 ? 1 : 0;  // never the set of the last frame: its planes stay valid for one more push
  const bool has_prev = o.temporal && p->prev >= 0;
  if ((rc = ensure(p, &p->set[k]))) return rc;
  if (o.moments && (rc = ensure(p, &p->cur))) return rc;
  if ((rc = ensure(p, &p->guide))) return rc;
  if (!src.acc) {
    if ((rc = ensure_shares(p, src.views, src.n))) return rc;
    gather_begin(&src.t, (uint32_t)p->w, (uint32_t)p->h, (uint32_t)src.n, p->share_stride);
  }
  rc = o.temporal ? push_temporal(p, src, v, k, has_prev) : push_frame(p, src, v, k);
  if (rc) return rc;
  if (p->filtered && (rc = push_filter(p, v, k))) return rc;
  // the frame is complete: it becomes the history and the last frame
  p->prev = o.temporal ? k : -1;
  p->cam_prev = v.cam;
  p->last = k;
  p->ppm_len = -1;
  p->had_history = has_prev;
  ++p->frames;
  return RT_OK;
}

// rt_pipeline_image's and rt_pipeline_ppm's prologue (p->mu held, DeviceGuard in the caller)
int last_frame(rt_pipeline* p, const char* who, hipStream_t* stream) {
  if (p->last < 0)
    return set_error(RT_ERR_INVALID, "%s: no frame yet: call rt_pipeline_push first", who);
  HIP_OK(hipSetDevice(p->device));
  return p->own_stream.pick(nullptr, stream);
}

}  // namespace
}  // namespace rt

using namespace rt;

extern "C" {

int rt_pipeline_create(const rt_pipeline_opts* opts, rt_pipeline** out) {
  if (!opts || !out) return set_error(RT_ERR_INVALID, "rt_pipeline_create: null opts/out");
  *out = nullptr;
  const int rc = check_opts(*opts);
  if (rc) return rc;
  rt_pipeline* p = new rt_pipeline();
  p->o = *opts;
  p->filtered = opts->filter != RT_PIPE_FILTER_NONE;
  p->split = p->filtered && opts->split_emitters;
  p->light = opts->mode == RT_REPROJECT_LIGHT;
  p->emit = opts->mode != RT_REPROJECT_PLAIN || p->split;
  *out = p;
  return RT_OK;
}

int rt_pipeline_destroy(rt_pipeline* p) {
  if (!p) return RT_OK;
  {
    std::lock_guard<std::mutex> lk(p->mu);  // a call in flight on another thread ends first
    drop_buffers(p);
  }
  delete p;
  return RT_OK;
}

int rt_pipeline_reset(rt_pipeline* p) {
  if (!p) return set_error(RT_ERR_INVALID, "rt_pipeline_reset: null pipeline");
  std::lock_guard<std::mutex> lk(p->mu);
  p->prev = -1;
  p->frames = 0;
  return RT_OK;
}

int rt_pipeline_push(rt_pipeline* p, rt_accum* acc) {
  const char* who = "rt_pipeline_push";
  if (!p || !acc) return set_error(RT_ERR_INVALID, "%s: null pipeline/accumulator", who);
  std::lock_guard<std::mutex> lk(p->mu);
  AccumView v;
  int rc = accum_view(acc, &v);
  if (rc) return rc;
  if ((rc = check_accum(who, p, v))) return rc;
  if (v.nranks != 1)
    return set_error(RT_ERR_INVALID, "%s: needs the whole image (an accumulator with nranks == 1, not %d)", who,
                     v.nranks);
  if ((rc = check_image(who, v.width, v.rows)) || (rc = device_ok(who, v.device))) return rc;
  FrameSource src{p, acc, nullptr, nullptr, 0, {}};
  return push_source(p, src, v);
}

int rt_pipeline_push_shares(rt_pipeline* p, rt_accum* const* accs, int32_t n) {
  const char* who = "rt_pipeline_push_shares";
  if (!p || !accs) return set_error(RT_ERR_INVALID, "%s: null pipeline/accumulator array", who);
  if (n < 1) return set_error(RT_ERR_INVALID, "%s: n = %d shares (at least 1)", who, n);
  for (int i = 0; i < n; ++i) {
    if (!accs[i]) return set_error(RT_ERR_INVALID, "%s: accs[%d] is null", who, i);
    for (int j = 0; j < i; ++j)
      if (accs[j] == accs[i]) return set_error(RT_ERR_INVALID, "%s: accs[%d] and accs[%d] are the same accumulator", who, j, i);
  }
  std::lock_guard<std::mutex> lk(p->mu);
  std::vector<AccumView> views(n);
  int rc;
  for (int i = 0; i < n; ++i)
    if ((rc = accum_view(accs[i], &views[i]))) return rc;
  const AccumView& v0 = views[0];
  if (n > v0.height)
    return set_error(RT_ERR_INVALID, "%s: %d shares of an image of %d rows (an empty share is not supported)", who, n,
                     v0.height);
  for (int i = 0; i < n; ++i) {
    const AccumView& v = views[i];
    if (v.rank != i || v.nranks != n)
      return set_error(RT_ERR_INVALID, "%s: accs[%d] is rank %d of %d, not rank %d of %d", who, i, v.rank, v.nranks, i, n);
    if ((rc = check_accum(who, p, v))) return rc;
    const char* what = v.scene != v0.scene                             ? "scene"
                       : memcmp(&v.cam, &v0.cam, sizeof(rt_camera))    ? "camera"
                       : v.width != v0.width || v.height != v0.height  ? "image size"
                       : v.features != v0.features                     ? "feature planes"
                       : v.spec_bounces != v0.spec_bounces || memcmp(&v.spec_fuzz, &v0.spec_fuzz, sizeof(float))
                           ? "chain limits (rt_accum_set_features_spec)"
                       : v.passes != v0.passes                         ? "pass count"
                                                                       : nullptr;
    if (what) return set_error(RT_ERR_INVALID, "%s: accs[%d] differs from accs[0] in its %s", who, i, what);
  }
  if ((rc = check_image(who, v0.width, v0.height))) return rc;
  for (int i = 0; i < n; ++i)
    if ((rc = device_ok(who, views[i].device))) return rc;
  // the frame as the stages see it: the whole image on the lead share's device and stream
  AccumView v = v0;
  v.rows = v0.height, v.rank = 0, v.nranks = 1;
  FrameSource src{p, nullptr, accs, views.data(), n, {}};
  return push_source(p, src, v);
}

int rt_pipeline_image(rt_pipeline* p, float* rgb_host) {
  const char* who = "rt_pipeline_image";
  if (!p || !rgb_host) return set_error(RT_ERR_INVALID, "%s: null pipeline/image", who);
  std::lock_guard<std::mutex> lk(p->mu);
  DeviceGuard dg;
  hipStream_t s;
  const int rc = last_frame(p, who, &s);
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(rgb_host, p->set[p->last].image, 3 * npix(p) * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return RT_OK;
}

int64_t rt_pipeline_ppm(rt_pipeline* p, char* out_host, int64_t cap) {
  const char* who = "rt_pipeline_ppm";
  if (!p) return set_error(RT_ERR_INVALID, "%s: null pipeline", who);
  if (cap < 0) return set_error(RT_ERR_INVALID, "%s: negative cap", who);
  std::lock_guard<std::mutex> lk(p->mu);
  DeviceGuard dg;
  hipStream_t s;
  const int rc = last_frame(p, who, &s);
  if (rc) return rc;
  if (p->ppm_len < 0) {  // the text is formatted once per frame, whoever asks first
    const int64_t n =
        rt_format_ppm_device(p->set[p->last].image, p->w, p->h, p->guide.ppm, p->guide.ppm_cap, p->device, s);
    if (n < 0) return n;
    p->ppm_len = n;
  }
  if (!out_host || cap == 0) return p->ppm_len;
  if (p->ppm_len > cap) return set_error(RT_ERR_INVALID, "%s: buffer too small (%lld bytes, the text has %lld)", who,
                                         (long long)cap, (long long)p->ppm_len);
  HIP_OK(hipMemcpyAsync(out_host, p->guide.ppm, (size_t)p->ppm_len, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return p->ppm_len;
}

int rt_pipeline_planes_device(rt_pipeline* p, rt_frame* blended, rt_aov_emit* light, float** lum2, float** image) {
  const char* who = "rt_pipeline_planes_device";
  if (!p) return set_error(RT_ERR_INVALID, "%s: null pipeline", who);
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->last < 0) return set_error(RT_ERR_INVALID, "%s: no frame yet: call rt_pipeline_push first", who);
  const HistSet& s = p->set[p->last];
  if (blended) *blended = {s.rgb, s.var, s.count, s.normal, s.depth, 0.0f, 0};
  if (light) *light = {s.emission, nullptr, s.coverage};
  if (lum2) *lum2 = s.lum2;
  if (image) *image = s.image;
  return RT_OK;
}

int rt_pipeline_info_get(rt_pipeline* p, rt_pipeline_info* out) {
  if (!p || !out) return set_error(RT_ERR_INVALID, "rt_pipeline_info_get: null");
  std::lock_guard<std::mutex> lk(p->mu);
  *out = rt_pipeline_info{};
  out->width = p->w, out->height = p->h, out->device = p->device;
  out->frames = p->frames, out->had_history = p->had_history;
  out->device_bytes =
      p->set[0].buf.bytes + p->set[1].buf.bytes + p->cur.buf.bytes + p->guide.buf.bytes + p->gather.bytes;
  out->allocations = p->allocations;
  return RT_OK;
}

}  // extern "C"
