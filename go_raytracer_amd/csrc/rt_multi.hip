// rt_multi.hip — rt_render_multi: one image over several devices.  Share i (rows r % n == i,
// camera.go:119-122) renders on devices[i] through rt_render.hip's render_share, one host
// thread and stream per share, each with its own render slot; the shares are peer-copied (or
// gathered by RCCL, RT_FLAG_GATHER_RCCL) to devices[0] and de-interleaved there.
// rt_accum_add_shares: one accumulator pass per share on the same kind of host threads.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "rt_hip_util.h"
#include "rt_host_units.h"

namespace rt {

// The RCCL gather: one communicator per device of the list (ncclCommInitAll), a stream and a
// padded send buffer per share, kept while the device list and the share size stay the same
struct RcclGather {
  std::vector<int> devs;
  std::vector<ncclComm_t> comms;
  std::vector<Stream> streams;
  std::vector<DeviceBuffer> send;
  size_t send_floats = 0;  // what every send buffer holds (0: grow them first)
  void release() {
    for (size_t i = 0; i < comms.size(); ++i) {
      (void)hipSetDevice(devs[i]);
      if (send.size() > i) send[i].reset();
      if (streams.size() > i) streams[i].reset();
      (void)ncclCommDestroy(comms[i]);
    }
    devs.clear();
    comms.clear();
    streams.clear();
    send.clear();
    send_floats = 0;
  }
};

// rt_render_multi's device state (Scene::multi, created by the first call, under multi_mu)
struct MultiState {
  DeviceBuffer gather;  // gather + image buffer on gather_dev, the device list's first
  int gather_dev = -1;
  RcclGather rccl;      // empty until a call asks for RT_FLAG_GATHER_RCCL
};

void release_multi(Scene* s) {
  if (!s->multi) return;
  s->multi->rccl.release();
  if (s->multi->gather.p) (void)hipSetDevice(s->multi->gather_dev);
  delete s->multi;
  s->multi = nullptr;
}

// rows of share i ([rows_per][W][3] at gather + i*rows_per*W*3) -> image rows r = i + n*k
__global__ __launch_bounds__(256) void k_deinterleave(const float* gather, float* out, uint32_t H,
                                                      uint32_t W, uint32_t n, uint32_t rows_per) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t row_floats = 3ull * W;
  if (i >= (uint64_t)H * row_floats) return;
  const uint32_t r = (uint32_t)(i / row_floats);
  const uint64_t x = i - (uint64_t)r * row_floats;
  out[i] = gather[((uint64_t)(r % n) * rows_per + r / n) * row_floats + x];
}

// the scene's gather + image buffer on device d0 (current), at least `need` bytes
static int ensure_gather_buffer(MultiState* ms, int d0, size_t need) {
  if (ms->gather.p && ms->gather_dev != d0) {  // another list's first device: freed there
    (void)hipSetDevice(ms->gather_dev);
    ms->gather.reset();
    HIP_OK(hipSetDevice(d0));
  }
  ms->gather_dev = d0;
  return ms->gather.grow(need, "rt_render_multi");
}

// xGMI peer access both ways.  "Already enabled" is success; any other failure is
// an error (the copies would silently fall back to staging through host memory).
// Devices that report no peer path copy through the runtime's staged path.
int enable_peer(const char* who, int from, int to) {
  HIP_OK(hipSetDevice(from));
  const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
  if (e == hipErrorPeerAccessAlreadyEnabled) {
    (void)hipGetLastError();  // clear the sticky "already enabled" status
    return RT_OK;
  }
  if (e != hipSuccess)
    return set_error(RT_ERR_DEVICE, "%s: peer access %d -> %d: %s", who, from, to, hipGetErrorString(e));
  return RT_OK;
}
// ... between devices[0] and every other device of the list; leaves devices[0] current
int enable_peers(const char* who, const int32_t* devices, int n) {
  const int d0 = devices[0];
  int rc;
  for (int i = 1; i < n; ++i)
    if (devices[i] != d0) {
      int can_a = 0, can_b = 0;
      HIP_OK(hipDeviceCanAccessPeer(&can_a, devices[i], d0));
      HIP_OK(hipDeviceCanAccessPeer(&can_b, d0, devices[i]));
      if (can_a && (rc = enable_peer(who, devices[i], d0))) return rc;
      if (can_b && (rc = enable_peer(who, d0, devices[i]))) return rc;
    }
  HIP_OK(hipSetDevice(d0));
  return RT_OK;
}

// The scene's RCCL state for this device list and share size: communicators over the list,
// cached, and a send buffer of share_floats per share.  Leaves devices[0] current.
static int setup_rccl(RcclGather* rg, const int32_t* devices, int n, size_t share_floats) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (devices[i] == devices[j])
        return set_error(RT_ERR_INVALID, "rt_render_multi: RCCL gather needs distinct devices");
  int rc;
  if (rg->devs != std::vector<int>(devices, devices + n)) {
    rg->release();
    rg->devs.assign(devices, devices + n);
    rg->comms.assign(n, nullptr);
    const ncclResult_t r = ncclCommInitAll(rg->comms.data(), n, devices);
    if (r != ncclSuccess) {
      rg->comms.clear();
      rg->devs.clear();
      return set_error(RT_ERR_DEVICE, "rt_render_multi: ncclCommInitAll: %s", ncclGetErrorString(r));
    }
    rg->streams.resize(n);
    rg->send.resize(n);
    for (int i = 0; i < n; ++i) {
      HIP_OK(hipSetDevice(devices[i]));
      if ((rc = rg->streams[i].ensure())) return rc;
    }
  }
  if (rg->send_floats < share_floats) {
    rg->send_floats = 0;  // until every buffer has grown: after a failure the next call grows again
    for (int i = 0; i < n; ++i) {
      HIP_OK(hipSetDevice(devices[i]));
      if ((rc = rg->send[i].grow(share_floats * sizeof(float), "rt_render_multi"))) return rc;
    }
    rg->send_floats = share_floats;
  }
  HIP_OK(hipSetDevice(devices[0]));
  return RT_OK;
}

// one collective: every share's [rows_per][W][3] tile to devices[0]'s gather buffer
// (rank-major, the layout k_deinterleave reads); rows past a short share are padding
static int gather_rccl(RcclGather* rg, const int32_t* devices, int n, size_t share_floats, float* gbuf) {
  ncclResult_t r = ncclGroupStart();
  for (int i = 0; r == ncclSuccess && i < n; ++i) {
    HIP_OK(hipSetDevice(devices[i]));
    r = ncclGather(rg->send[i].p, i == 0 ? (void*)gbuf : nullptr, share_floats, ncclFloat32, 0,
                   rg->comms[i], rg->streams[i].s);
  }
  const ncclResult_t r2 = ncclGroupEnd();
  if (r == ncclSuccess) r = r2;
  if (r != ncclSuccess)
    return set_error(RT_ERR_DEVICE, "rt_render_multi: ncclGather: %s", ncclGetErrorString(r));
  for (int i = 0; i < n; ++i) {
    HIP_OK(hipSetDevice(devices[i]));
    HIP_OK(hipStreamSynchronize(rg->streams[i].s));
  }
  return RT_OK;
}

// the image's rt_stats from its shares': counts summed, the slowest share's kernel times
static void sum_stats(rt_stats* stats, const std::vector<rt_stats>& st) {
  memset(stats, 0, sizeof *stats);
  *stats = st[0];
  stats->samples = stats->segments = stats->stack_pushes = stats->overflow_samples = 0;
  stats->extend_rays = stats->shade_rays = 0;
  stats->rows = 0;
  stats->ms_fused = stats->ms_extend = stats->ms_shade = 0;
  for (const rt_stats& si : st) {
    stats->samples += si.samples;
    stats->segments += si.segments;
    stats->stack_pushes += si.stack_pushes;
    stats->overflow_samples += si.overflow_samples;
    stats->extend_rays += si.extend_rays;
    stats->shade_rays += si.shade_rays;
    stats->rows += si.rows;
    // the slowest share bounds the render
    stats->ms_fused = std::max(stats->ms_fused, si.ms_fused);
    stats->ms_extend = std::max(stats->ms_extend, si.ms_extend);
    stats->ms_shade = std::max(stats->ms_shade, si.ms_shade);
  }
}

static int render_multi(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                        const int32_t* devices, int32_t n, float* out_host, float* out_dev,
                        rt_stats* stats) {
  if (!scene || !cam || !devices || n <= 0)
    return set_error(RT_ERR_INVALID, "rt_render_multi: null argument or n <= 0");
  rt_render_opts o{};
  if (opts) o = *opts;
  if (o.nranks > 1 || o.rank != 0)
    return set_error(RT_ERR_INVALID, "rt_render_multi: shards the image itself (rank/nranks)");
  if (o.stream) return set_error(RT_ERR_INVALID, "rt_render_multi: one stream per share (opts.stream)");
  int rc;
  for (int i = 0; i < n; ++i)
    if ((rc = device_ok("rt_render_multi", devices[i]))) return rc;
  rt_camera_derived cd;
  if ((rc = rt_camera_derive(cam, &cd))) return rc;
  Scene* s = &scene->s;
  std::lock_guard<std::mutex> multi(s->multi_mu);
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t H = (uint32_t)cd.height, W = (uint32_t)cd.width, N = (uint32_t)n;
  const uint32_t rows_per = (H + N - 1) / N;
  const size_t share_floats = (size_t)rows_per * W * 3;
  const size_t gather_floats = (size_t)N * share_floats, img_floats = (size_t)H * W * 3;
  const int d0 = devices[0];
  DeviceGuard dg;  // the caller's current device is restored on every return
  HIP_OK(hipSetDevice(d0));
  if (!s->multi) s->multi = new MultiState();
  if ((rc = ensure_gather_buffer(s->multi, d0, (gather_floats + img_floats) * sizeof(float)))) return rc;
  float* gbuf = (float*)s->multi->gather.p;
  float* img = out_dev ? out_dev : gbuf + gather_floats;
  if ((rc = enable_peers("rt_render_multi", devices, n))) return rc;
  // RT_FLAG_GATHER_RCCL: the shares gathered by one collective
  RcclGather* rg = (o.flags & RT_FLAG_GATHER_RCCL) ? &s->multi->rccl : nullptr;
  if (rg && (rc = setup_rccl(rg, devices, n, share_floats))) return rc;
  // rt_progress: this call's shares are the tracked render unless another holds it.
  // Claimed only after every early return of the setup above, so every return below
  // releases it.  (No slice events: the shares add their samples when done.)
  const bool track = claim_progress(s->prog, (uint64_t)H * W * cd.spp_sqrt * cd.spp_sqrt, d0);
  ProgressDone prog_done{s->prog, track};
  std::vector<rt_stats> st(n);
  std::vector<int> rcs(n, RT_OK);
  std::vector<std::string> errs(n);
  std::vector<std::thread> th;
  for (int i = 0; i < n; ++i)
    th.emplace_back([&, i] {
      rt_render_opts oi = o;
      oi.device = devices[i];
      oi.rank = i;
      oi.nranks = n;
      oi.progress_slices = 0;
      const Gather g = {gbuf + (size_t)i * share_floats, d0};
      // (RCCL: the share's rows into its padded send buffer; the gather follows)
      rcs[i] = render_share(scene, cam, &oi, &st[i], i, rg ? (float*)rg->send[i].p : nullptr, rg ? nullptr : &g);
      if (rcs[i] != RT_OK) {
        errs[i] = rt_last_error();
      } else if (track) {  // rt_progress advances share by share
        std::lock_guard<std::mutex> lk(s->prog.mu);
        s->prog.done = std::min(s->prog.total, s->prog.done + st[i].samples);
      }
    });
  for (auto& t : th) t.join();
  for (int i = 0; i < n; ++i)
    if (rcs[i] != RT_OK) return set_error(rcs[i], "rt_render_multi share %d: %s", i, errs[i].c_str());
  if (rg && share_floats > 0 && (rc = gather_rccl(rg, devices, n, share_floats, gbuf))) return rc;
  HIP_OK(hipSetDevice(d0));
  if (img_floats > 0) {
    hipLaunchKernelGGL(k_deinterleave, dim3((unsigned)((img_floats + 255) / 256)), dim3(256), 0,
                       (hipStream_t)0, gbuf, img, H, W, N, rows_per);
    HIP_OK(hipGetLastError());
    if (out_host)
      HIP_OK(hipMemcpy(out_host, img, img_floats * sizeof(float), hipMemcpyDeviceToHost));
  }
  HIP_OK(hipStreamSynchronize((hipStream_t)0));
  prog_done.ok = true;
  if (stats) {
    sum_stats(stats, st);
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return RT_OK;
}

// rt_accum_add_shares: one pass of every share, a host thread each as render_multi's shares have
static int accum_add_shares(rt_accum* const* accs, int32_t n, uint64_t seed, rt_stats* stats) {
  const char* who = "rt_accum_add_shares";
  if (!accs) return set_error(RT_ERR_INVALID, "%s: null accumulator array", who);
  if (n < 1) return set_error(RT_ERR_INVALID, "%s: n = %d shares (at least 1)", who, n);
  for (int i = 0; i < n; ++i)
    if (!accs[i]) return set_error(RT_ERR_INVALID, "%s: accs[%d] is null", who, i);
  std::vector<rt_stats> st(n);
  std::vector<int> rcs(n, RT_OK);
  std::vector<std::string> errs(n);
  std::vector<std::thread> th;
  for (int i = 0; i < n; ++i)
    th.emplace_back([&, i] {
      rcs[i] = rt_accum_add(accs[i], seed, &st[i]);
      if (rcs[i] != RT_OK) errs[i] = rt_last_error();
    });
  for (auto& t : th) t.join();
  // the lowest failing share's code and message; the others keep the pass they took
  for (int i = 0; i < n; ++i)
    if (rcs[i] != RT_OK) return set_error(rcs[i], "%s share %d: %s", who, i, errs[i].c_str());
  if (stats) sum_stats(stats, st);
  return RT_OK;
}

}  // namespace rt

extern "C" {

int rt_accum_add_shares(rt_accum* const* accs, int32_t n, uint64_t seed, rt_stats* stats) {
  return rt::accum_add_shares(accs, n, seed, stats);
}

int rt_render_multi(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                    const int32_t* devices, int32_t n, float* out_rgb, rt_stats* stats) {
  if (!out_rgb) return rt::set_error(RT_ERR_INVALID, "rt_render_multi: null output");
  return rt::render_multi(s, cam, opts, devices, n, out_rgb, nullptr, stats);
}

int rt_render_multi_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                           const int32_t* devices, int32_t n, float* out_rgb_device,
                           rt_stats* stats) {
  if (!out_rgb_device) return rt::set_error(RT_ERR_INVALID, "rt_render_multi_device: null output");
  return rt::render_multi(s, cam, opts, devices, n, nullptr, out_rgb_device, stats);
}

}  // extern "C"
