// rt_hip_util.h — the generic host-side HIP helpers of every HIP translation unit: the error
// macro, the current-device guard, with_flag, and the owners of device memory, streams and events.  No
// other unit calls hipMalloc, hipFree, hipStreamCreate*, hipStreamDestroy, hipEventCreate* or
// hipEventDestroy (DESIGN.md "Device resources"; tests/test_hip_resources.py).  What the render,
// the accumulator and the feature pass declare for one another is rt_host_units.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "rt_internal.h"

namespace rt {

#define HIP_OK(expr)                                                                    \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return set_error(RT_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e));   \
  } while (0)

// Restores the calling thread's current device on scope exit: every ABI entry that
// switches devices leaves the caller's (e.g. torch's) current device as it found it.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// RT_OK when `device` is a visible HIP device; RT_ERR_DEVICE without any, RT_ERR_INVALID else
inline int device_ok(const char* who, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return set_error(RT_ERR_DEVICE, "%s: no HIP device available", who);
  }
  if (device < 0 || device >= ndev)
    return set_error(RT_ERR_INVALID, "%s: device %d of %d", who, device, ndev);
  return RT_OK;
}

// A runtime flag as a compile-time constant, f(std::true_type{}) or f(std::false_type{}): how a
// host path picks a kernel instance by its template arguments (rt_aov.hip, rt_temporal.hip)
template <class F>
void with_flag(bool v, F&& f) { v ? f(std::true_type{}) : f(std::false_type{}); }

// ------------------------------------------------------------------- owners ---
// Device memory, streams and events belong to one of the types below, and each frees what it
// holds when it is destroyed.  None of them records or switches the device: whoever allocates
// from, resets or destroys an owner has the owner's device current, as the entries have after
// their hipSetDevice and as release_device, free_accum and RcclGather::release make it before
// they delete.  `who` names the ABI entry in the error message.

// A failed allocation, reported the same way by every owner: out of memory is RT_ERR_OOM,
// anything else RT_ERR_DEVICE, and HIP's last error is cleared (a failed hipMalloc is not
// sticky: the next hipGetLastError of the thread would report it as a launch failure).
inline int alloc_failed(const char* who, size_t bytes, hipError_t e) {
  (void)hipGetLastError();
  return set_error(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_DEVICE, "%s: device allocation of %zu bytes: %s",
                   who, bytes, hipGetErrorString(e));
}

// Allocations that die together: a scene's device copy, a render slot's buffers, one build.
struct DevicePool {
  std::vector<void*> allocs;
  DevicePool() = default;
  DevicePool(const DevicePool&) = delete;
  DevicePool& operator=(const DevicePool&) = delete;
  ~DevicePool() {
    for (void* p : allocs) (void)hipFree(p);
  }
  // `bytes` (> 0) or nothing: false without a word in rt_last_error, for a caller with a fallback
  bool try_alloc(void** out, size_t bytes, hipError_t* err = nullptr) {
    const hipError_t e = hipMalloc(out, bytes);
    if (err) *err = e;
    if (e != hipSuccess) {
      (void)hipGetLastError();
      *out = nullptr;
      return false;
    }
    allocs.push_back(*out);
    return true;
  }
  // count elements, a zero count rounded up to one
  template <typename T>
  int alloc(T** out, size_t count, const char* who) {
    const size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e;
    return try_alloc((void**)out, bytes, &e) ? RT_OK : alloc_failed(who, bytes, e);
  }
  // v's copy on the device; an empty v is a null pointer and no allocation
  template <typename T>
  int upload(const std::vector<T>& v, const T** out, const char* who) {
    *out = nullptr;
    if (v.empty()) return RT_OK;
    T* p = nullptr;
    const int rc = alloc(&p, v.size(), who);
    if (rc) return rc;
    HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = p;
    return RT_OK;
  }
  // one buffer ahead of the rest (a grow-on-demand member about to be replaced or dropped)
  template <typename T>
  int free(T** p) {
    if (!*p) return RT_OK;
    HIP_OK(hipFree(*p));
    allocs.erase(std::find(allocs.begin(), allocs.end(), (void*)*p));
    *p = nullptr;
    return RT_OK;
  }
};

// One allocation and its size; move-only.
struct DeviceBuffer {
  void* p = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  ~DeviceBuffer() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // at least `need` bytes (zero rounded up to one); the contents do not survive growing, and a
  // failure leaves the buffer empty: the old allocation is freed before the new one is made
  int grow(size_t need, const char* who) {
    if (p && bytes >= need) return RT_OK;
    reset();
    const size_t n = need ? need : 1;
    const hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      return alloc_failed(who, n, e);
    }
    bytes = n;
    return RT_OK;
  }
};

// A non-blocking stream, created on first use; move-only.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
  ~Stream() { reset(); }
  void reset() {
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
  }
  // the caller's stream when it gave one, else this one
  int pick(void* callers, hipStream_t* out) {
    if (!callers && !s) HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = callers ? (hipStream_t)callers : s;
    return RT_OK;
  }
  int ensure() { hipStream_t made; return pick(nullptr, &made); }
};

// Events created as they are first needed and kept for reuse.
struct Events {
  std::vector<hipEvent_t> ev;
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  ~Events() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  // at least n events, the new ones with `flags` (hipEventDefault, hipEventDisableTiming)
  int ensure(size_t n, unsigned flags) {
    while (ev.size() < n) {
      hipEvent_t e;
      HIP_OK(hipEventCreateWithFlags(&e, flags));
      ev.push_back(e);
    }
    return RT_OK;
  }
};

// Grow-only device scratch, one buffer per device ordinal (`device` is current), for a file-scope
// instance: no allocation per call once warm.  The buffers are never deleted: they live as long
// as the process, so nothing is freed while the runtime unloads.  The caller serialises its
// users, and no work that reads an old buffer may be in flight when a larger one is asked for.
struct DeviceScratch {
  std::vector<DeviceBuffer*> buf;
  int get(int device, size_t bytes, void** out, const char* who) {
    if ((int)buf.size() <= device) buf.resize(device + 1, nullptr);
    if (!buf[device]) buf[device] = new DeviceBuffer();
    const int rc = bytes ? buf[device]->grow(bytes, who) : RT_OK;
    *out = buf[device]->p;
    return rc;
  }
};

}  // namespace rt
