// hip_host.hpp -- host-side launch glue shared by the units under csrc/: the check of a HIP call, a wall clock, and what one
// one-shot call holds on the device: the exact-posterior units' and every pass over the resident sample pool
// (column_pass.hpp).  (The pooled, multi-stream Scratch objects of the coverage, density, text and insert passes are their
// own.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "host.hpp"

// a failed HIP call: MISO_ENODEVICE with the call's text and HIP's reason
#define HIP_OK(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      MISO_FAIL(MISO_ENODEVICE, std::string(#call) + ": " + hipGetErrorString(e_));        \
  } while (0)
// ... where running out of device memory is the caller's to act on: MISO_ENOMEM for that
#define HIP_OK_OR_NOMEM(call)                                                              \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      MISO_FAIL(e_ == hipErrorOutOfMemory ? MISO_ENOMEM : MISO_ENODEVICE,                  \
                std::string(#call) + ": " + hipGetErrorString(e_));                        \
  } while (0)

namespace miso {

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// What a single call holds: the stream it works on -- the one given (a batch's own) or, none given, a non-blocking one of
// its own, so that no other stream of the process waits --, its device buffers and, if asked for, the event pair around its
// kernels.  Everything is released on every way out, a failed call's included.
struct HipCall {
  hipStream_t st;
  explicit HipCall(hipStream_t given) : st(given) {
    if (!st) { HIP_OK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking)); st = own; }
  }
  HipCall(const HipCall &) = delete;
  HipCall &operator=(const HipCall &) = delete;
  ~HipCall() {
    for (void *p : bufs) (void) hipFree(p);
    if (e0) (void) hipEventDestroy(e0);
    if (e1) (void) hipEventDestroy(e1);
    if (own) (void) hipStreamDestroy(own);
  }
  // `bytes` of device memory, rounded up to 16 (and 16 at least); none left: MISO_ENOMEM
  template <class T = double> T *alloc(size_t bytes) {
    bufs.push_back(nullptr);
    HIP_OK_OR_NOMEM(hipMalloc(&bufs.back(), (std::max<size_t>(bytes, 1) + 15) & ~size_t{15}));
    return static_cast<T *>(bufs.back());
  }
  // a device copy of a host array, queued on the stream
  template <class T> T *upload(const T *src, size_t bytes) {
    T *d = alloc<T>(bytes);
    if (src && bytes) HIP_OK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st));
    return d;
  }
  // the HIP-event time between start() and stop(), once the stream has been synchronised
  void start() { HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1)); HIP_OK(hipEventRecord(e0, st)); }
  void stop() { HIP_OK(hipEventRecord(e1, st)); }
  float elapsed_ms() { float ms = 0.f; HIP_OK(hipEventElapsedTime(&ms, e0, e1)); return ms; }

 private:
  hipStream_t own = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<void *> bufs;
};

}  // namespace miso
