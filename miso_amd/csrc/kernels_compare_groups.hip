// kernels_compare_groups.hip -- every pair of two groups of samples in one device pass (miso_batch_compare_groups,
// include/miso_amd.h; miso_amd/samples_utils.py --compare-groups): kernel and host driver.
//
// Biological replicates are compared pair by pair (compare_miso, misopy/hypothesis_test.py:186-345, once per pair;
// filter_events.py --votes counts the pairs).  compare_kernel run n1 * n2 times fetches every sample column n2 (or n1)
// times with a stride of K doubles.  Here one workgroup per (event, isoform) copies the columns into LDS once -- contiguous
// there: lane l reads double l of a 256-B bank row, conflict-free for ds_read_b64 -- and runs compare_column
// (compare_column.hpp, the text compare_kernel runs) over every pair: the same 256-strided partial sums and the same tree,
// so the same bits.
//
// What is staged (MISO_STAGE_*): both groups (n1 + n2 columns), the smaller group only (the other group's columns come from
// global memory, min(n1, n2) times each, L2-resident after the first), or nothing.  More LDS per workgroup = fewer
// workgroups per CU to hide miso_det_exp's latency behind.  MISO_STAGE_AUTO takes the first that fits; which is fastest is
// for tools/compare_groups_bench.py to say ("Measured").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch.hpp"
#include "column_pass.hpp"
#include "compare_column.hpp"

namespace miso {

// FIRST / SECOND: group 1's / group 2's columns are staged.  A kernel per combination: one kernel with all four inlined
// compare_column variants needed 254 VGPRs.  As built for gfx950: both staged 111 VGPRs (compare_kernel: 89); the variants
// that read columns from global memory 177 (first staged), 243 (second staged) and 240 (none) -- the cached path's 32
// 64-bit row offsets are invariant over the pair loop and stay in registers -- i.e. two waves per SIMD; none spills VGPRs.
template <bool FIRST, bool SECOND>
__global__ __launch_bounds__(256) void compare_groups_kernel(const DevEvent *const *__restrict__ evs,
                                                             const unsigned char *const *__restrict__ pools,
                                                             int n1, int n2, int n_events, int S, double smoothing,
                                                             const uint64_t *cmp_off, uint64_t tot, double *out) {
  extern __shared__ double cols[];          // the staged columns, S doubles each
  __shared__ CompareScratch sc;
  const int ev = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  if (ev >= n_events) return;
  const int K = evs[0][ev].K;
  if (k >= K) return;
  // (workgroup-uniform, and said so: a base address in scalar registers, one 32-bit offset per lane and load)
  auto column = [&](int c) {
    const uint64_t a = reinterpret_cast<uint64_t>(pools[c] + evs[c][ev].off_samples) + 8ull * k;
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(a));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(a >> 32));
    return (GlobalColumn) reinterpret_cast<const double *>(static_cast<uint64_t>(hi) << 32 | lo);
  };
  const int c_lo = FIRST ? 0 : n1, c_hi = SECOND ? n1 + n2 : (FIRST ? n1 : c_lo);
  for (int c = c_lo; c < c_hi; c++) {
    const GlobalColumn x = column(c);
    double *dst = cols + static_cast<size_t>(c - c_lo) * S;
#pragma unroll 4
    for (int s = t; s < S; s += 256) dst[s] = x[static_cast<size_t>(s) * K];
  }
  const double *lds2 = cols + (FIRST ? static_cast<size_t>(n1) * S : 0);
  const bool cached = S <= 256 * SUMMARY_CACHE;
  for (int i = 0; i < n1; i++) {
    // (the address spaces are known at compile time: LDS columns are read with ds_read_b64, not through flat pointers)
    const double *a1 = cols + static_cast<size_t>(i) * S;
    const GlobalColumn ag = FIRST ? nullptr : column(i);
    for (int j = 0; j < n2; j++) {
      __syncthreads();                        // the staged columns are there; the pair before is done with `sc`
      double *o = out + static_cast<size_t>(i * n2 + j) * tot + cmp_off[ev] + 4 * k;
      const double *b1 = lds2 + static_cast<size_t>(j) * S;
      auto run = [&](auto a, int ka, auto b, int kb) {
        if (cached) compare_column<true>(a, ka, b, kb, S, smoothing, o, sc);
        else compare_column<false>(a, ka, b, kb, S, smoothing, o, sc);
      };
      if constexpr (FIRST && SECOND) run(a1, 1, b1, 1);
      else if constexpr (FIRST) run(a1, 1, column(n1 + j), K);
      else if constexpr (SECOND) run(ag, K, b1, 1);
      else run(ag, K, column(n1 + j), K);
    }
  }
}

// Which columns a workgroup of compare_groups_kernel can keep in LDS: `budget` bytes of dynamic LDS, S doubles a column.
int compare_groups_staging(int n1, int n2, int S, size_t budget) {
  const size_t col = static_cast<size_t>(S) * 8;
  if (static_cast<size_t>(n1 + n2) * col <= budget) return MISO_STAGE_BOTH;
  if (static_cast<size_t>(std::min(n1, n2)) * col <= budget) return MISO_STAGE_SMALLER;
  return MISO_STAGE_NONE;
}

// (a HIP runtime failure is MISO_ENODEVICE as everywhere in runtime.hip -- include/miso_amd.h: "no usable HIP device / HIP
// runtime error" -- except memory: a call whose n1 * n2 results do not fit is MISO_ENOMEM, MemoryError in Python: HipCall::alloc)
void compare_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, double smoothing, int staging,
                    double *out, int64_t out_len, float *kernel_ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the comparison has no CPU path");
  if (!(smoothing > 0)) MISO_FAIL(MISO_EINVAL, "Invalid smoothing parameter");
  if (staging < MISO_STAGE_AUTO || staging > MISO_STAGE_NONE) MISO_FAIL(MISO_EINVAL, "Invalid staging");
  const std::vector<miso_batch *> all = same_events_groups(g1, n1, g2, n2);
  miso_batch &r = *all[0];
  const int n = static_cast<int>(r.events.size()), S = r.S(), nb = n1 + n2;
  if (S < 2) MISO_FAIL(MISO_EINVAL, "Too few samples to compare");
  const ColumnLayout l = column_layout(r, 4);
  const uint64_t tot = l.total, need_len = static_cast<uint64_t>(n1) * n2 * tot;
  if (out_len < 0 || static_cast<uint64_t>(out_len) < need_len) MISO_FAIL(MISO_EINVAL, "out is too short for n1 * n2 * tot doubles");
  if (need_len && !out) MISO_FAIL(MISO_EINVAL, "out is NULL");
  if (kernel_ms) *kernel_ms = 0.f;
  if (n == 0) return;
  HIP_OK(hipSetDevice(r.device));
  for (miso_batch *b : all) { finish_rounds(*b); HIP_OK(hipStreamSynchronize(b->stream)); }

  // the LDS a workgroup may have beside the kernel's own reduction buffers
  int lds_max = 0;
  HIP_OK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, r.device));
  hipDeviceProp_t prop{};
  HIP_OK(hipGetDeviceProperties(&prop, r.device));
  // (gfx950: 160 KiB per CU, all of it open to one workgroup, whatever the attribute says)
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) == 0) lds_max = std::max(lds_max, 160 * 1024);
  using Kernel = void (*)(const DevEvent *const *, const unsigned char *const *, int, int, int, int, double, const uint64_t *,
                          uint64_t, double *);
  const Kernel kernels[4] = {compare_groups_kernel<false, false>, compare_groups_kernel<true, true>,
                             compare_groups_kernel<true, false>, compare_groups_kernel<false, true>};
  hipFuncAttributes fa{};
  HIP_OK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(kernels[1])));
  const size_t budget = static_cast<size_t>(lds_max) > fa.sharedSizeBytes ? lds_max - fa.sharedSizeBytes : 0;
  const size_t col = static_cast<size_t>(S) * 8;
  if (staging == MISO_STAGE_AUTO) staging = compare_groups_staging(n1, n2, S, budget);
  const size_t dyn = staging == MISO_STAGE_BOTH ? nb * col : staging == MISO_STAGE_SMALLER ? std::min(n1, n2) * col : 0;
  if (dyn > budget) MISO_FAIL(MISO_EINVAL, "The requested staging does not fit the workgroup's LDS");
  const Kernel kernel = kernels[staging == MISO_STAGE_BOTH ? 1 : staging == MISO_STAGE_NONE ? 0 : (n1 <= n2 ? 2 : 3)];

  const std::vector<const void *> ptrs = group_pointers(all);
  HipCall call(r.stream);
  const void *const *d_ptrs = call.upload(ptrs.data(), ptrs.size() * sizeof(void *));
  const float ms = column_pass(call, fn(kernel), dim3(n, l.kmax), dyn, l.off, need_len, out,
                               [&](dim3 grid, const uint64_t *d_off, double *d_cmp) {
                                 hipLaunchKernelGGL(kernel, grid, dim3(256), dyn, call.st, reinterpret_cast<const DevEvent *const *>(d_ptrs),
                                                    reinterpret_cast<const unsigned char *const *>(d_ptrs) + nb, n1, n2, n, S, smoothing,
                                                    d_off, tot, d_cmp);
                               });
  if (kernel_ms) *kernel_ms = ms;
}

}  // namespace miso
