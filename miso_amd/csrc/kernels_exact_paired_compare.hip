// kernels_exact_paired_compare.hip -- two paired-end exact-mode posteriors of one event compared without a draw
// (miso_batch_compare_exact_paired).
//
// Sample s has the density of kernels_exact_paired.hip,
//     log p_s(x) = (n10_s + h0_s - 1) log x + (n01_s + h1_s - 1) log y + P_s(x) - n_s log(x A0_s + y A1_s),
// P_s the sum over that sample's drawing pairs.  kernels_exact_compare.hip's reduction to five pooled numbers does not
// apply: the A differ between the samples (each sample has its own fragment-length law), and the pair sums do not pool.
// But p_1 p_2 is again an explicit density -- ExactSecondSegment in exact_paired.hpp: pooled exponents, hyperparameters
// h1 + h2 - 1, both pair sums, both denominators -- with g'' >= -(n1 + n2 + h0p + h1p) / 4, so the two-pass window and the
// fourth-order table of the paired mode tabulate it as they tabulate one sample's.  From there on everything is
// kernels_exact_compare.hip's:
//     log_d0 = (lZ12 - lZ1) - lZ2,  log Z = gref + log(F[G]);  log_bf = log_prior0 - log_d0 (log_prior0 from the host);
//     H(z) = P(psi_1 - psi_2 <= z): the trapezoid sum over the 2049 points of A, the posterior with the narrower window in
//     psi (a tie: sample 1), of w f_A / sum w f_A times B's tabulated CDF at the shifted argument (exact_cdf_at).
// One thing differs: A's f cannot be made again from scalars, it needs A's pair sum.  After A's table every lane writes the f
// of its own 32 points (33: lane 63) to the workgroup's row of a global buffer, point j of lane l at [64 j + l] so that the
// wavefront's accesses are contiguous, and reads them back in the quadrature; x and 1 - x there come from exact_point.
//
// ONE WAVEFRONT = one workgroup per pair, ExactPairedLds's 37 KB holding one F / f pair at a time: windows of both samples,
// table of A (scalars and own f kept), window and table of the pooled density (Z12, gref12), table of B, which stays for
// the n_z quadratures.  f64, no contraction, miso_det_exp / miso_det_log, IEEE division, no atomics;
// tests/_exact_paired_compare_ref.py restates it operation by operation (tests/test_gpu_exact_paired_compare.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"

#include "exact_paired.hpp"

namespace miso {

constexpr int EXPC_MAX_Z = 8;
constexpr double EXPC_BF_CAP = 1e12;
constexpr double EXPC_LN10 = 2.302585092994046;
constexpr int EXPC_ROW = EXACT_G + 64;      // doubles of a workgroup's row of A's f: 64 j + l, the grid's last point at 2048; 512-byte rows
constexpr int EXPC_LAUNCH = 8192;           // pairs per launch: bounds the rows' buffer (138 MB)

struct ExactPairedCmpLds {
  double F[EXACT_PAD], f[EXACT_PAD], red[256], mbuf[2 * EXP_CHUNK], fext[2];
  int redi[128];
};

// the tabulated, unnormalised CDF at psi = u; v = 1 - psi, computed on its own (kernels_exact_compare.hip's, operation by
// operation: that unit's function is not in a header, and stays where it is)
__device__ __forceinline__ double exact_paired_cdf_at(const ExactTable &T, double u, double v) {
  const bool uin = u > 0.0, vin = v > 0.0;
  const double t = miso_det_log(uin ? u : 1.0) - miso_det_log(vin ? v : 1.0);
  double s = (t - T.tL) / T.h;
  s = s > 0.0 ? s : 0.0;
  s = s < static_cast<double>(EXACT_G) ? s : static_cast<double>(EXACT_G);
  int j = static_cast<int>(s);
  j = j < EXACT_G - 1 ? j : EXACT_G - 1;   // 0 .. G - 1
  const double fr = s - static_cast<double>(j);
  const double F0 = T.F[exact_idx(j)], F1 = T.F[exact_idx(j + 1)];
  const double m0 = T.h * T.f[exact_idx(j)], m1 = T.h * T.f[exact_idx(j + 1)];
  const double dF = F1 - F0;
  const double c2 = (3.0 * dF - 2.0 * m0) - m1, c3 = (m0 + m1) - 2.0 * dF;
  double val = F0 + (m0 + fr * (c2 + fr * c3)) * fr;
  val = val > T.Z ? T.Z : val;
  val = val < 0.0 ? 0.0 : val;
  val = t >= T.tR ? T.Z : val;
  val = uin ? val : 0.0;
  val = vin ? val : T.Z;
  return val;
}

// the 64 lanes' values added in lane order (red: 64 doubles of LDS)
__device__ __forceinline__ double exact_paired_lanes_sum(double v, double *red, int lane) {
  red[lane] = v;
  __syncthreads();
  double s = 0.0;
  for (int m = 0; m < 64; m++) s = s + red[m];
  __syncthreads();
  return s;
}

// A value every lane holds alike, moved to scalar registers (the same bits).  The statistics, windows and table scalars of
// three densities live across five sweeps over the pairs; as vector registers they would not fit beside a sweep's points.
__device__ __forceinline__ double exact_uni(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ ExactStats exact_uni(const ExactStats &s) {
  return ExactStats{exact_uni(s.am1), exact_uni(s.bm1), exact_uni(s.a), exact_uni(s.b), exact_uni(s.c), exact_uni(s.n), exact_uni(s.e0), exact_uni(s.e1)};
}
__device__ __forceinline__ ExactTable exact_uni(const ExactTable &T) {
  return ExactTable{exact_uni(T.tm), exact_uni(T.gmax), exact_uni(T.tL), exact_uni(T.tR), exact_uni(T.h), exact_uni(T.Z), exact_uni(T.mean0),
                    exact_uni(T.mean1), exact_uni(T.sf), T.F, T.f};
}

// pair i of one sample: its statistics, c8 and drawing pairs
__device__ __forceinline__ void exact_paired_cmp_side(const ExactPairedCmpSide &sd, const int32_t *list, int i, ExactStats &st, double &c8,
                                                      ExactPairs &pr) {
  const double *q = sd.stats6 + 6 * static_cast<size_t>(i);
  if (sd.mm) {
    pr.rec = nullptr; pr.fp = nullptr; pr.il = 0;
    pr.mm = sd.mm + 2 * static_cast<size_t>(sd.offs[i]); pr.n = static_cast<int>(sd.offs[i + 1] - sd.offs[i]);
  } else {
    const DevEvent E = sd.events[list[i]];
    pr.rec = reinterpret_cast<const uint32_t *>(sd.in_pool + E.off_draw);   // plain records: u16 f0, f1 per pair
    pr.fp = sd.frag_prob; pr.il = sd.il; pr.mm = nullptr; pr.n = E.n_draw;
  }
  const double nn = (q[0] + q[1]) + static_cast<double>(pr.n), hm0 = q[4] - 1.0, hm1 = q[5] - 1.0;
  st = exact_uni(exact_stats(q[0], q[1], nn, q[2], q[3], hm0, hm1));
  c8 = exact_uni((nn + ((hm0 + 1.0) + (hm1 + 1.0))) * 0.03125);   // (n + h0 + h1) / 32 as kernels_exact_paired.hip makes it
}

// One workgroup = one wavefront = pair first + blockIdx.x.  out: 5 + n_z doubles per pair; frow: EXPC_ROW doubles per
// workgroup of the launch (unused, and may be null, when n_z = 0).
__global__ __launch_bounds__(64) void exact_paired_compare(const ExactPairedCmpSide s1, const ExactPairedCmpSide s2, const int32_t *list,
                                                           const double *log_prior0, int first, int n, const double *z, int n_z,
                                                           double *out, double *frow) {
  __shared__ ExactPairedCmpLds L;
  const int lane = threadIdx.x;
  const int i = first + static_cast<int>(blockIdx.x);
  if (i >= n) return;   // (uniform: the whole workgroup)
  ExactStats st1, st2; double c81, c82; ExactPairs pr1, pr2;
  exact_paired_cmp_side(s1, list, i, st1, c81, pr1);
  exact_paired_cmp_side(s2, list, i, st2, c82, pr2);
  const double *q1 = s1.stats6 + 6 * static_cast<size_t>(i), *q2 = s2.stats6 + 6 * static_cast<size_t>(i);
  // the pooled density: exponents, hyperparameters h1 + h2 - 1 and c = (a + b) - (n1 + n2) in st12, whose n, e0, e1 are sample
  // 1's; sample 2's pair count, A and pairs are the second segment
  const double hm0 = ((q1[4] + q2[4]) - 1.0) - 1.0, hm1 = ((q1[5] + q2[5]) - 1.0) - 1.0;
  const double n12 = st1.n + st2.n;
  ExactStats st12 = exact_stats(q1[0] + q2[0], q1[1] + q2[1], n12, st1.e0, st1.e1, hm0, hm1);
  st12.n = st1.n;
  st12 = exact_uni(st12);
  const ExactSecondSegment seg2{st2.n, st2.e0, st2.e1, pr2};
  const double c812 = exact_uni((n12 + ((hm0 + 1.0) + (hm1 + 1.0))) * 0.03125);

  const ExactTable W1 = exact_uni(exact_paired_window(st1, c81, pr1, L.mbuf, L.red, L.redi, lane));
  const ExactTable W2 = exact_uni(exact_paired_window(st2, c82, pr2, L.mbuf, L.red, L.redi, lane));
  const double w1 = exact_point(st1, W1.tR).x - exact_point(st1, W1.tL).x;
  const double w2 = exact_point(st2, W2.tR).x - exact_point(st2, W2.tL).x;
  const bool a2 = exact_uni(w2) < exact_uni(w1);   // A = sample 2
  const ExactStats stA = a2 ? st2 : st1, stB = a2 ? st1 : st2;
  const ExactPairs prA = a2 ? pr2 : pr1, prB = a2 ? pr1 : pr2;
  const ExactTable TA = exact_uni(exact_paired_table(stA, a2 ? W2 : W1, prA, L.mbuf, L.F, L.f, L.fext, L.red, lane));   // (its scalars and f are used from here on)
  const int i0 = EXACT_CELLS * lane;
  double *row = frow + static_cast<size_t>(EXPC_ROW) * blockIdx.x;
  if (n_z > 0) {
    for (int j = 0; j < EXACT_CELLS; j++) row[64 * j + lane] = L.f[exact_idx(i0 + j)];
    if (lane == 63) row[EXACT_G] = L.f[exact_idx(EXACT_G)];
  }
  __syncthreads();
  const ExactTable W12 = exact_uni(exact_paired_window(st12, c812, pr1, L.mbuf, L.red, L.redi, lane, seg2));
  const ExactTable T12 = exact_uni(exact_paired_table(st12, W12, pr1, L.mbuf, L.F, L.f, L.fext, L.red, lane, seg2));
  __syncthreads();
  const ExactTable TB = exact_paired_table(stB, a2 ? W1 : W2, prB, L.mbuf, L.F, L.f, L.fext, L.red, lane);
  const double lzA = TA.gmax + miso_det_log(TA.Z), lzB = TB.gmax + miso_det_log(TB.Z), lz12 = T12.gmax + miso_det_log(T12.Z);
  const double lz1 = a2 ? lzB : lzA, lz2 = a2 ? lzA : lzB;
  const double log_d0 = (lz12 - lz1) - lz2;
  const double log_bf = log_prior0[i] - log_d0;
  double bf = miso_det_exp(log_bf);
  bf = bf > EXPC_BF_CAP ? EXPC_BF_CAP : bf;
  double *o = out + static_cast<size_t>(5 + n_z) * static_cast<size_t>(i);
  if (lane == 0) {
    o[0] = a2 ? TB.mean0 : TA.mean0; o[1] = a2 ? TA.mean0 : TB.mean0;
    o[2] = log_d0; o[3] = bf; o[4] = log_bf / EXPC_LN10;
  }
  if (n_z <= 0) return;
  // the quadratures on A's grid, one z after the other (no unrolling over z: the tables' stages set this kernel's registers,
  // the quadratures are a hundredth of its time)
  const int n_own = EXACT_CELLS + (lane == 63 ? 1 : 0);   // the last lane owns the grid's last point too
#pragma unroll 1
  for (int k = 0; k < n_z; k++) {
    const double zk = z[k];
    double acc = 0.0;
#pragma unroll 1
    for (int j = 0; j < n_own; j++) {
      const int pt = i0 + j;
      const ExactPoint p = exact_point(stA, TA.tL + TA.h * static_cast<double>(pt));
      const double fa = j < EXACT_CELLS ? row[64 * j + lane] : row[EXACT_G];
      const double wf = ((pt == 0 || pt == EXACT_G) ? 0.5 : 1.0) * fa;
      const double val = a2 ? exact_paired_cdf_at(TB, p.x + zk, p.y - zk) : exact_paired_cdf_at(TB, p.x - zk, p.y + zk);
      acc = acc + wf * (val / TB.Z);
    }
    const double s = exact_paired_lanes_sum(acc, L.red, lane) / TA.sf;
    if (lane == 0) o[5 + k] = a2 ? s : 1.0 - s;
  }
}

#define HIP_OK(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      MISO_FAIL(MISO_ENODEVICE, std::string(#call) + ": " + hipGetErrorString(e_));        \
  } while (0)

// log of the prior density of psi_1 - psi_2 at 0 (kernels_exact_compare.hip exact_log_prior0 on stats6's h0, h1)
static double exact_paired_log_prior0(const double *q1, const double *q2) {
  const double h0p = (q1[4] + q2[4]) - 1.0, h1p = (q1[5] + q2[5]) - 1.0;
  double lp = (std::lgamma(h0p) + std::lgamma(h1p)) - std::lgamma(h0p + h1p);
  for (const double *q : {q1, q2}) lp = lp - ((std::lgamma(q[4]) + std::lgamma(q[5])) - std::lgamma(q[4] + q[5]));
  return lp;
}

// side[s]: stats6 (host), n rows; then EITHER m / offs (host: the selftest's caller-given probabilities, validated here) OR
// src (device pointers of a batch) with list (host, n event indices, the same for both samples).
void exact_paired_compare_run(const ExactPairedCmpInput &in1, const ExactPairedCmpInput &in2, const int32_t *list, int n, const double *z,
                              int n_z, double *out, hipStream_t st, float *ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0) MISO_FAIL(MISO_EINVAL, "Negative pair count");
  if (n_z < 0 || n_z > EXPC_MAX_Z) MISO_FAIL(MISO_EINVAL, "The number of delta psi points must lie in [0, 8]");
  for (int j = 0; j < n_z; j++) if (!(z[j] > -1.0 && z[j] < 1.0)) MISO_FAIL(MISO_EINVAL, "A delta psi point must lie inside (-1, 1)");
  const ExactPairedCmpInput *in[2] = {&in1, &in2};
  int64_t n_pairs[2] = {0, 0};
  for (int s = 0; s < 2 && n > 0; s++) {
    const ExactPairedCmpInput &I = *in[s];
    for (int i = 0; i < n; i++) {
      const double *q = I.stats6 + 6 * static_cast<size_t>(i);
      if (!(q[0] >= 0 && q[1] >= 0) || !exact_paired_eligible(2, q + 2, q + 4, false))
        MISO_FAIL(MISO_EINVAL, "An element is not eligible for the paired exact mode");
    }
    if (!I.m) continue;
    if (I.offs[0] != 0) MISO_FAIL(MISO_EINVAL, "The pair offsets must start at 0");
    for (int i = 0; i < n; i++)
      if (I.offs[i + 1] < I.offs[i] || I.offs[i + 1] - I.offs[i] > INT32_MAX) MISO_FAIL(MISO_EINVAL, "The pair offsets must ascend");
    n_pairs[s] = I.offs[n];
    for (int64_t r = 0; r < 2 * n_pairs[s]; r++)
      if (!(I.m[r] >= EXACT_PAIRED_MIN_PROB && I.m[r] <= 1.0)) MISO_FAIL(MISO_EINVAL, "A pair probability outside [2^-63, 1]");
  }
  std::vector<double> lp(std::max(n, 1));
  for (int i = 0; i < n; i++) lp[i] = exact_paired_log_prior0(in1.stats6 + 6 * static_cast<size_t>(i), in2.stats6 + 6 * static_cast<size_t>(i));
  if (ms) *ms = 0.f;
  if (n == 0) return;
  struct Held {   // freed on every way out, a failed call's included
    void *p[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipStream_t own = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Held() {
      for (void *q : p) if (q) (void) hipFree(q);
      if (e0) (void) hipEventDestroy(e0);
      if (e1) (void) hipEventDestroy(e1);
      if (own) (void) hipStreamDestroy(own);
    }
  } held;
  if (!st) { HIP_OK(hipStreamCreateWithFlags(&held.own, hipStreamNonBlocking)); st = held.own; }
  int slot = 0;
  auto up = [&](const void *src, size_t bytes) -> void * {   // a device copy of a host array (16 bytes at least)
    void *&d = held.p[slot++];
    HIP_OK(hipMalloc(&d, std::max<size_t>(bytes, 16)));
    if (src && bytes) HIP_OK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st));
    return d;
  };
  ExactPairedCmpSide side[2];
  for (int s = 0; s < 2; s++) {
    const ExactPairedCmpInput &I = *in[s];
    side[s] = ExactPairedCmpSide{};
    side[s].stats6 = static_cast<const double *>(up(I.stats6, static_cast<size_t>(n) * 6 * 8));
    if (I.m) {
      side[s].mm = static_cast<const double *>(up(I.m, static_cast<size_t>(n_pairs[s]) * 2 * 8));
      side[s].offs = static_cast<const int64_t *>(up(I.offs, static_cast<size_t>(n + 1) * 8));
    } else {
      side[s].events = I.events; side[s].in_pool = I.in_pool; side[s].frag_prob = I.frag_prob; side[s].il = I.il;
    }
  }
  const int32_t *d_list = (in1.m && in2.m) ? nullptr : static_cast<const int32_t *>(up(list, static_cast<size_t>(n) * 4));
  const double *d_lp = static_cast<const double *>(up(lp.data(), static_cast<size_t>(n) * 8));
  const double *d_z = static_cast<const double *>(up(z, static_cast<size_t>(n_z) * 8));
  const size_t ob = static_cast<size_t>(n) * (5 + n_z) * 8;
  double *d_o = static_cast<double *>(up(nullptr, ob));
  double *d_row = n_z ? static_cast<double *>(up(nullptr, static_cast<size_t>(std::min(n, EXPC_LAUNCH)) * EXPC_ROW * 8)) : nullptr;
  HIP_OK(hipEventCreate(&held.e0));
  HIP_OK(hipEventCreate(&held.e1));
  HIP_OK(hipEventRecord(held.e0, st));
  for (int first = 0; first < n; first += EXPC_LAUNCH) {   // (one stream: a launch's rows are free when the next begins)
    const int cnt = std::min(n - first, EXPC_LAUNCH);
    hipLaunchKernelGGL(exact_paired_compare, dim3(cnt), dim3(64), 0, st, side[0], side[1], d_list, d_lp, first, n, d_z, n_z, d_o, d_row);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipEventRecord(held.e1, st));
  HIP_OK(hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (ms) HIP_OK(hipEventElapsedTime(ms, held.e0, held.e1));
}

}  // namespace miso
