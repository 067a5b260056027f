// kernels_model_check.hip -- the posterior predictive model check of single-end events: do the event's reads
// fall into the gene's read classes as the model says they should?  No reference counterpart: users of the reference look at
// sashimi plots.  The kernel's body is model_check.hpp's, the arithmetic of one posterior row include/miso_model_check.h's;
// here are the kernel, the guards of a call and its launch (hip_host.hpp HipCall), for the raw call (miso_model_check) and
// the batch's pass (miso_batch::model_check, below) alike.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch.hpp"
#include "column_pass.hpp"
#include "hip_host.hpp"
#include "host.hpp"
#include "model_check.hpp"

namespace miso {

namespace {

// Grid: one workgroup per event; an event the host has ruled out (status) costs its workgroup one load.
__global__ __launch_bounds__(MC_BLOCK) void model_check_kernel(const ModelCheckArgs a, int n_events) {
  extern __shared__ double mc_acc[];
  const int ev = static_cast<int>(blockIdx.x);
  if (ev >= n_events || a.status[ev] != MISO_FIT_OK) return;
  model_check_event(a, ev, mc_acc);
}

constexpr int32_t MC_MAX_READS = 1 << 24;   // the sampler's own range (miso_binomial.h's table of log factorials)

}  // namespace

float model_check_run(const ModelCheckInput &in, const ModelCheckOutput &out, hipStream_t st) {
  const int n = in.n;
  if (n < 0) MISO_FAIL(MISO_EINVAL, "event count out of range");
  if (n == 0) return 0.f;
  if (!in.K || !in.C || !in.class_off || !in.sample_off || !in.S || !in.event_id) MISO_FAIL(MISO_EINVAL, "event arrays must not be NULL");
  if (in.class_off[0] != 0) MISO_FAIL(MISO_EINVAL, "class offsets start at 0");
  if (!in.h_samples && !in.d_samples) MISO_FAIL(MISO_EINVAL, "samples must not be NULL");
  // the guards: nothing the kernel indexes with may leave its array
  std::vector<int32_t> status(n), N(n, 0);
  int c_max = 1;
  int32_t n_max = 0;
  for (int i = 0; i < n; i++) {
    const std::string who = "event " + std::to_string(i) + ": ";
    const int64_t co = in.class_off[i], C64 = in.class_off[i + 1] - co;
    if (C64 < 0 || C64 != in.C[i]) MISO_FAIL(MISO_EINVAL, who + "class offsets do not match the class counts");
    if (in.K[i] < 1 || in.S[i] < 0) MISO_FAIL(MISO_EINVAL, who + "isoform or sample count out of range");
    status[i] = in.status_in ? in.status_in[i] : MISO_FIT_OK;
    if (status[i] != MISO_FIT_OK) continue;
    if (in.C[i] > MISO_FIT_MAX_CLASSES || in.K[i] > 64) { status[i] = MISO_FIT_TOO_MANY_CLASSES; continue; }
    if (in.C[i] < 1) MISO_FAIL(MISO_EINVAL, who + "an event with a gene has at least one class");
    if (!in.pattern || !in.m || !in.counts) MISO_FAIL(MISO_EINVAL, "class arrays must not be NULL");
    int64_t total = 0;
    const uint64_t valid = in.K[i] == 64 ? ~uint64_t{0} : ((uint64_t{1} << in.K[i]) - 1);
    for (int64_t c = co; c < co + C64; c++) {
      if (in.pattern[c] == 0 || (in.pattern[c] & ~valid)) MISO_FAIL(MISO_EINVAL, who + "a class pattern is empty or names an isoform the event does not have");
      if (in.m[c] < 1 || in.m[c] > (int64_t{1} << 40)) MISO_FAIL(MISO_EINVAL, who + "a class needs between 1 and 2^40 start positions");
      if (in.counts[c] < 0) MISO_FAIL(MISO_EINVAL, who + "negative read count");
      total += in.counts[c];
    }
    if (total > MC_MAX_READS) MISO_FAIL(MISO_EINVAL, who + "more than 2^24 reads");
    N[i] = static_cast<int32_t>(total);
    if (total == 0) { status[i] = MISO_FIT_NO_READS; continue; }
    const uint64_t need = static_cast<uint64_t>(in.K[i]) * static_cast<uint64_t>(in.S[i]);
    if (in.sample_off[i] > in.n_sample_doubles || need > in.n_sample_doubles - in.sample_off[i])
      MISO_FAIL(MISO_EINVAL, who + "sample rows lie outside the samples given");
    c_max = std::max(c_max, static_cast<int>(in.C[i]));
    n_max = std::max(n_max, N[i]);
  }
  const size_t n_cls = static_cast<size_t>(in.class_off[n]);
  std::vector<double> m_d(std::max<size_t>(n_cls, 1), 0.0);
  for (size_t c = 0; c < n_cls; c++) m_d[c] = in.m ? static_cast<double>(in.m[c]) : 0.0;
  std::vector<double> lf(static_cast<size_t>(n_max) + 1);
  miso_logfact_fill(lf.data(), static_cast<int32_t>(lf.size()));

  HipCall call(st);
  ModelCheckArgs a{};
  a.K = call.upload(in.K, n * sizeof(int32_t));
  a.C = call.upload(in.C, n * sizeof(int32_t));
  a.N = call.upload(N.data(), n * sizeof(int32_t));
  a.S = call.upload(in.S, n * sizeof(int32_t));
  a.status = call.upload(status.data(), n * sizeof(int32_t));
  a.class_off = call.upload(in.class_off, (static_cast<size_t>(n) + 1) * sizeof(int64_t));
  a.pattern = call.upload(in.pattern, n_cls * sizeof(uint64_t));
  a.m = call.upload(m_d.data(), n_cls * sizeof(double));
  a.n = call.upload(in.counts, n_cls * sizeof(int32_t));
  a.sample_off = call.upload(in.sample_off, n * sizeof(uint64_t));
  a.event_id = call.upload(in.event_id, n * sizeof(uint32_t));
  a.samples = in.d_samples ? in.d_samples : call.upload(in.h_samples, in.n_sample_doubles * sizeof(double));
  a.lf = call.upload(lf.data(), lf.size() * sizeof(double));
  a.seed = in.seed;
  // results: zeroed, so that an event the kernel leaves out reads as zeros
  const size_t b_int = static_cast<size_t>(n) * 3 * sizeof(int32_t), b_dbl = static_cast<size_t>(n) * 2 * sizeof(double);
  const size_t b_exp = std::max<size_t>(n_cls, 1) * sizeof(double), b_tail = std::max<size_t>(n_cls, 1) * sizeof(int32_t);
  a.ev_int = call.alloc<int32_t>(b_int);
  a.ev_dbl = call.alloc<double>(b_dbl);
  a.expected = call.alloc<double>(b_exp);
  a.ge = call.alloc<int32_t>(b_tail);
  a.le = call.alloc<int32_t>(b_tail);
  HIP_OK(hipMemsetAsync(a.ev_int, 0, b_int, call.st));
  HIP_OK(hipMemsetAsync(a.ev_dbl, 0, b_dbl, call.st));
  HIP_OK(hipMemsetAsync(a.expected, 0, b_exp, call.st));
  HIP_OK(hipMemsetAsync(a.ge, 0, b_tail, call.st));
  HIP_OK(hipMemsetAsync(a.le, 0, b_tail, call.st));

  // (thread t's running sum of every class's p_c: c_max x 256 doubles, 128 KiB at 64 classes, 6 KiB at three)
  const size_t dyn = static_cast<size_t>(c_max) * MC_BLOCK * sizeof(double);
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(model_check_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             static_cast<int>(dyn)));
  std::vector<int32_t> ev_int(static_cast<size_t>(n) * 3), ge(std::max<size_t>(n_cls, 1)), le(std::max<size_t>(n_cls, 1));
  std::vector<double> ev_dbl(static_cast<size_t>(n) * 2), expected(std::max<size_t>(n_cls, 1));
  call.start();
  hipLaunchKernelGGL(model_check_kernel, dim3(n), dim3(MC_BLOCK), dyn, call.st, a, n);
  HIP_OK(hipGetLastError());
  call.stop();
  HIP_OK(hipMemcpyAsync(ev_int.data(), a.ev_int, b_int, hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipMemcpyAsync(ev_dbl.data(), a.ev_dbl, b_dbl, hipMemcpyDeviceToHost, call.st));
  if (n_cls) {
    HIP_OK(hipMemcpyAsync(expected.data(), a.expected, n_cls * sizeof(double), hipMemcpyDeviceToHost, call.st));
    HIP_OK(hipMemcpyAsync(ge.data(), a.ge, n_cls * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
    HIP_OK(hipMemcpyAsync(le.data(), a.le, n_cls * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
  }
  HIP_OK(hipStreamSynchronize(call.st));
  const float ms = call.elapsed_ms();

  // only now, the call having succeeded, the caller's arrays change
  for (int i = 0; i < n; i++) {
    const bool ran = status[i] == MISO_FIT_OK;
    if (ran && ev_int[3 * i] == 0) status[i] = MISO_FIT_NO_ROWS;
    const bool ok = status[i] == MISO_FIT_OK;
    out.status[i] = status[i];
    out.rows[i] = ok ? ev_int[3 * i] : 0;
    out.bad_rows[i] = ran ? ev_int[3 * i + 1] : 0;
    out.exceed[i] = ok ? ev_int[3 * i + 2] : 0;
    out.sum_obs[i] = ok ? ev_dbl[2 * i] : 0.0;
    out.sum_rep[i] = ok ? ev_dbl[2 * i + 1] : 0.0;
    for (int64_t c = in.class_off[i]; c < in.class_off[i + 1]; c++) {
      out.expected[c] = ok ? expected[c] : 0.0;
      out.ge[c] = ok ? ge[c] : 0;
      out.le[c] = ok ? le[c] : 0;
    }
  }
  return ms;
}

}  // namespace miso

using namespace miso;

// The class table of the event added last: the columns of the assignment matrix as (set of isoforms, start positions).
void miso_batch::fit_add(const Gene *g) {
  fit_tables.resize(events.size());
  FitTable &t = fit_tables.back();
  t = FitTable{};
  if (!g) return;
  if (g->K > 64) { t.status = MISO_FIT_TOO_MANY_CLASSES; return; }   // the matrix's patterns are 64-bit sets
  const std::vector<double> a = assignment_matrix(*g, p.readLength, p.overHang == 0 ? 1 : p.overHang);
  const size_t K = static_cast<size_t>(g->K), nc = K ? a.size() / K : 0;
  t.status = nc > MISO_FIT_MAX_CLASSES ? MISO_FIT_TOO_MANY_CLASSES : MISO_FIT_OK;
  for (size_t c = 0; c < nc; c++) {
    uint64_t pat = 0;
    double m = 0.0;
    for (size_t k = 0; k < K; k++)
      if (a[c * K + k] > 0) { pat |= uint64_t{1} << k; m = a[c * K + k]; }
    t.pattern.push_back(pat);
    t.m.push_back(static_cast<int64_t>(m));
  }
}

// The event's reads by class: its own read classes (pattern, reads) each to the column with its pattern; a non-empty pattern
// that is no column counts in n_off, the empty pattern nowhere.
void miso_batch::fit_counts(int i, std::vector<int32_t> &n, int64_t *n_reads, int64_t *n_off) const {
  const FitTable &t = fit_table(i);
  const PackedEvent &e = events[i];
  n.assign(t.pattern.size(), 0);
  int64_t total = 0, off = 0;
  const size_t K = static_cast<size_t>(e.K), nrc = e.class_counts.size();
  for (size_t r = 0; r < nrc && t.status != MISO_FIT_NO_GENE && K <= 64; r++) {
    uint64_t pat = 0;
    for (size_t k = 0; k < K; k++)
      if (e.class_templates[r * K + k] > 0) pat |= uint64_t{1} << k;
    if (pat == 0) continue;
    const int64_t reads = static_cast<int64_t>(e.class_counts[r]);
    size_t c = 0;
    while (c < t.pattern.size() && t.pattern[c] != pat) c++;
    if (c == t.pattern.size()) { off += reads; continue; }
    n[c] += static_cast<int32_t>(reads);
    total += reads;
  }
  if (n_reads) *n_reads = total;
  if (n_off) *n_off = off;
}

// miso_batch_model_check: the raw call's driver over the resident samples (offsets: the events' own places in the pool)
void miso_batch::model_check(uint64_t seed) {
  if (!model_check_on) MISO_FAIL(MISO_EINVAL, "the model check was not switched on before the events were added (miso_batch_set_model_check)");
  if (!launched) MISO_FAIL(MISO_EINVAL, "batch not launched");
  if (!pending.empty()) MISO_FAIL(MISO_EINVAL, "events still to be matched");
  finish_rounds(*this);
  HIP_OK(hipSetDevice(device));
  const int n = static_cast<int>(events.size());
  FitResults r;
  std::vector<int32_t> K(n), C(n), S(n, this->S()), status_in(n), counts, ni;
  std::vector<uint64_t> pattern, sample_off(n);
  std::vector<int64_t> m;
  std::vector<uint32_t> ids(n);
  r.class_off.assign(1, 0);
  for (int i = 0; i < n; i++) {
    const FitTable &t = fit_table(i);
    K[i] = events[i].K;
    C[i] = static_cast<int32_t>(t.pattern.size());
    status_in[i] = event_unread(i) ? MISO_FIT_NO_GENE : t.status;
    fit_counts(i, ni, nullptr, nullptr);
    pattern.insert(pattern.end(), t.pattern.begin(), t.pattern.end());
    m.insert(m.end(), t.m.begin(), t.m.end());
    counts.insert(counts.end(), ni.begin(), ni.end());
    r.class_off.push_back(static_cast<int64_t>(pattern.size()));
    sample_off[i] = h_events[i].off_samples / 8;
    const bool pinned = i < static_cast<int>(event_ids.size()) && event_ids[i] >= 0;
    ids[i] = pinned ? static_cast<uint32_t>(event_ids[i]) : last_first_event_id + static_cast<uint32_t>(i);
  }
  const size_t nc = std::max<size_t>(pattern.size(), 1);
  r.status.assign(n, 0); r.rows.assign(n, 0); r.bad_rows.assign(n, 0); r.exceed.assign(n, 0);
  r.sum_obs.assign(n, 0.0); r.sum_rep.assign(n, 0.0);
  r.expected.assign(nc, 0.0); r.ge.assign(nc, 0); r.le.assign(nc, 0);
  pattern.resize(nc); m.resize(nc); counts.resize(nc);
  ModelCheckInput in;
  in.n = n; in.K = K.data(); in.C = C.data(); in.class_off = r.class_off.data(); in.pattern = pattern.data(); in.m = m.data();
  in.counts = counts.data(); in.sample_off = sample_off.data(); in.S = S.data(); in.event_id = ids.data();
  in.status_in = status_in.data(); in.d_samples = reinterpret_cast<const double *>(d_out); in.n_sample_doubles = out_bytes / 8;
  in.seed = seed;
  const ModelCheckOutput out{r.status.data(), r.rows.data(), r.bad_rows.data(), r.exceed.data(), r.sum_obs.data(), r.sum_rep.data(),
                             r.expected.data(), r.ge.data(), r.le.data()};
  const float ms = model_check_run(in, out, stream);
  fit = std::move(r);
  model_check_ms = ms;
  model_checked = true;
}
