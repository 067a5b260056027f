// The read loop's per-word arithmetic and finishing expression (miso_amd/csrc/k2_count.hpp) compiled for the host: runs them
// over cases from a file of 32-bit words and writes what they return (tests/test_k2_count_host.py compares it with the numpy
// restatement of the definition; tests/test_gpu_k2_count.py compares the device's assembly statements with it).
//   g++ -O2 -std=c++17 -Imiso_amd/csrc tools/k2_count_host.cpp -o k2_count_host
//   k2_count_host word IN OUT     IN: n, th[n], u[n]                                   OUT: k2_count_word(k2_count_p(th), u)[n]
//   k2_count_host seq IN OUT      IN: n, total, start[n + 1], th[n], u[total], inv[total]
//                                 OUT: acc[n], o[n] of k2_count_step over words start[i] .. start[i + 1] - 1, from acc = o = 0
//   k2_count_host finish IN OUT   IN: n, A[n], E[n], more[n]                           OUT: k2_count_finish[n]
//   k2_count_host top IN OUT      IN: n, A[n], flagged[n], N[n]                        OUT: k2_count_top_clean[n]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "k2_count.hpp"

static bool read_all(const char *path, std::vector<uint32_t> &v) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize(static_cast<size_t>(bytes) / 4);
  const bool ok = std::fread(v.data(), 4, v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

static bool write_all(const char *path, const std::vector<uint32_t> &v) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), 4, v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok;
}

static int usage() { std::fprintf(stderr, "usage: k2_count_host word|seq|finish|top IN OUT\n"); return 2; }

int main(int argc, char **argv) {
  if (argc != 4) return usage();
  std::vector<uint32_t> in, out;
  if (!read_all(argv[2], in) || in.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
  const size_t n = in[0];
  if (std::strcmp(argv[1], "word") == 0) {
    if (in.size() != 1 + 2 * n) { std::fprintf(stderr, "bad word input\n"); return 1; }
    const uint32_t *th = in.data() + 1, *u = th + n;
    out.resize(n);
    for (size_t i = 0; i < n; i++) out[i] = miso::k2_count_word(miso::k2_count_p(th[i]), u[i]);
  } else if (std::strcmp(argv[1], "seq") == 0) {
    if (in.size() < 2 || in.size() != 2 + (n + 1) + n + 2 * static_cast<size_t>(in[1])) { std::fprintf(stderr, "bad seq input\n"); return 1; }
    const size_t total = in[1];
    const uint32_t *start = in.data() + 2, *th = start + n + 1, *u = th + n, *inv = u + total;
    out.resize(2 * n);
    for (size_t i = 0; i < n; i++) {
      if (start[i] > start[i + 1] || start[i + 1] > total) { std::fprintf(stderr, "bad offsets\n"); return 1; }
      const uint32_t P = miso::k2_count_p(th[i]);
      uint32_t acc = 0, o = 0;
      for (uint32_t j = start[i]; j < start[i + 1]; j++) miso::k2_count_step(acc, o, P, u[j], inv[j]);
      out[i] = acc;
      out[n + i] = o;
    }
  } else if (std::strcmp(argv[1], "finish") == 0) {
    if (in.size() != 1 + 3 * n) { std::fprintf(stderr, "bad finish input\n"); return 1; }
    const uint32_t *A = in.data() + 1, *E = A + n, *more = E + n;
    out.resize(n);
    for (size_t i = 0; i < n; i++)
      out[i] = static_cast<uint32_t>(miso::k2_count_finish(static_cast<int>(A[i]), static_cast<int>(E[i]), static_cast<int>(more[i])));
  } else if (std::strcmp(argv[1], "top") == 0) {
    if (in.size() != 1 + 3 * n) { std::fprintf(stderr, "bad top input\n"); return 1; }
    const uint32_t *A = in.data() + 1, *fl = A + n, *N = fl + n;
    out.resize(n);
    for (size_t i = 0; i < n; i++) out[i] = miso::k2_count_top_clean(static_cast<int>(A[i]), fl[i], static_cast<int>(N[i])) ? 1u : 0u;
  } else {
    return usage();
  }
  if (!write_all(argv[3], out)) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
  return 0;
}
