// The read loop's bookkeeping functions (miso_amd/csrc/k2_flag.hpp) compiled for the host: runs them over cases from a
// file of 32-bit words and writes what they return (tests/test_k2_flag_host.py compares it with the numpy restatement).
//   g++ -O2 -std=c++17 -Imiso_amd/csrc tools/k2_flag_host.cpp -o k2_flag_host
//   k2_flag_host flag IN OUT    IN: n, total, start[n + 1], m[total], k[total]     OUT: code[n], pos[n]
//   k2_flag_host part IN OUT    IN: n, rem[n], w[n]                                OUT: k2_part_inv(rem, w)[n]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "k2_flag.hpp"

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

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: k2_flag_host flag|part IN OUT\n"); return 2; }
  std::vector<uint32_t> in, out;
  if (!read_all(argv[2], in) || in.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
  const size_t n = in[0];
  if (std::strcmp(argv[1], "flag") == 0) {
    if (in.size() < 2 || in.size() != 2 + (n + 1) + 2 * static_cast<size_t>(in[1])) { std::fprintf(stderr, "bad flag input\n"); return 1; }
    const size_t total = in[1];
    const uint32_t *start = in.data() + 2, *m = start + n + 1, *k = m + total;
    out.resize(2 * n);
    for (size_t i = 0; i < n; i++) {
      if (start[i] > start[i + 1] || start[i + 1] > total) { std::fprintf(stderr, "bad offsets\n"); return 1; }
      miso::K2Flag f;
      for (uint32_t j = start[i]; j < start[i + 1]; j++) miso::k2_flag_note(f, m[j], k[j]);
      uint32_t pos = 0;
      out[i] = static_cast<uint32_t>(miso::k2_flag_read(f, pos));
      out[n + i] = pos;
    }
  } else if (std::strcmp(argv[1], "part") == 0) {
    if (in.size() != 1 + 2 * n) { std::fprintf(stderr, "bad part input\n"); return 1; }
    const uint32_t *rem = in.data() + 1, *w = rem + n;
    out.resize(n);
    for (size_t i = 0; i < n; i++) out[i] = miso::k2_part_inv(static_cast<int>(rem[i]), static_cast<int>(w[i]));
  } else {
    std::fprintf(stderr, "usage: k2_flag_host flag|part IN OUT\n");
    return 2;
  }
  if (!write_all(argv[3], out)) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
  return 0;
}
