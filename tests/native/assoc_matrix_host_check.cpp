// The host half of vs_query_assoc_matrix (assoc_matrix_host.hpp) as a stand-alone program, built by tests/test_assoc_matrix_host.py
// with AddressSanitizer + UBSan: the quantiser and the panel writer over shapes at the tile edges, with heap buffers of the exact
// sizes, and the panel checked against the quantiser's integers.  Prints "ok <cells checked>".
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../variantstore_amd/csrc/host/assoc_matrix_host.hpp"

using namespace vsamd;

static int fail(const char* what, size_t n, uint32_t K) {
  std::printf("FAILED: %s (n = %zu, K = %u)\n", what, n, K);
  return 1;
}

int main() {
  std::mt19937_64 rng(7);
  std::normal_distribution<float> normal(0.0f, 3.0f);
  size_t checked = 0;
  const size_t ns[] = {1, 15, 16, 17, 63, 64, 65, 300};
  const uint32_t Ks[] = {1, 15, 16, 17, 33, 100};
  for (size_t n : ns)
    for (uint32_t K : Ks) {
      std::vector<float> y(n * K);
      for (size_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < K; ++k) {
          float v = normal(rng);
          if (k % 5 == 1) v = 0.0f;                                        // a column of zeros
          if (k % 5 == 2) v = std::ldexp((float)((int)(i % 7) - 3), -140);  // denormals
          if (k % 5 == 3) v = (float)((i * 37 + k) % 513) - 256.5f;         // ties at .5 once scaled
          if (k % 5 == 4 && i == 0) v = 3.0e38f;                            // close to the largest float
          y[i * K + k] = v;
        }
      // the columns in reverse: a permutation the panel writer must follow
      std::vector<uint32_t> col_of(n);
      for (size_t i = 0; i < n; ++i) col_of[i] = (uint32_t)(n - 1 - i);
      std::vector<int32_t> q(n * K), shift(K);
      if (!am_quantise(y.data(), n, K, q.data(), shift.data())) return fail("am_quantise refused finite values", n, K);
      AmPanel p;
      if (am_shifts(y.data(), n, K, p.shift) != n * (size_t)K) return fail("am_shifts refused finite values", n, K);
      const uint64_t pitch = (n + 15) & ~(uint64_t)15;
      am_write_panel(y.data(), n, K, col_of.data(), pitch, p);
      if (p.tiles != (K + 15) / 16 || p.words.size() * 8 < p.n_bytes()) return fail("panel size", n, K);
      const int8_t* b = p.bytes();
      for (uint32_t k = 0; k < K; ++k) {
        if (p.shift[k] != shift[k]) return fail("shift", n, K);
        int64_t sy = 0;
        unsigned __int128 syy = 0;
        for (size_t i = 0; i < n; ++i) {
          const int32_t v = q[i * K + k];
          if (v >= (1 << 30) || v <= -(1 << 30)) return fail("|q| >= 2^30", n, K);
          int64_t back = 0;
          for (uint32_t l = kAmLimbs; l-- > 0;)
            back = back * 256 + b[(((size_t)(k / 16) * kAmLimbs + l) * 16 + k % 16) * pitch + col_of[i]];
          if (back != v) return fail("limbs do not give q back", n, K);
          sy += v;
          syy += (unsigned __int128)((int64_t)v * v);
          ++checked;
        }
        if (sy != p.sy[k] || syy != p.syy[k]) return fail("Sy / Syy", n, K);
        for (size_t c = n; c < pitch; ++c)
          for (uint32_t l = 0; l < kAmLimbs; ++l)
            if (b[(((size_t)(k / 16) * kAmLimbs + l) * 16 + k % 16) * pitch + c]) return fail("padding column not zero", n, K);
      }
      for (uint32_t k = K; k < p.tiles * 16; ++k)   // the traits past K
        for (uint32_t l = 0; l < kAmLimbs; ++l)
          for (size_t c = 0; c < pitch; ++c)
            if (b[(((size_t)(k / 16) * kAmLimbs + l) * 16 + k % 16) * pitch + c]) return fail("trait past K not zero", n, K);
      // a value that is not finite is refused and named
      std::vector<float> bad = y;
      bad[n * K - 1] = std::numeric_limits<float>::infinity();
      std::vector<int32_t> sh2;
      if (am_shifts(bad.data(), n, K, sh2) != n * (size_t)K - 1) return fail("non-finite value not found", n, K);
      if (am_quantise(bad.data(), n, K, q.data(), shift.data())) return fail("non-finite value accepted", n, K);
    }
  std::printf("ok %zu\n", checked);
  return 0;
}
