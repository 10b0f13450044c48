// assoc_matrix_host.hpp -- the host half of vs_query_assoc_matrix: the traits' fixed-point form and the int8 limb panel the kernel
// (k_assoc_matrix.hip.h) multiplies the dosage matrix with.  Plain C++17, no device code: the engine includes it, and so does the
// stand-alone sanitizer check (tests/native/assoc_matrix_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vsamd {

constexpr uint32_t kTraitMatrixMax = 65536;          // VS_TRAIT_MATRIX_MAX
constexpr uint32_t kAmTraitTile = 16;                // traits of a panel tile: the N of one MFMA
constexpr uint32_t kAmLimbs = 4;                     // int8 limbs of a quantised value
constexpr uint32_t kAmTileRows = kAmLimbs * kAmTraitTile;   // panel rows of a tile
constexpr uint64_t kAmMaxCols = 1ull << 22;          // n < 2^22: a limb sum stays below 2^31 and |S| within 2^53

// Per trait column k: M_k = max |y| = m 2^e (0.5 <= m < 1), f_k = 30 - e (0 for a column of zeros), q = rint(y 2^f_k), ties to
// even: |q| < 2^30.  y 2^f is formed in double by a multiplication with the power of two, which is exact (a float32 times 2^f
// neither overflows nor underflows for f in -98 .. 179).
inline int32_t am_shift(float max_abs) {
  if (max_abs == 0.0f) return 0;
  int e = 0;
  (void)std::frexp((double)max_abs, &e);
  return 30 - e;
}
inline int32_t am_quantise_value(float y, double scale) { return (int32_t)std::nearbyint((double)y * scale); }

// The four balanced base-256 digits of q, low to high: q = b0 + 256 b1 + 65536 b2 + 2^24 b3, every b in [-128, 127].
inline void am_limbs(int32_t q, int8_t (&b)[kAmLimbs]) {
  for (uint32_t l = 0; l < kAmLimbs; ++l) {
    const int32_t d = ((q + 128) & 255) - 128;
    b[l] = (int8_t)d;
    q = (q - d) >> 8;   // (q - d is a multiple of 256: the shift is exact)
  }
}

// The shifts of the K columns of y (n x K, row-major).  Returns the index of the first value that is not finite, or n * K.
inline size_t am_shifts(const float* y, size_t n, uint32_t K, std::vector<int32_t>& shift) {
  std::vector<uint32_t> max_bits(K, 0);
  for (size_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < K; ++k) {
      uint32_t b;
      std::memcpy(&b, y + i * K + k, 4);
      b &= 0x7FFFFFFFu;
      if (b >= 0x7F800000u) return i * K + k;
      if (b > max_bits[k]) max_bits[k] = b;   // (the patterns of non-negative floats order as the values do)
    }
  shift.resize(K);
  for (uint32_t k = 0; k < K; ++k) {
    float m;
    std::memcpy(&m, &max_bits[k], 4);
    shift[k] = am_shift(m);
  }
  return n * (size_t)K;
}

struct AmPanel {
  std::vector<int32_t> shift;          // f_k
  std::vector<int64_t> sy;             // sum of q
  std::vector<unsigned __int128> syy;  // sum of q^2
  std::vector<double> vy;              // (double)(n Syy - Sy^2), converted once
  uint32_t tiles = 0;                  // ceil(K / 16)
  uint64_t pitch = 0;
  // [trait tile][limb][trait within the tile][pitch] int8; padding columns and the traits past K are zero
  std::vector<uint64_t> words;         // (8-byte words: the upload is 16-byte aligned at every tile)
  int8_t* bytes() { return reinterpret_cast<int8_t*>(words.data()); }
  const int8_t* bytes() const { return reinterpret_cast<const int8_t*>(words.data()); }
  size_t n_bytes() const { return (size_t)tiles * kAmTileRows * pitch; }
};

// The panel of y (n x K, row-major, finite: am_shifts has passed it): row i of y belongs to column col_of[i] (NULL: column i) of
// n_cols = n distinct columns, pitch >= n bytes apart.  A tile of 16 traits at a time: one cache line of y per sample and tile,
// written into the tile's 64 panel rows.
inline void am_write_panel(const float* y, size_t n, uint32_t K, const uint32_t* col_of, uint64_t pitch, AmPanel& p) {
  p.tiles = (K + kAmTraitTile - 1) / kAmTraitTile;
  p.pitch = pitch;
  p.sy.assign(K, 0);
  p.syy.assign(K, 0);
  p.vy.assign(K, 0.0);
  p.words.assign((p.n_bytes() + 7) / 8, 0);
  std::vector<double> scale(K);
  for (uint32_t k = 0; k < K; ++k) scale[k] = std::ldexp(1.0, p.shift[k]);
  int8_t* const out = p.bytes();
  for (uint32_t t = 0; t < p.tiles; ++t) {
    const uint32_t k0 = t * kAmTraitTile, kn = K - k0 < kAmTraitTile ? K - k0 : kAmTraitTile;
    int8_t* const tile = out + (size_t)t * kAmTileRows * pitch;
    for (size_t i = 0; i < n; ++i) {
      const size_t col = col_of ? col_of[i] : i;
      const float* row = y + i * K + k0;
      for (uint32_t j = 0; j < kn; ++j) {
        const int32_t q = am_quantise_value(row[j], scale[k0 + j]);
        p.sy[k0 + j] += q;
        p.syy[k0 + j] += (unsigned __int128)((int64_t)q * q);
        int8_t b[kAmLimbs];
        am_limbs(q, b);
        for (uint32_t l = 0; l < kAmLimbs; ++l) tile[((size_t)l * kAmTraitTile + j) * pitch + col] = b[l];
      }
    }
  }
  for (uint32_t k = 0; k < K; ++k) {
    const __int128 v = (__int128)((unsigned __int128)n * p.syy[k]) - (__int128)p.sy[k] * p.sy[k];
    p.vy[k] = (double)v;
  }
}

// q (n x K int32, row-major) and the K shifts of y.  Returns false on a value that is not finite.
inline bool am_quantise(const float* y, size_t n, uint32_t K, int32_t* q_out, int32_t* shift_out) {
  std::vector<int32_t> shift;
  if (am_shifts(y, n, K, shift) != n * (size_t)K) return false;
  std::vector<double> scale(K);
  for (uint32_t k = 0; k < K; ++k) { scale[k] = std::ldexp(1.0, shift[k]); shift_out[k] = shift[k]; }
  for (size_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < K; ++k) q_out[i * K + k] = am_quantise_value(y[i * K + k], scale[k]);
  return true;
}

}  // namespace vsamd
