// score_matrix_host.hpp -- what the host and the device share of vs_query_score_matrix: the bounds of a row total T (the sum of a
// weight column's fixed-point values over the reports of one table row) and its split into balanced base-256 digits, the int8
// "limbs" k_score_matrix (k_score_matrix.hip.h) multiplies the dosage matrix with.  Plain C++17 with the digit split marked
// __host__ __device__ under hipcc: the engine includes it, and so does the stand-alone check
// (tests/native/score_matrix_host_check.cpp).  The quantiser itself is assoc_matrix_host.hpp's (am_shifts, am_quantise_value).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VS_SM_HD __host__ __device__
#else
#define VS_SM_HD
#endif

namespace vsamd {

constexpr uint32_t kScoreMatrixMax = 65536;                      // VS_SCORE_MATRIX_MAX
constexpr uint32_t kSmScoreTile = 16;                            // scores of a panel tile: the N of one MFMA
constexpr uint32_t kSmLimbsMax = 5;                              // the panel is laid out for five limbs; the kernel reads four where they suffice
constexpr int64_t kSmMax4 = 2139062143ll;                        // 127 (256^4 - 1) / 255: the largest |T| four digits hold
constexpr int64_t kSmMax5 = 547599908735ll;                      // 127 (256^5 - 1) / 255: ... five digits
constexpr int64_t kSmMaxTotal = 1ll << 38;                       // the largest |T| a batch may hold (more than 256 reports of one row at |q| < 2^30 pass it)
constexpr uint64_t kSmMaxReports = 1ull << 26;                   // N < 2^26: |sum| <= 2 x 2^30 x N < 2^57

// The limbs a batch whose largest |T| is max_abs needs: 4 or 5 (max_abs <= kSmMaxTotal).
VS_SM_HD inline uint32_t sm_limbs_needed(uint64_t max_abs) { return max_abs <= (uint64_t)kSmMax4 ? 4u : 5u; }

// The five balanced base-256 digits of t, low to high: t = b0 + 2^8 b1 + 2^16 b2 + 2^24 b3 + 2^32 b4, every b in [-128, 127], for
// |t| <= kSmMax5; b4 is 0 for |t| <= kSmMax4.  Returns what is left of t behind the fifth digit: 0 within the bounds.
VS_SM_HD inline int64_t sm_limbs(int64_t t, int8_t (&b)[kSmLimbsMax]) {
  for (uint32_t l = 0; l < kSmLimbsMax; ++l) {
    const int64_t d = ((t + 128) & 255) - 128;
    b[l] = (int8_t)d;
    t = (t - d) >> 8;   // (t - d is a multiple of 256: the shift is exact)
  }
  return t;
}

}  // namespace vsamd
