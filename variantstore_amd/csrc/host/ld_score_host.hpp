// ld_score_host.hpp -- the one quotient of an LD-score query (vs_query_ld_scores): floor(cov^2 2^32 / (v_a v_b)) in exact integers.
// Host and device share this source: k_ld_score (k_ld_score.hip.h) forms every summed value with it, and
// tests/native/ld_score_host_check.cpp compiles it with g++ and holds it against a plain unsigned __int128 division.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VS_LDS_HD __host__ __device__
#else
#define VS_LDS_HD
#endif

namespace vsamd {

constexpr uint64_t kLdScoreOne = 1ull << 32;   // the value of r^2 = 1

// q32 = floor(mag^2 2^32 / (va vb)) for mag = |cov| < 2^44 and 0 < va, vb < 2^44 with mag^2 <= va vb (Cauchy-Schwarz), so that
// q32 lies in 0 .. 2^32.  Device code has no 128-bit division: the quotient is estimated in doubles -- four conversions and three
// operations, each within 2^-53 relative, on a value of at most 2^32: the estimate is within 2^-18 of the true quotient and its
// floor within one unit of the answer -- and then corrected with 128-bit products and comparisons until
// e den <= num 2^32 < (e + 1) den.  Two bounded steps either way, no open loop.  num 2^32 < 2^120, (e + 1) den < 2^122.
VS_LDS_HD inline uint64_t ld_score_q32(uint64_t mag, uint64_t va, uint64_t vb) {
  const unsigned __int128 num = ((unsigned __int128)mag * mag) << 32;
  const unsigned __int128 den = (unsigned __int128)va * vb;
  double est = (double)mag * (double)mag / ((double)va * (double)vb) * 4294967296.0;
  if (!(est >= 0.0)) est = 0.0;
  if (est > 4294967296.0) est = 4294967296.0;
  uint64_t e = (uint64_t)est;
  unsigned __int128 p = (unsigned __int128)e * den;
#if defined(__clang__)
#pragma unroll
#endif
  for (int step = 0; step < 2; ++step) {
    if (p > num) { --e; p -= den; }                 // (e >= 1 here: p > num >= 0)
    else if (num - p >= den) { ++e; p += den; }
  }
  return e;
}

}  // namespace vsamd
