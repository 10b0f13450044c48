// k_int128.hip.h -- the one conversion of a 128-bit integer to a double that k_gram_finish (the GRM cells) and k_assoc_matrix (the
// covariance of a CHI2 cell) share.  Part of kernels.hip.h (the kernel index is there).
#pragma once
#include <hip/hip_runtime.h>

namespace vsamd {

// A 128-bit integer as the nearest double (ties to even): the magnitude's top 64 bits with a sticky bit for what is shifted out
// -- 11 bits of room below the 53 a double keeps, so the hardware's rounding of the 64-bit value is the rounding of the whole --,
// scaled back exactly.
__device__ __forceinline__ double gram_to_double(__int128 x) {
  const bool neg = x < 0;
  const unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)x : (unsigned __int128)x;
  const unsigned long long hi = (unsigned long long)(m >> 64), lo = (unsigned long long)m;
  double d;
  if (hi == 0) d = (double)lo;
  else {
    const int sh = 64 - __clzll((long long)hi);   // 1 .. 64: the bits above the low word
    const unsigned long long top = (unsigned long long)(m >> sh);
    const unsigned long long lost = sh == 64 ? lo : lo & ((1ull << sh) - 1ull);
    d = ldexp((double)(top | (lost != 0 ? 1ull : 0ull)), sh);
  }
  return neg ? -d : d;
}

}  // namespace vsamd
