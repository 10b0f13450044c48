// Stand-alone check of the LD-score quotient (variantstore_amd/csrc/host/ld_score_host.hpp), the source the device compiles too:
// ld_score_q32 against a plain unsigned __int128 division.  Built by tests/test_ld_scores_host.py with g++, once plainly and once
// under -fsanitize=address,undefined.  Prints "ok <cases>" and returns 0, or the first mismatch and 1.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../variantstore_amd/csrc/host/ld_score_host.hpp"

typedef unsigned __int128 u128;

static unsigned long long g_cases = 0;

// floor(mag^2 2^32 / (va vb)) by division; the operands as the engine admits them: mag^2 <= va vb < 2^88
static bool check(uint64_t mag, uint64_t va, uint64_t vb, const char* what) {
  const u128 num = ((u128)mag * mag) << 32, den = (u128)va * vb;
  if (den == 0 || (u128)mag * mag > den) { std::printf("bad case (%s): mag %llu va %llu vb %llu\n", what, (unsigned long long)mag, (unsigned long long)va, (unsigned long long)vb); return false; }
  const uint64_t want = (uint64_t)(num / den), got = vsamd::ld_score_q32(mag, va, vb);
  ++g_cases;
  if (got == want) return true;
  std::printf("MISMATCH (%s): mag %llu va %llu vb %llu: got %llu want %llu\n", what, (unsigned long long)mag, (unsigned long long)va, (unsigned long long)vb,
              (unsigned long long)got, (unsigned long long)want);
  return false;
}

static uint64_t isqrt128(u128 x) {   // floor(sqrt(x)), x < 2^88
  uint64_t lo = 0, hi = 1ull << 44;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if ((u128)mid * mid <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

int main() {
  std::mt19937_64 rng(20261020);
  const uint64_t top = (1ull << 44) - 1;   // v and |cov| stay below 2^44 for n < 2^21
  bool ok = true;
  // random operands of every size up to the bounds
  for (int i = 0; i < 400000 && ok; ++i) {
    const int ba = 1 + (int)(rng() % 44), bb = 1 + (int)(rng() % 44);
    const uint64_t va = 1 + rng() % ((1ull << ba) - 1 ? (1ull << ba) - 1 : 1), vb = 1 + rng() % ((1ull << bb) - 1 ? (1ull << bb) - 1 : 1);
    const uint64_t cap = isqrt128((u128)va * vb);
    const uint64_t mag = rng() % (cap + 1);
    ok = ok && check(mag, va, vb, "random");
    ok = ok && check(cap, va, vb, "largest cov");
  }
  // cov^2 = va vb: exactly 2^32
  for (int i = 0; i < 100000 && ok; ++i) {
    const uint64_t v = 1 + rng() % top;
    ok = ok && check(v, v, v, "a = b");
    if (vsamd::ld_score_q32(v, v, v) != vsamd::kLdScoreOne) { std::printf("a = b is not 2^32 at v = %llu\n", (unsigned long long)v); ok = false; }
    const uint64_t s = 1 + rng() % ((1ull << 22) - 1), t = 1 + rng() % ((1ull << 22) - 1);   // va = s^2, vb = t^2, cov = s t
    ok = ok && check(s * t, s * s, t * t, "perfect");
    if (vsamd::ld_score_q32(s * t, s * s, t * t) != vsamd::kLdScoreOne) { std::printf("perfect pair is not 2^32\n"); ok = false; }
  }
  // cov = 0
  for (int i = 0; i < 1000 && ok; ++i) {
    const uint64_t va = 1 + rng() % top, vb = 1 + rng() % top;
    ok = ok && check(0, va, vb, "cov = 0");
    if (vsamd::ld_score_q32(0, va, vb) != 0) { std::printf("cov = 0 is not 0\n"); ok = false; }
  }
  // numerators that are exact multiples of the denominator, and those +- 1: mag^2 2^32 = k den with den = d^2 and mag = d j / 2^16,
  // i. e. d a multiple of 2^16 and k = j^2; mag +- 1 moves the numerator to either side of a multiple
  for (int i = 0; i < 200000 && ok; ++i) {
    const uint64_t d = ((1 + rng() % ((1ull << 27) - 1)) << 16);          // < 2^43, a multiple of 2^16
    const uint64_t j = rng() % ((1ull << 16) + 1);                          // 0 .. 2^16: mag = (d >> 16) j <= d
    const uint64_t mag = (d >> 16) * j;
    ok = ok && check(mag, d, d, "multiple");
    if (vsamd::ld_score_q32(mag, d, d) != j * j) { std::printf("multiple: not exact\n"); ok = false; }
    if (mag > 0) ok = ok && check(mag - 1, d, d, "multiple - 1");
    if (mag < d) ok = ok && check(mag + 1, d, d, "multiple + 1");
    // the same around an odd split of the denominator
    const uint64_t f = 1 + rng() % 65535;
    if (d % f == 0 && d * f <= top) ok = ok && check(mag, d / f, d * f, "multiple, split");
  }
  // numerators one below, at and one above a multiple of an arbitrary denominator: the nearest mag to sqrt(k den / 2^32)
  for (int i = 0; i < 200000 && ok; ++i) {
    const uint64_t va = 1 + rng() % top, vb = 1 + rng() % top;
    const u128 den = (u128)va * vb;
    const uint64_t k = rng() % ((1ull << 32) + 1);
    const uint64_t mag = isqrt128((den >> 32) * k + (((den & 0xFFFFFFFFull) * k) >> 32));
    for (uint64_t m = mag > 1 ? mag - 1 : 0; m <= mag + 1 && ok; ++m)
      if ((u128)m * m <= den) ok = ok && check(m, va, vb, "near a multiple");
  }
  // denominators at 2^88 - small
  for (int i = 0; i < 100000 && ok; ++i) {
    const uint64_t va = top - rng() % 64, vb = top - rng() % 64;
    const uint64_t cap = isqrt128((u128)va * vb);
    ok = ok && check(cap - rng() % 64, va, vb, "largest denominator, largest cov");
    ok = ok && check(rng() % (cap + 1), va, vb, "largest denominator");
    ok = ok && check(rng() % 4096, va, vb, "largest denominator, small cov");
  }
  if (!ok) return 1;
  std::printf("ok %llu\n", g_cases);
  return 0;
}
