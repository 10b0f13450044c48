// The digit split of vs_query_score_matrix (score_matrix_host.hpp) as a stand-alone program, built by tests/test_score_matrix_host.py
// plainly and with AddressSanitizer + UBSan: every row total splits into four balanced base-256 digits, or into five where it must,
// the digits lie in [-128, 127] and give the value back, and the shift of a weight column is the trait quantiser's
// (assoc_matrix_host.hpp).  Prints "ok <values checked>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../variantstore_amd/csrc/host/assoc_matrix_host.hpp"
#include "../../variantstore_amd/csrc/host/score_matrix_host.hpp"

using namespace vsamd;

static int fail(const char* what, long long v) {
  std::printf("FAILED: %s (value %lld)\n", what, v);
  return 1;
}

// 0: fine.  The digits of t; the engine runs four limbs exactly when |t| <= kSmMax4.
static int check(int64_t t) {
  int8_t b[kSmLimbsMax];
  const int64_t rest = sm_limbs(t, b);
  const uint64_t mag = t < 0 ? 0ull - (uint64_t)t : (uint64_t)t;
  if (mag <= (uint64_t)kSmMax5 && rest != 0) return fail("something is left behind the fifth digit", t);
  int64_t back = 0;
  for (uint32_t l = kSmLimbsMax; l-- > 0;) {
    if (b[l] < -128 || b[l] > 127) return fail("digit out of range", t);
    back = back * 256 + b[l];
  }
  if (mag <= (uint64_t)kSmMax5 && back != t) return fail("the digits do not give the value back", t);
  const uint32_t need = sm_limbs_needed(mag);
  if (need != (mag <= 2139062143ull ? 4u : 5u)) return fail("sm_limbs_needed", t);
  if (need == 4 && b[4] != 0) return fail("a fifth digit where four suffice", t);
  // (the digits are balanced, not symmetric: four reach down to -128 (256^4 - 1) / 255 = -2,155,905,152; the engine decides by |T|
  //  and runs five limbs for the few negative totals below -kSmMax4 that four would hold, with a fifth digit of zero)
  const bool four_hold = t <= kSmMax4 && t >= -2155905152ll;
  if (mag <= (uint64_t)kSmMax5 && (b[4] == 0) != four_hold) return fail("the fifth digit is zero exactly where four digits hold the value", t);
  if (need == 4) {   // the four digits alone
    int64_t back4 = 0;
    for (uint32_t l = 4; l-- > 0;) back4 = back4 * 256 + b[l];
    if (back4 != t) return fail("four digits do not give the value back", t);
  }
  return 0;
}

int main() {
  static_assert(kSmMax4 == 127ll * (256ll * 256 * 256 * 256 - 1) / 255, "four digits");
  static_assert(kSmMax5 == 127ll * (256ll * 256 * 256 * 256 * 256 - 1) / 255, "five digits");
  static_assert(kSmMaxTotal <= kSmMax5, "the refusal bound fits five digits");
  size_t checked = 0;
  const int64_t chosen[] = {0, 1, 127, 128, 129, 255, 256, 32767, 32768, 8355711, 8421504, 2139062143ll, 2139062144ll, 1ll << 32, (1ll << 38) - 1, 1ll << 38,
                            547599908735ll};
  for (int64_t v : chosen)
    for (int64_t s : {v, -v}) {
      if (check(s)) return 1;
      ++checked;
    }
  std::mt19937_64 rng(19);
  for (int i = 0; i < 1000000; ++i) {
    // a third below the four-digit bound, a third around it, a third anywhere up to the five-digit bound
    const uint64_t r = rng();
    int64_t v;
    if (i % 3 == 0) v = (int64_t)(r % (2ull * kSmMax4 + 1)) - kSmMax4;
    else if (i % 3 == 1) v = (int64_t)(r % 2048) - 1024 + ((r >> 20) & 1 ? kSmMax4 : -kSmMax4);
    else v = (int64_t)(r % (2ull * kSmMax5 + 1)) - kSmMax5;
    if (check(v)) return 1;
    ++checked;
  }
  // the shift of a weight column is the trait quantiser's: am_shifts (what the query calls) against am_quantise (what
  // vs_assoc_matrix_quantise calls) on the same column, and |q| < 2^30
  std::normal_distribution<float> normal(0.0f, 2.0f);
  for (uint32_t K : {1u, 15u, 16u, 17u, 33u}) {
    const size_t n = 200;
    std::vector<float> w(n * K);
    for (size_t i = 0; i < n; ++i)
      for (uint32_t k = 0; k < K; ++k) w[i * K + k] = k % 4 == 1 ? 0.0f : k % 4 == 2 ? std::ldexp(normal(rng), -60) : k % 4 == 3 ? 1.0e6f * normal(rng) : normal(rng);
    std::vector<int32_t> shift, q(n * K), shift2(K);
    if (am_shifts(w.data(), n, K, shift) != n * (size_t)K) return fail("am_shifts refused finite values", K);
    if (!am_quantise(w.data(), n, K, q.data(), shift2.data())) return fail("am_quantise refused finite values", K);
    for (uint32_t k = 0; k < K; ++k) {
      if (shift[k] != shift2[k]) return fail("the shifts differ", k);
      if (k % 4 == 1 && shift[k] != 0) return fail("a column of zeros has a shift", k);
      for (size_t i = 0; i < n; ++i) {
        const int32_t v = q[i * K + k];
        if (v >= (1 << 30) || v <= -(1 << 30)) return fail("|q| >= 2^30", v);
        if (v != am_quantise_value(w[i * K + k], std::ldexp(1.0, shift[k]))) return fail("q differs", v);
        if (check(v)) return 1;
        ++checked;
      }
    }
  }
  std::printf("ok %zu\n", checked);
  return 0;
}
