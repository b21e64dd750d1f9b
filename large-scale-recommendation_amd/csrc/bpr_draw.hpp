// bpr_draw.hpp -- the draw and the gradient weight of the BPR trainer (mf_bpr_run, include/mfhip.h): one
// definition for the kernels (kernels_bpr.hip) and mf_bpr_draws (abi.cpp).  mfhip/bpr.py states the same
// rules in Python integers and numpy.  Plain C++: the draw is integer arithmetic only, the weight is IEEE
// double arithmetic with every product rounded before it is added (no fma), so host, device and numpy agree
// bit for bit.
//
// Draw r (0 .. 1 + redraws, redraws <= kBprMaxRedraws) of slot s (< 2^24) of step t (< 2^26) is the SplitMix64
// finaliser neg_draw_bits (neg_sample.hpp) at state seed + gamma * (t * 2^38 + s * 64 + r + 1) mod 2^64: a
// draw depends on (seed, t, s, r) and on nothing the library keeps, not on the batch size and not on any
// other slot.  r = 0 picks the positive, entry bpr_entry(z, pairs) = mulhi64(z, pairs) of the seen set's
// user-major table; r >= 1 pick negatives, neg_pick_row(z, pool, positive row).
//
// bpr_weight(x) = 1 / (1 + E(x)) in f64, E an exponential written out here so that no library's exp is part
// of the contract: x clamped to [-40, 40] (a NaN stays a NaN), n = rint(x * log2 e), r = (x - n * ln2_hi) -
// n * ln2_lo, the degree-13 Taylor polynomial of e^r by Horner's rule with separate multiply and add, and
// ldexp(p, n).  Measured against numpy.exp over 4,000,001 evenly spaced points of [-40, 40] and 10^6 random
// ones: the largest relative difference is 2.22e-16 (2^-52), far below the 2^-40 (9.1e-13) the contract asks for.
#pragma once

#include <cmath>
#include <cstdint>

#include "neg_sample.hpp"

namespace mfhip {

constexpr int kBprMaxRedraws = 62;       // 2 + redraws draws per slot fit the stride of 64
constexpr int kBprSlotBits = 24;         // batch <= 2^24
constexpr int64_t kBprMaxBatch = int64_t{1} << kBprSlotBits;
constexpr int64_t kBprMaxSteps = int64_t{1} << 26;  // t * 2^38 stays below 2^64
constexpr int kBprMaxRank = 256;         // four factors per lane of a wave
constexpr int kBprChunk = 1024;          // entries of a row's segment summed in one chain

MF_NEG_HD inline uint64_t bpr_draw_bits(uint64_t seed, uint64_t t, uint32_t s, uint32_t r) {
  return neg_draw_bits(seed, (t << 32) | s, r);
}

MF_NEG_HD inline uint64_t bpr_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// The entry of the table the positive is: uniform over [0, pairs).
MF_NEG_HD inline uint64_t bpr_entry(uint64_t z, uint64_t pairs) { return bpr_mulhi64(z, pairs); }

// The rank of a negative among the pool - 1 item rows that are not the positive's (what neg_pick_row maps to a
// row); pool >= 2.
MF_NEG_HD inline uint32_t bpr_neg_rank(uint64_t z, uint32_t pool) {
  return static_cast<uint32_t>(((z >> 32) * static_cast<uint64_t>(pool - 1)) >> 32);
}

MF_NEG_HD inline double bpr_exp(double x) {
  if (x != x) return x;
  x = x < -40.0 ? -40.0 : (x > 40.0 ? 40.0 : x);
  const double n = std::rint(x * 1.4426950408889634);
  const double a = n * 6.93147180369123816490e-01;
  const double b = n * 1.90821492927058770002e-10;
  const double r = (x - a) - b;
  constexpr double c[14] = {1.0,
                            1.0,
                            1.0 / 2.0,
                            1.0 / 6.0,
                            1.0 / 24.0,
                            1.0 / 120.0,
                            1.0 / 720.0,
                            1.0 / 5040.0,
                            1.0 / 40320.0,
                            1.0 / 362880.0,
                            1.0 / 3628800.0,
                            1.0 / 39916800.0,
                            1.0 / 479001600.0,
                            1.0 / 6227020800.0};
  double p = c[13];
  for (int i = 12; i >= 0; --i) {
    const double m = p * r;
    p = m + c[i];
  }
  return std::ldexp(p, static_cast<int>(n));
}

MF_NEG_HD inline double bpr_weight(double x) { return 1.0 / (1.0 + bpr_exp(x)); }

}  // namespace mfhip
