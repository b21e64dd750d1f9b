// neg_sample.hpp -- the negative draw of mf_online_update_sampled (include/mfhip.h): one definition
// for the device expansion (kernels_negsample.hip), the host expansions (online.cpp) and
// mf_negative_draws (abi.cpp).  Plain C++: integer arithmetic only, the same bits on host and device.
//
// Negative s (0 .. negatives-1, negatives <= kNegMax) of stream event t is drawn from a SplitMix64
// stream indexed by the pair -- state seed + gamma * (t * 64 + s + 1), all mod 2^64 -- so a draw
// depends on (seed, t, s) and on nothing the library keeps.  The top 32 bits pick one of the
// pool - 1 rows that are not the positive's own (multiply-shift, no rejection loop).
#pragma once

#include <cstdint>

#ifdef __HIP__
#define MF_NEG_HD __host__ __device__
#else
#define MF_NEG_HD
#endif

namespace mfhip {

constexpr int kNegMax = 64;  // MF_NEG_MAX: the stride of t in the stream index

MF_NEG_HD inline uint64_t neg_draw_bits(uint64_t seed, uint64_t t, uint32_t s) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ULL * (t * static_cast<uint64_t>(kNegMax) + s + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// A row of [0, pool) other than pos_row; pool >= 2, pos_row < pool.
MF_NEG_HD inline uint32_t neg_pick_row(uint64_t z, uint32_t pool, uint32_t pos_row) {
  const uint32_t c = static_cast<uint32_t>(((z >> 32) * static_cast<uint64_t>(pool - 1)) >> 32);
  return c + (c >= pos_row ? 1u : 0u);
}

MF_NEG_HD inline uint32_t neg_row(uint64_t seed, uint64_t t, uint32_t s, uint32_t pool, uint32_t pos_row) {
  return neg_pick_row(neg_draw_bits(seed, t, s), pool, pos_row);
}

}  // namespace mfhip
