// kernels_negsample.hip -- the sampled online batch's expansion on the device
// (mf_online_update_sampled): the n_in positives, their ids already replaced by factor rows
// (launch_id_lookup), become the N = n_in * (1 + negatives) updates the sweep's plan takes: event j's
// own record, then its negatives s = 0, 1, ... -- the event's user row, a drawn item row
// (neg_sample.hpp) and the negative rating.  One thread per output record: 8 + 4 (or 8) bytes read,
// most of them shared by the 1 + negatives threads of an event, 12 (or 16) bytes written, consecutive
// in each of the three arrays.  HBM-bound: ~100 MB of stores for a 1M-event batch at 5 negatives.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "neg_sample.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = 256;

// pos: user rows [n_in], item rows [n_in], ratings R [n_in]; out: the same three arrays for N records.
// per = 1 + negatives.  skip (may be null): the id lookup's miss count -- non-zero, the rows in pos are
// not final and nothing is written (the host gives the new ids rows and expands again).
template <typename R>
__global__ __launch_bounds__(kThreads) void k_neg_expand(const uint32_t* __restrict__ pos, uint32_t n_in, uint32_t N,
                                                        uint32_t per, uint32_t pool, uint64_t seed,
                                                        uint64_t first_event, R neg_rating,
                                                        uint32_t* __restrict__ out,
                                                        const int32_t* __restrict__ skip) {
  if (skip && *skip != 0) return;
  const uint32_t x = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;
  if (x >= N) return;
  const uint32_t j = x / per, s = x - j * per;
  const uint32_t ur = pos[j], pr = pos[n_in + j];
  uint32_t ir = pr;
  R r = neg_rating;
  if (s == 0) r = reinterpret_cast<const R*>(pos + 2 * static_cast<size_t>(n_in))[j];
  else ir = neg_row(seed, first_event + j, s - 1, pool, pr);
  out[x] = ur;
  out[static_cast<size_t>(N) + x] = ir;
  reinterpret_cast<R*>(out + 2 * static_cast<size_t>(N))[x] = r;
}

}  // namespace

void launch_neg_expand(hipStream_t st, const uint32_t* pos, int64_t n_in, int32_t negatives, uint32_t pool,
                       int64_t seed, int64_t first_event, double neg_rating, bool rf32, uint32_t* out,
                       const int32_t* skip) {
  const int64_t N = n_in * (1 + negatives);
  MF_REQUIRE(n_in > 0 && negatives >= 1 && negatives <= kNegMax && N < (int64_t{1} << 31),
             "negative expansion: bad batch shape");
  // pool < 2 behind the lookup: the model holds no second item yet, and the caller has made sure the
  // batch brings one (online.cpp), so the lookup counts misses and the queued work is void anyway
  MF_REQUIRE(pool >= 2 || skip, "negative expansion: a pool of one row");
  if (pool < 2) return;
  const unsigned grid = static_cast<unsigned>((N + kThreads - 1) / kThreads);
  const uint32_t per = static_cast<uint32_t>(1 + negatives);
  if (rf32)
    hipLaunchKernelGGL(k_neg_expand<float>, dim3(grid), dim3(kThreads), 0, st, pos, static_cast<uint32_t>(n_in),
                       static_cast<uint32_t>(N), per, pool, static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(first_event), static_cast<float>(neg_rating), out, skip);
  else
    hipLaunchKernelGGL(k_neg_expand<double>, dim3(grid), dim3(kThreads), 0, st, pos, static_cast<uint32_t>(n_in),
                       static_cast<uint32_t>(N), per, pool, static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(first_event), neg_rating, out, skip);
  MF_HIP(hipGetLastError());
}

}  // namespace mfhip
