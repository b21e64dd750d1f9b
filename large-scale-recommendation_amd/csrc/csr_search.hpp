// csr_search.hpp -- the binary searches of the table kernels (the files that build, merge, search or compact
// a packed CSR on the device), one definition each, for the host and the device.  No HIP include: under
// hipcc the functions are __host__ __device__, under a plain C++ compiler they are ordinary inline functions
// (tests/csr_search_check.cpp runs them on the CPU against the standard library).
//
// Positions are int64_t and stay far below 2^62 (a CSR holds at most 2^42 entries), so the midpoint of
// [b, e) is (b + e) >> 1 everywhere: the sum cannot overflow, and every search agrees on the element it
// looks at first.  row_of alone needs the upper-biased midpoint; it says why.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MFHIP_HD __host__ __device__
#else
#define MFHIP_HD
#endif

namespace mfhip::dev {

// The row of entry e in the offsets off[]: the largest x in [lo, hi] with off[x] <= e, given
// off[lo] <= e < off[hi + 1].  Rows without entries share their offset with the next row: when rows
// x .. x + m all begin at off[x] and only row x + m has entries, every one of them has off[.] <= e, and the
// largest is the row that holds e.  The search keeps off[lo] <= e true and takes `hi` down past the rows
// that begin after e.  The midpoint is biased upwards (mid > lo whenever lo < hi) because the step
// `lo = mid` must make progress.
MFHIP_HD inline int64_t row_of(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The first position of [b, e) that holds a value >= x (e when there is none); the values ascend.
template <typename K>
MFHIP_HD inline int64_t lower(const K* __restrict__ a, int64_t b, int64_t e, K x) {
  while (b < e) {
    const int64_t m = (b + e) >> 1;
    if (a[m] < x) b = m + 1;
    else e = m;
  }
  return b;
}

// ... a value > x
template <typename K>
MFHIP_HD inline int64_t upper(const K* __restrict__ a, int64_t b, int64_t e, K x) {
  while (b < e) {
    const int64_t m = (b + e) >> 1;
    if (a[m] <= x) b = m + 1;
    else e = m;
  }
  return b;
}

// Is x among the ascending values of [b, e)?  Leaves at the first hit.
template <typename K>
MFHIP_HD inline bool contains(const K* __restrict__ a, int64_t b, int64_t e, K x) {
  while (b < e) {
    const int64_t m = (b + e) >> 1;
    const K v = a[m];
    if (v == x) return true;
    if (v < x) b = m + 1;
    else e = m;
  }
  return false;
}

}  // namespace mfhip::dev
