// csr_device.hpp -- the tile walk of the table kernels (k_als_move, k_seen_csr_keys, k_seen_move,
// k_remove_scan, k_fold_compact): a kernel that must touch every entry of a packed CSR and know each entry's row.
//
// Such a kernel walks the ENTRIES, not the rows.  A workgroup of kCsrThreads threads takes kCsrTile
// consecutive entries [t0, t1), whatever rows they belong to.  Threads 0 and 1 find the rows of the tile's
// first and last entry (two searches of off[] per workgroup); every lane then narrows the row of its own
// entry inside that span [lo, hi] only -- no step at all where the tile lies inside one row, which is every
// tile but two of a 200k-entry row.  A lane's entries ascend, so it carries its row forward as the lower end
// of its next search.  Reads are contiguous over the whole array; a long row is handled by as many
// workgroups as it has tiles, never by one lane, and rows without entries cost nothing (row_of,
// csr_search.hpp).  The grid is ceil(nnz / kCsrTile) workgroups, below 2^31: at most 2^42 entries.
#pragma once

#include <hip/hip_runtime.h>

#include "csr_search.hpp"

namespace mfhip::dev {

constexpr int kCsrThreads = 256;
constexpr int kCsrTile = kCsrThreads * 8;  // 2048 entries per workgroup
static_assert(kCsrTile == 2048, "the removal tests plant entries around multiples of 2048");

struct CsrTile {
  int64_t t0, t1;  // the workgroup's entries
  int64_t lo, hi;  // the rows of entries t0 and t1 - 1
};

// The prologue of a tiled kernel; every thread of the workgroup calls it, with a two-slot __shared__ span.
// False: the tile holds no entry (the grid has no such workgroup) and nothing was written or waited for.
// True: span[0 .. 1] hold T.lo and T.hi for further searches by threads 0 and 1 (k_remove_scan, k_seen_move).
__device__ __forceinline__ bool csr_tile(const int64_t* __restrict__ off, int64_t rows, int64_t nnz, int64_t* span,
                                         CsrTile& T) {
  T.t0 = blockIdx.x * static_cast<int64_t>(kCsrTile);
  T.t1 = T.t0 + kCsrTile < nnz ? T.t0 + kCsrTile : nnz;
  if (T.t0 >= T.t1) return false;
  if (threadIdx.x < 2) span[threadIdx.x] = row_of(off, 0, rows - 1, threadIdx.x == 0 ? T.t0 : T.t1 - 1);
  __syncthreads();
  T.lo = span[0];
  T.hi = span[1];
  return true;
}

}  // namespace mfhip::dev
