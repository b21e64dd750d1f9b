// kernels_als_append.hip -- mf_als_append: one side's packed CSR with a micro-batch appended, on the device.
// The layout after the call is the one mf_als_prepare builds from the concatenated arrays: row x holds its
// old entries in their old order, then the batch's entries of that row in the caller's order.  So
//   an old entry p of row x moves to      p + (new_off[x] - old_off[x]),
//   the batch entry at sorted position s  (row x, the t-th of x's run in the stable sort by row)
//                              lands at   new_off[x] + (old_off[x + 1] - old_off[x]) + t.
// k_als_move takes the old entries by the tile walk of csr_device.hpp: reads are contiguous over the whole
// array, writes are contiguous inside a row.  Every old entry is read once and written once; only the batch
// is sorted (sort_positions, stable by row); its run starts come from the sorted keys, so no atomics are
// needed and the placement does not depend on any order of execution.  Offsets are 64-bit.  Nothing here is
// floating-point arithmetic: ratings move as 4- or 8-byte words.

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "csr_device.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

using dev::kCsrThreads;
using dev::kCsrTile;

template <typename V>
__global__ __launch_bounds__(kCsrThreads) void k_als_move(const int64_t* __restrict__ old_off, int64_t old_rows,
                                                          int64_t old_nnz, const int64_t* __restrict__ new_off,
                                                          const int32_t* __restrict__ old_cols,
                                                          const V* __restrict__ old_vals,
                                                          int32_t* __restrict__ new_cols, V* __restrict__ new_vals) {
  __shared__ int64_t span[2];
  dev::CsrTile T;
  if (!dev::csr_tile(old_off, old_rows, old_nnz, span, T)) return;
  int64_t lo = T.lo;
  for (int64_t e = T.t0 + threadIdx.x; e < T.t1; e += kCsrThreads) {
    lo = dev::row_of(old_off, lo, T.hi, e);  // a lane's entries ascend, so its rows do
    const int64_t d = e + (new_off[lo] - old_off[lo]);
    new_cols[d] = old_cols[e];
    new_vals[d] = old_vals[e];
  }
}

template <typename V>
__global__ void k_als_place(const uint32_t* __restrict__ key, const int32_t* __restrict__ idx, int64_t n,
                            const int64_t* __restrict__ old_off, int64_t old_rows,
                            const int64_t* __restrict__ new_off, const uint32_t* __restrict__ bcol,
                            const V* __restrict__ bval, int32_t* __restrict__ new_cols, V* __restrict__ new_vals) {
  for (int64_t s = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; s < n;
       s += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint32_t x = key[s];
    const int64_t first = dev::lower<uint32_t>(key, 0, s, x);  // the first position of x's run in the sorted keys
    const int64_t had = static_cast<int64_t>(x) < old_rows ? old_off[x + 1] - old_off[x] : 0;
    const int64_t d = new_off[x] + had + (s - first);
    const int32_t j = idx[s];
    new_cols[d] = static_cast<int32_t>(bcol[j]);
    new_vals[d] = bval[j];
  }
}

template <typename V>
void append(const AlsAppendLaunch& L, AlsAppendScratch& sc) {
  if (L.old_nnz > 0)
    hipLaunchKernelGGL(k_als_move<V>, dim3(static_cast<unsigned>((L.old_nnz + kCsrTile - 1) / kCsrTile)),
                       dim3(kCsrThreads), 0, L.st, L.old_off, L.old_rows, L.old_nnz, L.new_off, L.old_cols,
                       static_cast<const V*>(L.old_vals), L.new_cols, static_cast<V*>(L.new_vals));
  if (L.n > 0)
    hipLaunchKernelGGL(k_als_place<V>, dim3(grid_for(L.n)), dim3(kGridThreads), 0, L.st, sc.key.as<uint32_t>(),
                       sc.idx.as<int32_t>(), L.n, L.old_off, L.old_rows, L.new_off, L.bcol,
                       static_cast<const V*>(L.bval), L.new_cols, static_cast<V*>(L.new_vals));
}

}  // namespace

void launch_als_append(const AlsAppendLaunch& L, AlsAppendScratch& sc) {
  MF_REQUIRE(L.n >= 0 && L.n < (int64_t{1} << 31) && L.old_rows >= 0 && L.new_rows >= L.old_rows && L.old_nnz >= 0 &&
                 (L.elem_bytes == 4 || L.elem_bytes == 8),
             "launch_als_append: bad sizes");
  // 2^31 - 1 workgroups of k_als_move at the most: 2^42 entries
  MF_REQUIRE((L.old_nnz + kCsrTile - 1) / kCsrTile < (int64_t{1} << 31), "launch_als_append: the CSR is too long");
  if (L.n > 0) {
    const size_t nb = static_cast<size_t>(L.n) * 4;
    sc.key.alloc(nb);
    sc.idx.alloc(nb);
    sort_positions(L.st, sc.tmp, sc.iota, L.brow, sc.key.as<uint32_t>(), sc.idx.as<int32_t>(), L.n,
                   radix_bits_for(static_cast<uint64_t>(L.new_rows)));
  }
  L.elem_bytes == 8 ? append<uint64_t>(L, sc) : append<uint32_t>(L, sc);
  MF_HIP(hipGetLastError());
}

}  // namespace mfhip
