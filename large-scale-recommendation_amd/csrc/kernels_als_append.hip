// kernels_als_append.hip -- mf_als_append: one side's packed CSR with a micro-batch appended, on the device.
// The layout after the call is the one mf_als_prepare builds from the concatenated arrays: row x holds its
// old entries in their old order, then the batch's entries of that row in the caller's order.  So
//   an old entry p of row x moves to      p + (new_off[x] - old_off[x]),
//   the batch entry at sorted position s  (row x, the t-th of x's run in the stable sort by row)
//                              lands at   new_off[x] + (old_off[x + 1] - old_off[x]) + t.
// k_als_move walks the OLD ENTRIES, not the rows: a workgroup takes 2048 consecutive entries, finds the
// rows its first and last entry belong to (two searches of old_off per workgroup), and every lane then
// narrows its entry's row inside that span only -- no step at all where the tile lies inside one row, which
// is every tile but two of a 200k-entry item row.  Reads are contiguous over the whole array, writes are
// contiguous inside a row: a long row is copied by as many workgroups as it has tiles, never by one lane.
// Every old entry is read once and written once; only the batch is sorted (rocprim's stable radix sort by
// row, as the online plan sorts); its run starts come from the sorted keys, so no atomics are needed and
// the placement does not depend on any order of execution.  Offsets are 64-bit.  Nothing here is
// floating-point arithmetic: ratings move as 4- or 8-byte words.

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = kThreads * 8;  // old entries per workgroup of k_als_move

// the merge-sort path off, as in kernels_online.hip: one histogram, one scan and a pass per 8 key bits
using SortCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;

int bits_for(uint64_t v) {  // radix bits that hold every key < v
  int b = 1;
  while (b < 32 && (uint64_t{1} << b) < v) ++b;
  return b;
}

unsigned grid_for(int64_t n) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 1 << 16)));
}

__global__ void k_als_iota(int64_t n, int32_t* __restrict__ out) {
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x)
    out[p] = static_cast<int32_t>(p);
}

// The row of entry e: the largest x in [lo, hi] with off[x] <= e, given off[lo] <= e < off[hi + 1].  Rows
// without entries share their offset with the next row, so the largest such x is the one that holds e.
__device__ inline int64_t row_of(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <typename V>
__global__ __launch_bounds__(kThreads) void k_als_move(const int64_t* __restrict__ old_off, int64_t old_rows,
                                                       int64_t old_nnz, const int64_t* __restrict__ new_off,
                                                       const int32_t* __restrict__ old_cols,
                                                       const V* __restrict__ old_vals, int32_t* __restrict__ new_cols,
                                                       V* __restrict__ new_vals) {
  __shared__ int64_t span[2];
  const int64_t t0 = blockIdx.x * static_cast<int64_t>(kTile);
  const int64_t t1 = t0 + kTile < old_nnz ? t0 + kTile : old_nnz;
  if (t0 >= t1) return;  // (the grid has no such workgroup)
  if (threadIdx.x < 2) span[threadIdx.x] = row_of(old_off, 0, old_rows - 1, threadIdx.x == 0 ? t0 : t1 - 1);
  __syncthreads();
  int64_t lo = span[0];
  const int64_t hi = span[1];
  for (int64_t e = t0 + threadIdx.x; e < t1; e += kThreads) {
    lo = row_of(old_off, lo, hi, e);  // a lane's entries ascend, so its rows do
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
    int64_t lo = 0, hi = s;  // the first position of x's run in the sorted keys
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (key[mid] < x) lo = mid + 1;
      else hi = mid;
    }
    const int64_t had = static_cast<int64_t>(x) < old_rows ? old_off[x + 1] - old_off[x] : 0;
    const int64_t d = new_off[x] + had + (s - lo);
    const int32_t j = idx[s];
    new_cols[d] = static_cast<int32_t>(bcol[j]);
    new_vals[d] = bval[j];
  }
}

template <typename V>
void append(const AlsAppendLaunch& L, AlsAppendScratch& sc) {
  if (L.old_nnz > 0)
    hipLaunchKernelGGL(k_als_move<V>, dim3(static_cast<unsigned>((L.old_nnz + kTile - 1) / kTile)), dim3(kThreads), 0,
                       L.st, L.old_off, L.old_rows, L.old_nnz, L.new_off, L.old_cols, static_cast<const V*>(L.old_vals),
                       L.new_cols, static_cast<V*>(L.new_vals));
  if (L.n > 0)
    hipLaunchKernelGGL(k_als_place<V>, dim3(grid_for(L.n)), dim3(kThreads), 0, L.st, sc.key.as<uint32_t>(),
                       sc.idx.as<int32_t>(), L.n, L.old_off, L.old_rows, L.new_off, L.bcol,
                       static_cast<const V*>(L.bval), L.new_cols, static_cast<V*>(L.new_vals));
}

}  // namespace

void launch_als_append(const AlsAppendLaunch& L, AlsAppendScratch& sc) {
  MF_REQUIRE(L.n >= 0 && L.n < (int64_t{1} << 31) && L.old_rows >= 0 && L.new_rows >= L.old_rows && L.old_nnz >= 0 &&
                 (L.elem_bytes == 4 || L.elem_bytes == 8),
             "launch_als_append: bad sizes");
  // 2^31 - 1 workgroups of k_als_move at the most: 2^42 entries
  MF_REQUIRE((L.old_nnz + kTile - 1) / kTile < (int64_t{1} << 31), "launch_als_append: the CSR is too long");
  if (L.n > 0) {
    const size_t nb = static_cast<size_t>(L.n) * 4;
    const unsigned int N = static_cast<unsigned int>(L.n);
    const int bits = bits_for(static_cast<uint64_t>(L.new_rows));
    sc.key.alloc(nb);
    sc.iota.alloc(nb);
    sc.idx.alloc(nb);
    hipLaunchKernelGGL(k_als_iota, dim3(grid_for(L.n)), dim3(kThreads), 0, L.st, L.n, sc.iota.as<int32_t>());
    size_t tb = 0;
    MF_HIP(rocprim::radix_sort_pairs<SortCfg>(nullptr, tb, L.brow, sc.key.as<uint32_t>(), sc.iota.as<int32_t>(),
                                               sc.idx.as<int32_t>(), N, 0, bits, L.st));
    // (may reallocate: the caller drains the stream between two launches that share `sc`, als_append_both)
    sc.tmp.alloc(std::max<size_t>(tb, 256));
    MF_HIP(rocprim::radix_sort_pairs<SortCfg>(sc.tmp.get(), tb, L.brow, sc.key.as<uint32_t>(), sc.iota.as<int32_t>(),
                                               sc.idx.as<int32_t>(), N, 0, bits, L.st));
  }
  L.elem_bytes == 8 ? append<uint64_t>(L, sc) : append<uint32_t>(L, sc);
  MF_HIP(hipGetLastError());
}

}  // namespace mfhip
