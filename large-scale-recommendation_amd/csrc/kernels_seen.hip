// kernels_seen.hip -- the resident seen set (mf_seen_set / mf_seen_add / mf_seen_from_als): the distinct
// (user, item) pairs a recommender hides, kept on the device as one CSR per orientation over that side's
// FACTOR ROWS: off (int64, rows + 1) and ent (int32, the row's distinct counterpart rows, ascending).  That
// is, per query row, exactly the range excluded() of kernels_recommend.hip and the pair-rank kernels search,
// so a consumer needs no table of its own: only the row.
//
//  build   every pair as one 64-bit key (row << 32) | counterpart row (k_seen_pair_keys from uploaded rows,
//          k_seen_csr_keys from a CSR that is already on the device: the prepared ALS data, or the set's
//          own user-major table when the item-major one is wanted), then kernels_rank.hip's pieces: radix
//          sort over the bits in use, run heads kept, offsets by lower bound (rank_keys_sort / rank_keys_csr).
//  merge   mf_seen_add sorts the batch alone.  k_seen_novel drops the heads the table already holds (a binary
//          search in the key's row) and notes, per remaining key, the table's keys below it.  The novel keys
//          become a small CSR of their own (rank_keys_csr again), and every position of the new arrays then
//          follows from the two sorted sequences:
//              an old entry e with key K       lands at  e + #(novel keys < K)
//              the i-th novel key, N           lands at  i + #(old keys < N)
//          k_seen_move takes the OLD ENTRIES by the tile walk of csr_device.hpp, with one more search per end
//          of the tile for the novel range of its first and last key; a lane narrows its row and its count
//          inside those spans.  Every old entry is read once and written once.
// No atomics, no floating point, and no kernel here waits on another wave: the placement depends on no order
// of execution.  Offsets and positions are 64-bit; a batch holds fewer than 2^31 - 1 pairs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "csr_device.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

using dev::lower;
constexpr int kThreads = dev::kCsrThreads;
constexpr int kTile = dev::kCsrTile;  // entries per workgroup of the tiled walks

__global__ void k_seen_pair_keys(const uint32_t* __restrict__ qrow, const uint32_t* __restrict__ crow, int64_t n,
                                 uint32_t rows, uint64_t* __restrict__ key) {
  for (int64_t x = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; x < n;
       x += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint32_t r = qrow[x], c = crow[x];
    key[x] = (r < rows && c != kRowMiss) ? (static_cast<uint64_t>(r) << 32) | c : static_cast<uint64_t>(rows) << 32;
  }
}

__global__ __launch_bounds__(kThreads) void k_seen_csr_keys(const int64_t* __restrict__ off, int64_t rows, int64_t nnz,
                                                            const int32_t* __restrict__ cols, bool swap,
                                                            uint64_t* __restrict__ key) {
  __shared__ int64_t span[2];
  dev::CsrTile T;
  if (!dev::csr_tile(off, rows, nnz, span, T)) return;
  int64_t lo = T.lo;
  for (int64_t e = T.t0 + threadIdx.x; e < T.t1; e += kThreads) {
    lo = dev::row_of(off, lo, T.hi, e);  // a lane's entries ascend, so its rows do
    const uint64_t r = static_cast<uint64_t>(lo), c = static_cast<uint32_t>(cols[e]);
    key[e] = swap ? (c << 32) | r : (r << 32) | c;
  }
}

__global__ void k_seen_novel(const uint64_t* __restrict__ key2, int32_t* __restrict__ head, int64_t n,
                             const int64_t* __restrict__ old_off, int64_t old_rows,
                             const int32_t* __restrict__ old_ent, int64_t* __restrict__ lb) {
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    if (!head[p]) continue;
    const uint64_t K = key2[p];
    const int64_t r = static_cast<int64_t>(K >> 32);
    const int32_t c = static_cast<int32_t>(static_cast<uint32_t>(K));
    int64_t at = old_off[old_rows];  // a row the table does not cover: every old key lies below
    if (r < old_rows) {
      const int64_t e = old_off[r + 1];
      at = lower<int32_t>(old_ent, old_off[r], e, c);
      if (at < e && old_ent[at] == c) head[p] = 0;
    }
    lb[p] = at;
  }
}

__global__ void k_seen_new_off(const int64_t* __restrict__ old_off, int64_t old_rows, const int64_t* __restrict__ nov_off,
                               int64_t new_rows, int64_t* __restrict__ new_off) {
  for (int64_t r = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; r <= new_rows;
       r += static_cast<int64_t>(gridDim.x) * blockDim.x)
    new_off[r] = old_off[r < old_rows ? r : old_rows] + nov_off[r];
}

__global__ __launch_bounds__(kThreads) void k_seen_move(const int64_t* __restrict__ old_off, int64_t old_rows,
                                                        int64_t old_nnz, const int32_t* __restrict__ old_ent,
                                                        const int64_t* __restrict__ nov_off,
                                                        const int32_t* __restrict__ nov_ent,
                                                        int32_t* __restrict__ new_ent) {
  __shared__ int64_t span[2], nspan[2];
  dev::CsrTile T;
  if (!dev::csr_tile(old_off, old_rows, old_nnz, span, T)) return;
  if (threadIdx.x < 2) {  // the novel keys below the key of the tile's first / last entry
    const int64_t e = threadIdx.x == 0 ? T.t0 : T.t1 - 1, r = span[threadIdx.x];
    nspan[threadIdx.x] = lower<int32_t>(nov_ent, nov_off[r], nov_off[r + 1], old_ent[e]);
  }
  __syncthreads();
  int64_t lo = T.lo;
  const int64_t hi = T.hi, nlo = nspan[0], nhi = nspan[1];
  for (int64_t e = T.t0 + threadIdx.x; e < T.t1; e += kThreads) {
    lo = dev::row_of(old_off, lo, hi, e);  // a lane's entries ascend, so its rows do
    const int32_t c = old_ent[e];
    // the novel keys below (lo, c) end inside the row's novel range and inside the tile's
    const int64_t b = nov_off[lo] > nlo ? nov_off[lo] : nlo;
    const int64_t f = nov_off[lo + 1] < nhi ? nov_off[lo + 1] : nhi;
    new_ent[e + lower<int32_t>(nov_ent, b, f, c)] = c;
  }
}

__global__ void k_seen_place(const uint64_t* __restrict__ key2, const int32_t* __restrict__ head,
                             const int32_t* __restrict__ wp, const int64_t* __restrict__ lb, int64_t n,
                             int32_t* __restrict__ new_ent) {
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x)
    if (head[p]) new_ent[wp[p] + lb[p]] = static_cast<int32_t>(static_cast<uint32_t>(key2[p]));
}

__global__ void k_seen_pad(int64_t* __restrict__ off, int64_t have, int64_t want) {
  const int64_t last = off[have];
  for (int64_t r = have + 1 + blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; r <= want;
       r += static_cast<int64_t>(gridDim.x) * blockDim.x)
    off[r] = last;
}

__global__ void k_seen_gather(const int64_t* __restrict__ off, const int32_t* __restrict__ qrows, int n,
                              int64_t* __restrict__ beg, int64_t* __restrict__ end) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int32_t r = qrows[q];
  beg[q] = off[r];
  end[q] = off[r + 1];
}

unsigned tiles_of(int64_t nnz) {
  // 2^31 - 1 workgroups at the most: 2^42 entries
  MF_REQUIRE((nnz + kTile - 1) / kTile < (int64_t{1} << 31), "the seen set is too long");
  return static_cast<unsigned>((nnz + kTile - 1) / kTile);
}

}  // namespace

void launch_seen_pair_keys(hipStream_t st, const uint32_t* qrow, const uint32_t* crow, int64_t n, uint32_t rows,
                           uint64_t* key) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_seen_pair_keys, dim3(grid_for(n)), dim3(kThreads), 0, st, qrow, crow, n, rows, key);
  MF_HIP(hipGetLastError());
}

void launch_seen_csr_keys(hipStream_t st, const int64_t* off, int64_t rows, int64_t nnz, const int32_t* cols, bool swap,
                          uint64_t* key) {
  if (nnz <= 0 || rows <= 0) return;
  hipLaunchKernelGGL(k_seen_csr_keys, dim3(tiles_of(nnz)), dim3(kThreads), 0, st, off, rows, nnz, cols, swap, key);
  MF_HIP(hipGetLastError());
}

void launch_seen_novel(hipStream_t st, const uint64_t* key2, int32_t* head, int64_t n, const int64_t* old_off,
                       int64_t old_rows, const int32_t* old_ent, int64_t* lb) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_seen_novel, dim3(grid_for(n)), dim3(kThreads), 0, st, key2, head, n, old_off, old_rows, old_ent,
                     lb);
  MF_HIP(hipGetLastError());
}

void launch_seen_merge(hipStream_t st, const int64_t* old_off, int64_t old_rows, int64_t old_nnz, const int32_t* old_ent,
                       const int64_t* nov_off, const int32_t* nov_ent, int64_t new_rows, const uint64_t* key2,
                       const int32_t* head, const int32_t* wp, const int64_t* lb, int64_t n, int64_t* new_off,
                       int32_t* new_ent) {
  MF_REQUIRE(old_rows >= 0 && new_rows >= old_rows && old_nnz >= 0 && n >= 0, "launch_seen_merge: bad sizes");
  hipLaunchKernelGGL(k_seen_new_off, dim3(grid_for(new_rows + 1)), dim3(kThreads), 0, st, old_off, old_rows, nov_off,
                     new_rows, new_off);
  if (old_nnz > 0 && old_rows > 0)
    hipLaunchKernelGGL(k_seen_move, dim3(tiles_of(old_nnz)), dim3(kThreads), 0, st, old_off, old_rows, old_nnz, old_ent,
                       nov_off, nov_ent, new_ent);
  if (n > 0)
    hipLaunchKernelGGL(k_seen_place, dim3(grid_for(n)), dim3(kThreads), 0, st, key2, head, wp, lb, n, new_ent);
  MF_HIP(hipGetLastError());
}

void launch_seen_pad(hipStream_t st, int64_t* off, int64_t have, int64_t want) {
  if (want <= have) return;
  hipLaunchKernelGGL(k_seen_pad, dim3(grid_for(want - have)), dim3(kThreads), 0, st, off, have, want);
  MF_HIP(hipGetLastError());
}

void launch_seen_gather(hipStream_t st, const int64_t* off, const int32_t* qrows, int n, int64_t* beg, int64_t* end) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_seen_gather, dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     off, qrows, n, beg, end);
  MF_HIP(hipGetLastError());
}

}  // namespace mfhip
