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
//          k_seen_move walks the OLD ENTRIES in tiles of 2048 as k_als_move does: two searches of old_off per
//          workgroup for the rows of its first and last entry, one search each for the novel range of its
//          first and last key, and a lane narrows its row and its count inside those spans.  Every old entry
//          is read once and written once; a long row is moved by as many workgroups as it has tiles.
// No atomics, no floating point, and no kernel here waits on another wave: the placement depends on no order
// of execution.  Offsets and positions are 64-bit; a batch holds fewer than 2^31 - 1 pairs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = kThreads * 8;  // entries per workgroup of the tiled walks
constexpr uint32_t kMiss = 0xFFFFFFFFu;

unsigned grid_for(int64_t n) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 1 << 16)));
}

// The row of entry e: the largest x in [lo, hi] with off[x] <= e, given off[lo] <= e < off[hi + 1] (rows
// without entries share their offset with the next row).
__device__ inline int64_t row_of(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The first position of [b, e) whose entry is >= c (e when there is none); entries ascend.
__device__ inline int64_t lower_bound(const int32_t* __restrict__ ent, int64_t b, int64_t e, int32_t c) {
  while (b < e) {
    const int64_t m = (b + e) >> 1;
    if (ent[m] < c) b = m + 1;
    else e = m;
  }
  return b;
}

__global__ void k_seen_pair_keys(const uint32_t* __restrict__ qrow, const uint32_t* __restrict__ crow, int64_t n,
                                 uint32_t rows, uint64_t* __restrict__ key) {
  for (int64_t x = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; x < n;
       x += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint32_t r = qrow[x], c = crow[x];
    key[x] = (r < rows && c != kMiss) ? (static_cast<uint64_t>(r) << 32) | c : static_cast<uint64_t>(rows) << 32;
  }
}

__global__ __launch_bounds__(kThreads) void k_seen_csr_keys(const int64_t* __restrict__ off, int64_t rows, int64_t nnz,
                                                            const int32_t* __restrict__ cols, bool swap,
                                                            uint64_t* __restrict__ key) {
  __shared__ int64_t span[2];
  const int64_t t0 = blockIdx.x * static_cast<int64_t>(kTile);
  const int64_t t1 = t0 + kTile < nnz ? t0 + kTile : nnz;
  if (t0 >= t1) return;  // (the grid has no such workgroup)
  if (threadIdx.x < 2) span[threadIdx.x] = row_of(off, 0, rows - 1, threadIdx.x == 0 ? t0 : t1 - 1);
  __syncthreads();
  int64_t lo = span[0];
  const int64_t hi = span[1];
  for (int64_t e = t0 + threadIdx.x; e < t1; e += kThreads) {
    lo = row_of(off, lo, hi, e);  // a lane's entries ascend, so its rows do
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
      at = lower_bound(old_ent, old_off[r], e, c);
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
  const int64_t t0 = blockIdx.x * static_cast<int64_t>(kTile);
  const int64_t t1 = t0 + kTile < old_nnz ? t0 + kTile : old_nnz;
  if (t0 >= t1) return;  // (the grid has no such workgroup)
  if (threadIdx.x < 2) {
    // the row of the tile's first / last entry, and the novel keys below that entry's key
    const int64_t e = threadIdx.x == 0 ? t0 : t1 - 1;
    const int64_t r = row_of(old_off, 0, old_rows - 1, e);
    span[threadIdx.x] = r;
    nspan[threadIdx.x] = lower_bound(nov_ent, nov_off[r], nov_off[r + 1], old_ent[e]);
  }
  __syncthreads();
  int64_t lo = span[0];
  const int64_t hi = span[1], nlo = nspan[0], nhi = nspan[1];
  for (int64_t e = t0 + threadIdx.x; e < t1; e += kThreads) {
    lo = row_of(old_off, lo, hi, e);  // a lane's entries ascend, so its rows do
    const int32_t c = old_ent[e];
    // the novel keys below (lo, c) end inside the row's novel range and inside the tile's
    const int64_t b = nov_off[lo] > nlo ? nov_off[lo] : nlo;
    const int64_t f = nov_off[lo + 1] < nhi ? nov_off[lo + 1] : nhi;
    new_ent[e + lower_bound(nov_ent, b, f, c)] = c;
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

__global__ void k_seen_iota(int32_t* __restrict__ out, int64_t n) {
  for (int64_t x = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; x < n;
       x += static_cast<int64_t>(gridDim.x) * blockDim.x)
    out[x] = static_cast<int32_t>(x);
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

void launch_seen_iota(hipStream_t st, int32_t* out, int64_t n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_seen_iota, dim3(grid_for(n)), dim3(kThreads), 0, st, out, n);
  MF_HIP(hipGetLastError());
}

}  // namespace mfhip
