// kernels_als_remove.hip -- mf_als_remove / mf_als_remove_rows / mf_seen_remove: entries taken out of a
// packed CSR on the device, the survivors keeping their order.  The mirror image of kernels_als_append.hip.
//
// Which entries go.  Either a batch of keys (row << 32) | col, where m keys naming one pair take the pair's
// m OLDEST entries (the first m in the row's order; fewer when the row holds fewer), or marks: every entry
// whose row, or whose column, is marked.
//
//  select   the batch is sorted (sort_positions: stable, the 64-bit keys carrying the caller's position j).
//           k_remove_scan takes the entries by the tile walk of csr_device.hpp, with one more search per end
//           of the tile for the batch keys of its first and last row, and every entry looks its own key up
//           in that span of the sorted batch.  The few that are named are the candidates.  One pass counts
//           them per tile, a scan of the tile counts gives every tile its base, a second pass writes them:
//           cand_e / cand_key, ascending by position.
//  age      the candidates are sorted by key (stable, so inside a pair's run they stay in position order,
//           which is their age).  The candidate at place t of its run goes when t < the pair's multiplicity in
//           the batch; the batch key at place t of its run is a hit when t < the run of candidates.  Both are
//           differences of positions in two sorted arrays: the cost is (candidates + batch) x log, never
//           (batch entries of a row) x (row length).
//  move     a scan of the kill flags (candidate order = position order) gives, per candidate, the entries
//           removed before it.  k_remove_move walks the entries in the same tiles: a tile's candidates are
//           cand_e[tile_base[t], tile_base[t + 1]), so an entry finds the removed entries before it with a
//           search of that short range, and moves to e - that count.  Every survivor is read once and written
//           once; reads are contiguous.  The new offsets are the old ones less the entries removed before them.
//
// Integer work only: the one floating-point operation is `value > 0` on the stored bits, for the per-row
// count of removed positive ratings (an atomic add of 1 whose sum alone is read).  No position depends on
// any order of execution.  Offsets and positions are 64-bit; a call names and removes fewer than 2^31 entries.

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "csr_device.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

using dev::lower;
using dev::upper;
constexpr int kThreads = dev::kCsrThreads;
constexpr int kTile = dev::kCsrTile;   // entries per workgroup of the tiled walks
constexpr int kPer = kTile / kThreads;
constexpr int kWaves = kThreads / 64;  // gfx950 runs wave64

// What marks an entry: its key in the sorted batch keys bkey[0, nb), or a mark on its row or its column.
struct Sel {
  const uint64_t* bkey;
  int64_t nb;
  const uint8_t* rowmark;
  const uint8_t* colmark;
};

__device__ inline uint64_t key_of(int64_t row, int32_t col) {
  return (static_cast<uint64_t>(row) << 32) | static_cast<uint32_t>(col);
}

// Flags set before this thread in the workgroup, in thread order; *total = all of them.  Every thread calls it.
__device__ inline int block_rank(bool f, int* __restrict__ wsum, int* total) {
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
  for (int x = 0; x < kWaves; ++x) {
    base += x < w ? wsum[x] : 0;
    tot += wsum[x];
  }
  __syncthreads();  // wsum is written again in the next round
  *total = tot;
  return base + __popcll(b & ((1ull << lane) - 1));
}

// The tiled walk of the entries.  kEmit = false: tile_cnt[tile] = the tile's candidates.  kEmit = true: the
// candidates written at tile_base[tile] onwards, in position order.
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void k_remove_scan(const int64_t* __restrict__ off, int64_t rows, int64_t nnz,
                                                          const int32_t* __restrict__ cols, Sel S,
                                                          int64_t* __restrict__ tile_cnt,
                                                          const int64_t* __restrict__ tile_base,
                                                          int64_t* __restrict__ cand_e, uint64_t* __restrict__ cand_key) {
  __shared__ int64_t span[4];
  __shared__ int wsum[kWaves];
  dev::CsrTile T;
  if (!dev::csr_tile(off, rows, nnz, span, T)) return;
  const int64_t t0 = T.t0, t1 = T.t1, hi = T.hi;
  if (threadIdx.x < 2) {  // the batch keys of the tile's rows
    span[2 + threadIdx.x] =
        S.bkey ? lower<uint64_t>(S.bkey, 0, S.nb, static_cast<uint64_t>(span[threadIdx.x] + threadIdx.x) << 32) : 0;
  }
  __syncthreads();
  int64_t lo = T.lo;
  const int64_t blo = span[2], bhi = span[3];
  if (S.bkey && blo == bhi) {  // no batch key names a row of this tile
    if (!kEmit && threadIdx.x == 0) tile_cnt[blockIdx.x] = 0;
    return;
  }
  int64_t at = kEmit ? tile_base[blockIdx.x] : 0;
  for (int i = 0; i < kPer; ++i) {
    const int64_t e = t0 + static_cast<int64_t>(i) * kThreads + threadIdx.x;
    bool f = false;
    uint64_t key = 0;
    if (e < t1) {
      lo = dev::row_of(off, lo, hi, e);  // a lane's entries ascend, so its rows do
      const int32_t col = cols[e];
      key = key_of(lo, col);
      if (S.bkey) {
        const int64_t p = lower<uint64_t>(S.bkey, blo, bhi, key);
        f = p < bhi && S.bkey[p] == key;
      } else {
        f = (S.rowmark && S.rowmark[lo]) || (S.colmark && S.colmark[col]);
      }
    }
    int tot;
    const int r = block_rank(f, wsum, &tot);
    if (kEmit && f) {
      cand_e[at + r] = e;
      cand_key[at + r] = key;
    }
    at += tot;
  }
  if (!kEmit && threadIdx.x == 0) tile_cnt[blockIdx.x] = at;
}

// skey[0, C): the candidates' keys sorted, sidx their candidate numbers (ascending inside a run: by age).
// kill[c] = 1 for the candidates whose place in their run is below the pair's multiplicity in the batch.
__global__ void k_remove_kill(const uint64_t* __restrict__ skey, const int32_t* __restrict__ sidx, int64_t C,
                              const uint64_t* __restrict__ bkey, int64_t nb, int32_t* __restrict__ kill) {
  for (int64_t s = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; s < C;
       s += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint64_t K = skey[s];
    const int64_t age = s - lower<uint64_t>(skey, 0, s, K);
    const int64_t b0 = lower<uint64_t>(bkey, 0, nb, K);
    const int64_t m = upper(bkey, b0, nb, K) - b0;
    if (age < m) kill[sidx[s]] = 1;
  }
}

// found[bidx[t]] = 1 where the batch key at place t of its run still finds a candidate (C may be 0).
__global__ void k_remove_found(const uint64_t* __restrict__ bkey, const int32_t* __restrict__ bidx, int64_t nb,
                               const uint64_t* __restrict__ skey, int64_t C, uint8_t* __restrict__ found) {
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < nb;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint64_t K = bkey[t];
    const int64_t place = t - lower<uint64_t>(bkey, 0, t, K);
    const int64_t c0 = lower<uint64_t>(skey, 0, C, K);
    const int64_t have = upper(skey, c0, C, K) - c0;
    found[bidx[t]] = place < have ? 1 : 0;
  }
}

// rempos[row] += 1 for every removed entry whose stored value is > 0 (kill == null: every candidate goes).
template <typename V>
__global__ void k_remove_positive(const int64_t* __restrict__ cand_e, const uint64_t* __restrict__ cand_key, int64_t C,
                                  const int32_t* __restrict__ kill, const V* __restrict__ vals,
                                  int32_t* __restrict__ rempos) {
  for (int64_t c = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; c < C;
       c += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    if (kill && !kill[c]) continue;
    if (vals[cand_e[c]] > V(0)) atomicAdd(&rempos[cand_key[c] >> 32], 1);
  }
}

// new_off[r] = off[r] less the entries removed before it, r = 0 .. rows.  before[c] (null: c itself) = the
// removed entries among the candidates [0, c), c = 0 .. C.
__global__ void k_remove_off(const int64_t* __restrict__ off, int64_t rows, const int64_t* __restrict__ cand_e, int64_t C,
                             const int32_t* __restrict__ before, int64_t* __restrict__ new_off) {
  for (int64_t r = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; r <= rows;
       r += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t c = lower<int64_t>(cand_e, 0, C, off[r]);
    new_off[r] = off[r] - (before ? before[c] : c);
  }
}

// V: the stored value as 4 or 8 bytes; kVals = false: a CSR without values.
template <typename V, bool kVals>
__global__ __launch_bounds__(kThreads) void k_remove_move(int64_t nnz, const int64_t* __restrict__ tile_base,
                                                          const int64_t* __restrict__ cand_e,
                                                          const int32_t* __restrict__ kill,
                                                          const int32_t* __restrict__ before,
                                                          const int32_t* __restrict__ cols, const V* __restrict__ vals,
                                                          int32_t* __restrict__ new_cols, V* __restrict__ new_vals) {
  const int64_t t0 = blockIdx.x * static_cast<int64_t>(kTile);
  const int64_t t1 = t0 + kTile < nnz ? t0 + kTile : nnz;
  const int64_t c0 = tile_base[blockIdx.x], c1 = tile_base[blockIdx.x + 1];
  for (int64_t e = t0 + threadIdx.x; e < t1; e += kThreads) {
    const int64_t c = lower<int64_t>(cand_e, c0, c1, e);
    if (c < c1 && cand_e[c] == e && (!kill || kill[c])) continue;  // this entry goes
    const int64_t d = e - (before ? before[c] : c);
    new_cols[d] = cols[e];
    if (kVals) new_vals[d] = vals[e];
  }
}

}  // namespace

int64_t launch_als_remove_select(const AlsRemoveLaunch& L, AlsRemoveScratch& sc, uint8_t* found, int32_t* rempos) {
  MF_REQUIRE(L.rows >= 0 && L.rows < (int64_t{1} << 31) && L.nnz >= 0 && L.nb >= 0 && L.nb < (int64_t{1} << 31) &&
                 (L.elem_bytes == 0 || L.elem_bytes == 4 || L.elem_bytes == 8),
             "launch_als_remove_select: bad sizes");
  const int64_t tiles = (L.nnz + kTile - 1) / kTile;
  MF_REQUIRE(tiles < (int64_t{1} << 31), "launch_als_remove_select: the CSR is too long");
  const bool batch = L.bkey != nullptr;
  MF_REQUIRE(batch || L.rowmark || L.colmark, "launch_als_remove_select: nothing selects");
  sc.batch = batch;
  sc.cands = 0;
  if (found && L.nb > 0) MF_HIP(hipMemsetAsync(found, 0, static_cast<size_t>(L.nb), L.st));
  if (rempos && L.rows > 0) MF_HIP(hipMemsetAsync(rempos, 0, static_cast<size_t>(L.rows) * 4, L.st));
  if (L.nnz == 0 || L.rows == 0 || (batch && L.nb == 0)) return 0;
  const int key_bits = 32 + radix_bits_for(static_cast<uint64_t>(L.rows));
  if (batch) {
    sc.key.alloc(static_cast<size_t>(L.nb) * 8);
    sc.idx.alloc(static_cast<size_t>(L.nb) * 4);
    sort_positions(L.st, sc.tmp, sc.iota, L.bkey, sc.key.as<uint64_t>(), sc.idx.as<int32_t>(), L.nb, key_bits);
  }
  const Sel S{batch ? sc.key.as<uint64_t>() : nullptr, batch ? L.nb : 0, L.rowmark, L.colmark};
  sc.tile_cnt.alloc(static_cast<size_t>(tiles + 1) * 8);
  sc.tile_base.alloc(static_cast<size_t>(tiles + 1) * 8);
  MF_HIP(hipMemsetAsync(sc.tile_cnt.as<int64_t>() + tiles, 0, 8, L.st));
  hipLaunchKernelGGL(k_remove_scan<false>, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, L.st, L.off, L.rows,
                     L.nnz, L.cols, S, sc.tile_cnt.as<int64_t>(), nullptr, nullptr, nullptr);
  scan_exclusive(L.st, sc.tmp, sc.tile_cnt.as<int64_t>(), sc.tile_base.as<int64_t>(), tiles + 1);
  int64_t C = 0;
  MF_HIP(hipMemcpyAsync(&C, sc.tile_base.as<int64_t>() + tiles, 8, hipMemcpyDeviceToHost, L.st));
  MF_HIP(hipStreamSynchronize(L.st));
  MF_REQUIRE(C < (int64_t{1} << 31) - 1, "one call names fewer than 2^31 - 1 stored entries");
  sc.cands = C;
  if (C == 0) return 0;
  sc.cand_e.alloc(static_cast<size_t>(C) * 8);
  sc.cand_key.alloc(static_cast<size_t>(C) * 8);
  hipLaunchKernelGGL(k_remove_scan<true>, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, L.st, L.off, L.rows,
                     L.nnz, L.cols, S, nullptr, sc.tile_base.as<int64_t>(), sc.cand_e.as<int64_t>(),
                     sc.cand_key.as<uint64_t>());
  int64_t gone = C;
  if (batch) {
    sc.skey.alloc(static_cast<size_t>(C) * 8);
    sc.sidx.alloc(static_cast<size_t>(C) * 4);
    sort_positions(L.st, sc.tmp, sc.iota, sc.cand_key.as<uint64_t>(), sc.skey.as<uint64_t>(), sc.sidx.as<int32_t>(), C,
                   key_bits);
    sc.kill.alloc(static_cast<size_t>(C + 1) * 4);
    sc.before.alloc(static_cast<size_t>(C + 1) * 4);
    MF_HIP(hipMemsetAsync(sc.kill.get(), 0, static_cast<size_t>(C + 1) * 4, L.st));
    hipLaunchKernelGGL(k_remove_kill, dim3(grid_for(C)), dim3(kThreads), 0, L.st, sc.skey.as<uint64_t>(),
                       sc.sidx.as<int32_t>(), C, sc.key.as<uint64_t>(), L.nb, sc.kill.as<int32_t>());
    if (found)
      hipLaunchKernelGGL(k_remove_found, dim3(grid_for(L.nb)), dim3(kThreads), 0, L.st, sc.key.as<uint64_t>(),
                         sc.idx.as<int32_t>(), L.nb, sc.skey.as<uint64_t>(), C, found);
    scan_exclusive(L.st, sc.tmp, sc.kill.as<int32_t>(), sc.before.as<int32_t>(), C + 1);
    int32_t g = 0;
    MF_HIP(hipMemcpyAsync(&g, sc.before.as<int32_t>() + C, 4, hipMemcpyDeviceToHost, L.st));
    MF_HIP(hipStreamSynchronize(L.st));
    gone = g;
  }
  if (rempos && L.elem_bytes != 0 && gone > 0) {
    const int32_t* kill = batch ? sc.kill.as<int32_t>() : nullptr;
    if (L.elem_bytes == 8)
      hipLaunchKernelGGL(k_remove_positive<double>, dim3(grid_for(C)), dim3(kThreads), 0, L.st, sc.cand_e.as<int64_t>(),
                         sc.cand_key.as<uint64_t>(), C, kill, static_cast<const double*>(L.vals), rempos);
    else
      hipLaunchKernelGGL(k_remove_positive<float>, dim3(grid_for(C)), dim3(kThreads), 0, L.st, sc.cand_e.as<int64_t>(),
                         sc.cand_key.as<uint64_t>(), C, kill, static_cast<const float*>(L.vals), rempos);
  }
  MF_HIP(hipGetLastError());
  return gone;
}

void launch_als_remove_move(const AlsRemoveLaunch& L, const AlsRemoveScratch& sc, int64_t* new_off, int32_t* new_cols,
                            void* new_vals) {
  MF_REQUIRE(sc.cands > 0 && L.nnz > 0, "launch_als_remove_move: nothing was selected");
  const int64_t tiles = (L.nnz + kTile - 1) / kTile, C = sc.cands;
  const int32_t* kill = sc.batch ? sc.kill.as<int32_t>() : nullptr;
  const int32_t* before = sc.batch ? sc.before.as<int32_t>() : nullptr;
  hipLaunchKernelGGL(k_remove_off, dim3(grid_for(L.rows + 1)), dim3(kThreads), 0, L.st, L.off, L.rows,
                     sc.cand_e.as<int64_t>(), C, before, new_off);
  const dim3 grid(static_cast<unsigned>(tiles)), block(kThreads);
  if (L.elem_bytes == 8)
    hipLaunchKernelGGL((k_remove_move<uint64_t, true>), grid, block, 0, L.st, L.nnz, sc.tile_base.as<int64_t>(),
                       sc.cand_e.as<int64_t>(), kill, before, L.cols, static_cast<const uint64_t*>(L.vals), new_cols,
                       static_cast<uint64_t*>(new_vals));
  else if (L.elem_bytes == 4)
    hipLaunchKernelGGL((k_remove_move<uint32_t, true>), grid, block, 0, L.st, L.nnz, sc.tile_base.as<int64_t>(),
                       sc.cand_e.as<int64_t>(), kill, before, L.cols, static_cast<const uint32_t*>(L.vals), new_cols,
                       static_cast<uint32_t*>(new_vals));
  else
    hipLaunchKernelGGL((k_remove_move<uint32_t, false>), grid, block, 0, L.st, L.nnz, sc.tile_base.as<int64_t>(),
                       sc.cand_e.as<int64_t>(), kill, before, L.cols, static_cast<const uint32_t*>(nullptr), new_cols,
                       static_cast<uint32_t*>(nullptr));
  MF_HIP(hipGetLastError());
}

}  // namespace mfhip
