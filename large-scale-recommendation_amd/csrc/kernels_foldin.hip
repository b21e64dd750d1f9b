// kernels_foldin.hip -- the transient CSR of a fold-in batch (mf_als_foldin, mf_recommend_foldin), built on the
// device from the callers' lists as uploaded.  Integer work but for one conversion and one `> 0` per entry.
//
//  resolve   launch_id_lookup (kernels_online.hip) over the counterpart side's id mirror: ids -> rows, kRowMiss
//            for an id the model does not hold.
//  place     a flag per entry (its id is known), an exclusive scan of the flags = where every kept entry lands:
//            the compaction is stable, a query's kept entries keep the order of its list.
//  compact   one walk over the ENTRIES in tiles (csr_device.hpp), whatever queries they belong to: a kept entry
//            moves to its place as (counterpart row, rating in the context's precision) -- the only move --
//            and, for the fused call, leaves its exclusion key (query position << 32) | row beside it; every
//            lane counts the kept entries and the ratings > 0 (after the conversion) of the query it is in
//            and adds them to the query's two counters when its query changes.  Integer atomics: the counts do
//            not depend on the order of the adds.  A list of 100k entries is 49 workgroups' work, never one
//            lane's.
// The searches, the tile walk, the scan and the identity come from csr_search.hpp, csr_device.hpp and
// kernels_table.hip; nothing of them is defined here again.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "csr_device.hpp"
#include "id_index.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = dev::kCsrThreads;

// flag[j] = 1 where entry j names a row (flag has n + 1 entries, the last 0: the scan's last value is the
// number of kept entries)
__global__ void k_fold_flags(const uint32_t* __restrict__ row, int64_t n, int32_t* __restrict__ flag) {
  for (int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; j <= n;
       j += static_cast<int64_t>(gridDim.x) * blockDim.x)
    flag[j] = (j < n && row[j] != kRowMiss) ? 1 : 0;
}

// off[nq + 1]: the batch's lists over its n entries; wp: the exclusive scan of the flags.  cnt[q] = (kept, n+).
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fold_compact(const int64_t* __restrict__ off, int64_t nq, int64_t n,
                                                           const uint32_t* __restrict__ row,
                                                           const double* __restrict__ rating,
                                                           const int32_t* __restrict__ wp, int32_t* __restrict__ cols,
                                                           T* __restrict__ vals, uint64_t* __restrict__ keys,
                                                           int32_t* __restrict__ cnt) {
  __shared__ int64_t span[2];
  dev::CsrTile Tl;
  if (!dev::csr_tile(off, nq, n, span, Tl)) return;
  int64_t lo = Tl.lo, cur = -1;
  int32_t kept = 0, pos = 0;
  for (int64_t e = Tl.t0 + threadIdx.x; e < Tl.t1; e += kThreads) {
    lo = dev::row_of(off, lo, Tl.hi, e);  // a lane's entries ascend, so its queries do
    const uint32_t c = row[e];
    if (c == kRowMiss) continue;
    const T v = static_cast<T>(rating[e]);  // the context's precision: one rounding, as mf_als_prepare's
    const int32_t w = wp[e];
    cols[w] = static_cast<int32_t>(c);
    vals[w] = v;
    if (keys) keys[w] = (static_cast<uint64_t>(lo) << 32) | c;
    if (lo != cur) {
      if (kept) {
        atomicAdd(cnt + 2 * cur, kept);
        if (pos) atomicAdd(cnt + 2 * cur + 1, pos);
      }
      cur = lo;
      kept = pos = 0;
    }
    ++kept;
    pos += v > T(0);
  }
  if (kept) {
    atomicAdd(cnt + 2 * cur, kept);
    if (pos) atomicAdd(cnt + 2 * cur + 1, pos);
  }
}

}  // namespace

void launch_foldin_compact(const FoldinLaunch& L, FoldinScratch& sc) {
  MF_REQUIRE(L.nq > 0 && L.n >= 0 && L.n < (int64_t{1} << 31) - 1, "fold-in: a batch holds fewer than 2^31 - 1 entries");
  MF_HIP(hipMemsetAsync(L.cnt, 0, static_cast<size_t>(L.nq) * 8, L.st));
  if (L.n == 0) return;
  int32_t* const miss = static_cast<int32_t*>(temp_storage(L.st, sc.miss, 4));
  int32_t* const flag = static_cast<int32_t*>(temp_storage(L.st, sc.flag, static_cast<size_t>(L.n + 1) * 4));
  int32_t* const wp = static_cast<int32_t*>(temp_storage(L.st, sc.wp, static_cast<size_t>(L.n + 1) * 4));
  // the lists' ids as the lookup's first array; its second (no table: all misses) is scratch behind them
  launch_id_lookup(L.st, L.ids, L.n, L.slots, L.mask, nullptr, 0, miss);
  hipLaunchKernelGGL(k_fold_flags, dim3(grid_for(L.n + 1)), dim3(kGridThreads), 0, L.st, L.ids, L.n, flag);
  scan_exclusive<int32_t>(L.st, sc.tmp, flag, wp, L.n + 1);
  const unsigned tiles = static_cast<unsigned>((L.n + dev::kCsrTile - 1) / dev::kCsrTile);
  if (L.f64)
    hipLaunchKernelGGL(k_fold_compact<double>, dim3(tiles), dim3(kThreads), 0, L.st, L.off, L.nq, L.n, L.ids, L.ratings,
                       wp, L.cols, static_cast<double*>(L.vals), L.keys, L.cnt);
  else
    hipLaunchKernelGGL(k_fold_compact<float>, dim3(tiles), dim3(kThreads), 0, L.st, L.off, L.nq, L.n, L.ids, L.ratings,
                       wp, L.cols, static_cast<float*>(L.vals), L.keys, L.cnt);
  MF_HIP(hipGetLastError());
}

}  // namespace mfhip
