// kernels_rank.hip -- ranking metrics of held-out pairs against the model's top-N lists
// (mf_rank_eval): the pair tables of a call built on the device, the per-query metrics of a batch
// of lists, and the fixed-order sums over all queries.
//
//  pair tables   rank_query_set: a flag per query-side row named by a known pair, an exclusive scan
//                of the flags = every row's position among the evaluated queries, and the ascending
//                row list launch_recommend takes as qrows.  rank_pair_csr: every pair as one 64-bit key
//                (query position << 32) | low, radix-sorted over the bits in use, run heads kept
//                (duplicates dropped), offsets by lower bound.  low = the candidate row (exclusions:
//                launch_recommend's excl_off / excl_rows) or the candidate id with the sign bit
//                flipped (ground truth: unsigned order = id order; stored back as the id).  A pair
//                that is dropped (unknown or unevaluated query, exclusion with an unknown candidate)
//                takes the key nq << 32 and sorts behind every kept pair.
//  k_rank_metrics  one wave per query of a batch, over the ids / counts k_rec_merge wrote: lane l looks
//                list positions l and l + 64 up in the query's ground-truth row (binary search), two
//                ballots give the 128-bit hit mask, and lane 0 takes the sums over its set bits in
//                ascending position, in f64.  Gains 1 / log(i + 2) and their prefix sums come from the
//                host (libm), so a host replay of the same sums matches bit for bit; this file is
//                compiled with -ffp-contract=off.
//  k_rank_slice / k_rank_total  the sums over all queries: slices of 1024 queries, a fixed tree inside
//                a slice, slices added in ascending order.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <hipcub/device/device_radix_sort.hpp>
#include <hipcub/device/device_scan.hpp>

#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "csr_search.hpp"
#include "kernels.hpp"
#include "mfhip.h"

namespace mfhip {
namespace {

constexpr int kThreads = kGridThreads;

// flag[row] = 1 for every known query row of the pairs (flag has rows + 1 entries, the last stays 0)
__global__ void k_rank_flags(const uint32_t* __restrict__ qrow, int64_t n, uint32_t rows, int32_t* __restrict__ flag) {
  for (int64_t x = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; x < n;
       x += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint32_t r = qrow[x];
    if (r < rows) flag[r] = 1;
  }
}

// qrows[pos[r]] = r for every flagged row: ascending rows
__global__ void k_rank_compact(const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, uint32_t rows,
                               int32_t* __restrict__ qrows) {
  for (int64_t r = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; r < rows;
       r += static_cast<int64_t>(gridDim.x) * blockDim.x)
    if (flag[r]) qrows[pos[r]] = static_cast<int32_t>(r);
}

// key[x] = (position of the pair's query << 32) | low, or nq << 32 for a pair that is dropped.
// gt: low = cand[x] (an id) with the sign bit flipped, unknown candidates kept; else low = cand[x] (a
// candidate row), kRowMiss dropped.
__global__ void k_rank_keys(const uint32_t* __restrict__ qrow, const uint32_t* __restrict__ cand, int64_t n,
                            uint32_t rows, const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int64_t nq,
                            bool gt, uint64_t* __restrict__ key) {
  for (int64_t x = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; x < n;
       x += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint32_t r = qrow[x], c = cand[x];
    uint64_t k = static_cast<uint64_t>(nq) << 32;
    if (r < rows && flag[r] && (gt || c != kRowMiss))
      k = (static_cast<uint64_t>(static_cast<uint32_t>(pos[r])) << 32) | (gt ? c ^ 0x80000000u : c);
    key[x] = k;
  }
}

// head[p] = 1 where a kept key differs from its predecessor (head has n + 1 entries, the last 0)
__global__ void k_rank_heads(const uint64_t* __restrict__ key, int64_t n, int64_t nq, int32_t* __restrict__ head) {
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p <= n;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x)
    head[p] = (p < n && static_cast<int64_t>(key[p] >> 32) < nq && (p == 0 || key[p] != key[p - 1])) ? 1 : 0;
}

// ent[wp[p]] = the low part of every run head (wp = exclusive scan of head)
__global__ void k_rank_entries(const uint64_t* __restrict__ key, const int32_t* __restrict__ head,
                               const int32_t* __restrict__ wp, int64_t n, bool gt, int32_t* __restrict__ ent) {
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    if (!head[p]) continue;
    const uint32_t low = static_cast<uint32_t>(key[p]);
    ent[wp[p]] = static_cast<int32_t>(gt ? low ^ 0x80000000u : low);
  }
}

// off[q] = distinct kept pairs before query q's first key, q = 0 .. nq (wp[n] = all of them)
__global__ void k_rank_offsets(const uint64_t* __restrict__ key, const int32_t* __restrict__ wp, int64_t n, int64_t nq,
                               int64_t* __restrict__ off) {
  for (int64_t q = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; q <= nq;
       q += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint64_t want = static_cast<uint64_t>(q) << 32;  // query q's first key
    off[q] = wp[dev::lower(key, 0, n, want)];
  }
}

// Is id in the query's sorted ground-truth ids [b, e)?
__device__ __forceinline__ bool in_truth(const int32_t* __restrict__ ent, int64_t b, int64_t e, int32_t id) {
  return dev::contains(ent, b, e, id);
}

// Grid: ceil(nb / 4) blocks of 4 waves, wave = query of the batch.  goff (nb + 1) / met / cnt point at the
// batch's first query; tab = 128 gains, then idcg[0 .. 128].
__global__ __launch_bounds__(256) void k_rank_metrics(const int32_t* __restrict__ ids, const int32_t* __restrict__ counts,
                                                      int nb, int N, const int64_t* __restrict__ goff,
                                                      const int32_t* __restrict__ gent, const double* __restrict__ tab,
                                                      double* __restrict__ met, int64_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nb) return;  // wave-uniform
  const int c = min(counts[q], N);
  const int64_t b = goff[q], e = goff[q + 1];
  const int32_t* list = ids + static_cast<int64_t>(q) * N;
  const bool h0 = lane < c && in_truth(gent, b, e, list[lane]);
  const bool h1 = lane + 64 < c && in_truth(gent, b, e, list[lane + 64]);
  const uint64_t m0 = __ballot(h0), m1 = __ballot(h1);
  if (lane != 0) return;
  const int64_t g = e - b;
  int hits = 0, first = -1;
  double ap = 0.0, dcg = 0.0;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    uint64_t m = half ? m1 : m0;
    while (m) {
      const int i = 64 * half + __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      ++hits;
      if (first < 0) first = i;
      ap = ap + static_cast<double>(hits) / static_cast<double>(i + 1);
      dcg = dcg + tab[i];
    }
  }
  const double dg = static_cast<double>(g);
  double* o = met + static_cast<int64_t>(q) * MF_RANK_NMETRICS;
  o[0] = static_cast<double>(hits) / static_cast<double>(N);
  o[1] = static_cast<double>(hits) / dg;
  o[2] = ap / dg;
  o[3] = dcg / tab[MF_RECOMMEND_MAX_TOP + (g < N ? static_cast<int>(g) : N)];
  o[4] = first >= 0 ? 1.0 / static_cast<double>(first + 1) : 0.0;
  o[5] = hits > 0 ? 1.0 : 0.0;
  cnt[2 * static_cast<int64_t>(q)] = hits;
  cnt[2 * static_cast<int64_t>(q) + 1] = g;
}

// Slice s = queries [1024 s, 1024 (s + 1)): thread t holds query 1024 s + t (0 past the end), pairwise
// tree t += t + d for d = 512 .. 1.  part[s][0 .. 6) the metric sums, ipart[s][0 .. 2) hits and g.
constexpr int kSlice = 1024;
__global__ __launch_bounds__(kSlice) void k_rank_slice(const double* __restrict__ met, const int64_t* __restrict__ cnt,
                                                       int64_t nq, double* __restrict__ part,
                                                       int64_t* __restrict__ ipart) {
  __shared__ double v[kSlice];
  __shared__ long long iv[kSlice];
  const int t = threadIdx.x;
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kSlice + t;
  for (int c = 0; c < MF_RANK_NMETRICS; ++c) {
    v[t] = q < nq ? met[q * MF_RANK_NMETRICS + c] : 0.0;
    __syncthreads();
    for (int d = kSlice / 2; d >= 1; d >>= 1) {
      if (t < d) v[t] = v[t] + v[t + d];
      __syncthreads();
    }
    if (t == 0) part[static_cast<int64_t>(blockIdx.x) * MF_RANK_NMETRICS + c] = v[0];
    __syncthreads();
  }
  for (int c = 0; c < 2; ++c) {
    iv[t] = q < nq ? cnt[2 * q + c] : 0;
    __syncthreads();
    for (int d = kSlice / 2; d >= 1; d >>= 1) {
      if (t < d) iv[t] += iv[t + d];
      __syncthreads();
    }
    if (t == 0) ipart[static_cast<int64_t>(blockIdx.x) * 2 + c] = iv[0];
    __syncthreads();
  }
}

// sums[c] = part[0][c] + part[1][c] + ... in ascending slice order; isums likewise
__global__ void k_rank_total(const double* __restrict__ part, const int64_t* __restrict__ ipart, int64_t slices,
                             double* __restrict__ sums, int64_t* __restrict__ isums) {
  const int t = threadIdx.x;
  if (t < MF_RANK_NMETRICS) {
    double a = 0.0;
    for (int64_t s = 0; s < slices; ++s) a = a + part[s * MF_RANK_NMETRICS + t];
    sums[t] = a;
  } else if (t < MF_RANK_NMETRICS + 2) {
    int64_t a = 0;
    for (int64_t s = 0; s < slices; ++s) a += ipart[s * 2 + (t - MF_RANK_NMETRICS)];
    isums[t - MF_RANK_NMETRICS] = a;
  }
}

}  // namespace

int64_t rank_query_set(hipStream_t st, RankScratch& sc, const uint32_t* qrow, int64_t n, uint32_t rows, DevBuf& qrows) {
  MF_REQUIRE(n >= 0 && n < (int64_t{1} << 31) && rows < (1u << 31), "rank tables: too many pairs or rows");
  if (n == 0 || rows == 0) return 0;
  const int R = static_cast<int>(rows) + 1;
  sc.flag.alloc(static_cast<size_t>(R) * 4);
  sc.pos.alloc(static_cast<size_t>(R) * 4);
  MF_HIP(hipMemsetAsync(sc.flag.get(), 0, static_cast<size_t>(R) * 4, st));
  hipLaunchKernelGGL(k_rank_flags, dim3(grid_for(n)), dim3(kThreads), 0, st, qrow, n, rows, sc.flag.as<int32_t>());
  size_t tb = 0;
  MF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, sc.flag.as<int32_t>(), sc.pos.as<int32_t>(), R, st));
  MF_HIP(hipcub::DeviceScan::ExclusiveSum(temp_storage(st, sc.tmp, tb), tb, sc.flag.as<int32_t>(),
                                          sc.pos.as<int32_t>(), R, st));
  int32_t nq = 0;  // pos[rows]: the flags before the zero that ends the array
  MF_HIP(hipMemcpyAsync(&nq, sc.pos.as<int32_t>() + rows, 4, hipMemcpyDeviceToHost, st));
  MF_HIP(hipStreamSynchronize(st));
  qrows.alloc(static_cast<size_t>(std::max(nq, 1)) * 4);
  if (nq > 0)
    hipLaunchKernelGGL(k_rank_compact, dim3(grid_for(rows)), dim3(kThreads), 0, st, sc.flag.as<int32_t>(),
                       sc.pos.as<int32_t>(), rows, qrows.as<int32_t>());
  MF_HIP(hipGetLastError());
  return nq;
}

void rank_pair_csr(hipStream_t st, RankScratch& sc, const uint32_t* qrow, const uint32_t* cand, int64_t n, uint32_t rows,
                   int64_t nq, bool gt, DevBuf& off, DevBuf& ent) {
  MF_REQUIRE(n >= 0 && n < (int64_t{1} << 31) - 1, "rank tables: too many pairs");
  off.alloc(static_cast<size_t>(nq + 1) * 8);
  ent.alloc(static_cast<size_t>(std::max<int64_t>(n, 1)) * 4);
  if (n == 0 || nq == 0) {
    MF_HIP(hipMemsetAsync(off.get(), 0, static_cast<size_t>(nq + 1) * 8, st));
    return;
  }
  rank_keys_reserve(sc, n);
  hipLaunchKernelGGL(k_rank_keys, dim3(grid_for(n)), dim3(kThreads), 0, st, qrow, cand, n, rows, sc.flag.as<int32_t>(),
                     sc.pos.as<int32_t>(), nq, gt, sc.key.as<uint64_t>());
  rank_keys_sort(st, sc, n, nq);
  rank_keys_csr(st, sc, n, nq, gt, off.as<int64_t>(), ent.as<int32_t>());
}

void rank_keys_reserve(RankScratch& sc, int64_t n) {
  MF_REQUIRE(n >= 0 && n < (int64_t{1} << 31) - 1, "rank tables: too many pairs");
  sc.key.alloc(static_cast<size_t>(std::max<int64_t>(n, 1)) * 8);
  sc.key2.alloc(static_cast<size_t>(std::max<int64_t>(n, 1)) * 8);
  sc.head.alloc(static_cast<size_t>(n + 1) * 4);
  sc.wp.alloc(static_cast<size_t>(n + 1) * 4);
}

void rank_keys_sort(hipStream_t st, RankScratch& sc, int64_t n, int64_t nq) {
  const int N = static_cast<int>(n);
  const int end_bit = 32 + radix_bits_for(static_cast<uint64_t>(nq) + 1);  // positions 0 .. nq (nq: dropped)
  size_t tb = 0;
  MF_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, sc.key.as<uint64_t>(), sc.key2.as<uint64_t>(), N, 0, end_bit, st));
  MF_HIP(hipcub::DeviceRadixSort::SortKeys(temp_storage(st, sc.tmp, tb), tb, sc.key.as<uint64_t>(),
                                           sc.key2.as<uint64_t>(), N, 0, end_bit, st));
  hipLaunchKernelGGL(k_rank_heads, dim3(grid_for(n + 1)), dim3(kThreads), 0, st, sc.key2.as<uint64_t>(), n, nq,
                     sc.head.as<int32_t>());
  MF_HIP(hipGetLastError());
}

void rank_keys_csr(hipStream_t st, RankScratch& sc, int64_t n, int64_t nq, bool gt, int64_t* off, int32_t* ent) {
  const int N = static_cast<int>(n);
  size_t tb = 0;
  MF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, sc.head.as<int32_t>(), sc.wp.as<int32_t>(), N + 1, st));
  MF_HIP(hipcub::DeviceScan::ExclusiveSum(temp_storage(st, sc.tmp, tb), tb, sc.head.as<int32_t>(),
                                          sc.wp.as<int32_t>(), N + 1, st));
  hipLaunchKernelGGL(k_rank_entries, dim3(grid_for(n)), dim3(kThreads), 0, st, sc.key2.as<uint64_t>(),
                     sc.head.as<int32_t>(), sc.wp.as<int32_t>(), n, gt, ent);
  hipLaunchKernelGGL(k_rank_offsets, dim3(grid_for(nq + 1)), dim3(kThreads), 0, st, sc.key2.as<uint64_t>(),
                     sc.wp.as<int32_t>(), n, nq, off);
  MF_HIP(hipGetLastError());
}

void launch_rank_metrics(hipStream_t st, const int32_t* ids, const int32_t* counts, int nb, int top_n,
                         const int64_t* gt_off, const int32_t* gt_ent, const double* tab, double* met, int64_t* cnt) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_rank_metrics, dim3(static_cast<unsigned>((nb + 3) / 4)), dim3(256), 0, st, ids, counts, nb, top_n,
                     gt_off, gt_ent, tab, met, cnt);
}

int64_t rank_reduce_slices(int64_t nq) { return (nq + kSlice - 1) / kSlice; }

void launch_rank_reduce(hipStream_t st, const double* met, const int64_t* cnt, int64_t nq, double* part, int64_t* ipart,
                        double* sums, int64_t* isums) {
  const int64_t slices = rank_reduce_slices(nq);
  if (slices > 0)
    hipLaunchKernelGGL(k_rank_slice, dim3(static_cast<unsigned>(slices)), dim3(kSlice), 0, st, met, cnt, nq, part, ipart);
  hipLaunchKernelGGL(k_rank_total, dim3(1), dim3(64), 0, st, part, ipart, slices, sums, isums);
}

}  // namespace mfhip
