// kernels_among.hip -- mf_recommend_among: the top N within caller-given candidate lists.
//
//  k_among_heads, k_among_compact   the shared list as resolved and sorted -> its distinct held rows, ascending.
//  k_among_gather  the shared list.  Those factor rows are copied into a compact slab
//                  with their ids beside them; launch_recommend (kernels_recommend.hip) then runs over that slab
//                  with the row list as its position -> row map, so the cost follows the list, not the catalogue.
//  k_among_score   per-query lists.  One query per list: the matrix cores have nothing to amortise, the work is
//                  a gather.  A task is one part of one list (the host cuts every list into parts of whole
//                  64-entry groups, at most 64 parts per list); a wave takes a task, four tasks share a
//                  workgroup, and the waves of a workgroup never wait for each other.  Lane = candidate: the
//                  wave's 64 gathered rows move through LDS in chunks of 128 bytes per row, so that every load
//                  instruction reads whole cache lines (a lane walking its own row would touch 64 lines per
//                  load), 16 bytes per lane where the rank allows, all of a chunk's loads in flight at once; the
//                  query's chunk sits beside them and is read wave-uniformly.  A candidate's chain over f stays
//                  in one lane and sequential -- f64: pq = pq + a * b (this file is compiled with
//                  -ffp-contract=off), f32: fmaf from 0 -- which is what makes the score mf_recommend's bits.
//                  An id the model does not hold is an idle lane.
//                  Selection is k_rec_f64's: the keys of rec_keys.hpp, tested against the query's exclusion
//                  rows only when they beat the list's N-th key; a key the list already holds is the same
//                  candidate named twice and is skipped (list_insert_distinct).
//  k_rec_merge     (rec_keys.hpp) the partial lists of a position's parts -> its final top N, with the part
//                  offsets pbeg: an id that two parts both kept counts once.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "csr_search.hpp"
#include "id_index.hpp"
#include "kernels.hpp"
#include "mfhip.h"
#include "rec_keys.hpp"

namespace mfhip {
namespace {

using namespace dev;

constexpr int kAmongWaves = 4;  // tasks per workgroup

template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> { using type = Key32; };
template <>
struct KeyOf<double> { using type = Key64; };

// dst row p = src row rows[p], ids[p] = row_id[rows[p]]; one thread per element, rows < 2^31 / k is not assumed.
template <typename T>
__global__ __launch_bounds__(kGridThreads) void k_among_gather(const T* __restrict__ src,
                                                               const int32_t* __restrict__ rows, int64_t n, int k,
                                                               const int32_t* __restrict__ row_id,
                                                               T* __restrict__ dst, int32_t* __restrict__ ids) {
  const int64_t total = n * k;
  for (int64_t x = static_cast<int64_t>(blockIdx.x) * kGridThreads + threadIdx.x; x < total;
       x += static_cast<int64_t>(gridDim.x) * kGridThreads) {
    const int64_t p = x / k;
    const int f = static_cast<int>(x - p * k);
    const int32_t r = rows[p];
    dst[x] = src[static_cast<int64_t>(r) * k + f];
    if (f == 0) ids[p] = row_id[r];
  }
}

// The shared list as resolved and sorted (kRowMiss last): head[p] = 1 where sorted[p] is a held row that differs
// from its predecessor; n + 1 entries, the last 0, so that the exclusive scan's entry n is the count.
__global__ __launch_bounds__(kGridThreads) void k_among_heads(const uint32_t* __restrict__ sorted, int64_t n,
                                                              int32_t* __restrict__ head) {
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kGridThreads + threadIdx.x; p <= n;
       p += static_cast<int64_t>(gridDim.x) * kGridThreads)
    head[p] = p < n && sorted[p] != kRowMiss && (p == 0 || sorted[p] != sorted[p - 1]) ? 1 : 0;
}
// ... and every head to its place wp[p]: the distinct held rows, ascending.
__global__ __launch_bounds__(kGridThreads) void k_among_compact(const uint32_t* __restrict__ sorted,
                                                                const int32_t* __restrict__ head,
                                                                const int32_t* __restrict__ wp, int64_t n,
                                                                int32_t* __restrict__ out) {
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kGridThreads + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * kGridThreads)
    if (head[p]) out[wp[p]] = static_cast<int32_t>(sorted[p]);
}

// V consecutive elements of a row, moved as one 16-byte access when V > 1.
template <typename T, int V>
using Pack = T __attribute__((ext_vector_type(V)));

// Grid: ceil(ntasks / kAmongWaves) workgroups of kAmongWaves waves.  crows: the batch's lists as resolved
// (factor rows of the candidate side, kRowMiss for an id it does not hold).  qrow / excl_beg / excl_end: per
// position of the batch its query row and exclusion range in excl_rows.  part: [ntasks][N] keys.
// VEC: a row is a whole number of 16-byte vectors (k % 4 == 0 in f32, k % 2 == 0 in f64).  A lane then moves 16
// bytes at a time: 8 lanes cover a row's 128-byte chunk, one load instruction 8 rows; the tile's row stride is
// 144 bytes, which keeps the vectors aligned and spreads the 16 lanes that a 16-byte LDS read serves together
// over all 64 banks.  Otherwise element by element, row stride odd in elements (k_row_inv_norm's tile).
template <typename T, bool VEC>
__global__ __launch_bounds__(kAmongWaves * 64) void k_among_score(
    const T* __restrict__ Qf, const T* __restrict__ Cf, const AmongTask* __restrict__ tasks, int64_t ntasks,
    const uint32_t* __restrict__ crows, const int32_t* __restrict__ qrow, const int32_t* __restrict__ cand_id,
    const int64_t* __restrict__ excl_beg, const int64_t* __restrict__ excl_end, const int32_t* __restrict__ excl_rows,
    int k, int N, typename KeyOf<T>::type* __restrict__ part) {
  using K = typename KeyOf<T>::type;
  constexpr int KC = 128 / sizeof(T);                  // elements of a row per chunk: one cache line
  constexpr int V = VEC ? 16 / sizeof(T) : 1;          // elements per access
  constexpr int LPR = KC / V;                          // lanes that cover a row's chunk = accesses per lane and chunk
  constexpr int STR = VEC ? 144 / sizeof(T) : KC + 1;  // row stride of the tile in elements
  using P = Pack<T, V>;
  __shared__ __align__(16) T tile[kAmongWaves][64][STR];
  __shared__ __align__(16) T qs[kAmongWaves][KC];
  __shared__ K lists[kAmongWaves][MF_RECOMMEND_MAX_TOP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kAmongWaves + wave;
  if (t >= ntasks) return;  // (no workgroup barrier below)
  const AmongTask tk = tasks[t];
  K* list = lists[wave];
  for (int x = lane; x < N; x += 64) list[x] = K{};
  const T* qp = Qf + static_cast<int64_t>(qrow[tk.pos]) * k;
  const int64_t eb = excl_beg[tk.pos], ee = excl_end[tk.pos];
  wave_lds_sync();
  for (int32_t g0 = 0; g0 < tk.len; g0 += 64) {  // tk.len is wave-uniform
    const uint32_t myrow = g0 + lane < tk.len ? crows[tk.beg + g0 + lane] : kRowMiss;
    T pq = 0;
    for (int f0 = 0; f0 < k; f0 += KC) {
      const int kc = min(KC, k - f0);  // a multiple of V
      P ld[LPR];
#pragma unroll
      for (int i = 0; i < LPR; ++i) {
        const int e = i * 64 + lane, c = (e % LPR) * V;
        const uint32_t row = __shfl(myrow, e / LPR);
        ld[i] = (row != kRowMiss && c < kc) ? *reinterpret_cast<const P*>(Cf + static_cast<int64_t>(row) * k + f0 + c)
                                            : P(T(0));
      }
      const T qv = lane < kc ? qp[f0 + lane] : T(0);
      wave_lds_sync();  // the previous chunk has been read
#pragma unroll
      for (int i = 0; i < LPR; ++i) {
        const int e = i * 64 + lane;
        *reinterpret_cast<P*>(&tile[wave][e / LPR][(e % LPR) * V]) = ld[i];
      }
      if (lane < KC) qs[wave][lane] = qv;
      wave_lds_sync();
      for (int c = 0; c < kc; c += V) {
        const P a = *reinterpret_cast<const P*>(&qs[wave][c]), b = *reinterpret_cast<const P*>(&tile[wave][lane][c]);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if constexpr (sizeof(T) == 4) pq = fmaf(a[v], b[v], pq);
          else pq = pq + a[v] * b[v];
        }
      }
    }
    const bool cok = myrow != kRowMiss;
    const K key = make_key(pq, cok ? cand_id[myrow] : 0);
    bool want = cok && key_gt(key, list[N - 1]);
    if (want) want = !contains(excl_rows, eb, ee, static_cast<int32_t>(myrow));
    wave_list_insert<true>(list, N, key, want, lane);
  }
  for (int x = lane; x < N; x += 64) part[t * N + x] = list[x];
}

}  // namespace

int64_t among_distinct_rows(hipStream_t st, RankScratch& sc, const uint32_t* rows, int64_t n, int32_t* out) {
  if (n <= 0) return 0;
  uint32_t* const sorted = static_cast<uint32_t*>(temp_storage(st, sc.key2, static_cast<size_t>(n) * 4));
  int32_t* const pos = static_cast<int32_t*>(temp_storage(st, sc.pos, static_cast<size_t>(n) * 4));
  int32_t* const head = static_cast<int32_t*>(temp_storage(st, sc.head, static_cast<size_t>(n + 1) * 4));
  int32_t* const wp = static_cast<int32_t*>(temp_storage(st, sc.wp, static_cast<size_t>(n + 1) * 4));
  sort_positions<uint32_t>(st, sc.tmp, sc.flag, rows, sorted, pos, n, 32);  // all 32 bits: kRowMiss sorts last
  hipLaunchKernelGGL(k_among_heads, dim3(grid_for(n + 1)), dim3(kGridThreads), 0, st, sorted, n, head);
  scan_exclusive<int32_t>(st, sc.tmp, head, wp, n + 1);
  hipLaunchKernelGGL(k_among_compact, dim3(grid_for(n)), dim3(kGridThreads), 0, st, sorted, head, wp, n, out);
  MF_HIP(hipGetLastError());
  int32_t cnt = 0;
  MF_HIP(hipMemcpyAsync(&cnt, wp + n, 4, hipMemcpyDeviceToHost, st));
  MF_HIP(hipStreamSynchronize(st));
  return cnt;
}

void launch_among_gather(hipStream_t st, const void* src, const int32_t* rows, int64_t n, int k, bool f64,
                         const int32_t* row_id, void* dst, int32_t* ids) {
  if (n <= 0) return;
  const dim3 grid(grid_for(n * k)), block(kGridThreads);
  if (f64)
    hipLaunchKernelGGL((k_among_gather<double>), grid, block, 0, st, static_cast<const double*>(src), rows, n, k,
                       row_id, static_cast<double*>(dst), ids);
  else
    hipLaunchKernelGGL((k_among_gather<float>), grid, block, 0, st, static_cast<const float*>(src), rows, n, k, row_id,
                       static_cast<float*>(dst), ids);
}

void launch_among(hipStream_t st, const void* Q, const void* Cf, const AmongTask* tasks, int64_t ntasks,
                  const int64_t* pbeg, int nq, const uint32_t* crows, const int32_t* qrow, const int32_t* cand_id,
                  const int64_t* excl_beg, const int64_t* excl_end, const int32_t* excl_rows, int k, int top_n, bool f64,
                  void* part, int32_t* ids, double* scores, int32_t* counts) {
  if (nq <= 0) return;
  const dim3 mgrid(static_cast<unsigned>((nq + 3) / 4)), mblock(256);
  const dim3 grid(static_cast<unsigned>((ntasks + kAmongWaves - 1) / kAmongWaves)), block(kAmongWaves * 64);
  auto score = [&](auto t, auto vec) {
    using T = decltype(t);
    using K = typename KeyOf<T>::type;
    if (ntasks > 0)
      hipLaunchKernelGGL((k_among_score<T, decltype(vec)::value>), grid, block, 0, st, static_cast<const T*>(Q),
                         static_cast<const T*>(Cf), tasks, ntasks, crows, qrow, cand_id, excl_beg, excl_end, excl_rows,
                         k, top_n, static_cast<K*>(part));
    hipLaunchKernelGGL((k_rec_merge<K>), mgrid, mblock, 0, st, static_cast<const K*>(part), pbeg, nq, 0, top_n, ids,
                       scores, counts);
  };
  // whole 16-byte vectors per row?
  if (f64) k % 2 == 0 ? score(double(), std::true_type()) : score(double(), std::false_type());
  else k % 4 == 0 ? score(float(), std::true_type()) : score(float(), std::false_type());
}

}  // namespace mfhip
