// kernels_pairrank.hip -- the position of given (query, candidate) pairs in the query's complete
// ranked list (mf_pair_ranks, mf_online_prequential), without building the list: a pair's rank is
// the number of other candidates whose key beats the pair's key.
//
//  k_pr_target    one thread per pair: the two negative codes, the pair's own score (the chain
//                 mf_recommend's kernels compute for that row: f32 the fmaf chain over f ascending,
//                 which the f32-input MFMA reproduces bit for bit; f64 pq = pq + a * b, k_predict's
//                 value; this file is compiled with -ffp-contract=off), its key, the list length
//                 C - |exclusion row| and a zeroed count.
//  k_pr_f32       fast contexts: k_rec_f32's walk (candidates = A operand, one query column per pair
//                 = B operand, four 32 x 32 accumulator tiles per wave over tiles of 128 candidates,
//                 k in chunks of 16 through the double-buffered k-major LDS stage) with the selection
//                 replaced by a compare: every in-range accumulator whose key beats the lane's
//                 target adds 1.  cand_id is read only where the score parts are equal.
//  k_pr_f64       deterministic contexts: plain VALU as k_rec_f64, lane = candidate, kQW pairs per wave.
//  k_pr_excl      exclusions by subtraction: the walks count EVERY candidate row; one wave per pair then
//                 scores the query's excluded rows with the same chain and takes those that beat the
//                 target off the count.  That is nnz(exclusion row) dot products per pair instead of
//                 a binary search per counted candidate (most of the catalogue for a badly ranked
//                 pair), and the walk needs no exclusion table at all.
//  k_pr_metrics   per pair ndcg / rr / pr and (hit, evaluated) in the row layout k_rank_slice /
//                 k_rank_total (kernels_rank.hip) sum in their fixed order.
//
// Counts are integers: the halves of a wave, the candidate splits and the subtraction combine with
// integer atomics, so a rank depends on no order, batch size or split.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "csr_search.hpp"
#include "kernels.hpp"
#include "mfhip.h"

namespace mfhip {
namespace {

// ---- keys: kernels_recommend.hip's order, restated ------------------------------------------
// Candidate id part: a smaller id gives a larger value.
__device__ __forceinline__ uint32_t id_bits(int32_t id) { return ~(static_cast<uint32_t>(id) ^ 0x80000000u); }
// Order-preserving score parts: NaN = 1 (below every number), -0 orders as +0, 0 = no key.
__device__ __forceinline__ uint32_t ord32(float s) {
  if (s != s) return 1u;
  if (s == 0.0f) return 0x80000000u;
  const uint32_t b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint64_t ord64(double s) {
  if (s != s) return 1u;
  if (s == 0.0) return 0x8000000000000000ULL;
  const uint64_t b = static_cast<uint64_t>(__double_as_longlong(s));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
// The score mf_recommend reports for a key (NaN canonical, -0 as +0).
__device__ __forceinline__ double score_of(uint32_t o) {
  if (o == 1u) return __longlong_as_double(0x7ff8000000000000LL);
  const uint32_t b = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  return static_cast<double>(__uint_as_float(b));
}
__device__ __forceinline__ double score_of(uint64_t o) {
  if (o == 1u) return __longlong_as_double(0x7ff8000000000000LL);
  const uint64_t b = (o >> 63) ? (o ^ 0x8000000000000000ULL) : ~o;
  return __longlong_as_double(static_cast<long long>(b));
}
// Does (score part a, id part ai) beat (b, bi)?
template <typename O>
__device__ __forceinline__ bool beats(O a, uint32_t ai, O b, uint32_t bi) { return a > b || (a == b && ai > bi); }

// Is candidate row `crow` in the sorted rows [b, e)?
__device__ __forceinline__ bool excluded(const int32_t* __restrict__ rows, int64_t b, int64_t e, int32_t crow) {
  return dev::contains(rows, b, e, crow);
}

// The pair's score part: the chain over f = 0 .. k-1 from 0.
__device__ __forceinline__ uint32_t chain_ord(const float* __restrict__ q, const float* __restrict__ c, int k) {
  float s = 0.f;
  if ((k & 3) == 0) {  // rows are 16-byte aligned: four elements per load, the same order of fmaf
    for (int f = 0; f < k; f += 4) {
      const float4 a = *reinterpret_cast<const float4*>(c + f), b = *reinterpret_cast<const float4*>(q + f);
      s = fmaf(a.x, b.x, s);
      s = fmaf(a.y, b.y, s);
      s = fmaf(a.z, b.z, s);
      s = fmaf(a.w, b.w, s);
    }
  } else {
    for (int f = 0; f < k; ++f) s = fmaf(c[f], q[f], s);
  }
  return ord32(s);
}
__device__ __forceinline__ uint64_t chain_ord(const double* __restrict__ q, const double* __restrict__ c, int k) {
  double s = 0.0;
  for (int f = 0; f < k; ++f) s = s + q[f] * c[f];
  return ord64(s);
}

template <typename T>
struct OrdOf;
template <>
struct OrdOf<float> { using type = uint32_t; };
template <>
struct OrdOf<double> { using type = uint64_t; };

// ---- targets ------------------------------------------------------------------------------
// qrow / crow: the pair's factor rows (kRowMiss: unknown id); qpos (rows + 1 entries): a known query
// row's position in the exclusion CSR eoff / erows.  tord == 0 marks a pair that is not ranked.
template <typename T>
__global__ __launch_bounds__(256) void k_pr_target(const T* __restrict__ Qf, const T* __restrict__ Cf,
                                                   const uint32_t* __restrict__ qrow, const uint32_t* __restrict__ crow,
                                                   int64_t n, int32_t C, int k, const int32_t* __restrict__ cand_id,
                                                   const int32_t* __restrict__ qpos, const int64_t* __restrict__ eoff,
                                                   const int32_t* __restrict__ erows,
                                                   typename OrdOf<T>::type* __restrict__ tord, uint32_t* __restrict__ tid,
                                                   int32_t* __restrict__ rank, int32_t* __restrict__ valid,
                                                   double* __restrict__ score) {
  using O = typename OrdOf<T>::type;
  const int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (j >= n) return;
  const uint32_t qr = qrow[j], cr = crow[j];
  O o = 0;
  uint32_t idp = 0;
  int32_t code = MF_PAIR_RANK_COLD, v = 0;
  if (qr != kRowMiss && cr != kRowMiss) {
    const int32_t p = qpos[qr];
    const int64_t b = eoff[p], e = eoff[p + 1];
    if (excluded(erows, b, e, static_cast<int32_t>(cr))) {
      code = MF_PAIR_RANK_EXCLUDED;
    } else {
      code = 0;
      v = C - static_cast<int32_t>(e - b);
      o = chain_ord(Qf + static_cast<int64_t>(qr) * k, Cf + static_cast<int64_t>(cr) * k, k);
      idp = id_bits(cand_id[cr]);
    }
  }
  tord[j] = o;
  tid[j] = idp;
  rank[j] = code;
  valid[j] = v;
  score[j] = code == 0 ? score_of(o) : 0.0;
}

// ---- f32: MFMA score + count ------------------------------------------------------------------
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kCT = 128;   // candidate rows per tile (4 accumulator tiles of 32)
constexpr int kKC = 16;    // k chunk staged per step
constexpr int kAStr = 160; // LDS row stride of the candidate stage (k-major): 160 = 32 mod 64 banks

__host__ __device__ constexpr int pr_bstr(int nw) { return nw * 32 + ((nw * 32) % 64 == 0 ? 32 : 0); }
__host__ __device__ constexpr int pr_stage_floats(int nw) { return kKC * (kAStr + pr_bstr(nw)); }

// Grid: (pair tiles of NW * 32, S).  Pairs [0, n) of the batch: qrow their query rows, tord / tid their
// target keys (tord == 0: not ranked, the column is fed zeros and counts nothing).  Candidates: rows
// [0, C) of slab Cf, split s takes [s * per, min(C, (s + 1) * per)).  VEC: k % 4 == 0.
template <int NW, bool VEC>
__global__ __launch_bounds__(NW * 64) void k_pr_f32(const float* __restrict__ Qf, const float* __restrict__ Cf,
                                                    const uint32_t* __restrict__ qrow, int n, int32_t C, int32_t per,
                                                    int k, const int32_t* __restrict__ cand_id,
                                                    const uint32_t* __restrict__ tord, const uint32_t* __restrict__ tid,
                                                    int32_t* __restrict__ rank) {
  constexpr int NT = NW * 64, QT = NW * 32, BSTR = pr_bstr(NW);
  constexpr int A_PER = kCT * 4 / NT;  // float4 slots of the candidate stage per thread
  constexpr int B_PER = QT * 4 / NT;   // ... of the query stage (= 2)
  __shared__ __align__(16) float stage[2 * pr_stage_floats(NW)];  // [2][kKC][kAStr + BSTR]
  const int tid_ = threadIdx.x, lane = tid_ & 63, wave = tid_ >> 6;
  const int q0 = blockIdx.x * QT, s = blockIdx.y;
  const int32_t cbeg = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(s) * per));
  const int32_t cend = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(cbeg) + per));

  // this thread's share of the query stage: row x / 4 of the tile, floats 4 * (x % 4) .. + 3 of a chunk
  const float* bsrc[B_PER];
#pragma unroll
  for (int i = 0; i < B_PER; ++i) {
    const int q = q0 + (tid_ + i * NT) / 4;
    bsrc[i] = (q < n && tord[q] != 0) ? Qf + static_cast<int64_t>(qrow[q]) * k : nullptr;
  }
  float4 ra[A_PER], rb[B_PER];
  auto load4 = [&](const float* row, int f) -> float4 {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row == nullptr) return v;
    if (VEC) {
      if (f < k) v = *reinterpret_cast<const float4*>(row + f);
    } else {
      if (f < k) v.x = row[f];
      if (f + 1 < k) v.y = row[f + 1];
      if (f + 2 < k) v.z = row[f + 2];
      if (f + 3 < k) v.w = row[f + 3];
    }
    return v;
  };
  auto fetch = [&](int32_t c0, int f0) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int x = tid_ + i * NT;
      const int32_t cr = c0 + x / 4;
      ra[i] = load4(cr < cend ? Cf + static_cast<int64_t>(cr) * k : nullptr, f0 + 4 * (x & 3));
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) rb[i] = load4(bsrc[i], f0 + 4 * ((tid_ + i * NT) & 3));
  };
  auto put = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int x = tid_ + i * NT, row = x / 4, kf = 4 * (x & 3);
      buf[(kf + 0) * kAStr + row] = ra[i].x;
      buf[(kf + 1) * kAStr + row] = ra[i].y;
      buf[(kf + 2) * kAStr + row] = ra[i].z;
      buf[(kf + 3) * kAStr + row] = ra[i].w;
    }
    float* bb = buf + kKC * kAStr;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int x = tid_ + i * NT, row = x / 4, kf = 4 * (x & 3);
      bb[(kf + 0) * BSTR + row] = rb[i].x;
      bb[(kf + 1) * BSTR + row] = rb[i].y;
      bb[(kf + 2) * BSTR + row] = rb[i].z;
      bb[(kf + 3) * BSTR + row] = rb[i].w;
    }
  };

  const int nkc = (k + kKC - 1) / kKC;
  const int ntile = (cend - cbeg + kCT - 1) / kCT;
  const int total = ntile * nkc;
  // the lane's pair: column lane & 31 of its wave's 32; half h takes candidate rows 4h + ...
  const int jq = wave * 32 + (lane & 31), h = lane >> 5;
  const int qme = q0 + jq;
  uint32_t thi = 0, tlo = 0;
  if (qme < n) { thi = tord[qme]; tlo = tid[qme]; }
  const bool act = thi != 0;
  int cnt = 0;

  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  if (total > 0) {
    fetch(cbeg, 0);
    put(stage);
  }
  __syncthreads();
  int tile = 0, kc = 0;
  for (int it = 0; it < total; ++it) {
    const float* cur = stage + (it & 1) * pr_stage_floats(NW);
    int ntile_i = tile, nkc_i = kc + 1;
    if (nkc_i == nkc) { nkc_i = 0; ++ntile_i; }
    if (it + 1 < total) fetch(cbeg + ntile_i * kCT, nkc_i * kKC);
    const float* ca = cur + h * kAStr + (lane & 31);
    const float* cb = cur + kKC * kAStr + h * BSTR + jq;
#pragma unroll
    for (int kk = 0; kk < kKC / 2; ++kk) {
      const float b = cb[2 * kk * BSTR];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[2 * kk * kAStr + 32 * t], b, acc[t], 0, 0, 0);
    }
    if (kc == nkc - 1) {
      // count: register r of accumulator tile t is candidate row c0 + 32 t + (r & 3) + 8 (r >> 2) + 4 h
      const int32_t c0 = cbeg + tile * kCT;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int32_t cr = c0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
          const uint32_t o = ord32(acc[t][r]);
          if (act && cr < cend) {
            if (o > thi) ++cnt;
            else if (o == thi && id_bits(cand_id[cr]) > tlo) ++cnt;
          }
          acc[t][r] = 0.f;
        }
      }
    }
    if (it + 1 < total) put(stage + ((it + 1) & 1) * pr_stage_floats(NW));
    __syncthreads();
    tile = ntile_i;
    kc = nkc_i;
  }
  // the two halves of the wave hold the same pair
  cnt += __shfl_xor(cnt, 32);
  if (act && h == 0 && cnt != 0) atomicAdd(rank + qme, cnt);
}

// ---- f64: VALU score + count ------------------------------------------------------------------
constexpr int kQW = 4;  // pairs per wave

// Grid: (ceil(n / (4 * kQW)), S), 4 waves per block.  Lane = candidate; the wave's kQW query rows are
// wave-uniform reads (row 0 stands in for a pair that is not ranked: Q has a row wherever a pair is).
__global__ __launch_bounds__(256) void k_pr_f64(const double* __restrict__ Qf, const double* __restrict__ Cf,
                                                const uint32_t* __restrict__ qrow, int n, int32_t C, int32_t per, int k,
                                                const int32_t* __restrict__ cand_id, const uint64_t* __restrict__ tord,
                                                const uint32_t* __restrict__ tid, int32_t* __restrict__ rank) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int q0 = (blockIdx.x * 4 + wave) * kQW;
  if (q0 >= n) return;  // wave-uniform
  const int32_t cbeg = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(s) * per));
  const int32_t cend = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(cbeg) + per));
  const double* qp[kQW];
  uint64_t thi[kQW];
  uint32_t tlo[kQW];
  int cnt[kQW];
#pragma unroll
  for (int i = 0; i < kQW; ++i) {
    const int q = q0 + i;
    thi[i] = q < n ? tord[q] : 0;
    tlo[i] = q < n ? tid[q] : 0;
    qp[i] = Qf + (thi[i] != 0 ? static_cast<int64_t>(qrow[q]) * k : 0);
    cnt[i] = 0;
  }
  for (int32_t c0 = cbeg; c0 < cend; c0 += 64) {
    const int32_t cr = c0 + lane;
    const bool cok = cr < cend;
    const double* cp = Cf + static_cast<int64_t>(cok ? cr : cbeg) * k;
    double pq[kQW];
#pragma unroll
    for (int i = 0; i < kQW; ++i) pq[i] = 0.0;
    for (int f = 0; f < k; ++f) {
      const double c = cp[f];
#pragma unroll
      for (int i = 0; i < kQW; ++i) pq[i] = pq[i] + qp[i][f] * c;
    }
    const uint32_t cidp = id_bits(cok ? cand_id[cr] : 0);
#pragma unroll
    for (int i = 0; i < kQW; ++i) {
      const bool b = cok && thi[i] != 0 && beats(ord64(pq[i]), cidp, thi[i], tlo[i]);
      cnt[i] += __popcll(__ballot(b));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kQW; ++i)
      if (thi[i] != 0 && cnt[i] != 0) atomicAdd(rank + q0 + i, cnt[i]);
  }
}

// ---- exclusions: subtract -----------------------------------------------------------------
// One wave per pair (4 per block), after the walk of the pair's batch: lane l scores excluded rows l,
// l + 64, ... of the pair's query.  The pair's own row is never among them (the pair would carry
// MF_PAIR_RANK_EXCLUDED).
template <typename T>
__global__ __launch_bounds__(256) void k_pr_excl(const T* __restrict__ Qf, const T* __restrict__ Cf,
                                                 const uint32_t* __restrict__ qrow, int n, int k,
                                                 const int32_t* __restrict__ cand_id, const int32_t* __restrict__ qpos,
                                                 const int64_t* __restrict__ eoff, const int32_t* __restrict__ erows,
                                                 const typename OrdOf<T>::type* __restrict__ tord,
                                                 const uint32_t* __restrict__ tid, int32_t* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;  // wave-uniform
  const auto thi = tord[j];
  if (thi == 0) return;
  const uint32_t tlo = tid[j];
  const uint32_t qr = qrow[j];
  const int32_t p = qpos[qr];
  const int64_t b = eoff[p], e = eoff[p + 1];
  const T* q = Qf + static_cast<int64_t>(qr) * k;
  int cnt = 0;
  for (int64_t x0 = b; x0 < e; x0 += 64) {
    const int64_t x = x0 + lane;
    bool beat = false;
    if (x < e) {
      const int32_t cr = erows[x];
      beat = beats(chain_ord(q, Cf + static_cast<int64_t>(cr) * k, k), id_bits(cand_id[cr]), thi, tlo);
    }
    cnt += __popcll(__ballot(beat));
  }
  if (lane == 0 && cnt != 0) rank[j] -= cnt;
}

// ---- metrics ------------------------------------------------------------------------------
// met[j][MF_RANK_NMETRICS] = ndcg, rr, pr, 0, 0, 0 and cnt[j][2] = (hit, evaluated): the rows k_rank_slice sums.
// tab: 128 gains, then idcg[0 .. 128] (the table of mf_rank_eval).
__global__ __launch_bounds__(256) void k_pr_metrics(const int32_t* __restrict__ rank, const int32_t* __restrict__ valid,
                                                    int64_t n, int N, const double* __restrict__ tab,
                                                    double* __restrict__ met, int64_t* __restrict__ cnt) {
  const int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (j >= n) return;
  const int32_t r = rank[j], V = valid[j];
  const bool ev = r >= 0, hit = ev && r < N;
  double* o = met + j * MF_RANK_NMETRICS;
  o[0] = hit ? tab[r] / tab[MF_RECOMMEND_MAX_TOP + 1] : 0.0;
  o[1] = hit ? 1.0 / static_cast<double>(r + 1) : 0.0;
  o[2] = (ev && V > 1) ? static_cast<double>(r) / static_cast<double>(V - 1) : 0.0;
  o[3] = o[4] = o[5] = 0.0;
  cnt[2 * j] = hit ? 1 : 0;
  cnt[2 * j + 1] = ev ? 1 : 0;
}

template <int NW>
void pr_f32_dispatch(hipStream_t st, const float* Q, const float* Cf, const uint32_t* qrow, int n, int32_t C, int S,
                     int32_t per, int k, const int32_t* cand_id, const uint32_t* tord, const uint32_t* tid,
                     int32_t* rank) {
  const dim3 grid(static_cast<unsigned>((n + NW * 32 - 1) / (NW * 32)), static_cast<unsigned>(S)), block(NW * 64);
  if (k % 4 == 0)
    hipLaunchKernelGGL((k_pr_f32<NW, true>), grid, block, 0, st, Q, Cf, qrow, n, C, per, k, cand_id, tord, tid, rank);
  else
    hipLaunchKernelGGL((k_pr_f32<NW, false>), grid, block, 0, st, Q, Cf, qrow, n, C, per, k, cand_id, tord, tid, rank);
}

}  // namespace

size_t pair_rank_ord_bytes(bool f64) { return f64 ? 8 : 4; }

int pair_rank_tile(bool f64, int nw) { return f64 ? 4 * kQW : 32 * nw; }

void launch_pair_targets(hipStream_t st, const void* Q, const void* Cf, const uint32_t* qrow, const uint32_t* crow,
                         int64_t n, int32_t C, int k, bool f64, const int32_t* cand_id, const int32_t* qpos,
                         const int64_t* excl_off, const int32_t* excl_rows, void* tord, uint32_t* tid, int32_t* rank,
                         int32_t* valid, double* score) {
  if (n <= 0) return;
  const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
  if (f64)
    hipLaunchKernelGGL((k_pr_target<double>), grid, block, 0, st, static_cast<const double*>(Q),
                       static_cast<const double*>(Cf), qrow, crow, n, C, k, cand_id, qpos, excl_off, excl_rows,
                       static_cast<uint64_t*>(tord), tid, rank, valid, score);
  else
    hipLaunchKernelGGL((k_pr_target<float>), grid, block, 0, st, static_cast<const float*>(Q),
                       static_cast<const float*>(Cf), qrow, crow, n, C, k, cand_id, qpos, excl_off, excl_rows,
                       static_cast<uint32_t*>(tord), tid, rank, valid, score);
}

void launch_pair_count(hipStream_t st, const void* Q, const void* Cf, const uint32_t* qrow, int n, int32_t C, int S,
                       int k, bool f64, int nw, const int32_t* cand_id, const int32_t* qpos, const int64_t* excl_off,
                       const int32_t* excl_rows, bool have_excl, const void* tord, const uint32_t* tid, int32_t* rank) {
  if (n <= 0 || C <= 0) return;
  const int32_t per = (C + S - 1) / S;
  const dim3 egrid(static_cast<unsigned>((n + 3) / 4)), eblock(256);
  if (f64) {
    const dim3 grid(static_cast<unsigned>((n + 4 * kQW - 1) / (4 * kQW)), static_cast<unsigned>(S)), block(256);
    hipLaunchKernelGGL(k_pr_f64, grid, block, 0, st, static_cast<const double*>(Q), static_cast<const double*>(Cf), qrow,
                       n, C, per, k, cand_id, static_cast<const uint64_t*>(tord), tid, rank);
    if (have_excl)
      hipLaunchKernelGGL((k_pr_excl<double>), egrid, eblock, 0, st, static_cast<const double*>(Q),
                         static_cast<const double*>(Cf), qrow, n, k, cand_id, qpos, excl_off, excl_rows,
                         static_cast<const uint64_t*>(tord), tid, rank);
  } else {
    const float* q = static_cast<const float*>(Q);
    const float* c = static_cast<const float*>(Cf);
    const uint32_t* to = static_cast<const uint32_t*>(tord);
    if (nw >= 4) pr_f32_dispatch<4>(st, q, c, qrow, n, C, S, per, k, cand_id, to, tid, rank);
    else if (nw >= 2) pr_f32_dispatch<2>(st, q, c, qrow, n, C, S, per, k, cand_id, to, tid, rank);
    else pr_f32_dispatch<1>(st, q, c, qrow, n, C, S, per, k, cand_id, to, tid, rank);
    if (have_excl)
      hipLaunchKernelGGL((k_pr_excl<float>), egrid, eblock, 0, st, q, c, qrow, n, k, cand_id, qpos, excl_off, excl_rows,
                         to, tid, rank);
  }
}

void launch_pair_metrics(hipStream_t st, const int32_t* rank, const int32_t* valid, int64_t n, int top_n,
                         const double* tab, double* met, int64_t* cnt) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pr_metrics, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, rank, valid, n, top_n,
                     tab, met, cnt);
}

}  // namespace mfhip
