// kernels_recommend.hip -- top-N recommendation (mf_recommend): score every candidate row against
// a batch of query rows and keep each query's N best, without materialising the score matrix.
//
//  k_rec_f32    fast contexts.  The dense product runs on the matrix cores (v_mfma_f32_32x32x2_f32):
//               candidates are the A operand, queries the B operand, so a lane's 16 accumulator
//               registers hold 16 candidates' scores of ONE query (column = lane & 31) and the
//               selection needs no cross-lane traffic.  A block of NW waves owns NW * 32 queries
//               (32 per wave) and walks its split of the candidate rows in tiles of 128: four
//               independent 32 x 32 accumulator tiles per wave, each taking the whole k loop in
//               ascending f (the f32-input MFMA is bit for bit the fmaf chain over f, so a score
//               depends on no tiling, split or batch size).  Both operands are staged through LDS in
//               k chunks of 16, double-buffered, stored k-major so that the fragment reads of a wave
//               fall on 64 distinct banks.
//  k_rec_f64    deterministic contexts.  Plain VALU: a lane owns one candidate's chain
//               pq = pq + a * b over f = 0..k-1 (this file is compiled with -ffp-contract=off), the
//               value k_predict gives for the pair, against QW query rows of its wave.
//  k_rec_merge  (rec_keys.hpp) the S partial lists of a query (one per candidate split) -> its final top N.
//  k_row_inv_norm  one inverse norm per row, 1 / sqrt(sum x_f^2), for the cosine metric (mf_similar,
//               mf_recommend_vectors).  Both score kernels take the metric as a template parameter COS:
//               with it, a score is dot * (inv(query) * inv(candidate)) before it meets the selection,
//               so thresholds, parked values, keys and the merge all carry the scaled score; without it
//               they are the kernels mf_recommend always ran, instruction for instruction.
//
// Selection (shared): a query's list is N keys in LDS, sorted descending; a key orders by score
// descending, then candidate id ascending, NaN below every number -- one unsigned compare.  A score
// is tested against the exclusion rows of its query (CSR, sorted candidate rows, binary search) only
// when it beats the list's N-th key, so insertions become rare after the first tiles.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "common.hpp"
#include "csr_search.hpp"
#include "kernels.hpp"
#include "mfhip.h"
#include "rec_keys.hpp"

namespace mfhip {
namespace {

using namespace dev;  // the keys and list_insert: rec_keys.hpp

// ---- f32: MFMA score + select -----------------------------------------------------------------
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kCT = 128;   // candidate rows per tile (4 accumulator tiles of 32)
constexpr int kKC = 16;    // k chunk staged per step
constexpr int kPend = 8;   // parked candidates per lane between two drains of the selection
constexpr int kAStr = 160; // LDS row stride of the candidate stage (k-major): 160 = 32 mod 64 banks

__host__ __device__ constexpr int rec_bstr(int nw) { return nw * 32 + ((nw * 32) % 64 == 0 ? 32 : 0); }
__host__ __device__ constexpr int rec_stage_floats(int nw) { return kKC * (kAStr + rec_bstr(nw)); }

// Grid: (query tiles, S).  qrows: the batch's query rows (all valid), nq of them.  Candidates:
// rows [0, C) of slab Cf, split s takes [s * per, min(C, (s + 1) * per)).  part: [nq][S][N] keys.
// VEC: k % 4 == 0, rows are loaded as float4.  COS: scores are scaled by qinv[query row] * cinv[candidate
// row]; a tile's 128 candidate inverses ride through LDS with it, one buffer per tile parity (a wave may
// stage tile T + 1 while another still selects from tile T).  MAP (mf_recommend_among's shared list): the
// candidates are a gathered slab, and the exclusion rows name factor rows: position p of the slab is factor row
// pos_row[p], read only for a score that has beaten the N-th key and is about to be tested.
template <int NW, bool VEC, bool COS, bool MAP>
__global__ __launch_bounds__(NW * 64) void k_rec_f32(const float* __restrict__ Qf, const float* __restrict__ Cf,
                                                     const int32_t* __restrict__ qrows, int nq, int32_t C, int32_t per,
                                                     int k, int N, const int32_t* __restrict__ cand_id,
                                                     const int64_t* __restrict__ excl_beg,
                                                     const int64_t* __restrict__ excl_end,
                                                     const int32_t* __restrict__ excl_rows, Key32* __restrict__ part,
                                                     const float* __restrict__ qinv,
                                                     const float* __restrict__ cinv,
                                                     const int32_t* __restrict__ pos_row) {
  constexpr int NT = NW * 64, QT = NW * 32, BSTR = rec_bstr(NW);
  constexpr int CI_PER = (kCT + NT - 1) / NT;  // candidate inverses of a tile per thread (COS)
  constexpr int A_PER = kCT * 4 / NT;  // float4 slots of the candidate stage per thread
  constexpr int B_PER = QT * 4 / NT;   // ... of the query stage (= 2)
  extern __shared__ __align__(16) unsigned char rec_smem[];
  Key32* lists = reinterpret_cast<Key32*>(rec_smem);                         // [QT][N]
  uint64_t* pend = reinterpret_cast<uint64_t*>(rec_smem + sizeof(Key32) * QT * N);  // [kPend][NT]
  float* stage = reinterpret_cast<float*>(pend + kPend * NT);                      // [2][kKC][kAStr + BSTR]
  float* cinv_s = stage + 2 * rec_stage_floats(NW);                                // [2][kCT], COS only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * QT, S = gridDim.y, s = blockIdx.y;
  const int32_t cbeg = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(s) * per));
  const int32_t cend = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(cbeg) + per));

  for (int x = tid; x < QT * N; x += NT) lists[x] = Key32{0};

  // this thread's share of the query stage: row x / 4 of the tile, floats 4 * (x % 4) .. + 3 of a chunk
  const float* bsrc[B_PER];
#pragma unroll
  for (int i = 0; i < B_PER; ++i) {
    const int q = q0 + (tid + i * NT) / 4;
    bsrc[i] = q < nq ? Qf + static_cast<int64_t>(qrows[q]) * k : nullptr;
  }
  float4 ra[A_PER], rb[B_PER];
  float rci[CI_PER];
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
      const int x = tid + i * NT;
      const int32_t crow = c0 + x / 4;
      ra[i] = load4(crow < cend ? Cf + static_cast<int64_t>(crow) * k : nullptr, f0 + 4 * (x & 3));
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) rb[i] = load4(bsrc[i], f0 + 4 * ((tid + i * NT) & 3));
    if constexpr (COS) {
      if (f0 == 0) {  // a new tile: its inverses
#pragma unroll
        for (int i = 0; i < CI_PER; ++i) {
          const int x = tid + i * NT;
          rci[i] = (x < kCT && c0 + x < cend) ? cinv[c0 + x] : 0.f;
        }
      }
    }
  };
  // ci: where a new tile's inverses go (null inside a tile)
  auto put = [&](float* buf, float* ci) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int x = tid + i * NT, row = x / 4, kf = 4 * (x & 3);
      buf[(kf + 0) * kAStr + row] = ra[i].x;
      buf[(kf + 1) * kAStr + row] = ra[i].y;
      buf[(kf + 2) * kAStr + row] = ra[i].z;
      buf[(kf + 3) * kAStr + row] = ra[i].w;
    }
    float* bb = buf + kKC * kAStr;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int x = tid + i * NT, row = x / 4, kf = 4 * (x & 3);
      bb[(kf + 0) * BSTR + row] = rb[i].x;
      bb[(kf + 1) * BSTR + row] = rb[i].y;
      bb[(kf + 2) * BSTR + row] = rb[i].z;
      bb[(kf + 3) * BSTR + row] = rb[i].w;
    }
    if constexpr (COS) {
      if (ci != nullptr) {
#pragma unroll
        for (int i = 0; i < CI_PER; ++i) {
          const int x = tid + i * NT;
          if (x < kCT) ci[x] = rci[i];
        }
      }
    }
  };

  const int nkc = (k + kKC - 1) / kKC;
  const int ntile = (cend - cbeg + kCT - 1) / kCT;
  const int total = ntile * nkc;
  // the lane's query: column lane & 31 of its wave's 32; half h takes candidate rows 4h + ...
  const int jq = wave * 32 + (lane & 31), h = lane >> 5;
  const int qme = q0 + jq;
  const bool qok = qme < nq;
  Key32* mylist = lists + jq * N;
  int64_t eb = 0, ee = 0;
  if (qok) { eb = excl_beg[qme]; ee = excl_end[qme]; }
  float qi = 0.f;
  if constexpr (COS) {
    if (qok) qi = qinv[qrows[qme]];
  }

  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  if (total > 0) {
    fetch(cbeg, 0);
    put(stage, cinv_s);
  }
  __syncthreads();
  int tile = 0, kc = 0;
  for (int it = 0; it < total; ++it) {
    const float* cur = stage + (it & 1) * rec_stage_floats(NW);
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
      // select: register r of accumulator tile t is candidate row c0 + 32 t + (r & 3) + 8 (r >> 2) + 4 h.
      // A score that reaches the list's N-th (as of the last drain) is parked in the lane's pending
      // slots; a drain then lets every lane insert its own parked candidates side by side, so the
      // wave pays one insertion round per parked candidate of its busiest lane, not one per score.
      const int32_t c0 = cbeg + tile * kCT;
      uint32_t thr_hi = static_cast<uint32_t>(mylist[N - 1].v >> 32);
      int cnt = 0;
      [[maybe_unused]] float4 ci4 = make_float4(0.f, 0.f, 0.f, 0.f);
      auto drain = [&]() {
        for (int i = 0; __any(i < cnt); ++i) {
          bool have = i < cnt;
          Key32 key{0};
          if (have) {
            const uint64_t pv = pend[i * NT + tid];
            const int32_t crow = c0 + static_cast<int32_t>(pv & 0xFFFFFFFFu);
            key = Key32{(pv & 0xFFFFFFFF00000000ULL) | id_bits(cand_id[crow])};
            if constexpr (MAP)
              have = key_gt(key, mylist[N - 1]) && !contains(excl_rows, eb, ee, pos_row[crow]);
            else
              have = key_gt(key, mylist[N - 1]) && !contains(excl_rows, eb, ee, crow);
          }
          // the two halves of the wave share a query's list: one half at a time
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            if (have && h == hh && key_gt(key, mylist[N - 1])) list_insert(mylist, N, key);
            __builtin_amdgcn_wave_barrier();
          }
        }
        cnt = 0;
        thr_hi = static_cast<uint32_t>(mylist[N - 1].v >> 32);
      };
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int32_t local = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
          float sc = acc[t][r];
          if constexpr (COS) {
            if ((r & 3) == 0) ci4 = *reinterpret_cast<const float4*>(cinv_s + (tile & 1) * kCT + local);
            const float ci = (r & 3) == 0 ? ci4.x : (r & 3) == 1 ? ci4.y : (r & 3) == 2 ? ci4.z : ci4.w;
            sc = sc * (qi * ci);
          }
          const uint32_t o = ord32(sc);
          if (qok && c0 + local < cend && o >= thr_hi) {
            pend[cnt * NT + tid] = (static_cast<uint64_t>(o) << 32) | static_cast<uint32_t>(local);
            ++cnt;
          }
          if (__any(cnt == kPend)) drain();
          acc[t][r] = 0.f;
        }
      }
      drain();
    }
    if (it + 1 < total)
      put(stage + ((it + 1) & 1) * rec_stage_floats(NW), nkc_i == 0 ? cinv_s + (ntile_i & 1) * kCT : nullptr);
    __syncthreads();
    tile = ntile_i;
    kc = nkc_i;
  }
  // the wave's lists -> part[q][s][0..N)
  for (int x = lane; x < 32 * N; x += 64) {
    const int j = x / N, q = q0 + wave * 32 + j;
    if (q < nq) part[(static_cast<int64_t>(q) * S + s) * N + (x - j * N)] = lists[wave * 32 * N + x];
  }
}

// ---- f64: VALU score + select -----------------------------------------------------------------
constexpr int kQW = 4;  // queries per wave

// Grid: (ceil(nq / (4 * kQW)), S), 4 waves per block.  Lane = candidate; the wave's kQW query rows
// are wave-uniform reads.  COS: as k_rec_f32, one inverse per candidate lane, the queries' wave-uniform.
// MAP: as k_rec_f32.
template <bool COS, bool MAP>
__global__ __launch_bounds__(256) void k_rec_f64(const double* __restrict__ Qf, const double* __restrict__ Cf,
                                                 const int32_t* __restrict__ qrows, int nq, int32_t C, int32_t per,
                                                 int k, int N, const int32_t* __restrict__ cand_id,
                                                 const int64_t* __restrict__ excl_beg,
                                                 const int64_t* __restrict__ excl_end,
                                                 const int32_t* __restrict__ excl_rows, Key64* __restrict__ part,
                                                 const double* __restrict__ qinv,
                                                 const double* __restrict__ cinv,
                                                 const int32_t* __restrict__ pos_row) {
  __shared__ Key64 lists[4][kQW * MF_RECOMMEND_MAX_TOP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = gridDim.y, s = blockIdx.y;
  const int q0 = (blockIdx.x * 4 + wave) * kQW;
  const int32_t cbeg = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(s) * per));
  const int32_t cend = static_cast<int32_t>(min(static_cast<int64_t>(C), static_cast<int64_t>(cbeg) + per));
  Key64* wl = lists[wave];
  for (int x = lane; x < kQW * N; x += 64) wl[x] = Key64{0, 0};
  const double* qp[kQW];
  [[maybe_unused]] double qi[kQW];
#pragma unroll
  for (int i = 0; i < kQW; ++i) {
    const int q = min(q0 + i, nq - 1);
    qp[i] = Qf + static_cast<int64_t>(qrows[max(q, 0)]) * k;
    if constexpr (COS) qi[i] = qinv[qrows[max(q, 0)]];
  }
  for (int32_t c0 = cbeg; c0 < cend; c0 += 64) {
    const int32_t crow = c0 + lane;
    const bool cok = crow < cend;
    const double* cp = Cf + static_cast<int64_t>(cok ? crow : cbeg) * k;
    double pq[kQW];
#pragma unroll
    for (int i = 0; i < kQW; ++i) pq[i] = 0.0;
    for (int f = 0; f < k; ++f) {
      const double c = cp[f];
#pragma unroll
      for (int i = 0; i < kQW; ++i) pq[i] = pq[i] + qp[i][f] * c;
    }
    const int32_t cid = cok ? cand_id[crow] : 0;
    if constexpr (COS) {
      const double ci = cok ? cinv[crow] : 0.0;
#pragma unroll
      for (int i = 0; i < kQW; ++i) pq[i] = pq[i] * (qi[i] * ci);
    }
#pragma unroll
    for (int i = 0; i < kQW; ++i) {
      const int q = q0 + i;
      if (q >= nq) break;  // wave-uniform
      Key64* list = wl + i * N;
      const Key64 key = make_key(pq[i], cid);
      bool want = cok && key_gt(key, list[N - 1]);
      if constexpr (MAP) {
        if (want) want = !contains(excl_rows, excl_beg[q], excl_end[q], pos_row[crow]);
      } else {
        if (want) want = !contains(excl_rows, excl_beg[q], excl_end[q], crow);
      }
      wave_list_insert<false>(list, N, key, want, lane);
    }
  }
  for (int x = lane; x < kQW * N; x += 64) {
    const int i = x / N, q = q0 + i;
    if (q < nq) part[(static_cast<int64_t>(q) * S + s) * N + (x - i * N)] = wl[x];
  }
}

// ---- row norms (cosine) -------------------------------------------------------------------------
// inv[row] = 1 / sqrt(nn), nn the sum over ascending f from 0 of x_f * x_f in T (f32: an fmaf chain; f64:
// nn = nn + x * x, not fused), the square root and the division in f64, rounded once to T.  A zero row
// gives +inf.  One lane per row, the chain is sequential in f; a wave moves its 64 rows through LDS in
// chunks of 128 bytes per row, so that the loads are whole cache lines (a lane walking its own row would
// touch 64 lines per load), all of a chunk's loads in flight at once.  The row stride of the tile is odd in
// elements: the lanes' reads of their own rows fall on distinct banks.  One wave per block: a batch of a
// few thousand query vectors still spreads over as many CUs.
constexpr int kNormRows = 64;  // rows per block

template <typename T>
__global__ __launch_bounds__(kNormRows) void k_row_inv_norm(const T* __restrict__ X, int64_t rows, int k,
                                                            T* __restrict__ inv) {
  constexpr int KC = 128 / sizeof(T);
  __shared__ T tile[kNormRows][KC + 1];
  const int lane = threadIdx.x;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kNormRows;
  T nn = 0;
  for (int f0 = 0; f0 < k; f0 += KC) {  // k is uniform
    const int kc = min(KC, k - f0);
    T ld[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      const int e = i * 64 + lane, r = e / KC, c = e % KC;
      ld[i] = (r0 + r < rows && c < kc) ? X[(r0 + r) * k + f0 + c] : T(0);
    }
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      const int e = i * 64 + lane;
      tile[e / KC][e % KC] = ld[i];
    }
    __syncthreads();
    for (int c = 0; c < kc; ++c) {
      const T v = tile[lane][c];
      if constexpr (sizeof(T) == 4) nn = fmaf(v, v, nn);
      else nn = nn + v * v;
    }
    __syncthreads();
  }
  if (r0 + lane < rows) inv[r0 + lane] = static_cast<T>(1.0 / sqrt(static_cast<double>(nn)));
}

template <int NW, bool VEC, bool COS, bool MAP>
void rec_f32_launch(const RecLaunch& L, const int32_t* qrows, int nq, int32_t per) {
  const int N = L.top_n;
  const dim3 grid(static_cast<unsigned>((nq + NW * 32 - 1) / (NW * 32)), static_cast<unsigned>(L.S)), block(NW * 64);
  const size_t smem = sizeof(Key32) * NW * 32 * N + 8 * kPend * NW * 64 + sizeof(float) * 2 * rec_stage_floats(NW) +
                      (COS ? sizeof(float) * 2 * kCT : 0);
  // up to 72 KB (NW = 4, top 16; 1 KB more with COS): above the 64 KB a kernel gets without asking
  const void* fn = reinterpret_cast<const void*>(&k_rec_f32<NW, VEC, COS, MAP>);
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) != hipSuccess)
    fail(MF_ERR_HIP, "k_rec_f32: " + std::to_string(smem) + " bytes of LDS refused");
  hipLaunchKernelGGL((k_rec_f32<NW, VEC, COS, MAP>), grid, block, smem, L.st, static_cast<const float*>(L.Q),
                     static_cast<const float*>(L.Cf), qrows, nq, L.C, per, L.k, N, L.cand_id, L.excl_beg, L.excl_end,
                     L.excl_rows, static_cast<Key32*>(L.part), static_cast<const float*>(L.q_inv),
                     static_cast<const float*>(L.c_inv), L.pos_row);
}

template <bool COS, bool MAP>
void rec_f64_launch(const RecLaunch& L, const int32_t* qrows, int nq, int32_t per) {
  const dim3 grid(static_cast<unsigned>((nq + 4 * kQW - 1) / (4 * kQW)), static_cast<unsigned>(L.S)), block(256);
  hipLaunchKernelGGL((k_rec_f64<COS, MAP>), grid, block, 0, L.st, static_cast<const double*>(L.Q),
                     static_cast<const double*>(L.Cf), qrows, nq, L.C, per, L.k, L.top_n, L.cand_id, L.excl_beg,
                     L.excl_end, L.excl_rows, static_cast<Key64*>(L.part), static_cast<const double*>(L.q_inv),
                     static_cast<const double*>(L.c_inv), L.pos_row);
}

// (the map is never combined with the cosine metric: no caller asks for it)
template <int NW, typename... A>
void rec_f32_dispatch(bool vec, bool cos, bool map, const A&... a) {
  if (cos) vec ? rec_f32_launch<NW, true, true, false>(a...) : rec_f32_launch<NW, false, true, false>(a...);
  else if (map) vec ? rec_f32_launch<NW, true, false, true>(a...) : rec_f32_launch<NW, false, false, true>(a...);
  else vec ? rec_f32_launch<NW, true, false, false>(a...) : rec_f32_launch<NW, false, false, false>(a...);
}

}  // namespace

size_t recommend_key_bytes(bool f64) { return f64 ? sizeof(Key64) : sizeof(Key32); }

int recommend_query_tile(int top_n, bool f64) {
  if (f64) return 4 * kQW;
  return top_n <= 16 ? 128 : top_n <= 48 ? 64 : 32;
}

void launch_row_inv_norm(hipStream_t st, const void* X, int64_t rows, int k, bool f64, void* inv) {
  if (rows <= 0) return;
  const dim3 grid(static_cast<unsigned>((rows + kNormRows - 1) / kNormRows)), block(kNormRows);
  if (f64)
    hipLaunchKernelGGL((k_row_inv_norm<double>), grid, block, 0, st, static_cast<const double*>(X), rows, k,
                       static_cast<double*>(inv));
  else
    hipLaunchKernelGGL((k_row_inv_norm<float>), grid, block, 0, st, static_cast<const float*>(X), rows, k,
                       static_cast<float*>(inv));
}

void launch_recommend(const RecLaunch& L, const int32_t* qrows, int nq) {
  if (nq <= 0) return;
  const int32_t per = (L.C + L.S - 1) / L.S;
  const bool cos = L.c_inv != nullptr, map = L.pos_row != nullptr;
  if (cos && map) fail(MF_ERR_INVALID, "launch_recommend: a position map with the cosine metric");
  if (L.f64) {
    if (cos) rec_f64_launch<true, false>(L, qrows, nq, per);
    else if (map) rec_f64_launch<false, true>(L, qrows, nq, per);
    else rec_f64_launch<false, false>(L, qrows, nq, per);
  } else {
    // the lists of a block stay within 32 KB of LDS: 128 queries per block up to top 16, 64 up to 48, else 32
    const bool vec = L.k % 4 == 0;
    if (L.top_n <= 16) rec_f32_dispatch<4>(vec, cos, map, L, qrows, nq, per);
    else if (L.top_n <= 48) rec_f32_dispatch<2>(vec, cos, map, L, qrows, nq, per);
    else rec_f32_dispatch<1>(vec, cos, map, L, qrows, nq, per);
  }
  const dim3 mgrid(static_cast<unsigned>((nq + 3) / 4)), mblock(256);
  if (L.f64)
    hipLaunchKernelGGL((k_rec_merge<Key64>), mgrid, mblock, 0, L.st, static_cast<const Key64*>(L.part), nullptr, nq, L.S,
                       L.top_n, L.ids, L.scores, L.counts);
  else
    hipLaunchKernelGGL((k_rec_merge<Key32>), mgrid, mblock, 0, L.st, static_cast<const Key32*>(L.part), nullptr, nq, L.S,
                       L.top_n, L.ids, L.scores, L.counts);
}

}  // namespace mfhip
