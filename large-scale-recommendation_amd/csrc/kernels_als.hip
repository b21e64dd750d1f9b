// kernels_als.hip -- one ALS half-sweep (mf_als_run): for every rated row of one side the normal
// equations (sum_j q_j q_j^T + lambda' I) x = sum_j r_j q_j over that row's ratings, factorised and
// solved on the device.
//
//  k_als<float>   fast contexts.  One workgroup of 4 waves per work item (a whole row, or one chunk
//                 of a long row).  The counterpart rows are gathered through LDS in tiles of
//                 kTile ratings, k zero-padded to KP = a multiple of 32; Q^T Q is accumulated on the
//                 matrix cores (v_mfma_f32_32x32x2_f32), the lower-triangle 32 x 32 blocks only,
//                 dealt round-robin to the waves, each block 16 accumulator registers per lane
//                 for the whole item.  Q^T r is accumulated by threads 0..KP-1 alongside.
//  k_als<double>  deterministic contexts: the same structure on the VALU.  The 256 threads form a
//                 16 x 16 grid, thread (ty, tx) owns the entries (ty + 16 a, tx + 16 b) of the
//                 blocks with a >= b.
//  An item that is a whole row stores its accumulators into the LDS normal matrix (which reuses
//  the tile's storage: at most 66 KiB f32, 132 KiB f64, requested with hipFuncSetAttribute), adds
//  lambda' to the diagonal, factorises (Cholesky, right-looking, the trailing matrix in registers:
//  finish_row) and solves both triangles there; the matrix never goes to global memory.  A chunk
//  stores its partial matrix and right-hand side to a scratch slab; k_als_reduce adds a row's
//  partials in ascending chunk order into LDS and runs the same factorisation.  No workgroup waits
//  for another; every loop of the factorisation and the solves is bounded by k.  A pivot that is
//  not a positive finite number makes the whole row NaN.  The order of every sum is a function of
//  the row's ratings (in CSR order) and the chunk alone.
//
// The implicit-feedback half-sweep (mf_als_run_implicit) is the same two kernels with the template
// flag W set: (G + sum_j w_j q_j q_j^T + lambda' I) x = sum_{r_j > 0} (1 + w_j) q_j, w_j = alpha |r_j|.
// The weights are staged in LDS beside the ratings and multiply the A operand; G, the Gram matrix of
// the counterpart's rated rows, is read from global memory when the accumulators (whole rows) or the
// summed partials (split rows) go to the LDS matrix.  k_als_gram computes G: each workgroup takes a
// contiguous slice of the rated-row list through the same tiles and GramAcc and stores a KP x KP
// partial; k_als_gram_reduce adds the partials in ascending slice order.
//
// The non-negative half-sweeps (mf_als_run_nonneg, mf_als_run_implicit_nonneg) are the same two kernels
// with the template flag N set: the LDS matrix is symmetrised in place from its lower triangle and
// nnls_row (als_nnls_device.hpp) takes the place of finish_row, its six vectors in LDS beside the matrix
// (als_lds_bytes: at most 137 KiB, f64 at KP = 128).  The instances without N are untouched by it.
//
// These kernels take ranks 1..128 (rank buckets NB = 1..4).  Ranks 129..256, where the normal matrix no
// longer fits in LDS, go to kernels_als_wide.hip: launch_als and launch_als_gram hand them on.
#include <hip/hip_runtime.h>

#include <limits>
#include <string>

#include "als_device.hpp"
#include "als_nnls_device.hpp"
#include "common.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = 256;

template <typename T> struct GramAcc;

// f32: lower-triangle blocks w, w + 4, w + 8 of wave w (at most 3 of the 10 at KP = 128).
template <> struct GramAcc<float> : MfmaAcc<kThreads / 64, 3> {};

// f64: thread (ty, tx) of the 16 x 16 grid, entries (ty + 16 a, tx + 16 b), a >= b, a, b < 2 NB.
template <> struct GramAcc<double> {
  double acc[8][8];
  __device__ void zero() {
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
  }
  template <int NB, bool W = false>
  __device__ void tile(int tid, const double* q, int kp, int rows, const double* w = nullptr) {
    const int ty = tid >> 4, tx = tid & 15;
    for (int t = 0; t < rows; ++t) {
      const double* row = q + t * kp;
      double qa[2 * NB], qb[2 * NB];
#pragma unroll
      for (int a = 0; a < 2 * NB; ++a) {
        qa[a] = row[ty + 16 * a];
        if constexpr (W) qa[a] *= w[t];
        qb[a] = row[tx + 16 * a];
      }
#pragma unroll
      for (int a = 0; a < 2 * NB; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) acc[a][b] = fma(qa[a], qb[b], acc[a][b]);
    }
  }
  template <int NB, bool ADD = false>
  __device__ void store(int tid, double* M, int ld, const double* G = nullptr) const {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int a = 0; a < 2 * NB; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        if constexpr (ADD) M[(ty + 16 * a) * ld + tx + 16 * b] = acc[a][b] + G[(ty + 16 * a) * (32 * NB) + tx + 16 * b];
        else M[(ty + 16 * a) * ld + tx + 16 * b] = acc[a][b];
      }
  }
};

// The row's system in LDS: A (lower triangle valid, row stride ld, lambda' already on the
// diagonal, rows and columns k..KP-1 zero), rhs[k].  Either dumps it (the testing hook) or
// factorises, solves and stores x.  y, col, colraw: KP scratch values each in LDS.  Called by all
// threads of the workgroup.
// The factorisation (Cholesky, right-looking) keeps the trailing matrix in registers: thread
// (ty, tx) of the 16 x 16 grid owns the entries (ty + 16 p, tx + 16 q), q <= p.  Per column j the
// threads that own it publish it through LDS (colraw), threads 0..k-1 scale it by the pivot (col),
// and every thread takes the outer product out of the columns past j: two barriers and at most 36
// FMAs per thread and column instead of a pass over the matrix in LDS.  L then goes back to LDS for
// the two triangular solves.
template <typename T, int NB>
__device__ void finish_row(T* A, int ld, T* rhs, T* y, T* col, T* colraw, int k, T* x_out, T* dump) {
  constexpr int MB = 2 * NB;
  const int tid = threadIdx.x;
  if (dump) return als_dump_system<T, kThreads>(tid, A, ld, rhs, k, dump);
  const int ty = tid >> 4, tx = tid & 15;
  T a[MB][MB];
#pragma unroll
  for (int p = 0; p < MB; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) a[p][q] = A[(ty + 16 * p) * ld + tx + 16 * q];
  if (tid < 32 * NB) col[tid] = T(0);
  bool bad = false;
#pragma unroll
  for (int jb = 0; jb < MB; ++jb) {
    const int jn = min(16, k - 16 * jb);
    for (int jj = 0; jj < jn; ++jj) {
      const int j = 16 * jb + jj;
      if (tx == jj) {
#pragma unroll
        for (int p = jb; p < MB; ++p) colraw[ty + 16 * p] = a[p][jb];
      }
      __syncthreads();
      const T d = colraw[j];
      if (!(d > T(0)) || !(d <= std::numeric_limits<T>::max())) bad = true;  // uniform: every thread reads d
      const T piv = sqrt(d);
      if (tid >= j && tid < k) col[tid] = tid == j ? piv : colraw[tid] / piv;
      __syncthreads();
      T ca[MB], cb[MB];
#pragma unroll
      for (int p = jb; p < MB; ++p) {
        ca[p] = col[ty + 16 * p];
        cb[p] = col[tx + 16 * p];
      }
      // (rows above j of column j are upper-triangle entries: whatever they take is never read)
      if (tx == jj) {
#pragma unroll
        for (int p = jb; p < MB; ++p) a[p][jb] = ca[p];
      }
#pragma unroll
      for (int p = jb; p < MB; ++p) {
        if (tx > jj) a[p][jb] -= ca[p] * cb[jb];
#pragma unroll
        for (int q = jb + 1; q <= p; ++q) a[p][q] -= ca[p] * cb[q];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < MB; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) A[(ty + 16 * p) * ld + tx + 16 * q] = a[p][q];
  // L y = rhs
  for (int j = 0; j < k; ++j) {
    __syncthreads();
    const T yj = rhs[j] / A[j * ld + j];
    if (tid == j) y[j] = yj;
    else if (tid > j && tid < k) rhs[tid] -= A[tid * ld + j] * yj;
  }
  // L^T x = y
  for (int j = k - 1; j >= 0; --j) {
    __syncthreads();
    const T xj = y[j] / A[j * ld + j];
    if (tid == j) rhs[j] = xj;
    else if (tid < j) y[tid] -= A[j * ld + tid] * xj;
  }
  __syncthreads();
  if (tid < k) x_out[tid] = bad ? std::numeric_limits<T>::quiet_NaN() : rhs[tid];
}

// LDS layout (elements of T): M[KP * (KP + 1)] (first the gather tile, then the normal matrix),
// rhs[KP], y[KP], col[KP], colraw[KP], rv[kTile]; nnls: y, col and colraw are the first three of
// nnls_row's six vectors, and rv follows the sixth.
template <typename T>
constexpr size_t als_lds_bytes(int kp, bool nnls = false) {
  return (static_cast<size_t>(kp) * (kp + 1) + (nnls ? 7 : 4) * kp + kTile) * sizeof(T);
}

// The row's system as finish_row takes it, solved for x >= 0: the upper triangle is filled from the lower
// and nnls_row runs on the LDS matrix.  vec: 6 KP values in LDS.
template <typename T, int NB>
__device__ void finish_row_nnls(T* A, int ld, T* rhs, T* vec, int k, T* x_out, T* dump, unsigned long long* stats) {
  const int tid = threadIdx.x;
  for (int e = tid; e < k * k; e += kThreads) {
    const int i = e / k, j = e % k;
    if (j > i) A[i * ld + j] = A[j * ld + i];
  }
  nnls_row<T, kThreads>(A, ld, rhs, vec, 32 * NB, k, x_out, dump, stats);
}


// One work item per workgroup.  W (the implicit half-sweep): the ratings become confidences w = alpha |r|
// (rv) and right-hand-side coefficients 1 + w for r > 0, else 0 (cf, which borrows col: the
// factorisation's scratch is idle while the tiles run); G is the counterpart's Gram matrix, KP x KP.  A
// row with no positive rating has a zero right-hand side: its x is zero, and nothing is accumulated
// for it.  The explicit instances ignore G and alpha.  N: the non-negative solve; nnls are its counters.
template <typename T, int NB, bool W, bool N = false>
__global__ __launch_bounds__(kThreads) void k_als(const AlsItem* __restrict__ items, const int32_t* __restrict__ cols,
                                                   const T* __restrict__ vals, const T* __restrict__ Q,
                                                   T* __restrict__ X, int k, T lambda, int weighted,
                                                   T* __restrict__ partial, T* __restrict__ dump,
                                                   const T* __restrict__ G, T alpha,
                                                   unsigned long long* __restrict__ nnls) {
  constexpr int KP = 32 * NB;
  constexpr int LD = KP + 1;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* M = reinterpret_cast<T*>(smem_raw);
  T* rhs = M + KP * LD;
  T* y = rhs + KP;
  T* col = y + KP;
  T* colraw = col + KP;
  T* rv = colraw + KP + (N ? 3 * KP : 0);
  const AlsItem it = items[blockIdx.x];
  const int tid = threadIdx.x;
  if constexpr (W) {
    if (it.npos == 0 && !dump) {  // (a chunk of such a row stores no partial: k_als_reduce reads none)
      if (it.slot < 0 && tid < k) X[static_cast<size_t>(it.row) * k + tid] = T(0);
      if constexpr (N) {
        if (it.slot < 0 && tid == 0) nnls_count_zero_row(nnls);
      }
      return;
    }
  }
  T* cf = col;

  GramAcc<T> g;
  g.zero();
  T bacc = T(0);
  for (int t0 = 0; t0 < it.count; t0 += kTile) {
    const int rows = min(kTile, it.count - t0);
    __syncthreads();  // the previous tile has been read
    for (int e = tid; e < kTile * KP; e += kThreads) {
      const int t = e / KP, f = e % KP;
      T v = T(0);
      if (t < rows && f < k) v = Q[static_cast<size_t>(cols[it.begin + t0 + t]) * k + f];
      M[e] = v;
    }
    if constexpr (W) {
      if (tid < kTile) {
        const T r = tid < rows ? vals[it.begin + t0 + tid] : T(0);
        const T w = alpha * (r < T(0) ? -r : r);
        rv[tid] = w;
        cf[tid] = r > T(0) ? T(1) + w : T(0);
      }
    } else {
      if (tid < kTile) rv[tid] = tid < rows ? vals[it.begin + t0 + tid] : T(0);
    }
    __syncthreads();
    // (rows past the end are zero: the f32 path always runs whole pairs)
    g.template tile<NB, W>(tid, M, KP, (rows + 1) & ~1, rv);
    if constexpr (W) {
      if (tid < KP)
        for (int t = 0; t < rows; ++t) {
          const T c = cf[t];
          if (c != T(0)) bacc = fma(c, M[t * KP + tid], bacc);  // r > 0 only
        }
    } else {
      if (tid < KP)
        for (int t = 0; t < rows; ++t) bacc = fma(rv[t], M[t * KP + tid], bacc);
    }
  }
  __syncthreads();
  if (it.slot >= 0) {  // a chunk of a long row: the partial system goes to the scratch slab
    T* P = partial + static_cast<size_t>(it.slot) * (KP * KP + KP);
    g.template store<NB>(tid, P, KP);
    if (tid < KP) P[KP * KP + tid] = bacc;
    return;
  }
  g.template store<NB, W>(tid, M, LD, G);
  if (tid < KP) rhs[tid] = bacc;
  __syncthreads();
  const T lam = weighted ? lambda * static_cast<T>(W ? it.npos : it.count) : lambda;
  if (tid < k) M[tid * LD + tid] += lam;
  __syncthreads();
  if constexpr (N) finish_row_nnls<T, NB>(M, LD, rhs, y, k, X + static_cast<size_t>(it.row) * k, dump, nnls);
  else finish_row<T, NB>(M, LD, rhs, y, col, colraw, k, X + static_cast<size_t>(it.row) * k, dump);
}

// One workgroup per split row: partials [slot0, slot0 + chunks) added in ascending order.
// W: plus G, once, after the partial sum; a row with no positive rating is set to zero.
template <typename T, int NB, bool W, bool N = false>
__global__ __launch_bounds__(kThreads) void k_als_reduce(const AlsSplit* __restrict__ rows, const T* __restrict__ partial,
                                                          T* __restrict__ X, int k, T lambda, int weighted,
                                                          T* __restrict__ dump, const T* __restrict__ G,
                                                          unsigned long long* __restrict__ nnls) {
  constexpr int KP = 32 * NB;
  constexpr int LD = KP + 1;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* M = reinterpret_cast<T*>(smem_raw);
  T* rhs = M + KP * LD;
  T* y = rhs + KP;
  T* col = y + KP;
  T* colraw = col + KP;
  const AlsSplit sp = rows[blockIdx.x];
  const int tid = threadIdx.x;
  if constexpr (W) {
    if (sp.npos == 0 && !dump) {
      if (tid < k) X[static_cast<size_t>(sp.row) * k + tid] = T(0);
      if constexpr (N) {
        if (tid == 0) nnls_count_zero_row(nnls);
      }
      return;
    }
  }
  als_sum_partials<T, KP, kThreads, W>(tid, sp, partial, G, M, LD, rhs);
  __syncthreads();
  const T lam = weighted ? lambda * static_cast<T>(W ? sp.npos : sp.count) : lambda;
  if (tid < k) M[tid * LD + tid] += lam;
  __syncthreads();
  if constexpr (N) finish_row_nnls<T, NB>(M, LD, rhs, y, k, X + static_cast<size_t>(sp.row) * k, dump, nnls);
  else finish_row<T, NB>(M, LD, rhs, y, col, colraw, k, X + static_cast<size_t>(sp.row) * k, dump);
}

// G = sum over the rated rows of Y of y y^T.  Workgroup b takes rows [b * slice, (b + 1) * slice) of
// the list through the tiles and GramAcc of k_als and stores its KP x KP partial (lower-triangle
// blocks) to part[b]; k_als_gram_reduce adds the partials in ascending slice order into the full
// symmetric G.  The order of every sum is a function of the list and the slice length alone.
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void k_als_gram(const int32_t* __restrict__ rated, int m, int slice,
                                                        const T* __restrict__ Y, int k, T* __restrict__ part) {
  constexpr int KP = 32 * NB;
  __shared__ T tile[kTile * KP];
  const int tid = threadIdx.x;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * slice;
  const int64_t hi = min(static_cast<int64_t>(m), lo + slice);
  GramAcc<T> g;
  g.zero();
  for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
    const int rows = static_cast<int>(min(static_cast<int64_t>(kTile), hi - t0));
    __syncthreads();  // the previous tile has been read
    for (int e = tid; e < kTile * KP; e += kThreads) {
      const int t = e / KP, f = e % KP;
      T v = T(0);
      if (t < rows && f < k) v = Y[static_cast<size_t>(rated[t0 + t]) * k + f];
      tile[e] = v;
    }
    __syncthreads();
    g.template tile<NB>(tid, tile, KP, (rows + 1) & ~1);
  }
  g.template store<NB>(tid, part + static_cast<size_t>(blockIdx.x) * KP * KP, KP);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_als_gram_reduce(const T* __restrict__ part, int slices, int kp,
                                                               T* __restrict__ G) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= kp * kp) return;
  const int i = e / kp, j = e % kp;
  const int src = i >= j ? e : j * kp + i;  // the partials hold the lower triangle
  T sum = T(0);
  for (int s = 0; s < slices; ++s) sum += part[static_cast<size_t>(s) * kp * kp + src];
  G[e] = sum;
}

template <typename T, int NB, bool W, bool N>
void launch_nb(const AlsLaunch& L) {
  const size_t smem = als_lds_bytes<T>(32 * NB, N);
  if (smem > 64 * 1024)
    for (const void* fn : {reinterpret_cast<const void*>(&k_als<T, NB, W, N>),
                           reinterpret_cast<const void*>(&k_als_reduce<T, NB, W, N>)})
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) != hipSuccess)
        fail(MF_ERR_HIP, "k_als: " + std::to_string(smem) + " bytes of LDS refused");
  T* X = static_cast<T*>(L.X);
  T* partial = static_cast<T*>(L.partial);
  T* dump = static_cast<T*>(L.dump);
  const T* G = static_cast<const T*>(L.gram);
  const T lambda = static_cast<T>(L.lambda);
  const int weighted = L.weighted ? 1 : 0;
  unsigned long long* stats = static_cast<unsigned long long*>(L.nnls_stats);
  if (L.n_items > 0)
    hipLaunchKernelGGL((k_als<T, NB, W, N>), dim3(static_cast<unsigned>(L.n_items)), dim3(kThreads), smem, L.st, L.items,
                       L.cols, static_cast<const T*>(L.vals), static_cast<const T*>(L.Q), X, L.k, lambda, weighted,
                       partial, dump, G, static_cast<T>(L.alpha), stats);
  if (L.n_splits > 0)
    hipLaunchKernelGGL((k_als_reduce<T, NB, W, N>), dim3(static_cast<unsigned>(L.n_splits)), dim3(kThreads), smem, L.st,
                       L.splits, partial, X, L.k, lambda, weighted, dump, G, stats);
}

}  // namespace

void als_refuse_rank() { fail(MF_ERR_INVALID, "ALS supports a rank of at most " + std::to_string(kAlsMaxRank)); }

size_t als_partial_elems(int k) {
  const size_t kp = static_cast<size_t>((k + 31) / 32) * 32;
  return kp * kp + kp;
}

size_t als_gram_elems(int k) {
  const size_t kp = static_cast<size_t>((k + 31) / 32) * 32;
  return kp * kp;
}

int als_gram_slices(int m, int slice) { return static_cast<int>((static_cast<int64_t>(m) + slice - 1) / slice); }

void launch_als(const AlsLaunch& L) {
  if (L.nnls && !L.nnls_stats) fail(MF_ERR_INVALID, "launch_als: the non-negative solve needs its counters");
  if (L.k > 128) return launch_als_wide(L);  // kernels_als_wide.hip
  als_dispatch<1>(L.f64, L.gram != nullptr, L.k, [&](auto t, auto w, auto nb) {
    if (L.nnls) launch_nb<decltype(t), decltype(nb)::value, decltype(w)::value, true>(L);
    else launch_nb<decltype(t), decltype(nb)::value, decltype(w)::value, false>(L);
  });
}

void launch_als_gram(const AlsGramLaunch& L) {
  const int kp = (L.k + 31) / 32 * 32;
  const int slices = als_gram_slices(L.m, L.slice);
  if (slices > 0 && L.k > 128) launch_als_gram_wide(L);  // refuses a rank above kAlsMaxRank
  if (slices > 0 && L.k <= 128)
    als_dispatch<1>(L.f64, false, L.k, [&](auto t, auto, auto nb) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_als_gram<T, decltype(nb)::value>), dim3(static_cast<unsigned>(slices)), dim3(kThreads), 0,
                         L.st, L.rated, L.m, L.slice, static_cast<const T*>(L.Y), L.k, static_cast<T*>(L.part));
    });
  als_dispatch(L.f64, false, [&](auto t, auto) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_als_gram_reduce<T>), dim3(static_cast<unsigned>((kp * kp + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, L.st, static_cast<const T*>(L.part), slices, kp, static_cast<T*>(L.G));
  });
}

}  // namespace mfhip
