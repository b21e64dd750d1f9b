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
// These kernels take ranks 1..128 (rank buckets NB = 1..4).  Ranks 129..256, where the normal matrix no
// longer fits in LDS, go to kernels_als_wide.hip: launch_als and launch_als_gram hand them on.
#include <hip/hip_runtime.h>

#include <limits>
#include <string>

#include "common.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;  // ratings per LDS tile (a multiple of 2: one MFMA takes two ratings)

typedef float v16f __attribute__((ext_vector_type(16)));

template <typename T> struct GramAcc;

// f32: lower-triangle blocks w, w + 4, w + 8 of wave w (at most 3 of the 10 at KP = 128).
template <> struct GramAcc<float> {
  v16f acc[3];
  __device__ void zero() {
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;
  }
  // block number b -> (bi, bj), bj <= bi, row-major over the triangle
  __device__ static void block_of(int b, int& bi, int& bj) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= b) ++bi;  // bi <= 3
    bj = b - bi * (bi + 1) / 2;
  }
  // W: w[t] (LDS) multiplies rating t's A operand
  template <int NB, bool W = false>
  __device__ void tile(const float* q, int kp, int rows, const float* w = nullptr) {
    constexpr int kBlocks = NB * (NB + 1) / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const int b = wave + 4 * x;
      if (b >= kBlocks) break;
      int bi, bj;
      block_of(b, bi, bj);
      const float* pa = q + h * kp + 32 * bi + c;
      const float* pb = q + h * kp + 32 * bj + c;
      if constexpr (W) {
        for (int t = 0; t < rows; t += 2)
          acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[t + h] * pa[t * kp], pb[t * kp], acc[x], 0, 0, 0);
      } else {
        for (int t = 0; t < rows; t += 2)
          acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[t * kp], pb[t * kp], acc[x], 0, 0, 0);
      }
    }
  }
  // accumulators -> M (row stride ld); register r of a block is row (r & 3) + 8 (r >> 2) + 4 h
  // ADD: plus G (row stride 32 NB) on the way
  template <int NB, bool ADD = false>
  __device__ void store(float* M, int ld, const float* G = nullptr) const {
    constexpr int kBlocks = NB * (NB + 1) / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const int b = wave + 4 * x;
      if (b >= kBlocks) break;
      int bi, bj;
      block_of(b, bi, bj);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (ADD) {
          const int row = 32 * bi + (r & 3) + 8 * (r >> 2) + 4 * h;
          M[row * ld + 32 * bj + c] = acc[x][r] + G[row * (32 * NB) + 32 * bj + c];
        } else {
          M[(32 * bi + (r & 3) + 8 * (r >> 2) + 4 * h) * ld + 32 * bj + c] = acc[x][r];
        }
      }
    }
  }
};

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
  __device__ void tile(const double* q, int kp, int rows, const double* w = nullptr) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
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
  __device__ void store(double* M, int ld, const double* G = nullptr) const {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
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
  if (dump) {  // full symmetric k x k, then the right-hand side
    for (int e = tid; e < k * k; e += kThreads) {
      const int i = e / k, j = e % k;
      dump[e] = i >= j ? A[i * ld + j] : A[j * ld + i];
    }
    if (tid < k) dump[k * k + tid] = rhs[tid];
    return;
  }
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
// rhs[KP], y[KP], col[KP], colraw[KP], rv[kTile]
template <typename T>
constexpr size_t als_lds_bytes(int kp) {
  return (static_cast<size_t>(kp) * (kp + 1) + 4 * kp + kTile) * sizeof(T);
}

// W (the implicit half-sweep): the ratings become confidences w = alpha |r| (rv) and right-hand-side
// coefficients 1 + w for r > 0, else 0 (cf, which borrows col: the factorisation's scratch is idle
// while the tiles run); G is the counterpart's Gram matrix, KP x KP.  A row with no positive rating
// has a zero right-hand side: its x is zero, and nothing is accumulated for it.
template <typename T, int NB, bool W>
__device__ __forceinline__ void als_item(const AlsItem* __restrict__ items, const int32_t* __restrict__ cols,
                                         const T* __restrict__ vals, const T* __restrict__ Q, T* __restrict__ X,
                                         int k, T lambda, int weighted, T* __restrict__ partial,
                                         T* __restrict__ dump, const T* __restrict__ G, T alpha) {
  constexpr int KP = 32 * NB;
  constexpr int LD = KP + 1;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* M = reinterpret_cast<T*>(smem_raw);
  T* rhs = M + KP * LD;
  T* y = rhs + KP;
  T* col = y + KP;
  T* colraw = col + KP;
  T* rv = colraw + KP;
  const AlsItem it = items[blockIdx.x];
  const int tid = threadIdx.x;
  if constexpr (W) {
    if (it.npos == 0 && !dump) {  // (a chunk of such a row stores no partial: k_als_reduce reads none)
      if (it.slot < 0 && tid < k) X[static_cast<size_t>(it.row) * k + tid] = T(0);
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
    g.template tile<NB, W>(M, KP, (rows + 1) & ~1, rv);
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
    g.template store<NB>(P, KP);
    if (tid < KP) P[KP * KP + tid] = bacc;
    return;
  }
  g.template store<NB, W>(M, LD, G);
  if (tid < KP) rhs[tid] = bacc;
  __syncthreads();
  const T lam = weighted ? lambda * static_cast<T>(W ? it.npos : it.count) : lambda;
  if (tid < k) M[tid * LD + tid] += lam;
  __syncthreads();
  finish_row<T, NB>(M, LD, rhs, y, col, colraw, k, X + static_cast<size_t>(it.row) * k, dump);
}

template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void k_als(const AlsItem* __restrict__ items, const int32_t* __restrict__ cols,
                                                   const T* __restrict__ vals, const T* __restrict__ Q,
                                                   T* __restrict__ X, int k, T lambda, int weighted,
                                                   T* __restrict__ partial, T* __restrict__ dump) {
  als_item<T, NB, false>(items, cols, vals, Q, X, k, lambda, weighted, partial, dump, nullptr, T(0));
}

template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void k_als_implicit(const AlsItem* __restrict__ items,
                                                            const int32_t* __restrict__ cols,
                                                            const T* __restrict__ vals, const T* __restrict__ Q,
                                                            T* __restrict__ X, int k, T lambda, int weighted,
                                                            T* __restrict__ partial, T* __restrict__ dump,
                                                            const T* __restrict__ G, T alpha) {
  als_item<T, NB, true>(items, cols, vals, Q, X, k, lambda, weighted, partial, dump, G, alpha);
}

// One workgroup per split row: partials [slot0, slot0 + chunks) added in ascending order.
// W: plus G, once, after the partial sum; a row with no positive rating is set to zero.
template <typename T, int NB, bool W>
__device__ __forceinline__ void als_split(const AlsSplit* __restrict__ rows, const T* __restrict__ partial,
                                          T* __restrict__ X, int k, T lambda, int weighted, T* __restrict__ dump,
                                          const T* __restrict__ G) {
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
      return;
    }
  }
  constexpr size_t kStride = static_cast<size_t>(KP) * KP + KP;
  for (int e = tid; e < KP * KP + KP; e += kThreads) {
    const int i = e / KP, j = e % KP;
    if (i < KP && j > i) continue;  // only the lower triangle is defined
    T sum = T(0);
    for (int c = 0; c < sp.chunks; ++c) sum += partial[(static_cast<size_t>(sp.slot0) + c) * kStride + e];
    if constexpr (W) {
      if (i < KP) sum += G[e];
    }
    if (i < KP) M[i * LD + j] = sum;
    else rhs[j] = sum;
  }
  __syncthreads();
  const T lam = weighted ? lambda * static_cast<T>(W ? sp.npos : sp.count) : lambda;
  if (tid < k) M[tid * LD + tid] += lam;
  __syncthreads();
  finish_row<T, NB>(M, LD, rhs, y, col, colraw, k, X + static_cast<size_t>(sp.row) * k, dump);
}

template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void k_als_reduce(const AlsSplit* __restrict__ rows, const T* __restrict__ partial,
                                                          T* __restrict__ X, int k, T lambda, int weighted,
                                                          T* __restrict__ dump) {
  als_split<T, NB, false>(rows, partial, X, k, lambda, weighted, dump, nullptr);
}

template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void k_als_reduce_implicit(const AlsSplit* __restrict__ rows,
                                                                   const T* __restrict__ partial, T* __restrict__ X,
                                                                   int k, T lambda, int weighted, T* __restrict__ dump,
                                                                   const T* __restrict__ G) {
  als_split<T, NB, true>(rows, partial, X, k, lambda, weighted, dump, G);
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
    g.template tile<NB>(tile, KP, (rows + 1) & ~1);
  }
  g.template store<NB>(part + static_cast<size_t>(blockIdx.x) * KP * KP, KP);
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

template <typename T, int NB>
void launch_nb(hipStream_t st, const AlsItem* items, int n_items, const AlsSplit* splits, int n_splits,
               const int32_t* cols, const void* vals, const void* Q, void* X, int k, double lambda, int weighted,
               void* partial, void* dump, const void* gram, double alpha) {
  constexpr int KP = 32 * NB;
  const size_t smem = als_lds_bytes<T>(KP);
  const void* f1 = gram ? reinterpret_cast<const void*>(&k_als_implicit<T, NB>) : reinterpret_cast<const void*>(&k_als<T, NB>);
  const void* f2 = gram ? reinterpret_cast<const void*>(&k_als_reduce_implicit<T, NB>)
                        : reinterpret_cast<const void*>(&k_als_reduce<T, NB>);
  if (smem > 64 * 1024)
    for (const void* fn : {f1, f2})
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) != hipSuccess)
        fail(MF_ERR_HIP, "k_als: " + std::to_string(smem) + " bytes of LDS refused");
  const dim3 gi(static_cast<unsigned>(n_items)), gs(static_cast<unsigned>(n_splits));
  if (n_items > 0 && !gram)
    hipLaunchKernelGGL((k_als<T, NB>), gi, dim3(kThreads), smem, st, items, cols,
                       static_cast<const T*>(vals), static_cast<const T*>(Q), static_cast<T*>(X), k,
                       static_cast<T>(lambda), weighted, static_cast<T*>(partial), static_cast<T*>(dump));
  if (n_items > 0 && gram)
    hipLaunchKernelGGL((k_als_implicit<T, NB>), gi, dim3(kThreads), smem, st, items, cols,
                       static_cast<const T*>(vals), static_cast<const T*>(Q), static_cast<T*>(X), k,
                       static_cast<T>(lambda), weighted, static_cast<T*>(partial), static_cast<T*>(dump),
                       static_cast<const T*>(gram), static_cast<T>(alpha));
  if (n_splits > 0 && !gram)
    hipLaunchKernelGGL((k_als_reduce<T, NB>), gs, dim3(kThreads), smem, st, splits,
                       static_cast<const T*>(partial), static_cast<T*>(X), k, static_cast<T>(lambda), weighted,
                       static_cast<T*>(dump));
  if (n_splits > 0 && gram)
    hipLaunchKernelGGL((k_als_reduce_implicit<T, NB>), gs, dim3(kThreads), smem, st, splits,
                       static_cast<const T*>(partial), static_cast<T*>(X), k, static_cast<T>(lambda), weighted,
                       static_cast<T*>(dump), static_cast<const T*>(gram));
}

template <typename T>
void launch_t(hipStream_t st, const AlsItem* items, int n_items, const AlsSplit* splits, int n_splits,
              const int32_t* cols, const void* vals, const void* Q, void* X, int k, double lambda, int weighted,
              void* partial, void* dump, const void* gram, double alpha) {
  switch ((k + 31) / 32) {
    case 1: return launch_nb<T, 1>(st, items, n_items, splits, n_splits, cols, vals, Q, X, k, lambda, weighted, partial, dump, gram, alpha);
    case 2: return launch_nb<T, 2>(st, items, n_items, splits, n_splits, cols, vals, Q, X, k, lambda, weighted, partial, dump, gram, alpha);
    case 3: return launch_nb<T, 3>(st, items, n_items, splits, n_splits, cols, vals, Q, X, k, lambda, weighted, partial, dump, gram, alpha);
    case 4: return launch_nb<T, 4>(st, items, n_items, splits, n_splits, cols, vals, Q, X, k, lambda, weighted, partial, dump, gram, alpha);
    default: fail(MF_ERR_INVALID, "ALS supports a rank of at most " + std::to_string(kAlsMaxRank));
  }
}

template <typename T>
void launch_gram_t(hipStream_t st, const int32_t* rated, int m, int slice, const void* Y, int k, void* part, void* G) {
  const int nb = (k + 31) / 32, kp = 32 * nb;
  const int slices = als_gram_slices(m, slice);
  const dim3 grid(static_cast<unsigned>(slices)), block(kThreads);
  const T* y = static_cast<const T*>(Y);
  T* p = static_cast<T*>(part);
  if (slices > 0) switch (nb) {
    case 1: hipLaunchKernelGGL((k_als_gram<T, 1>), grid, block, 0, st, rated, m, slice, y, k, p); break;
    case 2: hipLaunchKernelGGL((k_als_gram<T, 2>), grid, block, 0, st, rated, m, slice, y, k, p); break;
    case 3: hipLaunchKernelGGL((k_als_gram<T, 3>), grid, block, 0, st, rated, m, slice, y, k, p); break;
    case 4: hipLaunchKernelGGL((k_als_gram<T, 4>), grid, block, 0, st, rated, m, slice, y, k, p); break;
    default: launch_als_gram_wide(st, rated, m, slice, Y, k, sizeof(T) == 8, part);  // refuses a rank above kAlsMaxRank
  }
  hipLaunchKernelGGL((k_als_gram_reduce<T>), dim3(static_cast<unsigned>((kp * kp + kThreads - 1) / kThreads)), block, 0,
                     st, static_cast<const T*>(part), slices, kp, static_cast<T*>(G));
}

}  // namespace

size_t als_partial_elems(int k) {
  const size_t kp = static_cast<size_t>((k + 31) / 32) * 32;
  return kp * kp + kp;
}

size_t als_gram_elems(int k) {
  const size_t kp = static_cast<size_t>((k + 31) / 32) * 32;
  return kp * kp;
}

int als_gram_slices(int m, int slice) { return static_cast<int>((static_cast<int64_t>(m) + slice - 1) / slice); }

void launch_als(hipStream_t st, const AlsItem* items, int n_items, const AlsSplit* splits, int n_splits,
                const int32_t* cols, const void* vals, const void* Q, void* X, int k, double lambda, bool weighted,
                bool f64, void* partial, void* dump, const void* gram, double alpha, void* slab, int slabs) {
  if (k > 128)  // kernels_als_wide.hip
    return launch_als_wide(st, items, n_items, splits, n_splits, cols, vals, Q, X, k, lambda, weighted, f64, partial, dump,
                           gram, alpha, slab, slabs);
  if (f64) launch_t<double>(st, items, n_items, splits, n_splits, cols, vals, Q, X, k, lambda, weighted ? 1 : 0, partial, dump, gram, alpha);
  else launch_t<float>(st, items, n_items, splits, n_splits, cols, vals, Q, X, k, lambda, weighted ? 1 : 0, partial, dump, gram, alpha);
}

void launch_als_gram(hipStream_t st, const int32_t* rated, int m, int slice, const void* Y, int k, bool f64, void* part,
                     void* G) {
  if (f64) launch_gram_t<double>(st, rated, m, slice, Y, k, part, G);
  else launch_gram_t<float>(st, rated, m, slice, Y, k, part, G);
}

}  // namespace mfhip
