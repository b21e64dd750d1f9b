// als_nnls_device.hpp -- the non-negative solve of the ALS half-sweeps (mf_als_run_nonneg,
// mf_als_run_implicit_nonneg): a projected conjugate-gradient NNLS on the row's normal matrix where it
// already stands, the LDS matrix of kernels_als.hip (ranks 1..128) or the global slab of
// kernels_als_wide.hip (129..256).  One routine for both: it sees a full symmetric matrix (row stride
// ld), the right-hand side and six scratch vectors in LDS.  The rules, the reason codes and the order of
// every sum are those mfhip.h states for mf_nnls_solve, whose host code (nnls.cpp) replays this file
// operation for operation; a change here is a change there.  Included by those two kernel files only.
//
// Thread i < k owns element i of every vector and row i of the matrix; every scalar (a dot product, the
// step, the wall clamp) is computed by every thread from the same LDS values in the same order, so all
// threads hold the same bits and every branch on them is uniform.  No floating-point atomics; every loop
// is bounded by k or the iteration cap.  FP contraction is off inside these functions whatever the file
// is built with: every fma is written, every other operation is a single rounding.
#pragma once
#include <hip/hip_runtime.h>

#include <limits>

namespace mfhip {
namespace {

enum : int { kNnlsConverged = 0, kNnlsCapped = 1, kNnlsStep = 2, kNnlsNan = 3 };
// the device counters behind mf_als_nonneg_stats, in the order of the struct
enum : int { kNnRows = 0, kNnIterations, kNnMaxIterations, kNnCapped, kNnReason2, kNnNanRows };

template <typename T>
__device__ __forceinline__ bool nnls_finite(T v) {
  return v - v == T(0);
}

// a . b: lane l of the wave sums f = l, l + 64, ... ascending (s = fma(a[f], b[f], s) from 0), the 64 lane
// sums are added by the butterfly xor 32, 16, 8, 4, 2, 1.  Every wave computes it, from LDS.
template <typename T>
__device__ __forceinline__ T nnls_dot(const T* a, const T* b, int k) {
#pragma clang fp contract(off)
  T s = T(0);
  for (int f = threadIdx.x & 63; f < k; f += 64) s = fma(a[f], b[f], s);
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// (A v)[i]: s = fma(A[j][i], v[j], s) from 0 over j = 0 .. k-1 (A is symmetric bit for bit; column i of
// row j is the access that neither conflicts in LDS nor strides in global memory).
template <typename T>
__device__ __forceinline__ T nnls_matvec(const T* A, int ld, const T* v, int k, int i) {
#pragma clang fp contract(off)
  T s = T(0);
  for (int j = 0; j < k; ++j) s = fma(A[j * ld + i], v[j], s);
  return s;
}

template <typename T>
__device__ __forceinline__ bool nnls_stop(T step, T nd, T thresh) {
  return !nnls_finite(step) || !(step > T(0)) || nd <= thresh;
}

// Solves the row.  A: k x k, full symmetric, row stride ld (LDS or global; the last store to it lies
// behind a barrier or is the caller's own: this routine starts with one).  b: k values in LDS.  vec: six
// vectors of kp elements in LDS (x, res, g, dir, lastDir, A v).  dump == null: x goes to x_out and the
// row to the counters; else (the testing hook) dump[0 .. k) = x, dump[k] = iterations, dump[k + 1] =
// reason, and neither x_out nor the counters are touched.  Called by all THREADS threads of the workgroup.
template <typename T, int THREADS>
__device__ __forceinline__ void nnls_row(const T* A, int ld, const T* b, T* vec, int kp, int k, T* x_out, T* dump,
                                         unsigned long long* stats) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const bool mine = tid < k;
  T* x = vec;
  T* res = x + kp;
  T* g = res + kp;
  T* dir = g + kp;
  T* last = dir + kp;
  T* av = last + kp;
  if (mine) {
    x[tid] = T(0);
    last[tid] = T(0);
  }
  __syncthreads();
  const T bb = nnls_dot(b, b, k);
  const T thresh = static_cast<T>(1e-12) * bb;
  const T slack = T(1) - T(64) * std::numeric_limits<T>::epsilon();
  const int cap = max(400, 20 * k);
  int it = 0, last_wall = 0, reason = kNnlsCapped;
  T last_norm = T(0);
  if (!nnls_finite(bb)) {
    reason = kNnlsNan;
  } else {
    for (; it < cap; ++it) {
      T gi = T(0);
      if (mine) {
        const T r = nnls_matvec(A, ld, x, k, tid) - b[tid];
        gi = (r > T(0) && x[tid] == T(0)) ? T(0) : r;
        res[tid] = r;
        g[tid] = gi;
      }
      __syncthreads();
      const T ng = nnls_dot(g, g, k);
      const T gr = nnls_dot(g, res, k);
      if (mine) av[tid] = nnls_matvec(A, ld, g, k, tid);
      __syncthreads();
      T step = gr / nnls_dot(g, av, k);
      T nd = ng;
      bool conj = false;
      if (it > last_wall + 1) {
        const T beta = ng / last_norm;
        if (mine) dir[tid] = fma(beta, last[tid], gi);
        __syncthreads();  // (every thread has read av by now)
        if (mine) av[tid] = nnls_matvec(A, ld, dir, k, tid);
        __syncthreads();
        const T s2 = nnls_dot(dir, res, k) / nnls_dot(dir, av, k);
        const T n2 = nnls_dot(dir, dir, k);
        if (!nnls_stop(s2, n2, thresh)) {
          conj = true;
          step = s2;
          nd = n2;
        }
      }
      if (nd <= thresh) {
        reason = kNnlsConverged;
        break;
      }
      if (!nnls_finite(step)) {
        reason = kNnlsNan;
        break;
      }
      if (!(step > T(0))) {
        reason = kNnlsStep;
        break;
      }
      __syncthreads();  // the conjugate direction has been read
      if (!conj && mine) dir[tid] = gi;
      __syncthreads();
      for (int i = 0; i < k; ++i) {  // do not cross a wall: ascending, every thread alike
        const T d = dir[i], xi = x[i];
        if (step * d > xi) step = xi / d;
      }
      __syncthreads();  // x has been read
      bool wall = false;
      if (mine) {
        const T d = dir[tid], xi = x[tid], sd = step * d;
        if (sd > xi * slack) {
          x[tid] = T(0);
          wall = true;
        } else {
          x[tid] = xi - sd;
        }
        last[tid] = d;
      }
      if (__syncthreads_or(wall)) last_wall = it;
      last_norm = ng;
    }
  }
  if (mine) (dump ? dump : x_out)[tid] = reason == kNnlsNan ? std::numeric_limits<T>::quiet_NaN() : x[tid];
  if (tid == 0) {
    if (dump) {
      dump[k] = static_cast<T>(it);
      dump[k + 1] = static_cast<T>(reason);
    } else {
      atomicAdd(stats + kNnRows, 1ull);
      atomicAdd(stats + kNnIterations, static_cast<unsigned long long>(it));
      atomicMax(stats + kNnMaxIterations, static_cast<unsigned long long>(it));
      if (reason == kNnlsCapped) atomicAdd(stats + kNnCapped, 1ull);
      if (reason == kNnlsStep) atomicAdd(stats + kNnReason2, 1ull);
      if (reason == kNnlsNan) atomicAdd(stats + kNnNanRows, 1ull);
    }
  }
}

// A row that is set to zero without a solve (an implicit row with no positive rating).
__device__ __forceinline__ void nnls_count_zero_row(unsigned long long* stats) {
  atomicAdd(stats + kNnRows, 1ull);
}

}  // namespace
}  // namespace mfhip
