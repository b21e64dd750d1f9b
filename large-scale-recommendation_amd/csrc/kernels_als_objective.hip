// kernels_als_objective.hip -- the value of the ALS objective on the prepared data (mf_als_objective; the
// arithmetic is defined in include/mfhip.h and replayed by mfhip/als.py replay_objective).  Compiled without FP
// contraction: every product is rounded before it is added.
//
//  fit     one wave per work item of the USER side (a whole row of at most als_chunk ratings, or one chunk of a
//          longer row).  The user side on purpose: its gathers hit the item table (9 MB at the benchmark's shape),
//          the item side's would hit the user table (246 MB).  The wave keeps x_a in registers, lane l holding
//          x[l], x[l + 64], ..., reads 64 (col, rating) pairs with one coalesced load each, and gathers the item
//          rows straight into registers, lane l taking q[l], q[l + 64], ... (one coalesced row per load
//          instruction), kAlsObjFlight rows before the first is used.  Every q_j is used once: nothing is staged in
//          LDS.  Per rating the 64 partials go through the xor butterfly, so every lane holds d; the term of
//          rating j of the tile is kept by lane j, and lane l's f64 chain over the tiles is sum64's.
//  norms   one wave per rated row: dot64(x, x), widened and multiplied by the row's count (the ratings > 0,
//          counted from the stored values, when implicit).
//  trace   one wave: sum64 over e = f * k + g of GU[f][g] * GI[f][g].
//  sum64   one wave: lane l chains v[l], v[l + 64], ..., 16 loads in flight; then the butterfly.
// Every loop is bounded by a count, no workgroup waits for another, no atomics.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"
#include "wave_device.hpp"

namespace mfhip {
namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;

__device__ __forceinline__ float lane_of(float v, int l) { return dev::rlf(v, l); }
__device__ __forceinline__ double lane_of(double v, int l) { return dev::rld(v, l); }
__device__ __forceinline__ float abs_of(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double abs_of(double v) { return __builtin_fabs(v); }

// v[l] = v[l] + v[l ^ 32], then 16, 8, 4, 2, 1: every lane ends with the same sum.
template <typename T>
__device__ __forceinline__ T butterfly(T x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, 64);
  return x;
}

// dot64 of two rows held as lane l -> f = l, l + 64, ...: the partial's chain from 0, then the butterfly.
template <typename T, int NF>
__device__ __forceinline__ T dot64(const T (&a)[NF], const T (&b)[NF], int lane, int k) {
  T d = T(0);
#pragma unroll
  for (int c = 0; c < NF; ++c) {
    if (lane + 64 * c < k) {
      const T m = a[c] * b[c];
      d = d + m;
    }
  }
  return butterfly(d);
}

template <typename T, int NF>
__device__ __forceinline__ void load_row(const T* __restrict__ row, int lane, int k, T (&v)[NF]) {
#pragma unroll
  for (int c = 0; c < NF; ++c) {
    const int f = lane + 64 * c;
    v[c] = f < k ? row[f] : T(0);
  }
}

template <typename T, bool IMPLICIT>
__device__ __forceinline__ T fit_term(T r, T d, T alpha) {
  if constexpr (IMPLICIT) {
    const T w = alpha * abs_of(r);
    if (r > T(0)) {
      const T c = T(1) + w;
      const T e = T(1) - d;
      const T ce = c * e;
      const T a = ce * e;
      const T dd = d * d;
      return a - dd;
    }
    const T wd = w * d;
    return wd * d;
  } else {
    const T e = r - d;
    return e * e;
  }
}

template <typename T, int NF, bool IMPLICIT>
__global__ __launch_bounds__(kThreads) void k_als_obj_fit(const AlsItem* __restrict__ items, int64_t n_items,
                                                         const int32_t* __restrict__ cols, const T* __restrict__ vals,
                                                         const T* __restrict__ X, const T* __restrict__ Q, int k,
                                                         T alpha, double* __restrict__ out) {
  const int64_t it = blockIdx.x * static_cast<int64_t>(kWaves) + (threadIdx.x >> 6);
  if (it >= n_items) return;  // the whole wave; there is no barrier below
  constexpr int FL = kAlsObjFlight;
  const int lane = threadIdx.x & 63;
  const AlsItem item = items[it];
  const int n = __builtin_amdgcn_readfirstlane(item.count);
  const int row = __builtin_amdgcn_readfirstlane(item.row);
  const int64_t begin = (static_cast<int64_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(item.begin >> 32))) << 32) |
                        static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(item.begin)));
  T xv[NF];
  load_row<T, NF>(X + static_cast<size_t>(row) * k, lane, k, xv);
  double acc = 0.0;
  for (int t0 = 0; t0 < n; t0 += 64) {
    const int m = n - t0 < 64 ? n - t0 : 64;
    int32_t col = 0;
    T r = T(0);
    if (lane < m) {
      col = cols[begin + t0 + lane];
      r = vals[begin + t0 + lane];
    }
    T term = T(0);
    for (int j0 = 0; j0 < m; j0 += FL) {
      T qv[FL][NF];
#pragma unroll
      for (int u = 0; u < FL; ++u) {  // past the tile's end: its last row again, not used
        const int src = j0 + u < m ? j0 + u : m - 1;
        const int32_t cj = static_cast<int32_t>(dev::rl(static_cast<uint32_t>(col), src));
        load_row<T, NF>(Q + static_cast<size_t>(cj) * k, lane, k, qv[u]);
      }
#pragma unroll
      for (int u = 0; u < FL; ++u) {
        if (j0 + u < m) {
          const T d = dot64<T, NF>(xv, qv[u], lane, k);
          const T t = fit_term<T, IMPLICIT>(lane_of(r, j0 + u), d, alpha);
          if (lane == j0 + u) term = t;
        }
      }
    }
    if (lane < m) acc = acc + static_cast<double>(term);
  }
  acc = butterfly(acc);
  if (lane == 0) out[it] = acc;
}

// weight: 0 = none, 1 = the row's ratings, 2 = the row's ratings > 0
template <typename T, int NF>
__global__ __launch_bounds__(kThreads) void k_als_obj_norms(const int32_t* __restrict__ rated, int64_t m,
                                                           const int64_t* __restrict__ off, const T* __restrict__ vals,
                                                           const T* __restrict__ X, int k, int weight,
                                                           double* __restrict__ out) {
  const int64_t a = blockIdx.x * static_cast<int64_t>(kWaves) + (threadIdx.x >> 6);
  if (a >= m) return;
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane(rated[a]);
  T xv[NF];
  load_row<T, NF>(X + static_cast<size_t>(row) * k, lane, k, xv);
  double v = static_cast<double>(dot64<T, NF>(xv, xv, lane, k));
  if (weight != 0) {
    const int64_t b0 = off[row], b1 = off[row + 1];
    int64_t cnt = b1 - b0;
    if (weight == 2) {
      cnt = 0;
      for (int64_t e0 = b0; e0 < b1; e0 += 64) {
        const int64_t e = e0 + lane;
        cnt += __popcll(__ballot(e < b1 && vals[e] > T(0)));
      }
    }
    v = v * static_cast<double>(cnt);
  }
  if (lane == 0) out[a] = v;
}

template <typename T>
__global__ __launch_bounds__(64) void k_als_obj_trace(const T* __restrict__ GU, const T* __restrict__ GI, int k, int kp,
                                                     double* __restrict__ out) {
  const int lane = threadIdx.x;
  const int n = k * k;
  double acc = 0.0;
  for (int e0 = 0; e0 < n; e0 += 64 * 8) {
    T p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 64 * u + lane;
      const int f = e < n ? e / k : 0, g = e < n ? e - f * k : 0;
      p[u] = GU[static_cast<size_t>(f) * kp + g] * GI[static_cast<size_t>(f) * kp + g];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (e0 + 64 * u + lane < n) acc = acc + static_cast<double>(p[u]);
  }
  acc = butterfly(acc);
  if (lane == 0) *out = acc;
}

__global__ __launch_bounds__(64) void k_sum64(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  int64_t i = lane;
  for (; i + 15 * 64 < n; i += 16 * 64) {
    double t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = v[i + 64 * u];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = acc + t[u];
  }
  for (; i < n; i += 64) acc = acc + v[i];
  acc = butterfly(acc);
  if (lane == 0) *out = acc;
}

unsigned wave_grid(int64_t n) { return static_cast<unsigned>((n + kWaves - 1) / kWaves); }

// The rank as the factors a lane holds: f(std::integral_constant<int, NF>()), NF = ceil(k / 64) in 1 .. 4.
template <typename F>
void by_lane_factors(int k, F&& f) {
  switch ((k + 63) / 64) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    default: als_refuse_rank();
  }
}

}  // namespace

void launch_als_objective_fit(const AlsObjectiveLaunch& L) {
  if (L.n_items == 0) return;
  als_dispatch(L.f64, L.implicit, [&](auto t, auto w) {
    using T = decltype(t);
    constexpr bool W = decltype(w)::value;
    by_lane_factors(L.k, [&](auto nf) {
      constexpr int NF = decltype(nf)::value;
      hipLaunchKernelGGL((k_als_obj_fit<T, NF, W>), dim3(wave_grid(L.n_items)), dim3(kThreads), 0, L.st, L.items,
                         L.n_items, L.cols, static_cast<const T*>(L.vals), static_cast<const T*>(L.X),
                         static_cast<const T*>(L.Q), L.k, static_cast<T>(L.alpha), L.item_sums);
    });
  });
}

void launch_als_objective_norms(hipStream_t st, const int32_t* rated, int64_t m, const int64_t* off, const void* vals,
                                const void* X, int k, bool f64, int weight, double* out) {
  if (m == 0) return;
  als_dispatch(f64, false, [&](auto t, auto) {
    using T = decltype(t);
    by_lane_factors(k, [&](auto nf) {
      constexpr int NF = decltype(nf)::value;
      hipLaunchKernelGGL((k_als_obj_norms<T, NF>), dim3(wave_grid(m)), dim3(kThreads), 0, st, rated, m, off,
                         static_cast<const T*>(vals), static_cast<const T*>(X), k, weight, out);
    });
  });
}

void launch_als_objective_trace(hipStream_t st, const void* GU, const void* GI, int k, bool f64, double* out) {
  const int kp = (k + 31) / 32 * 32;
  if (f64)
    hipLaunchKernelGGL(k_als_obj_trace<double>, dim3(1), dim3(64), 0, st, static_cast<const double*>(GU),
                       static_cast<const double*>(GI), k, kp, out);
  else
    hipLaunchKernelGGL(k_als_obj_trace<float>, dim3(1), dim3(64), 0, st, static_cast<const float*>(GU),
                       static_cast<const float*>(GI), k, kp, out);
}

void launch_sum64(hipStream_t st, const double* v, int64_t n, double* out) {
  hipLaunchKernelGGL(k_sum64, dim3(1), dim3(64), 0, st, v, n, out);
}

}  // namespace mfhip
