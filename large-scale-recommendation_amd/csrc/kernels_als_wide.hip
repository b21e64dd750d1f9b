// kernels_als_wide.hip -- the ALS half-sweep of kernels_als.hip at ranks 129..256 (rank buckets
// NB = 5..8, KP = 32 NB = 160..256), where a row's normal matrix no longer fits in LDS.
//
// One workgroup of 512 threads (8 waves, two per SIMD: 256 registers per lane) per work item, for
// both precisions:
//  - The Gram accumulation is that of the narrow path, dealt wider.  f32: the 15..36 lower-triangle
//    32 x 32 blocks go round-robin to the 8 waves (at most 5 each, 80 accumulator registers per
//    lane, v_mfma_f32_32x32x2_f32).  f64: the threads form a 16 x 32 grid, thread (ty, tx) owns the
//    entries (ty + 16 a, tx + 32 b) of the blocks on and below the diagonal (at most 72 doubles),
//    plain FMAs on the VALU.
//  - The normal matrix lives in global memory, one KP x KP slab (row stride KP, lower triangle) per
//    resident workgroup: the grid is a small multiple of the CU count and workgroup g takes the work
//    items g, g + gridDim.x, ... of the launch.  No workgroup waits for another.
//  - finish_wide factorises the slab with a blocked left-looking Cholesky.  A panel of 32 columns is
//    held in registers (thread (ty, tx): column tx, rows ty + 16 a of the panel), updated by the
//    columns to its left (staged through LDS 32 at a time, ascending), factorised with the narrow
//    path's column scheme (the raw column published through LDS, scaled by the pivot, the outer
//    product taken out of the columns past it: two barriers per column), and written back.  The
//    forward solve rides on the same column steps; the backward solve reloads the panels into LDS
//    last to first.  Every loop is bounded by k or KP; every product-sum is an explicit fma, so the
//    instances of the routine in k_als_wide and k_als_reduce_wide round alike.
// Chunks of long rows store partials exactly as the narrow path does; k_als_reduce_wide adds them
// in ascending chunk order into the slab and runs the same finish_wide.
// The template flag N (the non-negative half-sweeps) fills the slab's upper triangle from the lower and
// runs nnls_row (als_nnls_device.hpp) over it instead of finish_wide; its six vectors take the stage
// panel's place in LDS, so the LDS request is the same.  The instances without N are untouched by it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <string>

#include "als_device.hpp"
#include "als_nnls_device.hpp"
#include "common.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kWThreads = 512;
constexpr int kRY = kWThreads / 32;  // rows of the thread grid (32 columns)
constexpr int kPLd = 33;    // row stride of a 32-column panel in LDS

template <typename T> struct WideAcc;

// f32: lower-triangle blocks w, w + 8, ..., w + 32 of wave w (36 blocks at KP = 256: at most 5).
template <> struct WideAcc<float> : MfmaAcc<kWThreads / 64, 5> {};

// f64: thread (ty, tx) of the 16 x 32 grid, entries (ty + 16 a, tx + 32 b), a < 2 NB, b <= a * kRY / 32.
template <> struct WideAcc<double> {
  double acc[16][8];
  __device__ void zero() {
#pragma unroll
    for (int a = 0; a < 16; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
  }
  template <int NB, bool W = false>
  __device__ void tile(int tid, const double* q, int kp, int rows, const double* w = nullptr) {
    const int ty = tid >> 5, tx = tid & 31;
#pragma unroll 1
    for (int t = 0; t < rows; ++t) {
      const double* row = q + t * kp;
      double qb[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) qb[b] = row[tx + 32 * b];
#pragma unroll
      for (int a = 0; a < 32 * NB / kRY; ++a) {
        if (a % 2 == 0) __builtin_amdgcn_sched_barrier(0);  // at most two rows' loads in flight: registers
        double qa = row[ty + kRY * a];
        if constexpr (W) qa *= w[t];
#pragma unroll
        for (int b = 0; b <= a * kRY / 32; ++b) acc[a][b] = fma(qa, qb[b], acc[a][b]);
      }
    }
  }
  template <int NB>
  __device__ void store(int tid, double* M, int ld) const {
    const int ty = tid >> 5, tx = tid & 31;
#pragma unroll
    for (int a = 0; a < 32 * NB / kRY; ++a)
#pragma unroll
      for (int b = 0; b <= a * kRY / 32; ++b) M[(ty + kRY * a) * ld + tx + 32 * b] = acc[a][b];
  }
};

// The row's system: S (global, the workgroup's slab: lower triangle valid, row stride KP, lambda'
// already on the diagonal, rows and columns k..KP-1 zero) and rhs[k] (LDS).  Either dumps it (the
// testing hook) or factorises, solves and stores x.  P, stage: KP x 33 each in LDS; y, col, colraw:
// KP values each.  Called by all threads of the workgroup, behind a barrier after the last store to S.
template <typename T, int NB>
__device__ __forceinline__ void finish_wide(T* S, T* P, T* stage, T* rhs, T* y, T* col, T* colraw, int k, T* x_out, T* dump) {
  constexpr int KP = 32 * NB;
  // (an opaque copy: what is derived from it is formed here, after the Gram accumulators have died, not
  // hoisted out of the caller's item loop to be spilled across them)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid) : : "memory");
  if (dump) return als_dump_system<T, kWThreads>(tid, S, KP, rhs, k, dump);
  const int ty = tid >> 5, tx = tid & 31;
  bool bad = false;
#pragma unroll 1
  for (int p = 0; p < NB; ++p) {
    const int c0 = 32 * p, nrem = 32 * (NB - p) / kRY, nrows = KP - c0, jn = min(32, k - c0);
    // the panel: entries (c0 + ty + 16 a, c0 + tx), a < nrem; what lies above the diagonal is never read
    T acc[32 * NB / kRY];
#pragma unroll
    for (int a = 0; a < 32 * NB / kRY; ++a) {
      const int r = ty + kRY * a;
      acc[a] = (a < nrem && r >= tx) ? S[(c0 + r) * KP + c0 + tx] : T(0);
    }
    // minus the columns to its left, 32 at a time, ascending
    for (int q = 0; q < p; ++q) {
      __syncthreads();  // the columns have been written back; the previous stage has been read
      for (int e = tid; e < nrows * 32; e += kWThreads) {
        const int r = e >> 5, c = e & 31;
        stage[r * kPLd + c] = S[(c0 + r) * KP + 32 * q + c];
      }
      __syncthreads();
#pragma unroll 4
      for (int c = 0; c < 32; ++c) {
        const T b = stage[tx * kPLd + c];
#pragma unroll
        for (int a = 0; a < 32 * NB / kRY; ++a)
          if (a < nrem) acc[a] = fma(-stage[(ty + kRY * a) * kPLd + c], b, acc[a]);
      }
    }
    // the panel's own columns, and the forward solve L y = rhs along with them
    for (int jj = 0; jj < jn; ++jj) {
      if (tx == jj) {
#pragma unroll
        for (int a = 0; a < 32 * NB / kRY; ++a)
          if (a < nrem) colraw[ty + kRY * a] = acc[a];
      }
      __syncthreads();
      const T d = colraw[jj];
      if (!(d > T(0)) || !(d <= std::numeric_limits<T>::max())) bad = true;  // uniform: every thread reads d
      const T piv = sqrt(d);
      const T yj = rhs[c0 + jj] / piv;
      if (tid < nrows) {
        T l = T(0);
        if (tid >= jj && c0 + tid < k) l = tid == jj ? piv : colraw[tid] / piv;
        col[tid] = l;
        if (tid == jj) y[c0 + jj] = yj;
        else if (tid > jj && c0 + tid < k) rhs[c0 + tid] = fma(-l, yj, rhs[c0 + tid]);
      }
      __syncthreads();
      if (tx == jj) {
#pragma unroll
        for (int a = 0; a < 32 * NB / kRY; ++a)
          if (a < nrem) acc[a] = col[ty + kRY * a];
      } else if (tx > jj) {
        const T cb = col[tx];
#pragma unroll
        for (int a = 0; a < 32 * NB / kRY; ++a)
          if (a < nrem) acc[a] = fma(-col[ty + kRY * a], cb, acc[a]);
      }
    }
    if (tx < jn) {
#pragma unroll
      for (int a = 0; a < 32 * NB / kRY; ++a) {
        const int r = ty + kRY * a;
        if (a < nrem && r >= tx) S[(c0 + r) * KP + c0 + tx] = acc[a];
      }
    }
  }
  // L^T x = y, the panels last to first; x takes rhs's place
#pragma unroll 1
  for (int p = NB - 1; p >= 0; --p) {
    const int c0 = 32 * p, nr = k - c0, jn = min(32, nr);
    __syncthreads();  // L has been written back; the previous panel has been read
    for (int e = tid; e < nr * 32; e += kWThreads) {
      const int r = e >> 5, c = e & 31;
      P[r * kPLd + c] = (c < jn && r >= c) ? S[(c0 + r) * KP + c0 + c] : T(0);
    }
    __syncthreads();
    if (tid < jn) {  // the rows below the diagonal block: their x is known
      T s = y[c0 + tid];
      for (int r = nr - 1; r >= 32; --r) s = fma(-P[r * kPLd + tid], rhs[c0 + r], s);
      y[c0 + tid] = s;
    }
    __syncthreads();
    for (int jj = jn - 1; jj >= 0; --jj) {
      const T xj = y[c0 + jj] / P[jj * kPLd + jj];
      if (tid == jj) rhs[c0 + jj] = xj;
      else if (tid < jj) y[c0 + tid] = fma(-P[jj * kPLd + tid], xj, y[c0 + tid]);
      __syncthreads();
    }
  }
  if (tid < k) x_out[tid] = bad ? std::numeric_limits<T>::quiet_NaN() : rhs[tid];
}

// The row's system as finish_wide takes it, solved for x >= 0 by nnls_row over the slab.
template <typename T, int NB>
__device__ __forceinline__ void finish_wide_nnls(T* S, T* vec, T* rhs, int k, T* x_out, T* dump,
                                                 unsigned long long* stats) {
  constexpr int KP = 32 * NB;
  static_assert(6 * KP <= KP * kPLd, "nnls_row's vectors fit in the stage panel");
  const int tid = threadIdx.x;
  for (int e = tid; e < k * k; e += kWThreads) {
    const int i = e / k, j = e % k;
    if (j > i) S[i * KP + j] = S[j * KP + i];
  }
  nnls_row<T, kWThreads>(S, KP, rhs, vec, KP, k, x_out, dump, stats);
}

// LDS layout (elements of T): P[KP * 33] (first the gather tile, then the backward solve's panel),
// stage[KP * 33], rhs[KP], y[KP], col[KP], colraw[KP], rv[kTile], cf[kTile]
template <typename T>
constexpr size_t wide_lds_bytes(int kp) {
  return (static_cast<size_t>(2) * kp * kPLd + 4 * kp + 2 * kTile) * sizeof(T);
}

template <typename T, int KP>
struct WideLds {
  T *P, *stage, *rhs, *y, *col, *colraw, *rv, *cf;
  __device__ explicit WideLds(unsigned char* raw) {
    P = reinterpret_cast<T*>(raw);
    stage = P + KP * kPLd;
    rhs = stage + KP * kPLd;
    y = rhs + KP;
    col = y + KP;
    colraw = col + KP;
    rv = colraw + KP;
    cf = rv + kTile;
  }
};

// The work items blockIdx.x, blockIdx.x + gridDim.x, ... of the launch; W, G and alpha as in kernels_als.hip.
template <typename T, int NB, bool W, bool N = false>
__global__ __launch_bounds__(kWThreads) void k_als_wide(const AlsItem* __restrict__ items, int n_items,
                                                         const int32_t* __restrict__ cols, const T* __restrict__ vals,
                                                         const T* __restrict__ Q, T* __restrict__ X, int k, T lambda,
                                                         int weighted, T* __restrict__ partial, T* __restrict__ dump,
                                                         const T* __restrict__ G, T alpha, T* __restrict__ slab,
                                                         unsigned long long* __restrict__ nnls) {
  constexpr int KP = 32 * NB;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const WideLds<T, KP> L(smem_raw);
  T* M = L.P;
  T* S = slab + static_cast<size_t>(blockIdx.x) * KP * KP;
  for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
    __syncthreads();  // the previous item has left LDS
    // (an opaque copy per item: what is derived from it is not carried across finish_wide and spilled)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid) : : "memory");
    const AlsItem it = items[wi];
    if constexpr (W) {
      if (it.npos == 0 && !dump) {  // (a chunk of such a row stores no partial: the reduce reads none)
        if (it.slot < 0 && tid < k) X[static_cast<size_t>(it.row) * k + tid] = T(0);
        if constexpr (N) {
          if (it.slot < 0 && tid == 0) nnls_count_zero_row(nnls);
        }
        continue;
      }
    }
    WideAcc<T> g;
    g.zero();
    T bacc = T(0);
    for (int t0 = 0; t0 < it.count; t0 += kTile) {
      const int rows = min(kTile, it.count - t0);
      __syncthreads();  // the previous tile has been read
      int tg = tid;  // (opaque: the tile coordinates are formed per tile, not kept across the accumulation)
      asm volatile("" : "+v"(tg));
#pragma unroll 2
      for (int e = tg; e < kTile * KP; e += kWThreads) {
        const int t = e / KP, f = e % KP;
        T v = T(0);
        if (t < rows && f < k) v = Q[static_cast<size_t>(cols[it.begin + t0 + t]) * k + f];
        M[e] = v;
      }
      if constexpr (W) {
        if (tid < kTile) {
          const T r = tid < rows ? vals[it.begin + t0 + tid] : T(0);
          const T w = alpha * (r < T(0) ? -r : r);
          L.rv[tid] = w;
          L.cf[tid] = r > T(0) ? T(1) + w : T(0);
        }
      } else {
        if (tid < kTile) L.rv[tid] = tid < rows ? vals[it.begin + t0 + tid] : T(0);
      }
      __syncthreads();
      // (rows past the end are zero: the f32 path always runs whole pairs)
      g.template tile<NB, W>(tid, M, KP, (rows + 1) & ~1, L.rv);
      if constexpr (W) {
        if (tid < KP) {
#pragma unroll 4
          for (int t = 0; t < rows; ++t) {
            const T c = L.cf[t];
            if (c != T(0)) bacc = fma(c, M[t * KP + tid], bacc);  // r > 0 only
          }
        }
      } else {
        if (tid < KP) {
#pragma unroll 4
          for (int t = 0; t < rows; ++t) bacc = fma(L.rv[t], M[t * KP + tid], bacc);
        }
      }
    }
    // a chunk of a long row: the partial system goes to the scratch slab; a whole row: to the
    // workgroup's matrix.  (An opaque copy: the store addresses are formed here, not hoisted out of
    // the item loop and spilled.)
    T* D = it.slot >= 0 ? partial + static_cast<size_t>(it.slot) * (KP * KP + KP) : S;
    asm volatile("" : "+v"(D));
    g.template store<NB>(tid, D, KP);
    if (it.slot >= 0) {
      if (tid < KP) D[KP * KP + tid] = bacc;
      continue;
    }
    if (tid < KP) L.rhs[tid] = bacc;
    __syncthreads();
    if constexpr (W) {  // + G, in a pass of its own: the accumulators are dead by now
      for (int e = tid; e < KP * KP; e += kWThreads)
        if (e % KP <= e / KP) S[e] += G[e];
      __syncthreads();
    }
    const T lam = weighted ? lambda * static_cast<T>(W ? it.npos : it.count) : lambda;
    if (tid < k) S[tid * KP + tid] += lam;
    __syncthreads();
    if constexpr (N) finish_wide_nnls<T, NB>(S, L.stage, L.rhs, k, X + static_cast<size_t>(it.row) * k, dump, nnls);
    else finish_wide<T, NB>(S, L.P, L.stage, L.rhs, L.y, L.col, L.colraw, k, X + static_cast<size_t>(it.row) * k, dump);
  }
}

// The split rows blockIdx.x, blockIdx.x + gridDim.x, ...: partials [slot0, slot0 + chunks) added in
// ascending order into the slab.  W: plus G, once, after the partial sum; a row with no positive
// rating is set to zero.
template <typename T, int NB, bool W, bool N = false>
__global__ __launch_bounds__(kWThreads) void k_als_reduce_wide(const AlsSplit* __restrict__ rows, int n_rows,
                                                                const T* __restrict__ partial, T* __restrict__ X, int k,
                                                                T lambda, int weighted, T* __restrict__ dump,
                                                                const T* __restrict__ G, T* __restrict__ slab,
                                                                unsigned long long* __restrict__ nnls) {
  constexpr int KP = 32 * NB;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const WideLds<T, KP> L(smem_raw);
  T* S = slab + static_cast<size_t>(blockIdx.x) * KP * KP;
  const int tid = threadIdx.x;
  for (int wi = blockIdx.x; wi < n_rows; wi += gridDim.x) {
    __syncthreads();  // the previous row has left LDS
    const AlsSplit sp = rows[wi];
    if constexpr (W) {
      if (sp.npos == 0 && !dump) {
        if (tid < k) X[static_cast<size_t>(sp.row) * k + tid] = T(0);
        if constexpr (N) {
          if (tid == 0) nnls_count_zero_row(nnls);
        }
        continue;
      }
    }
    als_sum_partials<T, KP, kWThreads, W>(tid, sp, partial, G, S, KP, L.rhs);
    __syncthreads();
    const T lam = weighted ? lambda * static_cast<T>(W ? sp.npos : sp.count) : lambda;
    if (tid < k) S[tid * KP + tid] += lam;
    __syncthreads();
    if constexpr (N) finish_wide_nnls<T, NB>(S, L.stage, L.rhs, k, X + static_cast<size_t>(sp.row) * k, dump, nnls);
    else finish_wide<T, NB>(S, L.P, L.stage, L.rhs, L.y, L.col, L.colraw, k, X + static_cast<size_t>(sp.row) * k, dump);
  }
}

// k_als_gram of kernels_als.hip with the wide accumulators; the tile is dynamic LDS (64 KiB in f64
// at KP = 256).
template <typename T, int NB>
__global__ __launch_bounds__(kWThreads) void k_als_gram_wide(const int32_t* __restrict__ rated, int m, int slice,
                                                              const T* __restrict__ Y, int k, T* __restrict__ part) {
  constexpr int KP = 32 * NB;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const int tid = threadIdx.x;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * slice;
  const int64_t hi = min(static_cast<int64_t>(m), lo + slice);
  WideAcc<T> g;
  g.zero();
  for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
    const int rows = static_cast<int>(min(static_cast<int64_t>(kTile), hi - t0));
    __syncthreads();  // the previous tile has been read
    for (int e = tid; e < kTile * KP; e += kWThreads) {
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

// One launch of `grid` workgroups with `smem` bytes of dynamic LDS; the arguments are converted to the
// kernel's parameter types (the launch description holds void pointers and doubles).
template <typename... P, typename... A>
void launch_wide_kernel(void (*fn)(P...), int grid, size_t smem, hipStream_t st, A... args) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(smem)) != hipSuccess)
    fail(MF_ERR_HIP, "k_als_wide: " + std::to_string(smem) + " bytes of LDS refused");
  hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(grid)), dim3(kWThreads), smem, st, static_cast<P>(args)...);
}

}  // namespace

int als_wide_slabs(int k, bool f64, int cus) {
  if (k <= 128) return 0;
  return f64 ? cus : 2 * cus;  // the workgroups one CU's LDS holds at once (141 KiB f64, 70 KiB f32 at KP = 256)
}

void launch_als_wide(const AlsLaunch& L) {
  if (!L.slab || L.slabs <= 0) fail(MF_ERR_INVALID, "launch_als_wide: no matrix slabs");
  als_dispatch<5>(L.f64, L.gram != nullptr, L.k, [&](auto t, auto w, auto nb) {
    using T = decltype(t);
    constexpr int NB = decltype(nb)::value;
    constexpr bool W = decltype(w)::value;
    const size_t smem = wide_lds_bytes<T>(32 * NB);
    unsigned long long* stats = static_cast<unsigned long long*>(L.nnls_stats);
    auto run = [&](auto n) {
      constexpr bool N = decltype(n)::value;
      if (L.n_items > 0)
        launch_wide_kernel(&k_als_wide<T, NB, W, N>, std::min(L.n_items, L.slabs), smem, L.st, L.items, L.n_items,
                           L.cols, L.vals, L.Q, L.X, L.k, L.lambda, L.weighted, L.partial, L.dump, L.gram, L.alpha,
                           L.slab, stats);
      if (L.n_splits > 0)
        launch_wide_kernel(&k_als_reduce_wide<T, NB, W, N>, std::min(L.n_splits, L.slabs), smem, L.st, L.splits,
                           L.n_splits, L.partial, L.X, L.k, L.lambda, L.weighted, L.dump, L.gram, L.slab, stats);
    };
    L.nnls ? run(std::true_type()) : run(std::false_type());
  });
}

void launch_als_gram_wide(const AlsGramLaunch& L) {
  const int slices = als_gram_slices(L.m, L.slice);
  als_dispatch<5>(L.f64, false, L.k, [&](auto t, auto, auto nb) {
    using T = decltype(t);
    constexpr int NB = decltype(nb)::value;
    if (slices > 0)
      launch_wide_kernel(&k_als_gram_wide<T, NB>, slices, static_cast<size_t>(kTile) * 32 * NB * sizeof(T), L.st,
                         L.rated, L.m, L.slice, L.Y, L.k, L.part);
  });
}

}  // namespace mfhip

