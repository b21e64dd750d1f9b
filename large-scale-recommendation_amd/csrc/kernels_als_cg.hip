// kernels_als_cg.hip -- ALS half-sweeps by conjugate gradients (mf_als_run_cg, mf_als_run_implicit_cg):
// every rated row of one side takes `steps` CG steps on its normal equations from its current value,
// and the k x k matrix of a row is never formed.  One code path for every rank 1..256, in f32 and f64.
//
//  A pass over a row's ratings j (counterpart rows q_j, CSR order) and a k-vector v computes
//      acc[f] = sum_j e_j q_j[f],   e_j = a coefficient of the rating r_j and of d_j = q_j . v:
//        kPassRes  e_j = r_j - d_j          (W: c_j - w_j d_j)    the residual b - A x without lambda' and G
//        kPassAp   e_j = d_j                (W: w_j d_j)          A p without lambda' and G
//        kPassB    e_j = r_j                (W: c_j)              b (the testing hook)
//      W (implicit feedback): w_j = alpha |r_j|, c_j = 1 + w_j where r_j > 0 and 0 elsewhere.
//  The vectors q_j stand in LDS, at most `cap` of them (what a fixed budget of 64 KiB holds at this k).
//  A whole row with count <= cap is staged once and all its passes run from LDS; a longer row gathers
//  cap vectors at a time in every pass.  The arithmetic is the same either way:
//      d_j      lane l of a wave takes f = l, l + 64, ... ascending (s = fma(q[f], v[f], s) from 0); the 64
//               lane sums are added by the butterfly xor 32, 16, 8, 4, 2, 1.  The waves take the ratings
//               of a tile of 64 in turn, four at a time (independent sums), and store e_j;
//      acc[f]   thread f: acc = fma(e_j, q_j[f], acc) from 0 over the ratings in CSR order;
//      (G v)[f] thread f: s = fma(G[g][f], v[g], s) from 0 over g = 0 .. k-1 (G is symmetric bit for bit);
//      r . r, p . Ap   thread f holds one product; wave sums by the butterfly, then ((w0 + w1) + w2) + w3.
//  The file is built without FP contraction: every fma above is written, every other operation is a
//  single rounding.
//
//  k_als_cg         one workgroup (4 waves) per whole row: residual, then `steps` steps, x stored once.
//  k_als_cg_chunk   one workgroup per chunk of a long row: one pass over the chunk, acc to partial[slot].
//  k_als_cg_update  one workgroup per long row: its partials added in ascending chunk order, then the
//                   same scalar update on the row's state (x, r, p, rs, status) in global memory.
//  No workgroup waits for another; every loop is bounded by a rating count, k or `steps`.
#include <hip/hip_runtime.h>

#include <limits>
#include <string>

#include "common.hpp"
#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kDTile = 64;                  // ratings whose coefficients are formed before they are used
constexpr size_t kCgLdsBytes = 64 * 1024;  // all LDS of a workgroup: two workgroups per CU
constexpr int kDots = 4;                    // ratings whose dot products one wave forms side by side
constexpr int kCgSmall = kAlsMaxRank + kDTile + 8;  // v, the tile's coefficients, the wave sums

enum : int { kPassRes = 0, kPassAp = 1, kPassB = 2 };
enum : int { kUpInit = 0, kUpStep = 1, kUpHookB = 2, kUpHookAv = 3 };
// status of a long row, kept as a T beside rs: still iterating, or finished (X holds its final value)
constexpr int kRunning = 0, kDone = 1;

template <typename T>
constexpr int cg_capacity(int k) {
  return static_cast<int>((kCgLdsBytes / sizeof(T) - kCgSmall) / static_cast<size_t>(k));
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// The sum of one value per thread, the same bits in every thread.  red: kWaves elements.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const T s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

template <typename T, bool W>
__device__ __forceinline__ T coef(int pass, T r, T dot, T alpha) {
  if constexpr (W) {
    const T w = alpha * (r < T(0) ? -r : r);
    const T c = r > T(0) ? T(1) + w : T(0);
    if (pass == kPassB) return c;
    if (pass == kPassAp) return w * dot;
    return c - w * dot;
  } else {
    if (pass == kPassB) return r;
    if (pass == kPassAp) return dot;
    return r - dot;
  }
}

// qs[j * k + f] = the counterpart row of rating first + j, j < rows.  A wave moves kGather rows at a time,
// so that many row reads are in flight behind one read of their column indices.
constexpr int kGather = 8;
template <typename T>
__device__ __forceinline__ void gather(const int32_t* __restrict__ cols, const T* __restrict__ Q, int64_t first,
                                       int rows, int k, T* __restrict__ qs) {
  const int tid = threadIdx.x;
  if (k >= 64) {
    for (int j0 = (tid >> 6) * kGather; j0 < rows; j0 += kWaves * kGather) {
      const T* src[kGather];
#pragma unroll
      for (int u = 0; u < kGather; ++u) src[u] = Q + static_cast<size_t>(cols[first + min(j0 + u, rows - 1)]) * k;
      for (int f = tid & 63; f < k; f += 64) {
        T v[kGather];
#pragma unroll
        for (int u = 0; u < kGather; ++u) v[u] = src[u][f];
#pragma unroll
        for (int u = 0; u < kGather; ++u)
          if (j0 + u < rows) qs[(j0 + u) * k + f] = v[u];
      }
    }
  } else {
    for (int e = tid; e < rows * k; e += kThreads) {
      const int j = e / k;
      qs[e] = Q[static_cast<size_t>(cols[first + j]) * k + (e - j * k)];
    }
  }
}

// One pass over ratings [begin, begin + n): thread f < k returns acc[f].  vs holds v (written by the
// caller before the call, no barrier needed); staged: qs already holds all n vectors.
template <typename T, bool W>
__device__ __forceinline__ T row_pass(int pass, const int32_t* __restrict__ cols, const T* __restrict__ vals,
                                      const T* __restrict__ Q, int64_t begin, int n, int k, int cap, bool staged,
                                      T alpha, const T* vs, T* d, T* qs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T acc = T(0);
  for (int c0 = 0; c0 < n; c0 += cap) {
    const int rows = min(cap, n - c0);
    if (!staged) {
      __syncthreads();  // the previous vectors have been read
      gather(cols, Q, begin + c0, rows, k, qs);
    }
    __syncthreads();
    for (int t0 = 0; t0 < rows; t0 += kDTile) {
      const int tr = min(kDTile, rows - t0);
      // a wave takes kDots ratings at a time: independent sums, each in the order of the file comment
      for (int j0 = wave * kDots; j0 < tr; j0 += kWaves * kDots) {
        T s[kDots];
#pragma unroll
        for (int u = 0; u < kDots; ++u) s[u] = T(0);
        if (pass != kPassB) {
          for (int f = lane; f < k; f += 64) {
            const T v = vs[f];
#pragma unroll
            for (int u = 0; u < kDots; ++u) s[u] = fma(qs[(t0 + min(j0 + u, tr - 1)) * k + f], v, s[u]);
          }
          for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
            for (int u = 0; u < kDots; ++u) s[u] += __shfl_xor(s[u], m, 64);
          }
        }
#pragma unroll
        for (int u = 0; u < kDots; ++u)
          if (lane == u && j0 + u < tr) d[j0 + u] = coef<T, W>(pass, vals[begin + c0 + t0 + j0 + u], s[u], alpha);
      }
      __syncthreads();
      if (tid < k)
        for (int j = 0; j < tr; ++j) acc = fma(d[j], qs[(t0 + j) * k + tid], acc);
      __syncthreads();
    }
  }
  return acc;
}

template <typename T>
__device__ __forceinline__ T gram_mv(const T* __restrict__ G, int kp, int k, const T* vs) {
  T s = T(0);
  if (static_cast<int>(threadIdx.x) < k)
    for (int g = 0; g < k; ++g) s = fma(G[static_cast<size_t>(g) * kp + threadIdx.x], vs[g], s);
  return s;
}

template <typename T>
__device__ __forceinline__ bool finite(T v) {
  return v - v == T(0);
}

template <typename T, bool W>
__global__ __launch_bounds__(kThreads) void k_als_cg(const AlsItem* __restrict__ items,
                                                      const int32_t* __restrict__ cols, const T* __restrict__ vals,
                                                      const T* __restrict__ Q, T* __restrict__ X, int k, T lambda,
                                                      int weighted, int steps, int cap, int stage,
                                                      const T* __restrict__ G, T alpha, const T* __restrict__ hook_v,
                                                      T* __restrict__ dump) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* vs = reinterpret_cast<T*>(smem_raw);
  T* d = vs + kAlsMaxRank;
  T* red = d + kDTile;
  T* qs = vs + kCgSmall;
  const AlsItem it = items[blockIdx.x];
  if (it.slot >= 0) return;  // a chunk of a long row: k_als_cg_chunk
  const int tid = threadIdx.x;
  const bool mine = tid < k;
  T* xrow = X + static_cast<size_t>(it.row) * k;
  if constexpr (W) {
    if (it.npos == 0 && !dump) {
      if (mine) xrow[tid] = T(0);
      return;
    }
  }
  const bool staged = stage && it.count <= cap;
  const int kp = (k + 31) / 32 * 32;
  const T lam = weighted ? lambda * static_cast<T>(W ? it.npos : it.count) : lambda;
  T x = T(0);
  if (mine) x = dump ? hook_v[tid] : xrow[tid];
  if (mine) vs[tid] = x;
  if (staged) gather(cols, Q, it.begin, it.count, k, qs);
  // A v for the v in vs, whose own element is `mine_v`: the hook's and the iteration's one code
  auto apply_a = [&](T mine_v) {
    T av = row_pass<T, W>(kPassAp, cols, vals, Q, it.begin, it.count, k, cap, staged, alpha, vs, d, qs);
    if constexpr (W) av += gram_mv(G, kp, k, vs);
    av += lam * mine_v;
    return av;
  };
  if (dump) {  // the testing hook: b and A v, v = hook_v
    const T b = row_pass<T, W>(kPassB, cols, vals, Q, it.begin, it.count, k, cap, staged, alpha, vs, d, qs);
    const T av = apply_a(x);
    if (mine) {
      dump[tid] = av;
      dump[k + tid] = b;
    }
    return;
  }
  T r = row_pass<T, W>(kPassRes, cols, vals, Q, it.begin, it.count, k, cap, staged, alpha, vs, d, qs);
  if constexpr (W) r -= gram_mv(G, kp, k, vs);
  r -= lam * x;
  T p = r;
  T rs = block_sum(r * r, red);
  bool bad = false;
  for (int s = 0; s < steps; ++s) {
    if (!finite(rs)) {
      bad = true;
      break;
    }
    if (rs == T(0)) break;
    if (mine) vs[tid] = p;  // (the barriers of block_sum lie between the last read of vs and this)
    const T ap = apply_a(p);
    const T pap = block_sum(p * ap, red);
    if (!finite(pap)) {
      bad = true;
      break;
    }
    if (pap == T(0)) break;
    const T a = rs / pap;
    x = fma(a, p, x);
    r = fma(-a, ap, r);
    const T rsn = block_sum(r * r, red);
    p = fma(rsn / rs, p, r);
    rs = rsn;
  }
  if (!finite(rs)) bad = true;
  if (mine) xrow[tid] = bad ? std::numeric_limits<T>::quiet_NaN() : x;
}

// One chunk of a long row: work[b] = (its item, its row's index among the launch's long rows).  The
// vector v is x as the model holds it (kPassRes) or the p of the row's state (kPassAp).
template <typename T, bool W>
__global__ __launch_bounds__(kThreads) void k_als_cg_chunk(const AlsCgWork* __restrict__ work,
                                                            const AlsItem* __restrict__ items,
                                                            const int32_t* __restrict__ cols,
                                                            const T* __restrict__ vals, const T* __restrict__ Q,
                                                            const T* __restrict__ X, int k, int cap, T alpha, int pass,
                                                            int hook, const T* __restrict__ state,
                                                            T* __restrict__ partial, size_t pstride) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* vs = reinterpret_cast<T*>(smem_raw);
  T* d = vs + kAlsMaxRank;
  T* qs = vs + kCgSmall;
  const AlsCgWork w = work[blockIdx.x];
  const AlsItem it = items[w.item];
  const int tid = threadIdx.x;
  const int kp = (k + 31) / 32 * 32;
  const T* st = state + static_cast<size_t>(w.split) * (4 * kp);
  if constexpr (W) {
    if (it.npos == 0 && !hook) return;
  }
  if (pass == kPassAp && st[3 * kp + 1] != T(kRunning)) return;
  if (tid < k) {
    if (pass == kPassRes) vs[tid] = X[static_cast<size_t>(it.row) * k + tid];
    if (pass == kPassAp) vs[tid] = st[2 * kp + tid];
  }
  const T acc = row_pass<T, W>(pass, cols, vals, Q, it.begin, it.count, k, cap, false, alpha, vs, d, qs);
  if (tid < k) partial[static_cast<size_t>(it.slot) * pstride + tid] = acc;
}

// One long row: the chunks' partials in ascending order, then the update.  state: x | r | p | rs, status,
// 4 * KP elements per row of the launch.
template <typename T, bool W>
__global__ __launch_bounds__(kThreads) void k_als_cg_update(const AlsSplit* __restrict__ rows,
                                                             const T* __restrict__ partial, size_t pstride,
                                                             T* __restrict__ X, int k, T lambda, int weighted,
                                                             const T* __restrict__ G, T* __restrict__ state, int mode,
                                                             int last, T* __restrict__ dump) {
  __shared__ T vs[kAlsMaxRank];
  __shared__ T red[kWaves];
  const AlsSplit sp = rows[blockIdx.x];
  const int tid = threadIdx.x;
  const bool mine = tid < k;
  const int kp = (k + 31) / 32 * 32;
  T* st = state + static_cast<size_t>(blockIdx.x) * (4 * kp);
  T* scal = st + 3 * kp;
  T* xrow = X + static_cast<size_t>(sp.row) * k;
  const T nan = std::numeric_limits<T>::quiet_NaN();
  if (mode == kUpStep && scal[1] != T(kRunning)) return;
  if constexpr (W) {
    if (sp.npos == 0 && mode == kUpInit) {
      if (mine) xrow[tid] = T(0);
      if (tid == 0) scal[1] = T(kDone);
      return;
    }
  }
  T sum = T(0);
  if (mine)
    for (int c = 0; c < sp.chunks; ++c) sum += partial[(static_cast<size_t>(sp.slot0) + c) * pstride + tid];
  const T lam = weighted ? lambda * static_cast<T>(W ? sp.npos : sp.count) : lambda;
  if (mode == kUpHookB) {
    if (mine) dump[k + tid] = sum;
    if (tid == 0) scal[1] = T(kRunning);
    return;
  }
  if (mode == kUpInit) {
    const T x = mine ? xrow[tid] : T(0);
    if (mine) vs[tid] = x;
    __syncthreads();
    T r = sum;
    if constexpr (W) r -= gram_mv(G, kp, k, vs);
    r -= lam * x;
    const T rs = block_sum(r * r, red);
    if (mine) {
      st[tid] = x;
      st[kp + tid] = r;
      st[2 * kp + tid] = r;
      if (!finite(rs)) xrow[tid] = nan;
    }
    if (tid == 0) {
      scal[0] = rs;
      scal[1] = T(finite(rs) && rs != T(0) ? kRunning : kDone);
    }
    return;
  }
  T x = T(0), r = T(0), p = T(0);
  if (mine) {
    x = st[tid];
    r = st[kp + tid];
    p = st[2 * kp + tid];
    vs[tid] = p;
  }
  const T rs = scal[0];
  __syncthreads();
  T ap = sum;
  if constexpr (W) ap += gram_mv(G, kp, k, vs);
  ap += lam * p;
  if (mode == kUpHookAv) {
    if (mine) dump[tid] = ap;
    return;
  }
  const T pap = block_sum(p * ap, red);
  if (!finite(pap) || pap == T(0)) {
    if (mine) xrow[tid] = finite(pap) ? x : nan;
    if (tid == 0) scal[1] = T(kDone);
    return;
  }
  const T a = rs / pap;
  x = fma(a, p, x);
  r = fma(-a, ap, r);
  const T rsn = block_sum(r * r, red);
  p = fma(rsn / rs, p, r);
  const bool done = last || !finite(rsn) || rsn == T(0);
  if (mine) {
    st[tid] = x;
    st[kp + tid] = r;
    st[2 * kp + tid] = p;
    if (done) xrow[tid] = finite(rsn) ? x : nan;
  }
  if (tid == 0) {
    scal[0] = rsn;
    if (done) scal[1] = T(kDone);
  }
}

template <typename T, bool W>
void launch_cg(const AlsLaunch& L) {
  const hipStream_t st = L.st;
  const T* vals = static_cast<const T*>(L.vals);
  const T* Q = static_cast<const T*>(L.Q);
  T* X = static_cast<T*>(L.X);
  T* partial = static_cast<T*>(L.partial);
  T* state = static_cast<T*>(L.state);
  T* dump = static_cast<T*>(L.dump);
  const T* G = static_cast<const T*>(L.gram);
  const T lam = static_cast<T>(L.lambda), al = static_cast<T>(L.alpha);
  const int k = L.k, steps = L.steps, weighted = L.weighted ? 1 : 0;
  const int cap = cg_capacity<T>(k);
  const size_t pstride = als_partial_elems(k);
  const int kp = (k + 31) / 32 * 32;
  const dim3 block(kThreads), gi(static_cast<unsigned>(L.n_items)), gw(static_cast<unsigned>(L.n_work)),
      gs(static_cast<unsigned>(L.n_splits));
  if (L.n_items > 0)
    hipLaunchKernelGGL((k_als_cg<T, W>), gi, block, kCgLdsBytes, st, L.items, L.cols, vals, Q, X, k, lam, weighted, steps,
                       cap, L.stage ? 1 : 0, G, al, static_cast<const T*>(L.hook_v), dump);
  if (L.n_work == 0 || L.n_splits == 0) return;
  auto chunk = [&](int pass) {
    hipLaunchKernelGGL((k_als_cg_chunk<T, W>), gw, block, kCgLdsBytes, st, L.work, L.items, L.cols, vals, Q, X, k, cap, al,
                       pass, dump ? 1 : 0, state, partial, pstride);
  };
  auto update = [&](int mode, int last) {
    hipLaunchKernelGGL((k_als_cg_update<T, W>), gs, block, 0, st, L.splits, partial, pstride, X, k, lam, weighted, G,
                       state, mode, last, dump);
  };
  if (dump) {  // one long row: v becomes the p of its state
    if (hipMemcpyAsync(state + 2 * kp, L.hook_v, static_cast<size_t>(k) * sizeof(T), hipMemcpyDeviceToDevice, st) !=
        hipSuccess)
      fail(MF_ERR_HIP, "k_als_cg: the hook's vector could not be copied");
    chunk(kPassB);
    update(kUpHookB, 0);
    chunk(kPassAp);
    update(kUpHookAv, 0);
    return;
  }
  chunk(kPassRes);
  update(kUpInit, 0);
  for (int s = 0; s < steps; ++s) {
    chunk(kPassAp);
    update(kUpStep, s == steps - 1 ? 1 : 0);
  }
}

}  // namespace

size_t als_cg_state_elems(int k) { return 4 * static_cast<size_t>((k + 31) / 32 * 32); }

int als_cg_capacity(int k, bool f64) { return f64 ? cg_capacity<double>(k) : cg_capacity<float>(k); }

void launch_als_cg(const AlsLaunch& L) {
  if (L.k < 1 || L.k > kAlsMaxRank) als_refuse_rank();
  als_dispatch(L.f64, L.gram != nullptr, [&](auto t, auto w) { launch_cg<decltype(t), decltype(w)::value>(L); });
}

}  // namespace mfhip
