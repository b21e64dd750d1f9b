// als_device.hpp -- the device pieces the two Cholesky ALS kernel files share (kernels_als.hip at
// ranks 1..128, kernels_als_wide.hip at 129..256): the f32 accumulation on the matrix cores, the sum
// of a split row's partials and the testing hook's dump.  THREADS is the workgroup size, KP = 32 NB the
// padded rank; tid is the caller's (possibly opaque) copy of threadIdx.x.  Included by those two files
// only.  The tile loop's own steps (gather, staging of the ratings, right-hand side) stay written out in
// each item kernel: as shared functions they kept every resource figure but moved the scalar code of the
// loop, and the f32 half-sweep at k = 128 measured 0.5 to 0.9 % slower.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mfhip {
namespace {

constexpr int kTile = 32;  // ratings per LDS tile (a multiple of 2: one MFMA takes two ratings)

typedef float v16f __attribute__((ext_vector_type(16)));

// block number b -> (bi, bj), bj <= bi, row-major over the triangle
__device__ __forceinline__ void block_of(int b, int& bi, int& bj) {
  bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= b) ++bi;  // bi <= 7
  bj = b - bi * (bi + 1) / 2;
}

// f32 Gram accumulation (v_mfma_f32_32x32x2_f32): the lower-triangle 32 x 32 blocks w, w + WAVES, ...
// of wave w, at most MAX of them, 16 accumulator registers per lane each.
template <int WAVES, int MAX>
struct MfmaAcc {
  v16f acc[MAX];
  __device__ void zero() {
#pragma unroll
    for (int x = 0; x < MAX; ++x)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][r] = 0.f;
  }
  // W: w[t] (LDS) multiplies rating t's A operand
  template <int NB, bool W = false>
  __device__ void tile(int tid, const float* q, int kp, int rows, const float* w = nullptr) {
    constexpr int kBlocks = NB * (NB + 1) / 2;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, c = lane & 31;
#pragma unroll
    for (int x = 0; x < MAX; ++x) {
      const int b = wave + WAVES * x;
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
  __device__ void store(int tid, float* M, int ld, const float* G = nullptr) const {
    constexpr int kBlocks = NB * (NB + 1) / 2;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, c = lane & 31;
#pragma unroll
    for (int x = 0; x < MAX; ++x) {
      const int b = wave + WAVES * x;
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

// A split row's partials [slot0, slot0 + chunks) added in ascending order: the lower triangle into A
// (row stride ld), the right-hand side into rhs.  W: plus G, once, after the partial sum.
template <typename T, int KP, int THREADS, bool W>
__device__ __forceinline__ void als_sum_partials(int tid, const AlsSplit& sp, const T* __restrict__ partial,
                                                 const T* __restrict__ G, T* A, int ld, T* rhs) {
  constexpr size_t kStride = static_cast<size_t>(KP) * KP + KP;
  for (int e = tid; e < KP * KP + KP; e += THREADS) {
    const int i = e / KP, j = e % KP;
    if (i < KP && j > i) continue;  // only the lower triangle is defined
    T sum = T(0);
    for (int c = 0; c < sp.chunks; ++c) sum += partial[(static_cast<size_t>(sp.slot0) + c) * kStride + e];
    if constexpr (W) {
      if (i < KP) sum += G[e];
    }
    if (i < KP) A[i * ld + j] = sum;
    else rhs[j] = sum;
  }
}

// The testing hook: the full symmetric k x k of A (lower triangle valid, row stride ld), then rhs.
template <typename T, int THREADS>
__device__ __forceinline__ void als_dump_system(int tid, const T* A, int ld, const T* rhs, int k, T* dump) {
  for (int e = tid; e < k * k; e += THREADS) {
    const int i = e / k, j = e % k;
    dump[e] = i >= j ? A[i * ld + j] : A[j * ld + i];
  }
  if (tid < k) dump[k * k + tid] = rhs[tid];
}

}  // namespace
}  // namespace mfhip
