// rec_keys.hpp -- the selection keys of the top-N kernels (kernels_recommend.hip, kernels_among.hip): what
// defines mf_recommend's order bit for bit.  A key orders by score descending, then candidate id ascending
// (signed), NaN below every number, -0 as +0 -- one unsigned compare; the all-zero key is the empty slot.
// A list is N keys sorted descending.  With the keys: the insertions into a list, one lane's and a wave's, and
// the merge of partial lists (k_rec_merge), one definition each.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfhip::dev {

// Candidate id part: a smaller id gives a larger value.
__device__ __forceinline__ uint32_t id_bits(int32_t id) { return ~(static_cast<uint32_t>(id) ^ 0x80000000u); }
__device__ __forceinline__ int32_t id_from_bits(uint32_t b) { return static_cast<int32_t>((~b) ^ 0x80000000u); }

// f32: (order-preserving u32 of the score) << 32 | id part.  The score part is >= 1 for every real
// key (1 = NaN, which no number maps to), so 0 is the empty slot.  -0 orders as +0.
struct Key32 {
  uint64_t v;
};
__device__ __forceinline__ bool key_gt(Key32 a, Key32 b) { return a.v > b.v; }
__device__ __forceinline__ bool key_empty(Key32 a) { return a.v == 0; }
__device__ __forceinline__ uint32_t ord32(float s) {
  if (s != s) return 1u;
  if (s == 0.0f) return 0x80000000u;
  const uint32_t b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ Key32 make_key(float s, int32_t id) {
  return Key32{(static_cast<uint64_t>(ord32(s)) << 32) | id_bits(id)};
}
__device__ __forceinline__ double key_score(Key32 k) {
  const uint32_t o = static_cast<uint32_t>(k.v >> 32);
  if (o == 1u) return __longlong_as_double(0x7ff8000000000000LL);
  const uint32_t b = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  return static_cast<double>(__uint_as_float(b));
}
__device__ __forceinline__ int32_t key_id(Key32 k) { return id_from_bits(static_cast<uint32_t>(k.v)); }
__device__ __forceinline__ Key32 key_shfl_xor(Key32 k, int m) {
  const uint32_t lo = __shfl_xor(static_cast<uint32_t>(k.v), m), hi = __shfl_xor(static_cast<uint32_t>(k.v >> 32), m);
  return Key32{(static_cast<uint64_t>(hi) << 32) | lo};
}

// f64: the same with a 64-bit score part (hi) and the id part in lo.
struct Key64 {
  uint64_t hi, lo;
};
__device__ __forceinline__ bool key_gt(Key64 a, Key64 b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
__device__ __forceinline__ bool key_empty(Key64 a) { return a.hi == 0; }
__device__ __forceinline__ Key64 make_key(double s, int32_t id) {
  uint64_t o;
  if (s != s) o = 1u;
  else if (s == 0.0) o = 0x8000000000000000ULL;
  else {
    const uint64_t b = static_cast<uint64_t>(__double_as_longlong(s));
    o = (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
  }
  return Key64{o, id_bits(id)};
}
__device__ __forceinline__ double key_score(Key64 k) {
  if (k.hi == 1u) return __longlong_as_double(0x7ff8000000000000LL);
  const uint64_t b = (k.hi >> 63) ? (k.hi ^ 0x8000000000000000ULL) : ~k.hi;
  return __longlong_as_double(static_cast<long long>(b));
}
__device__ __forceinline__ int32_t key_id(Key64 k) { return id_from_bits(static_cast<uint32_t>(k.lo)); }
__device__ __forceinline__ Key64 key_shfl_xor(Key64 k, int m) {
  const Key32 a = key_shfl_xor(Key32{k.hi}, m), b = key_shfl_xor(Key32{k.lo}, m);
  return Key64{a.v, b.v};
}

// list[0..N) sorted descending, key beats list[N-1]: insert it, dropping the last.
template <typename K>
__device__ __forceinline__ void list_insert(K* list, int N, K key) {
  int p = N - 1;
  while (p > 0 && key_gt(key, list[p - 1])) {
    list[p] = list[p - 1];
    --p;
  }
  list[p] = key;
}

// The same for a caller whose candidates may repeat (kernels_among.hip): a key the list already holds is the
// same candidate named twice and is not inserted.  Exact: a key that left the list is below its N-th key,
// which only rises, so it never passes the caller's test against list[N-1] again.
template <typename K>
__device__ __forceinline__ void list_insert_distinct(K* list, int N, K key) {
  int p = N - 1;  // the place: the first slot whose key does not beat `key`
  while (p > 0 && !key_gt(list[p - 1], key)) --p;
  if (!key_gt(key, list[p])) return;  // equal (list[p] does not beat key, key does not beat list[p])
  for (int x = N - 1; x > p; --x) list[x] = list[x - 1];
  list[p] = key;
}

// The lanes of a wave exchange data through LDS without a workgroup barrier: order the wave's own LDS accesses.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One lane at a time inserts into the list its wave shares (k_rec_f64, k_among_score): per round the first lane
// that still wants to and whose key still beats the N-th.  DISTINCT: candidates may repeat (list_insert_distinct).
template <bool DISTINCT, typename K>
__device__ __forceinline__ void wave_list_insert(K* list, int N, K key, bool want, int lane) {
  for (;;) {
    want = want && key_gt(key, list[N - 1]);
    const uint64_t m = __ballot(want);
    if (m == 0) break;
    if (lane == __ffsll(static_cast<long long>(m)) - 1) {
      if constexpr (DISTINCT) list_insert_distinct(list, N, key);
      else list_insert(list, N, key);
      want = false;
    }
    wave_lds_sync();
  }
}

// The partial lists of a query -> its final top N.  One wave per query: lane l < S holds the head of the
// query's l-th partial list (each sorted descending, keys distinct inside it); N rounds of a wave-wide
// maximum.  The lists are parts [q * S, (q + 1) * S) of `part`, or with pbeg (nq + 1 offsets, at most 64
// parts a query) parts [pbeg[q], pbeg[q + 1]).  Every lane whose head equals the round's maximum advances, so
// an id that two parts both kept (mf_recommend_among: a list may name a candidate twice) counts once; where
// the parts are disjoint candidate splits exactly one lane holds the maximum.  Slots past the count hold
// id 0 / score 0.0.  scores may be null.  No floating-point arithmetic: the same code in every file.
template <typename K>
__global__ __launch_bounds__(256) void k_rec_merge(const K* __restrict__ part, const int64_t* __restrict__ pbeg,
                                                   int nq, int S, int N, int32_t* __restrict__ ids,
                                                   double* __restrict__ scores, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  int64_t p0 = static_cast<int64_t>(q) * S;
  if (pbeg != nullptr) {
    p0 = pbeg[q];
    S = static_cast<int>(pbeg[q + 1] - p0);
  }
  const K* mine = part + (p0 + lane) * N;
  int pos = 0;
  int cnt = 0;
  for (int o = 0; o < N; ++o) {
    K head{};
    if (lane < S && pos < N) head = mine[pos];
    K best = head;
    for (int m = 1; m < 64; m <<= 1) {
      const K other = key_shfl_xor(best, m);
      if (key_gt(other, best)) best = other;
    }
    const bool live = !key_empty(best);
    if (live && lane < S && pos < N && !key_gt(best, head) && !key_gt(head, best)) ++pos;
    if (lane == 0) {
      ids[static_cast<int64_t>(q) * N + o] = live ? key_id(best) : 0;
      if (scores) scores[static_cast<int64_t>(q) * N + o] = live ? key_score(best) : 0.0;
    }
    cnt += live ? 1 : 0;
  }
  if (lane == 0) counts[q] = cnt;
}

}  // namespace mfhip::dev
