// rec_keys.hpp -- the selection keys of the top-N kernels (kernels_recommend.hip, kernels_among.hip): what
// defines mf_recommend's order bit for bit.  A key orders by score descending, then candidate id ascending
// (signed), NaN below every number, -0 as +0 -- one unsigned compare; the all-zero key is the empty slot.
// A list is N keys sorted descending.
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

}  // namespace mfhip::dev
