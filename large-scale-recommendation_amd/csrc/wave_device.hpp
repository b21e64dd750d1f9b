// wave_device.hpp -- the gfx950 wave primitives the sweep kernels share, one definition each: lane
// reads, the DPP move, raw-buffer resources, vmcnt waits (the s_waitcnt layout) and the 16-B store
// with its hazard wait.  No floating-point arithmetic lives here: some kernel files are built with
// -ffp-contract=off and some are not, so a shared add or multiply would mean different things in
// different files (which is why the wave sums stay with their kernels).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "plan.hpp"

namespace mfhip::dev {

typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// Lane reads (v_readlane_b32): lane l's value, wave-uniform.
__device__ __forceinline__ uint32_t rl(uint32_t v, int l) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), l));
}
__device__ __forceinline__ float rlf(float v, int l) { return __uint_as_float(rl(__float_as_uint(v), l)); }
__device__ __forceinline__ double rld(double v, int l) {
  const uint64_t b = static_cast<uint64_t>(__double_as_longlong(v));
  const uint64_t lo = rl(static_cast<uint32_t>(b), l), hi = rl(static_cast<uint32_t>(b >> 32), l);
  return __longlong_as_double(static_cast<long long>((hi << 32) | lo));
}

// v as the DPP control CTRL moves it between lanes (every row and bank enabled)
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Cache policy of a buffer access: 0 = plain; kSC1 = sc1 (L1 bypass on loads, write-through and
// dropped from the XCD's L2 on stores), used for rows and tickets handed between waves inside one
// launch (MI355X_MICROARCH.md, inter-workgroup visibility, valid forms).
constexpr int kSC1 = 16;

// `bytes` from `base` as a raw buffer (a load past its end returns 0, a store is dropped), clamped to `limit`:
// kSlabLimit keeps the row offset kOffOOB (plan.hpp) out of range; kernels_fast.hip uses no such offset.
constexpr uint32_t kWholeRange = 0xFFFFFFFFu;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_rsrc(const void* base, uint64_t bytes,
                                                            uint32_t limit = kSlabLimit) {
  const uint32_t n = bytes > limit ? limit : static_cast<uint32_t>(bytes);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}

// s_waitcnt vmcnt(N) the compiler can see: at most N vector-memory operations of the wave still in
// flight.  gfx9 encoding: vmcnt in bits 0-3 and 14-15; 0x0F70 leaves expcnt and lgkmcnt unconstrained.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}

// A 16-B buffer store, then two wait states before its data VGPRs can be rewritten.  gfx950
// reads a store's data after issuing it: a VALU that overwrites the data VGPRs right behind a
// buffer_store_dwordx4 corrupts the stored row under load -- 1.2% of 16-B records with the offset
// in an SGPR and no wait state, 1.5% with soffset 0 and one wait state, none with two
// (tools/micro/store_data_hazard.hip, profiles/r05_store_data_hazard.txt).  LLVM pads one wait
// state, and none at all when soffset is an SGPR (the table's exemption), so the round-4 k = 256
// lean sweep, whose compiler reused the data VGPRs one or two instructions after the store, wrote
// torn user rows: it did not repeat itself and biased RMSE by 0.27%.  The s_nop below takes the
// data as operands, so no instruction can rewrite those VGPRs before it, and it is ordered after
// the store (both have side effects).  tests/test_isa.py checks every wide store of the library.
// policy: 0 or kSC1 (the builtin takes it as an immediate).
__device__ __forceinline__ void store_b128(u4v d, __amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff, int policy) {
  if (policy == kSC1) __builtin_amdgcn_raw_buffer_store_b128(d, rs, voff, soff, kSC1);
  else __builtin_amdgcn_raw_buffer_store_b128(d, rs, voff, soff, 0);
  asm volatile("s_nop 1" ::"v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]));
}

}  // namespace mfhip::dev
