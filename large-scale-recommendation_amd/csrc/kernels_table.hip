// kernels_table.hip -- what the table kernels share on the host side (kernels.hpp, "table kernels"): the
// identity array, the one rule for library temp storage, and the stable radix sort and exclusive scan that
// kernels_als_append.hip and kernels_als_remove.hip build their tables with.  Integer work only.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "common.hpp"
#include "csr_device.hpp"
#include "kernels.hpp"
#include "radix_sort_cfg.hpp"

namespace mfhip {
namespace {

static_assert(dev::kCsrThreads == kGridThreads, "grid_for counts in the tile walk's workgroup size");

__global__ void k_iota(int32_t* __restrict__ out, int64_t n) {
  for (int64_t x = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; x < n;
       x += static_cast<int64_t>(gridDim.x) * blockDim.x)
    out[x] = static_cast<int32_t>(x);
}

}  // namespace

void launch_iota(hipStream_t st, int32_t* out, int64_t n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_iota, dim3(grid_for(n)), dim3(kGridThreads), 0, st, out, n);
  MF_HIP(hipGetLastError());
}

void* temp_storage(hipStream_t st, DevBuf& buf, size_t bytes) {
  if (buf.get() && buf.bytes() >= bytes) return buf.get();
  if (buf.get()) MF_HIP(hipStreamSynchronize(st));  // work queued on st may still use the block that goes
  buf.alloc(std::max<size_t>(bytes, 256));
  return buf.get();
}

template <typename K>
void sort_positions(hipStream_t st, DevBuf& tmp, DevBuf& iota, const K* kin, K* kout, int32_t* pos, int64_t n,
                    int end_bit) {
  MF_REQUIRE(n > 0 && n < (int64_t{1} << 31), "sort_positions: positions are 32-bit");
  int32_t* const id = static_cast<int32_t*>(temp_storage(st, iota, static_cast<size_t>(n) * 4));
  launch_iota(st, id, n);
  const unsigned int N = static_cast<unsigned int>(n);
  size_t tb = 0;
  MF_HIP(rocprim::radix_sort_pairs<SortCfg>(nullptr, tb, kin, kout, id, pos, N, 0, end_bit, st));
  void* const t = temp_storage(st, tmp, tb);
  MF_HIP(rocprim::radix_sort_pairs<SortCfg>(t, tb, kin, kout, id, pos, N, 0, end_bit, st));
}
template void sort_positions(hipStream_t, DevBuf&, DevBuf&, const uint32_t*, uint32_t*, int32_t*, int64_t, int);
template void sort_positions(hipStream_t, DevBuf&, DevBuf&, const uint64_t*, uint64_t*, int32_t*, int64_t, int);

template <typename T>
void scan_exclusive(hipStream_t st, DevBuf& tmp, const T* in, T* out, int64_t n) {
  size_t tb = 0;
  MF_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, T(0), static_cast<size_t>(n), rocprim::plus<T>(), st));
  void* const t = temp_storage(st, tmp, tb);
  MF_HIP(rocprim::exclusive_scan(t, tb, in, out, T(0), static_cast<size_t>(n), rocprim::plus<T>(), st));
}
template void scan_exclusive(hipStream_t, DevBuf&, const int32_t*, int32_t*, int64_t);
template void scan_exclusive(hipStream_t, DevBuf&, const int64_t*, int64_t*, int64_t);

}  // namespace mfhip
