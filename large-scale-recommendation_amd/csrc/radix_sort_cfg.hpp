// radix_sort_cfg.hpp -- the configuration of every stable rocprim radix sort of the library
// (kernels_table.hip's sort_positions, kernels_online.hip's plan sorts).
#pragma once

#include <rocprim/device/device_radix_sort.hpp>

namespace mfhip {

// rocprim's radix sort with the merge-sort path off.  Its default config sorts up to 2^20 keys by block
// sort + 8 merge passes (17 launches of 5-10 us for a 1M batch); onesweep takes a histogram, a scan and one
// pass per 8 key bits.  Both are stable: the same output.
using SortCfg =
    rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;

}  // namespace mfhip
