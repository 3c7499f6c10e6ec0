// rtm_grid_prims.hip — rocPRIM's exclusive scan and radix sort for the device grid build (rtm_grid_prims.h says why they have
// a translation unit of their own).  rocPRIM is header-only and ships with ROCm.
#include "rtm_grid_prims.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace rtm {

hipError_t grid_scan_counts(void* tmp, size_t& tmp_bytes, const unsigned* in, unsigned long long* out, size_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0ull, n, rocprim::plus<unsigned long long>(), stream);
}
hipError_t grid_scan_flags(void* tmp, size_t& tmp_bytes, const unsigned* in, unsigned* out, size_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, n, rocprim::plus<unsigned>(), stream);
}
hipError_t grid_sort_keys(void* tmp, size_t& tmp_bytes, const unsigned long long* in, unsigned long long* out, size_t n,
                          unsigned end_bit, hipStream_t stream) {
    return rocprim::radix_sort_keys(tmp, tmp_bytes, in, out, n, 0u, end_bit, stream);
}

}  // namespace rtm
