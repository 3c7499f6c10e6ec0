// rtm_grid_prims.h — the two library primitives of the device grid build (rtm_grid_build.hip): rocPRIM's exclusive scan and
// radix sort, instantiated in a translation unit of their own (rtm_grid_prims.hip).  Not in rtm_kernels.hip: with rocPRIM's
// kernels in that unit the compiler made other instructions for the wave shuffles of 93 kernels that were there before, the
// render kernels among them — the same values, but not the code that was measured.
// Each call follows rocPRIM's convention: with tmp == nullptr it only sets tmp_bytes; else it enqueues on `stream`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rtm {
// out[i] = in[0] + ... + in[i - 1] as 64-bit sums
hipError_t grid_scan_counts(void* tmp, size_t& tmp_bytes, const unsigned* in, unsigned long long* out, size_t n, hipStream_t stream);
// ... as 32-bit sums (the flags of at most 2^31 spheres)
hipError_t grid_scan_flags(void* tmp, size_t& tmp_bytes, const unsigned* in, unsigned* out, size_t n, hipStream_t stream);
// out = in sorted ascending by bits [0, end_bit)
hipError_t grid_sort_keys(void* tmp, size_t& tmp_bytes, const unsigned long long* in, unsigned long long* out, size_t n,
                          unsigned end_bit, hipStream_t stream);
}  // namespace rtm
