// rtm_compare.hip — rtm_compare / rtm_compare_work_bytes (include/rtm.h): argument checks, the work buffer's layout and the
// launches of rtm_compare_kernel.h.  The call keeps no state: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_host.h"
#include "rtm_compare_kernel.h"

namespace rtm {

namespace {
constexpr size_t kCmpAlign = 256;  // work_dev's alignment and the size of its last part

size_t cmp_tiles_x(int32_t width) { return ((size_t)width + kCmpTile - 1) / kCmpTile; }
size_t cmp_tiles(int32_t width, int32_t height) { return cmp_tiles_x(width) * (((size_t)height + kCmpTile - 1) / kCmpTile); }
size_t cmp_partial_bytes(size_t tiles) { return (tiles * sizeof(CmpPartial) + kCmpAlign - 1) / kCmpAlign * kCmpAlign; }

template <typename T>
using PartialKernel = void (*)(CmpArgs, const T*, const T*, CmpPartial*, float*);

// with_result: the SSIM mean is part of the record, so the window passes always run; a map-only call runs them only for the
// SSIM map
template <typename T, bool VEC>
PartialKernel<T> cmp_partial_kernel(bool with_result, bool with_map, int map) {
    if (!with_map) return compare_partial_kernel<T, kCmpMapNone, true, VEC>;
    if (map == RTM_COMPARE_MAP_SSIM) return compare_partial_kernel<T, kCmpMapSsim, true, VEC>;
    return with_result ? compare_partial_kernel<T, kCmpMapAbs, true, VEC> : compare_partial_kernel<T, kCmpMapAbs, false, VEC>;
}

template <typename T>
void cmp_launch(const CmpArgs& args, unsigned tiles, const void* a, const void* b, CmpPartial* partials, bool with_map, int map,
                float* map_out, hipStream_t stream) {
    const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    const PartialKernel<T> kern = vec ? cmp_partial_kernel<T, true>(partials != nullptr, with_map, map)
                                      : cmp_partial_kernel<T, false>(partials != nullptr, with_map, map);
    kern<<<tiles, kCmpBlock, 0, stream>>>(args, (const T*)a, (const T*)b, partials, map_out);
}
}  // namespace

static_assert(sizeof(CmpPartial) == 48, "one 48-byte partial per tile");
static_assert(sizeof(rtm_compare_params) == 32 && sizeof(rtm_compare_result) == 80, "include/rtm.h states these sizes");
static_assert(sizeof(rtm_compare_result) <= kCmpAlign, "the final record fits the work buffer's last part");

// [0, round256(48 tiles)) the tile partials, then 256 bytes for the final record
size_t compare_work_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > SIZE_MAX / (3 * sizeof(double))) return SIZE_MAX;
    return cmp_partial_bytes(cmp_tiles(width, height)) + kCmpAlign;
}

int compare(const rtm_compare_params* prm, int32_t width, int32_t height, int device, const void* a, const void* b, void* work,
            rtm_compare_result* result_out, float* map_out, void* stream_v) {
    if (!prm || !a || !b || !work) return invalid("null params, a_dev, b_dev or work_dev");
    if (!result_out && !map_out) return invalid("both outputs are null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (prm->dtype != RTM_COMPARE_F32 && prm->dtype != RTM_COMPARE_F64) return invalid("dtype is not an RTM_COMPARE_F* value");
    if (prm->map != RTM_COMPARE_MAP_ABS && prm->map != RTM_COMPARE_MAP_SSIM) return invalid("map is not an RTM_COMPARE_MAP_* value");
    if (!std::isfinite(prm->tolerance) || prm->tolerance < 0.0) return invalid("tolerance is negative, NaN or infinite");
    if (!std::isfinite(prm->peak) || !(prm->peak > 0.0)) return invalid("peak is not finite and positive");
    if (!std::isfinite(prm->rel_epsilon) || !(prm->rel_epsilon > 0.0)) return invalid("rel_epsilon is not finite and positive");
    const uintptr_t elem = prm->dtype == RTM_COMPARE_F64 ? sizeof(double) : sizeof(float);
    if (((uintptr_t)a & (elem - 1)) != 0 || ((uintptr_t)b & (elem - 1)) != 0) return invalid("a frame pointer is not aligned to its element");
    if (!aligned256(work)) return invalid("work_dev is not 256-byte aligned");
    if (((uintptr_t)result_out & 7) != 0 || ((uintptr_t)map_out & 3) != 0) return invalid("an output pointer is not aligned to its element");
    if (work == a || work == b || (const void*)result_out == a || (const void*)result_out == b ||
        (map_out && ((const void*)map_out == a || (const void*)map_out == b)))
        return invalid("work_dev or an output aliases a_dev or b_dev");
    if (map_out && ((void*)map_out == work || (void*)map_out == (void*)result_out))
        return invalid("map_out_dev aliases work_dev or result_out_dev");
    if ((void*)result_out == work) return invalid("result_out_dev aliases work_dev");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > SIZE_MAX / (3 * sizeof(double)) || pix > 0x7FFFFFFFu)  // the partials index pixels in 32 bits
        return unsupported("frame too large for one launch of the comparison");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    CmpArgs args;
    for (int i = 0; i <= kCmpRadius; ++i) args.g[i] = std::exp(-(double)(i * i) / 4.5);
    args.tolerance = prm->tolerance;
    args.rel_epsilon = prm->rel_epsilon;
    args.c1 = (0.01 * prm->peak) * (0.01 * prm->peak);
    args.c2 = (0.03 * prm->peak) * (0.03 * prm->peak);
    args.peak = prm->peak;
    args.width = width;
    args.height = height;
    args.tiles_x = (int32_t)cmp_tiles_x(width);
    const size_t tiles = cmp_tiles(width, height);
    CmpPartial* partials = result_out ? (CmpPartial*)work : nullptr;  // a map-only call reduces nothing
    if (prm->dtype == RTM_COMPARE_F64)
        cmp_launch<double>(args, (unsigned)tiles, a, b, partials, map_out != nullptr, prm->map, map_out, stream);
    else
        cmp_launch<float>(args, (unsigned)tiles, a, b, partials, map_out != nullptr, prm->map, map_out, stream);
    if (result_out)
        compare_final_kernel<<<1, kCmpBlock, 0, stream>>>(args, partials, (uint32_t)tiles,
                                                          (rtm_compare_result*)((char*)work + cmp_partial_bytes(tiles)), result_out);
    return launched("compare");
}

}  // namespace rtm
