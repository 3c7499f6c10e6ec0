// rtm_upsample.hip — rtm_upsample / rtm_upsample_work_bytes (include/rtm.h): argument checks, the spatial weight table, the
// work buffer's layout and the two launches of rtm_upsample_kernel.h.  The call keeps no state: it only enqueues on the
// caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_host.h"
#include "rtm_upsample_kernel.h"

namespace rtm {

namespace {
constexpr size_t kUpRecord = sizeof(float4);  // 16 B
constexpr size_t kUpPlanes = 2;               // (e, object bits) and (n, z) per low pixel
constexpr size_t kUpFullPixelBytes = 12 * (size_t)kUpMaxFactor * kUpMaxFactor;  // the full frame at f = 8, per low pixel

using UpKernel = void (*)(UpsampleFrame, const float4*, const float4*, const float*, const float*, const float*, const int32_t*,
                          float*, uint8_t*);

UpKernel up_kernel(int factor) {
    switch (factor) {
        case 2: return upsample_kernel<2>;
        case 3: return upsample_kernel<3>;
        case 4: return upsample_kernel<4>;
        case 5: return upsample_kernel<5>;
        case 6: return upsample_kernel<6>;
        case 7: return upsample_kernel<7>;
        default: return upsample_kernel<8>;
    }
}
}  // namespace

// Two planes of w x h 16-byte records: [0] (e, object bits), [1] (n, z).  SIZE_MAX when the full frame at f = 8 does not
// fit a size_t (no output can then be given).
size_t upsample_work_bytes(int32_t low_width, int32_t low_height) {
    if (low_width <= 0 || low_height <= 0) return 0;
    const size_t pix = (size_t)low_width * (size_t)low_height;
    if (pix > SIZE_MAX / kUpFullPixelBytes) return SIZE_MAX;
    return pix * kUpPlanes * kUpRecord;
}

int upsample(const rtm_upsample_params* prm, int32_t low_width, int32_t low_height, int device, const float* color_low,
             const rtm_aov_buffers* guide_low, const rtm_aov_buffers* guide_high, void* work, float* out32, uint8_t* out8,
             void* stream_v) {
    if (!prm || !color_low || !work) return invalid("null params, color_low_dev or work_dev");
    if (!out32 && !out8) return invalid("both outputs are null");
    if (low_width <= 0 || low_height <= 0) return invalid("non-positive frame size");
    if (prm->factor < 2 || prm->factor > kUpMaxFactor) return invalid("factor outside 2..8");
    if (!std::isfinite(prm->sigma_spatial) || prm->sigma_spatial < 0.25f || prm->sigma_spatial > 4.0f)
        return invalid("sigma_spatial outside [0.25, 4], NaN or infinite");
    for (const float v : {prm->sigma_normal, prm->sigma_depth})
        if (!std::isfinite(v) || v < 0.0f) return invalid("a sigma is negative, NaN or infinite");
    if ((guide_low == nullptr) != (guide_high == nullptr)) return invalid("one guide struct is null and the other is not");
    const rtm_aov_buffers none{nullptr, nullptr, nullptr, nullptr};
    const rtm_aov_buffers lo = guide_low ? *guide_low : none, hi = guide_high ? *guide_high : none;
    if ((lo.depth == nullptr) != (hi.depth == nullptr) || (lo.normal == nullptr) != (hi.normal == nullptr) ||
        (lo.albedo == nullptr) != (hi.albedo == nullptr) || (lo.object == nullptr) != (hi.object == nullptr))
        return invalid("a guide plane is given at one resolution only");
    if (((uintptr_t)work & (kUpRecord - 1)) != 0) return invalid("work_dev is not 16-byte aligned");
    if (work == (void*)out32 || work == (void*)out8 || (const void*)color_low == (const void*)out32 ||
        (const void*)color_low == (const void*)out8)
        return invalid("work_dev or color_low_dev aliases an output");
    if (device < 0) return invalid("negative device");
    const int f = prm->factor;
    const int64_t W = (int64_t)f * low_width, H = (int64_t)f * low_height;
    const size_t pix = (size_t)low_width * (size_t)low_height;
    const size_t tiles_x = ((size_t)W + kUpTileX - 1) / kUpTileX, tiles = tiles_x * (((size_t)H + kUpTileY - 1) / kUpTileY);
    if (W > INT32_MAX || H > INT32_MAX || pix > SIZE_MAX / kUpFullPixelBytes || tiles > 0x7FFFFFFFu / (kUpTileX * kUpTileY))
        return unsupported("frame too large for one launch of the upsampler");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    UpsampleFrame U;
    U.w = low_width;
    U.h = low_height;
    U.W = (int)W;
    U.H = (int)H;
    U.has_geo = lo.depth != nullptr || lo.normal != nullptr;
    U.has_depth = lo.depth != nullptr;
    U.depth_term = lo.depth != nullptr && prm->sigma_depth > 0.0f;
    U.normal_term = lo.normal != nullptr && prm->sigma_normal > 0.0f;
    U.sigma_n = prm->sigma_normal;
    U.depth_scale = prm->sigma_depth * (float)f;
    const double two_sigma2 = 2.0 * (double)prm->sigma_spatial * (double)prm->sigma_spatial;
    for (int j = 0; j < kUpMaxFactor; ++j)
        for (int k = 0; k < 4; ++k) {
            const double t = (double)(2 * j + (f % 2 == 0 ? 1 : 0)) / (double)(2 * f), d = (double)(k - 1) - t;
            U.tab[4 * j + k] = j < f ? (float)std::exp(-d * d / two_sigma2) : 0.0f;
        }
    float4* rec_e = (float4*)work;
    float4* rec_g = (float4*)work + pix;
    const unsigned block = kUpTileX * kUpTileY;
    U.tiles_x = (low_width + kUpTileX - 1) / kUpTileX;
    const unsigned low_tiles = (unsigned)U.tiles_x * (unsigned)((low_height + kUpTileY - 1) / kUpTileY);
    upsample_pack_kernel<<<low_tiles, block, 0, stream>>>(U, color_low, lo.depth, lo.normal, lo.albedo, lo.object, rec_e, rec_g);
    U.tiles_x = (int)tiles_x;
    up_kernel(f)<<<(unsigned)tiles, block, 0, stream>>>(U, rec_e, rec_g, hi.depth, hi.normal, hi.albedo, hi.object, out32, out8);
    return launched("upsample");
}

}  // namespace rtm
