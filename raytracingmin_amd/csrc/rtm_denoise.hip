// rtm_denoise.hip — rtm_denoise / rtm_denoise_work_bytes (include/rtm.h): argument checks, the work buffer's layout and
// the launches of rtm_denoise_kernel.h.  The call keeps no state: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_denoise_kernel.h"
#include "rtm_internal.h"

namespace rtm {

namespace {
constexpr size_t kDnRecord = sizeof(float4);  // 16 B
constexpr size_t kDnPlanes = 3;               // colour records ping and pong, geometry records

int invalid(const char* what) {
    set_last_error(what);
    return RTM_ERR_INVALID_ARGUMENT;
}
}  // namespace

// Three planes of width x height 16-byte records: [0] colour ping, [1] colour pong, [2] (n, z).  SIZE_MAX when that does
// not fit a size_t (no buffer can then be given).
size_t denoise_work_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > SIZE_MAX / (kDnPlanes * kDnRecord)) return SIZE_MAX;
    return pix * kDnPlanes * kDnRecord;
}

int denoise(const rtm_denoise_params* prm, int32_t width, int32_t height, int device, const float* color,
            const rtm_aov_buffers* guide, void* work, float* out32, uint8_t* out8, void* stream_v) {
    if (!prm || !color || !work) return invalid("null params, color_dev or work_dev");
    if (!out32 && !out8) return invalid("both outputs are null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (prm->iterations < 0 || prm->iterations > 10) return invalid("iterations outside 0..10");
    for (const float v : {prm->sigma_color, prm->sigma_normal, prm->sigma_depth})
        if (!std::isfinite(v) || v < 0.0f) return invalid("a sigma is negative, NaN or infinite");
    if ((const void*)color == (const void*)out32 || (const void*)color == work)
        return invalid("color_dev aliases out_f32_dev or work_dev");
    if (((uintptr_t)work & (kDnRecord - 1)) != 0) return invalid("work_dev is not 16-byte aligned");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    const size_t tiles_x = ((size_t)width + kDnTileX - 1) / kDnTileX, tiles = tiles_x * (((size_t)height + kDnTileY - 1) / kDnTileY);
    if (tiles > 0x7FFFFFFFu / (kDnTileX * kDnTileY)) {
        set_last_error("frame too large for one launch of the denoiser");
        return RTM_ERR_UNSUPPORTED;
    }
    const hipError_t se = hipSetDevice(device);
    if (se != hipSuccess) {
        set_last_error(std::string("hipSetDevice: ") + hipGetErrorString(se));
        return RTM_ERR_HIP;
    }
    const hipStream_t stream = (hipStream_t)stream_v;
    const rtm_aov_buffers g = guide ? *guide : rtm_aov_buffers{nullptr, nullptr, nullptr, nullptr};
    if (prm->iterations == 0) {
        const size_t n = pix * 3;
        const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
        denoise_copy_kernel<<<blocks, 256, 0, stream>>>(color, n, out32, out8);
    } else {
        DenoiseFrame F;
        F.W = width;
        F.H = height;
        F.tiles_x = (int)tiles_x;
        F.has_geo = g.depth != nullptr || g.normal != nullptr;
        F.has_depth = g.depth != nullptr;
        F.depth_term = g.depth != nullptr && prm->sigma_depth > 0.0f;
        F.normal_term = g.normal != nullptr && prm->sigma_normal > 0.0f;
        F.color_term = prm->sigma_color > 0.0f;
        F.sigma_n = prm->sigma_normal;
        float4* rec[2] = {(float4*)work, (float4*)work + pix};
        float4* rec_g = (float4*)work + 2 * pix;
        const unsigned grid = (unsigned)tiles, block = kDnTileX * kDnTileY;
        denoise_prepass_kernel<<<grid, block, 0, stream>>>(F, color, g.depth, g.normal, g.albedo, g.object, rec[0], rec_g);
        const double sc = (double)prm->sigma_color;
        for (int i = 0; i < prm->iterations; ++i) {
            const int s = 1 << i;
            // 4^i / sigma_c^2 * log2(e), capped at FLT_MAX: a tiny sigma then still gives w_c = 1 for equal colours
            const float color_scale =
                F.color_term ? (float)std::fmin(std::ldexp(1.0, 2 * i) / (sc * sc) * 1.4426950408889634, (double)FLT_MAX) : 0.0f;
            const float depth_scale = prm->sigma_depth * (float)s;
            if (i + 1 < prm->iterations)
                denoise_level_kernel<false><<<grid, block, 0, stream>>>(F, s, color_scale, depth_scale, rec[i & 1], rec_g,
                                                                        rec[(i + 1) & 1], g.albedo, nullptr, nullptr);
            else
                denoise_level_kernel<true><<<grid, block, 0, stream>>>(F, s, color_scale, depth_scale, rec[i & 1], rec_g,
                                                                       nullptr, g.albedo, out32, out8);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(std::string("denoise kernel launch: ") + hipGetErrorString(e));
        return RTM_ERR_HIP;
    }
    return RTM_OK;
}

}  // namespace rtm
