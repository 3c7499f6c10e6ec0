// rtm_denoise.hip — rtm_denoise / rtm_denoise_work_bytes and rtm_denoise_variance / rtm_denoise_variance_work_bytes
// (include/rtm.h): argument checks, the work buffers' layouts and the launches of rtm_denoise_kernel.h and
// rtm_denoise_var_kernel.h.  The calls keep no state: they only enqueue on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_denoise_kernel.h"
#include "rtm_denoise_var_kernel.h"
#include "rtm_host.h"

namespace rtm {

namespace {
constexpr size_t kDnRecord = sizeof(float4);  // 16 B
constexpr size_t kDnPlanes = 3;               // colour records ping and pong, geometry records

}  // namespace

// Three planes of width x height 16-byte records: [0] colour ping, [1] colour pong, [2] (n, z).  SIZE_MAX when that does
// not fit a size_t (no buffer can then be given).
size_t denoise_work_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > SIZE_MAX / (kDnPlanes * kDnRecord)) return SIZE_MAX;
    return pix * kDnPlanes * kDnRecord;
}

// (rtm_denoise_variance below makes the same checks and fills the same DenoiseFrame in dv_plan: keep the two in step.)
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
    if (tiles > 0x7FFFFFFFu / (kDnTileX * kDnTileY))
        return unsupported("frame too large for one launch of the denoiser");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
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
    return launched("denoise");
}

// ---- the variance-guided filter --------------------------------------------------------------------------------------
namespace {
constexpr size_t kDvPixelBytes = kDnPlanes * kDnRecord + 2 * sizeof(float);  // rtm_denoise's planes + variance ping and pong
constexpr int kDvShippedForm = 2;  // denoise_variance_kernel<2>: the form with the fewest loads per pixel

struct DvPlan {
    DenoiseFrame F;
    size_t pix;
    unsigned grid;  // blocks of 64 x 4 pixels
    float4 *rec[2], *rec_g;
    float* v[2];
};

// what rtm_denoise and rtm_denoise_variance check alike, then the frame's flags and the work buffer's planes:
// [0] colour ping, [1] colour pong, [2] (n, z) as rtm_denoise lays them out, then two planes of one float per pixel
int dv_plan(int32_t iterations, const float (&sigmas)[3], int32_t width, int32_t height, int device, const rtm_aov_buffers& g,
            void* work, DvPlan& P) {
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (iterations < 0 || iterations > 10) return invalid("iterations outside 0..10");
    for (const float v : sigmas)
        if (!std::isfinite(v) || v < 0.0f) return invalid("a sigma is negative, NaN or infinite");
    if (((uintptr_t)work & (kDnRecord - 1)) != 0) return invalid("work_dev is not 16-byte aligned");
    if (device < 0) return invalid("negative device");
    P.pix = (size_t)width * (size_t)height;
    const size_t tiles_x = ((size_t)width + kDnTileX - 1) / kDnTileX, tiles = tiles_x * (((size_t)height + kDnTileY - 1) / kDnTileY);
    if (tiles > 0x7FFFFFFFu / (kDnTileX * kDnTileY))
        return unsupported("frame too large for one launch of the denoiser");
    P.grid = (unsigned)tiles;
    P.F.W = width;
    P.F.H = height;
    P.F.tiles_x = (int)tiles_x;
    P.F.has_geo = g.depth != nullptr || g.normal != nullptr;
    P.F.has_depth = g.depth != nullptr;
    P.F.depth_term = g.depth != nullptr && sigmas[2] > 0.0f;
    P.F.normal_term = g.normal != nullptr && sigmas[1] > 0.0f;
    P.F.color_term = sigmas[0] > 0.0f;
    P.F.sigma_n = sigmas[1];
    P.rec[0] = (float4*)work;
    P.rec[1] = (float4*)work + P.pix;
    P.rec_g = (float4*)work + 2 * P.pix;
    P.v[0] = (float*)((float4*)work + kDnPlanes * P.pix);
    P.v[1] = P.v[0] + P.pix;
    return RTM_OK;
}

// v0 from the records of the prepass; form 0: every tap from L2, 1 / 2: the LDS form with tiles of 64 x 4 / 64 x 8
void dv_launch_variance(int form, const DvPlan& P, float sigma_depth, float* v_out, float* var_out, hipStream_t stream) {
    const unsigned block = kDnTileX * kDnTileY;
    const unsigned tall = (unsigned)P.F.tiles_x * (unsigned)((P.F.H + 2 * kDnTileY - 1) / (2 * kDnTileY));
    if (form == 0)
        denoise_variance_direct_kernel<<<P.grid, block, 0, stream>>>(P.F, sigma_depth, P.rec[0], P.rec_g, v_out, var_out);
    else if (form == 1)
        denoise_variance_kernel<1><<<P.grid, block, 0, stream>>>(P.F, P.F.tiles_x, sigma_depth, P.rec[0], P.rec_g, v_out, var_out);
    else
        denoise_variance_kernel<2><<<tall, block, 0, stream>>>(P.F, P.F.tiles_x, sigma_depth, P.rec[0], P.rec_g, v_out, var_out);
}
}  // namespace

// rtm_denoise's 48 bytes per pixel and two variance planes of one float each.  SIZE_MAX when that does not fit a size_t.
size_t denoise_variance_work_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > SIZE_MAX / kDvPixelBytes) return SIZE_MAX;
    return pix * kDvPixelBytes;
}

int denoise_variance(const rtm_denoise_var_params* prm, int32_t width, int32_t height, int device, const float* color,
                     const rtm_aov_buffers* guide, void* work, float* out32, uint8_t* out8, float* var_out, void* stream_v) {
    if (!prm || !color || !work) return invalid("null params, color_dev or work_dev");
    if (!out32 && !out8 && !var_out) return invalid("every output is null");
    if ((const void*)color == (const void*)out32 || (const void*)color == work)
        return invalid("color_dev aliases out_f32_dev or work_dev");
    if (var_out && ((const void*)var_out == (const void*)color || (const void*)var_out == work || var_out == out32))
        return invalid("variance_out_dev aliases color_dev, work_dev or out_f32_dev");
    const rtm_aov_buffers g = guide ? *guide : rtm_aov_buffers{nullptr, nullptr, nullptr, nullptr};
    DvPlan P;
    const float sigmas[3] = {prm->sigma_lum, prm->sigma_normal, prm->sigma_depth};
    const int rc = dv_plan(prm->iterations, sigmas, width, height, device, g, work, P);
    if (rc != RTM_OK) return rc;
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    const unsigned block = kDnTileX * kDnTileY;
    const int K = (out32 || out8) ? prm->iterations : 0;  // a variance-only call filters nothing
    if (K > 0 || var_out) {
        denoise_prepass_kernel<<<P.grid, block, 0, stream>>>(P.F, color, g.depth, g.normal, g.albedo, g.object, P.rec[0], P.rec_g);
        dv_launch_variance(kDvShippedForm, P, prm->sigma_depth, K > 0 ? P.v[0] : nullptr, var_out, stream);
    }
    if (K == 0 && (out32 || out8)) {
        const size_t n = P.pix * 3;
        const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
        denoise_copy_kernel<<<blocks, 256, 0, stream>>>(color, n, out32, out8);
    }
    for (int i = 0; i < K; ++i) {
        const int s = 1 << i;
        const float depth_scale = prm->sigma_depth * (float)s;
        if (i + 1 < K)
            denoise_level_var_kernel<false><<<P.grid, block, 0, stream>>>(P.F, s, prm->sigma_lum, depth_scale, P.rec[i & 1], P.rec_g,
                                                                          P.v[i & 1], P.rec[(i + 1) & 1], P.v[(i + 1) & 1],
                                                                          g.albedo, nullptr, nullptr);
        else
            denoise_level_var_kernel<true><<<P.grid, block, 0, stream>>>(P.F, s, prm->sigma_lum, depth_scale, P.rec[i & 1], P.rec_g,
                                                                         P.v[i & 1], nullptr, nullptr, g.albedo, out32, out8);
    }
    return launched("denoise_variance");
}

// rtm_debug_denoise_variance_kernel (include/rtm_debug.h): one form of the variance kernel alone, on the records a
// rtm_denoise_variance call of the same frame left in `work`
int denoise_variance_kernel_probe(int form, const rtm_denoise_var_params* prm, int32_t width, int32_t height, int device,
                                  const rtm_aov_buffers* guide, void* work, float* var_out, void* stream_v) {
    if (!prm || !work || !var_out) return invalid("null params, work_dev or variance_out_dev");
    if (form < 0 || form > 2) return invalid("form outside 0..2");
    if ((const void*)var_out == work) return invalid("variance_out_dev aliases work_dev");
    const rtm_aov_buffers g = guide ? *guide : rtm_aov_buffers{nullptr, nullptr, nullptr, nullptr};
    DvPlan P;
    const float sigmas[3] = {prm->sigma_lum, prm->sigma_normal, prm->sigma_depth};
    const int rc = dv_plan(prm->iterations, sigmas, width, height, device, g, work, P);
    if (rc != RTM_OK) return rc;
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    dv_launch_variance(form, P, prm->sigma_depth, nullptr, var_out, (hipStream_t)stream_v);
    return launched("denoise_variance");
}

}  // namespace rtm
