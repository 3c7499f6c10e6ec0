// rtm_tonemap_local.hip — rtm_tonemap_local / rtm_tonemap_local_work_bytes (include/rtm.h): argument checks, the work
// buffer's layout and the launches of rtm_tonemap_local_kernel.h.  The call keeps no state: it only enqueues on the caller's
// stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_host.h"
#include "rtm_tonemap_local_kernel.h"

namespace rtm {

namespace {
constexpr size_t kLtAlign = 256;      // work_dev's alignment and that of every plane
constexpr size_t kLtPixelBytes = 12;  // the frame: three floats a pixel
constexpr size_t kLtRecord = 16;      // a level's record
constexpr int kLtMaxLevels = 8;

int half_up(int n) { return (n + 1) / 2; }  // a side that has reached 1 stays 1
unsigned tiles_of(int n, int tile) { return (unsigned)((n + tile - 1) / tile); }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
size_t plane_bytes(int w, int h) { return ((size_t)w * (size_t)h * kLtRecord + kLtAlign - 1) / kLtAlign * kLtAlign; }
}  // namespace

// the I plane and the W plane of levels 1..L, each rounded up to 256 bytes, in that order
size_t tonemap_local_work_bytes(int32_t width, int32_t height, int32_t levels) {
    if (width <= 0 || height <= 0 || levels < 1 || levels > kLtMaxLevels) return 0;
    if ((size_t)width * (size_t)height > SIZE_MAX / kLtPixelBytes) return SIZE_MAX;
    size_t sum = 0;
    int w = width, h = height;
    for (int l = 1; l <= levels; ++l) {
        w = half_up(w);
        h = half_up(h);
        const size_t records = (size_t)w * (size_t)h;
        if (records > (SIZE_MAX - kLtAlign) / kLtRecord) return SIZE_MAX;
        const size_t plane = plane_bytes(w, h);
        if (plane > (SIZE_MAX - sum) / 2) return SIZE_MAX;
        sum += 2 * plane;
    }
    return sum;
}

int tonemap_local(const rtm_tonemap_local_params* prm, int32_t width, int32_t height, int device, const float* color,
                  const rtm_tonemap_stats* stats, void* work, float* out32, uint8_t* out8, float* fused_out, void* stream_v) {
    if (!prm || !color) return invalid("null params or color_dev");
    if (!out32 && !out8 && !fused_out) return invalid("every output is null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (!std::isfinite(prm->anchor) || !std::isfinite(prm->shadows) || !std::isfinite(prm->highlights) || !std::isfinite(prm->sigma))
        return invalid("anchor, shadows, highlights or sigma is NaN or infinite");
    if (!(prm->anchor > 0.0f)) return invalid("anchor <= 0");
    if (prm->shadows < 0.0f || prm->shadows > 8.0f) return invalid("shadows outside [0, 8]");
    if (prm->highlights < 0.0f || prm->highlights > 8.0f) return invalid("highlights outside [0, 8]");
    if (prm->sigma < 0.1f || prm->sigma > 1.0f) return invalid("sigma outside [0.1, 1]");
    if (prm->levels < 0 || prm->levels > kLtMaxLevels) return invalid("levels outside 0..8");
    if (prm->levels > 0 && !work) return invalid("null work_dev with levels > 0");
    if (!aligned4(color) || !aligned4(out32) || !aligned4(fused_out) || !aligned4(stats))
        return invalid("a float buffer is not 4-byte aligned");
    if (!aligned256(work)) return invalid("work_dev is not 256-byte aligned");
    if (work && (work == (const void*)color || work == (void*)out32 || work == (void*)out8 || work == (void*)fused_out ||
                 work == (const void*)stats))
        return invalid("work_dev aliases another buffer");
    if (fused_out && ((const void*)fused_out == (const void*)color || fused_out == out32))
        return invalid("fused_out_dev aliases color_dev or out_f32_dev");
    if (stats && ((const void*)stats == (const void*)color || (const void*)stats == (const void*)out32))
        return invalid("stats_dev aliases color_dev or out_f32_dev");
    if (out8 && (const void*)out8 == (const void*)color) return invalid("out_u8_dev aliases color_dev");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFu) return unsupported("frame too large for one launch of the local tone operator");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    const int L = prm->levels;
    const LocalToneArgs args = {prm->anchor, exp2f(prm->shadows), exp2f(-prm->highlights),
                                -1.0f / (2.0f * prm->sigma * prm->sigma)};
    int w[kLtMaxLevels + 1], h[kLtMaxLevels + 1];
    float4 *plane_i[kLtMaxLevels + 1], *plane_w[kLtMaxLevels + 1];
    w[0] = width;
    h[0] = height;
    plane_i[0] = plane_w[0] = nullptr;
    size_t at = 0;
    for (int l = 1; l <= L; ++l) {
        w[l] = half_up(w[l - 1]);
        h[l] = half_up(h[l - 1]);
        plane_i[l] = (float4*)((char*)work + at);
        at += plane_bytes(w[l], h[l]);
        plane_w[l] = (float4*)((char*)work + at);
        at += plane_bytes(w[l], h[l]);
    }
    const auto down_grid = [&](int l, unsigned& tiles_x) {
        tiles_x = tiles_of(w[l], kBlTileX);
        return tiles_x * tiles_of(h[l], kBlTileY);
    };
    const auto pixel_grid = [&](int l, unsigned& tiles_x) {
        tiles_x = tiles_of(w[l], kBlPixTileX);
        return tiles_x * tiles_of(h[l], kBlPixTileY);
    };
    unsigned tx = 0, grid = 0;
    if (L >= 1) {
        grid = down_grid(1, tx);
        if (((uintptr_t)color & 15) == 0)
            local_base_down_kernel<true><<<grid, kBlBlock, 0, stream>>>(width, height, w[1], h[1], (int)tx, color, stats, args, L == 1, plane_i[1], plane_w[1]);
        else
            local_base_down_kernel<false><<<grid, kBlBlock, 0, stream>>>(width, height, w[1], h[1], (int)tx, color, stats, args, L == 1, plane_i[1], plane_w[1]);
    }
    for (int l = 2; l <= L; ++l) {
        grid = down_grid(l, tx);
        local_down_kernel<<<grid, kBlBlock, 0, stream>>>(w[l - 1], h[l - 1], w[l], h[l], (int)tx, plane_i[l - 1], plane_w[l - 1], l == L, plane_i[l], plane_w[l]);
    }
    for (int l = L - 1; l >= 1; --l) {
        grid = pixel_grid(l, tx);
        local_collapse_kernel<<<grid, kBlPixTileX * kBlPixTileY, 0, stream>>>(w[l], h[l], w[l + 1], h[l + 1], (int)tx, plane_i[l + 1], plane_w[l], plane_i[l]);
    }
    grid = pixel_grid(0, tx);
    local_apply_kernel<<<grid, kBlPixTileX * kBlPixTileY, 0, stream>>>(width, height, L ? w[1] : 1, L ? h[1] : 1, (int)tx, color, stats, args, L ? plane_i[1] : nullptr, out32, out8, fused_out);
    return launched("tonemap_local");
}

}  // namespace rtm
