// rtm_tonemap.hip — rtm_tonemap / rtm_tonemap_work_bytes (include/rtm.h): argument checks, the work buffer's layout and the
// launches of rtm_tonemap_kernel.h.  The call keeps no state: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_host.h"
#include "rtm_tonemap_kernel.h"

namespace rtm {

namespace {
constexpr size_t kTmAlign = 256;      // work_dev's alignment and the size of its last part
constexpr size_t kTmPixelBytes = 12;  // the frame: three floats a pixel

size_t tm_blocks(size_t pix) { return (pix + kTmBlockPixels - 1) / kTmBlockPixels; }
size_t tm_partial_bytes(size_t pix) { return (tm_blocks(pix) * sizeof(TmPartial) + kTmAlign - 1) / kTmAlign * kTmAlign; }

using MapKernel = void (*)(int, int, int, const float*, const float*, float, float, float*, uint8_t*);

template <int OP, int TRANSFER>
MapKernel tm_map_kernel(int dither) {
    return dither ? tonemap_map_kernel<OP, TRANSFER, 1> : tonemap_map_kernel<OP, TRANSFER, 0>;
}
template <int OP>
MapKernel tm_map_kernel(int transfer, int dither) {
    return transfer == RTM_TRANSFER_SRGB ? tm_map_kernel<OP, RTM_TRANSFER_SRGB>(dither) : tm_map_kernel<OP, RTM_TRANSFER_LINEAR>(dither);
}
MapKernel tm_map_kernel(int op, int transfer, int dither) {
    switch (op) {
        case RTM_TONEMAP_REINHARD: return tm_map_kernel<RTM_TONEMAP_REINHARD>(transfer, dither);
        case RTM_TONEMAP_ACES: return tm_map_kernel<RTM_TONEMAP_ACES>(transfer, dither);
        default: return tm_map_kernel<RTM_TONEMAP_CLAMP>(transfer, dither);
    }
}
}  // namespace

static_assert(sizeof(TmPartial) == 16, "one 16-byte partial per block");

// [0, round256(16 blocks)) the block partials, then 256 bytes for what tonemap_final_kernel derives from them
size_t tonemap_work_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > SIZE_MAX / kTmPixelBytes) return SIZE_MAX;
    return tm_partial_bytes(pix) + kTmAlign;
}

int tonemap(const rtm_tonemap_params* prm, int32_t width, int32_t height, int device, const float* color, void* work,
            float* out32, uint8_t* out8, rtm_tonemap_stats* stats_out, void* stream_v) {
    if (!prm || !color || !work) return invalid("null params, color_dev or work_dev");
    if (!out32 && !out8 && !stats_out) return invalid("every output is null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (prm->op < RTM_TONEMAP_CLAMP || prm->op > RTM_TONEMAP_ACES) return invalid("op is not an RTM_TONEMAP_* value");
    if (prm->transfer < RTM_TRANSFER_LINEAR || prm->transfer > RTM_TRANSFER_SRGB) return invalid("transfer is not an RTM_TRANSFER_* value");
    if ((prm->auto_exposure != 0 && prm->auto_exposure != 1) || (prm->dither != 0 && prm->dither != 1))
        return invalid("auto_exposure and dither are 0 or 1");
    if (!std::isfinite(prm->ev) || !std::isfinite(prm->key) || !std::isfinite(prm->white)) return invalid("ev, key or white is NaN or infinite");
    if (std::fabs(prm->ev) > 32.0f) return invalid("|ev| > 32");
    if (!(prm->key > 0.0f)) return invalid("key <= 0");
    if (prm->white < 0.0f) return invalid("white < 0");
    if (!aligned256(work)) return invalid("work_dev is not 256-byte aligned");
    if (work == (const void*)color || work == (void*)out32 || work == (void*)out8 || work == (void*)stats_out)
        return invalid("work_dev aliases another buffer");
    if (stats_out && ((const void*)stats_out == (const void*)color || (void*)stats_out == (void*)out32))
        return invalid("stats_out_dev aliases color_dev or out_f32_dev");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    const size_t tiles_x = ((size_t)width + kTmTileX - 1) / kTmTileX, tiles = tiles_x * (((size_t)height + kTmTileY - 1) / kTmTileY);
    if (pix > SIZE_MAX / kTmPixelBytes || tiles > 0x7FFFFFFFu / (kTmTileX * kTmTileY))
        return unsupported("frame too large for one launch of the display transform");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    const float e_scale = std::exp2(prm->ev);
    const bool reinhard_auto_white = prm->op == RTM_TONEMAP_REINHARD && prm->white == 0.0f;
    const bool need_stats = prm->auto_exposure != 0 || reinhard_auto_white || stats_out != nullptr;
    float* fin = nullptr;
    if (need_stats) {
        TmPartial* partials = (TmPartial*)work;
        fin = (float*)((char*)work + tm_partial_bytes(pix));
        const unsigned blocks = (unsigned)tm_blocks(pix);
        if (((uintptr_t)color & 15) == 0)
            tonemap_partial_kernel<true><<<blocks, kTmBlock, 0, stream>>>(color, pix, partials);
        else
            tonemap_partial_kernel<false><<<blocks, kTmBlock, 0, stream>>>(color, pix, partials);
        tonemap_final_kernel<<<1, kTmBlock, 0, stream>>>(partials, blocks, e_scale, prm->auto_exposure, prm->key, prm->white, fin,
                                                        stats_out);
    }
    if (out32 || out8)
        tm_map_kernel(prm->op, prm->transfer, prm->dither)<<<(unsigned)tiles, kTmTileX * kTmTileY, 0, stream>>>(
            width, height, (int)tiles_x, color, fin, e_scale, prm->white, out32, out8);
    return launched("tonemap");
}

}  // namespace rtm
