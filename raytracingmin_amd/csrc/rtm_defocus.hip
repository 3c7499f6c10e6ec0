// rtm_defocus.hip — rtm_defocus (include/rtm.h): argument checks and the one launch of rtm_defocus_kernel.h.  The call keeps
// no state and needs no work buffer: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rtm_defocus_kernel.h"
#include "rtm_host.h"

namespace rtm {

namespace {
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// the instantiation of the smallest R class that holds max_radius
template <bool BOUND>
void df_launch(unsigned grid, hipStream_t stream, int W, int H, int tiles_x, const rtm_defocus_params* prm, const float* color,
               const float* depth, float* out32, uint8_t* out8, float* coc_out) {
    const int R = prm->max_radius;
    const float zf = prm->focus_distance, A = prm->aperture;
    if (R <= 4)
        defocus_kernel<4, BOUND><<<grid, kDfBlock, 0, stream>>>(W, H, tiles_x, R, zf, A, color, depth, out32, out8, coc_out);
    else if (R <= 8)
        defocus_kernel<8, BOUND><<<grid, kDfBlock, 0, stream>>>(W, H, tiles_x, R, zf, A, color, depth, out32, out8, coc_out);
    else
        defocus_kernel<16, BOUND><<<grid, kDfBlock, 0, stream>>>(W, H, tiles_x, R, zf, A, color, depth, out32, out8, coc_out);
}

// form 0: the shipped kernel; form 1: without the window bound and the pass-through (rtm_debug_defocus_form)
int defocus_form(int form, const rtm_defocus_params* prm, int32_t width, int32_t height, int device, const float* color,
                 const float* depth, float* out32, uint8_t* out8, float* coc_out, void* stream_v) {
    if (!prm || !color || !depth) return invalid("null params, color_dev or depth_dev");
    if (!out32 && !out8 && !coc_out) return invalid("every output is null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (!std::isfinite(prm->focus_distance) || !(prm->focus_distance > 0.0f))
        return invalid("focus_distance is NaN, infinite or not positive");
    if (!std::isfinite(prm->aperture) || prm->aperture < 0.0f) return invalid("aperture is NaN, infinite or negative");
    if (prm->max_radius < 1 || prm->max_radius > kDfMaxRadius) return invalid("max_radius outside 1..16");
    if (!aligned4(color) || !aligned4(depth) || !aligned4(out32) || !aligned4(coc_out))
        return invalid("a float buffer is not 4-byte aligned");
    const void* const in[2] = {color, depth};
    for (const void* src : in)
        if ((out32 && (const void*)out32 == src) || (out8 && (const void*)out8 == src) || (coc_out && (const void*)coc_out == src))
            return invalid("an output aliases color_dev or depth_dev: the gather cannot run in place");
    if (coc_out && coc_out == out32) return invalid("coc_out_dev aliases out_f32_dev");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFu) return unsupported("frame too large for one launch of defocus");
    // one 512-lane block a tile: a frame thinner than a tile has far more lanes than pixels, and a launch holds fewer than 2^32
    const size_t tiles = (size_t)((width + kDfTileX - 1) / kDfTileX) * (size_t)((height + kDfTileY - 1) / kDfTileY);
    if (tiles >= ((size_t)1 << 32) / kDfBlock) return unsupported("frame too large for one launch of defocus: 2^23 tiles or more");
    if (device < 0) return invalid("negative device");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    const unsigned tiles_x = (unsigned)((width + kDfTileX - 1) / kDfTileX);
    const unsigned grid = tiles_x * (unsigned)((height + kDfTileY - 1) / kDfTileY);
    if (form == 0)
        df_launch<true>(grid, stream, width, height, (int)tiles_x, prm, color, depth, out32, out8, coc_out);
    else
        df_launch<false>(grid, stream, width, height, (int)tiles_x, prm, color, depth, out32, out8, coc_out);
    return launched("defocus");
}
}  // namespace

int defocus(const rtm_defocus_params* prm, int32_t width, int32_t height, int device, const float* color, const float* depth,
            float* out32, uint8_t* out8, float* coc_out, void* stream) {
    return defocus_form(0, prm, width, height, device, color, depth, out32, out8, coc_out, stream);
}

int defocus_form_probe(int form, const rtm_defocus_params* prm, int32_t width, int32_t height, int device, const float* color,
                       const float* depth, float* out32, uint8_t* out8, float* coc_out, void* stream) {
    if (form < 0 || form > 1) return invalid("form outside 0..1");
    return defocus_form(form, prm, width, height, device, color, depth, out32, out8, coc_out, stream);
}

}  // namespace rtm
