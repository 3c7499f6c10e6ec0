// rtm_matte.hip — the coverage AOVs (include/rtm.h: rtm_render_mattes, rtm_matte, rtm_composite; include/rtm_debug.h:
// rtm_debug_matte_rank): the launches of rtm_matte_kernel.h and the argument checks of the three calls that keep no state.
// rtm_render_mattes' own checks, its serialisation and the scene's lifetime are with the other renders (rtm_kernels.hip:
// render_mattes).  NOT a translation unit of its own: rtm_kernels.hip includes this file at its end, so that the kernels
// here live in the code object of the render and AOV kernels ("Coverage AOVs", says what a separate one did).
#include "rtm_matte_kernel.h"

namespace rtm {

namespace {
bool misaligned4(const void* p) { return ((uintptr_t)p & 3) != 0; }
}  // namespace

// rtm_render_mattes' launch for the planned P; search = kAov*, lds = aov_lds_bytes(search, P.SS).  The caller (render_mattes)
// has set the device, checked every argument and holds the stream's lock.
static int launch_matte(const RenderParams& P, int search, bool planes, unsigned tiles, size_t lds, int32_t layers, size_t plane,
                        const rtm_matte_buffers& out, hipStream_t stream) {
    if (search == kAovGrid)
        matte_kernel<kAovGrid, SceneGlobal><<<tiles, 64, lds, stream>>>(P, out, layers, plane);
    else if (search == kAovGeneral)
        matte_kernel<kAovGeneral, SceneGlobal><<<tiles, 64, lds, stream>>>(P, out, layers, plane);
    else if (planes)
        matte_kernel<kAovChunked, SceneGlobalObjects><<<tiles, 64, lds, stream>>>(P, out, layers, plane);
    else
        matte_kernel<kAovChunked, SceneGlobal><<<tiles, 64, lds, stream>>>(P, out, layers, plane);
    return launched("matte");
}

int matte_rank_probe(int32_t super_samples, int32_t layers, int device, const int32_t* ids, size_t n_pixels, int32_t* id_out,
                     float* coverage_out, float* alpha_out, void* stream_v) {
    if (layers < 1 || layers > kMatteMaxLayers) return invalid("layers outside 1..8");
    if (super_samples < 1) return invalid("super_samples is not positive");
    if (!ids) return invalid("null ids_dev");
    if (!id_out && !coverage_out && !alpha_out) return invalid("every output is null");
    if (misaligned4(ids) || misaligned4(id_out) || misaligned4(coverage_out) || misaligned4(alpha_out))
        return invalid("a buffer is not 4-byte aligned");
    if (device < 0) return invalid("negative device");
    if (super_samples > kMatteMaxSS)
        return unsupported("the ranking serves superSamples up to 8 (the id lists of a block: 16 KiB of LDS)");
    if (n_pixels > 0x7FFFFFFFull) return unsupported("2^31 pixels or more");
    if (n_pixels == 0) return RTM_OK;
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const rtm_matte_buffers out{id_out, coverage_out, alpha_out};
    matte_rank_kernel<<<(unsigned)((n_pixels + 63) / 64), 64, aov_lds_bytes(kAovChunked, super_samples), (hipStream_t)stream_v>>>(
        super_samples * super_samples, layers, ids, n_pixels, out);
    return launched("matte rank");
}

int matte(int32_t width, int32_t height, int32_t layers, int device, const int32_t* layer_id, const float* layer_coverage,
          const int32_t* ids, int32_t n_ids, float* matte_out, void* stream_v) {
    if (layers < 1 || layers > kMatteMaxLayers) return invalid("layers outside 1..8");
    if (n_ids < 1 || n_ids > kMatteMaxIds) return invalid("n_ids outside 1..64");
    if (!layer_id || !layer_coverage || !ids || !matte_out) return invalid("null layer_id_dev, layer_coverage_dev, ids_dev or matte_out_dev");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (misaligned4(layer_id) || misaligned4(layer_coverage) || misaligned4(ids) || misaligned4(matte_out))
        return invalid("a buffer is not 4-byte aligned");
    if ((const void*)matte_out == (const void*)layer_id || (const void*)matte_out == (const void*)layer_coverage ||
        (const void*)matte_out == (const void*)ids)
        return invalid("matte_out_dev is one of the inputs");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFull) return unsupported("a frame of 2^31 pixels or more");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    matte_extract_kernel<<<(unsigned)((pix + 255) / 256), 256, 0, (hipStream_t)stream_v>>>(pix, layers, layer_id, layer_coverage, ids,
                                                                                         n_ids, matte_out);
    return launched("matte extract");
}

int composite(const rtm_composite_params* prm, int32_t width, int32_t height, int device, const float* color, const float* alpha,
              const float* background, float* out32, uint8_t* out8, void* stream_v) {
    if (!prm || !color || !alpha) return invalid("null params, color_dev or alpha_dev");
    if (!out32 && !out8) return invalid("both outputs are null");
    if (!std::isfinite(prm->background[0]) || !std::isfinite(prm->background[1]) || !std::isfinite(prm->background[2]))
        return invalid("the constant background is NaN or infinite");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (misaligned4(color) || misaligned4(alpha) || misaligned4(background) || misaligned4(out32))
        return invalid("a float buffer is not 4-byte aligned");
    if ((const void*)out32 == (const void*)alpha || (const void*)out8 == (const void*)alpha ||
        (background && ((const void*)out32 == (const void*)background || (const void*)out8 == (const void*)background)))
        return invalid("an output is alpha_dev or background_dev");
    if ((const void*)out8 == (const void*)color) return invalid("out_u8_dev is color_dev");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFull) return unsupported("a frame of 2^31 pixels or more");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    composite_kernel<<<(unsigned)((pix + 255) / 256), 256, 0, (hipStream_t)stream_v>>>(
        pix, color, alpha, background, prm->background[0], prm->background[1], prm->background[2], out32, out8);
    return launched("composite");
}

}  // namespace rtm
