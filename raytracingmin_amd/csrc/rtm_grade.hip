// rtm_grade.hip — rtm_grade (include/rtm.h): argument checks, which steps are live, the host's two derived numbers (the
// exposure gain and the LUT's scale per channel) and the one launch of rtm_grade_kernel.h.  The call keeps no state and
// needs no work buffer: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "rtm_grade_kernel.h"
#include "rtm_host.h"

namespace rtm {

namespace {
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
bool within(float v, float lo, float hi) { return v >= lo && v <= hi; }  // false for a NaN
bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// what rtm_grade refuses of the parameters: the refusal's text, or null
const char* bad_params(const rtm_grade_params& p) {
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(p.matrix[k])) return "matrix holds a NaN or an infinity";
    if (!std::isfinite(p.exposure) || std::fabs(p.exposure) > 32.0f) return "exposure is NaN, infinite or |ev| > 32";
    if (!within(p.contrast, 0.25f, 4.0f)) return "contrast is NaN or outside [0.25, 4]";
    if (!std::isfinite(p.pivot) || !(p.pivot > 0.0f)) return "pivot is NaN, infinite or not positive";
    if (!finite3(p.slope) || p.slope[0] < 0.0f || p.slope[1] < 0.0f || p.slope[2] < 0.0f) return "slope is NaN, infinite or negative";
    if (!finite3(p.offset)) return "offset is NaN or infinite";
    for (int c = 0; c < 3; ++c)
        if (!within(p.power[c], 0.1f, 10.0f)) return "power is NaN or outside [0.1, 10]";
    if (!within(p.saturation, 0.0f, 4.0f)) return "saturation is NaN or outside [0, 4]";
    if (p.lut_size != 0 && (p.lut_size < 2 || p.lut_size > 256)) return "lut_size is neither 0 nor in 2..256";
    if (p.lut_interp != RTM_GRADE_TRILINEAR && p.lut_interp != RTM_GRADE_TETRAHEDRAL) return "lut_interp is not an RTM_GRADE_* value";
    if (!finite3(p.lut_min) || !finite3(p.lut_max)) return "lut_min or lut_max is NaN or infinite";
    for (int c = 0; c < 3; ++c)
        if (!(p.lut_max[c] > p.lut_min[c])) return "lut_max <= lut_min in a channel";
    return nullptr;
}

// the live steps (rtm.h: a step whose parameters all equal their defaults exactly is skipped)
uint32_t live_steps(const rtm_grade_params& p) {
    static const float identity[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    uint32_t live = 0;
    for (int k = 0; k < 9; ++k)
        if (p.matrix[k] != identity[k]) live |= kGrMatrix;
    if (p.exposure != 0.0f) live |= kGrExposure;
    if (p.contrast != 1.0f || p.pivot != 0.18f) live |= kGrContrast;
    for (int c = 0; c < 3; ++c)
        if (p.slope[c] != 1.0f || p.offset[c] != 0.0f || p.power[c] != 1.0f) live |= kGrCdl;
    if (p.saturation != 1.0f) live |= kGrSaturation;
    return live;
}
}  // namespace

int grade(const rtm_grade_params* prm, int32_t width, int32_t height, int device, const float* color, const float* lut,
          float* out32, uint8_t* out8, void* stream_v) {
    if (!prm || !color) return invalid("null params or color_dev");
    if (!out32 && !out8) return invalid("every output is null: out_f32_dev and out_u8_dev");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size (width, height)");
    if (const char* why = bad_params(*prm)) return invalid(why);
    if (prm->lut_size > 0 && !lut) return invalid("lut_dev is null with lut_size > 0");
    if (prm->lut_size == 0 && lut) return invalid("lut_dev is not null with lut_size = 0");
    if (!aligned4(color) || !aligned4(out32) || !aligned4(lut))
        return invalid("a float buffer (color_dev, lut_dev, out_f32_dev) is not 4-byte aligned");
    if (lut && ((const void*)lut == (const void*)out32 || (const void*)lut == (const void*)out8))
        return invalid("lut_dev aliases an output");
    if (out8 && (const void*)out8 == (const void*)color) return invalid("out_u8_dev aliases color_dev");
    if ((uint64_t)width * (uint64_t)height >= ((uint64_t)1 << 31)) return unsupported("frame too large for grade: 2^31 pixels or more");
    if (device < 0) return invalid("negative device");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    GrArgs a;
    a.pixels = (uint32_t)((uint64_t)width * (uint64_t)height);
    a.live = live_steps(*prm);
    std::memcpy(a.m, prm->matrix, sizeof a.m);
    a.gain = (float)std::exp2((double)prm->exposure);
    a.contrast = prm->contrast;
    a.pivot = prm->pivot;
    std::memcpy(a.slope, prm->slope, sizeof a.slope);
    std::memcpy(a.offset, prm->offset, sizeof a.offset);
    std::memcpy(a.power, prm->power, sizeof a.power);
    a.saturation = prm->saturation;
    a.n = prm->lut_size;
    for (int c = 0; c < 3; ++c) {
        a.lo[c] = prm->lut_min[c];
        a.inv[c] = (float)((double)(prm->lut_size - 1) / ((double)prm->lut_max[c] - (double)prm->lut_min[c]));
    }
    const unsigned grid = (a.pixels + kGrBlock - 1) / kGrBlock;  // fewer than 2^23 blocks
    if (prm->lut_size == 0)
        grade_kernel<kGrLutNone><<<grid, kGrBlock, 0, stream>>>(a, color, nullptr, out32, out8);
    else if (prm->lut_interp == RTM_GRADE_TRILINEAR)
        grade_kernel<kGrLutTrilinear><<<grid, kGrBlock, 0, stream>>>(a, color, lut, out32, out8);
    else
        grade_kernel<kGrLutTetrahedral><<<grid, kGrBlock, 0, stream>>>(a, color, lut, out32, out8);
    return launched("grade");
}

}  // namespace rtm
