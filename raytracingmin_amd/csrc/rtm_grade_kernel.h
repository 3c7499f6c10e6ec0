// rtm_grade_kernel.h — the colour grade (include/rtm.h: rtm_grade).  Included by rtm_grade.hip.
//
// One kernel, no LDS, no atomics, no scratch.  Nothing in the grade depends on where a pixel lies, so the frame is taken as
// a flat run of pixels: a block of 256 lanes owns 256 consecutive pixels, one pixel a lane, and a wave's loads and stores
// cover 768 bytes without a gap.  A lane reads its pixel before it writes it and touches no other, so the call may run in
// place.
//   steps   which of matrix, exposure, contrast, CDL and saturation are live is decided on the host (rtm.h: a step whose
//           parameters all equal their defaults is skipped) and arrives as bits of GrArgs::live: every branch on them is
//           wave-uniform, a scalar compare and jump, so a dead step costs no vector work and "matrix only" stays a copy
//           with nine multiplies.  The three pow sites (contrast, and the CDL power per channel) are exp2(p log2(v)) on the
//           transcendental unit; a CDL channel whose power is 1 skips its own.
//   LUT     instantiated on the interpolation (none, trilinear, tetrahedral), which decides how many table entries a lane
//           gathers: 8 or 4 of three floats, straight from global memory through the caches.  Neighbouring pixels of an
//           image fall into neighbouring cells, and a 33^3 table (431 KB) fits an XCD's L2 many times over.  Every index
//           comes from gr_lut_index (rtm_grade_index.h), whose cell is in [0, N - 2] for any float: no read leaves the table.
#ifndef RTM_GRADE_KERNEL_H
#define RTM_GRADE_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"
#include "rtm_grade_index.h"

namespace rtm {

constexpr int kGrBlock = 256;  // lanes, and pixels, of a block: four wave64s

// the live steps (GrArgs::live)
enum : uint32_t { kGrMatrix = 1u, kGrExposure = 2u, kGrContrast = 4u, kGrCdl = 8u, kGrSaturation = 16u };
// the kernel's LUT template argument
enum { kGrLutNone = 0, kGrLutTrilinear = 1, kGrLutTetrahedral = 2 };

// the kernel's arguments beyond the pointers
struct GrArgs {
    uint32_t pixels;  // fewer than 2^31
    uint32_t live;    // kGr* bits
    float m[9];
    float gain;  // (float)exp2((double)exposure)
    float contrast, pivot;
    float slope[3], offset[3], power[3];
    float saturation;
    int n;                  // the table's size per axis
    float lo[3], inv[3];    // inv_c = (float)((double)(n - 1) / ((double)hi_c - (double)lo_c))
};

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t gr_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

// pow(v, p) for v >= 0 and p > 0 in the device's fast form: log2(0) = -inf, so pow(0, p) = 0; pow(inf, p) = inf
__device__ inline float gr_pow(float v, float p) { return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(v)); }

__device__ inline float gr_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// step 6 for one pixel: y[] in, the interpolated entry out
template <int LUT>
__device__ inline void gr_lut(const GrArgs& a, const float* __restrict__ lut, float* y) {
    int i[3];
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gr_lut_index((y[c] - a.lo[c]) * a.inv[c], a.n, i[c], f[c]);
    // i[c] is in [0, n - 2]: the entries (i_r + {0,1}, i_g + {0,1}, i_b + {0,1}) lie inside the 3 n^3 floats
    const int sr = 3, sg = 3 * a.n, sb = 3 * a.n * a.n;
    const float* const t = lut + (i[0] * sr + i[1] * sg + i[2] * sb);
    if constexpr (LUT == kGrLutTrilinear) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float c000 = t[c], c100 = t[sr + c], c010 = t[sg + c], c110 = t[sg + sr + c];
            const float c001 = t[sb + c], c101 = t[sb + sr + c], c011 = t[sb + sg + c], c111 = t[sb + sg + sr + c];
            const float c00 = c000 + f[0] * (c100 - c000), c10 = c010 + f[0] * (c110 - c010);
            const float c01 = c001 + f[0] * (c101 - c001), c11 = c011 + f[0] * (c111 - c011);
            const float c0 = c00 + f[1] * (c10 - c00), c1 = c01 + f[1] * (c11 - c01);
            y[c] = c0 + f[2] * (c1 - c0);
        }
    } else {
        // the fractions descending, a tie taking the earlier channel first: (f1, s1) >= (f2, s2) >= (f3, ·)
        float f1, f2, f3;
        int s1, s2;
        if (f[0] >= f[1]) {
            if (f[1] >= f[2]) f1 = f[0], f2 = f[1], f3 = f[2], s1 = sr, s2 = sg;
            else if (f[0] >= f[2]) f1 = f[0], f2 = f[2], f3 = f[1], s1 = sr, s2 = sb;
            else f1 = f[2], f2 = f[0], f3 = f[1], s1 = sb, s2 = sr;
        } else {
            if (f[0] >= f[2]) f1 = f[1], f2 = f[0], f3 = f[2], s1 = sg, s2 = sr;
            else if (f[1] >= f[2]) f1 = f[1], f2 = f[2], f3 = f[0], s1 = sg, s2 = sb;
            else f1 = f[2], f2 = f[1], f3 = f[0], s1 = sb, s2 = sg;
        }
        const float w0 = 1.0f - f1, w1 = f1 - f2, w2 = f2 - f3;
        const float* const t1 = t + s1;
        const float* const t2 = t1 + s2;
        const float* const t3 = t + (sr + sg + sb);
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c] = ((w0 * t[c] + w1 * t1[c]) + w2 * t2[c]) + f3 * t3[c];
    }
}

// color and out32 may be the same buffer (in place); lut is read only and is no output
template <int LUT>
__global__ __launch_bounds__(kGrBlock) void grade_kernel(const GrArgs a, const float* color, const float* __restrict__ lut,
                                                         float* out32, uint8_t* __restrict__ out8) {
    const uint32_t pixel = blockIdx.x * (uint32_t)kGrBlock + threadIdx.x;
    if (pixel >= a.pixels) return;
    const size_t p = (size_t)pixel * 3;
    const uint32_t* const words = (const uint32_t*)color;
    uint32_t word[3] = {words[p], words[p + 1], words[p + 2]};  // what is stored: the input's words until a step changes them
    float y[3] = {__uint_as_float(word[0]), __uint_as_float(word[1]), __uint_as_float(word[2])};
    const bool counts = __builtin_isfinite(y[0]) && __builtin_isfinite(y[1]) && __builtin_isfinite(y[2]);
    if (counts && (a.live != 0u || LUT != kGrLutNone)) {
        if (a.live & kGrMatrix) {
            const float r = y[0], g = y[1], b = y[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = (a.m[3 * c] * r + a.m[3 * c + 1] * g) + a.m[3 * c + 2] * b;
        }
        if (a.live & kGrExposure) {
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = y[c] * a.gain;
        }
        if (a.live & kGrContrast) {
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = a.pivot * gr_pow(fmaxf(y[c], 0.0f) / a.pivot, a.contrast);
        }
        if (a.live & kGrCdl) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = fmaxf(y[c] * a.slope[c] + a.offset[c], 0.0f);
                y[c] = a.power[c] == 1.0f ? v : gr_pow(v, a.power[c]);
            }
        }
        if (a.live & kGrSaturation) {
            const float L = gr_lum(y[0], y[1], y[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = L + a.saturation * (y[c] - L);
        }
        if constexpr (LUT != kGrLutNone) gr_lut<LUT>(a, lut, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) word[c] = __float_as_uint(y[c]);
    }
    if (out32) {
        uint32_t* const ow = (uint32_t*)out32;
#pragma unroll
        for (int c = 0; c < 3; ++c) ow[p + c] = word[c];
    }
    if (out8) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out8[p + c] = gr_quantise(__uint_as_float(word[c]));
    }
}

}  // namespace rtm
#endif
