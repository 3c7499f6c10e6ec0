// rtm_lens_kernel.h — lens distortion, chromatic aberration and vignette (include/rtm.h: rtm_lens).  Included by rtm_lens.hip.
//
// One kernel, no LDS, no atomics, no scratch.  A block of 256 lanes owns a 64 x 4 tile of output pixels, one pixel a lane
// and one row a wave: the tile is wide and short so that the taps of a wave, whose source positions run along a gently
// bent row, fall on a few source rows and every load of the wave touches a few cache lines.
//   position  the fp64 arithmetic of rtm.h step 1, once per pixel (ln_factor: shared with the host's rtm_lens_fit_zoom, so
//             that both decide "inside" from the same bits).  The Newton solve of INVERSE is shared by the three channels:
//             only m_c differs.
//   taps      gathered straight from global memory through the caches: 1 (NEAREST), 4 (BILINEAR) or 16 (BICUBIC) source
//             pixels per tap set.  With chroma = 0 the three channels share one tap set and one weight set; with chroma != 0
//             (CHROMA) each channel has its own, and a tap still reads all three components, because whether a pixel
//             counts is a property of the pixel.
//   border    decided per lane and per channel: a block whose corner positions are all outside the frame may still hold
//             inside pixels (a barrel's edge bends back in), so there is no block-level exit.
// Instantiated on (filter, channels, chroma != 0); mode and every other parameter are run-time values.
#ifndef RTM_LENS_KERNEL_H
#define RTM_LENS_KERNEL_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kLnTileX = 64, kLnTileY = 4;     // a block's tile: a wave a row
constexpr int kLnBlock = kLnTileX * kLnTileY;  // 256 lanes
constexpr int kLnNewtonSteps = 12;             // rtm.h: exactly 12
constexpr float kLnMinWeight = 0.0625f;        // rtm.h: D below it is a hole

// what the positions need, in double (rtm.h step 1); a3 = 3 k1 and b5 = 5 k2 are the products the Newton step names
struct LnMap {
    double cx, cy, R2, iz, k1, k2, a3, b5, chroma;
    int inverse;
};

inline LnMap ln_map(const rtm_lens_params& p, float zoom, int32_t w, int32_t h) {
    LnMap m;
    m.cx = (double)w / 2.0;
    m.cy = (double)h / 2.0;
    m.R2 = m.cx * m.cx + m.cy * m.cy;
    m.iz = 1.0 / (double)zoom;
    m.k1 = (double)p.k1;
    m.k2 = (double)p.k2;
    m.a3 = 3.0 * m.k1;
    m.b5 = 5.0 * m.k2;
    m.chroma = (double)p.chroma;
    m.inverse = p.mode == RTM_LENS_INVERSE;
    return m;
}

// F of rtm.h for the pixel whose centre is (dx, dy) from the frame's: the order of every operation is the header's
__host__ __device__ inline double ln_factor(const LnMap& m, const double dx, const double dy) {
    const double r2 = ((dx * dx + dy * dy) / m.R2) * (m.iz * m.iz);
    if (!m.inverse) return (1.0 + r2 * (m.k1 + r2 * m.k2)) * m.iz;
    const double r = sqrt(r2);
    double rho = r;
    for (int i = 0; i < kLnNewtonSteps; ++i) {
        const double t = rho * rho;
        rho = rho - (rho * (1.0 + t * (m.k1 + t * m.k2)) - r) / (1.0 + t * (m.a3 + t * m.b5));
    }
    return (r > 0.0 ? rho / r : 1.0) * m.iz;
}

// m_c = 1 + chroma (1 - c)
__host__ __device__ inline double ln_channel_scale(const LnMap& m, const int c) { return 1.0 + m.chroma * (double)(1 - c); }

// (u, v) of a channel whose factor is Fc, and whether it is inside the frame (false for a NaN position)
__host__ __device__ inline bool ln_position(const LnMap& m, const double dx, const double dy, const double Fc, const int w,
                                            const int h, double& u, double& v) {
    u = m.cx + dx * Fc - 0.5;
    v = m.cy + dy * Fc - 0.5;
    return u >= -0.5 && u < (double)w - 0.5 && v >= -0.5 && v < (double)h - 0.5;
}

// the kernel's arguments beyond the pointers
struct LnArgs {
    LnMap map;
    int w, h, tiles_x;
    float vignette, falloff2;  // falloff2 = falloff * falloff, in float
    uint32_t border[3];        // border[c]'s words
};

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t ln_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

// the first tap and the float weights of an axis at source coordinate u (inside: floor(u) is in -1 .. n - 1)
template <int FILTER>
__device__ inline int ln_weights(const double u, float* wt) {
    const double f = floor(u), t = u - f;
    if (FILTER == RTM_LENS_BILINEAR) {
        wt[0] = (float)(1.0 - t);
        wt[1] = (float)t;
        return (int)f;
    }
    wt[0] = (float)((((2.0 - t) * t - 1.0) * t) / 2.0);
    wt[1] = (float)((((3.0 * t - 5.0) * t) * t + 2.0) / 2.0);
    wt[2] = (float)((((4.0 - 3.0 * t) * t + 1.0) * t) / 2.0);
    wt[3] = (float)((((t - 1.0) * t) * t) / 2.0);
    return (int)f - 1;
}

// N (all C components) and D of the tap set at (u, v): rows outer, columns inner, ascending; a tap outside the frame or one
// that does not count is skipped
template <int FILTER, int C>
__device__ inline void ln_sample(const float* __restrict__ src, const int w, const int h, const double u, const double v,
                                 float* n, float& d) {
    constexpr int T = FILTER == RTM_LENS_BILINEAR ? 2 : 4;
    float wx[T], wy[T];
    const int x0 = ln_weights<FILTER>(u, wx), y0 = ln_weights<FILTER>(v, wy);
#pragma unroll
    for (int k = 0; k < C; ++k) n[k] = 0.0f;
    d = 0.0f;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int y = y0 + j;
        if (y < 0 || y >= h) continue;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const int x = x0 + i;
            if (x < 0 || x >= w) continue;
            const size_t p = ((size_t)y * (size_t)w + (size_t)x) * C;  // inside the frame: the bounds were just checked
            float c[C];
            bool counts = true;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                c[k] = src[p + k];
                counts = counts && __builtin_isfinite(c[k]);
            }
            if (!counts) continue;
            const float wgt = wx[i] * wy[j];
#pragma unroll
            for (int k = 0; k < C; ++k) n[k] += wgt * c[k];
            d += wgt;
        }
    }
}

template <int FILTER, int C, bool CHROMA>
__global__ __launch_bounds__(kLnBlock) void lens_kernel(const LnArgs a, const float* __restrict__ src,
                                                        float* __restrict__ out32, uint8_t* __restrict__ out8) {
    static_assert(C == 1 || C == 3, "a plane or a frame");
    static_assert(!CHROMA || (C == 3 && FILTER != RTM_LENS_NEAREST), "chroma needs three channels and a filter that weighs");
    const int X = ((int)blockIdx.x % a.tiles_x) * kLnTileX + (int)threadIdx.x % kLnTileX;
    const int Y = ((int)blockIdx.x / a.tiles_x) * kLnTileY + (int)threadIdx.x / kLnTileX;
    if (X >= a.w || Y >= a.h) return;  // (no barrier in this kernel)
    const double dx = ((double)X + 0.5) - a.map.cx, dy = ((double)Y + 0.5) - a.map.cy;
    const double F = ln_factor(a.map, dx, dy);
    uint32_t word[C];  // the output's words
    bool inside[C];
    if (FILTER == RTM_LENS_NEAREST) {
        double u, v;
        const bool in = ln_position(a.map, dx, dy, F, a.w, a.h, u, v);
        // (inside: u + 0.5 is in [0, w], and w itself only by the rounding of the sum)
        const int xs = in ? min((int)floor(u + 0.5), a.w - 1) : 0, ys = in ? min((int)floor(v + 0.5), a.h - 1) : 0;
        const uint32_t* words = (const uint32_t*)src;
        const size_t p = ((size_t)ys * (size_t)a.w + (size_t)xs) * C;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            inside[k] = in;
            word[k] = in ? words[p + k] : a.border[k];
        }
    } else {
        const float qnan = __uint_as_float(0x7FC00000u);
        float val[C];
        if (CHROMA) {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                double u, v;
                inside[k] = ln_position(a.map, dx, dy, F * ln_channel_scale(a.map, k), a.w, a.h, u, v);
                val[k] = 0.0f;
                if (inside[k]) {
                    float n[C], d;
                    ln_sample<FILTER, C>(src, a.w, a.h, u, v, n, d);
                    val[k] = d >= kLnMinWeight ? n[k] / d : qnan;
                }
            }
        } else {
            double u, v;
            const bool in = ln_position(a.map, dx, dy, F, a.w, a.h, u, v);  // m_c = 1.0: F_c = F
            float n[C], d = 0.0f;
#pragma unroll
            for (int k = 0; k < C; ++k) n[k] = 0.0f;
            if (in) ln_sample<FILTER, C>(src, a.w, a.h, u, v, n, d);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                inside[k] = in;
                val[k] = d >= kLnMinWeight ? n[k] / d : qnan;
            }
        }
        // the vignette of rtm.h step 5: vignette = 0 gives gain = 1 exactly
        const float rv = (float)((dx * dx + dy * dy) / a.map.R2);
        const float q = 1.0f + a.falloff2 * rv;
        const float c4 = 1.0f / (q * q);
        const float gain = 1.0f - a.vignette * (1.0f - c4);
#pragma unroll
        for (int k = 0; k < C; ++k) word[k] = inside[k] ? __float_as_uint(val[k] * gain) : a.border[k];
    }
    const size_t o = ((size_t)Y * (size_t)a.w + (size_t)X) * C;
    if (out32) {
        uint32_t* const ow = (uint32_t*)out32;
#pragma unroll
        for (int k = 0; k < C; ++k) ow[o + k] = word[k];
    }
    if (out8) {
#pragma unroll
        for (int k = 0; k < C; ++k) out8[o + k] = ln_quantise(__uint_as_float(word[k]));
    }
}

}  // namespace rtm
#endif
