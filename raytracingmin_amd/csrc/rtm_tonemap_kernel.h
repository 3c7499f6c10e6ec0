// rtm_tonemap_kernel.h — the display transform (include/rtm.h: rtm_tonemap).  Included by rtm_tonemap.hip.
//
// Three kernels, all fp32 except the sum of logarithms, which is carried in double:
//   tonemap_partial_kernel  blocks of 256 lanes; block b reduces the pixels [4096 b, 4096 (b + 1)) of the flattened frame
//                           to one 16-byte partial (double sum of log(1e-4 + Y), float max Y, uint32 count)
//   tonemap_final_kernel    one block: folds the partials in ascending order, derives L_avg, L_max, E and W and leaves them
//                           in the work buffer's last 256 bytes (and in stats_out)
//   tonemap_map_kernel      one lane per pixel, blocks of 64 x 4 pixels like the denoiser: exposure, tone curve, transfer
//                           function, the f32 store and the (dithered) 8-bit store
// No atomics; every reduction is a fixed tree over counts that depend on the frame size alone, so the same inputs give the
// same bits on every call.
#ifndef RTM_TONEMAP_KERNEL_H
#define RTM_TONEMAP_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kTmBlock = 256;                                        // lanes of a reduction block: four wave64s
constexpr int kTmGroup = 4;                                          // pixels a lane takes at once: 48 B, three dwordx4 loads
constexpr int kTmRounds = 4;                                         // groups per lane
constexpr int kTmBlockPixels = kTmBlock * kTmGroup * kTmRounds;      // 4096
constexpr int kTmTileX = 64, kTmTileY = 4;                           // the map kernel's block of pixels
// the floats of the work buffer's last 256 bytes, written by tonemap_final_kernel
enum { kTmFinLavg = 0, kTmFinLmax = 1, kTmFinE = 2, kTmFinPixels = 3, kTmFinW = 4 };

struct TmPartial {  // 16 bytes
    double sum_log;
    float max_y;
    uint32_t count;
};

__device__ inline float tm_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ inline bool tm_counts(float r, float g, float b) {
    return __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b);
}
__device__ inline float tm_log(float v) { return __builtin_amdgcn_logf(v) * 0.6931471805599453f; }

__device__ inline void tm_take(TmPartial& a, float r, float g, float b) {
    if (!tm_counts(r, g, b)) return;
    const float y = fmaxf(tm_lum(r, g, b), 0.0f);
    a.sum_log += (double)tm_log(1e-4f + y);
    a.max_y = fmaxf(a.max_y, y);
    a.count += 1u;
}

// a + b of two partials; the callers fix the order
__device__ inline TmPartial tm_fold(const TmPartial& a, const TmPartial& b) {
    return TmPartial{a.sum_log + b.sum_log, fmaxf(a.max_y, b.max_y), a.count + b.count};
}

// butterfly over the 64 lanes of a wave (xor 32, 16, .. 1): every lane ends with the same bits
__device__ inline TmPartial tm_wave_fold(TmPartial a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        TmPartial o;
        o.sum_log = __shfl_xor(a.sum_log, m, 64);
        o.max_y = __shfl_xor(a.max_y, m, 64);
        o.count = __shfl_xor(a.count, m, 64);
        a = tm_fold(a, o);
    }
    return a;
}

// the block's four wave results through LDS, folded in wave order by lane 0; valid in lane 0 only
__device__ inline TmPartial tm_block_fold(TmPartial a, TmPartial* lds) {
    a = tm_wave_fold(a);
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = lds[0];
#pragma unroll
        for (int w = 1; w < kTmBlock / 64; ++w) a = tm_fold(a, lds[w]);
    }
    return a;
}

// Lane t of block b takes, in round j, the four pixels from 4096 b + 4 (256 j + t): a wave's loads of a round cover 3 KiB
// without a gap.  VEC: color is 16-byte aligned, so a group that lies inside the frame is three dwordx4 loads; the plain
// path reads the same pixels in the same order with dword loads, hence the same bits.
template <bool VEC>
__global__ __launch_bounds__(kTmBlock) void tonemap_partial_kernel(const float* __restrict__ color, const size_t pixels,
                                                                   TmPartial* __restrict__ partials) {
    __shared__ TmPartial lds[kTmBlock / 64];
    TmPartial a{0.0, 0.0f, 0u};
    const size_t base = (size_t)blockIdx.x * kTmBlockPixels;
#pragma unroll
    for (int j = 0; j < kTmRounds; ++j) {
        const size_t p0 = base + (size_t)kTmGroup * (size_t)(j * kTmBlock + (int)threadIdx.x);
        if (VEC && p0 + kTmGroup <= pixels) {
            const float4* v = (const float4*)(color + p0 * 3);
            const float4 q0 = v[0], q1 = v[1], q2 = v[2];
            tm_take(a, q0.x, q0.y, q0.z);
            tm_take(a, q0.w, q1.x, q1.y);
            tm_take(a, q1.z, q1.w, q2.x);
            tm_take(a, q2.y, q2.z, q2.w);
        } else {
#pragma unroll
            for (int k = 0; k < kTmGroup; ++k) {
                const size_t p = p0 + k;
                if (p < pixels) tm_take(a, color[p * 3], color[p * 3 + 1], color[p * 3 + 2]);
            }
        }
    }
    a = tm_block_fold(a, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

// One block.  Lane t folds the partials t, t + 256, .. in ascending order, then the block tree.  e_scale = 2^ev (from the
// host, so that a call that skips the statistics uses the same bits).  fin: the work buffer's last 256 bytes.
__global__ __launch_bounds__(kTmBlock) void tonemap_final_kernel(const TmPartial* __restrict__ partials, const uint32_t n_partials,
                                                                 const float e_scale, const int auto_exposure, const float key,
                                                                 const float white, float* __restrict__ fin,
                                                                 rtm_tonemap_stats* __restrict__ stats_out) {
    __shared__ TmPartial lds[kTmBlock / 64];
    TmPartial a{0.0, 0.0f, 0u};
    for (uint32_t i = threadIdx.x; i < n_partials; i += kTmBlock) a = tm_fold(a, partials[i]);
    a = tm_block_fold(a, lds);
    if (threadIdx.x != 0) return;
    float l_avg = 1.0f, l_max = 1.0f;
    if (a.count != 0u) {
        l_avg = __builtin_amdgcn_exp2f((float)(a.sum_log / (double)a.count) * 1.4426950408889634f);
        l_max = a.max_y;
    }
    const float e = auto_exposure ? e_scale * (key / l_avg) : e_scale;
    fin[kTmFinLavg] = l_avg;
    fin[kTmFinLmax] = l_max;
    fin[kTmFinE] = e;
    fin[kTmFinPixels] = __uint_as_float(a.count);
    fin[kTmFinW] = white > 0.0f ? white : e * l_max;
    if (stats_out) {
        stats_out->log_average = l_avg;
        stats_out->max_luminance = l_max;
        stats_out->exposure = e;
        stats_out->pixels = a.count;
    }
}

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t tm_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

// the 8 x 8 Bayer index of (x & 7, y & 7): bit i of x ^ y and of y interleaved, the lowest bit of the coordinates highest
__device__ inline uint32_t tm_bayer(uint32_t x, uint32_t y) {
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        b |= ((((x >> i) ^ (y >> i)) & 1u) << (2 * (2 - i) + 1)) | (((y >> i) & 1u) << (2 * (2 - i)));
    return b;
}

__device__ inline uint8_t tm_dither(float t, float bias) {  // bias = (B + 0.5) / 64
    return (uint8_t)fminf(255.0f, floorf(255.0f * t + bias));
}

__device__ inline float tm_aces(float x) {
    // past 1e4 the curve is above 1.03 and the result is clamped to 1 either way; the cap keeps x * x finite
    x = fminf(x, 1e4f);
    return x * (2.51f * x + 0.03f) / (x * (2.43f * x + 0.59f) + 0.14f);
}

__device__ inline float tm_transfer_srgb(float t) {
    return t <= 0.0031308f ? 12.92f * t : 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(t) * (1.0f / 2.4f)) - 0.055f;
}

// fin non-null: E and W are what tonemap_final_kernel left (one uniform load per wave); else the arguments (a call that
// skipped the statistics).  color and out32 may be the same buffer: a lane reads its pixel before it writes it and
// touches no other.
template <int OP, int TRANSFER, int DITHER>
__global__ __launch_bounds__(kTmTileX * kTmTileY) void tonemap_map_kernel(const int W, const int H, const int tiles_x,
                                                                         const float* color, const float* __restrict__ fin,
                                                                         const float e_arg, const float w_arg, float* out32,
                                                                         uint8_t* __restrict__ out8) {
    const int tile = (int)blockIdx.x;
    const int x = (tile % tiles_x) * kTmTileX + (int)threadIdx.x % kTmTileX;
    const int y = (tile / tiles_x) * kTmTileY + (int)threadIdx.x / kTmTileX;
    if (x >= W || y >= H) return;
    const float E = fin ? fin[kTmFinE] : e_arg;
    const size_t p = ((size_t)y * W + x) * 3;
    const float cr = color[p], cg = color[p + 1], cb = color[p + 2];
    float tr = 0.0f, tg = 0.0f, tb = 0.0f;
    if (tm_counts(cr, cg, cb)) {
        const float xr = fmaxf(cr * E, 0.0f), xg = fmaxf(cg * E, 0.0f), xb = fmaxf(cb * E, 0.0f);
        if constexpr (OP == RTM_TONEMAP_REINHARD) {
            const float Wp = fin ? fin[kTmFinW] : w_arg;
            const float yx = tm_lum(xr, xg, xb);
            const float s = (yx > 0.0f && Wp > 0.0f) ? (1.0f + yx / (Wp * Wp)) / (1.0f + yx) : 1.0f;
            tr = xr * s;
            tg = xg * s;
            tb = xb * s;
        } else if constexpr (OP == RTM_TONEMAP_ACES) {
            tr = tm_aces(xr);
            tg = tm_aces(xg);
            tb = tm_aces(xb);
        } else {
            tr = xr;
            tg = xg;
            tb = xb;
        }
        tr = fminf(fmaxf(tr, 0.0f), 1.0f);
        tg = fminf(fmaxf(tg, 0.0f), 1.0f);
        tb = fminf(fmaxf(tb, 0.0f), 1.0f);
        if constexpr (TRANSFER == RTM_TRANSFER_SRGB) {
            tr = tm_transfer_srgb(tr);
            tg = tm_transfer_srgb(tg);
            tb = tm_transfer_srgb(tb);
        }
    }
    if (out32) {
        out32[p] = tr;
        out32[p + 1] = tg;
        out32[p + 2] = tb;
    }
    if (out8) {
        if constexpr (DITHER) {
            const float bias = ((float)tm_bayer((uint32_t)x & 7u, (uint32_t)y & 7u) + 0.5f) / 64.0f;
            out8[p] = tm_dither(tr, bias);
            out8[p + 1] = tm_dither(tg, bias);
            out8[p + 2] = tm_dither(tb, bias);
        } else {
            out8[p] = tm_quantise(tr);
            out8[p + 1] = tm_quantise(tg);
            out8[p + 2] = tm_quantise(tb);
        }
    }
}

}  // namespace rtm
#endif
