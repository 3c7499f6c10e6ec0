// rtm_bloom_kernel.h — bloom (include/rtm.h: rtm_bloom).  Included by rtm_bloom.hip.
//
// Four kernels, all fp32, no atomics.  A level is one plane of 16-byte records (r, g, b, 0).
//   bloom_bright_down_kernel  color -> level 1.  A block of 256 lanes makes a 32 x 8 tile of level 1: it loads the 66 x 18
//                             pixels of the tile and its halo into LDS, applies the count rule and the bright pass there,
//                             filters horizontally into LDS, then vertically, and stores one record per lane
//   bloom_down_kernel         level l-1 -> l: the same tile scheme on records
//   bloom_up_kernel           in place on level l: u_l = (1 - scatter) d_l + scatter up_l(u_{l+1}), one lane per record
//   bloom_combine_kernel      one lane per full-resolution pixel, blocks of 64 x 4 like the map kernel of the display
//                             transform: B = up_0(u_1), out = c + intensity B, the f32, u8 and bloom stores
// Every sum has one fixed order, so the same inputs give the same bits on every call.
#ifndef RTM_BLOOM_KERNEL_H
#define RTM_BLOOM_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kBlBlock = 256;                          // lanes of a block: four wave64s
constexpr int kBlTileX = 32, kBlTileY = 8;             // the coarse tile a down block makes
constexpr int kBlInX = 2 * kBlTileX + 2;               // 66: the fine columns 2 X0 - 1 .. 2 X0 + 64 under it
constexpr int kBlInY = 2 * kBlTileY + 2;               // 18 fine rows
constexpr int kBlRowVec = (3 * kBlInX + 3 + 3) / 4;    // 51: dwordx4 slots of a fine row, up to 3 floats of lead included
constexpr int kBlRowFloats = 4 * kBlRowVec;            // 204: the LDS stride of a fine row, 16-byte aligned
constexpr int kBlPixTileX = 64, kBlPixTileY = 4;       // the block of the per-pixel kernels (up, combine)

__device__ inline float bl_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ inline bool bl_counts(float r, float g, float b) {
    return __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b);
}

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t bl_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

// steps 1-2 of a pixel: b0, (0, 0, 0) for a pixel that does not count.  knee_t = knee * threshold
__device__ inline void bl_bright(float& r, float& g, float& b, const float threshold, const float knee_t) {
    if (!bl_counts(r, g, b)) {
        r = g = b = 0.0f;
        return;
    }
    r = fmaxf(r, 0.0f);
    g = fmaxf(g, 0.0f);
    b = fmaxf(b, 0.0f);
    const float y = bl_lum(r, g, b);
    float soft = fminf(fmaxf(y - threshold + knee_t, 0.0f), 2.0f * knee_t);
    soft = soft * soft / (4.0f * knee_t + 1e-5f);
    const float gain = fmaxf(soft, y - threshold) / fmaxf(y, 1e-5f);
    r *= gain;
    g *= gain;
    b *= gain;
}

// The four weights of step 3 for the coarse index X over a fine side of n, already divided by the sum of those in the
// frame; a tap outside has weight 0 (and reads a zero).  The tap 2X is always inside.
__device__ inline void bl_down_weights(const int X, const int n, float w[4]) {
    const float k0 = 2 * X - 1 >= 0 ? 0.125f : 0.0f, k2 = 2 * X + 1 < n ? 0.375f : 0.0f, k3 = 2 * X + 2 < n ? 0.125f : 0.0f;
    const float inv = 1.0f / ((k0 + 0.375f) + (k2 + k3));
    w[0] = k0 * inv;
    w[1] = 0.375f * inv;
    w[2] = k2 * inv;
    w[3] = k3 * inv;
}

// What both down kernels do once the fine tile is in `fine` (kBlInY rows of kBlRowFloats floats; the pixel of local column
// i, fine column 2 X0 - 1 + i, at float lead[row] + 3 i, out-of-frame pixels zero): the horizontal pass into `hor`
// ([3][kBlInY][kBlTileX]), the vertical pass, one record per lane.  Wf x Hf the fine level, Wc x Hc the coarse one.
__device__ inline void bl_filter_tile(const float* fine, const int* lead, float* hor, const int X0, const int Y0, const int Wf,
                                      const int Hf, const int Wc, const int Hc, float4* __restrict__ dst) {
    for (int it = (int)threadIdx.x; it < kBlInY * kBlTileX; it += kBlBlock) {
        const int r = it / kBlTileX, xl = it % kBlTileX;
        if (X0 + xl >= Wc) continue;
        float w[4];
        bl_down_weights(X0 + xl, Wf, w);
        const float* p = fine + r * kBlRowFloats + lead[r] + 3 * (2 * xl);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            hor[(c * kBlInY + r) * kBlTileX + xl] = (w[0] * p[c] + w[1] * p[3 + c]) + (w[2] * p[6 + c] + w[3] * p[9 + c]);
    }
    __syncthreads();
    const int xl = (int)threadIdx.x % kBlTileX, yl = (int)threadIdx.x / kBlTileX;
    const int X = X0 + xl, Y = Y0 + yl;
    if (X >= Wc || Y >= Hc) return;
    float w[4];
    bl_down_weights(Y, Hf, w);
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = hor + (c * kBlInY + 2 * yl) * kBlTileX + xl;
        o[c] = (w[0] * p[0] + w[1] * p[kBlTileX]) + (w[2] * p[2 * kBlTileX] + w[3] * p[3 * kBlTileX]);
    }
    dst[(size_t)Y * Wc + X] = make_float4(o[0], o[1], o[2], 0.0f);
}

#ifndef RTM_BLOOM_FILTERS_ONLY  // rtm_tonemap_local_kernel.h shares the filters above and bl_up_taps, not the kernels
// color -> level 1.  Fine row r of the tile starts at float a = 3 ((2 Y0 - 1 + r) W + 2 X0 - 1) of the frame; its slots
// are the dwordx4s from a rounded down to a multiple of four, so lead = a mod 4 floats precede the first pixel.  VEC: color
// is 16-byte aligned and a slot that lies inside the frame's floats is one dwordx4 load; the plain path reads the same floats
// as dwords, hence the same bits.  A slot may hold floats of the row before or after (never of outside the frame's
// memory): the bright pass overwrites every out-of-frame pixel with zero.
template <bool VEC>
__global__ __launch_bounds__(kBlBlock) void bloom_bright_down_kernel(const int W, const int H, const int Wc, const int Hc,
                                                                     const int tiles_x, const float* __restrict__ color,
                                                                     const float threshold, const float knee_t,
                                                                     float4* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) float fine[kBlInY * kBlRowFloats];
    __shared__ float hor[3 * kBlInY * kBlTileX];
    __shared__ int lead[kBlInY];
    const int X0 = ((int)blockIdx.x % tiles_x) * kBlTileX, Y0 = ((int)blockIdx.x / tiles_x) * kBlTileY;
    const long long total = 3ll * W * H;
    for (int it = (int)threadIdx.x; it < kBlInY * kBlRowVec; it += kBlBlock) {
        const int r = it / kBlRowVec, j = it % kBlRowVec;
        const int y = 2 * Y0 - 1 + r;
        const long long a = 3ll * ((long long)y * W + (2 * X0 - 1));
        if (j == 0) lead[r] = (int)(a & 3);
        if (y < 0 || y >= H) continue;
        const long long g = (a & ~3ll) + 4 * j;
        float4 v;
        if (VEC && g >= 0 && g + 4 <= total) {
            v = *(const float4*)(color + g);
        } else {
            v.x = (g >= 0 && g < total) ? color[g] : 0.0f;
            v.y = (g + 1 >= 0 && g + 1 < total) ? color[g + 1] : 0.0f;
            v.z = (g + 2 >= 0 && g + 2 < total) ? color[g + 2] : 0.0f;
            v.w = (g + 3 >= 0 && g + 3 < total) ? color[g + 3] : 0.0f;
        }
        *(float4*)(fine + r * kBlRowFloats + 4 * j) = v;
    }
    __syncthreads();
    for (int it = (int)threadIdx.x; it < kBlInY * kBlInX; it += kBlBlock) {
        const int r = it / kBlInX, i = it % kBlInX;
        const int x = 2 * X0 - 1 + i, y = 2 * Y0 - 1 + r;
        float* p = fine + r * kBlRowFloats + lead[r] + 3 * i;
        float cr = 0.0f, cg = 0.0f, cb = 0.0f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            cr = p[0];
            cg = p[1];
            cb = p[2];
            bl_bright(cr, cg, cb, threshold, knee_t);
        }
        p[0] = cr;
        p[1] = cg;
        p[2] = cb;
    }
    __syncthreads();
    bl_filter_tile(fine, lead, hor, X0, Y0, W, H, Wc, Hc, dst);
}

// level l-1 (Wf x Hf records) -> level l (Wc x Hc)
__global__ __launch_bounds__(kBlBlock) void bloom_down_kernel(const int Wf, const int Hf, const int Wc, const int Hc,
                                                              const int tiles_x, const float4* __restrict__ src,
                                                              float4* __restrict__ dst) {
    __shared__ float fine[kBlInY * kBlRowFloats];
    __shared__ float hor[3 * kBlInY * kBlTileX];
    __shared__ int lead[kBlInY];
    const int X0 = ((int)blockIdx.x % tiles_x) * kBlTileX, Y0 = ((int)blockIdx.x / tiles_x) * kBlTileY;
    if (threadIdx.x < kBlInY) lead[threadIdx.x] = 0;
    for (int it = (int)threadIdx.x; it < kBlInY * kBlInX; it += kBlBlock) {
        const int r = it / kBlInX, i = it % kBlInX;
        const int x = 2 * X0 - 1 + i, y = 2 * Y0 - 1 + r;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (x >= 0 && x < Wf && y >= 0 && y < Hf) v = src[(size_t)y * Wf + x];
        float* p = fine + r * kBlRowFloats + 3 * i;
        p[0] = v.x;
        p[1] = v.y;
        p[2] = v.z;
    }
    __syncthreads();
    bl_filter_tile(fine, lead, hor, X0, Y0, Wf, Hf, Wc, Hc, dst);
}

#endif  // RTM_BLOOM_FILTERS_ONLY

// The taps and weights of step 4 for the fine index x over a coarse side of n: t0 and t1 are in the frame (an outside tap
// is moved onto the other one and weighs 0, which leaves the 3/4 tap with the whole weight: 0.75 / 0.75)
__device__ inline void bl_up_taps(const int x, const int n, int& t0, int& t1, float& w0, float& w1) {
    t0 = (x - 1) >> 1;  // floor division: x = 0 gives -1
    t1 = t0 + 1;
    w0 = (x & 1) ? 0.75f : 0.25f;
    w1 = 1.0f - w0;
    if (t0 < 0) {
        t0 = t1;
        w0 = 0.0f;
        w1 = 1.0f;
    }
    if (t1 >= n) {
        t1 = t0;
        w0 = 1.0f;
        w1 = 0.0f;
    }
}

#ifndef RTM_BLOOM_FILTERS_ONLY
// up(coarse)(x, y): the horizontal pairs first, then the rows
__device__ inline float4 bl_up(const float4* __restrict__ coarse, const int Wc, const int Hc, const int x, const int y) {
    int x0, x1, y0, y1;
    float wx0, wx1, wy0, wy1;
    bl_up_taps(x, Wc, x0, x1, wx0, wx1);
    bl_up_taps(y, Hc, y0, y1, wy0, wy1);
    const float4 a = coarse[(size_t)y0 * Wc + x0], b = coarse[(size_t)y0 * Wc + x1];
    const float4 c = coarse[(size_t)y1 * Wc + x0], d = coarse[(size_t)y1 * Wc + x1];
    float4 o;
    o.x = wy0 * (wx0 * a.x + wx1 * b.x) + wy1 * (wx0 * c.x + wx1 * d.x);
    o.y = wy0 * (wx0 * a.y + wx1 * b.y) + wy1 * (wx0 * c.y + wx1 * d.y);
    o.z = wy0 * (wx0 * a.z + wx1 * b.z) + wy1 * (wx0 * c.z + wx1 * d.z);
    o.w = 0.0f;
    return o;
}

// in place on level l (Wf x Hf): a lane reads its own record and four of level l+1 (Wc x Hc), and writes its own
__global__ __launch_bounds__(kBlPixTileX * kBlPixTileY) void bloom_up_kernel(const int Wf, const int Hf, const int Wc,
                                                                            const int Hc, const int tiles_x,
                                                                            const float4* __restrict__ coarse,
                                                                            const float scatter, float4* __restrict__ level) {
    const int x = ((int)blockIdx.x % tiles_x) * kBlPixTileX + (int)threadIdx.x % kBlPixTileX;
    const int y = ((int)blockIdx.x / tiles_x) * kBlPixTileY + (int)threadIdx.x / kBlPixTileX;
    if (x >= Wf || y >= Hf) return;
    const float4 u = bl_up(coarse, Wc, Hc, x, y);
    const size_t p = (size_t)y * Wf + x;
    const float4 d = level[p];
    const float keep = 1.0f - scatter;
    level[p] = make_float4(keep * d.x + scatter * u.x, keep * d.y + scatter * u.y, keep * d.z + scatter * u.z, 0.0f);
}

// color and out32 may be the same buffer: a lane reads its pixel before it writes it and touches no other.  A pixel that
// does not count keeps its words.
__global__ __launch_bounds__(kBlPixTileX * kBlPixTileY) void bloom_combine_kernel(const int W, const int H, const int Wc,
                                                                                 const int Hc, const int tiles_x,
                                                                                 const float* color,
                                                                                 const float4* __restrict__ level1,
                                                                                 const float intensity, float* out32,
                                                                                 uint8_t* __restrict__ out8,
                                                                                 float* __restrict__ bloom_out) {
    const int x = ((int)blockIdx.x % tiles_x) * kBlPixTileX + (int)threadIdx.x % kBlPixTileX;
    const int y = ((int)blockIdx.x / tiles_x) * kBlPixTileY + (int)threadIdx.x / kBlPixTileX;
    if (x >= W || y >= H) return;
    const float4 B = bl_up(level1, Wc, Hc, x, y);
    const size_t p = ((size_t)y * W + x) * 3;
    if (bloom_out) {
        bloom_out[p] = B.x;
        bloom_out[p + 1] = B.y;
        bloom_out[p + 2] = B.z;
    }
    if (!out32 && !out8) return;
    const uint32_t* words = (const uint32_t*)color;
    uint32_t wr = words[p], wg = words[p + 1], wb = words[p + 2];
    const float cr = __uint_as_float(wr), cg = __uint_as_float(wg), cb = __uint_as_float(wb);
    if (bl_counts(cr, cg, cb)) {
        wr = __float_as_uint(cr + intensity * B.x);
        wg = __float_as_uint(cg + intensity * B.y);
        wb = __float_as_uint(cb + intensity * B.z);
    }
    if (out32) {
        uint32_t* o = (uint32_t*)out32;
        o[p] = wr;
        o[p + 1] = wg;
        o[p + 2] = wb;
    }
    if (out8) {
        out8[p] = bl_quantise(__uint_as_float(wr));
        out8[p + 1] = bl_quantise(__uint_as_float(wg));
        out8[p + 2] = bl_quantise(__uint_as_float(wb));
    }
}

#endif  // RTM_BLOOM_FILTERS_ONLY

}  // namespace rtm
#endif
