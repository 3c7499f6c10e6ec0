// rtm_firefly_kernel.h — the firefly clamp and the repair of non-finite pixels (include/rtm.h: rtm_firefly).  Included by
// rtm_firefly.hip.
//
// One kernel, fp32, no atomics.  A block of 512 lanes owns a 32 x 16 tile of pixels, one pixel a lane (rtm_defocus's shape).
//   fill     the tile and its halo of R pixels go into LDS as one plane of luminances: Y (step 1, >= 0) of a pixel that
//            counts, -1 for one outside the frame or one that does not count, so that one compare serves both skips.  At
//            R = 3 that is 38 x 22 floats, 3.3 KB.  Colours are not staged: a lane reads its own pixel's three floats again.
//   select   a lane walks its (2R+1)^2 - 1 taps in the plane and keeps the K largest in registers, sorted, by a branch-free
//            insertion chain: per tap, for j = 0..K-1: t = max(top[j], v); v = min(top[j], v); top[j] = t.  The -1 of a skipped
//            tap sinks through every Y, so the chain needs no branch; the lane counts its valid taps to know n < K.  A wave's
//            lanes read 32 consecutive floats of two rows with each ds_read_b32: free of bank conflicts at every R.
//   repair   only in a lane whose own pixel does not count, with repair on: rare and divergent.  It reads the colours of the
//            taps the plane marks as counting from global memory, dy outer and dx inner.
// The kernel is instantiated on R (1..3) and on K (1..8), so that the window loops and the chain unroll fully and top[] is
// never indexed by a run-time value (which would send it to scratch memory): 24 instantiations, none with scratch.
#ifndef RTM_FIREFLY_KERNEL_H
#define RTM_FIREFLY_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kFfTileX = 32, kFfTileY = 16;    // the tile of pixels a block owns
constexpr int kFfBlock = kFfTileX * kFfTileY;  // 512 lanes: eight wave64s, a wave covers two rows of the tile
constexpr int kFfMaxRadius = 3, kFfMaxRank = 8;
constexpr int ff_plane(int r) { return (kFfTileX + 2 * r) * (kFfTileY + 2 * r); }  // tile + halo

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t ff_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

// step 1: Y of a pixel that counts, -1 of one that does not
__device__ inline float ff_luminance(float r, float g, float b) {
    if (!(__builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b))) return -1.0f;
    const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    return l > 0.0f ? l : 0.0f;
}

template <int R, int K>
__global__ __launch_bounds__(kFfBlock) void firefly_kernel(const int W, const int H, const int tiles_x, const float k,
                                                           const float floor, const int repair, const float* __restrict__ color,
                                                           float* __restrict__ out32, uint8_t* __restrict__ out8,
                                                           uint8_t* __restrict__ mask_out, float* __restrict__ thr_out) {
    constexpr int IW = kFfTileX + 2 * R, IH = kFfTileY + 2 * R;
    __shared__ float lum[IW * IH];
    const int X0 = ((int)blockIdx.x % tiles_x) * kFfTileX, Y0 = ((int)blockIdx.x / tiles_x) * kFfTileY;
    for (int it = (int)threadIdx.x; it < IW * IH; it += kFfBlock) {
        const int iy = it / IW, ix = it - iy * IW;
        const int x = X0 - R + ix, y = Y0 - R + iy;
        float v = -1.0f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t q = (size_t)y * W + x;
            v = ff_luminance(color[3 * q], color[3 * q + 1], color[3 * q + 2]);
        }
        lum[it] = v;
    }
    __syncthreads();

    const int lx = (int)threadIdx.x % kFfTileX, ly = (int)threadIdx.x / kFfTileX;
    const int x = X0 + lx, y = Y0 + ly;
    if (x >= W || y >= H) return;  // (no barrier follows)
    const int centre = (ly + R) * IW + lx + R;
    const float Yp = lum[centre];
    float top[K];
#pragma unroll
    for (int j = 0; j < K; ++j) top[j] = -1.0f;
    int n = 0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if (dx == 0 && dy == 0) continue;  // (folded: the loops unroll)
            float v = lum[centre + dy * IW + dx];
            n += v >= 0.0f ? 1 : 0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float t = fmaxf(top[j], v);
                v = fminf(top[j], v);
                top[j] = t;
            }
        }
    }
    const bool counts = Yp >= 0.0f;
    const float T = (counts && n >= K) ? (k * top[K - 1]) + floor : __builtin_inff();
    const size_t p = (size_t)y * W + x;
    const uint32_t* words = (const uint32_t*)color;
    uint32_t wr = words[3 * p], wg = words[3 * p + 1], wb = words[3 * p + 2];  // the input, for the pixels that keep it
    uint8_t m = 0;
    if (counts) {
        if (Yp > T) {  // T is finite here, and >= 0
            const float s = T / Yp;
            wr = __float_as_uint(__uint_as_float(wr) * s);
            wg = __float_as_uint(__uint_as_float(wg) * s);
            wb = __float_as_uint(__uint_as_float(wb) * s);
            m = 1;
        }
    } else if (repair) {
        float sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                if (dx == 0 && dy == 0) continue;
                if (lum[centre + dy * IW + dx] >= 0.0f) {  // inside the frame, and it counts
                    const size_t q = (size_t)(y + dy) * W + (x + dx);
                    sr += color[3 * q];
                    sg += color[3 * q + 1];
                    sb += color[3 * q + 2];
                }
            }
        }
        const float fn = (float)n;
        wr = n ? __float_as_uint(sr / fn) : 0u;
        wg = n ? __float_as_uint(sg / fn) : 0u;
        wb = n ? __float_as_uint(sb / fn) : 0u;
        m = 2;
    }
    if (out32) {
        uint32_t* o = (uint32_t*)out32;
        o[3 * p] = wr;
        o[3 * p + 1] = wg;
        o[3 * p + 2] = wb;
    }
    if (out8) {
        out8[3 * p] = ff_quantise(__uint_as_float(wr));
        out8[3 * p + 1] = ff_quantise(__uint_as_float(wg));
        out8[3 * p + 2] = ff_quantise(__uint_as_float(wb));
    }
    if (mask_out) mask_out[p] = m;
    if (thr_out) thr_out[p] = T;
}

}  // namespace rtm
#endif
