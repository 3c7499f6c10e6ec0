// rtm_tonemap_local_kernel.h — the local tone operator (include/rtm.h: rtm_tonemap_local).  Included by
// rtm_tonemap_local.hip.
//
// Four kernels, all fp32, no atomics.  A level l >= 1 is two planes of 16-byte records: (GI_0, GI_1, GI_2, R) and
// (GW_0, GW_1, GW_2, 0).  Level 0 is never stored: I and w^ are pointwise in the colour.
//   local_base_down_kernel  color -> level 1.  rtm_bloom's tile scheme: a block of 256 lanes makes a 32 x 8 tile of level 1
//                           out of the 66 x 18 pixels under it.  It loads them into LDS, turns each into its three I there,
//                           filters, turns the I in place into the three w^ and filters again
//   local_down_kernel       level l-1 -> l: the same tile, the I plane and then the W plane through the same LDS
//                           (the launch that makes level L also writes R_L = sum_k GW_L,k GI_L,k into the fourth slot)
//   local_collapse_kernel   level l = L-1 .. 1, one lane per record: R_l into the fourth slot of its own I record.  Level l+1
//                           is only read, level l's first three slots are only read
//   local_apply_kernel      one lane per full-resolution pixel: I and w^ again from the colour, R_0 from four records of
//                           level 1, the f32, u8 and fused stores
// The down weights and the up taps are rtm_bloom_kernel.h's (bl_down_weights, bl_up_taps); its kernels are left out here.
// Every sum has one fixed order, so the same inputs give the same bits on every call.
#ifndef RTM_TONEMAP_LOCAL_KERNEL_H
#define RTM_TONEMAP_LOCAL_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"
#define RTM_BLOOM_FILTERS_ONLY  // the weights, the taps and the constants; bloom's kernels stay in rtm_bloom.o
#include "rtm_bloom_kernel.h"

namespace rtm {

// what the kernels need of rtm_tonemap_local_params, made once on the host
struct LocalToneArgs {
    float anchor;   // A without the statistics' exposure
    float e0, e2;   // exp2(shadows), exp2(-highlights); e_1 = 1
    float neg_inv;  // -1 / (2 sigma^2)
};

// step 2's A: the anchor times the exposure of the (nullable, device) statistics
__device__ inline float lt_anchor(const LocalToneArgs& a, const rtm_tonemap_stats* __restrict__ stats) {
    return a.anchor * (stats ? stats->exposure : 1.0f);
}

// steps 1-2 of a pixel: x, and xc in place; a pixel that does not count is black
__device__ inline float lt_exposed(float& r, float& g, float& b, const float A) {
    if (!bl_counts(r, g, b)) r = g = b = 0.0f;
    r = fmaxf(r, 0.0f);
    g = fmaxf(g, 0.0f);
    b = fmaxf(b, 0.0f);
    return fminf(A * bl_lum(r, g, b), 1e6f);
}

// step 3
__device__ inline void lt_exposures(const float x, const LocalToneArgs& a, float I[3]) {
    const float x0 = a.e0 * x, x2 = a.e2 * x;
    I[0] = x0 / (1.0f + x0);
    I[1] = x / (1.0f + x);
    I[2] = x2 / (1.0f + x2);
}

// step 4, from the three I
__device__ inline void lt_weights(const float I[3], const float neg_inv, float w[3]) {
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float d = sqrtf(I[k]) - 0.5f;
        w[k] = __expf((d * d) * neg_inv);
        sum += w[k];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] *= inv;
}

// rtm_bloom's down filter of the fine tile in `fine` (bl_filter_tile's layout) for this lane's coarse pixel: the horizontal
// pass into `hor`, a barrier, the vertical pass into o.  Every lane of the block calls it; false: the lane has no pixel.
__device__ inline bool lt_filter_tile(const float* fine, const int* lead, float* hor, const int X0, const int Y0, const int Wf,
                                      const int Hf, const int Wc, const int Hc, float o[3]) {
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
    if (X0 + xl >= Wc || Y0 + yl >= Hc) return false;
    float w[4];
    bl_down_weights(Y0 + yl, Hf, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = hor + (c * kBlInY + 2 * yl) * kBlTileX + xl;
        o[c] = (w[0] * p[0] + w[1] * p[kBlTileX]) + (w[2] * p[2 * kBlTileX] + w[3] * p[3 * kBlTileX]);
    }
    return true;
}

// the two records of this lane's coarse pixel; last: the level is L and the fourth slot receives R_L
__device__ inline void lt_store(const bool mine, const int X0, const int Y0, const int Wc, const float gi[3], const float gw[3],
                                const bool last, float4* __restrict__ dst_i, float4* __restrict__ dst_w) {
    if (!mine) return;
    const int X = X0 + (int)threadIdx.x % kBlTileX, Y = Y0 + (int)threadIdx.x / kBlTileX;
    const float R = last ? (gw[0] * gi[0] + gw[1] * gi[1]) + gw[2] * gi[2] : 0.0f;
    const size_t p = (size_t)Y * Wc + X;
    dst_i[p] = make_float4(gi[0], gi[1], gi[2], R);
    dst_w[p] = make_float4(gw[0], gw[1], gw[2], 0.0f);
}

// color -> level 1.  The load is bloom_bright_down_kernel's: fine row r of the tile starts at float
// a = 3 ((2 Y0 - 1 + r) W + 2 X0 - 1) of the frame, its slots are the dwordx4s from a rounded down to a multiple of four, and
// lead = a mod 4 floats precede the first pixel.  VEC: color is 16-byte aligned and a slot inside the frame's floats is one
// dwordx4 load; the plain path reads the same floats as dwords, hence the same bits.  No slot reaches outside the frame's
// memory, and every out-of-frame pixel is overwritten with zero (its filter weight is zero as well).
template <bool VEC>
__global__ __launch_bounds__(kBlBlock) void local_base_down_kernel(const int W, const int H, const int Wc, const int Hc,
                                                                   const int tiles_x, const float* __restrict__ color,
                                                                   const rtm_tonemap_stats* __restrict__ stats,
                                                                   const LocalToneArgs args, const int last,
                                                                   float4* __restrict__ dst_i, float4* __restrict__ dst_w) {
    __shared__ __attribute__((aligned(16))) float fine[kBlInY * kBlRowFloats];
    __shared__ float hor[3 * kBlInY * kBlTileX];
    __shared__ int lead[kBlInY];
    const int X0 = ((int)blockIdx.x % tiles_x) * kBlTileX, Y0 = ((int)blockIdx.x / tiles_x) * kBlTileY;
    const long long total = 3ll * W * H;
    const float A = lt_anchor(args, stats);
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
        float I[3] = {0.0f, 0.0f, 0.0f};
        if (x >= 0 && x < W && y >= 0 && y < H) {
            float cr = p[0], cg = p[1], cb = p[2];
            lt_exposures(lt_exposed(cr, cg, cb, A), args, I);
        }
        p[0] = I[0];
        p[1] = I[1];
        p[2] = I[2];
    }
    __syncthreads();
    float gi[3], gw[3];
    const bool mine = lt_filter_tile(fine, lead, hor, X0, Y0, W, H, Wc, Hc, gi);
    __syncthreads();  // hor and fine are read to the end before they are written again
    for (int it = (int)threadIdx.x; it < kBlInY * kBlInX; it += kBlBlock) {
        const int r = it / kBlInX, i = it % kBlInX;
        float* p = fine + r * kBlRowFloats + lead[r] + 3 * i;
        const float I[3] = {p[0], p[1], p[2]};
        float w[3];
        lt_weights(I, args.neg_inv, w);
        p[0] = w[0];
        p[1] = w[1];
        p[2] = w[2];
    }
    __syncthreads();
    lt_filter_tile(fine, lead, hor, X0, Y0, W, H, Wc, Hc, gw);
    lt_store(mine, X0, Y0, Wc, gi, gw, last != 0, dst_i, dst_w);
}

// the first three slots of the records of level l-1 under the tile into `fine`, out-of-frame pixels zero
__device__ inline void lt_load_records(const float4* __restrict__ src, const int X0, const int Y0, const int Wf, const int Hf,
                                       float* fine) {
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
}

// level l-1 (Wf x Hf records in each plane) -> level l (Wc x Hc)
__global__ __launch_bounds__(kBlBlock) void local_down_kernel(const int Wf, const int Hf, const int Wc, const int Hc,
                                                              const int tiles_x, const float4* __restrict__ src_i,
                                                              const float4* __restrict__ src_w, const int last,
                                                              float4* __restrict__ dst_i, float4* __restrict__ dst_w) {
    __shared__ float fine[kBlInY * kBlRowFloats];
    __shared__ float hor[3 * kBlInY * kBlTileX];
    __shared__ int lead[kBlInY];
    const int X0 = ((int)blockIdx.x % tiles_x) * kBlTileX, Y0 = ((int)blockIdx.x / tiles_x) * kBlTileY;
    if (threadIdx.x < kBlInY) lead[threadIdx.x] = 0;
    lt_load_records(src_i, X0, Y0, Wf, Hf, fine);
    __syncthreads();
    float gi[3], gw[3];
    const bool mine = lt_filter_tile(fine, lead, hor, X0, Y0, Wf, Hf, Wc, Hc, gi);
    __syncthreads();  // hor and fine are read to the end before they are written again
    lt_load_records(src_w, X0, Y0, Wf, Hf, fine);
    __syncthreads();
    lt_filter_tile(fine, lead, hor, X0, Y0, Wf, Hf, Wc, Hc, gw);
    lt_store(mine, X0, Y0, Wc, gi, gw, last != 0, dst_i, dst_w);
}

// up(coarse)(x, y) of all four slots (rtm_bloom's bl_up leaves the fourth out): the horizontal pairs first, then the rows
__device__ inline float4 lt_up(const float4* __restrict__ coarse, const int Wc, const int Hc, const int x, const int y) {
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
    o.w = wy0 * (wx0 * a.w + wx1 * b.w) + wy1 * (wx0 * c.w + wx1 * d.w);
    return o;
}

// step 6 at one pixel: sum_k w_k (I_k - up(GI)_k) + up(R)
__device__ inline float lt_blend(const float I[3], const float w[3], const float4 u) {
    return ((w[0] * (I[0] - u.x) + w[1] * (I[1] - u.y)) + w[2] * (I[2] - u.z)) + u.w;
}

// level l (Wf x Hf): a lane reads its own two records and four I records of level l+1 (Wc x Hc), and writes the fourth slot
// of its own I record.  No lane reads that slot of level l, so the planes need no second copy.
__global__ __launch_bounds__(kBlPixTileX * kBlPixTileY) void local_collapse_kernel(const int Wf, const int Hf, const int Wc,
                                                                                  const int Hc, const int tiles_x,
                                                                                  const float4* __restrict__ coarse_i,
                                                                                  const float4* __restrict__ level_w,
                                                                                  float4* level_i) {
    const int x = ((int)blockIdx.x % tiles_x) * kBlPixTileX + (int)threadIdx.x % kBlPixTileX;
    const int y = ((int)blockIdx.x / tiles_x) * kBlPixTileY + (int)threadIdx.x / kBlPixTileX;
    if (x >= Wf || y >= Hf) return;
    const float4 u = lt_up(coarse_i, Wc, Hc, x, y);
    const size_t p = (size_t)y * Wf + x;
    const float4 gi = level_i[p], gw = level_w[p];
    const float I[3] = {gi.x, gi.y, gi.z}, w[3] = {gw.x, gw.y, gw.z};
    ((float*)(level_i + p))[3] = lt_blend(I, w, u);
}

// color and out32 may be the same buffer: a lane reads its pixel before it writes it and touches no other.  level1_i null:
// levels = 0, the pointwise blend.
__global__ __launch_bounds__(kBlPixTileX * kBlPixTileY) void local_apply_kernel(const int W, const int H, const int Wc,
                                                                               const int Hc, const int tiles_x,
                                                                               const float* color,
                                                                               const rtm_tonemap_stats* __restrict__ stats,
                                                                               const LocalToneArgs args,
                                                                               const float4* __restrict__ level1_i, float* out32,
                                                                               uint8_t* __restrict__ out8,
                                                                               float* __restrict__ fused_out) {
    const int x = ((int)blockIdx.x % tiles_x) * kBlPixTileX + (int)threadIdx.x % kBlPixTileX;
    const int y = ((int)blockIdx.x / tiles_x) * kBlPixTileY + (int)threadIdx.x / kBlPixTileX;
    if (x >= W || y >= H) return;
    const float A = lt_anchor(args, stats);
    const size_t p = ((size_t)y * W + x) * 3;
    float cr = color[p], cg = color[p + 1], cb = color[p + 2];
    const bool counts = bl_counts(cr, cg, cb);
    const float ex = lt_exposed(cr, cg, cb, A);
    float I[3], w[3];
    lt_exposures(ex, args, I);
    lt_weights(I, args.neg_inv, w);
    float R;
    if (level1_i)
        R = lt_blend(I, w, lt_up(level1_i, Wc, Hc, x, y));
    else
        R = (w[0] * I[0] + w[1] * I[1]) + w[2] * I[2];
    const float F = fminf(fmaxf(R, 0.0f), 1.0f);
    if (fused_out) fused_out[(size_t)y * W + x] = F;
    if (!out32 && !out8) return;
    const float gain = counts ? A * (F / fmaxf(ex, 1e-4f)) : 0.0f;
    const float o0 = cr * gain, o1 = cg * gain, o2 = cb * gain;  // a pixel that does not count: +0 * +0
    if (out32) {
        out32[p] = o0;
        out32[p + 1] = o1;
        out32[p + 2] = o2;
    }
    if (out8) {
        out8[p] = bl_quantise(o0);
        out8[p + 1] = bl_quantise(o1);
        out8[p + 2] = bl_quantise(o2);
    }
}

}  // namespace rtm
#endif
