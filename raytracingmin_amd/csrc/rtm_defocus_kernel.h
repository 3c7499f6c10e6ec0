// rtm_defocus_kernel.h — depth of field (include/rtm.h: rtm_defocus).  Included by rtm_defocus.hip.
//
// One kernel, fp32, no atomics.  A block of 512 lanes owns a 32 x 16 tile of output pixels, one pixel a lane.
//   fill     the tile and its halo of R pixels go into LDS as two planes of records: (c.x, c.y, c.z, z) in 16 bytes and
//            (s, ia) in 8, so that a wave's lanes read consecutive records of one row with one ds_read_b128 and one
//            ds_read_b64, both free of bank conflicts.  s and ia (steps 1-2) are computed here, once per loaded pixel.  A
//            pixel outside the frame or one that does not count is (0, 0, 0, 0) and (0, 0): ia = 0 marks it, its weight is
//            +0 and its zero colour keeps 0 * NaN out of the sums.
//   bound    the block reduces max r over everything it loaded.  No tap can weigh more than +0 at |dx| or |dy| beyond
//            B = min(R, ceil(max r + 0.5)), so the loop runs over -B..B; with max r <= 0.5 every non-centre weight is +0 and
//            the block stores its inputs and leaves.  Adding +0 changes no sum, so both are bit-neutral.  The distances of
//            step 3 go into LDS for that window only (__fsqrt_rn: correctly rounded, what the host's sqrtf gives), and not
//            at all in a block that passes through.
//   taps     rows first, then columns, the centre in its place: one fixed order, the same bits on every call.
// The LDS is sized by a class of R (template parameter RC = 4, 8 or 16: 23, 37 and 76 KiB, rtm_defocus.hip picks the
// smallest that holds max_radius); R itself is a run-time value, and the strides follow it.
#ifndef RTM_DEFOCUS_KERNEL_H
#define RTM_DEFOCUS_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kDfTileX = 32, kDfTileY = 16;        // the tile of output pixels a block owns
constexpr int kDfBlock = kDfTileX * kDfTileY;      // 512 lanes: eight wave64s, a wave covers two rows of the tile
constexpr int kDfMaxRadius = 16;
constexpr int df_records(int rc) { return (kDfTileX + 2 * rc) * (kDfTileY + 2 * rc); }  // tile + halo
constexpr int df_table(int rc) { return (2 * rc + 1) * (2 * rc + 1); }
// static LDS of an instantiation: 24 bytes a record, the distance table, the eight wave maxima
constexpr size_t df_lds_bytes(int rc) { return (size_t)df_records(rc) * 24 + (size_t)df_table(rc) * 4 + 8 * 4; }
static_assert(2 * df_lds_bytes(kDfMaxRadius) <= 160 * 1024, "two blocks of the R = 16 class must fit a CU's LDS");

__device__ inline bool df_counts(float r, float g, float b, float z) {
    return __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b) && z > 0.0f;  // NaN > 0 is false
}

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t df_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

// step 2 of a counting pixel: the signed radius and the reciprocal area of its disc
__device__ inline void df_coc(const float z, const float zf, const float A, const float Rf, float& s, float& ia) {
    // z = +inf: the quotient is +0.  A quotient that overflows counts as the largest float, so that A = 0 gives -0, not NaN
    s = A * fmaxf(1.0f - zf / z, -3.402823466e+38f);
    s = fminf(fmaxf(s, -Rf), Rf);
    const float m = fmaxf(fabsf(s), 0.5f);
    ia = 1.0f / ((3.14159265358979323846f * m) * m);
}

// BOUND: the window bound and the pass-through of sharp tiles (false: every block runs all (2R+1)^2 taps — the form
// profiles/defocus_pass.py times next to the shipped one; the bits are the same)
template <int RC, bool BOUND>
__global__ __launch_bounds__(kDfBlock) void defocus_kernel(const int W, const int H, const int tiles_x, const int R,
                                                           const float zf, const float A,
                                                           const float* __restrict__ color,
                                                           const float* __restrict__ depth, float* __restrict__ out32,
                                                           uint8_t* __restrict__ out8, float* __restrict__ coc_out) {
    __shared__ __attribute__((aligned(16))) float4 rec_c[df_records(RC)];  // (c.x, c.y, c.z, z)
    __shared__ __attribute__((aligned(8))) float2 rec_s[df_records(RC)];   // (s, ia)
    __shared__ float dist[df_table(RC)];
    __shared__ float wave_max[kDfBlock / 64];
    const int X0 = ((int)blockIdx.x % tiles_x) * kDfTileX, Y0 = ((int)blockIdx.x / tiles_x) * kDfTileY;
    const int IW = kDfTileX + 2 * R, IH = kDfTileY + 2 * R, D = 2 * R + 1;  // R <= RC: within the arrays
    const float Rf = (float)R;
    float max_r = 0.0f;
    for (int it = (int)threadIdx.x; it < IW * IH; it += kDfBlock) {
        const int iy = it / IW, ix = it - iy * IW;
        const int x = X0 - R + ix, y = Y0 - R + iy;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float2 s = make_float2(0.0f, 0.0f);
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t p = (size_t)y * W + x;
            const float cr = color[3 * p], cg = color[3 * p + 1], cb = color[3 * p + 2], z = depth[p];
            if (df_counts(cr, cg, cb, z)) {
                c = make_float4(cr, cg, cb, z);
                df_coc(z, zf, A, Rf, s.x, s.y);
                max_r = fmaxf(max_r, fabsf(s.x));
            }
        }
        rec_c[it] = c;
        rec_s[it] = s;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) max_r = fmaxf(max_r, __shfl_xor(max_r, off, 64));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = max_r;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kDfBlock / 64; ++i) max_r = fmaxf(max_r, wave_max[i]);  // the same value in every lane
    const bool sharp_tile = BOUND && max_r <= 0.5f;
    const int B = BOUND ? min(R, (int)ceilf(max_r + 0.5f)) : R;
    if (!sharp_tile) {  // block-uniform: the distances of the window that will be read, (2B+1)^2 of the table's (2R+1)^2
        const int DB = 2 * B + 1;
        for (int it = (int)threadIdx.x; it < DB * DB; it += kDfBlock) {
            const int dy = it / DB - B, dx = it % DB - B;
            dist[(dy + R) * D + dx + R] = __fsqrt_rn((float)(dx * dx + dy * dy));
        }
        __syncthreads();
    }

    const int lx = (int)threadIdx.x % kDfTileX, ly = (int)threadIdx.x / kDfTileX;
    const int x = X0 + lx, y = Y0 + ly;
    if (x >= W || y >= H) return;  // (no barrier follows)
    const int centre = (ly + R) * IW + lx + R;
    const float4 cp = rec_c[centre];
    const float2 sp = rec_s[centre];
    const size_t p = (size_t)y * W + x;
    if (coc_out) coc_out[p] = sp.x;  // +0 for a pixel that does not count
    if (!out32 && !out8) return;
    const uint32_t* words = (const uint32_t*)color;
    uint32_t wr = words[3 * p], wg = words[3 * p + 1], wb = words[3 * p + 2];  // the input, for the cases that keep it
    if (sp.y != 0.0f && !sharp_tile) {
        const float zp = cp.w, rp = fabsf(sp.x), iap = sp.y;
        float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
        bool others = false;  // a tap other than the centre weighs more than +0
        for (int dy = -B; dy <= B; ++dy) {
            const int row = centre + dy * IW;
            const float* drow = dist + (dy + R) * D + R;
            for (int dx = -B; dx <= B; ++dx) {
                const float4 cq = rec_c[row + dx];
                const float2 sq = rec_s[row + dx];
                const float rq = fabsf(sq.x);
                const bool own = cq.w > zp && rp < rq;  // behind p and wider than p: no further than p's own blur
                const float re = own ? rp : rq, iae = own ? iap : sq.y;
                const float w = fminf(fmaxf(re + 0.5f - drow[dx], 0.0f), 1.0f) * iae;
                others |= w > 0.0f && (dx | dy) != 0;
                sw += w;
                sr += w * cq.x;
                sg += w * cq.y;
                sb += w * cq.z;
            }
        }
        if (others) {
            wr = __float_as_uint(sr / sw);
            wg = __float_as_uint(sg / sw);
            wb = __float_as_uint(sb / sw);
        }
    }
    if (out32) {
        uint32_t* o = (uint32_t*)out32;
        o[3 * p] = wr;
        o[3 * p + 1] = wg;
        o[3 * p + 2] = wb;
    }
    if (out8) {
        out8[3 * p] = df_quantise(__uint_as_float(wr));
        out8[3 * p + 1] = df_quantise(__uint_as_float(wg));
        out8[3 * p + 2] = df_quantise(__uint_as_float(wb));
    }
}

}  // namespace rtm
#endif
