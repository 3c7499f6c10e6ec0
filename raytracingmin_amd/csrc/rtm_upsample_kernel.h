// rtm_upsample_kernel.h — the AOV-guided (joint bilateral) upsampler (include/rtm.h: rtm_upsample).  Included by
// rtm_upsample.hip.
//
// Two kernels, all fp32, one lane per pixel, blocks of 64 x 4 pixels (one wave = 64 pixels of one row):
//   upsample_pack_kernel  the low-resolution prepass: demodulates the low colour and packs each low pixel into two 16-byte
//                         records of the work buffer, (e.x, e.y, e.z, object bits) and (n.x, n.y, n.z, z), the denoiser's
//                         record layout
//   upsample_kernel<F>    one lane per FULL-resolution pixel.  A block's 4 x 4-tap footprints cover at most
//                         (ceil(63 / F) + 4) x (ceil(3 / F) + 4) low pixels (36 x 6 at F = 2): those records are staged in
//                         LDS once per block, one record pair per lane, and the 16 taps are taken from there.  The factor
//                         is a template parameter: the tap rule's floor divisions are by constants.
// LDS layout: two arrays of float4 (16-byte stride), rows back to back.  A wave reads one staged row only, and its lanes'
// records are contiguous there (F neighbouring lanes share one record, a broadcast), so a 16-lane group of a ds_read_b128
// touches at most 16 consecutive 16-byte slots = one 256-byte bank row: conflict-free for every row stride, no padding.
// Frame-edge taps are masked by coordinates, never clamped.  No atomics and a fixed tap order (dy outer, dx inner).
#ifndef RTM_UPSAMPLE_KERNEL_H
#define RTM_UPSAMPLE_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rtm {

constexpr int kUpTileX = 64, kUpTileY = 4;  // 256 lanes per block, 4 waves, each one row segment
constexpr int kUpMaxFactor = 8;

struct UpsampleFrame {
    int w, h;             // the low frame
    int W, H;             // the full frame: F w x F h
    int tiles_x;          // ceil(W / 64) (upsample_kernel) or ceil(w / 64) (upsample_pack_kernel)
    int has_geo;          // a normal or depth plane was given: the second record of each low pixel is read
    int has_depth;        // the +inf miss rules
    int depth_term;       // has_depth && sigma_depth > 0
    int normal_term;      // normal given && sigma_normal > 0
    float sigma_n;        // the normal weight's exponent
    float depth_scale;    // sigma_depth F
    // the spatial weights: tab[4 j + dx + 1] = exp(-(dx - t)^2 / (2 sigma_s^2)), t = r / (2 F), for the F remainders
    // r = 2 j + (F even ? 1 : 0) a pixel can have; computed in double on the host
    float tab[4 * kUpMaxFactor];
};

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t up_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

__device__ inline float up_demod(const float* albedo, size_t i) {
    if (!albedo) return 1.0f;
    const float a = albedo[i];
    return a > 1e-3f ? a : 1.0f;
}

// The tap rule for the full-resolution coordinate c >= 0: num = 2 c + 1 - F, base = floor(num / 2F) (the tap dx = 0),
// j = (num - 2F base) / 2 (the row of the weight table).  num >= 1 - F > -2F, so num + 2F is positive.
template <int F>
__device__ inline int up_base(int c, int& j) {
    const int num = 2 * c + 1 - F;
    const int base = (num + 2 * F) / (2 * F) - 1;
    j = (num - 2 * F * base) >> 1;
    return base;
}

__global__ __launch_bounds__(kUpTileX * kUpTileY) void upsample_pack_kernel(
    const UpsampleFrame U, const float* __restrict__ color, const float* __restrict__ depth, const float* __restrict__ normal,
    const float* __restrict__ albedo, const int32_t* __restrict__ object, float4* __restrict__ rec_e, float4* __restrict__ rec_g) {
    const int tile = (int)blockIdx.x;
    const int x = (tile % U.tiles_x) * kUpTileX + (int)threadIdx.x % kUpTileX;
    const int y = (tile / U.tiles_x) * kUpTileY + (int)threadIdx.x / kUpTileX;
    if (x >= U.w || y >= U.h) return;
    const size_t p = (size_t)y * U.w + x;
    const float ex = color[p * 3] / up_demod(albedo, p * 3);
    const float ey = color[p * 3 + 1] / up_demod(albedo, p * 3 + 1);
    const float ez = color[p * 3 + 2] / up_demod(albedo, p * 3 + 2);
    rec_e[p] = make_float4(ex, ey, ez, __int_as_float(object ? object[p] : 0));  // no object plane: every id is 0
    if (U.has_geo) {
        const float z = depth ? depth[p] : 0.0f;
        rec_g[p] = normal ? make_float4(normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2], z) : make_float4(0.0f, 0.0f, 0.0f, z);
    }
}

// out_p = A_p sum_q w(p, q) e_q / sum_q w(p, q) over the 4 x 4 low taps q around p, w = h_x h_y (g(p, q) + 1e-6f); p's guides
// are the full-resolution planes, q's the packed low records.
template <int F>
__global__ __launch_bounds__(kUpTileX * kUpTileY) void upsample_kernel(
    const UpsampleFrame U, const float4* __restrict__ rec_e, const float4* __restrict__ rec_g, const float* __restrict__ depth,
    const float* __restrict__ normal, const float* __restrict__ albedo, const int32_t* __restrict__ object,
    float* __restrict__ out32, uint8_t* __restrict__ out8) {
    static_assert(F >= 2 && F <= kUpMaxFactor, "factor 2..8");
    // X0 of the block's last column is at most ceil(63 / F) past that of its first; one tap before, two after
    constexpr int SW = (kUpTileX - 1 + F - 1) / F + 4, SH = (kUpTileY - 1 + F - 1) / F + 4, SN = SW * SH;
    static_assert(SN <= kUpTileX * kUpTileY, "one staged record pair per lane");
    __shared__ float4 s_e[SN];  // (e, object bits)
    __shared__ float4 s_g[SN];  // (n, z)
    const int x0 = ((int)blockIdx.x % U.tiles_x) * kUpTileX, y0 = ((int)blockIdx.x / U.tiles_x) * kUpTileY;
    int unused;
    const int bx = up_base<F>(x0, unused) - 1, by = up_base<F>(y0, unused) - 1;  // the low pixel staged at (0, 0)
    if ((int)threadIdx.x < SN) {
        const int sy = (int)threadIdx.x / SW, sx = (int)threadIdx.x - sy * SW;
        const int gx = bx + sx, gy = by + sy;
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = e;
        if (gx >= 0 && gx < U.w && gy >= 0 && gy < U.h) {  // outside the frame: never read back (the taps are masked)
            const size_t q = (size_t)gy * U.w + gx;
            e = rec_e[q];
            if (U.has_geo) g = rec_g[q];
        }
        s_e[threadIdx.x] = e;
        if (U.has_geo) s_g[threadIdx.x] = g;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x % kUpTileX, y = y0 + (int)threadIdx.x / kUpTileX;
    if (x >= U.W || y >= U.H) return;
    int jx, jy;
    const int X0 = up_base<F>(x, jx), Y0 = up_base<F>(y, jy);
    const size_t p = (size_t)y * U.W + x;
    const int obj_p = object ? object[p] : 0;
    const float zp = depth ? depth[p] : 0.0f;
    float npx = 0.0f, npy = 0.0f, npz = 0.0f;
    if (normal) {
        npx = normal[p * 3];
        npy = normal[p * 3 + 1];
        npz = normal[p * 3 + 2];
    }
    const bool p_miss = __builtin_isinf(zp);
    const int c = (Y0 - by) * SW + (X0 - bx);  // the staged tap (dx, dy) = (0, 0)
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 2; ++dy) {
        if (Y0 + dy < 0 || Y0 + dy >= U.h) continue;
        const float hy = U.tab[4 * jy + dy + 1];
#pragma unroll
        for (int dx = -1; dx <= 2; ++dx) {
            if (X0 + dx < 0 || X0 + dx >= U.w) continue;
            const int q = c + dy * SW + dx;
            const float4 eq = s_e[q];
            float g = __float_as_int(eq.w) == obj_p ? 1.0f : 0.0f;
            if (U.has_geo) {
                const float4 gq = s_g[q];
                float wz = 1.0f, wn = 1.0f;
                if (U.depth_term)
                    wz = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(zp - gq.w) / (U.depth_scale * fmaxf(zp, gq.w)));
                if (U.normal_term)
                    wn = __builtin_amdgcn_exp2f(U.sigma_n * __builtin_amdgcn_logf(fmaxf(0.0f, npx * gq.x + npy * gq.y + npz * gq.z)));
                const bool q_miss = __builtin_isinf(gq.w);
                // two misses: 1 and nothing else; one miss: 0 (selects: the NaN of inf - inf never reaches g)
                const float geo = !U.has_depth ? wz * wn : (p_miss && q_miss) ? 1.0f : (p_miss != q_miss) ? 0.0f : wz * wn;
                g = g * geo;
            }
            const float w = (U.tab[4 * jx + dx + 1] * hy) * (g + 1e-6f);
            sx += w * eq.x;
            sy += w * eq.y;
            sz += w * eq.z;
            ws += w;
        }
    }
    const float ox = sx / ws * up_demod(albedo, p * 3), oy = sy / ws * up_demod(albedo, p * 3 + 1),
                oz = sz / ws * up_demod(albedo, p * 3 + 2);
    if (out32) {
        out32[p * 3] = ox;
        out32[p * 3 + 1] = oy;
        out32[p * 3 + 2] = oz;
    }
    if (out8) {
        out8[p * 3] = up_quantise(ox);
        out8[p * 3 + 1] = up_quantise(oy);
        out8[p * 3 + 2] = up_quantise(oz);
    }
}

}  // namespace rtm
#endif
