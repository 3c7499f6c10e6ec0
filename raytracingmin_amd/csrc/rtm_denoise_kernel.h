// rtm_denoise_kernel.h — the edge-avoiding à-trous denoiser (include/rtm.h: rtm_denoise).  Included by rtm_denoise.hip.
//
// Three kernels, all fp32, one lane per pixel, blocks of 64 x 4 pixels (one wave = 64 pixels of one row, so every
// record load of a tap is one coalesced 1 KiB row segment):
//   denoise_prepass_kernel  demodulates the colour and packs each pixel into two 16-byte records of the work buffer,
//                           (e.x, e.y, e.z, object bits) and (n.x, n.y, n.z, z): a tap is one or two dwordx4 loads
//   denoise_level_kernel    one à-trous level (step s = 2^i, 5 x 5 taps); ping-pongs the colour records, and the last
//                           level remodulates and stores out_f32 / out_u8 instead
//   denoise_copy_kernel     K = 0: out_f32 = color bit for bit, out_u8 its quantisation
// No atomics and a fixed tap order (dy outer, dx inner): the same inputs give the same bits on every call.
#ifndef RTM_DENOISE_KERNEL_H
#define RTM_DENOISE_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rtm {

constexpr int kDnTileX = 64, kDnTileY = 4;  // 256 lanes per block, 4 waves, each one row segment

struct DenoiseFrame {
    int W, H;
    int tiles_x;          // ceil(W / 64)
    int has_geo;          // a normal or depth plane was given: the second record of each pixel is read
    int has_depth;        // the +inf miss rules
    int depth_term;       // has_depth && sigma_depth > 0
    int normal_term;      // normal given && sigma_normal > 0
    int color_term;       // sigma_color > 0
    float sigma_n;        // the normal weight's exponent
};

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t dn_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

__device__ inline float dn_demod(const float* albedo, size_t i) {
    if (!albedo) return 1.0f;
    const float a = albedo[i];
    return a > 1e-3f ? a : 1.0f;
}

__device__ inline bool dn_pixel(const DenoiseFrame& F, int& x, int& y) {
    const int tile = (int)blockIdx.x;
    x = (tile % F.tiles_x) * kDnTileX + (int)threadIdx.x % kDnTileX;
    y = (tile / F.tiles_x) * kDnTileY + (int)threadIdx.x / kDnTileX;
    return x < F.W && y < F.H;
}

__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_prepass_kernel(
    const DenoiseFrame F, const float* __restrict__ color, const float* __restrict__ depth, const float* __restrict__ normal,
    const float* __restrict__ albedo, const int32_t* __restrict__ object, float4* __restrict__ rec_e, float4* __restrict__ rec_g) {
    int x, y;
    if (!dn_pixel(F, x, y)) return;
    const size_t p = (size_t)y * F.W + x;
    const float ex = color[p * 3] / dn_demod(albedo, p * 3);
    const float ey = color[p * 3 + 1] / dn_demod(albedo, p * 3 + 1);
    const float ez = color[p * 3 + 2] / dn_demod(albedo, p * 3 + 2);
    rec_e[p] = make_float4(ex, ey, ez, __int_as_float(object ? object[p] : 0));  // no object plane: every id is 0
    if (F.has_geo) {
        const float z = depth ? depth[p] : 0.0f;
        rec_g[p] = normal ? make_float4(normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2], z) : make_float4(0.0f, 0.0f, 0.0f, z);
    }
}

// Level i: e_out(p) = sum_q w(p, q) e_in(q) / sum_q w(p, q) over q = p + s (dx, dy), dx, dy in -2..2, taps outside the
// frame skipped.  color_scale = 4^i / sigma_c^2 * log2(e), depth_scale = sigma_z * s.  LAST: out = e_out * a instead of
// the record store.  (The geometry weight below has a twin, dn_geometry of rtm_denoise_var_kernel.h, kept apart so that this
// kernel's code does not move: a change to one belongs in the other.)
template <bool LAST>
__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_level_kernel(
    const DenoiseFrame F, const int s, const float color_scale, const float depth_scale, const float4* __restrict__ rec_in,
    const float4* __restrict__ rec_g, float4* __restrict__ rec_out, const float* __restrict__ albedo, float* __restrict__ out32,
    uint8_t* __restrict__ out8) {
    constexpr float kH[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    int x, y;
    if (!dn_pixel(F, x, y)) return;
    const size_t p = (size_t)y * F.W + x;
    const float4 ep = rec_in[p];
    const float4 gp = F.has_geo ? rec_g[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool p_miss = __builtin_isinf(gp.w);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= F.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= F.W) continue;
            const size_t q = (size_t)qy * F.W + qx;
            const float4 eq = rec_in[q];
            float w = kH[dy + 2] * kH[dx + 2];
            if (dx != 0 || dy != 0) {  // q == p: g = 1 and w_c = 1
                float g = __float_as_int(eq.w) == __float_as_int(ep.w) ? 1.0f : 0.0f;
                if (F.has_geo) {
                    const float4 gq = rec_g[q];
                    float wz = 1.0f, wn = 1.0f;
                    if (F.depth_term)
                        wz = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(gp.w - gq.w) /
                                                    (depth_scale * fmaxf(gp.w, gq.w)));
                    if (F.normal_term)
                        wn = __builtin_amdgcn_exp2f(F.sigma_n *
                                                    __builtin_amdgcn_logf(fmaxf(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z)));
                    const bool q_miss = __builtin_isinf(gq.w);
                    // two misses: 1 and nothing else; one miss: 0 (selects: the NaN of inf - inf never reaches w)
                    const float geo = !F.has_depth ? wz * wn : (p_miss && q_miss) ? 1.0f : (p_miss != q_miss) ? 0.0f : wz * wn;
                    g = g * geo;
                }
                if (F.color_term) {
                    const float cx = ep.x - eq.x, cy = ep.y - eq.y, cz = ep.z - eq.z;
                    g = g * __builtin_amdgcn_exp2f(-(cx * cx + cy * cy + cz * cz) * color_scale);
                }
                w = w * g;
            }
            sx += w * eq.x;
            sy += w * eq.y;
            sz += w * eq.z;
            ws += w;
        }
    }
    const float ex = sx / ws, ey = sy / ws, ez = sz / ws;
    if constexpr (!LAST) {
        rec_out[p] = make_float4(ex, ey, ez, ep.w);
    } else {
        const float ox = ex * dn_demod(albedo, p * 3), oy = ey * dn_demod(albedo, p * 3 + 1), oz = ez * dn_demod(albedo, p * 3 + 2);
        if (out32) {
            out32[p * 3] = ox;
            out32[p * 3 + 1] = oy;
            out32[p * 3 + 2] = oz;
        }
        if (out8) {
            out8[p * 3] = dn_quantise(ox);
            out8[p * 3 + 1] = dn_quantise(oy);
            out8[p * 3 + 2] = dn_quantise(oz);
        }
    }
}

// K = 0: the colour itself, bit for bit, and its quantisation
__global__ __launch_bounds__(256) void denoise_copy_kernel(const float* __restrict__ color, size_t n, float* __restrict__ out32,
                                                           uint8_t* __restrict__ out8) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float v = color[i];
        if (out32) out32[i] = v;
        if (out8) out8[i] = dn_quantise(v);
    }
}

}  // namespace rtm
#endif
