// rtm_denoise_var_kernel.h — the variance-guided à-trous denoiser (include/rtm.h: rtm_denoise_variance).  Included by
// rtm_denoise.hip after rtm_denoise_kernel.h, whose prepass, record layout, 64 x 4 block shape, DenoiseFrame flags and K = 0
// copy it reuses (DenoiseFrame::color_term here means sigma_lum > 0).
//
// Two kernels, all fp32, one lane per pixel:
//   denoise_variance_kernel   v0: the geometry-weighted first and second moments of the demodulated luminance over a 7 x 7
//                             window.  The LDS form stages the block's tile plus a 3-pixel halo as (l, object bits) and
//                             (n, z) and takes its 49 taps from there; ROWS pixels per lane make the tile 64 x 4 ROWS.
//                             denoise_variance_direct_kernel is the same arithmetic with every tap loaded from L2.
//   denoise_level_var_kernel  one à-trous level whose colour weight is relative to the pixel's own standard deviation
//                             (sqrt of the 3 x 3 prefiltered variance), and which carries the variance through the level
// Frame-edge and halo taps are masked, never clamped.  No atomics and a fixed tap order (dy outer, dx inner).
#ifndef RTM_DENOISE_VAR_KERNEL_H
#define RTM_DENOISE_VAR_KERNEL_H
#include "rtm_denoise_kernel.h"

namespace rtm {

constexpr int kDvHalo = 3;                          // the 7 x 7 window's reach
constexpr int kDvStageW = kDnTileX + 2 * kDvHalo;   // 70 staged pixels per row

__device__ inline float dn_lum(const float4& e) { return 0.2126f * e.x + 0.7152f * e.y + 0.0722f * e.z; }

// g_s(p, q) of rtm_denoise for q != p: the object test, the +inf miss rules, w_z with depth_scale = sigma_depth s, w_n.
// gp / gq are read only where F.has_geo.
__device__ inline float dn_geometry(const DenoiseFrame& F, const float depth_scale, const float obj_p, const float obj_q,
                                    const float4& gp, const float4& gq, const bool p_miss) {
    float g = __float_as_int(obj_q) == __float_as_int(obj_p) ? 1.0f : 0.0f;
    if (F.has_geo) {
        float wz = 1.0f, wn = 1.0f;
        if (F.depth_term)
            wz = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(gp.w - gq.w) / (depth_scale * fmaxf(gp.w, gq.w)));
        if (F.normal_term)
            wn = __builtin_amdgcn_exp2f(F.sigma_n * __builtin_amdgcn_logf(fmaxf(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z)));
        const bool q_miss = __builtin_isinf(gq.w);
        // two misses: 1 and nothing else; one miss: 0 (selects: the NaN of inf - inf never reaches g)
        const float geo = !F.has_depth ? wz * wn : (p_miss && q_miss) ? 1.0f : (p_miss != q_miss) ? 0.0f : wz * wn;
        g = g * geo;
    }
    return g;
}

// v0 = max(0, m2 - m1^2) of the differences d = l_q - l_p (the shift by l_p keeps the subtraction from cancelling)
__device__ inline float dv_finish(const float U, const float s1, const float s2) {
    const float m1 = s1 / U, m2 = s2 / U;
    return fmaxf(0.0f, m2 - m1 * m1);
}

// The LDS form.  Block of 256 lanes, tile 64 x (4 ROWS) pixels: lane (lx, ly) owns the pixels (x0 + lx, y0 + ly + 4 r).
// depth_scale = sigma_depth (the step is 1).  v_out (the level kernels' first variance plane) and var_out (the caller's)
// may each be null.
template <int ROWS>
__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_variance_kernel(
    const DenoiseFrame F, const int tiles_x, const float depth_scale, const float4* __restrict__ rec_e,
    const float4* __restrict__ rec_g, float* __restrict__ v_out, float* __restrict__ var_out) {
    constexpr int TH = kDnTileY * ROWS, SH = TH + 2 * kDvHalo, SN = SH * kDvStageW;
    __shared__ float2 s_l[SN];  // (l, object bits)
    __shared__ float4 s_g[SN];  // (n, z)
    const int x0 = ((int)blockIdx.x % tiles_x) * kDnTileX, y0 = ((int)blockIdx.x / tiles_x) * TH;
    for (int i = (int)threadIdx.x; i < SN; i += kDnTileX * kDnTileY) {
        const int sy = i / kDvStageW, sx = i - sy * kDvStageW;
        const int gx = x0 - kDvHalo + sx, gy = y0 - kDvHalo + sy;
        float2 l = make_float2(0.0f, 0.0f);
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < F.W && gy >= 0 && gy < F.H) {  // outside the frame: never read back (the taps are masked)
            const size_t q = (size_t)gy * F.W + gx;
            const float4 e = rec_e[q];
            l = make_float2(dn_lum(e), e.w);
            if (F.has_geo) g = rec_g[q];
        }
        s_l[i] = l;
        if (F.has_geo) s_g[i] = g;
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % kDnTileX, ly = (int)threadIdx.x / kDnTileX;
    const int x = x0 + lx;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int ty = ly + kDnTileY * r, y = y0 + ty;
        if (x >= F.W || y >= F.H) continue;
        const int c = (ty + kDvHalo) * kDvStageW + lx + kDvHalo;
        const float2 lp = s_l[c];
        const float4 gp = F.has_geo ? s_g[c] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const bool p_miss = __builtin_isinf(gp.w);
        float U = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int dy = -kDvHalo; dy <= kDvHalo; ++dy) {
            if (y + dy < 0 || y + dy >= F.H) continue;
#pragma unroll
            for (int dx = -kDvHalo; dx <= kDvHalo; ++dx) {
                if (x + dx < 0 || x + dx >= F.W) continue;
                if (dx == 0 && dy == 0) {  // u = 1, d = 0
                    U += 1.0f;
                    continue;
                }
                const int q = c + dy * kDvStageW + dx;
                const float2 lq = s_l[q];
                const float u = dn_geometry(F, depth_scale, lp.y, lq.y, gp, F.has_geo ? s_g[q] : gp, p_miss);
                const float d = lq.x - lp.x;
                U += u;
                s1 += u * d;
                s2 += u * d * d;
            }
        }
        const float v = dv_finish(U, s1, s2);
        const size_t p = (size_t)y * F.W + x;
        if (v_out) v_out[p] = v;
        if (var_out) var_out[p] = v;
    }
}

// The direct form: every tap's records come from L2, as in denoise_level_kernel.
__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_variance_direct_kernel(
    const DenoiseFrame F, const float depth_scale, const float4* __restrict__ rec_e, const float4* __restrict__ rec_g,
    float* __restrict__ v_out, float* __restrict__ var_out) {
    int x, y;
    if (!dn_pixel(F, x, y)) return;
    const size_t p = (size_t)y * F.W + x;
    const float4 ep = rec_e[p];
    const float lp = dn_lum(ep);
    const float4 gp = F.has_geo ? rec_g[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool p_miss = __builtin_isinf(gp.w);
    float U = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int dy = -kDvHalo; dy <= kDvHalo; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= F.H) continue;
#pragma unroll
        for (int dx = -kDvHalo; dx <= kDvHalo; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= F.W) continue;
            if (dx == 0 && dy == 0) {
                U += 1.0f;
                continue;
            }
            const size_t q = (size_t)qy * F.W + qx;
            const float4 eq = rec_e[q];
            const float u = dn_geometry(F, depth_scale, ep.w, eq.w, gp, F.has_geo ? rec_g[q] : gp, p_miss);
            const float d = dn_lum(eq) - lp;
            U += u;
            s1 += u * d;
            s2 += u * d * d;
        }
    }
    const float v = dv_finish(U, s1, s2);
    if (v_out) v_out[p] = v;
    if (var_out) var_out[p] = v;
}

// Level i with variance: w(p, q) = h h g_s(p, q) w_l(p, q), w_l = exp(-|l_p - l_q| / (sigma_lum sqrt(v~_p) + 1e-4)) with v~_p
// the 3 x 3 {1/4, 1/2, 1/4} prefilter of v_in around p (in-frame taps, normalised; only v~_p enters, never v~_q);
// e_out = sum w e / sum w and v_out = sum w^2 v_in / (sum w)^2.  depth_scale = sigma_depth s.  LAST: out = e_out a instead
// of the record and variance stores.
template <bool LAST>
__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_level_var_kernel(
    const DenoiseFrame F, const int s, const float sigma_lum, const float depth_scale, const float4* __restrict__ rec_in,
    const float4* __restrict__ rec_g, const float* __restrict__ v_in, float4* __restrict__ rec_out, float* __restrict__ v_out,
    const float* __restrict__ albedo, float* __restrict__ out32, uint8_t* __restrict__ out8) {
    constexpr float kH[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    constexpr float kK[3] = {1.0f / 4, 1.0f / 2, 1.0f / 4};
    int x, y;
    if (!dn_pixel(F, x, y)) return;
    const size_t p = (size_t)y * F.W + x;
    const float4 ep = rec_in[p];
    const float4 gp = F.has_geo ? rec_g[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool p_miss = __builtin_isinf(gp.w);
    const float lp = dn_lum(ep);
    float lum_scale = 0.0f;  // -log2(e) / (sigma_lum sqrt(v~_p) + 1e-4)
    if (F.color_term) {
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= F.H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= F.W) continue;
                const float k = kK[dy + 1] * kK[dx + 1];
                num += k * v_in[(size_t)qy * F.W + qx];
                den += k;
            }
        }
        lum_scale = -1.4426950408889634f / (sigma_lum * __builtin_amdgcn_sqrtf(num / den) + 1e-4f);
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, ws = 0.0f, vs = 0.0f;
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
            if (dx != 0 || dy != 0) {  // q == p: g = 1 and w_l = 1
                float g = dn_geometry(F, depth_scale, ep.w, eq.w, gp, F.has_geo ? rec_g[q] : gp, p_miss);
                if (F.color_term) g = g * __builtin_amdgcn_exp2f(fabsf(lp - dn_lum(eq)) * lum_scale);
                w = w * g;
            }
            sx += w * eq.x;
            sy += w * eq.y;
            sz += w * eq.z;
            ws += w;
            if constexpr (!LAST) vs += w * w * v_in[q];
        }
    }
    const float ex = sx / ws, ey = sy / ws, ez = sz / ws;
    if constexpr (!LAST) {
        rec_out[p] = make_float4(ex, ey, ez, ep.w);
        v_out[p] = vs / (ws * ws);
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

}  // namespace rtm
#endif
