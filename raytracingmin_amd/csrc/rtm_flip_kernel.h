// rtm_flip_kernel.h — the perceptual frame difference (include/rtm.h: rtm_flip).  Included by rtm_flip.hip.
//
// Three kernels, all arithmetic in double, every filter separable with replicate padding:
//   flip_rows_kernel   blocks of 256 lanes; a block owns 256 pixels of one row.  It takes the strip and its halo of
//                      R = max(r, rf) pixels on each side (coordinates clamped to the row: replicate padding) through steps
//                      1-3 once, into LDS, and runs the HORIZONTAL pass of the seven filters of each frame out of LDS: Y, Cx,
//                      the two Gaussians of Cz, and g, d, p on y = (Y + 16) / 116.  The fourteen planes go to the work buffer.
//   flip_cols_kernel   a block owns a 64 x 16 tile of pixels, four per lane.  Per pixel the VERTICAL pass over the planes (row
//                      clamped to the frame), then steps 5-7, the map, and the lane's share of the pooled record; the block
//                      folds its lanes to one 32-byte partial and adds its LDS histogram to the call's 256 bins.
//   flip_final_kernel  one block: folds the partials in ascending order and writes rtm_flip_result.
// The planes go through memory rather than LDS: a tile with the 18-pixel halo of the largest tables is 68 x 68 doubles per
// plane, and fourteen of those are 3.2 times the LDS of a CU; the horizontal pass alone needs one row and fits in 14 KiB.
// The only atomics are integer additions (the histogram, in LDS and then to the work buffer): which lane takes which pixel and
// every floating-point reduction tree depend on the frame size alone, so the same inputs give the same bits on every call.
#ifndef RTM_FLIP_KERNEL_H
#define RTM_FLIP_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kFlipBlock = 256;                   // lanes of a block: four wave64s
constexpr int kFlipMaxR = 18;                     // r at pixels_per_degree 128
constexpr int kFlipMaxRf = 16;                    // rf at pixels_per_degree 128
constexpr int kFlipStrip = kFlipBlock;            // pixels of a row a block of the horizontal pass owns
constexpr int kFlipStaged = kFlipStrip + 2 * kFlipMaxR;
constexpr int kFlipPlanes = 7;                    // per frame: Y, Cx, Cz1, Cz2, g y, d y, p y after the horizontal pass
constexpr int kFlipTileW = 64, kFlipTileH = 16;   // the vertical pass's tile: a wave per row, four rows per lane
constexpr int kFlipBins = 256;
enum { kFlipY = 0, kFlipCx = 1, kFlipCz1 = 2, kFlipCz2 = 3, kFlipG = 4, kFlipD = 5, kFlipP = 6 };

struct FlipPartial {  // 32 bytes: one per tile
    double sum;    // sum of the map over the tile's counting pixels
    double min;    // +inf without a counting pixel
    double max;    // -1 without a counting pixel
    uint32_t arg;  // the lowest row-major pixel index that attains max
    uint32_t n;
};

struct FlipTotal {  // the final kernel's accumulator: the partial with a 64-bit count
    double sum, min, max;
    uint64_t n;
    uint32_t arg;
};

struct FlipArgs {  // by value: uniform, read through the scalar cache
    double csf_y[2 * kFlipMaxR + 1], csf_cx[2 * kFlipMaxR + 1], csf_cz1[2 * kFlipMaxR + 1], csf_cz2[2 * kFlipMaxR + 1];
    double feat_g[2 * kFlipMaxRf + 1], feat_d[2 * kFlipMaxRf + 1], feat_p[2 * kFlipMaxRf + 1];  // entry k + r (k + rf)
    double m[3][3], m_inv[3][3], white[3];
    double cmax;
    int32_t width, height, r, rf, srgb, tiles_x;
};

__device__ inline double flip_clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// X / Xn, Y / Yn, Z / Zn of a linear colour
__device__ inline void flip_xyz_over_white(const FlipArgs& k, const double rgb[3], double out[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = ((k.m[i][0] * rgb[0] + k.m[i][1] * rgb[1]) + k.m[i][2] * rgb[2]) / k.white[i];
}

// steps 1-3 of one frame's pixel: three components as stored -> (Y, Cx, Cz); `counts`: the pixel's six components are finite
__device__ inline void flip_to_ycxcz(const FlipArgs& k, const float* __restrict__ px, bool counts, double out[3]) {
    double rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = flip_clamp01(counts ? (double)px[c] : 0.0);
        rgb[c] = k.srgb ? (v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4)) : v;
    }
    double w[3];
    flip_xyz_over_white(k, rgb, w);
    out[0] = 116.0 * w[1] - 16.0;
    out[1] = 500.0 * (w[0] - w[1]);
    out[2] = 200.0 * (w[1] - w[2]);
}

__device__ inline double flip_lab_f(double t) {
    return t > (6.0 / 29.0) * (6.0 / 29.0) * (6.0 / 29.0) ? cbrt(t) : t / (3.0 * ((6.0 / 29.0) * (6.0 / 29.0))) + 4.0 / 29.0;
}

// step 5 up to the Hunt adjustment: filtered (Y, Cx, Cz) -> (L, 0.01 L a, 0.01 L b)
__device__ inline void flip_hunt_lab(const FlipArgs& k, double Y, double Cx, double Cz, double out[3]) {
    const double y = (Y + 16.0) / 116.0;
    const double xyz[3] = {(Cx / 500.0 + y) * k.white[0], y * k.white[1], (y - Cz / 200.0) * k.white[2]};
    double rgb[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        rgb[i] = flip_clamp01((k.m_inv[i][0] * xyz[0] + k.m_inv[i][1] * xyz[1]) + k.m_inv[i][2] * xyz[2]);
    flip_xyz_over_white(k, rgb, w);
    const double fx = flip_lab_f(w[0]), fy = flip_lab_f(w[1]), fz = flip_lab_f(w[2]);
    const double L = 116.0 * fy - 16.0;
    out[0] = L;
    out[1] = 0.01 * L * (500.0 * (fx - fy));
    out[2] = 0.01 * L * (200.0 * (fy - fz));
}

__device__ inline bool flip_finite6(const float* __restrict__ a, const float* __restrict__ b) {
    return __builtin_isfinite(a[0]) && __builtin_isfinite(a[1]) && __builtin_isfinite(a[2]) && __builtin_isfinite(b[0]) &&
           __builtin_isfinite(b[1]) && __builtin_isfinite(b[2]);
}

// planes: 2 x kFlipPlanes planes of height x width doubles, frame a's seven first.  hist: the call's 256 bins, zeroed here
// (nullable: a map-only call pools nothing).
__global__ __launch_bounds__(kFlipBlock) void flip_rows_kernel(const FlipArgs k, const float* __restrict__ fa,
                                                               const float* __restrict__ fb, double* __restrict__ planes,
                                                               uint32_t* __restrict__ hist) {
    __shared__ double ycc[2][3][kFlipStaged];
    const int W = k.width;
    const int t = (int)threadIdx.x;
    const int strips = (W + kFlipStrip - 1) / kFlipStrip;
    const int y = (int)(blockIdx.x / (unsigned)strips);
    const int x0 = (int)(blockIdx.x % (unsigned)strips) * kFlipStrip;
    const int R = k.r > k.rf ? k.r : k.rf;
    const size_t pix = (size_t)W * (size_t)k.height;
    const size_t row0 = (size_t)y * (size_t)W;
    if (hist != nullptr && blockIdx.x == 0) hist[t] = 0u;

    for (int i = t; i < kFlipStrip + 2 * R; i += kFlipBlock) {
        int x = x0 - R + i;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);  // replicate padding: the tap's coordinate clamped to the row
        const float* pa = fa + (row0 + (size_t)x) * 3;
        const float* pb = fb + (row0 + (size_t)x) * 3;
        const bool counts = flip_finite6(pa, pb);
        double va[3], vb[3];
        flip_to_ycxcz(k, pa, counts, va);
        flip_to_ycxcz(k, pb, counts, vb);
#pragma unroll
        for (int c = 0; c < 3; ++c) ycc[0][c][i] = va[c], ycc[1][c][i] = vb[c];
    }
    __syncthreads();
    const int x = x0 + t;
    if (x >= W) return;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const double* sY = &ycc[f][0][t + R];
        const double* sCx = &ycc[f][1][t + R];
        const double* sCz = &ycc[f][2][t + R];
        double hy = 0.0, hcx = 0.0, hcz1 = 0.0, hcz2 = 0.0;
        for (int d = -k.r; d <= k.r; ++d) {
            hy += k.csf_y[d + k.r] * sY[d];
            hcx += k.csf_cx[d + k.r] * sCx[d];
            hcz1 += k.csf_cz1[d + k.r] * sCz[d];
            hcz2 += k.csf_cz2[d + k.r] * sCz[d];
        }
        double hg = 0.0, hd = 0.0, hp = 0.0;
        for (int d = -k.rf; d <= k.rf; ++d) {
            const double v = (sY[d] + 16.0) / 116.0;
            hg += k.feat_g[d + k.rf] * v;
            hd += k.feat_d[d + k.rf] * v;
            hp += k.feat_p[d + k.rf] * v;
        }
        double* out = planes + (size_t)(f * kFlipPlanes) * pix + row0 + (size_t)x;
        out[kFlipY * pix] = hy;
        out[kFlipCx * pix] = hcx;
        out[kFlipCz1 * pix] = hcz1;
        out[kFlipCz2 * pix] = hcz2;
        out[kFlipG * pix] = hg;
        out[kFlipD * pix] = hd;
        out[kFlipP * pix] = hp;
    }
}

// the better of two (max, arg) pairs: the larger value, the lower index on a tie
__device__ inline bool flip_better(double d, uint32_t p, double best_d, uint32_t best_p) {
    return d > best_d || (d == best_d && p < best_p);
}

__device__ inline FlipPartial flip_fold(const FlipPartial& a, const FlipPartial& b) {
    FlipPartial o;
    o.sum = a.sum + b.sum;
    o.min = fmin(a.min, b.min);
    const bool take_b = flip_better(b.max, b.arg, a.max, a.arg);
    o.max = take_b ? b.max : a.max;
    o.arg = take_b ? b.arg : a.arg;
    o.n = a.n + b.n;
    return o;
}

// POOL: the record is wanted (partials and hist are non-null).  MAP: map_out is non-null.
template <bool POOL, bool MAP>
__global__ __launch_bounds__(kFlipBlock) void flip_cols_kernel(const FlipArgs k, const float* __restrict__ fa,
                                                               const float* __restrict__ fb, const double* __restrict__ planes,
                                                               FlipPartial* __restrict__ partials, uint32_t* __restrict__ hist,
                                                               float* __restrict__ map_out) {
    __shared__ uint32_t bins[POOL ? kFlipBins : 1];
    __shared__ FlipPartial fold_lds[kFlipBlock / 64];
    const int W = k.width, H = k.height;
    const int t = (int)threadIdx.x;
    const int tile = (int)blockIdx.x;
    const int x = (tile % k.tiles_x) * kFlipTileW + t % kFlipTileW;
    const int ty0 = (tile / k.tiles_x) * kFlipTileH;
    const size_t pix = (size_t)W * (size_t)H;
    if constexpr (POOL) {
        bins[t] = 0u;
        __syncthreads();
    }
    FlipPartial acc{0.0, __builtin_inf(), -1.0, 0xFFFFFFFFu, 0u};
    for (int j = 0; j < kFlipTileH / (kFlipBlock / kFlipTileW); ++j) {
        const int y = ty0 + t / kFlipTileW + j * (kFlipBlock / kFlipTileW);
        if (x >= W || y >= H) continue;
        const size_t p = (size_t)y * (size_t)W + (size_t)x;
        if (!flip_finite6(fa + p * 3, fb + p * 3)) {
            if constexpr (MAP) map_out[p] = __builtin_nanf("");
            continue;
        }
        double lab[2][3], edge[2], point[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const double* col = planes + (size_t)(f * kFlipPlanes) * pix + (size_t)x;
            double Y = 0.0, Cx = 0.0, cz1 = 0.0, cz2 = 0.0;
            for (int d = -k.r; d <= k.r; ++d) {
                int yy = y + d;
                yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);  // replicate padding
                const double* q = col + (size_t)yy * (size_t)W;
                Y += k.csf_y[d + k.r] * q[kFlipY * pix];
                Cx += k.csf_cx[d + k.r] * q[kFlipCx * pix];
                cz1 += k.csf_cz1[d + k.r] * q[kFlipCz1 * pix];
                cz2 += k.csf_cz2[d + k.r] * q[kFlipCz2 * pix];
            }
            double ex = 0.0, ey = 0.0, px = 0.0, py = 0.0;
            for (int d = -k.rf; d <= k.rf; ++d) {
                int yy = y + d;
                yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
                const double* q = col + (size_t)yy * (size_t)W;
                const double g = k.feat_g[d + k.rf];
                const double hg = q[kFlipG * pix];
                ex += g * q[kFlipD * pix];
                ey += k.feat_d[d + k.rf] * hg;
                px += g * q[kFlipP * pix];
                py += k.feat_p[d + k.rf] * hg;
            }
            flip_hunt_lab(k, Y, Cx, cz1 + cz2, lab[f]);
            edge[f] = sqrt(ex * ex + ey * ey);
            point[f] = sqrt(px * px + py * py);
        }
        const double da = lab[0][1] - lab[1][1], db = lab[0][2] - lab[1][2];
        const double c = pow(fabs(lab[0][0] - lab[1][0]) + sqrt(da * da + db * db), 0.7);
        const double lim = 0.4 * k.cmax;
        const double dEc = c < lim ? (0.95 / lim) * c : 0.95 + (c - lim) / (k.cmax - lim) * 0.05;
        const double dEf = sqrt(fmax(fabs(edge[1] - edge[0]), fabs(point[1] - point[0])) / 1.4142135623730951);
        const double dE = dEc == 0.0 ? 0.0 : pow(dEc, 1.0 - dEf);
        const float m = (float)dE;
        if constexpr (MAP) map_out[p] = m;
        if constexpr (POOL) {
            const int bin = (int)(m * 256.0f);
            atomicAdd(&bins[bin > kFlipBins - 1 ? kFlipBins - 1 : (bin < 0 ? 0 : bin)], 1u);
            acc.sum += dE;
            acc.min = fmin(acc.min, dE);
            if (flip_better(dE, (uint32_t)p, acc.max, acc.arg)) acc.max = dE, acc.arg = (uint32_t)p;
            acc.n += 1u;
        }
    }
    if constexpr (POOL) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {  // butterfly over the wave: every lane ends with the same bits
            FlipPartial o;
            o.sum = __shfl_xor(acc.sum, m, 64);
            o.min = __shfl_xor(acc.min, m, 64);
            o.max = __shfl_xor(acc.max, m, 64);
            o.arg = __shfl_xor(acc.arg, m, 64);
            o.n = __shfl_xor(acc.n, m, 64);
            acc = flip_fold(acc, o);
        }
        if ((t & 63) == 0) fold_lds[t >> 6] = acc;
        __syncthreads();  // also: every lane's histogram additions are in
        if (bins[t] != 0u) atomicAdd(&hist[t], bins[t]);
        if (t == 0) {
            acc = fold_lds[0];
#pragma unroll
            for (int w = 1; w < kFlipBlock / 64; ++w) acc = flip_fold(acc, fold_lds[w]);
            partials[tile] = acc;
        }
    }
}

__device__ inline FlipTotal flip_fold_total(const FlipTotal& a, const FlipTotal& b) {
    FlipTotal o;
    o.sum = a.sum + b.sum;
    o.min = fmin(a.min, b.min);
    const bool take_b = flip_better(b.max, b.arg, a.max, a.arg);
    o.max = take_b ? b.max : a.max;
    o.arg = take_b ? b.arg : a.arg;
    o.n = a.n + b.n;
    return o;
}

// One block.  Lane t folds the partials t, t + 256, .. in ascending order; then the wave butterflies and the four wave results
// in wave order.  Lane t also copies bin t of the call's histogram.
__global__ __launch_bounds__(kFlipBlock) void flip_final_kernel(const FlipArgs k, const FlipPartial* __restrict__ partials,
                                                                const uint32_t n_partials, const uint32_t* __restrict__ hist,
                                                                rtm_flip_result* __restrict__ result_out) {
    __shared__ FlipTotal lds[kFlipBlock / 64];
    FlipTotal a{0.0, __builtin_inf(), -1.0, 0u, 0xFFFFFFFFu};
    for (uint32_t i = threadIdx.x; i < n_partials; i += kFlipBlock) {
        const FlipPartial p = partials[i];
        a = flip_fold_total(a, FlipTotal{p.sum, p.min, p.max, p.n, p.arg});
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        FlipTotal o;
        o.sum = __shfl_xor(a.sum, m, 64);
        o.min = __shfl_xor(a.min, m, 64);
        o.max = __shfl_xor(a.max, m, 64);
        o.n = __shfl_xor((unsigned long long)a.n, m, 64);
        o.arg = __shfl_xor(a.arg, m, 64);
        a = flip_fold_total(a, o);
    }
    result_out->hist[threadIdx.x] = hist[threadIdx.x];
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    a = lds[0];
#pragma unroll
    for (int w = 1; w < kFlipBlock / 64; ++w) a = flip_fold_total(a, lds[w]);
    const uint64_t frame = (uint64_t)k.width * (uint64_t)k.height;
    result_out->mean = a.n ? a.sum / (double)a.n : 0.0;
    result_out->max = a.n ? a.max : 0.0;
    result_out->min = a.n ? a.min : 0.0;
    result_out->pixels = a.n;
    result_out->nonfinite = frame - a.n;
    result_out->argmax_x = a.n ? (int32_t)(a.arg % (uint32_t)k.width) : -1;
    result_out->argmax_y = a.n ? (int32_t)(a.arg / (uint32_t)k.width) : -1;
}

}  // namespace rtm
#endif
