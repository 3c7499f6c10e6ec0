// rtm_compare_kernel.h — on-device frame comparison (include/rtm.h: rtm_compare).  Included by rtm_compare.hip.
//
// Two kernels, all arithmetic in double:
//   compare_partial_kernel  blocks of 256 lanes; a block owns a 32 x 32 tile of pixels.  It walks the tile (with its
//                           5-pixel halo when SSIM is wanted) in groups of 48 bytes of each frame — 4 float pixels or 2 double
//                           pixels, aligned in the row-major pixel index, so that a 16-byte aligned frame is read with
//                           16-byte loads — takes the per-pixel error terms of the tile's own pixels and stages the two
//                           luminance planes in LDS.  SSIM's window is then two passes out of LDS, horizontal and vertical,
//                           over the tile's two halves of 16 rows; the five moments never leave the chip.  The block folds
//                           its lanes to one 48-byte partial.
//   compare_final_kernel    one block: folds the partials in ascending order and writes rtm_compare_result.
// No atomics; which lane takes which pixel and every reduction tree depend on the frame size alone, and the plain load path
// visits the same pixels in the same order as the 16-byte one, so the same inputs give the same bits on every call.
#ifndef RTM_COMPARE_KERNEL_H
#define RTM_COMPARE_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kCmpBlock = 256;                         // lanes of a block: four wave64s
constexpr int kCmpTile = 32;                           // a block's tile: 32 x 32 pixels, four per lane
constexpr int kCmpRadius = 5;                          // SSIM's window: 11 x 11
constexpr int kCmpTaps = 2 * kCmpRadius + 1;
constexpr int kCmpHalo = kCmpTile + 2 * kCmpRadius;    // 42: the staged luminance planes are 42 x 42
constexpr int kCmpHalf = kCmpTile / 2;                 // rows the window passes finish at once
constexpr int kCmpHRows = kCmpHalf + 2 * kCmpRadius;   // 26: rows of the horizontal pass that feed 16 rows
constexpr int kCmpMoments = 5;                         // E[a], E[b], E[a a], E[b b], E[a b]
enum { kCmpMapNone = 0, kCmpMapAbs = 1, kCmpMapSsim = 2 };

struct CmpPartial {  // 48 bytes: one per tile
    double sum_sq;    // sum over counting pixels of (dR^2 + dG^2) + dB^2
    double sum_rel;   // sum of d_c^2 / (b_c^2 + rel_epsilon)
    double sum_ssim;  // sum of S_p over the tile's in-frame pixels
    double max_abs;   // max D_p, -1 without a counting pixel
    uint32_t arg;     // the lowest row-major pixel index that attains max_abs
    uint32_t n, outside, mismatch;
};

struct CmpTotal {  // the final kernel's accumulator: the partial with 64-bit counts
    double sum_sq, sum_rel, sum_ssim, max_abs;
    uint64_t n, outside, mismatch;
    uint32_t arg;
};

struct CmpArgs {  // by value: everything lands in SGPRs
    double g[kCmpRadius + 1];  // g[k] = exp(-k^2 / 4.5), from the host
    double tolerance, rel_epsilon, c1, c2, peak;
    int32_t width, height, tiles_x;
};

__device__ inline double cmp_lum(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }
__device__ inline bool cmp_finite3(double r, double g, double b) {
    return __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b);
}
// a component that makes a non-counting pixel a mismatch: neither both NaN nor equal
__device__ inline bool cmp_differs(double a, double b) { return !((a != a && b != b) || a == b); }

// the better of two (max_abs, arg) pairs: the larger error, the lower index on a tie
__device__ inline bool cmp_better(double d, uint32_t p, double best_d, uint32_t best_p) {
    return d > best_d || (d == best_d && p < best_p);
}

__device__ inline CmpPartial cmp_fold(const CmpPartial& a, const CmpPartial& b) {
    CmpPartial o;
    o.sum_sq = a.sum_sq + b.sum_sq;
    o.sum_rel = a.sum_rel + b.sum_rel;
    o.sum_ssim = a.sum_ssim + b.sum_ssim;
    const bool take_b = cmp_better(b.max_abs, b.arg, a.max_abs, a.arg);
    o.max_abs = take_b ? b.max_abs : a.max_abs;
    o.arg = take_b ? b.arg : a.arg;
    o.n = a.n + b.n;
    o.outside = a.outside + b.outside;
    o.mismatch = a.mismatch + b.mismatch;
    return o;
}

// butterfly over the 64 lanes of a wave (xor 32, 16, .. 1): every lane ends with the same bits
__device__ inline CmpPartial cmp_wave_fold(CmpPartial a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        CmpPartial o;
        o.sum_sq = __shfl_xor(a.sum_sq, m, 64);
        o.sum_rel = __shfl_xor(a.sum_rel, m, 64);
        o.sum_ssim = __shfl_xor(a.sum_ssim, m, 64);
        o.max_abs = __shfl_xor(a.max_abs, m, 64);
        o.arg = __shfl_xor(a.arg, m, 64);
        o.n = __shfl_xor(a.n, m, 64);
        o.outside = __shfl_xor(a.outside, m, 64);
        o.mismatch = __shfl_xor(a.mismatch, m, 64);
        a = cmp_fold(a, o);
    }
    return a;
}

// one pixel's six components, widened exactly
struct CmpPixel {
    double a[3], b[3];
};

template <typename T>
struct CmpVec;
template <>
struct CmpVec<float> {
    using type = float4;  // 16 bytes: four components
    static constexpr int kGroup = 4;  // pixels per 48-byte group
};
template <>
struct CmpVec<double> {
    using type = double2;  // 16 bytes: two components
    static constexpr int kGroup = 2;
};

// the 12 (float) or 6 (double) components of an aligned group through three 16-byte loads, as doubles
__device__ inline void cmp_load_group(const float* p, double* out) {
    const float4* v = (const float4*)p;
    const float4 q0 = v[0], q1 = v[1], q2 = v[2];
    out[0] = q0.x, out[1] = q0.y, out[2] = q0.z, out[3] = q0.w;
    out[4] = q1.x, out[5] = q1.y, out[6] = q1.z, out[7] = q1.w;
    out[8] = q2.x, out[9] = q2.y, out[10] = q2.z, out[11] = q2.w;
}
__device__ inline void cmp_load_group(const double* p, double* out) {
    const double2* v = (const double2*)p;
    const double2 q0 = v[0], q1 = v[1], q2 = v[2];
    out[0] = q0.x, out[1] = q0.y, out[2] = q1.x, out[3] = q1.y, out[4] = q2.x, out[5] = q2.y;
}

// Sum of g over the taps of pixel `v` that lie in [0, size): G_x or G_y of the contract.
__device__ inline double cmp_window_norm(const CmpArgs& k, int v, int size) {
    double s = 0.0;
#pragma unroll
    for (int d = -kCmpRadius; d <= kCmpRadius; ++d)
        if (v + d >= 0 && v + d < size) s += k.g[d < 0 ? -d : d];
    return s;
}

// T: the frames' element type.  MAP: what map_out receives (kCmpMap*).  SSIM: the window passes run (the result is
// wanted, or the SSIM map).  VEC: both frames are 16-byte aligned.
template <typename T, int MAP, bool SSIM, bool VEC>
__global__ __launch_bounds__(kCmpBlock) void compare_partial_kernel(const CmpArgs k, const T* __restrict__ fa,
                                                                    const T* __restrict__ fb, CmpPartial* __restrict__ partials,
                                                                    float* __restrict__ map_out) {
    constexpr int G = CmpVec<T>::kGroup;
    constexpr int R = SSIM ? kCmpRadius : 0;
    constexpr int RW = kCmpTile + 2 * R;          // side of the region the block reads
    constexpr int GR = (RW + G - 2) / G + 1;      // groups that can touch one row of the region
    __shared__ double lum[SSIM ? 2 : 1][SSIM ? kCmpHalo * kCmpHalo : 1];
    __shared__ double hbuf[SSIM ? kCmpMoments : 1][SSIM ? kCmpHRows * kCmpTile : 1];
    __shared__ CmpPartial fold_lds[kCmpBlock / 64];

    const int W = k.width, H = k.height;
    const int tile = (int)blockIdx.x;
    const int tx0 = (tile % k.tiles_x) * kCmpTile, ty0 = (tile / k.tiles_x) * kCmpTile;
    const size_t total = (size_t)W * (size_t)H;
    const int t = (int)threadIdx.x;

    if constexpr (SSIM) {  // out-of-frame taps read 0: the window's weights are renormalised over the in-frame ones
        for (int i = t; i < kCmpHalo * kCmpHalo; i += kCmpBlock) lum[0][i] = 0.0, lum[1][i] = 0.0;
        __syncthreads();
    }

    CmpPartial acc{0.0, 0.0, 0.0, -1.0, 0xFFFFFFFFu, 0u, 0u, 0u};
    const int xs = tx0 - R < 0 ? 0 : tx0 - R, xe = tx0 + kCmpTile + R > W ? W : tx0 + kCmpTile + R;
    for (int s = t; s < RW * GR; s += kCmpBlock) {
        const int r = s / GR, j = s % GR;
        const int y = ty0 - R + r;
        if (y < 0 || y >= H) continue;
        const size_t row0 = (size_t)y * (size_t)W;
        const size_t p_lo = row0 + (size_t)xs, p_hi = row0 + (size_t)xe;
        const size_t gp = (p_lo / G + (size_t)j) * G;  // the group's first pixel: a multiple of G, hence 16-byte aligned
        if (gp >= p_hi) continue;
        double ca[3 * G], cb[3 * G];
        const bool whole = VEC && gp + G <= total;
        if (whole) {
            cmp_load_group(fa + gp * 3, ca);
            cmp_load_group(fb + gp * 3, cb);
        }
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const size_t p = gp + (size_t)q;
            if (p < p_lo || p >= p_hi) continue;
            CmpPixel px;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                px.a[c] = whole ? ca[3 * q + c] : (double)fa[p * 3 + c];
                px.b[c] = whole ? cb[3 * q + c] : (double)fb[p * 3 + c];
            }
            const int x = (int)(p - row0);
            const bool counts = cmp_finite3(px.a[0], px.a[1], px.a[2]) && cmp_finite3(px.b[0], px.b[1], px.b[2]);
            if constexpr (SSIM) {
                const int li = r * kCmpHalo + (x - (tx0 - R));
                lum[0][li] = counts ? cmp_lum(px.a[0], px.a[1], px.a[2]) : 0.0;
                lum[1][li] = counts ? cmp_lum(px.b[0], px.b[1], px.b[2]) : 0.0;
            }
            if (x < tx0 || x >= tx0 + kCmpTile || y < ty0 || y >= ty0 + kCmpTile) continue;  // a halo pixel: another tile's
            if (counts) {
                const double dr = fabs(px.a[0] - px.b[0]), dg = fabs(px.a[1] - px.b[1]), db = fabs(px.a[2] - px.b[2]);
                const double D = fmax(fmax(dr, dg), db);
                acc.sum_sq += (dr * dr + dg * dg) + db * db;
                acc.sum_rel += (dr * dr / (px.b[0] * px.b[0] + k.rel_epsilon) + dg * dg / (px.b[1] * px.b[1] + k.rel_epsilon)) +
                               db * db / (px.b[2] * px.b[2] + k.rel_epsilon);
                if (cmp_better(D, (uint32_t)p, acc.max_abs, acc.arg)) acc.max_abs = D, acc.arg = (uint32_t)p;
                acc.n += 1u;
                acc.outside += D > k.tolerance ? 1u : 0u;
                if constexpr (MAP == kCmpMapAbs) map_out[p] = (float)D;
            } else {
                acc.mismatch += (cmp_differs(px.a[0], px.b[0]) || cmp_differs(px.a[1], px.b[1]) || cmp_differs(px.a[2], px.b[2])) ? 1u : 0u;
                if constexpr (MAP == kCmpMapAbs) map_out[p] = __builtin_nanf("");
            }
        }
    }

    if constexpr (SSIM) {
        __syncthreads();
        for (int half = 0; half < 2; ++half) {
            const int base = half * kCmpHalf;  // the half's first tile row; its window rows are base .. base + 25 of the planes
            if (ty0 + base >= H) break;        // (uniform) no pixel of this half is in the frame
            // horizontal: row r of the pass is plane row base + r; column c sums plane columns c .. c + 10
            for (int i = t; i < kCmpHRows * kCmpTile; i += kCmpBlock) {
                const int r = i / kCmpTile, c = i % kCmpTile;
                const double* la = &lum[0][(base + r) * kCmpHalo + c];
                const double* lb = &lum[1][(base + r) * kCmpHalo + c];
                double m[kCmpMoments] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int d = 0; d < kCmpTaps; ++d) {
                    const double g = k.g[d < kCmpRadius ? kCmpRadius - d : d - kCmpRadius];
                    const double va = la[d], vb = lb[d];
                    m[0] = fma(g, va, m[0]);
                    m[1] = fma(g, vb, m[1]);
                    m[2] = fma(g, va * va, m[2]);
                    m[3] = fma(g, vb * vb, m[3]);
                    m[4] = fma(g, va * vb, m[4]);
                }
#pragma unroll
                for (int q = 0; q < kCmpMoments; ++q) hbuf[q][i] = m[q];
            }
            __syncthreads();
            // vertical: lane t finishes the pixels (c, rr) and (c, rr + 8) of the half
            const int c = t % kCmpTile;
            const int x = tx0 + c;
#pragma unroll
            for (int jj = 0; jj < kCmpHalf / (kCmpBlock / kCmpTile); ++jj) {
                const int rr = t / kCmpTile + jj * (kCmpBlock / kCmpTile);
                const int y = ty0 + base + rr;
                if (x >= W || y >= H) continue;
                double m[kCmpMoments] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int d = 0; d < kCmpTaps; ++d) {
                    const double g = k.g[d < kCmpRadius ? kCmpRadius - d : d - kCmpRadius];
#pragma unroll
                    for (int q = 0; q < kCmpMoments; ++q) m[q] = fma(g, hbuf[q][(rr + d) * kCmpTile + c], m[q]);
                }
                const double inv = 1.0 / (cmp_window_norm(k, x, W) * cmp_window_norm(k, y, H));
                const double mu_a = m[0] * inv, mu_b = m[1] * inv;
                const double var_a = m[2] * inv - mu_a * mu_a, var_b = m[3] * inv - mu_b * mu_b;
                const double cov = m[4] * inv - mu_a * mu_b;
                const double S = ((2.0 * mu_a * mu_b + k.c1) * (2.0 * cov + k.c2)) /
                                 ((mu_a * mu_a + mu_b * mu_b + k.c1) * (var_a + var_b + k.c2));
                acc.sum_ssim += S;
                if constexpr (MAP == kCmpMapSsim) map_out[(size_t)y * (size_t)W + (size_t)x] = (float)S;
            }
            __syncthreads();  // the next half overwrites hbuf
        }
    }

    if (partials == nullptr) return;  // (uniform) a map-only call
    acc = cmp_wave_fold(acc);
    if ((t & 63) == 0) fold_lds[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        acc = fold_lds[0];
#pragma unroll
        for (int w = 1; w < kCmpBlock / 64; ++w) acc = cmp_fold(acc, fold_lds[w]);
        partials[tile] = acc;
    }
}

__device__ inline CmpTotal cmp_fold_total(const CmpTotal& a, const CmpTotal& b) {
    CmpTotal o;
    o.sum_sq = a.sum_sq + b.sum_sq;
    o.sum_rel = a.sum_rel + b.sum_rel;
    o.sum_ssim = a.sum_ssim + b.sum_ssim;
    const bool take_b = cmp_better(b.max_abs, b.arg, a.max_abs, a.arg);
    o.max_abs = take_b ? b.max_abs : a.max_abs;
    o.arg = take_b ? b.arg : a.arg;
    o.n = a.n + b.n;
    o.outside = a.outside + b.outside;
    o.mismatch = a.mismatch + b.mismatch;
    return o;
}

// One block.  Lane t folds the partials t, t + 256, .. in ascending order; then the wave butterflies and the four wave results
// in wave order.  record: the work buffer's last 256 bytes; result_out: the caller's (nullable).
__global__ __launch_bounds__(kCmpBlock) void compare_final_kernel(const CmpArgs k, const CmpPartial* __restrict__ partials,
                                                                  const uint32_t n_partials, rtm_compare_result* __restrict__ record,
                                                                  rtm_compare_result* __restrict__ result_out) {
    __shared__ CmpTotal lds[kCmpBlock / 64];
    CmpTotal a{0.0, 0.0, 0.0, -1.0, 0u, 0u, 0u, 0xFFFFFFFFu};
    for (uint32_t i = threadIdx.x; i < n_partials; i += kCmpBlock) {
        const CmpPartial p = partials[i];
        a = cmp_fold_total(a, CmpTotal{p.sum_sq, p.sum_rel, p.sum_ssim, p.max_abs, p.n, p.outside, p.mismatch, p.arg});
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        CmpTotal o;
        o.sum_sq = __shfl_xor(a.sum_sq, m, 64);
        o.sum_rel = __shfl_xor(a.sum_rel, m, 64);
        o.sum_ssim = __shfl_xor(a.sum_ssim, m, 64);
        o.max_abs = __shfl_xor(a.max_abs, m, 64);
        o.n = __shfl_xor((unsigned long long)a.n, m, 64);
        o.outside = __shfl_xor((unsigned long long)a.outside, m, 64);
        o.mismatch = __shfl_xor((unsigned long long)a.mismatch, m, 64);
        o.arg = __shfl_xor(a.arg, m, 64);
        a = cmp_fold_total(a, o);
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    a = lds[0];
#pragma unroll
    for (int w = 1; w < kCmpBlock / 64; ++w) a = cmp_fold_total(a, lds[w]);
    const uint64_t frame = (uint64_t)k.width * (uint64_t)k.height;
    rtm_compare_result r;
    r.max_abs = a.n ? a.max_abs : 0.0;
    r.mse = a.n ? a.sum_sq / (3.0 * (double)a.n) : 0.0;
    r.psnr = r.mse > 0.0 ? 10.0 * log10(k.peak * k.peak / r.mse) : __builtin_inf();
    r.rel_mse = a.n ? a.sum_rel / (3.0 * (double)a.n) : 0.0;
    r.ssim = a.sum_ssim / (double)frame;
    r.pixels = a.n;
    r.outside = a.outside;
    r.nonfinite = frame - a.n;
    r.nonfinite_mismatch = a.mismatch;
    r.argmax_x = a.n ? (int32_t)(a.arg % (uint32_t)k.width) : -1;
    r.argmax_y = a.n ? (int32_t)(a.arg / (uint32_t)k.width) : -1;
    *record = r;
    if (result_out) *result_out = r;
}

}  // namespace rtm
#endif
