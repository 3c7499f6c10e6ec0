// rtm_resize_kernel.h — filtered resampling (include/rtm.h: rtm_resize).  Included by rtm_resize.hip.
//
// Three kernels, no atomics, no scratch.
//   tables      one lane per destination index of either axis (W + H lanes): the integer taps of rtm.h, the kernel in
//               double, the normalised weights rounded to float.  Stored tap-major ([i][X]) so that the 64 lanes of a wave,
//               which run along X in both passes, read consecutive floats; the first tap j0 goes to an int array.
//   horizontal  a block of 256 lanes owns 64 destination columns of 4 source rows, one row a wave.  The source span of
//               the 64 columns, j0[X0] .. j0[X0 + 63] + Tx, is staged in LDS in chunks of kRsChunk pixels as records
//               (c m, m): a pixel that does not count or lies outside the frame is all zeros, which adds +-0 to every
//               sum and so selects it out.  The chunks ascend, and inside a chunk the taps ascend, so each lane adds its
//               taps in ascending order whatever the ratio.  Each lane stores one record, coalesced.
//   vertical    the same 64 x 4 tile of destination pixels; a loop over the Ty rows of records (each load a coalesced row),
//               the threshold, the division and the stores of out_f32 and out_u8, word by word and byte by byte: the same
//               instructions at any alignment.
// Both passes walk their tiles with a grid-stride loop, so a frame a few pixels wide and 2^30 high needs no huge grid.
#ifndef RTM_RESIZE_KERNEL_H
#define RTM_RESIZE_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kRsTileX = 64, kRsTileY = 4;      // a block's tile: a wave a row
constexpr int kRsBlock = kRsTileX * kRsTileY;   // 256 lanes
constexpr int kRsChunk = 256;                   // source pixels a row staged at once: 4 x 256 x 16 bytes = 16 KiB (C = 3)
constexpr int kRsTableBlock = 256;
constexpr float kRsMinWeight = 0.0625f;         // rtm.h: D below it is a hole

template <int C> struct rs_record;
template <> struct rs_record<3> { typedef float4 type; };
template <> struct rs_record<1> { typedef float2 type; };

// rtm_quantise of (double)v: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0
__device__ inline uint8_t rs_quantise(float f) {
    const double v = (double)f;
    const double q = 255 * ((1.0 < v) ? 1.0 : v);
    return (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
}

// k(t) of rtm.h for TRIANGLE, MITCHELL and LANCZOS3 (BOX is decided in integers by the caller)
__device__ inline double rs_kernel(int filter, double t) {
    const double a = fabs(t);
    if (filter == RTM_RESIZE_TRIANGLE) return a < 1.0 ? 1.0 - a : 0.0;
    if (filter == RTM_RESIZE_MITCHELL) {
        if (a < 1.0) return (7.0 * a * a * a - 12.0 * a * a + 16.0 / 3.0) / 6.0;
        if (a < 2.0) return (-7.0 / 3.0 * a * a * a + 12.0 * a * a - 20.0 * a + 32.0 / 3.0) / 6.0;
        return 0.0;
    }
    if (a == 0.0) return 1.0;
    if (a >= 3.0) return 0.0;
    const double x = 3.14159265358979323846 * t, x3 = x / 3.0;
    return (sin(x) / x) * (sin(x3) / x3);
}

// the raw weight of the tap at source index j: a = 2 N j - b, t = a / (2 M)
__device__ inline double rs_raw(int filter, int64_t N, int64_t M, int64_t b, int64_t j) {
    const int64_t a = 2 * N * j - b;
    if (filter == RTM_RESIZE_BOX) return (-M < a && a <= M) ? 1.0 : 0.0;
    return rs_kernel(filter, (double)a / (double)(2 * M));
}

// lanes 0..W-1: the x axis (w -> W); lanes W..W+H-1: the y axis (h -> H).  q = 2 r.
__global__ __launch_bounds__(kRsTableBlock) void resize_tables_kernel(const int w, const int h, const int W, const int H,
                                                                      const int filter, const int q, const int Tx, const int Ty,
                                                                      float* __restrict__ tab_x, float* __restrict__ tab_y,
                                                                      int* __restrict__ j0_x, int* __restrict__ j0_y) {
    const int64_t lane = (int64_t)blockIdx.x * kRsTableBlock + threadIdx.x;
    if (lane >= (int64_t)W + H) return;
    const bool xa = lane < W;
    const int64_t X = xa ? lane : lane - W;
    const int64_t n = xa ? w : h, N = xa ? W : H, M = n > N ? n : N;
    const int T = xa ? Tx : Ty;
    float* const tab = xa ? tab_x : tab_y;
    const int64_t b = (2 * X + 1) * n - N;
    const int64_t num = b - (int64_t)q * M, den = 2 * N;
    int64_t fl = num / den;
    if (num % den != 0 && num < 0) --fl;  // floor toward minus infinity
    const int64_t j0 = fl + 1;
    (xa ? j0_x : j0_y)[X] = (int)j0;
    double sum = 0.0;
    for (int i = 0; i < T; ++i) sum += rs_raw(filter, N, M, b, j0 + i);
    for (int i = 0; i < T; ++i) tab[(size_t)i * (size_t)N + (size_t)X] = (float)(rs_raw(filter, N, M, b, j0 + i) / sum);
}

template <int C>
__device__ inline typename rs_record<C>::type rs_zero();
template <> __device__ inline float4 rs_zero<3>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
template <> __device__ inline float2 rs_zero<1>() { return make_float2(0.0f, 0.0f); }

// a source pixel as a record: (c, 1) when it counts, zeros when not
__device__ inline float4 rs_load(const float* __restrict__ src, size_t p, float4*) {
    const float r = src[3 * p], g = src[3 * p + 1], b = src[3 * p + 2];
    const bool m = __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b);
    return m ? make_float4(r, g, b, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
__device__ inline float2 rs_load(const float* __restrict__ src, size_t p, float2*) {
    const float c = src[p];
    return __builtin_isfinite(c) ? make_float2(c, 1.0f) : make_float2(0.0f, 0.0f);
}
__device__ inline void rs_add(float4& acc, float wt, const float4 r) {
    acc.x += wt * r.x;
    acc.y += wt * r.y;
    acc.z += wt * r.z;
    acc.w += wt * r.w;
}
__device__ inline void rs_add(float2& acc, float wt, const float2 r) {
    acc.x += wt * r.x;
    acc.y += wt * r.y;
}

// records[y][X] = sum_i w^x[X][i] (m c, m)(y, j0x[X] + i), for y in 0..h-1 and X in 0..W-1
template <int C>
__global__ __launch_bounds__(kRsBlock) void resize_horizontal_kernel(const int w, const int h, const int W, const int Tx,
                                                                     const unsigned tiles_x, const size_t tiles,
                                                                     const float* __restrict__ src,
                                                                     const float* __restrict__ tab_x,
                                                                     const int* __restrict__ j0_x,
                                                                     typename rs_record<C>::type* __restrict__ records) {
    typedef typename rs_record<C>::type rec_t;
    __shared__ rec_t span[kRsTileY][kRsChunk];
    const int lx = (int)threadIdx.x % kRsTileX, ly = (int)threadIdx.x / kRsTileX;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // (64-bit: X0 + 64 and Y0 + 4 may pass 2^31 on a frame one pixel thin)
        const int64_t X0 = (int64_t)(tile % tiles_x) * kRsTileX;
        const int64_t Y0 = (int64_t)(tile / tiles_x) * kRsTileY;   // tile / tiles_x < ceil(h / 4)
        const int64_t X1 = min(X0 + kRsTileX, (int64_t)W) - 1;      // the tile's last column
        const int rows = (int)min((int64_t)kRsTileY, h - Y0);
        // the in-frame span of the tile's taps: j0 ascends with X (block-uniform)
        const int64_t s_begin = max(j0_x[X0], 0);
        const int64_t s_end = min((int64_t)j0_x[X1] + Tx, (int64_t)w);
        const int64_t X = X0 + lx, y = Y0 + ly;
        const bool live = X < W && y < h;
        const int j0 = live ? j0_x[X] : 0;
        rec_t acc = rs_zero<C>();
        for (int64_t cs = s_begin; cs < s_end; cs += kRsChunk) {  // (64-bit: cs + kRsChunk may pass 2^31)
            const int len = (int)min((int64_t)kRsChunk, s_end - cs);
            for (int it = (int)threadIdx.x; it < rows * len; it += kRsBlock) {
                const int r = it / len, c = it - r * len;
                span[r][c] = rs_load(src, (size_t)(Y0 + r) * (size_t)w + (size_t)(cs + c), (rec_t*)nullptr);
            }
            __syncthreads();
            if (live) {  // this lane's taps inside the chunk: j0 + i in [cs, cs + len)
                const int i_lo = (int)max((int64_t)0, cs - j0);
                const int i_hi = (int)min((int64_t)Tx, cs + len - j0);
                const int at = (int)(j0 - cs);  // span[ly][at + i]: in 0..len-1 for i_lo <= i < i_hi
                for (int i = i_lo; i < i_hi; ++i)
                    rs_add(acc, tab_x[(size_t)i * (size_t)W + (size_t)X], span[ly][at + i]);
            }
            __syncthreads();
        }
        if (live) records[(size_t)y * (size_t)W + (size_t)X] = acc;
    }
}

__device__ inline void rs_write(const float4 n, const float d, size_t p, float* __restrict__ out32, uint8_t* __restrict__ out8) {
    const bool ok = d >= kRsMinWeight;  // (d is a sum of weights times 0 or 1: never NaN)
    const float qnan = __uint_as_float(0x7FC00000u);
    const float r = ok ? n.x / d : qnan, g = ok ? n.y / d : qnan, b = ok ? n.z / d : qnan;
    if (out32) {
        out32[3 * p] = r;
        out32[3 * p + 1] = g;
        out32[3 * p + 2] = b;
    }
    if (out8) {
        out8[3 * p] = rs_quantise(r);
        out8[3 * p + 1] = rs_quantise(g);
        out8[3 * p + 2] = rs_quantise(b);
    }
}
__device__ inline void rs_write(const float2 n, const float, size_t p, float* __restrict__ out32, uint8_t* __restrict__ out8) {
    const float v = n.y >= kRsMinWeight ? n.x / n.y : __uint_as_float(0x7FC00000u);
    if (out32) out32[p] = v;
    if (out8) out8[p] = rs_quantise(v);
}
__device__ inline float rs_weight(const float4 r) { return r.w; }
__device__ inline float rs_weight(const float2 r) { return r.y; }

// out[Y][X] = (sum_i w^y[Y][i] records[j0y[Y] + i][X]).c / .m over the rows inside the frame
template <int C>
__global__ __launch_bounds__(kRsBlock) void resize_vertical_kernel(const int h, const int W, const int H, const int Ty,
                                                                   const unsigned tiles_x, const size_t tiles,
                                                                   const typename rs_record<C>::type* __restrict__ records,
                                                                   const float* __restrict__ tab_y,
                                                                   const int* __restrict__ j0_y, float* __restrict__ out32,
                                                                   uint8_t* __restrict__ out8) {
    typedef typename rs_record<C>::type rec_t;
    const int lx = (int)threadIdx.x % kRsTileX, ly = (int)threadIdx.x / kRsTileX;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t X = (int64_t)(tile % tiles_x) * kRsTileX + lx;
        const int64_t Y = (int64_t)(tile / tiles_x) * kRsTileY + ly;
        if (X >= W || Y >= H) continue;  // (no barrier in this kernel)
        const int j0 = j0_y[Y];
        const int i_lo = max(0, -j0);
        const int i_hi = (int)min((int64_t)Ty, (int64_t)h - j0);
        rec_t acc = rs_zero<C>();
        for (int i = i_lo; i < i_hi; ++i)
            rs_add(acc, tab_y[(size_t)i * (size_t)H + (size_t)Y], records[(size_t)(j0 + i) * (size_t)W + (size_t)X]);
        rs_write(acc, rs_weight(acc), (size_t)Y * (size_t)W + (size_t)X, out32, out8);
    }
}

}  // namespace rtm
#endif
