// rtm_scope_kernel.h — the frame scopes (include/rtm.h: rtm_scopes, rtm_scope_draw).  Included by rtm_scope.hip.
//
// The first stage here whose hot path is a scatter: every counting pixel adds 1 to four bins.  Integer atomics only, on LDS
// and on the outputs' words; the sums are exact, so no order can change a word.
//   histogram  (hist_out alone) at most kScHistGrid blocks of sixteen waves, one a CU, run over the frame with a grid stride,
//              one pixel a lane.  A block keeps kScCopies copies of the histogram in LDS, 4 channels x 258 slots (256 bins,
//              below, above) x 8 words, 33 KB, and a lane adds to copy lane & 7.  What decides the cost is a wave whose lanes
//              all hit one bin (a wall, a constant frame): LDS adds to one word are served one after the other, and the copies
//              cut a wave's 64 to 8 a word, in 8 neighbouring banks.  After the frame the block sums the copies and issues
//              one global add per non-zero slot.  Those adds are why the grid is small: every block adds to the same 1032
//              words, the adds to one word are served one after the other (about 30 ns each, measured), and with 2048 blocks
//              they were most of the call.  (Built, measured and folded out: a private histogram per wave with the lanes
//              that share the first active lane's bin counted by a ballot and added once, with and without a loop over the
//              rest.  With the copies in place the ballot only costs.  DESIGN.md §Scopes has the numbers.)
//   waveform   (waveform_out, with or without hist_out) a block owns a strip of kScStrip output columns and a band of rows
//              and keeps the strip's [4][256][kScStrip] counts in LDS (32 KB).  Its lanes walk the strip's frame columns row
//              by row, so a wave reads a run of consecutive pixels.  The fold issues one global add per non-zero word.  With
//              hist_out the same block also keeps below[4] and above[4] and gives the histogram from its strip's row sums:
//              the frame is read once for both outputs.
//   draw       one lane per output pixel, no atomics.
#ifndef RTM_SCOPE_KERNEL_H
#define RTM_SCOPE_KERNEL_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtm.h"

namespace rtm {

constexpr int kScBlock = 256;                 // four wave64s: the waveform's and the picture's block
constexpr int kScHistBlock = 1024;            // sixteen wave64s: the histogram's block, one a CU
constexpr int kScHistGrid = 256;              // the most blocks the histogram launches: every block adds to the same words
constexpr int kScCopies = 8;                  // copies of every slot in the histogram's LDS, one per lane & 7
constexpr int kScSlots = 258;                 // 256 bins, then BELOW, then ABOVE
constexpr int kScBelow = 256, kScAbove = 257;
constexpr int kScStrip = 8;                   // output columns a waveform block owns
// rtm_scope_histogram as words: bins[4][256], below[4], above[4], pixels, not_counting, reserved[2]
constexpr int kScHistBelow = 1024, kScHistAbove = 1028, kScHistPixels = 1032, kScHistWords = 1036;
static_assert(sizeof(rtm_scope_histogram) == kScHistWords * 4, "rtm_scope_histogram is 4144 bytes without padding");

// steps 3 and 4: the slot of one channel value of a counting pixel
__device__ inline int scope_slot(float v, int mode) {
    if (mode == RTM_SCOPE_LOG2) {
        const uint32_t u = __float_as_uint(v);
        const uint32_t top = u >> 20;  // sign, exponent, three bits of the fraction
        if (top < 888u) return kScBelow;
        if (top >= 2048u) return kScBelow;  // the sign bit is set
        const uint32_t b = top - 888u;
        return b > 255u ? kScAbove : (int)b;
    }
    if (v < 0.0f) return kScBelow;
    if (v > 1.0f) return kScAbove;
    return (int)(255.0 * (double)v);
}

// steps 1 and 2: whether the pixel counts, and its four slots
__device__ inline bool scope_pixel(const float* __restrict__ color, size_t q, int mode, int slot[4]) {
    const float r = color[3 * q], g = color[3 * q + 1], b = color[3 * q + 2];
    if (!(__builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b))) return false;
    const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    slot[0] = scope_slot(l > 0.0f ? l : 0.0f, mode);
    slot[1] = scope_slot(r, mode);
    slot[2] = scope_slot(g, mode);
    slot[3] = scope_slot(b, mode);
    return true;
}

__global__ __launch_bounds__(kScHistBlock) void scope_hist_kernel(const uint32_t pix, const int mode,
                                                                  const float* __restrict__ color, uint32_t* __restrict__ hist) {
    __shared__ uint32_t lds[4 * kScSlots * kScCopies];
    __shared__ uint32_t tally[2];  // counting, not counting
    for (int s = (int)threadIdx.x; s < 4 * kScSlots * kScCopies; s += kScHistBlock) lds[s] = 0u;
    if (threadIdx.x < 2) tally[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t* const mine = lds + (threadIdx.x & (unsigned)(kScCopies - 1));  // this lane's copy: its words kScCopies apart
    uint32_t counting = 0u, not_counting = 0u;
    const uint32_t stride = gridDim.x * (uint32_t)kScHistBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kScHistBlock + threadIdx.x; q < pix; q += stride) {
        int slot[4];
        if (!scope_pixel(color, (size_t)q, mode, slot)) {
            ++not_counting;
            continue;
        }
        ++counting;
#pragma unroll
        for (int c = 0; c < 4; ++c) atomicAdd(&mine[(c * kScSlots + slot[c]) * kScCopies], 1u);
    }
    if (counting) atomicAdd(&tally[0], counting);
    if (not_counting) atomicAdd(&tally[1], not_counting);
    __syncthreads();
    for (int s = (int)threadIdx.x; s < 4 * kScSlots; s += kScHistBlock) {
        uint32_t sum = 0u;
#pragma unroll
        for (int k = 0; k < kScCopies; ++k) sum += lds[s * kScCopies + k];
        if (sum == 0u) continue;
        const int c = s / kScSlots, k = s - c * kScSlots;
        atomicAdd(&hist[k < 256 ? c * 256 + k : k == kScBelow ? kScHistBelow + c : kScHistAbove + c], sum);
    }
    if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(&hist[kScHistPixels + threadIdx.x], tally[threadIdx.x]);
}

// grid.x: the strips of kScStrip output columns; grid.y: the bands of `band` rows
template <bool HIST>
__global__ __launch_bounds__(kScBlock) void scope_wave_kernel(const int W, const int H, const int columns, const int mode,
                                                              const int band, const float* __restrict__ color,
                                                              uint32_t* __restrict__ hist, uint32_t* __restrict__ wave) {
    __shared__ uint32_t cnt[4 * 256 * kScStrip];
    __shared__ uint32_t edge[10];  // below[4], above[4], counting, not counting
    for (int s = (int)threadIdx.x; s < 4 * 256 * kScStrip; s += kScBlock) cnt[s] = 0u;
    if (threadIdx.x < 10) edge[threadIdx.x] = 0u;
    __syncthreads();
    const int oc0 = (int)blockIdx.x * kScStrip;
    const int oc1 = oc0 + kScStrip < columns ? oc0 + kScStrip : columns;
    // output column oc holds the frame columns from ceil(oc W / columns) on
    const int x0 = (int)(((int64_t)oc0 * W + columns - 1) / columns), x1 = (int)(((int64_t)oc1 * W + columns - 1) / columns);
    const int r0 = (int)blockIdx.y * band, r1 = r0 + band < H ? r0 + band : H;
    const uint32_t nx = (uint32_t)(x1 - x0);
    const uint32_t total = nx * (uint32_t)(r1 - r0);  // at most the frame's pixels, under 2^31
    const bool narrow = (uint64_t)W * (uint64_t)columns <= 0xFFFFFFFFull;  // x columns fits 32 bits
    uint32_t counting = 0u, not_counting = 0u;
    for (uint32_t i = threadIdx.x; i < total; i += kScBlock) {
        const uint32_t dy = i / nx;
        const uint32_t x = (uint32_t)x0 + (i - dy * nx);
        const size_t q = (size_t)(r0 + (int)dy) * (size_t)W + x;
        int slot[4];
        if (!scope_pixel(color, q, mode, slot)) {
            ++not_counting;
            continue;
        }
        ++counting;
        const uint32_t oc = narrow ? x * (uint32_t)columns / (uint32_t)W : (uint32_t)((uint64_t)x * (uint64_t)columns / (uint64_t)W);
        const uint32_t at = oc - (uint32_t)oc0;  // < kScStrip
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = slot[c];
            const int b = k == kScBelow ? 0 : k == kScAbove ? 255 : k;
            atomicAdd(&cnt[(c * 256 + b) * kScStrip + at], 1u);
            if (HIST && k >= kScBelow) atomicAdd(&edge[(k - kScBelow) * 4 + c], 1u);
        }
    }
    if (HIST) {
        if (counting) atomicAdd(&edge[8], counting);
        if (not_counting) atomicAdd(&edge[9], not_counting);
    }
    __syncthreads();
    const int strip = oc1 - oc0;
    for (int s = (int)threadIdx.x; s < 4 * 256 * kScStrip; s += kScBlock) {
        const uint32_t v = cnt[s];
        const int cb = s / kScStrip, at = s - cb * kScStrip;
        if (v != 0u && at < strip) atomicAdd(&wave[(size_t)cb * (size_t)columns + (size_t)(oc0 + at)], v);
    }
    if (HIST) {
        for (int cb = (int)threadIdx.x; cb < 4 * 256; cb += kScBlock) {
            uint32_t sum = 0u;
#pragma unroll
            for (int at = 0; at < kScStrip; ++at) sum += cnt[cb * kScStrip + at];
            const int c = cb >> 8, b = cb & 255;
            if (b == 0) sum -= edge[c];
            if (b == 255) sum -= edge[4 + c];
            if (sum != 0u) atomicAdd(&hist[cb], sum);
        }
        // below[4] and above[4] follow each other in the record, and so do pixels and not_counting
        if (threadIdx.x < 8 && edge[threadIdx.x]) atomicAdd(&hist[kScHistBelow + threadIdx.x], edge[threadIdx.x]);
        if (threadIdx.x >= 8 && threadIdx.x < 10 && edge[threadIdx.x])
            atomicAdd(&hist[kScHistPixels + threadIdx.x - 8], edge[threadIdx.x]);
    }
}

// 256 rows of `out_w` RGB pixels, bin 255 on top; out_w is columns, or 3 columns for the parade
__global__ __launch_bounds__(kScBlock) void scope_draw_kernel(const uint32_t columns, const uint32_t out_w, const int layout,
                                                              const uint32_t gain, const uint32_t* __restrict__ wave,
                                                              uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * (uint32_t)kScBlock + threadIdx.x;
    if (i >= 256u * out_w) return;
    const uint32_t row = i / out_w, x = i - row * out_w;
    const uint32_t b = 255u - row;
    const auto value = [&](uint32_t plane, uint32_t oc) {
        const uint64_t v = (uint64_t)wave[((size_t)plane * 256 + b) * columns + oc] * gain;
        return (uint8_t)(v < 255u ? v : 255u);
    };
    uint8_t red, green, blue;
    if (layout == RTM_SCOPE_LUMA) {
        red = green = blue = value(0u, x);
    } else if (layout == RTM_SCOPE_OVERLAY) {
        red = value(1u, x);
        green = value(2u, x);
        blue = value(3u, x);
    } else {
        const uint32_t panel = x / columns;
        const uint8_t v = value(1u + panel, x - panel * columns);
        red = panel == 0u ? v : (uint8_t)0;
        green = panel == 1u ? v : (uint8_t)0;
        blue = panel == 2u ? v : (uint8_t)0;
    }
    out[3 * (size_t)i] = red;
    out[3 * (size_t)i + 1] = green;
    out[3 * (size_t)i + 2] = blue;
}

}  // namespace rtm
#endif
