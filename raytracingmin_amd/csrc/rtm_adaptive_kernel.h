// rtm_adaptive_kernel.h — the kernels of tile-adaptive sampling (rtm_render_adaptive, include/rtm.h): the list of every
// tile, the checkpoint's error estimate and decision per listed tile, and the compaction of the still-active tiles into the
// next pass's list.  Included by rtm_adaptive.hip only; no render kernel lives here.
//
// The accumulator and the snapshot share rtm_render_scene's out_f64 layout: local output row r, column x at ((r * W) + x) * 3.
// Tile t covers columns 8 (t % tiles_x) .. +7 and local rows 8 (t / tiles_x) .. +7 (band_row maps them to image rows the
// same way for a row range or a band part); a pixel is in the frame iff x < W and r < rows.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rtm {

struct AdaptiveCheck {
    const double* __restrict__ acc;     // the accumulator after the pass that ended at b
    double* __restrict__ snap;          // the accumulator after the pass that ended at a (the previous checkpoint)
    const unsigned* __restrict__ list;  // the pass's tiles
    unsigned* __restrict__ flags;       // per list entry: 1 = the tile stays active
    unsigned* __restrict__ tile_samples;  // per frame tile: samples traced (nullable)
    int W, rows, tiles_x;
    unsigned frame_tiles;
    unsigned b;           // b_i: this checkpoint's end
    unsigned last;        // b_i == N: no tile stays active
    double sb, sa;        // N / b_i, N / b_{i-1}: the preview scales of rtm_render_scene_samples
    double threshold;
};

// Every tile: list[t] = t and tile_samples[t] = b_0.
__global__ __launch_bounds__(256) void adaptive_begin_kernel(unsigned* __restrict__ list, unsigned* __restrict__ tile_samples,
                                                             unsigned n, unsigned b0) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    list[t] = t;
    if (tile_samples) tile_samples[t] = b0;
}

// One wave per list entry, lane = pixel of the tile.  E <= threshold exactly when every in-frame pixel's e_p <= threshold
// (a NaN e_p fails the test, as a NaN E would), so the wave's maximum is a ballot of the failing lanes.
__global__ __launch_bounds__(64) void adaptive_check_kernel(const AdaptiveCheck A) {
    const unsigned i = blockIdx.x;
    const int lane = threadIdx.x;
    const unsigned t = A.list[i];
    if (t >= A.frame_tiles) {  // (an entry past the frame: its render blocks returned at once; it is dropped)
        if (lane == 0) A.flags[i] = 0u;
        return;
    }
    const int x = (int)(t % (unsigned)A.tiles_x) * 8 + (lane & 7);
    const int r = (int)(t / (unsigned)A.tiles_x) * 8 + (lane >> 3);
    const bool valid = x < A.W && r < A.rows;
    const size_t o = ((size_t)r * (size_t)A.W + (size_t)x) * 3;
    bool ok = true;  // e_p <= threshold (pixels outside the frame do not take part)
    if (valid) {
        const double ir = A.acc[o] * A.sb, ig = A.acc[o + 1] * A.sb, ib = A.acc[o + 2] * A.sb;
        const double jr = A.snap[o] * A.sa, jg = A.snap[o + 1] * A.sa, jb = A.snap[o + 2] * A.sa;
        const double d = (fabs(ir - jr) + fabs(ig - jg)) + fabs(ib - jb);
        const double e = d / (1e-3 + sqrt((ir + ig) + ib));
        ok = e <= A.threshold;
    }
    const bool stop = __builtin_amdgcn_ballot_w64(!ok) == 0ull;
    const bool active = A.last == 0u && !stop;
    if (active && valid) {
        A.snap[o] = A.acc[o];
        A.snap[o + 1] = A.acc[o + 1];
        A.snap[o + 2] = A.acc[o + 2];
    }
    if (lane == 0) {
        A.flags[i] = active ? 1u : 0u;
        if (A.tile_samples) A.tile_samples[t] = A.b;
    }
}

// The active entries of `list`, in list order, to `out`, and their count to *count: one block, each thread a contiguous run
// of entries, an exclusive scan of the runs' counts in LDS.  No atomics: equal inputs give equal lists.
constexpr unsigned kCompactThreads = 1024;
__global__ __launch_bounds__(kCompactThreads) void adaptive_compact_kernel(const unsigned* __restrict__ flags,
                                                                           const unsigned* __restrict__ list, unsigned n,
                                                                           unsigned* __restrict__ out,
                                                                           unsigned* __restrict__ count) {
    __shared__ unsigned scan[kCompactThreads];
    const unsigned tid = threadIdx.x;
    const unsigned per = (n + kCompactThreads - 1u) / kCompactThreads;
    const unsigned begin = tid * per < n ? tid * per : n;
    const unsigned end = begin + per < n ? begin + per : n;
    unsigned mine = 0u;
    for (unsigned j = begin; j < end; ++j) mine += flags[j];
    scan[tid] = mine;
    __syncthreads();
    for (unsigned step = 1u; step < kCompactThreads; step <<= 1) {  // inclusive Hillis-Steele scan
        const unsigned add = tid >= step ? scan[tid - step] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    unsigned pos = scan[tid] - mine;
    for (unsigned j = begin; j < end; ++j)
        if (flags[j]) out[pos++] = list[j];
    if (tid == kCompactThreads - 1u) *count = scan[tid];
}

}  // namespace rtm
