// rtm_matte_kernel.h — coverage AOVs of a frame: alpha and the ranked, Cryptomatte-style id / coverage layers behind every
// pixel (include/rtm.h: rtm_render_mattes), the matte of a set of objects cut from them (rtm_matte) and premultiplied "over"
// a background (rtm_composite).  Included by rtm_matte.hip, whose -ffp-contract=off build is the reference's own arithmetic.
// rtm_matte.hip itself is included by rtm_kernels.hip: one code object with the render and AOV kernels.
//
// matte_kernel is aov_kernel's shape (rtm_aov_kernel.h): one wave per 8x8 tile, lane = pixel, the SS^2 sub-pixels in the
// reference's loop order through the same wave-uniform nearest-hit searches.  Instead of reducing normals and colours, each
// lane files the SS^2 object ids it meets in dynamic LDS laid out [sub-pixel][lane] — word k * 64 + lane, so the 64 lanes of
// an access fall into 64 consecutive words: no bank conflict —, behind the grid walk's candidate queue where there is one
// (aov_lds_bytes, the one size rule of both launchers).  matte_rank then turns that list into the ranked layers.
#ifndef RTM_MATTE_KERNEL_H
#define RTM_MATTE_KERNEL_H
#include "rtm_aov_kernel.h"

namespace rtm {

constexpr int kMatteMaxLayers = 8;  // rtm_render_mattes' layers: the ranking keeps this many in registers
constexpr int kMatteMaxSS = 8;      // 8^2 ids x 64 lanes x 4 B = 16 KiB of LDS
constexpr int kMatteMaxIds = 64;    // rtm_matte's id list, staged once per block

// What matte_rank leaves: the kMatteMaxLayers best (id, count) pairs, best first, (-1, 0) where the pixel has fewer objects;
// `hits` the number of sub-pixels that hit anything.  Only ever indexed by unrolled loops: registers, never scratch.
struct MatteRank {
    int id[kMatteMaxLayers];
    int cnt[kMatteMaxLayers];
    int hits;
};

// Ranks one lane's id list ids[k * 64] (k = 0 .. n - 1; `ids` already points at the lane's word).  Any negative id is a miss.
// An in-place sort followed by run-length counting:
//   1 Batcher's odd-even merge sort of the n words, ascending as signed integers.  Its comparators do not depend on the data
//     and n is wave-uniform, so the whole wave runs one instruction stream; a comparator that would reach past n - 1 is left
//     out, which is the network for the next power of two with +inf in the missing places (they never move).  543
//     comparators for n = 64, against 2 016 of a transposition sort.
//   2 one pass over the sorted list: each run of equal ids is one object and its count.  Runs arrive by ascending id, so
//     placing a run behind every kept pair whose count is at least its own orders ties by ascending id; negative runs come
//     first and are only skipped.  The kept pairs live in MatteRank's registers: an unrolled shift-insert, no indexed array.
// It holds for n distinct ids (every run has count 1: the lowest kMatteMaxLayers ids stay) and for any id up to 2^31 - 1.
__device__ __forceinline__ MatteRank matte_rank(int* ids, int n) {
    for (int p = 1; p < n; p *= 2) {
        for (int k = p; k >= 1; k /= 2) {
            for (int j = k % p; j + k < n; j += 2 * k) {
                const int span = min(k, n - j - k);
                for (int i = 0; i < span; ++i) {
                    if ((i + j) / (2 * p) != (i + j + k) / (2 * p)) continue;
                    const int a = ids[(i + j) * 64], b = ids[(i + j + k) * 64];
                    ids[(i + j) * 64] = min(a, b);
                    ids[(i + j + k) * 64] = max(a, b);
                }
            }
        }
    }
    MatteRank r;
#pragma unroll
    for (int l = 0; l < kMatteMaxLayers; ++l) {
        r.id[l] = -1;
        r.cnt[l] = 0;
    }
    r.hits = 0;
    int k = 0;
    while (k < n) {
        const int id = ids[k * 64];
        int cnt = 1;
        for (++k; k < n && ids[k * 64] == id; ++k) ++cnt;
        if (id < 0) continue;
        r.hits += cnt;
        int cid = id, cc = cnt;
        bool shift = false;
#pragma unroll
        for (int l = 0; l < kMatteMaxLayers; ++l) {
            shift = shift || cnt > r.cnt[l];  // the run's place: before the first kept pair with a smaller count
            if (shift) {
                const int tid = r.id[l], tc = r.cnt[l];
                r.id[l] = cid;
                r.cnt[l] = cc;
                cid = tid;
                cc = tc;
            }
        }
    }
    return r;
}

// The layers and alpha of one pixel from its ranking: plane l of id / coverage at l * plane + pix.
__device__ __forceinline__ void matte_store(const MatteRank& r, int n_sub, int layers, size_t plane, size_t pix,
                                            const rtm_matte_buffers& out) {
    const double n = (double)n_sub;
#pragma unroll
    for (int l = 0; l < kMatteMaxLayers; ++l) {
        if (l >= layers) break;
        if (out.id) out.id[(size_t)l * plane + pix] = r.id[l];
        if (out.coverage) out.coverage[(size_t)l * plane + pix] = (float)((double)r.cnt[l] / n);
    }
    if (out.alpha) out.alpha[pix] = (float)((double)r.hits / n);
}

template <int SEARCH, class Scene>
__global__ __launch_bounds__(64) void matte_kernel(const RenderParams P, const rtm_matte_buffers out, const int layers,
                                                   const size_t plane) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];  // [kAovGrid: the walks' queue][the id lists]
    const int lane = threadIdx.x;
    int* ids = reinterpret_cast<int*>(lds_raw + aov_lds_bytes(SEARCH)) + lane;
    Scene sc;
    sc.v = P.scene;
    const int tile = (int)blockIdx.x;
    const int px = (tile % P.tiles_x) * 8 + (lane & 7), py = band_row(P, tile / P.tiles_x, lane >> 3);
    const bool valid = px < P.W && py < P.row_end;  // (a lane outside the frame traces a finite ray and stores nothing)
    int k = 0;
    for (int sx = 1; sx <= P.SS; ++sx) {
        for (int sy = 1; sy <= P.SS; ++sy, ++k) {
            const D3 dir = primary_dir(P, px, py, sx, sy);  // :227-232
            double dis;
            int id;
            if constexpr (SEARCH == kAovGrid)
                id = nearest_hit_grid<MathFast, Scene>(sc, P.cam_org, dir, dis, lds_raw, 64, lane);
            else if constexpr (SEARCH == kAovGeneral)
                id = nearest_hit<MathRef, 1>(sc, P.cam_org, dir, dis);
            else
                id = nearest_hit<MathFast, 8>(sc, P.cam_org, dir, dis);
            ids[k * 64] = id;  // (read back by this lane alone: no barrier)
        }
    }
    const MatteRank r = matte_rank(ids, k);
    if (!valid) return;
    matte_store(r, k, layers, plane, out_index(P, px, py) / 3, out);
}

// rtm_debug_matte_rank: the ranking alone on caller-given id lists, 64 pixels a block in matte_kernel's LDS layout
__global__ __launch_bounds__(64) void matte_rank_kernel(const int n_sub, const int layers, const int32_t* __restrict__ ids_in,
                                                        const size_t n_pixels, const rtm_matte_buffers out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x;
    int* ids = reinterpret_cast<int*>(lds_raw) + lane;
    const size_t pix = (size_t)blockIdx.x * 64 + lane;
    const bool valid = pix < n_pixels;
    for (int k = 0; k < n_sub; ++k) ids[k * 64] = valid ? ids_in[pix * (size_t)n_sub + k] : -1;
    const MatteRank r = matte_rank(ids, n_sub);
    if (!valid) return;
    matte_store(r, n_sub, layers, n_pixels, pix, out);
}

// rtm_matte: the summed coverage of the layers whose id is in the list, in double from +0 over ascending layers, at most 1
__global__ __launch_bounds__(256) void matte_extract_kernel(const size_t n_pixels, const int layers,
                                                            const int32_t* __restrict__ layer_id,
                                                            const float* __restrict__ layer_coverage,
                                                            const int32_t* __restrict__ sel, const int n_sel,
                                                            float* __restrict__ matte) {
    __shared__ int s_sel[kMatteMaxIds];
    if ((int)threadIdx.x < n_sel) s_sel[threadIdx.x] = sel[threadIdx.x];
    __syncthreads();
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= n_pixels) return;
    double sum = 0.0;
    for (int l = 0; l < layers; ++l) {
        const int id = layer_id[(size_t)l * n_pixels + pix];
        if (id < 0) continue;
        bool in = false;
        for (int s = 0; s < n_sel; ++s) in = in || s_sel[s] == id;  // (one LDS word for the whole wave: a broadcast)
        if (in) sum = sum + (double)layer_coverage[(size_t)l * n_pixels + pix];
    }
    matte[pix] = (float)(sum < 1.0 ? sum : 1.0);
}

// rtm_composite: premultiplied "over" per channel in float, out = color + (1 - alpha) * B, and its quantised bytes
// (rtm_quantise of (double)out: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0).  color and out32 may
// be one buffer: a thread reads its pixel before it writes it.
__global__ __launch_bounds__(256) void composite_kernel(const size_t n_pixels, const float* color,
                                                        const float* __restrict__ alpha, const float* __restrict__ background,
                                                        const float b0, const float b1, const float b2, float* out32,
                                                        uint8_t* __restrict__ out8) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= n_pixels) return;
    const float t = 1.0f - alpha[pix];
    const float bg[3] = {background ? background[pix * 3] : b0, background ? background[pix * 3 + 1] : b1,
                         background ? background[pix * 3 + 2] : b2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = color[pix * 3 + c] + t * bg[c];
        if (out32) out32[pix * 3 + c] = v;
        if (out8) {
            const double d = (double)v, q = 255 * ((1.0 < d) ? 1.0 : d);
            out8[pix * 3 + c] = (q >= 0.0 && q < 256.0) ? (uint8_t)q : (uint8_t)0;
        }
    }
}

}  // namespace rtm
#endif
