// rtm_render_kernel.h — the hot kernel of the RaytracingMin path on gfx950 (render_tiles_kernel) and the second half of
// its sample split (split_finalize_kernel).  Included by rtm_kernels.hip, which holds the host side (scene lifetime,
// per-stream contexts, variant selection, launches).
//
// Path (reference file:line): Renderer::Render's pixel/sample loop src/Renderer.cpp:215-250, png::PathTracing
// src/Renderer.cpp:57-117 (through rtm_path.h), the per-sample normalise + clamp + accumulate src/Renderer.cpp:240-248,
// the quantiser src/Renderer.cpp:251-254.
#pragma once
#include <type_traits>

#include "rtm_path.h"

namespace RTM_NS {

struct RenderParams {
    SceneView scene;
    int W, H, S, SS;
    int row_begin, row_end;
    int band_count, band_index;  // interleaved 8-row bands (rtm_options); 1, 0 = every band
    int tiles_x;
    int mode, max_bounces;
    unsigned total_samples;  // SS*SS*S per pixel: the frame's N (the divisors below are the frame's, whatever the pass)
    // this call's samples [sample_begin, sample_end) of every pixel (rtm_render_scene_samples; [0, N) for a whole frame);
    // seeded: every accumulator starts from the value out64 holds (a pass that continues a frame), else from +0
    unsigned sample_begin, sample_end, seeded;
    double preview_scale;    // N / sample_end: the f32 / u8 views of a pass that ends before N
    float rate;             // 1.0 / (1 + SS) as float, src/Renderer.cpp:227
    double dSS, dS;          // divisors of src/Renderer.cpp:240
    double inv_ss, inv_s;    // exact reciprocals when SS and S are powers of two, else 0
    D3 cam_org, ax, by, cz;  // origin, camX*fovx, camY*fovy, camZ (src/Renderer.cpp:202-208)
    uint64_t seed_mult;
    double* __restrict__ out64;
    float* __restrict__ out32;
    uint8_t* __restrict__ out8;
    unsigned long long* __restrict__ counters;  // casts, bounces, draws, overflow flag
    // deep-path record pool (only when a path may run deeper than the LDS record stack)
    unsigned char* __restrict__ pool;       // pool_slots x kPoolLevels records
    unsigned* __restrict__ pool_next;       // bump allocator
    unsigned pool_slots;
    unsigned long long* __restrict__ stamps;  // STAMP builds: per block {nearest, shade, end, iterations}
    // sample split (SPLIT kernels): `split` waves per tile; wave 0 traces samples [0, split_head), wave f >= 1
    // samples [split_head + (f-1)*split_len, split_head + f*split_len)
    // Tiles [0, split_first) are NOT split (one wave traces all their samples and stores the pixel itself): a
    // long launch splits only its last tiles, whose short waves fill the SIMDs that the last whole tiles leave
    // idle one after another.  n_tiles counts the split tiles; their blocks follow the whole tiles' in the grid.
    unsigned n_tiles, split, split_head, split_len, split_first;
    double* __restrict__ partial;  // [tile][3][64]: accumulator of wave 0 after its split_head samples
    // per-sample terms of waves 1..: one block of split_len rows per (tile, small wave), a row = 64 terms in the order
    // the wave FOLDED them ([3][64] doubles, whole lines from one store instruction) + 64 tags (owner lane, sample)
    unsigned char* __restrict__ contrib;
    // ... and how many terms each small wave stored, [tile][small wave]: a path end that provably adds (+0, +0, +0) is not
    // stored (SceneView::emit_mask), so the count is no longer split_len x the tile's valid pixels
    unsigned* __restrict__ split_counts;
    // in-wave sample stealing (STEAL kernels, whole tiles): per tile a block of kStealHdrBytes (terms stored, every
    // pixel's final own-sample end) + 3 x 64 doubles (the accumulators) + steal_rows rows of kStealRowBytes (64 terms in
    // fold order + 64 four-byte tags (pixel lane, sample)); steal_finalize_kernel turns the block into pixels
    unsigned char* __restrict__ steal_ws;
    unsigned steal_rows, steal_depth;  // capacity in rows per tile; how far below the last sample a pixel may be stolen from
    unsigned magic_S, magic_SS;        // floor(2^32 / d) + 1: x / d == umulhi(x, magic) for x, d < 2^16 (a stolen sample's sub-pixel)
    // grid kernel (rtm_grid_kernel.h): blocks are dealt round-robin to the 8 XCDs, each with its own L2; with xcd_on, block
    // b of a launch renders its tile (b % 8) * xcd_q + min(b % 8, xcd_rem) + b / 8, so that an XCD's blocks cover one
    // contiguous part of the frame and its L2 holds that part's cells (xcd_q = tiles / 8, xcd_rem = tiles % 8)
    unsigned xcd_on, xcd_q, xcd_rem;
    // the launch's LDS holds the near-unit Normalize table behind the sincos constants (rtm_device.h; set by the launcher
    // where the 256 bytes do not cost a wave per CU: unit_table_fits)
    unsigned unit_tab;
    // the tolerance translation unit (RTM_TOL): per tile of the launch 64 words — bit s of word p: "sub-pixel s of pixel p
    // has a primary ray whose nearest hit last-bit differences could change" (prim_prepass_kernel); null elsewhere
    const unsigned long long* __restrict__ prim_masks;
    // ... and, from the same pre-pass, every sub-pixel's primary direction ([tile][pixel][sub-pixel][component] doubles):
    // a lane that moves on to its next sub-pixel LOADS its direction instead of running the five correctly rounded
    // divisions of src/Renderer.cpp:228-232 alone in its wave (some lane of a wave does about every 4.4 trips: 4 % of the
    // frame).  Null: the directions are computed where they are needed, as before.
    const double* __restrict__ prim_dirs;
    // grid kernel: one bit per (tile, sample, pixel) of the launch — "this sample's term is not all zeros and was stored";
    // zeroed before the launch, set with atomicOr, read by grid_finalize_kernel.  A term of (+-0, +-0, +-0) changes no sum
    // it is added to (the accumulator starts at +0 and no term is negative zero's only partner), so it is neither stored nor
    // read: 94 % of the samples of BASELINE configs[4] (a path that reaches no emitter returns 0).
    unsigned* __restrict__ nz_bits;
    // tile-list renders (rtm_render_scene_tiles): launch-local tile t renders frame tile tile_map[t] (tx = % tiles_x, ty =
    // / tiles_x); an entry of frame_tiles or more makes its blocks return before any load or store.  Null: tile t is frame
    // tile t (every other call).  The work buffers above stay indexed by launch-local tile.
    const unsigned* __restrict__ tile_map;
    unsigned frame_tiles;
};
constexpr size_t kTermRowBytes = 3 * 64 * sizeof(double) + 64 * sizeof(unsigned short);  // 1664 = 13 lines of 128 B
constexpr size_t kStealRowBytes = 3 * 64 * sizeof(double) + 64 * sizeof(unsigned);       // 1792 = 14 lines of 128 B
constexpr size_t kStealHdrBytes = 256;                                                    // unsigned n_terms; ...; u16 end[64] at +128
__host__ __device__ inline size_t steal_tile_bytes(unsigned rows) { return kStealHdrBytes + 3 * 64 * sizeof(double) + (size_t)rows * kStealRowBytes; }

__device__ __forceinline__ unsigned long long stamp_now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

constexpr int kPoolLevels = 960;  // records per pool slot beyond the LDS levels

// Per-lane stack of hit records: the first LDS_D levels live in LDS ([depth][lane]); a lane whose
// path runs deeper takes, once, a slot of kPoolLevels records from a global pool.  Exhausting the
// pool or the slot raises the overflow flag and the call fails with RTM_ERR_UNSUPPORTED.
template <typename RecT, int LDS_D>
struct RecordStack {
    RecT* lds;  // this wave's [LDS_D][64]
    int lane;
    const RenderParams* P;
    int slot = -1;
    bool overflow = false;
    __device__ __forceinline__ RecT* slot_ptr() {
        if (slot < 0) {
            const unsigned got = P->pool ? atomicAdd(P->pool_next, 1u) : 0xFFFFFFFFu;
            if (got >= P->pool_slots) {
                overflow = true;
                return nullptr;
            }
            slot = (int)got;
        }
        return reinterpret_cast<RecT*>(P->pool) + (size_t)slot * kPoolLevels;
    }
    __device__ __forceinline__ void push(int d, int id) {
        if (d < LDS_D) {
            lds[d * 64 + lane] = (RecT)id;
        } else if (d - LDS_D < kPoolLevels) {
            if (RecT* p = slot_ptr()) p[d - LDS_D] = (RecT)id;
        } else {
            overflow = true;
        }
    }
    __device__ __forceinline__ int pop(int d) {
        if (d < LDS_D) return (int)lds[d * 64 + lane];
        if (slot < 0 || d - LDS_D >= kPoolLevels) return 0;  // only after an overflow: image is discarded
        return (int)(reinterpret_cast<const RecT*>(P->pool) + (size_t)slot * kPoolLevels)[d - LDS_D];
    }
    static constexpr int kCapacity = LDS_D + kPoolLevels;
};

constexpr size_t kUnitTableBytes = (size_t)(kShadeConstCount - kTrigConstCount) * sizeof(double);  // rtm_device.h: the near-unit Normalize table
// Does a launch whose workgroups (one wave each) take `lds` bytes keep its waves per CU with the near-unit Normalize table's
// 256 bytes on top?  160 KB of LDS per CU, at most 16 waves (4 per SIMD at the kernels' 128 registers).
inline bool unit_table_fits(size_t lds) {
    auto waves = [](size_t b) { const size_t w = b ? (size_t)163840 / b : 16; return w > 16 ? (size_t)16 : w; };
    return waves(lds) == waves(lds + kUnitTableBytes);
}
// LDS copy of the scene tables: n geometry rows (4 doubles) + n+1 material rows (8 doubles, the last
// one is the identity row) + n normal-length rows (3 doubles: |hit - centre| as Magnitude returns it, its refined
// reciprocal, and the float r*r in the low word of the third)
// rows: the tolerance unit's axis-signature kernels keep geometry, normal row and kd * 2^24 of a sphere in one 8-double row
// (rtm_path.h: SceneLdsRows) — 8 bytes per sphere more
__host__ __device__ inline size_t lds_table_bytes(int n, bool rows) {
    return ((size_t)n * (rows ? 8 : 7) + ((size_t)n + 1) * 8) * sizeof(double);
}
// Which instantiations take the row layout: the tolerance unit's axis-signature kernels (UNROLL <= -1000: exactly 7 spheres,
// the headline kernel among them).  Tried for every table kernel and not kept elsewhere (profiles/r11/trip_slots.md): the exact
// unit's -105 .. -107 kernels went from 24 to 40 bytes of scratch and the tolerance unit's generic n < 8 kernel from 8 to 16; the
// chunked kernel (UNROLL 8) serves 8 .. 256 spheres, where 8 bytes a sphere more cost its any-depth tolerance shape a wave per CU
// at 22 and 23 spheres and the near-unit table at 24.
constexpr bool lds_rows_for(int unroll) { return RTM_TOL != 0 && unroll <= -1000; }

// src/Renderer.cpp:227-232; sx, sy in 1..SS
__device__ __forceinline__ D3 primary_dir(const RenderParams& P, int x, int y, int sx, int sy) {
    const double px = 2.0 * ((double)x + (double)(P.rate * (float)sx)) / P.W - 1.0;
    const double py = 2.0 * ((double)y + (double)(P.rate * (float)sy)) / P.H - 1.0;
    return normalize((P.ax * px + P.by * py) + P.cz);
}

// The same, with the nine camera-basis doubles read from an LDS block (cam[0..8] = ax, by, cz).  The
// block is read once per sub-pixel; keeping those doubles in registers across the render loop made
// hipcc spill them to scratch per lane (200 MB of stray HBM writes per 1080p frame).
__device__ __forceinline__ D3 primary_dir_lds(const RenderParams& P, const double* cam, int x, int y, int sx,
                                              int sy) {
#if RTM_TOL
    // the tolerance translation unit: the primary ray stays the reference's bit for bit (separately rounded multiplies and
    // adds, true divisions) — once per S samples, and what rtm_path.h: nearest_hit_exactfp settles exact ties on
#pragma clang fp contract(off)
    const double px = 2.0 * ((double)x + (double)(P.rate * (float)sx)) / P.W - 1.0;
    const double py = 2.0 * ((double)y + (double)(P.rate * (float)sy)) / P.H - 1.0;
    const double vx = (cam[0] * px + cam[3] * py) + cam[6];
    const double vy = (cam[1] * px + cam[4] * py) + cam[7];
    const double vz = (cam[2] * px + cam[5] * py) + cam[8];
    const float len2 = (float)(vx * vx + vy * vy + vz * vz);  // src/Ray.h:67-69
    const double m = (double)__builtin_sqrtf(len2);
    return D3{vx / m, vy / m, vz / m};                          // src/Ray.h:70-72
#else
    int w = P.W, h = P.H;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(w), "+s"(h));  // (opaque: their conversions to double are not worth a register pair each across the render loop)
#endif
    const double px = 2.0 * ((double)x + (double)(P.rate * (float)sx)) / w - 1.0;
    const double py = 2.0 * ((double)y + (double)(P.rate * (float)sy)) / h - 1.0;
    const D3 ax = d3(cam[0], cam[1], cam[2]), by = d3(cam[3], cam[4], cam[5]), cz = d3(cam[6], cam[7], cam[8]);
    return normalize((ax * px + by * py) + cz);
#endif
}

__device__ __forceinline__ void wave_add_counter(unsigned long long* dst, unsigned v) {
    unsigned long long s = v;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(dst, s);
}

// src/Renderer.cpp:246-254: image[] += acc; optional float3 / 8-bit views of the same pixel
// Image row of row `sub` (0..7) of this call's band `local_band`: the call renders bands
// band_index, band_index + band_count, ... of [row_begin, row_end) and stores them back to back.
__device__ __forceinline__ int band_row(const RenderParams& P, int local_band, int sub) {
    return P.row_begin + (local_band * P.band_count + P.band_index) * 8 + sub;
}

// The frame tile that launch-local tile t renders (RenderParams::tile_map); ~0u: a list entry past the frame.  Every
// tile -> (x, y) mapping of the render kernels goes through here (render_tiles_kernel through the LDS slot it fills from it).
__device__ __forceinline__ unsigned frame_tile(const RenderParams& P, unsigned t) {
    if (P.tile_map == nullptr) return t;
    const unsigned m = P.tile_map[t];
    return m < P.frame_tiles ? m : ~0u;
}

__device__ __forceinline__ size_t out_index(const RenderParams& P, int x, int y) {
    const int rel = y - P.row_begin;
    const int out_row = (P.band_count > 1) ? ((rel >> 3) / P.band_count) * 8 + (rel & 7) : rel;
    return ((size_t)out_row * P.W + x) * 3;
}

// The value a pixel's accumulator starts from: what the previous pass of the frame left in out64 (never -0: it went
// +0 -> +t0 -> ..., so continuing the fold from it is the one-shot fold), or +0
__device__ __forceinline__ D3 seed_of(const RenderParams& P, bool valid, int x, int y) {
    if (!P.seeded || !valid) return d3(0, 0, 0);
    const size_t o = out_index(P, x, y);
    return d3(P.out64[o], P.out64[o + 1], P.out64[o + 2]);
}

__device__ __forceinline__ void store_pixel(const RenderParams& P, bool valid, int x, int y, D3 acc) {
    if (!valid) return;
    const size_t o = out_index(P, x, y);
    double r = 0.0 + acc.x, g = 0.0 + acc.y, b = 0.0 + acc.z;  // :246-248
    if (P.out64) {
        P.out64[o] = r;
        P.out64[o + 1] = g;
        P.out64[o + 2] = b;
    }
    if (P.sample_end != P.total_samples) {  // a pass before the last: the views preview the frame (wave-uniform)
        r *= P.preview_scale;
        g *= P.preview_scale;
        b *= P.preview_scale;
    }
    if (P.out32) {
        P.out32[o] = (float)r;
        P.out32[o + 1] = (float)g;
        P.out32[o + 2] = (float)b;
    }
    if (P.out8) {  // :253: (unsigned char)255 * std::min(v, 1.0), truncation
        const double q[3] = {r, g, b};
        for (int c = 0; c < 3; ++c) {
            const double v = 255 * ((1.0 < q[c]) ? 1.0 : q[c]);
            P.out8[o + c] = (v >= 0.0 && v < 256.0) ? (uint8_t)v : (uint8_t)0;
        }
    }
}

// Does a path that ended on object `hit_id` (-1: a miss, the identity row) take an entry of the fold queue?  Not
// where the host has proven that its term is (+0, +0, +0): SceneView::emit_mask (all ones without the proof; ids from 64 up
// only occur then).  Skipping such an end is invisible because x + (+0) == x for every x but -0, and a -0 accumulator — only
// a seeded pass could start from one: a caller's out64 holding -0 — is stored as 0.0 + acc = +0 by store_pixel whether +0 was
// added to it or not, and gives t either way once a non-zero t is added.  That covers every entry point that seeds
// (rtm_render_scene_samples, tile lists, the adaptive render's passes); the head wave's partial and a stealing tile's
// accumulators reach store_pixel through the finalize kernels.
// Two vector instructions (round 6; eight before): the mask is bit-reversed (scalar), so that shifting it LEFT by the id brings
// the object's bit to the sign bit, and the test is one signed compare that yields the lane mask.  The raw hit id serves
// as it is: a 64-bit shift takes its low six bits, so a miss (-1) asks for bit 63 — never set under the proof (at most 63
// objects: bits 0..62), set without it, which is the identity row's answer in both cases; ids from 64 up only meet all ones.
__device__ __forceinline__ bool zero_term_queued(const SceneView& v, const int hit_id) {
    const unsigned long long reversed = __builtin_bitreverse64(v.emit_mask);
    int hi = (int)((reversed << ((unsigned)hit_id & 63u)) >> 32);
    asm("" : "+v"(hi));  // (opaque: the compare is of the high word alone, not a 64-bit one)
    return hi < 0;
}

// ------------------------------------------------------------------------------------------------
// Shape flags of the render kernel (its template parameter F)
constexpr unsigned kLdsTab = 1u << 0, kPark = 1u << 1, kStamp = 1u << 2, kPack8 = 1u << 3, kSplit = 1u << 4;
constexpr unsigned kDefer = 1u << 5, kPackL = 1u << 6, kReuse = 1u << 7, kPlanes = 1u << 8, kSteal = 1u << 9;

// The render kernel, render_tiles_kernel<M, F, UNROLL, RecT, LDS_D, WPE>.
//   M       Math policy (rtm_path.h)
//   F       the shape: an OR of the flags below (the kernel body reads them as the bools LDS_TAB, PARK, ...)
//   UNROLL  spheres whose geometry is fetched together (wave-uniform loads)
//   RecT    hit-record type (u8 when n_spheres <= 256), LDS_D: record depth staged in LDS per lane
//   WPE     launch bound: waves per SIMD
// Dynamic LDS layout (16-byte aligned base): [geom n*4 doubles][mat (n+1)*8][norm n*3] (kLdsTab; lds_rows_for(UNROLL), the
// tolerance unit's axis-signature kernels: [rows n*8][mat (n+1)*8], rtm_path.h: SceneLdsRows), [camera 10]
// [sincos constants 16][accumulator + primary direction 6 x 64] (kPark), then the record stack
// [LDS_D][64] or the fold queue (kDefer).  render_lds_bytes, just above the kernel, is a launch's size of it.
//   kLdsTab scene tables (centres + materials) copied to LDS for the per-lane look-ups
//   kPark   the pixel accumulator and the cached primary direction live in LDS ([component][lane]),
//           not in VGPRs: they are touched once per sample, and the 12 registers they would pin
//           are what the unrolled sphere chunk needs to stay under 128 VGPRs without scratch spills
//   kStamp  diagnostic build: s_memtime around the three segments of an iteration (never timed itself)
//   kPack8  max_bounces <= 8 and n < 256: hit records packed in a 64-bit register, no LDS stack
//   kSplit  P.split waves per tile, each tracing a contiguous range of the pixel's samples.  Wave 0
//           accumulates as usual and leaves its accumulator in P.partial; the others store every
//           sample's term (src/Renderer.cpp:240-242, after the clamp) to P.contrib, and
//           split_finalize_kernel adds them IN THE REFERENCE'S ORDER, so the image does not change by
//           a bit.  Used when a strip has too few tiles to keep every SIMD busy to the end (few rows
//           per GPU, small images): the launch's tail is then the spread of per-tile cost.
//   kDefer  (with kPack8 + kPark) path ends are queued and folded 64 at a time.  The fold, the /SS/SS/S and
//           the clamp of a finished path are a pure function of its hit ids, but only ~22 % of the
//           lanes finish a path in a given iteration, so doing that work on the spot runs ~100
//           instructions with a fifth of the lanes (13 % of the frame, measured).  Instead the ending
//           lanes append (records, terminal id) to a wave-shared ring in LDS and start their next
//           sample at once; whenever 64 entries are waiting, all 64 lanes fold one entry each and leave
//           the term in LDS, and every owner then adds its terms to its accumulator in the order its
//           paths ended (a per-lane FIFO of ring positions keeps that order) — the accumulation order
//           of src/Renderer.cpp:241-242 is untouched.
//   kPackL  (with kDefer) packed records for paths of ANY depth (max_bounces < 0 or > 8): level d in byte
//           d & 7 of word d >> 3 — word 0 in a register, word 1 in LDS per lane, levels from 16 up (about
//           kd^16 of the paths) in the pooled global stack.  A queue entry carries both words and the pool
//           slot; a lane that queues a path deeper than 16 forces a pass, so its slot is free again
//           before its next path can reach level 16.
//   kReuse  (with kDefer + kPack8; variant 15, a SEPARATELY LABELLED row, never the default) the S samples of a
//           sub-pixel share one primary ray (no jitter, src/Renderer.cpp:224-232), so its nearest hit is computed
//           once per sub-pixel and reused: a lane whose path ended restarts at "primary hit known" in the SAME
//           trip and joins the shading block with the lanes that bounced.  Every trip is then one nearest-hit
//           search and one bounce for every lane (no idle lanes in either block) and a sample costs C - 1 trips
//           instead of C.  Same image, same counters (a reused primary hit still counts as the cast the reference
//           performs); different work per sample than the reference, hence the label.
constexpr int kFoldRing = 128;  // entries of the ring: < 64 waiting + <= 64 appended per iteration
constexpr size_t kFoldQueueBytes = kFoldRing * 16 + 3 * 64 * 8 + 64 * 8 + 64 * 4;  // the FIFO form: ring, terms, FIFO, counts
// kScatter kernels (every deferred-fold kernel but the primary-hit-reuse row): no staged terms, no FIFO — ring, the pixels'
// counts of added entries (a small wave's tags in their place), the lanes' counts: 1 792 bytes less per wave, which is what lets
// the any-depth kernels keep the near-unit Normalize table at 16 waves per CU
constexpr size_t kFoldQueueBytesS = kFoldRing * 16 + 64 * 4 + 64 * 4;
constexpr size_t kFoldQueueBytesLS = kFoldQueueBytesS + kFoldRing * 8 + 64 * 8;
// (kSplit: a small wave's ring entries carry a 2-byte tag (owner lane, sample).  The tags live in the per-lane FIFO array,
// which a small wave does not use: 256 of its 512 bytes.  A separate array put the any-depth kernel at 10 328 bytes of LDS per
// wave — 15 instead of 16 waves per CU, 5 % on every unlimited-depth frame, profiles/r3/ab_r2_vs_r3.txt.)

//   kSteal  (with kDefer + kPack8) in-wave sample stealing for WHOLE tiles.  All 64 lanes of a wave trace the same number of
//           samples but not the same number of casts, so a wave runs until its slowest lane is done: 4.4 % of the lane-trips
//           of the headline frame are spent by lanes that have finished (8.9 % at 256 spp, 15 % at 64 spp:
//           profiles/r3/ragged_end.txt).  When the first lane runs out of samples the wave leaves the main loop for a
//           TAIL loop in which a lane without own samples takes the LAST unstarted sample of the pixel that has most left
//           (wave-uniform choice, no atomics: one victim per trip), traces it — the RNG is keyed by (pixel, sample) — and
//           leaves its clamped term, tagged (pixel, sample), in the tile's row buffer in HBM; a pixel's own lane
//           accumulates samples [0, end) in order as before, and steal_finalize_kernel adds the stolen terms [end, total)
//           in order on top.  Only the ORDER of the additions is observable, and it is the reference's.
//   kPlanes (with kLdsTab) the scene holds png::PlaneObject entries: SceneLdsObjects / object_chunk / MathSpecZ
//           (rtm_path.h) — a plane's test in its index slot of the chunk, its normal from the LDS table

// The dynamic LDS bytes of a render_tiles_kernel launch of shape F for a scene of n objects, `pad` bytes on top (the
// RTM_DEBUG_LDS_PAD knob): the carve-up at the top of the kernel, term by term.  *unit_tab: the launch holds the near-unit
// Normalize table too (where its bytes do not cost a wave per CU: unit_table_fits) — RenderParams::unit_tab.
template <unsigned F, typename RecT, int LDS_D>
inline size_t render_lds_bytes(int n, bool rows, size_t pad, unsigned* unit_tab) {
    size_t b = (F & kLdsTab) ? lds_table_bytes(n, rows) : 0;  // scene tables
    b += (10 + kTrigConstCount) * sizeof(double);        // camera, sincos constants
    if (F & kPark) b += 6 * 64 * sizeof(double);         // accumulator + primary direction
    if (!(F & (kPack8 | kPackL))) b += (size_t)LDS_D * 64 * sizeof(RecT);  // record stack: unpacked records only
    if (F & kDefer) b += (F & kReuse) ? kFoldQueueBytes : (F & kPackL) ? kFoldQueueBytesLS : kFoldQueueBytesS;
    // every pixel's next own sample and own-sample end; the tolerance unit's primary-ray masks
    if (F & kSteal) b += 2 * 64 * sizeof(unsigned) + (RTM_TOL ? 64 * sizeof(unsigned long long) : 0);
    b += pad;
    *unit_tab = unit_table_fits(b) ? 1u : 0u;
    return b + (*unit_tab ? kUnitTableBytes : 0);
}

template <class M, unsigned F, int UNROLL, typename RecT, int LDS_D, int WPE>
__global__ __launch_bounds__(64, WPE) void render_tiles_kernel(const RenderParams P) {
    constexpr bool LDS_TAB = (F & kLdsTab) != 0, PARK = (F & kPark) != 0, STAMP = (F & kStamp) != 0;
    constexpr bool PACK8 = (F & kPack8) != 0, SPLIT = (F & kSplit) != 0, DEFER = (F & kDefer) != 0;
    constexpr bool PACKL = (F & kPackL) != 0, REUSE = (F & kReuse) != 0, PLANES = (F & kPlanes) != 0;
    constexpr bool STEAL = (F & kSteal) != 0;
    static_assert(!STEAL || (DEFER && PACK8 && !REUSE && !PACKL), "sample stealing rides on the deferred fold with packed records");
    static_assert(!PLANES || (LDS_TAB && !REUSE), "plane scenes ride on the LDS tables");
    static_assert(!SPLIT || DEFER, "the sample split's small waves store their terms from the fold queue");
    static_assert(!DEFER || ((PACK8 || PACKL) && PARK && !STAMP), "the fold queue rides on packed records and the LDS accumulator");
    static_assert(!REUSE || (DEFER && PACK8 && !SPLIT), "primary-hit reuse rides on the deferred fold with packed records");
    static_assert(!PACKL || (DEFER && !PACK8 && LDS_D == 0 && sizeof(RecT) == 1), "PACKL: deferred fold, byte records, pooled stack only");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x;
    // this block's tile of the launch, and the frame tile it renders (a tile-list render: a bad entry returns here)
    const unsigned block_tile = (SPLIT && blockIdx.x >= P.split_first) ? P.split_first + (blockIdx.x - P.split_first) % P.n_tiles
                                                                        : blockIdx.x;
    const unsigned block_frame_tile = frame_tile(P, block_tile);
    if (block_frame_tile == ~0u) return;
    // The exact-n instantiations (UNROLL in -101 .. -107, or an axis signature: UNROLL <= -1000) are launched for scenes of
    // exactly that many spheres, so the count COULD be a compile-time constant there (the LDS tables' offsets, the identity
    // row's index and the empty record word as immediates).  Measured and not kept (profiles/r4/ctn_ab.txt): the
    // tolerance row does not move, the exact kernel loses 3 %.
    const int scene_n = P.scene.n;
    // ... and the index an empty record word is filled with: for the tolerance unit's axis-signature instantiations the sphere
    // count their UNROLL encodes (rtm_path.h: axis_unroll; launched for exactly that count) — the word is then a constant of
    // the code where the render loop restarts a path, not a spilled scalar pair read back.  For this word only (round 4: the
    // count as a constant everywhere was worth nothing or a loss).
    // Not for the any-depth kernel with the sample split: it pays for either of round 13's two items with 12 bytes of scratch
    // that its parent does not have (-Rpass-analysis=kernel-resource-usage; profiles/r13/merged_mix.md), like kPairsShape.
    constexpr bool kAxisTolShape = RTM_TOL != 0 && UNROLL <= -1000 && (F & (kPackL | kSplit)) != (kPackL | kSplit);
    [[maybe_unused]] const int empty_n = kAxisTolShape ? axis_unroll_n(UNROLL) : scene_n;
    constexpr bool kRowTab = LDS_TAB && lds_rows_for(UNROLL);  // one row per sphere: SceneLdsRows
    static_assert(!(kRowTab && PLANES), "a plane's normal has no place in a sphere's row");
    double* lgeom = reinterpret_cast<double*>(lds_raw);  // (kRowTab: the rows)
    double* lmat = lgeom + (LDS_TAB ? scene_n * (kRowTab ? kLdsRowDoubles : 4) : 0);
    [[maybe_unused]] double* lnrm = lmat + (LDS_TAB ? (scene_n + 1) * 8 : 0);
    double* cam = reinterpret_cast<double*>(lds_raw + (LDS_TAB ? lds_table_bytes(scene_n, kRowTab) : 0));
    double* trig = cam + 10;                 // 9 camera doubles + pad
    // the shading constants: sincos and — where the launcher found the LDS for it — the near-unit Normalize table
    // wave-uniform; the axis-signature instantiations are launched only when the table is there (the launchers check), so it is
    // a compile-time constant for them
    const bool unit_tab = UNROLL <= -1000 ? true : (P.unit_tab != 0u);
    double* park = trig + (unit_tab ? kShadeConstCount : kTrigConstCount);
#if RTM_TOL
    ShadeLds shade_lds_tab(trig, unit_tab);
    shade_lds_tab.tab = g_trig_tab;
    const ShadeLds shade_lds = shade_lds_tab;
#else
    const ShadeLds shade_lds(trig, unit_tab);
#endif
    RecT* rec = reinterpret_cast<RecT*>(park + (PARK ? 6 * 64 : 0));
    // DEFER: [ring 128 x uint4][terms 3 x 64 doubles][per-lane FIFO of ring positions][per-lane count]; kScatter (below):
    // [ring][per pixel: entries added so far, 64 words — a small wave's 128 two-byte tags in their place][per-lane count]
    constexpr bool kScatter = DEFER && (PACK8 || PACKL) && !REUSE;
    uint4* fq_in = reinterpret_cast<uint4*>(park + 6 * 64);
    double* fq_out = reinterpret_cast<double*>(fq_in + kFoldRing);  // (the FIFO form only)
    unsigned long long* fq_fifo = kScatter ? reinterpret_cast<unsigned long long*>(fq_in + kFoldRing)
                                           : reinterpret_cast<unsigned long long*>(fq_out + 3 * 64);
    unsigned* fq_pend = kScatter ? reinterpret_cast<unsigned*>(fq_fifo) + 64 : reinterpret_cast<unsigned*>(fq_fifo + 64);
    unsigned long long* fq_in1 = reinterpret_cast<unsigned long long*>(fq_pend + 64);  // PACKL: word 1 of the entries
    unsigned long long* rec_w1 = fq_in1 + kFoldRing;                                   // PACKL: word 1 of the lanes
    // SPLIT, small waves only: tag of every ring entry, in the FIFO array they have no other use for
    unsigned short* fq_tag = reinterpret_cast<unsigned short*>(fq_fifo);
    static_assert(kFoldRing * sizeof(unsigned short) <= 64 * sizeof(unsigned), "the tags fit the FIFO array, and the counts' that takes its place");
    // Who adds a folded term to its pixel (fold_pass).  Round 1's form: the OWNER finds its entries through a per-lane FIFO of
    // ring positions and reads the terms back from LDS — as many rounds as the busiest pixel has entries in the pass, each with
    // the FIFO's decoding (23 vector instructions and 10 LDS operations a round, ~4.5 rounds a pass).  kScatter (round 4, the
    // packed-record kernels): the entry carries (owner lane, the owner's running count of path ends) and the FOLDING lane adds
    // its term to the owner's accumulator itself, in the round that is the entry's turn — rank = count - the owner's count of
    // entries already added (fq_done) — straight from its registers: a compare, three LDS read-add-writes and the count per
    // round, no FIFO, no term staging, and no forced passes (a FIFO held 8 positions).  The order of a pixel's additions is the
    // order of its path ends either way.
    // (PACKL, the any-depth kernels: owner and count ride in the entry's third word above term id and depth, and the lane's
    // "may a deep entry of mine still be waiting" is the count it had after its last deep path against fq_done — fq_pend bits
    // 8..15 and 16)
    unsigned* fq_done = reinterpret_cast<unsigned*>(fq_fifo);  // kScatter: per lane, entries of its pixel added so far (the FIFO's place)
    if constexpr (DEFER) fq_pend[lane] = 0u;  // entries waiting (FIFO form) / path ends so far (kScatter)
    if constexpr (kScatter) fq_done[lane] = 0u;
    if constexpr (PACKL) rec_w1[lane] = packed8_empty(scene_n);
    fill_shade_consts(trig, lane, unit_tab);
    if (lane < 9) {
        const double v9[9] = {P.ax.x, P.ax.y, P.ax.z, P.by.x, P.by.y, P.by.z, P.cz.x, P.cz.y, P.cz.z};
        double pick = v9[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) pick = (lane == k) ? v9[k] : pick;
        cam[lane] = pick;
    }
    {  // the spare slot: word 0 this tile's first entry of the pre-pass's direction table (primary_of below; the table holds
       // at most 4 GiB / 1.5 KiB entries), word 1 the frame tile the block renders (pixel_xy)
        const unsigned first = block_tile * (unsigned)(P.SS * P.SS);
        const double slot = __longlong_as_double((long long)(((unsigned long long)block_frame_tile << 32) | first));
        if (lane == 9) cam[9] = slot;
    }
    __syncthreads();
    if constexpr (LDS_TAB) {
        const double* gsrc = reinterpret_cast<const double*>(P.scene.geom);
        for (int i = lane; i < scene_n * 4; i += 64) lgeom[kRowTab ? (i >> 2) * kLdsRowDoubles + (i & 3) : i] = gsrc[i];
        for (int i = lane; i < (scene_n + 1) * 8; i += 64) lmat[i] = P.scene.mat[i];
        for (int i = lane; i < scene_n; i += 64) {
            if constexpr (kRowTab) {
                fill_norm_row(lgeom + i * kLdsRowDoubles + 4, gsrc[i * 4 + 3]);
                lgeom[i * kLdsRowDoubles + 7] = P.scene.mat[i * 8 + 7];
                continue;
            }
            if (PLANES && gsrc[i * 4 + 3] < 0.0) {  // a plane's row: its normal (SceneLdsObjects::plane_normal)
                lnrm[i * 3] = P.scene.plane[(size_t)i * 16 + 3];
                lnrm[i * 3 + 1] = P.scene.plane[(size_t)i * 16 + 4];
                lnrm[i * 3 + 2] = P.scene.plane[(size_t)i * 16 + 5];
                continue;
            }
            fill_norm_row(lnrm + i * 3, gsrc[i * 4 + 3]);
        }
        __syncthreads();  // one wave per block: orders the LDS writes before the reads
    }
    using SceneTab = typename std::conditional<kRowTab, SceneLdsRows, SceneLds>::type;
    using Scene = typename std::conditional<PLANES, SceneLdsObjects,
                                            typename std::conditional<LDS_TAB, SceneTab, SceneGlobal>::type>::type;
    Scene sc;
    sc.v = P.scene;
    sc.v.n = scene_n;
    // The axis-signature instantiations (UNROLL <= -1000) are launched for RTM_MODE_REPAIRED only: the mode is a compile-time
    // constant there (the shading block's "literal mode: the normal stays 0" arm and its wave-uniform test go away; a literal-mode
    // render of such a scene takes the plain exact-n kernel)
    const int mode = UNROLL <= -1000 ? (int)RTM_MODE_REPAIRED : P.mode;
    if constexpr (kRowTab) {
        sc.lrow = lgeom;
        sc.lmat = lmat;
    } else if constexpr (LDS_TAB) {
        sc.lgeom = lgeom;
        sc.lmat = lmat;
        sc.lnrm = lnrm;
    }

    // Pixel coordinates are recomputed where they are needed (sub-pixel change, final store) from an
    // opaque copy of the lane id, so that nothing derived from them stays live across the render loop.
    auto pixel_xy = [&](int& px, int& py) {
        int l = lane;
        asm volatile("" : "+v"(l));
        const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<const unsigned*>(cam + 9)[1]);
        const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
        px = tx * 8 + (l & 7);
        py = band_row(P, ty, l >> 3);
    };
    int x, y;
    pixel_xy(x, y);
    const bool valid = (x < P.W) && (y < P.row_end);
    const uint32_t pixel = (uint32_t)y * (uint32_t)P.W + (uint32_t)x;  // GLOBAL pixel index

    PathCounters pc = {0, 0, 0};
    RecordStack<RecT, LDS_D> stack{rec, lane, &P};
    // The tolerance translation unit (RTM_TOL, rtm_kernels_tol.hip; STEAL instantiations only): per pixel a bit per sub-pixel —
    // "the contracted search does not find the reference's hit for this sub-pixel's primary ray" (an exact tie in real
    // arithmetic: rtm_path.h, nearest_hit_exactfp) —, in LDS so that a lane that steals a sample of another pixel finds it.
    // Sub-pixels from 64 up have no bit and always take the exact loop.
    // (round 4, later: the any-depth kernels too — PACKL has no stealing, a lane only ever asks for its OWN pixel's word and
    // reads it from the pre-pass's table when it moves on to a sub-pixel: no LDS, no register pair across the loop)
    constexpr bool kPrimFix = (RTM_TOL != 0) && (STEAL || PACKL);
    // ... and a lane whose path ends opens its next sample's stream inside the mix32 pair of the bounce's draws (rtm_path.h:
    // path_shade_core_reopen; round 13): the deferred-fold loops of the tolerance unit's axis-signature kernels
    [[maybe_unused]] constexpr bool kReopen = kPrimFix && DEFER && !REUSE && kAxisTolShape;
    unsigned long long* prim_mask = reinterpret_cast<unsigned long long*>(fq_pend + 3 * 64);  // STEAL: behind its two arrays
    [[maybe_unused]] auto own_prim_mask = [&]() -> unsigned long long {
        if constexpr (STEAL) {
            return prim_mask[lane];
        } else {
            unsigned b = blockIdx.x;
            asm volatile("" : "+s"(b));  // (opaque, like split_wave's: nothing of this stays live across the render loop)
            const unsigned tile_id = (SPLIT && b >= P.split_first) ? P.split_first + (b - P.split_first) % P.n_tiles : b;
            return P.prim_masks[(size_t)tile_id * 64 + (unsigned)lane];
        }
    };
    [[maybe_unused]] bool prim_fix = false;  // this lane's current sample is of a flagged sub-pixel
    [[maybe_unused]] auto prim_flag_of = [&](const unsigned long long mask, const unsigned sub) {
        return sub >= 64u || ((mask >> sub) & 1ull) != 0ull;
    };
    if constexpr (PACKL) {
        if (P.pool) stack.slot = (int)((blockIdx.x * 64u + (unsigned)lane) * 2u);  // two pooled stacks per lane, no allocator
    }
    // (a small wave of a split tile accumulates nothing: its seed is never used)
    D3 acc = seed_of(P, valid, x, y);

    // this wave's samples [n_first, n_end) of the pixel (wave-uniform)
    const bool whole = !SPLIT || blockIdx.x < P.split_first;  // this wave traces all samples of its tile
    // Which wave of a split tile this is, recomputed from an OPAQUE copy of the block index wherever it is needed (a
    // small wave's fold passes, the head wave's final store): kept live across the render loop, these scalars pushed
    // hipcc over its SGPR budget and it spilled loop-carried scalars to VGPR lanes (27 v_readlane / v_writelane more in
    // the kernel: +1 % on the headline frame, profiles/r3/ab_r2_vs_r3.txt).
    auto split_wave = [&](unsigned& f, unsigned& tile) {
        unsigned b = blockIdx.x;
        asm volatile("" : "+s"(b));
        f = (b - P.split_first) / P.n_tiles;
        tile = (b - P.split_first) % P.n_tiles;  // index into partial / contrib
    };
    // (a pass of a frame, rtm_render_scene_samples: the same, offset by sample_begin — split_head / split_len cut the pass)
    unsigned n_first = P.sample_begin, n_end = P.sample_end;
    if (!whole) {
        unsigned f, tile;
        split_wave(f, tile);
        n_first = f != 0u ? P.sample_begin + P.split_head + (f - 1u) * P.split_len : P.sample_begin;
        n_end = f != 0u ? n_first + P.split_len : P.sample_begin + P.split_head;
    }
    // a SMALL wave of the sample split (wave-uniform; its first sample is never 0: wave 0 keeps at least one share):
    // it accumulates nothing — every term goes to P.contrib in the order the wave folds them, 64 to a row, and
    // split_finalize_kernel puts each pixel's terms back in sample order
    // The render loop is compiled TWICE into a SPLIT kernel (`trace` below, generic over a compile-time tag) and a wave
    // picks its copy once: a whole or head wave runs exactly the loop of the unsplit kernel, a small wave a loop without
    // the per-lane FIFO.  One copy with wave-uniform "am I small" branches cost every whole wave of a split launch 1 %
    // (profiles/r3/ab_r2_vs_r3.txt: 181.1 against round 2's 179.3 ms with 64 split tiles).
    unsigned terms_out = 0;  // terms this small wave has stored (wave-uniform)
    unsigned n = valid ? n_first : n_end;  // sample index ((sx-1)*SS + (sy-1))*S + s
    int left_in_sub = P.S - (int)(n_first % (unsigned)P.S);  // samples left before the sub-pixel changes
    const int sub_first = (int)(n_first / (unsigned)P.S);
    // The deferred-fold loops' running sub-pixel index (round 6): a lane's own samples go up by one, so the sub-pixel it moves
    // on to when left_in_sub reaches zero is the next one — no n / S per move.  Right for any first sample (a pass or a small
    // wave that starts inside a sub-pixel: left_in_sub above is what is left of THAT one).  It advances for LIVE lanes only: a
    // lane past its range keeps tracing dummies with n at n_end and the index at n_end / S, a lane outside the frame stays at
    // its wave's first sub-pixel — both within what prim_prepass_kernel wrote for this pass (the pass's sub-pixels and the next
    // one); the direction table's other entries are never read.
    [[maybe_unused]] int sub_cur = sub_first;
    if constexpr (kPrimFix) {
        const unsigned tile_id = (SPLIT && blockIdx.x >= P.split_first) ? P.split_first + (blockIdx.x - P.split_first) % P.n_tiles
                                                                         : blockIdx.x;
        const unsigned long long mask = P.prim_masks[(size_t)tile_id * 64 + (unsigned)lane];  // prim_prepass_kernel, the same launch
        if constexpr (STEAL) prim_mask[lane] = mask;
        prim_fix = prim_flag_of(mask, (unsigned)sub_first);
    }
    // The primary direction of sub-pixel `sub` of the tile's pixel `pl` (its lane number; px, py: its coordinates): from the
    // pre-pass's table where there is one (wave-uniform choice), else computed here.
    constexpr bool kPrimDirs = DEFER && !REUSE;  // the deferred-fold kernels (both translation units)
    [[maybe_unused]] auto primary_of = [&](const unsigned pl, const int px, const int py, const unsigned sub) -> D3 {
        if constexpr (kPrimDirs) {
            if (P.prim_dirs != nullptr) {
                // (the tile's first entry, parked in the camera block's spare LDS slot by the prologue: an integer
                // division to recompute, and a register pair too many to keep across the loop)
                // (a lane that is past its range keeps tracing dummies and keeps asking: its "next sub-pixel" may be one
                // past the pixel's last — clamped, the table ends with the last tile's last sub-pixel)
                const unsigned all = (unsigned)(P.SS * P.SS);
                const unsigned long long first = reinterpret_cast<const unsigned*>(cam + 9)[0];
                unsigned col = pl & 63u;
                asm volatile("" : "+v"(col));  // (opaque: hipcc otherwise hoists the lane's table address out of the render
                                               // loop into a register pair it then spills — 28 GB of scratch reloads per frame)
                // [tile][sub-pixel][component][pixel]
                const double* q = P.prim_dirs + (first + (sub < all ? sub : all - 1u)) * 192 + col;
                constexpr int kStep = 64;
                return D3{q[0], q[kStep], q[2 * kStep]};
            }
        }
        return primary_dir_lds(P, cam, px, py, (int)(sub / (unsigned)P.SS) + 1, (int)(sub % (unsigned)P.SS) + 1);
    };
    D3 pdir = kPrimDirs ? primary_of((unsigned)lane, x, y, (unsigned)sub_first)
                        : primary_dir_lds(P, cam, x, y, sub_first / P.SS + 1, sub_first % P.SS + 1);
    D3 org = P.cam_org, dir = pdir;
    int depth = 0;
    const RngPixelKey pkey = rng_pixel_key(P.seed_mult, pixel);
    RngStream rng = rng_open(pkey, n_first);
    if constexpr (PARK) {
        park[0 * 64 + lane] = acc.x;
        park[1 * 64 + lane] = acc.y;
        park[2 * 64 + lane] = acc.z;
        park[3 * 64 + lane] = pdir.x;
        park[4 * 64 + lane] = pdir.y;
        park[5 * 64 + lane] = pdir.z;
    }

    unsigned long long recq = packed8_empty(empty_n);  // PACK8 records, most recent bounce in the low byte
    auto push = [&](int d, int id) {
        if constexpr (PACK8) {
            recq = (recq << 8) | (unsigned long long)(unsigned)id;
        } else if constexpr (PACKL) {
            // the byte still holds the identity index: xor turns it into id
            const unsigned long long flip = (unsigned long long)((unsigned)id ^ (unsigned)scene_n) << (8 * (d & 7));
            if (d < 8)
                recq ^= flip;
            else if (d < 16)
                rec_w1[lane] ^= flip;
            else
                stack.push(d - 16, id);  // LDS_D == 0: straight to the pooled stack
        } else {
            stack.push(d, id);
        }
    };
    auto pop = [&](int d) -> int { return stack.pop(d); };
    const bool pow2 = P.inv_s != 0.0;  // wave-uniform

    // DEFER: ring indices (wave-uniform) and one pass of the queue
    unsigned fq_head = 0, fq_tail = 0, fq_count = 0;
    // what a lane of the STEAL tail loop folded in this pass, kept for the export behind the per-lane part
    D3 tail_add = d3(0, 0, 0);
    unsigned tail_tag = 0u;
    unsigned stolen_out = 0u;  // STEAL: terms this wave has exported (wave-uniform)
    // MODE 0: whole / head waves, 1: small waves of the sample split, 2: the STEAL tail loop
    auto fold_pass = [&](auto mode_tag) {
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr bool SMALL = SPLIT && MODE == 1;
        constexpr bool TAIL = STEAL && MODE == 2;
        if constexpr (TAIL) tail_tag = 0u;
        [[maybe_unused]] D3 scatter_add = d3(0, 0, 0);
        [[maybe_unused]] unsigned scatter_w = 0x80000000u;  // (a lane without an entry: nobody's)
        const unsigned m = fq_count < 64u ? fq_count : 64u;
        if ((unsigned)lane < m) {
            const unsigned at = (fq_head + (unsigned)lane) & (kFoldRing - 1);
            const uint4 e = fq_in[at];
            const unsigned long long w0 = (unsigned long long)e.x | ((unsigned long long)e.y << 32);
            D3 L;
            if constexpr (PACKL)
                L = path_fold_packed16(sc, (int)(e.z & 0xFFu), (int)((e.z >> 8) & 0x3FFu), w0, fq_in1[at],
                                       P.pool + (size_t)e.w * kPoolLevels);
            else
                L = path_fold_packed8_all(sc, (int)e.z, w0);
            const D3 cal = pow2 ? ((L * P.inv_ss) * P.inv_ss) * P.inv_s : ((L / P.dSS) / P.dSS) / P.dS;  // :240
            const D3 add = clamp01_d3(cal);
            if constexpr (SMALL) {
                // Whole lines from one instruction: the 64 folding lanes write their terms back to back (three 512-byte
                // rows) with the entry's tag behind them.  Round 2 let every OWNER store its term into a [sample][lane]
                // cell: 32-byte stores scattered over the tile's buffer, each completed to the memory's 64-byte granule by
                // a read (PMC: 4.5 GB fetched + 1.6 GB written per headline launch for 1.2 GB of terms).
                unsigned sf, stile;
                split_wave(sf, stile);
                unsigned char* term_rows = P.contrib + ((size_t)stile * (P.split - 1u) + (sf - 1u)) * P.split_len * kTermRowBytes;
                const unsigned pos = terms_out + (unsigned)lane;
                unsigned char* row = term_rows + (size_t)(pos >> 6) * kTermRowBytes;
                double* v = reinterpret_cast<double*>(row) + (pos & 63u);
                // NON-TEMPORAL stores: a plain store of a whole 512-byte row still made L2 fetch the lines it was about to
                // overwrite (PMC, profiles/r3/term_store_modes.txt: 1.25 GB fetched in the render kernel against 0.48 with
                // `nt`; 16-byte-per-lane stores through LDS changed nothing)
                __builtin_nontemporal_store(add.x, v);
                __builtin_nontemporal_store(add.y, v + 64);
                __builtin_nontemporal_store(add.z, v + 128);
                const unsigned tag = fq_tag[at];
                __builtin_nontemporal_store((unsigned short)tag, reinterpret_cast<unsigned short*>(row + 3 * 64 * sizeof(double)) + (pos & 63u));
                if constexpr (PACKL) {
                    // this entry's levels from 16 up have just been read from its owner's pooled stack: one deep entry fewer
                    // of that lane is waiting (two folding lanes may serve the same owner in one pass: an LDS atomic)
                    if (((e.z >> 8) & 0x3FFu) > 16u) atomicSub(&fq_pend[tag & 63u], 0x100u);
                }
            } else if constexpr (kScatter) {
                scatter_add = add;
                // own sample: owner lane | count << 8; stolen (TAIL): 0x80000000 | pixel lane << 16 | sample
                scatter_w = PACKL ? (((e.z >> 18) & 63u) | ((e.z >> 24) << 8)) : e.w;
                if constexpr (TAIL) {
                    tail_add = add;
                    tail_tag = (e.w >> 31) != 0u ? e.w : 0u;
                }
            } else {
                if constexpr (TAIL) {
                    tail_add = add;
                    tail_tag = e.w;  // 0: the owner's own sample; else 0x80000000 | pixel lane << 16 | sample
                }
                if (!TAIL || e.w == 0u) {
                    fq_out[0 * 64 + lane] = add.x;
                    fq_out[1 * 64 + lane] = add.y;
                    fq_out[2 * 64 + lane] = add.z;
                }
            }
        }
        if constexpr (TAIL) {
            // stolen samples' terms leave the chip in fold order, densely packed into the tile's rows (non-temporal)
            const bool out = tail_tag != 0u;
            const unsigned long long m_out = __builtin_amdgcn_ballot_w64(out);
            if (m_out != 0ull) {
                if (out) {
                    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m_out >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_out, 0u));
                    const unsigned pos = stolen_out + rank;
                    unsigned char* row = P.steal_ws + (size_t)blockIdx.x * steal_tile_bytes(P.steal_rows) + kStealHdrBytes +
                                         3 * 64 * sizeof(double) + (size_t)(pos >> 6) * kStealRowBytes;
                    double* v = reinterpret_cast<double*>(row) + (pos & 63u);
                    __builtin_nontemporal_store(tail_add.x, v);
                    __builtin_nontemporal_store(tail_add.y, v + 64);
                    __builtin_nontemporal_store(tail_add.z, v + 128);
                    __builtin_nontemporal_store(tail_tag & 0x7FFFFFFFu, reinterpret_cast<unsigned*>(row + 3 * 64 * sizeof(double)) + (pos & 63u));
                }
                stolen_out += (unsigned)__builtin_popcountll(m_out);
            }
        }
        if constexpr (SMALL) {
            terms_out += m;
        } else if constexpr (kScatter) {
            // every folding lane adds its term to its entry's pixel when it is the entry's turn (:241-242 on the LDS accumulator)
            const bool own_entry = (scatter_w >> 31) == 0u;
            const unsigned owner = scatter_w & 63u, count = (scatter_w >> 8) & 0xFFu;
            const unsigned rank = own_entry ? ((count - fq_done[owner]) & 0xFFu) : 0xFFFFFFFFu;  // 0: the pixel's next term
            for (unsigned round = 0u;; ++round) {
                if (__builtin_amdgcn_ballot_w64(own_entry && rank >= round) == 0) break;
                if (own_entry && rank == round) {
                    park[0 * 64 + owner] += scatter_add.x;
                    park[1 * 64 + owner] += scatter_add.y;
                    park[2 * 64 + owner] += scatter_add.z;
                    fq_done[owner] = count + 1u;  // (rounds go in order: the last write is the pixel's last entry of the pass)
                }
            }
        } else {
            // every owner adds its terms of this pass, oldest first (:241-242 on the LDS accumulator)
            for (;;) {
                const unsigned pend = fq_pend[lane] & 0xFFu;  // (PACKL: bit 8 = "a deep entry of this lane may be waiting")
                const unsigned oldest = (unsigned)(fq_fifo[lane] >> (8u * ((pend ? pend : 1u) - 1u))) & 0xFFu;
                const unsigned rel = (oldest - fq_head) & (kFoldRing - 1);
                const bool mine = pend != 0u && rel < m;
                if (__builtin_amdgcn_ballot_w64(mine) == 0) break;
                if (mine) {
                    park[0 * 64 + lane] += fq_out[0 * 64 + rel];
                    park[1 * 64 + lane] += fq_out[1 * 64 + rel];
                    park[2 * 64 + lane] += fq_out[2 * 64 + rel];
                    // (the last of the lane's entries: the deep flag goes too; otherwise it stays)
                    fq_pend[lane] = pend == 1u ? 0u : (fq_pend[lane] - 1u);
                }
            }
        }
        fq_head = (fq_head + m) & (kFoldRing - 1);
        fq_count -= m;
        (void)mode_tag;
    };
    using ModeWhole = std::integral_constant<int, 0>;
    using ModeSmall = std::integral_constant<int, 1>;
    using ModeTail = std::integral_constant<int, 2>;

    (void)fold_pass;
    // wave-level counters of the DEFER loop (scalar registers): every live lane casts once per trip
    unsigned w_casts = 0, w_bounces = 0, w_draws = 0;
    if constexpr (DEFER && REUSE) {
        // ---- primary-hit reuse (see REUSE above) ----
        // the primary hit of the lane's current sub-pixel: recomputed when the sub-pixel changes (once per S samples)
        double pdis;
        int pid = nearest_hit<M, UNROLL>(sc, P.cam_org, pdir, pdis);
        int id = pid;       // the hit the lane is about to classify ...
        double dis = pdis;  // ... for its ray (org, dir) at `depth`; every lane starts at its first sample's primary hit
        bool have_fresh_rays = false;
        for (;;) {
            const unsigned long long m_live0 = __builtin_amdgcn_ballot_w64(n < n_end);
            if (m_live0 == 0ull) break;
            if (have_fresh_rays) id = nearest_hit<M, UNROLL>(sc, org, dir, dis);  // wave-uniform: one search per lane and trip
            // ---- classify until every live lane holds a hit whose path continues (src/Renderer.cpp:74-78, :112, :116) ----
            bool settled = !(n < n_end);  // a lane past its range: nothing to classify; it shades a dummy below
            for (;;) {
                const bool pending = !settled;
                const unsigned long long m_pend = __builtin_amdgcn_ballot_w64(pending);
                if (m_pend == 0ull) break;
                bool ends = false, drew = false, fifo_full = false;
                if (pending) {
                    const bool capped = P.max_bounces >= 0 && depth >= P.max_bounces;
                    drew = id >= 0 && !capped;
                    bool rr_pass = false;
                    if (drew) rr_pass = rng_next_m(rng) <= sc.kd24(id);  // :78
                    ends = !rr_pass;
                    settled = rr_pass;
                    if (ends) {
                        // queue this path end: ring position = tail + rank among the lanes ending now
                        const unsigned long long ending = __builtin_amdgcn_ballot_w64(true);
                        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(ending >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((unsigned)ending, 0u));
                        const unsigned pos = (fq_tail + rank) & (kFoldRing - 1);
                        const unsigned term_id = (unsigned)(id < 0 ? scene_n : id);
                        fq_in[pos] = uint4{(unsigned)recq, (unsigned)(recq >> 32), term_id, 0u};
                        const unsigned pend = fq_pend[lane] + 1u;
                        fq_fifo[lane] = (fq_fifo[lane] << 8) | pos;
                        fq_pend[lane] = pend;
                        fifo_full = pend >= 8u;
                        // next sample of this pixel: its primary ray and — new — its primary hit
                        ++n;
                        if (--left_in_sub == 0) {
                            left_in_sub = P.S;
                            if (n < n_end) {
                                const int sub = (int)(n / (unsigned)P.S);
                                int px, py;
                                pixel_xy(px, py);
                                pdir = primary_dir_lds(P, cam, px, py, sub / P.SS + 1, sub % P.SS + 1);
                                park[3 * 64 + lane] = pdir.x;
                                park[4 * 64 + lane] = pdir.y;
                                park[5 * 64 + lane] = pdir.z;
                                pid = nearest_hit<M, UNROLL>(sc, P.cam_org, pdir, pdis);  // once per S samples
                            }
                        }
                        org = P.cam_org;
                        dir = d3(park[3 * 64 + lane], park[4 * 64 + lane], park[5 * 64 + lane]);
                        depth = 0;
                        recq = packed8_empty(scene_n);
                        rng = rng_open(pkey, n);
                        id = pid;
                        dis = pdis;
                        settled = !(n < n_end);  // out of samples: done (shades a dummy below)
                    }
                }
                // counters: every classified hit is one PathTracing invocation of the reference
                w_casts += (unsigned)__builtin_popcountll(m_pend);
                w_draws += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(drew));
                const unsigned added = (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ends));
                if (added != 0u) {
                    fq_tail = (fq_tail + added) & (kFoldRing - 1);
                    fq_count += added;
                    const bool force = __builtin_amdgcn_ballot_w64(fifo_full) != 0;
                    while (fq_count >= 64u || (force && fq_count > 0u)) fold_pass(ModeWhole{});
                }
            }
            // ---- bounce: every lane holds a hit that passed the roulette (lanes out of samples: a dummy) ----
            const bool live = n < n_end;
            const unsigned n_live = (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
            if (n_live == 0u) break;
            const int sid = id < 0 ? 0 : id;  // dummies may hold a miss; the scene has at least one sphere here
            ShadeOut o;
            {
                MathSpec m;
                m.set_lds(shade_lds);
                path_bounce_core(m, sc, sid, dis, mode, org, dir, rng, o);
                if (__builtin_amdgcn_ballot_w64(m.bad) != 0) {
                    MathRefI r;
                    r.set_lds(shade_lds);
                    path_bounce_core(r, sc, sid, dis, mode, org, dir, rng, o);
                }
            }
            w_draws += 2u * n_live;
            w_bounces += n_live;
            push(depth, sid);
            depth++;
            org = o.org;
            dir = bounce_dir(o);
            rng.ctr = o.ctr;  // (two draws on from the roulette's, which this loop makes itself: not shade_commit's three)
            have_fresh_rays = true;
        }
        while (fq_count > 0u) fold_pass(ModeWhole{});
    }
    if constexpr (DEFER && !REUSE) {
      bool to_tail = false;  // STEAL: the main loop was left because a lane ran out of samples (wave-uniform)
      auto trace = [&](auto mode_tag) {
        constexpr bool SMALL = SPLIT && decltype(mode_tag)::value == 1;
        // Wave-uniform loop: fold_pass needs all 64 lanes whatever their own state, so a lane that has finished
        // its samples cannot leave.  It does not idle either: it keeps tracing (samples beyond its range, results
        // discarded — `live` gates the queue, the counters and nothing else), which costs nothing — the lanes are
        // there anyway — and keeps the whole body free of a per-lane "am I still in range" region, i.e. of the
        // exec-mask bookkeeping and register copies hipcc generates around one (-14 VALU per trip).
        for (;;) {
            // lane masks as scalars (SGPR pairs straight from the compares): every count below is a popcount
            const unsigned long long m_live = __builtin_amdgcn_ballot_w64(n < n_end);
            if (m_live == 0ull) break;
            if constexpr (STEAL && !SMALL) {
                // a whole tile's first lane has run out of samples: the rest of the tile is the tail loop's
                if (whole && m_live != ~0ull) {
                    to_tail = true;
                    return;
                }
            }
            const bool live = n < n_end;
            bool fifo_full = false;
            D3 term;
            int hit_id;
            const int depth_before = depth;
            PathCounters unused = {0, 0, 0};
            bool cont;
#if RTM_TOL
            // the next sample's stream of a lane whose path ends in this trip: opened inside the bounce's draws (rtm_path.h:
            // path_shade_core_reopen), for the sample index the restart below moves the lane to
            [[maybe_unused]] StreamReopen reopen{pkey, n, m_live, RngStream{0u, 0u}};
            if constexpr (kPrimFix) {
                double dis;
                hit_id = nearest_hit<M, UNROLL>(sc, org, dir, dis);
                const bool flagged = prim_fix && depth == 0;  // rare: a primary ray whose hit last-bit differences could change
                cont = path_shade_spec_fix(sc, hit_id, dis, mode, P.max_bounces, org, dir, depth, rng, term, unused, push, shade_lds,
                                           flagged, [&](int& id_fix, double& dis_fix) {
                                               double dis_ref;
                                               const int id_ref = nearest_hit_exactfp(sc, org, dir, dis_ref);
                                               id_fix = flagged ? id_ref : id_fix;
                                               dis_fix = flagged ? dis_ref : dis_fix;
                                           }, /*stream_after_end=*/false, kReopen ? &reopen : nullptr);  // (kReopen: a path end takes its next stream from there)
            } else
#endif
            cont = path_step<M, UNROLL>(sc, mode, P.max_bounces, org, dir, depth, rng, term, unused, push,
                                        shade_lds, &hit_id, /*stream_after_end=*/false);
            if (PACKL && cont && stack.overflow) {  // records exhausted: the call fails loudly
                cont = false;
#if RTM_TOL
                // (the lane went on: what it holds are its draws' bits, not the stream the restart below takes)
                if constexpr (kReopen) reopen.next = rng_open(pkey, reopen.n_next());
#endif
            }
            // counters (src/Renderer.cpp has none; rtm_stats): one cast per live lane, one draw for the RR test of a
            // hit below the depth cap, two more and a bounce when the path continues
            // (lane masks from compares, combined as scalars: a ballot of a bool that is no compare goes through a VGPR and
            // back.  A path that continued is one whose depth went up — but for a PACKL lane that was stopped just above)
            const unsigned long long m_cont = (PACKL ? __builtin_amdgcn_ballot_w64(cont) : __builtin_amdgcn_ballot_w64(depth != depth_before)) & m_live;
            unsigned long long m_drew = __builtin_amdgcn_ballot_w64(hit_id >= 0) & m_live;
            if (P.max_bounces >= 0) m_drew &= ~__builtin_amdgcn_ballot_w64(depth_before >= P.max_bounces);
            const unsigned n_cont = (unsigned)__builtin_popcountll(m_cont);
            w_casts += (unsigned)__builtin_popcountll(m_live);
            w_draws += (unsigned)__builtin_popcountll(m_drew) + 2u * n_cont;
            w_bounces += n_cont;
            // A path end whose terminal object has no bit in SceneView::emit_mask adds (+0, +0, +0) to an accumulator that is
            // never -0 where a bit of the image depends on it (zero_term_queued): it takes no ring entry — no rank, no count,
            // no tag, no fold, no store — and its lane goes straight on to its next sample.  The counters above have counted it.
            const bool emits = zero_term_queued(P.scene, hit_id);
            const bool queued = !cont && live && emits;
            const unsigned long long m_queued = m_live & ~m_cont & __builtin_amdgcn_ballot_w64(emits);
            if (!cont) {
                if (queued) {
                    // queue this path end: ring position = tail + rank among the lanes queueing now
                    const unsigned term_id = (unsigned)(hit_id < 0 ? scene_n : hit_id);
                    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m_queued >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((unsigned)m_queued, 0u));
                    const unsigned pos = (fq_tail + rank) & (kFoldRing - 1);
                    if constexpr (PACKL && kScatter && !SMALL) {
                        // fq_pend: bits 0..7 the lane's QUEUED path ends so far, 8..15 that count after its last queued DEEP path, 16:
                        // there was one.  (A deep path that is not queued leaves all of it alone: nobody will read its levels in
                        // the pooled stack, so the lane keeps the stack it has — its next deep path overwrites them — and no
                        // "deep entry waiting" state arises.)
                        const unsigned word = fq_pend[lane];
                        const unsigned count = word & 0xFFu, next = (count + 1u) & 0xFFu;
                        fq_in[pos] = uint4{(unsigned)recq, (unsigned)(recq >> 32),
                                           term_id | ((unsigned)depth << 8) | ((unsigned)lane << 18) | (count << 24),
                                           (unsigned)(stack.slot < 0 ? 0 : stack.slot)};
                        fq_in1[pos] = rec_w1[lane];
                        if (depth > 16) {
                            // Levels from 16 up sit in the lane's pooled stack and are read when the entry is folded; the lane has
                            // TWO pooled stacks and changes over whenever it queues such a path.  Only if its previous deep entry
                            // may still be waiting — fq_done has not reached the count the lane had after it (mod 256: a count
                            // that ran far ahead reads as "waiting", which only costs a pass) — is a pass forced.
                            const unsigned behind = (((word >> 8) & 0xFFu) - fq_done[lane]) & 0xFFu;
                            fifo_full = (word & 0x10000u) != 0u && behind != 0u && behind <= 128u;
                            stack.slot ^= 1;
                            fq_pend[lane] = next | (next << 8) | 0x10000u;
                        } else {
                            fq_pend[lane] = next | (word & 0x1FF00u);
                        }
                    } else if constexpr (PACKL) {
                        fq_in[pos] = uint4{(unsigned)recq, (unsigned)(recq >> 32), term_id | ((unsigned)depth << 8),
                                           (unsigned)(stack.slot < 0 ? 0 : stack.slot)};
                        fq_in1[pos] = rec_w1[lane];
                    } else if constexpr (kScatter && !SMALL) {
                        // (fold_pass: the folding lane adds the term to this lane's pixel when the count says it is its turn.  The
                        // count is of QUEUED path ends — fq_pend here, fq_done there —, so a pixel's additions keep the order of its
                        // non-zero path ends; a zero one has no place in that order because it changes no bit)
                        const unsigned ends_so_far = fq_pend[lane];
                        fq_in[pos] = uint4{(unsigned)recq, (unsigned)(recq >> 32), term_id, (unsigned)lane | ((ends_so_far & 0xFFu) << 8)};
                        fq_pend[lane] = ends_so_far + 1u;
                    } else {
                        fq_in[pos] = uint4{(unsigned)recq, (unsigned)(recq >> 32), term_id, 0u};
                    }
                    if constexpr (SPLIT) {
                        if constexpr (SMALL) fq_tag[pos] = (unsigned short)((unsigned)lane | ((n - n_first) << 6));
                    }
                    if constexpr (!(kScatter && !SMALL)) {
                    // whole waves: count of the lane's waiting entries, and (PACKL) bit 8: a deep entry of the lane may be waiting.
                    // A small wave never picks its terms up again, so it keeps no count — only (PACKL) the NUMBER of the
                    // lane's deep entries still waiting, in bits 8 up, taken down by whoever folds one (fold_pass)
                    const unsigned pend_word = fq_pend[lane];
                    const unsigned pend = SMALL ? 0u : (pend_word & 0xFFu) + 1u;
                    if constexpr (!SMALL) fq_fifo[lane] = (fq_fifo[lane] << 8) | pos;
                    fifo_full = !SMALL && pend >= 8u;
                    const bool deep_now = PACKL && depth > 16;
                    if constexpr (SMALL) {
                        if constexpr (PACKL) fq_pend[lane] = pend_word + (deep_now ? 0x100u : 0u);
                    } else {
                        fq_pend[lane] = pend | (pend_word & 0x100u) | (deep_now ? 0x100u : 0u);
                    }
                    if constexpr (PACKL) {
                        // Levels from 16 up sit in the lane's pooled stack and are read when the entry is folded, so the
                        // lane's next path must not write there before.  The lane has TWO pooled stacks and changes over
                        // whenever it queues such a path; only if the other one may still be waiting in the queue (a second
                        // deep path before the lane's entries have all been folded: rare squared) is a pass forced.  Forcing
                        // one for every deep path (P(depth > 16) = 1.5 % of the paths: every fifth trip of a wave) ran the
                        // fold half empty that often: +4 % on the 512x512 unlimited-depth frame.
                        if (deep_now) {
                            fifo_full = fifo_full || (pend_word >> 8) != 0u;
                            stack.slot ^= 1;
                        }
                    }
                    }  // (the FIFO form, or a small wave)
                }
                if constexpr (PACKL) {
                    if (depth > 8) rec_w1[lane] = packed8_empty(scene_n);
                }
                // next sample of this pixel (src/Renderer.cpp:236-239); a lane past its range stays at n_end, so that
                // "n - pending" remains the sample index of its queued path ends (fold_pass, SPLIT)
                n = add_lane_bit(n, m_live);
                if (--left_in_sub == 0) {
                    left_in_sub = P.S;
                    // (== n / S for a lane in its range: n has just become a multiple of S; a lane past it stays where it is)
                    const int sub = sub_cur = (int)add_lane_bit((uint32_t)sub_cur, m_live);
                    int px, py;
                    pixel_xy(px, py);
                    if constexpr (kPrimDirs) pdir = primary_of((unsigned)lane, px, py, (unsigned)sub);
                    else pdir = primary_dir_lds(P, cam, px, py, sub / P.SS + 1, sub % P.SS + 1);
                    park[3 * 64 + lane] = pdir.x;
                    park[4 * 64 + lane] = pdir.y;
                    park[5 * 64 + lane] = pdir.z;
                    if constexpr (kPrimFix) prim_fix = n < n_end && prim_flag_of(own_prim_mask(), (unsigned)sub);
                }
                if constexpr (kPrimFix) prim_fix = prim_fix && n < n_end;
                org = P.cam_org;
                dir = d3(park[3 * 64 + lane], park[4 * 64 + lane], park[5 * 64 + lane]);
                depth = 0;
                recq = packed8_empty(empty_n);
#if RTM_TOL
                if constexpr (kReopen) rng = reopen.next;  // == rng_open(pkey, n)
                else
#endif
                rng = rng_open(pkey, n);
            }
            const unsigned added = (unsigned)__builtin_popcountll(m_queued);  // queued entries only
            if (added != 0u) {
                fq_tail = (fq_tail + added) & (kFoldRing - 1);
                fq_count += added;
                const bool force = __builtin_amdgcn_ballot_w64(fifo_full) != 0;  // a lane's FIFO holds 8 positions
                while (fq_count >= 64u || (force && fq_count > 0u)) fold_pass(mode_tag);
            }
        }
        while (fq_count > 0u) fold_pass(mode_tag);
        if constexpr (SMALL) {
            // how many terms split_finalize_kernel will find in this wave's rows (an absent (lane, sample) is nothing to add)
            unsigned sf, stile;
            split_wave(sf, stile);
            if (lane == 0) P.split_counts[(size_t)stile * (P.split - 1u) + (sf - 1u)] = terms_out;
        }
      };
      if constexpr (SPLIT) {
          if (n_first != P.sample_begin) trace(ModeSmall{});  // (a small wave's first sample is never the pass's first: wave 0 keeps at least one share)
          else trace(ModeWhole{});
      } else {
          trace(ModeWhole{});
      }
      if constexpr (STEAL) {
       if (whole) {
        unsigned end_own = valid ? P.sample_end : 0u;  // one past the last sample this lane's pixel accumulated itself
        if (to_tail) {
          // ---- the tail loop of a whole tile (see STEAL above) ----
          unsigned* st_next = reinterpret_cast<unsigned*>(fq_pend + 64);  // per pixel: the next own sample its lane will START
          unsigned* st_end = st_next + 64;                               // per pixel: one past its last OWN sample
          const unsigned total = P.sample_end;
          bool busy = n < n_end;                                         // this lane has a path in flight ...
          if constexpr (kPrimFix) prim_fix = prim_fix && busy;
          unsigned cur = ((unsigned)lane << 16) | (busy ? n : 0u);       // ... of (pixel lane, sample)
          unsigned own_next = busy ? n + 1u : total;
          st_next[lane] = own_next;
          st_end[lane] = valid ? total : 0u;
          unsigned claimed = 0u;                                         // samples taken from other pixels so far (wave-uniform)
          const unsigned cap = P.steal_rows * 64u;
          const unsigned floor_s = total > P.steal_depth ? total - P.steal_depth : 0u;
          const unsigned ftile = (unsigned)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<const unsigned*>(cam + 9)[1]);
          const unsigned tile_x8 = (ftile % (unsigned)P.tiles_x) * 8u, tile_y = ftile / (unsigned)P.tiles_x;
          for (;;) {
            const unsigned long long m_busy = __builtin_amdgcn_ballot_w64(busy);
            if (m_busy == 0ull) break;
            bool fifo_full = false;
            D3 term;
            int hit_id;
            const int depth_before = depth;
            PathCounters unused = {0, 0, 0};
            bool cont;
#if RTM_TOL
            if constexpr (kPrimFix) {
                double dis;
                hit_id = nearest_hit<M, UNROLL>(sc, org, dir, dis);
                const bool flagged = prim_fix && depth == 0;  // rare: a primary ray whose hit last-bit differences could change
                cont = path_shade_spec_fix(sc, hit_id, dis, mode, P.max_bounces, org, dir, depth, rng, term, unused, push, shade_lds,
                                           flagged, [&](int& id_fix, double& dis_fix) {
                                               double dis_ref;
                                               const int id_ref = nearest_hit_exactfp(sc, org, dir, dis_ref);
                                               id_fix = flagged ? id_ref : id_fix;
                                               dis_fix = flagged ? dis_ref : dis_fix;
                                           }, /*stream_after_end=*/false);  // (a path end reopens the lane's stream below: plainly —
                                                                            // the main loop's hand-over here costs the headline kernel
                                                                            // its 128th register and 8 bytes of scratch)
            } else
#endif
            cont = path_step<M, UNROLL>(sc, mode, P.max_bounces, org, dir, depth, rng, term, unused, push, shade_lds, &hit_id,
                                        /*stream_after_end=*/false);
            const unsigned long long m_cont = __builtin_amdgcn_ballot_w64(depth != depth_before) & m_busy;  // (the main loop's rule)
            unsigned long long m_drew = __builtin_amdgcn_ballot_w64(hit_id >= 0) & m_busy;
            if (P.max_bounces >= 0) m_drew &= ~__builtin_amdgcn_ballot_w64(depth_before >= P.max_bounces);
            const unsigned n_cont = (unsigned)__builtin_popcountll(m_cont);
            w_casts += (unsigned)__builtin_popcountll(m_busy);
            w_draws += (unsigned)__builtin_popcountll(m_drew) + 2u * n_cont;
            w_bounces += n_cont;
            const bool need = !busy || !cont;  // this lane wants a new sample
            // (the main loop's rule: a path end that provably adds (+0, +0, +0) is not queued — an own sample keeps out of its
            // pixel's count, a stolen one is not exported and steal_finalize_kernel finds nothing under its (pixel, sample))
            const bool emits = zero_term_queued(P.scene, hit_id);
            const bool ended = busy && !cont && emits;
            const unsigned long long m_ended = m_busy & ~m_cont & __builtin_amdgcn_ballot_w64(emits);
            if (ended) {
                const unsigned term_id = (unsigned)(hit_id < 0 ? scene_n : hit_id);
                const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m_ended >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_ended, 0u));
                const unsigned pos = (fq_tail + rank) & (kFoldRing - 1);
                const bool own = (cur >> 16) == (unsigned)lane;
                if constexpr (kScatter) {
                    const unsigned ends_so_far = fq_pend[lane];  // (of this lane's OWN pixel)
                    fq_in[pos] = uint4{(unsigned)recq, (unsigned)(recq >> 32), term_id,
                                       own ? ((unsigned)lane | ((ends_so_far & 0xFFu) << 8)) : (0x80000000u | cur)};
                    if (own) fq_pend[lane] = ends_so_far + 1u;
                } else {
                fq_in[pos] = uint4{(unsigned)recq, (unsigned)(recq >> 32), term_id, own ? 0u : (0x80000000u | cur)};
                if (own) {  // the owner picks its term up again, in the order its paths ended
                    const unsigned pend = (fq_pend[lane] & 0xFFu) + 1u;
                    fq_fifo[lane] = (fq_fifo[lane] << 8) | pos;
                    fq_pend[lane] = pend;
                    fifo_full = pend >= 8u;
                }
                }
            }
            const unsigned added = (unsigned)__builtin_popcountll(m_ended);  // queued entries only
            // (1) the lane's own next sample, if its pixel still has one that nobody took
            bool got = false;
            if (need && own_next < st_end[lane]) {
                cur = ((unsigned)lane << 16) | own_next;
                ++own_next;
                st_next[lane] = own_next;
                got = true;
                if (--left_in_sub == 0) {
                    left_in_sub = P.S;
                    const int sub = ++sub_cur;  // (own samples — always within the pass here — go up by one as in the main loop)
                    int px, py;
                    pixel_xy(px, py);
                    if constexpr (kPrimDirs) pdir = primary_of((unsigned)lane, px, py, (unsigned)sub);
                    else pdir = primary_dir_lds(P, cam, px, py, sub / P.SS + 1, sub % P.SS + 1);
                    park[3 * 64 + lane] = pdir.x;
                    park[4 * 64 + lane] = pdir.y;
                    park[5 * 64 + lane] = pdir.z;
                }
                dir = d3(park[3 * 64 + lane], park[4 * 64 + lane], park[5 * 64 + lane]);
                rng = rng_open(pkey, cur & 0xFFFFu);
                if constexpr (kPrimFix) {
                    const unsigned s_own = cur & 0xFFFFu;
                    prim_fix = prim_flag_of(prim_mask[lane], P.S == 1 ? s_own : __umulhi(s_own, P.magic_S));
                }
            }
            // (2) lanes left without one take the LAST unstarted samples of the pixel that has most to give: what it has
            // not started, but one, and not below the depth the finalize kernel's index covers
            const unsigned long long m_want = __builtin_amdgcn_ballot_w64(need && !got);
            if (m_want != 0ull && claimed < cap) {
                const unsigned e_l = st_end[lane], n_l = st_next[lane];
                unsigned give = e_l > n_l + 1u ? e_l - n_l - 1u : 0u;
                const unsigned above = e_l > floor_s ? e_l - floor_s : 0u;
                give = give < above ? give : above;
                give = give < 255u ? give : 255u;
                unsigned long long cand = ~0ull;  // bitwise search for the largest `give`, lowest lane on ties
#pragma unroll
                for (int b = 7; b >= 0; --b) {
                    const unsigned long long mb = __builtin_amdgcn_ballot_w64(((give >> b) & 1u) != 0u) & cand;
                    cand = mb != 0ull ? mb : cand;
                }
                const int v = (int)__builtin_ctzll(cand);
                const unsigned give_v = (unsigned)__builtin_amdgcn_readlane((int)give, v);
                unsigned take = (unsigned)__builtin_popcountll(m_want);
                take = take < give_v ? take : give_v;
                take = take < cap - claimed ? take : cap - claimed;
                if (take != 0u) {
                    const unsigned e_v = (unsigned)__builtin_amdgcn_readlane((int)e_l, v);
                    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m_want >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_want, 0u));
                    if (need && !got && rank < take) {
                        const unsigned s_st = e_v - 1u - rank;
                        cur = ((unsigned)v << 16) | s_st;
                        got = true;
                        // pixel v of this tile, sample s_st: its primary ray and RNG stream from scratch (wave-uniform pixel)
                        const int px = (int)tile_x8 + (v & 7), py = band_row(P, (int)tile_y, v >> 3);
                        const RngPixelKey vkey = rng_pixel_key(P.seed_mult, (uint32_t)py * (uint32_t)P.W + (uint32_t)px);
                        // s_st / S and sub / SS by multiplication (exact for operands below 2^16; a divisor of 1 has no magic)
                        const unsigned sub = P.S == 1 ? s_st : __umulhi(s_st, P.magic_S);
                        const unsigned sxm1 = P.SS == 1 ? sub : __umulhi(sub, P.magic_SS);
                        if constexpr (kPrimDirs) dir = primary_of((unsigned)v, px, py, sub);
                        else dir = primary_dir_lds(P, cam, px, py, (int)sxm1 + 1, (int)(sub - sxm1 * (unsigned)P.SS) + 1);
                        rng = rng_open(vkey, s_st);
                        if constexpr (kPrimFix) prim_fix = prim_flag_of(prim_mask[v], sub);
                    }
                    if (lane == v) st_end[lane] = e_v - take;
                    claimed += take;
                }
            }
            if (need) {
                busy = got;
                org = P.cam_org;
                depth = 0;
                recq = packed8_empty(empty_n);
                if constexpr (kPrimFix) prim_fix = prim_fix && got;
            }
            if (added != 0u) {
                fq_tail = (fq_tail + added) & (kFoldRing - 1);
                fq_count += added;
                const bool force = __builtin_amdgcn_ballot_w64(fifo_full) != 0;
                while (fq_count >= 64u || (force && fq_count > 0u)) fold_pass(ModeTail{});
            }
          }
          while (fq_count > 0u) fold_pass(ModeTail{});
          end_own = st_end[lane];
        }
        // the tile's block: accumulators, every pixel's own-sample end, the number of stolen terms
        unsigned char* blk = P.steal_ws + (size_t)blockIdx.x * steal_tile_bytes(P.steal_rows);
        double* part = reinterpret_cast<double*>(blk + kStealHdrBytes) + lane;
        part[0] = park[0 * 64 + lane];
        part[64] = park[1 * 64 + lane];
        part[128] = park[2 * 64 + lane];
        reinterpret_cast<unsigned short*>(blk + 128)[lane] = (unsigned short)end_own;
        if (lane == 0) reinterpret_cast<unsigned*>(blk)[0] = stolen_out;
       }
      }
    }
    unsigned long long st_near = 0, st_shade = 0, st_end = 0, st_iters = 0;
    while (!DEFER && n < n_end) {
        D3 term;
        bool cont;
        unsigned long long ts0 = 0, ts1 = 0, ts2 = 0;
        if constexpr (STAMP) {
            ts0 = stamp_now();
            double dis;
            const int id = nearest_hit<M, UNROLL>(sc, org, dir, dis);
            ts1 = stamp_now();
            cont = path_shade_spec(sc, id, dis, mode, P.max_bounces, org, dir, depth, rng, term, pc, push, shade_lds);
            ts2 = stamp_now();
        } else {
            cont = path_step<M, UNROLL>(sc, mode, P.max_bounces, org, dir, depth, rng, term, pc, push, shade_lds);
        }
        if (cont && stack.overflow) {  // records exhausted: stop the path; the call fails loudly
            cont = false;
            term = d3(0, 0, 0);
            depth = 0;
        }
        if (!cont) {
            // all ending lanes within the LDS levels (always, when max_bounces < 16): blocked fold
            const bool deep = depth > LDS_D;
            D3 L;
            if constexpr (PACK8)
                L = path_fold_packed8(sc, term, depth, recq);
            else
                L = (__builtin_amdgcn_ballot_w64(deep) == 0)
                        ? path_fold_blocked(sc, term, depth, [&](int d) { return (int)rec[d * 64 + lane]; })
                        : path_fold(sc, term, depth, pop);
            // :240 cal / SS / SS / S.  x/2^k and x*2^-k are the same correctly rounded value, so
            // power-of-two divisors are applied as multiplications.
            const D3 cal = pow2 ? ((L * P.inv_ss) * P.inv_ss) * P.inv_s : ((L / P.dSS) / P.dSS) / P.dS;
            const D3 add = clamp01_d3(cal);
            if constexpr (PARK) {  // :241-242 on the LDS-resident accumulator
                park[0 * 64 + lane] += add.x;
                park[1 * 64 + lane] += add.y;
                park[2 * 64 + lane] += add.z;
            } else {
                acc = acc + add;
            }
            ++n;
            if (--left_in_sub == 0) {
                left_in_sub = P.S;
                if (n < n_end) {
                    const int sub = (int)(n / (unsigned)P.S);
                    int px, py;
                    pixel_xy(px, py);
                    pdir = primary_dir_lds(P, cam, px, py, sub / P.SS + 1, sub % P.SS + 1);
                    if constexpr (PARK) {
                        park[3 * 64 + lane] = pdir.x;
                        park[4 * 64 + lane] = pdir.y;
                        park[5 * 64 + lane] = pdir.z;
                    }
                }
            }
            org = P.cam_org;
            if constexpr (PARK)
                dir = d3(park[3 * 64 + lane], park[4 * 64 + lane], park[5 * 64 + lane]);
            else
                dir = pdir;
            depth = 0;
            if constexpr (PACK8) recq = packed8_empty(scene_n);
            rng = rng_open(pkey, n);
        }
        if constexpr (STAMP) {
            const unsigned long long ts3 = stamp_now();
            st_near += ts1 - ts0;
            st_shade += ts2 - ts1;
            st_end += ts3 - ts2;
            st_iters += 1;
        }
    }
    if constexpr (STAMP) {
        if (lane == 0 && P.stamps) {
            P.stamps[blockIdx.x * 4 + 0] = st_near;
            P.stamps[blockIdx.x * 4 + 1] = st_shade;
            P.stamps[blockIdx.x * 4 + 2] = st_end;
            P.stamps[blockIdx.x * 4 + 3] = st_iters;
        }
    }

    if constexpr (PARK) acc = d3(park[0 * 64 + lane], park[1 * 64 + lane], park[2 * 64 + lane]);
    if (STEAL && whole) {
        // steal_finalize_kernel stores the pixel (the tail loop has left the tile's block in P.steal_ws)
    } else if (whole) {
        int px, py;
        pixel_xy(px, py);
        store_pixel(P, (px < P.W) && (py < P.row_end), px, py, acc);
    } else if (n_first == P.sample_begin) {  // the head wave of a split tile
        unsigned hf, split_tile;
        split_wave(hf, split_tile);
        double* dst = P.partial + (size_t)split_tile * 192 + lane;
        dst[0] = acc.x;
        dst[64] = acc.y;
        dst[128] = acc.z;
    }
    if (P.counters) {
        if constexpr (DEFER) {
            if (lane == 0) {
                atomicAdd(P.counters + 0, (unsigned long long)w_casts);
                atomicAdd(P.counters + 1, (unsigned long long)w_bounces);
                atomicAdd(P.counters + 2, (unsigned long long)w_draws);
            }
        } else {
            wave_add_counter(P.counters + 0, pc.casts);
            wave_add_counter(P.counters + 1, pc.bounces);
            wave_add_counter(P.counters + 2, pc.draws);
        }
        if (stack.overflow) atomicOr(P.counters + 3, 1ull);
    }
}

// Second half of a SPLIT render: image[pixel] = (((partial + term[split_head]) + term[split_head+1]) + ...), the
// accumulation order of src/Renderer.cpp:241-242.  One workgroup of four waves per split tile.  The small waves left
// their terms in FOLD order (render_tiles_kernel: rows of 64 terms + tags); for one small wave at a time the block
// scatters its rows into LDS by (sample, owner lane) — the tag — and waves 0..2 then add, each for ONE colour channel
// (the three sums are independent), their pixel's terms in sample order.  LDS: split_len x 64 x 3 doubles (96 KB at
// the 64 samples a small wave traces at most).
// A small wave stores only the path ends it queued (SceneView::emit_mask): P.split_counts says how many, and a word per sample
// behind the slots — bit l: "lane l's term of this sample is there" — says which; an absent one is nothing to add (its slot
// holds whatever was there before and is not read).  The words are cleared per small wave: split_len x 8 bytes, not the slots.
__global__ __launch_bounds__(256) void split_finalize_kernel(const RenderParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* slot = reinterpret_cast<double*>(lds_raw);  // [channel][sample][lane]
    unsigned* present = reinterpret_cast<unsigned*>(slot + (size_t)P.split_len * 64u * 3u);  // [sample][2]
    const int tid = threadIdx.x, lane = tid & 63, chan = tid >> 6;
    const unsigned tile = frame_tile(P, P.split_first + blockIdx.x);  // blockIdx.x: index among the split tiles
    if (tile == ~0u) return;
    const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
    const int px = tx * 8 + (lane & 7), py = band_row(P, ty, lane >> 3);
    const bool valid = (px < P.W) && (py < P.row_end);
    const unsigned plane_sz = P.split_len * 64u;  // doubles per channel
    double acc = chan < 3 ? P.partial[(size_t)blockIdx.x * 192 + chan * 64 + lane] : 0.0;
    for (unsigned f = 1; f < P.split; ++f) {
        const unsigned char* rows = P.contrib + ((size_t)blockIdx.x * (P.split - 1u) + (f - 1u)) * P.split_len * kTermRowBytes;
        // terms this small wave has stored: at most one per pixel and sample of its range (a count beyond that: a stale or
        // foreign buffer, which must not turn into a fault)
        unsigned n_terms = P.split_counts[(size_t)blockIdx.x * (P.split - 1u) + (f - 1u)];
        n_terms = n_terms <= plane_sz ? n_terms : 0u;
        for (unsigned m = (unsigned)tid; m < P.split_len * 2u; m += 256u) present[m] = 0u;
        __syncthreads();
        for (unsigned e = (unsigned)tid; e < n_terms; e += 256u) {
            const unsigned char* row = rows + (size_t)(e >> 6) * kTermRowBytes;
            const double* v = reinterpret_cast<const double*>(row) + (e & 63u);
            const unsigned tag = reinterpret_cast<const unsigned short*>(row + 3 * 64 * sizeof(double))[e & 63u];
            if ((tag >> 6) >= P.split_len) continue;  // (never, when the render kernel wrote the row)
            const unsigned at = (tag >> 6) * 64u + (tag & 63u);  // [sample][owner lane]
            slot[at] = v[0];
            slot[plane_sz + at] = v[64];
            slot[2 * plane_sz + at] = v[128];
            atomicOr(&present[(tag >> 6) * 2u + ((tag >> 5) & 1u)], 1u << (tag & 31u));
        }
        __syncthreads();
        if (chan < 3) {
            const double* mine = slot + (size_t)chan * plane_sz + lane;
            const unsigned* bits = present + (lane >> 5);
            for (unsigned m = 0; m < P.split_len; ++m)  // in sample order, the terms that are there
                if ((bits[m * 2u] >> (lane & 31)) & 1u) acc = acc + mine[m * 64u];
        }
        __syncthreads();
    }
    if (chan < 3) slot[chan * 64 + lane] = acc;
    __syncthreads();
    if (chan == 0) store_pixel(P, valid, px, py, d3(slot[lane], slot[64 + lane], slot[128 + lane]));
}

// Second half of a STEAL render (whole tiles): pixel = ((partial + term[end]) + term[end + 1]) + ... — the accumulation
// order of src/Renderer.cpp:241-242 — where `partial` holds the samples [0, end) the pixel's own lane traced and the terms
// of [end, total) were traced by other lanes of the tile and lie, in fold order and tagged (pixel lane, sample), in the
// tile's rows.  One wave per tile: an index of row positions by (sample, pixel) in LDS, then every lane walks its pixel's
// stolen samples in order.  LDS: steal_depth x 64 two-byte entries, cleared to "absent" first: a stolen sample whose path
// end provably adds (+0, +0, +0) was not exported (SceneView::emit_mask) and is nothing to add.
__global__ __launch_bounds__(64) void steal_finalize_kernel(const RenderParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    unsigned short* idx = reinterpret_cast<unsigned short*>(lds_raw);  // [sample - floor][pixel lane] -> position in the rows
    const int lane = threadIdx.x;
    const unsigned tile = blockIdx.x;
    const unsigned ftile = frame_tile(P, tile);
    if (ftile == ~0u) return;
    const int tx = ftile % P.tiles_x, ty = ftile / P.tiles_x;
    const int px = tx * 8 + (lane & 7), py = band_row(P, ty, lane >> 3);
    const bool valid = (px < P.W) && (py < P.row_end);
    const unsigned char* blk = P.steal_ws + (size_t)tile * steal_tile_bytes(P.steal_rows);
    unsigned n_terms = reinterpret_cast<const unsigned*>(blk)[0];
    unsigned end_own = reinterpret_cast<const unsigned short*>(blk + 128)[lane];
    // (never out of range when the render kernel wrote the block; a stale or foreign block must not turn into a fault)
    n_terms = n_terms <= P.steal_rows * 64u ? n_terms : 0u;
    const unsigned floor_chk = P.sample_end > P.steal_depth ? P.sample_end - P.steal_depth : 0u;
    end_own = (n_terms != 0u && end_own >= floor_chk && end_own <= P.sample_end) ? end_own : P.sample_end;
    const double* part = reinterpret_cast<const double*>(blk + kStealHdrBytes) + lane;
    D3 acc = d3(part[0], part[64], part[128]);
    if (n_terms != 0u) {  // wave-uniform
        const unsigned total = P.sample_end;
        const unsigned floor_s = total > P.steal_depth ? total - P.steal_depth : 0u;
        const unsigned char* rows = blk + kStealHdrBytes + 3 * 64 * sizeof(double);
        for (unsigned k = (unsigned)lane; k < P.steal_depth * 32u; k += 64u) reinterpret_cast<unsigned*>(idx)[k] = 0xFFFFFFFFu;
        __syncthreads();
        for (unsigned e = (unsigned)lane; e < n_terms; e += 64u) {
            const unsigned tag = reinterpret_cast<const unsigned*>(rows + (size_t)(e >> 6) * kStealRowBytes + 3 * 64 * sizeof(double))[e & 63u];
            const unsigned ts = tag & 0xFFFFu, tv = (tag >> 16) & 63u;
            if (ts >= floor_s && ts < total) idx[(ts - floor_s) * 64u + tv] = (unsigned short)e;
        }
        __syncthreads();
        if (valid) {
            for (unsigned s = end_own; s < total; ++s) {
                const unsigned e = idx[(s - floor_s) * 64u + (unsigned)lane];
                if (e >= n_terms) continue;  // absent (0xFFFF; a tile holds at most steal_rows x 64 < 65 535 terms)
                const double* v = reinterpret_cast<const double*>(rows + (size_t)(e >> 6) * kStealRowBytes) + (e & 63u);
                acc = acc + d3(v[0], v[64], v[128]);
            }
        }
    }
    store_pixel(P, valid, px, py, acc);
}

// Host side: every launch of the three kernels above goes through these.
// render_tiles_kernel<M, F, UNROLL, RecT, LDS_D, WPE> over `grid` tiles with render_lds_bytes' LDS and RenderParams::unit_tab
template <class M, unsigned F, int UNROLL, typename RecT, int LDS_D, int WPE>
void launch_tiles(RenderParams P, unsigned grid, size_t pad, hipStream_t stream) {
    const size_t lds = render_lds_bytes<F, RecT, LDS_D>(P.scene.n, lds_rows_for(UNROLL), pad, &P.unit_tab);
    render_tiles_kernel<M, F, UNROLL, RecT, LDS_D, WPE><<<grid, 64, lds, stream>>>(P);
}
// after a split launch (kSplit): one block per split tile
inline void launch_split_finalize(const RenderParams& P, hipStream_t stream) {
    split_finalize_kernel<<<P.n_tiles, 256, (size_t)P.split_len * (64 * 3 * sizeof(double) + 2 * sizeof(unsigned)), stream>>>(P);
}
// after a stealing launch (kSteal) of `grid` blocks: one block per whole tile
inline void launch_steal_finalize(const RenderParams& P, unsigned grid, hipStream_t stream) {
    const unsigned n_whole = P.split > 1 ? P.split_first : grid;
    if (n_whole) steal_finalize_kernel<<<n_whole, 64, (size_t)P.steal_depth * 64 * sizeof(unsigned short), stream>>>(P);
}

// The pre-pass of the deferred-fold kernels, one wave per tile of the launch, lane = pixel: every sub-pixel's primary direction
// (src/Renderer.cpp:227-232: shared by the sub-pixel's S samples) goes to RenderParams::prim_dirs, computed HERE by all 64
// lanes at once with the very function the render loop would call — so that a lane of the render kernel that moves on to its
// next sub-pixel loads three doubles instead of running five correctly rounded divisions alone in its wave (about every 4.4
// trips some lane of a wave does: 4 % of the frame; same bits by construction).  In the tolerance translation unit it also
// leaves, per pixel, a bit per sub-pixel (the first 64 of them): "this primary ray is one whose nearest hit last-bit
// differences could change" (rtm_path.h: primary_tie_risk; the shipped Cornell box has such rays along the image's
// diagonals, where the seam of two wall spheres projects exactly) — the render kernel settles those rays' primary hits with
// the reference's own arithmetic (nearest_hit_exactfp).
__global__ __launch_bounds__(64) void prim_prepass_kernel(const RenderParams P, unsigned long long* __restrict__ masks,
                                                          double* __restrict__ dirs) {
    const int lane = threadIdx.x;
    const unsigned tile = blockIdx.x;
    const unsigned ftile = frame_tile(P, tile);
    if (ftile == ~0u) return;
    auto store_dir = [&](const unsigned sub, const D3 d) {  // RenderParams::prim_dirs: [tile][pixel][sub-pixel][component]
        const unsigned all_s = (unsigned)(P.SS * P.SS);
        double* q = dirs + ((size_t)tile * all_s + sub) * 192 + (unsigned)lane;
        constexpr int kStep = 64;
        __builtin_nontemporal_store(d.x, q);
        __builtin_nontemporal_store(d.y, q + kStep);
        __builtin_nontemporal_store(d.z, q + 2 * kStep);
    };
    const int x = (int)(ftile % (unsigned)P.tiles_x) * 8 + (lane & 7);
    const int y = band_row(P, (int)(ftile / (unsigned)P.tiles_x), lane >> 3);
    const double cam[9] = {P.ax.x, P.ax.y, P.ax.z, P.by.x, P.by.y, P.by.z, P.cz.x, P.cz.y, P.cz.z};
    [[maybe_unused]] unsigned long long mask = 0ull;
    const unsigned all = (unsigned)(P.SS * P.SS);
    // the sub-pixels of the pass's samples, and the next one (a lane past its range asks for it: render_tiles_kernel's primary_of)
    const unsigned sub_end = (P.sample_end - 1u) / (unsigned)P.S + 2u;
    for (unsigned sub = P.sample_begin / (unsigned)P.S; sub < (sub_end < all ? sub_end : all); ++sub) {
        if (dirs == nullptr && (masks == nullptr || sub >= 64u)) break;
        const D3 d = primary_dir_lds(P, cam, x, y, (int)(sub / (unsigned)P.SS) + 1, (int)(sub % (unsigned)P.SS) + 1);
#if RTM_TOL
        if (masks != nullptr && sub < 64u) {
            SceneGlobal sc;
            sc.v = P.scene;
            mask |= primary_tie_risk(sc, P.cam_org, d) ? (1ull << sub) : 0ull;
        }
#endif
        if (dirs != nullptr) store_dir(sub, d);
    }
#if RTM_TOL
    if (masks != nullptr) masks[(size_t)tile * 64 + (unsigned)lane] = mask;
#endif
}

}  // namespace RTM_NS
