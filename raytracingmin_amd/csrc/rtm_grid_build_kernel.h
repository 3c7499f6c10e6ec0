// rtm_grid_build_kernel.h — the uniform grid of a large scene (rtm_grid_header.h: GridHeader) built ON THE DEVICE from the
// flattened geometry rows (cx, cy, cz, float r*r): the kernels behind rtm_scene_create_device (rtm_grid_build.hip is their driver).
//
// The per-sphere expressions they share with the host builder (rtm_scene_facts.cpp: make_grid) are in rtm_grid_exprs.h, which says
// why a sphere gets the same bits from either.  The scalar arithmetic of a build (the cell edge with its cbrt, t_ok, the dims,
// the header) is host code for both paths (rtm_scene_facts.cpp: grid_round_scalars, grid_header_from_box).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rtm_grid_exprs.h"

namespace rtm {

// ---- stage 1: a classification round ----------------------------------------------------------------------------------------
// What one round reduces the spheres to.  `bad`: rows that are not finite or whose r*r has bits in the 29 the records keep the
// index in; lo / hi: the box of the spheres that are not big AFTER this round's classification; plo / phi: the same with the
// round's pads (the grid's box when this round turns out to be the last).
//
// min / max are order-free except for the sign of a zero, and the folds below take whichever of -0 / +0 their fixed tree
// meets first, which need not be the one the host's left-to-right std::min / std::max keeps.  No later value depends on it:
// lo / hi enter the host's arithmetic only as ext = hi - lo — whose own zero sign vanishes in ext * ext, in
// max(longest, ext) (longest starts as +0 and std::max keeps its first argument on a tie) and in max(ext, longest * 1e-3)
// with longest > 0 —, and plo / phi only as plo - 0.01 h and phi + 0.01 h - (plo - 0.01 h) with 0.01 h > 0 (h >= longest / 1022 >
// 0; 0.01 h rounds to zero only for scenes under 1e-319 across, where the host's own conversions to int are undefined).
struct GridRound {
    double lo[3], hi[3], plo[3], phi[3];
    unsigned long long n_small, changed, bad;
};
constexpr int kGridBuildBlock = 256;       // threads per block of every kernel here (4 waves of 64)
constexpr int kGridRoundMaxBlocks = 1024;  // partial results of a round: folded by one block of the second kernel

__device__ inline void grid_round_merge(GridRound& a, const GridRound& b) {
    for (int k = 0; k < 3; ++k) {
        a.lo[k] = b.lo[k] < a.lo[k] ? b.lo[k] : a.lo[k];
        a.hi[k] = b.hi[k] > a.hi[k] ? b.hi[k] : a.hi[k];
        a.plo[k] = b.plo[k] < a.plo[k] ? b.plo[k] : a.plo[k];
        a.phi[k] = b.phi[k] > a.phi[k] ? b.phi[k] : a.phi[k];
    }
    a.n_small += b.n_small;
    a.changed += b.changed;
    a.bad += b.bad;
}
__device__ inline GridRound grid_round_identity() {
    GridRound r;
    for (int k = 0; k < 3; ++k) {
        r.lo[k] = r.plo[k] = HUGE_VAL;
        r.hi[k] = r.phi[k] = -HUGE_VAL;
    }
    r.n_small = r.changed = r.bad = 0;
    return r;
}
// a block's threads fold their values through LDS, pairwise in a fixed order: thread 0 returns the block's
__device__ inline GridRound grid_round_block_fold(GridRound v, GridRound* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = kGridBuildBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            GridRound a = lds[threadIdx.x];
            grid_round_merge(a, lds[threadIdx.x + s]);
            lds[threadIdx.x] = a;
        }
        __syncthreads();
    }
    return lds[0];
}
// classify = 0: the round before the first (flags = "is a plane", the finite check, the box of the rest);
// classify = 1: the host loop's classification with the round's h and t_ok, and the boxes of what it leaves small.
// flags[i] = 1: sphere i is tested by every ray.  Grid-stride over the spheres; partial[blockIdx.x] gets the block's fold.
__global__ __launch_bounds__(kGridBuildBlock) void grid_round_kernel(const double4* __restrict__ geom, unsigned n,
                                                                     unsigned* __restrict__ flags, int classify, double h,
                                                                     double t_ok, GridRound* __restrict__ partial) {
    __shared__ GridRound lds[kGridBuildBlock];
    GridRound acc = grid_round_identity();
    for (size_t i = (size_t)blockIdx.x * kGridBuildBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kGridBuildBlock) {
        const double4 g = geom[i];
        const bool plane = g.w < 0.0;
        if (!classify) {
            const unsigned long long wbits = (unsigned long long)__double_as_longlong(g.w);
            const bool finite = isfinite(g.x) && isfinite(g.y) && isfinite(g.z) && isfinite(g.w);
            acc.bad += (!finite || (!plane && (wbits & 0x1FFFFFFFull) != 0ull)) ? 1u : 0u;
        }
        const double R = grid_sphere_R(g.w);
        const double pad = classify ? grid_sphere_pad(R, h, t_ok) : 0.0;
        const bool big = plane || (classify && grid_sphere_is_big(R, pad, h));
        if (classify) acc.changed += (big ? 1u : 0u) != flags[i] ? 1u : 0u;
        flags[i] = big ? 1u : 0u;
        if (big) continue;
        ++acc.n_small;
        const double c[3] = {g.x, g.y, g.z};
        for (int k = 0; k < 3; ++k) {
            const double a = c[k] - R, b = c[k] + R, pa = c[k] - R - pad, pb = c[k] + R + pad;
            acc.lo[k] = a < acc.lo[k] ? a : acc.lo[k];
            acc.hi[k] = b > acc.hi[k] ? b : acc.hi[k];
            acc.plo[k] = pa < acc.plo[k] ? pa : acc.plo[k];
            acc.phi[k] = pb > acc.phi[k] ? pb : acc.phi[k];
        }
    }
    const GridRound r = grid_round_block_fold(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
// one block: the partials' fold, in a fixed order
__global__ __launch_bounds__(kGridBuildBlock) void grid_round_fold_kernel(const GridRound* __restrict__ partial, unsigned n_partial,
                                                                          GridRound* __restrict__ out) {
    __shared__ GridRound lds[kGridBuildBlock];
    GridRound acc = grid_round_identity();
    for (unsigned i = threadIdx.x; i < n_partial; i += kGridBuildBlock) grid_round_merge(acc, partial[i]);
    const GridRound r = grid_round_block_fold(acc, lds);
    if (threadIdx.x == 0) *out = r;
}

// ---- stages 3 and 4: a small sphere's cells, counted and then written as sortable keys ----------------------------------------
// count[i] = the number of cells sphere i goes to (0 for a big one); count[n] = 0 so that an exclusive scan over n + 1 values
// leaves the total behind the offsets.
__global__ __launch_bounds__(kGridBuildBlock) void grid_count_kernel(const double4* __restrict__ geom, unsigned n,
                                                                     const unsigned* __restrict__ flags, GridBuildDims D,
                                                                     double t_ok, unsigned* __restrict__ count) {
    const size_t i = (size_t)blockIdx.x * kGridBuildBlock + threadIdx.x;
    if (i > n) return;
    unsigned c = 0;
    if (i < n && !flags[i]) {
        const double4 g4 = geom[i];
        const double g[4] = {g4.x, g4.y, g4.z, g4.w};
        c = grid_sphere_cells(g, grid_sphere_pad(grid_sphere_R(g4.w), D.h, t_ok), D, [](size_t) {});
    }
    count[i] = c;
}
// keys[offset[i] + j] = cell << 32 | i for the j-th cell of sphere i.  The walk is the count kernel's, so it writes exactly
// offset[i + 1] - offset[i] keys; every store is checked against that end and the counted total all the same.
__global__ __launch_bounds__(kGridBuildBlock) void grid_fill_kernel(const double4* __restrict__ geom, unsigned n,
                                                                    const unsigned* __restrict__ flags, GridBuildDims D, double t_ok,
                                                                    const unsigned long long* __restrict__ offset,
                                                                    unsigned long long total, unsigned long long* __restrict__ keys) {
    const size_t i = (size_t)blockIdx.x * kGridBuildBlock + threadIdx.x;
    if (i >= n || flags[i]) return;
    const double4 g4 = geom[i];
    const double g[4] = {g4.x, g4.y, g4.z, g4.w};
    unsigned long long at = offset[i];
    const unsigned long long end = offset[i + 1] < total ? offset[i + 1] : total;
    grid_sphere_cells(g, grid_sphere_pad(grid_sphere_R(g4.w), D.h, t_ok), D, [&](size_t cell) {
        if (at < end) keys[at] = ((unsigned long long)cell << 32) | (unsigned long long)i;
        ++at;
    });
}

// ---- stage 5: a cell's range in the sorted keys -------------------------------------------------------------------------------
// first key that is not below `key`
__device__ inline unsigned grid_lower_bound(const unsigned long long* __restrict__ keys, unsigned total, unsigned long long key) {
    unsigned lo = 0, hi = total;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// range[c] = (first, one past last) entry of cell c: an empty cell gets (x, x) with x the entries of the cells before it,
// which is what the host's counting sort leaves there
__global__ __launch_bounds__(kGridBuildBlock) void grid_ranges_kernel(const unsigned long long* __restrict__ keys, unsigned total,
                                                                      unsigned long long cells, uint2* __restrict__ range) {
    const unsigned long long c = (unsigned long long)blockIdx.x * kGridBuildBlock + threadIdx.x;
    if (c >= cells) return;
    range[c] = make_uint2(grid_lower_bound(keys, total, c << 32), grid_lower_bound(keys, total, (c + 1) << 32));
}

// ---- stage 6: the self-contained records ------------------------------------------------------------------------------------
// recs[k] = the geometry row of entry k's sphere with its index in r*r's 29 zero mantissa bits; without entries (total = 0,
// n_recs = 1) the one dummy record the host keeps: row 0 with index 0
__global__ __launch_bounds__(kGridBuildBlock) void grid_records_kernel(const double4* __restrict__ geom, unsigned n,
                                                                       const unsigned long long* __restrict__ keys, unsigned total,
                                                                       unsigned n_recs, double4* __restrict__ recs) {
    const size_t k = (size_t)blockIdx.x * kGridBuildBlock + threadIdx.x;
    if (k >= n_recs) return;
    unsigned i = k < total ? (unsigned)(keys[k] & 0xFFFFFFFFull) : 0u;
    if (i >= n) i = 0u;  // (never: the keys were made from indices below n)
    double4 row = geom[i];
    row.w = __longlong_as_double(__double_as_longlong(row.w) | (long long)i);
    recs[k] = row;
}

// ---- stage 7: the ascending list of the spheres every ray tests ---------------------------------------------------------------
// big[offset[i]] = i for every flagged sphere (offset: the exclusive scan of the flags); rows[5 j ..] = that sphere's geometry
// row and kd, which the host's grid_far_bounces decision reads
__global__ __launch_bounds__(kGridBuildBlock) void grid_big_kernel(const double4* __restrict__ geom, const double* __restrict__ mat,
                                                                   unsigned n, const unsigned* __restrict__ flags,
                                                                   const unsigned* __restrict__ offset, unsigned n_big,
                                                                   int* __restrict__ big, double* __restrict__ rows) {
    const size_t i = (size_t)blockIdx.x * kGridBuildBlock + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const unsigned j = offset[i];
    if (j >= n_big) return;
    big[j] = (int)i;
    const double4 g = geom[i];
    rows[(size_t)j * 5 + 0] = g.x;
    rows[(size_t)j * 5 + 1] = g.y;
    rows[(size_t)j * 5 + 2] = g.z;
    rows[(size_t)j * 5 + 3] = g.w;
    rows[(size_t)j * 5 + 4] = mat[i * 8 + 6];
}

}  // namespace rtm
