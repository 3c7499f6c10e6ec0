// rtm_grid_exprs.h — the per-sphere expressions of a uniform grid's build, shared by the host builder (rtm_scene_facts.cpp:
// make_grid) and the device build's kernels (rtm_grid_build_kernel.h).
//
// One source of truth: every per-sphere value — R, the pad, the "big" test, a sphere's cell range per axis, the slab gap and
// its reach — is one of the inline functions below, called by make_grid on the host and by the kernels.  Both are
// compiled with -ffp-contract=off, and sqrt / division / floor of doubles are correctly rounded on both sides, so a sphere gets
// the same bits from either.  No kernel here: a plain C++ unit includes this file too (it needs HIP's include directory and
// -D__HIP_PLATFORM_AMD__ for the header below, which gives it __host__ __device__).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace rtm {

constexpr int kGridBigCells = 125;   // a sphere whose padded box covers more cells goes to the list every ray tests
constexpr double kGridDdTol = 4e-7;  // |dir.dir - 1| the pads cover: twice what the reference's float-sqrt Normalize leaves (1.8e-7)

// ---- the per-sphere expressions ------------------------------------------------------------------------------------------
// radius from the stored float product r*r (a plane's row has a negative one: it is tested by every ray, R = 0)
__host__ __device__ inline double grid_sphere_R(double w) { return w < 0.0 ? 0.0 : sqrt(w); }
// (rtm_path.h: a hit at parameter t lies sqrt(r^2 + t^2 (d.d - 1)) from the centre)
__host__ __device__ inline double grid_sphere_pad(double R, double h, double t_ok) {
    return 0.05 * h + (sqrt(R * R + kGridDdTol * t_ok * t_ok) - R) + 1e-6 * t_ok;
}
__host__ __device__ inline bool grid_sphere_is_big(double R, double pad, double h) {
    const double side = 2.0 * (R + pad) / h + 1.0;
    return !(side * side * side <= (double)kGridBigCells);
}
// the cells [a, b] along one axis that the padded sphere's box touches: centre coordinate c, e = R + pad
__host__ __device__ inline void grid_cell_range(double c, double e, double lo, double h, int dim, int& a, int& b) {
    a = (int)floor((c - e - lo) / h);
    b = (int)floor((c + e - lo) / h);
    a = a < 0 ? 0 : a;
    b = b >= dim ? dim - 1 : b;
}
// of the box's cells, those within R + pad of the centre get the sphere (a hit point is, and lies in its cell)
__host__ __device__ inline double grid_sphere_reach2(double e) { return e * e * (1.0 + 1e-9); }
// distance from the centre's coordinate ck to the cell's slab along one axis
__host__ __device__ inline double grid_slab_gap(double ck, double lo, double h, int cell) {
    const double c0 = lo + (double)cell * h;
    return ck < c0 ? c0 - ck : (ck > c0 + h ? ck - (c0 + h) : 0.0);
}

// what the list stages need of a GridHeader
struct GridBuildDims {
    double lo[3], h;
    int dim[3];
};
// The cells of one small sphere, in the host's order (x fastest): calls emit(cell) for each, returns their number.
template <typename Emit>
__host__ __device__ inline unsigned grid_sphere_cells(const double g[4], double pad, const GridBuildDims& D, Emit emit) {
    const double R = grid_sphere_R(g[3]), e = R + pad;
    int a[3], b[3];
    for (int k = 0; k < 3; ++k) grid_cell_range(g[k], e, D.lo[k], D.h, D.dim[k], a[k], b[k]);
    const double reach2 = grid_sphere_reach2(e);
    unsigned count = 0;
    for (int z = a[2]; z <= b[2]; ++z)
        for (int y = a[1]; y <= b[1]; ++y)
            for (int x = a[0]; x <= b[0]; ++x) {
                const double gx = grid_slab_gap(g[0], D.lo[0], D.h, x), gy = grid_slab_gap(g[1], D.lo[1], D.h, y),
                             gz = grid_slab_gap(g[2], D.lo[2], D.h, z);
                if (gx * gx + gy * gy + gz * gz > reach2) continue;
                emit(((size_t)z * D.dim[1] + y) * D.dim[0] + x);
                ++count;
            }
    return count;
}

}  // namespace rtm
