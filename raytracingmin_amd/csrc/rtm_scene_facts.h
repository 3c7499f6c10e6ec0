// rtm_scene_facts.h — the host-only half of making a scene (rtm_scene_facts.cpp): flattening, the proofs behind
// SceneView::axis_pat / fold_flags / emit_mask, the axis rows, png::PlaneObject's row, the host grid builder and the scalar
// arithmetic it shares with the device build (rtm_grid_build.hip).  Plain C++: nothing here touches a device.  The host-only
// test hooks of all this (scene_facts_host ... grid_build_host) are declared in rtm_internal.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "rtm_internal.h"
#include "rtm_grid_exprs.h"
#include "rtm_grid_header.h"
#include "rtm_scene_flags.h"

namespace rtm {

// src/Ray.h / src/Renderer.cpp:202-208 on the host, same operation order as the device code
namespace host {
struct H3 {
    double x, y, z;
};
inline H3 sub(H3 a, H3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline H3 cross(H3 a, H3 b) {
    return {a.y * b.z - a.z * b.y, -a.x * b.z + a.z * b.x, a.x * b.y - a.y * b.x};
}
inline H3 normalize(H3 a) {
    const float len2 = (float)(a.x * a.x + a.y * a.y + a.z * a.z);
    const double m = (double)sqrtf(len2);
    return {a.x / m, a.y / m, a.z / m};
}
}  // namespace host

// Flatten rtm_sphere[] to the kernel layout (geom: 4 doubles per sphere, mat: 8 per sphere and the identity row, surf: 4)
void flatten_scene(const rtm_sphere* sp, size_t n, std::vector<double>& geom, std::vector<double>& mat,
                   std::vector<double>* surf = nullptr);
// png::PlaneObject's constructor on the host: the 16 doubles of SceneView::plane
void plane_row(const rtm_object& o, double row[16]);

// the axis rows a scene of n spheres keeps behind its n geometry rows: n of them, or none beyond kAxisRowsMax spheres
inline size_t axis_row_count(size_t n) { return n <= kAxisRowsMax ? n : 0; }
// Everything the host proves about a scene from its flattened rows, for host and device sphere arrays alike: the ONE place
// the proofs are put together.
struct SceneFacts {
    uint64_t axis_pat = 0;              // SceneView::axis_pat
    unsigned fold_flags = 0;            // SceneView::fold_flags: every proven bit
    uint64_t emit_mask = ~(uint64_t)0;  // SceneView::emit_mask
};
// geom: n rows of 4, mat: n rows of 8; axis_rows_out: axis_row_count(n) rows of 4, filled (may alias nothing of geom's n rows)
SceneFacts scene_facts(const double* geom, const double* mat, size_t n, double* axis_rows_out);

// ---- the uniform grid of a large scene, built on the host ----------------------------------------------------------
double grid_cells_per_sphere();  // RTM_DEBUG_GRID_CELLS, else 1.5
struct GridBuild {
    GridHeader hdr;
    std::vector<unsigned> cell_start, items;
    std::vector<int> big;
    size_t refs = 0;  // entries of `items` that are real (items holds one dummy when there is none)
};
inline bool n_refs_valid(const GridBuild& B) { return B.refs != 0; }
// The scalar arithmetic of a build, host code for the host builder and for the device build (rtm_grid_build.hip) alike.
bool grid_round_scalars(const double lo[3], const double hi[3], size_t n_small, double lambda, double& h, double& t_ok);
bool grid_header_from_box(double lo[3], const double hi[3], double h, double t_ok, size_t n, size_t n_big, GridHeader& H,
                          size_t* cells_out);
GridBuildDims grid_build_dims(const GridHeader& H);
// g: n geometry rows.  false: the scene gets no grid.  pads_out (optional): n doubles
bool make_grid(const double* g, size_t n, GridBuild& out, double* pads_out = nullptr);

// A diffuse sphere that ENCLOSES the gridded ones from farther away than the pads reach (an environment sphere) sends
// its bounces back from origins the walk cannot serve: each of them would take the exhaustive loop inside the grid
// kernel, one lane at a time.  Such a scene keeps its grid for variant 17 by name; variant 0 leaves it alone (grid_for).
// Decided from the rows of the spheres every ray tests: row_of(j, i) = the geometry row of big[j] = i, diffuse_of(j, i) = its
// kd > 0 — the host builder reads them from its tables, the device build from the few rows that came back.  1 / 0, or -1
// where a plane is among them and there are no plane rows to judge it by (the scene then gets no grid).
template <typename RowOf, typename DiffuseOf>
int grid_far_bounces_of(const GridHeader& H, const int* big, size_t n_big, const double* plane_rows, RowOf row_of,
                        DiffuseOf diffuse_of) {
    int far = 0;
    const double reach = std::sqrt(H.reach2);
    for (size_t j = 0; j < n_big; ++j) {
        const int i = big[j];
        const double* row = row_of(j, i);
        const bool diffuse = diffuse_of(j, i);
        if (row[3] < 0.0) {  // a plane: any of its square's corners beyond the reach?
            if (!plane_rows) return -1;
            const double* pl = plane_rows + (size_t)i * 16;
            for (int c = 0; c < 4 && diffuse; ++c) {
                double d2 = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double p = pl[k] + ((c & 1) ? pl[6 + k] : -pl[6 + k]) + ((c & 2) ? pl[9 + k] : -pl[9 + k]);
                    d2 += (p - H.cb[k]) * (p - H.cb[k]);
                }
                if (!(std::sqrt(d2) <= reach)) far = 1;
            }
            continue;
        }
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) d2 += (row[k] - H.cb[k]) * (row[k] - H.cb[k]);
        if (diffuse && std::sqrt(row[3]) - std::sqrt(d2) > reach) far = 1;
    }
    return far;
}
// Where the tables of a grid lie in an rtm_scene's `grid` block: the header, the cells' ranges, the records, the big list
struct GridLayout {
    size_t off_cs, off_items, off_big, bytes;
};
GridLayout grid_layout(size_t n_cells, size_t n_recs, size_t n_big);

}  // namespace rtm
