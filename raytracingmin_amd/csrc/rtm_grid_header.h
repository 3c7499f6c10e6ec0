// rtm_grid_header.h — GridHeader, the head of a scene's uniform grid as the kernels read it and the builders write it.  Only
// HIP's vector types are needed: included by rtm_path.h (the kernels) and by rtm_scene_facts.h (the host builder).
#pragma once
#include <hip/hip_vector_types.h>

#ifndef RTM_NS
#define RTM_NS rtm
#endif

namespace RTM_NS {

// Uniform grid over a large scene's spheres (rtm_kernels.hip: build_scene_grid; rtm_path.h: nearest_hit_grid).  Device memory,
// read through wave-uniform scalar loads.  A sphere is listed in every cell its box — centre +- (radius + pad_i) —
// overlaps; the few spheres whose box would cover too many cells are in `big` instead and are tested by every ray.
struct GridHeader {
    double lo[3], hi[3];  // the grid's box: hi = lo + dim * h
    double h, inv_h;      // cell edge
    double cb[3], reach2; // a ray whose origin is farther than sqrt(reach2) from the box's centre cb, ...
    double dd_tol;        // ... or whose |dir.dir - 1| is larger, takes the exhaustive loop (the pads do not cover it)
    double t_ok;          // the largest hit parameter the pads were sized for (host side; reach2 follows from it)
    int dim[3];
    int n_big;
    unsigned n_recs, pad_;
    const uint2* cell_range;     // per cell (dim[0]*dim[1]*dim[2] of them): first and one-past-last entry of its list in `recs`
    const double4* recs;         // a cell's spheres, self-contained: (cx, cy, cz, r*r | index), ascending index within a cell
    const int* big;              // n_big sphere indices, ascending
};

}  // namespace RTM_NS
