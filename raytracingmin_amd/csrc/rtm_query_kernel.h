// rtm_query_kernel.h — ray queries on a scene object (include/rtm.h: rtm_scene_nearest, rtm_scene_occluded;
// include/rtm_debug.h: rtm_debug_scene_query): the nearest-hit loop of src/Renderer.cpp:58-73 for rays of the caller's, and
// the question "is there any hit before tmax".  Included by rtm_query.hip, which is part of rtm_kernels.hip's translation
// unit: its -ffp-contract=off build is the reference's own arithmetic.
//
// One lane per ray, one wave per block ("Ray queries", says why 64).  The search is one of the render kernels'
// own (rtm_path.h), chosen by the host as aov_kernel's is:
//   kQueryGrid     GridWalk over the scene's uniform grid, its candidate queue in LDS; a ray the grid cannot serve (an origin
//                  beyond reach2, |d.d - 1| > dd_tol) sends its wave through the walk's exhaustive loop
//   kQueryChunked  nearest_hit<MathFast, 8>: every object, planes through object_chunk (SceneGlobalObjects)
// Every lane of a wave stays in the searches' wave-uniform loops and ballots: a lane past n_rays traces the last ray again
// and stores nothing.
#ifndef RTM_QUERY_KERNEL_H
#define RTM_QUERY_KERNEL_H
#include "rtm_aov_kernel.h"

namespace rtm {

constexpr int kQueryBlock = 64;
enum { kQueryGrid = 0, kQueryChunked = 1 };

// DEVICE pointers, each may be null.  tests / steps: the counting instantiations only.
struct QueryOut {
    int32_t* object;
    double* t;
    double* normal;
    uint8_t* occluded;
    unsigned* tests;
    unsigned* steps;
};

__host__ __device__ inline size_t query_lds_bytes(int search) {
    return search == kQueryGrid ? GridWalk<MathFast, SceneGlobal>::queue_bytes(kQueryBlock) : 0;
}

// ANY (kQueryGrid only): the walk starts from dis = the ray's limit and ends at its first acceptance (rtm_path.h, above
// kGridBatch); out.object / out.t then name that hit, which need not be the nearest.  !ANY: the nearest hit, and
// out.occluded = its t < tmax.
// tmax null: every hit counts.  A limit that is NaN, zero or negative admits nothing.
template <int SEARCH, class Scene, bool ANY, bool COUNT>
__global__ __launch_bounds__(kQueryBlock) void query_kernel(const SceneView scene, const double* __restrict__ org,
                                                            const double* __restrict__ dir, const double* __restrict__ tmax,
                                                            const unsigned n_rays, const QueryOut out) {
    static_assert(SEARCH == kQueryGrid || (!ANY && !COUNT), "the early exit and the counts are the grid walk's");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];  // kQueryGrid: the walks' candidate queue
    const unsigned lane = threadIdx.x;
    const unsigned i = blockIdx.x * (unsigned)kQueryBlock + lane;
    const size_t r = i < n_rays ? i : n_rays - 1u;
    Scene sc;
    sc.v = scene;
    const D3 o = d3(org[r * 3], org[r * 3 + 1], org[r * 3 + 2]);
    const D3 d = d3(dir[r * 3], dir[r * 3 + 1], dir[r * 3 + 2]);
    const double lim = tmax != nullptr ? tmax[r] : __builtin_huge_val();
    double dis;
    int id;
    unsigned tests = 0, steps = 0;
    if constexpr (SEARCH == kQueryGrid) {
        if constexpr (ANY) {
            // an accepted t is below DBL_MAX in the nearest loop (its dis starts there), so the limit is min(tmax, DBL_MAX)
            dis = lim > 0.0 ? (lim < DBL_MAX ? lim : DBL_MAX) : 0.0;
            id = any_hit_grid<MathFast, Scene, COUNT>(sc, o, d, dis, lds_raw, kQueryBlock, (int)lane, &tests, &steps);
        } else {
            id = nearest_hit_grid<MathFast, Scene, COUNT>(sc, o, d, dis, lds_raw, kQueryBlock, (int)lane, &tests, &steps);
        }
    } else {
        id = nearest_hit<MathFast, 8>(sc, o, d, dis);
    }
    if (i >= n_rays) return;
    if (out.object) out.object[i] = id;
    if (out.t) out.t[i] = id < 0 ? __builtin_huge_val() : dis;
    if (out.occluded) out.occluded[i] = (ANY ? id >= 0 : (id >= 0 && dis < lim)) ? 1 : 0;
    if (out.normal) {
        // Intersect's out_normal in repaired mode (src/SettingData.cpp:214-215; a plane's m_normal), as aov_kernel forms it
        D3 normal = d3(0, 0, 0);
        if (id >= 0) {
            const double* pl = sc.v.plane != nullptr && sc.v.geom[id].w < 0.0 ? sc.v.plane + (size_t)id * 16 : nullptr;
            normal = pl ? d3(pl[3], pl[4], pl[5]) : normalize((d * dis + o) - sc.center(id));
        }
        out.normal[(size_t)i * 3] = normal.x;
        out.normal[(size_t)i * 3 + 1] = normal.y;
        out.normal[(size_t)i * 3 + 2] = normal.z;
    }
    if constexpr (COUNT) {
        if (out.tests) out.tests[i] = tests;
        if (out.steps) out.steps[i] = steps;
    }
}

}  // namespace rtm
#endif
