// rtm_aov_kernel.h — first-hit feature buffers (AOVs) of a frame: depth, shading normal, albedo and object index behind
// every pixel (include/rtm.h: rtm_render_aov).  Included by rtm_kernels.hip, whose -ffp-contract=off build is the
// reference's own arithmetic.
//
// Primary rays have no jitter (src/Renderer.cpp:224-232), so a sub-pixel's ray is a fixed function of (x, y, sx, sy) and
// its nearest hit (:58-73) a fixed function of the scene: every value here is deterministic.  One wave per 8x8 tile,
// lane = pixel, each lane walks its SS^2 sub-pixels in the reference's loop order (sx outer, sy inner).  The scene loop is
// one of the render kernels' own nearest-hit searches (rtm_path.h), wave-uniform with scalar geometry loads:
//   kAovChunked  nearest_hit<MathFast, 8>: exact chunks of 8 spheres and a tail, planes through object_chunk
//   kAovGeneral  nearest_hit<MathRef, 1>: the general per-object loop (variant 1)
//   kAovGrid     nearest_hit_grid: the scene's uniform grid, one LDS candidate queue per block (variant 17)
#ifndef RTM_AOV_KERNEL_H
#define RTM_AOV_KERNEL_H
#include "rtm_render_kernel.h"

namespace rtm {

// SceneGlobal for scenes that hold planes: nearest_hit's chunked loop then takes object_chunk
struct SceneGlobalObjects : SceneGlobal {
    static constexpr bool kPlanes = true;
};

enum { kAovChunked = 0, kAovGeneral = 1, kAovGrid = 2 };
// Dynamic LDS of a block of aov_kernel, and of matte_kernel (rtm_matte_kernel.h) at matte_ss = SS: the grid walk's queue,
// then the 64 lanes' SS^2 object ids; aov_lds_bytes(search) is therefore where the id lists start
__host__ __device__ inline size_t aov_lds_bytes(int search, int matte_ss = 0) {
    return (search == kAovGrid ? GridWalk<MathFast, SceneGlobal>::queue_bytes(64) : 0) +
           (size_t)matte_ss * (size_t)matte_ss * 64 * sizeof(int);
}

// depth / object: the centre sub-pixel c = (SS + 1) / 2 in both axes; normal / albedo: the sums over the SS^2 sub-pixels in
// loop order, in double from +0, divided by SS^2 and rounded to float.  A miss adds nothing: +0 would leave the sum as it
// is, since a sum that starts at +0 is never -0.
template <int SEARCH, class Scene>
__global__ __launch_bounds__(64) void aov_kernel(const RenderParams P, const rtm_aov_buffers out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];  // kAovGrid: the walks' candidate queue
    const int lane = threadIdx.x;
    Scene sc;
    sc.v = P.scene;
    const int tile = (int)blockIdx.x;
    const int px = (tile % P.tiles_x) * 8 + (lane & 7), py = band_row(P, tile / P.tiles_x, lane >> 3);
    const bool valid = px < P.W && py < P.row_end;  // (a lane outside the frame traces a finite ray and stores nothing)
    const int c = (P.SS + 1) / 2;
    const bool repaired = P.mode != RTM_MODE_LITERAL;
    D3 nsum = d3(0, 0, 0), asum = d3(0, 0, 0);
    double depth = DBL_MAX;
    int object = -1;
    for (int sx = 1; sx <= P.SS; ++sx) {
        for (int sy = 1; sy <= P.SS; ++sy) {
            const D3 dir = primary_dir(P, px, py, sx, sy);  // :227-232
            double dis;
            int id;
            if constexpr (SEARCH == kAovGrid)
                id = nearest_hit_grid<MathFast, Scene>(sc, P.cam_org, dir, dis, lds_raw, 64, lane);
            else if constexpr (SEARCH == kAovGeneral)
                id = nearest_hit<MathRef, 1>(sc, P.cam_org, dir, dis);
            else
                id = nearest_hit<MathFast, 8>(sc, P.cam_org, dir, dis);
            if (sx == c && sy == c) {  // wave-uniform
                depth = dis;
                object = id;
            }
            if (id < 0) continue;
            // Intersect's normal (src/SettingData.cpp:214-215; a plane's m_normal), lost in literal mode (D2): vec3()
            D3 normal = d3(0, 0, 0);
            if (repaired) {
                const double* pl = sc.v.plane != nullptr && sc.v.geom[id].w < 0.0 ? sc.v.plane + (size_t)id * 16 : nullptr;
                normal = pl ? d3(pl[3], pl[4], pl[5]) : normalize((dir * dis + P.cam_org) - sc.center(id));  // :79
            }
            // :82-83 the orienting normal PathTracing holds: Dot(normal, dir) < 0 ? normal : normal * -1.0
            nsum = nsum + (dot(normal, dir) < 0.0 ? normal : normal * -1.0);
            const double* col = sc.v.surf + (size_t)id * 4;  // the raw material colour (rtm_scene::surf)
            asum = asum + d3(col[0], col[1], col[2]);
        }
    }
    if (!valid) return;
    const size_t pix = out_index(P, px, py) / 3;
    if (out.depth) out.depth[pix] = object < 0 ? __builtin_huge_valf() : (float)depth;
    if (out.object) out.object[pix] = object;
    const double n_sub = (double)(P.SS * P.SS);
    if (out.normal) {
        out.normal[pix * 3] = (float)(nsum.x / n_sub);
        out.normal[pix * 3 + 1] = (float)(nsum.y / n_sub);
        out.normal[pix * 3 + 2] = (float)(nsum.z / n_sub);
    }
    if (out.albedo) {
        out.albedo[pix * 3] = (float)(asum.x / n_sub);
        out.albedo[pix * 3 + 1] = (float)(asum.y / n_sub);
        out.albedo[pix * 3 + 2] = (float)(asum.z / n_sub);
    }
}

}  // namespace rtm
#endif
