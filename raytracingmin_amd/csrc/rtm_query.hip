// rtm_query.hip — ray queries on a scene object (include/rtm.h: rtm_scene_nearest, rtm_scene_occluded; include/rtm_debug.h:
// rtm_debug_scene_query): the argument checks and the launches of rtm_query_kernel.h.  NOT a translation unit of its own:
// rtm_scene, the (device, stream) contexts and note_scene_use are private to rtm_kernels.hip, which includes this file at
// its end.
//
// The contract is rtm_render_aov's (begin_first_hit): every argument is checked before anything touches a device; then the
// call only enqueues one launch on the caller's stream on the scene's device, serialised with the other calls on that
// (device, stream), and records a use of the scene.  Nothing is allocated, copied or waited for.
#include "rtm_query_kernel.h"

namespace rtm {

namespace {
bool misaligned(const void* p, size_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// The checks the three entries share, in the order the header lists them; the scene is not looked into.
int check_query(const rtm_scene* scene, const double* org, const double* dir, const double* tmax, size_t n_rays) {
    if (!scene) return invalid("null scene");
    if (!org || !dir) return invalid("null org_dev or dir_dev");
    if (misaligned(org, 8) || misaligned(dir, 8) || misaligned(tmax, 8))
        return invalid("org_dev, dir_dev or tmax_dev is not 8-byte aligned");
    if (n_rays > 0x7FFFFFFFull) return invalid("n_rays = " + std::to_string(n_rays) + ": more than 2^31 - 1 rays");
    return RTM_OK;
}

template <int SEARCH, class Scene, bool ANY, bool COUNT>
void launch_query_as(const SceneView& view, const double* org, const double* dir, const double* tmax, unsigned n_rays,
                     const QueryOut& out, hipStream_t stream) {
    query_kernel<SEARCH, Scene, ANY, COUNT><<<(n_rays + kQueryBlock - 1) / kQueryBlock, kQueryBlock, query_lds_bytes(SEARCH), stream>>>(
        view, org, dir, tmax, n_rays, out);
}

// The launch for checked arguments and n_rays > 0.  any: the occlusion walk's early exit, where the scene has a grid (a
// scene without one answers out.occluded from its nearest hit: its loop is over all objects anyway).  count: the grid
// walk's counting instantiations (rtm_debug_scene_query; the caller has refused a scene without a grid).
int enqueue_query(const char* stage, const rtm_scene* scene, bool any, bool count, const double* org, const double* dir,
                  const double* tmax, size_t n_rays, const QueryOut& out, hipStream_t stream) {
    std::shared_lock<std::shared_mutex> gate(g_gate);
    reap_scenes(false);
    RTM_HIP_CHECK(hipSetDevice(scene->device));
    std::unique_lock<std::mutex> ctx_lock(get_ctx(scene->device, stream)->mu);
    // the grid whenever the scene has one: there is no camera to ask grid_for about, and the walk's own guard (reach2,
    // dd_tol) sends every ray it cannot serve through the exhaustive loop
    const SceneView view = view_of(*scene, scene->grid.p);
    const unsigned n = (unsigned)n_rays;
    if (scene->grid.p) {
        if (count) {
            if (any)
                launch_query_as<kQueryGrid, SceneGlobal, true, true>(view, org, dir, tmax, n, out, stream);
            else
                launch_query_as<kQueryGrid, SceneGlobal, false, true>(view, org, dir, tmax, n, out, stream);
        } else if (any) {
            launch_query_as<kQueryGrid, SceneGlobal, true, false>(view, org, dir, tmax, n, out, stream);
        } else {
            launch_query_as<kQueryGrid, SceneGlobal, false, false>(view, org, dir, tmax, n, out, stream);
        }
    } else if (scene->has_planes) {
        launch_query_as<kQueryChunked, SceneGlobalObjects, false, false>(view, org, dir, tmax, n, out, stream);
    } else {
        launch_query_as<kQueryChunked, SceneGlobal, false, false>(view, org, dir, tmax, n, out, stream);
    }
    const int rc = launched(stage);
    note_scene_use(scene, stream);
    return rc;
}
}  // namespace

int scene_nearest(const rtm_scene* scene, const double* org, const double* dir, size_t n_rays, const rtm_hit_buffers* out,
                  void* stream_v) {
    if (!out) return invalid("out_dev: the buffer set is null");
    if (!out->object && !out->t && !out->normal) return invalid("out_dev: every plane is null");
    if (misaligned(out->object, 4) || misaligned(out->t, 8) || misaligned(out->normal, 8))
        return invalid("out_dev: object is not 4-byte aligned, or t or normal not 8-byte aligned");
    if (const int rc = check_query(scene, org, dir, nullptr, n_rays); rc != RTM_OK) return rc;
    if (n_rays == 0) return RTM_OK;
    const QueryOut q{out->object, out->t, out->normal, nullptr, nullptr, nullptr};
    return enqueue_query("ray query (nearest)", scene, false, false, org, dir, nullptr, n_rays, q, (hipStream_t)stream_v);
}

int scene_occluded(const rtm_scene* scene, const double* org, const double* dir, const double* tmax, size_t n_rays, uint8_t* out,
                   void* stream_v) {
    if (!out) return invalid("null out_dev");
    if (const int rc = check_query(scene, org, dir, tmax, n_rays); rc != RTM_OK) return rc;
    if (n_rays == 0) return RTM_OK;
    const QueryOut q{nullptr, nullptr, nullptr, out, nullptr, nullptr};
    return enqueue_query("ray query (occluded)", scene, true, false, org, dir, tmax, n_rays, q, (hipStream_t)stream_v);
}

// rtm_debug_scene_query: either walk through GridWalk's counting instantiation, with the sphere tests and cell steps per ray
int scene_query_probe(const rtm_scene* scene, int any, const double* org, const double* dir, const double* tmax, size_t n_rays,
                      int32_t* out_object, double* out_t, uint8_t* out_occluded, uint32_t* out_tests, uint32_t* out_steps,
                      void* stream_v) {
    if (any != 0 && any != 1) return invalid("any is neither 0 nor 1");
    if (!out_object && !out_t && !out_occluded && !out_tests && !out_steps) return invalid("every output is null");
    if (misaligned(out_object, 4) || misaligned(out_t, 8) || misaligned(out_tests, 4) || misaligned(out_steps, 4))
        return invalid("an output is not aligned to its element");
    if (const int rc = check_query(scene, org, dir, tmax, n_rays); rc != RTM_OK) return rc;
    if (!scene->grid.p) return unsupported("this scene has no grid");
    if (n_rays == 0) return RTM_OK;
    const QueryOut q{out_object, out_t, nullptr, out_occluded, out_tests, out_steps};
    return enqueue_query("ray query (counting)", scene, any != 0, true, org, dir, tmax, n_rays, q, (hipStream_t)stream_v);
}

}  // namespace rtm
