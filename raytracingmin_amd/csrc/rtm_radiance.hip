// rtm_radiance.hip — radiance queries on a scene object (include/rtm.h: rtm_scene_radiance): the argument checks, the record
// pool and the launches of rtm_radiance_kernel.h.  NOT a translation unit of its own: rtm_scene, the (device, stream)
// contexts and note_scene_use are private to rtm_kernels.hip, which includes this file at its end, behind rtm_query.hip.
//
// The contract is the ray queries' (rtm_query.hip): every argument is checked before anything touches a device; then the call
// only enqueues on the caller's stream on the scene's device, serialised with the other calls on that (device, stream), and
// records a use of the scene.  One addition: a call whose paths may run deeper than the kernel's on-chip record levels takes
// the stream context's record pool exactly as a render does (render_view), and RTM_MODE_HOST_TRIG the device's trig table —
// whichever call needs either first sets it up, which may allocate and wait once.
#include "rtm_radiance_kernel.h"

namespace rtm {

namespace {
// does a path of this call stay within the kernel's LDS record levels?  (a cap of k bounces pushes levels 0 .. k - 1)
bool radiance_stays_on_chip(int max_bounces) { return max_bounces >= 0 && max_bounces <= kRadianceLdsLevels; }
// lanes of one launch of a call that takes the record pool, and the pool's slots at most: 4 096 waves, the wave slots of 256
// CUs at the kernel's 16 waves per CU (960 MiB of records at that size)
constexpr unsigned kRadiancePoolLanes = 262144u;

template <int SEARCH, class Scene>
void launch_radiance_as(RenderParams& P, const RadianceArgs& A, hipStream_t stream) {
    size_t lds = radiance_lds_bytes(SEARCH, false);
    P.unit_tab = unit_table_fits(lds) ? 1u : 0u;
    if (P.unit_tab) lds = radiance_lds_bytes(SEARCH, true);
    radiance_kernel<SEARCH, Scene><<<(A.n_rays + kQueryBlock - 1) / kQueryBlock, kQueryBlock, lds, stream>>>(P, A);
}
}  // namespace

int scene_radiance(const rtm_scene* scene, const double* org, const double* dir, size_t n_rays, const rtm_radiance_params* prm,
                   const rtm_radiance_buffers* out, void* stream_v) {
    if (!prm) return invalid("null params");
    if (!out) return invalid("out_dev: the buffer set is null");
    if (!out->radiance && !out->casts && !out->draws) return invalid("out_dev: every plane is null");
    if (misaligned(out->radiance, 8) || misaligned(out->casts, 4) || misaligned(out->draws, 4))
        return invalid("out_dev: radiance is not 8-byte aligned, or casts or draws not 4-byte aligned");
    if (const int rc = check_query(scene, org, dir, nullptr, n_rays); rc != RTM_OK) return rc;
    if ((uint64_t)prm->key_base + (uint64_t)n_rays > 0x100000000ull)
        return invalid("key_base + n_rays = " + std::to_string((uint64_t)prm->key_base + (uint64_t)n_rays) + ": stream keys end at 2^32");
    if (prm->samples == 0) return invalid("samples = 0: a ray takes at least one sample");
    if (prm->max_bounces < -1) return invalid("max_bounces = " + std::to_string(prm->max_bounces) + ": -1 (unlimited) or a cap >= 0");
    if (prm->max_bounces > kRadianceLdsLevels + kPoolLevels)
        return unsupported("max_bounces exceeds the hit-record capacity (976); use -1 for unlimited");
    if ((prm->flags & ~RTM_RADIANCE_CLAMP) != 0u) return invalid("flags: unknown bits (RTM_RADIANCE_CLAMP or 0)");
    if (prm->reserved != 0u) return invalid("reserved is not 0");
    if (prm->mode & RTM_MODE_SURFACE_SAMPLE)
        return unsupported("RTM_MODE_SURFACE_SAMPLE: a radiance query is png::PathTracing; png::SurfaeSample is served by renders only");
    if ((prm->mode & ~RTM_MODE_HOST_TRIG) != RTM_MODE_LITERAL && (prm->mode & ~RTM_MODE_HOST_TRIG) != RTM_MODE_REPAIRED)
        return invalid("unknown mode (RTM_MODE_LITERAL or RTM_MODE_REPAIRED, optionally | RTM_MODE_HOST_TRIG)");
    if (n_rays == 0) return RTM_OK;

    hipStream_t stream = (hipStream_t)stream_v;
    std::shared_lock<std::shared_mutex> gate(g_gate);
    reap_scenes(false);
    RTM_HIP_CHECK(hipSetDevice(scene->device));
    StreamCtx& ctx = *get_ctx(scene->device, stream);
    std::unique_lock<std::mutex> ctx_lock(ctx.mu);

    RenderParams P;
    std::memset(&P, 0, sizeof P);
    // the grid whenever the scene has one, as enqueue_query takes it: the walk's own guard serves what the grid cannot
    P.scene = view_of(*scene, scene->grid.p);
    if (prm->mode & RTM_MODE_HOST_TRIG) {
        const uint32_t* fix = nullptr;
        if (const int rc = ensure_trig_fix(scene->device, &fix); rc != RTM_OK) return rc;
        P.scene.trig_fix = fix;
    }
    P.mode = prm->mode & ~RTM_MODE_HOST_TRIG;
    P.max_bounces = prm->max_bounces;
    P.seed_mult = seed_multiplier(prm->seed);

    RadianceArgs A;
    std::memset(&A, 0, sizeof A);
    A.samples = prm->samples;
    A.clamp = prm->flags & RTM_RADIANCE_CLAMP;
    A.dS = (double)prm->samples;  // (the rays, their keys and the outputs: per launch, below)

    const bool pooled = !radiance_stays_on_chip(prm->max_bounces);
    // A lane takes a pool slot once, at its first path beyond the LDS levels, and keeps it for all its samples (RecordStack),
    // so a launch can need as many slots as it has lanes, the last wave's padding lanes included: the pool holds one per lane
    // and a pooled call of more than kRadiancePoolLanes rays runs as launches of that many, one behind the other on the
    // stream with the bump counter zeroed in between.  No launch can run out of slots.
    const unsigned chunk = pooled ? kRadiancePoolLanes : 0x80000000u;
    if (pooled) {
        if (const int rc = ctx.init(); rc != RTM_OK) return rc;
        const size_t lanes = (n_rays + kQueryBlock - 1) / kQueryBlock * kQueryBlock;
        P.pool_slots = (unsigned)std::min<size_t>(lanes, chunk);
        const size_t pool_bytes = (size_t)P.pool_slots * kPoolLevels * sizeof(uint32_t);
        unsigned char* pool = nullptr;  // (the buffer a render on this (device, stream) keeps its records in: one call behind the other)
        if (const int rc = scratch_acquire(ctx, kScratchPool, pool_bytes + 64, (void**)&pool); rc != RTM_OK) return rc;
        P.pool = pool;
        P.pool_next = reinterpret_cast<unsigned*>(pool + pool_bytes);
        A.overflow = ctx.sticky + 3;
    }

    int rc = RTM_OK;
    for (size_t first = 0; first < n_rays && rc == RTM_OK; first += chunk) {
        A.n_rays = (unsigned)std::min<size_t>(chunk, n_rays - first);
        A.org = org + first * 3;
        A.dir = dir + first * 3;
        A.key_base = prm->key_base + (unsigned)first;
        A.radiance = out->radiance ? out->radiance + first * 3 : nullptr;
        A.casts = out->casts ? out->casts + first : nullptr;
        A.draws = out->draws ? out->draws + first : nullptr;
        if (pooled) {
            const hipError_t e = hipMemsetAsync(P.pool_next, 0, sizeof(unsigned), stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                rc = fail(RTM_ERR_HIP, std::string("hipMemsetAsync (record pool counter): ") + hipGetErrorString(e));
                break;
            }
        }
        if (scene->grid.p)
            launch_radiance_as<kQueryGrid, SceneGlobal>(P, A, stream);
        else if (scene->has_planes)
            launch_radiance_as<kQueryChunked, SceneGlobalObjects>(P, A, stream);
        else
            launch_radiance_as<kQueryChunked, SceneGlobal>(P, A, stream);
        rc = launched("radiance query");
    }
    note_scene_use(scene, stream);
    if (rc != RTM_OK) return rc;
    // the stream's sticky flag travels to the host behind the launch, without anybody waiting for it (as behind a render)
    if (pooled) RTM_HIP_CHECK(hipMemcpyAsync(ctx.flag_host, ctx.sticky + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return RTM_OK;
}

}  // namespace rtm
