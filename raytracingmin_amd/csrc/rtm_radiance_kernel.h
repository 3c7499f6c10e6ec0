// rtm_radiance_kernel.h — radiance queries on a scene object (include/rtm.h: rtm_scene_radiance): png::PathTracing
// (src/Renderer.cpp:57-117) for rays of the caller's, S samples per ray, summed as the reference sums a pixel's samples
// (:240-242 at superSamples == 1).  Included by rtm_radiance.hip, which is part of rtm_kernels.hip's translation unit: its
// -ffp-contract=off build is the reference's own arithmetic.
//
// One lane per ray, one wave per block, like query_kernel.  A lane loops over its S samples itself: when its path ends it
// folds its records (path_fold), adds the sample's term to its accumulator, opens the stream (key, s + 1) and starts again
// from the caller's ray; the wave leaves when a ballot finds no lane with a sample left.  The sum over a ray's samples is
// thereby made in sample order by one lane, without any cross-lane reduction, and a lane whose paths are short does not
// wait for its neighbours' long ones sample by sample.  Parallelism is over rays only.
//
// The search is one of the render kernels' own (rtm_path.h), chosen by the host as query_kernel's is:
//   kQueryGrid     nearest_hit_grid<MathFast> over the scene's uniform grid, its candidate queue in LDS; a ray the grid
//                  cannot serve sends its wave through the walk's exhaustive loop.  A plane in such a scene is among the
//                  objects every ray tests and is shaded as render_grid_kernel shades it (found at run time).
//   kQueryChunked  nearest_hit<MathFast, 8>: every object, planes through object_chunk (SceneGlobalObjects)
// Shading is path_shade_spec, the speculative block of the default render kernel with its MathRef fallback, on the
// SceneGlobal view of the scene.  Hit records: RecordStack, kRadianceLdsLevels levels per lane in LDS, then the stream
// context's record pool (P.pool; null when the depth cap keeps every path on chip).
// Every lane of a wave stays in the searches' wave-uniform loops and ballots: a lane past n_rays traces the last ray again
// and stores nothing; a lane that has finished its samples keeps the ray it ended on and is not shaded.
#ifndef RTM_RADIANCE_KERNEL_H
#define RTM_RADIANCE_KERNEL_H
#include "rtm_query_kernel.h"

namespace rtm {

constexpr int kRadianceLdsLevels = 16;  // on-chip record levels per lane (4 KiB per wave: 16 waves per CU keep their LDS)
constexpr int kRadianceWavesPerSimd = 4;  // the bound render_grid_kernel runs the same walk and shading block under

struct RadianceArgs {
    const double* __restrict__ org;  // n_rays x 3
    const double* __restrict__ dir;  // n_rays x 3
    unsigned n_rays;
    unsigned samples;   // S >= 1
    unsigned key_base;  // ray i draws from the streams (seed, key_base + i, s)
    unsigned clamp;     // RTM_RADIANCE_CLAMP
    double dS;          // (double)S
    double* __restrict__ radiance;  // n_rays x 3, or null
    uint32_t* __restrict__ casts;   // n_rays, or null
    uint32_t* __restrict__ draws;   // n_rays, or null
    unsigned long long* __restrict__ overflow;  // the stream's sticky flag word, or null where no path can leave the LDS levels
};

// the block's dynamic LDS: the shading constants (with the near-unit Normalize table when unit_tab), the records, the queue
__host__ __device__ inline size_t radiance_lds_bytes(int search, bool unit_tab) {
    return (size_t)(unit_tab ? kShadeConstCount : kTrigConstCount) * sizeof(double) +
           (size_t)kRadianceLdsLevels * kQueryBlock * sizeof(uint32_t) + query_lds_bytes(search);
}

// P: scene (with trig_fix under RTM_MODE_HOST_TRIG), mode, max_bounces, seed_mult, unit_tab and the record pool; nothing
// else of it is read.
template <int SEARCH, class Scene>
__global__ __launch_bounds__(kQueryBlock, kRadianceWavesPerSimd) void radiance_kernel(const RenderParams P, const RadianceArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x;
    double* trig = reinterpret_cast<double*>(lds_raw);
    const bool unit_tab = P.unit_tab != 0u;  // wave-uniform
    uint32_t* rec = reinterpret_cast<uint32_t*>(trig + (unit_tab ? kShadeConstCount : kTrigConstCount));
    [[maybe_unused]] unsigned char* queue = reinterpret_cast<unsigned char*>(rec + kRadianceLdsLevels * kQueryBlock);  // 16-byte aligned
    fill_shade_consts(trig, lane, unit_tab);
    __syncthreads();

    const unsigned i = blockIdx.x * (unsigned)kQueryBlock + (unsigned)lane;
    const size_t r = i < A.n_rays ? i : A.n_rays - 1u;
    Scene sc;
    sc.v = P.scene;
    const SceneGlobal& shade_sc = sc;  // (SceneGlobalObjects differs in the search alone)
    const D3 o = d3(A.org[r * 3], A.org[r * 3 + 1], A.org[r * 3 + 2]);
    const D3 d = d3(A.dir[r * 3], A.dir[r * 3 + 1], A.dir[r * 3 + 2]);
    const RngPixelKey key = rng_pixel_key(P.seed_mult, A.key_base + (unsigned)r);

    PathCounters pc = {0, 0, 0};
    RecordStack<uint32_t, kRadianceLdsLevels> stack{rec, lane, &P};
    auto push = [&](int dd, int id) { stack.push(dd, id); };
    auto pop = [&](int dd) -> int { return stack.pop(dd); };

    unsigned s = 0;
    D3 org = o, dir = d, acc = d3(0, 0, 0);
    int depth = 0;
    RngStream rng = rng_open(key, 0u);
    bool busy = true, overflowed = false;
    while (__builtin_amdgcn_ballot_w64(busy) != 0) {  // wave-uniform
        double dis;
        int id;
        if constexpr (SEARCH == kQueryGrid)
            id = nearest_hit_grid<MathFast, Scene>(sc, org, dir, dis, queue, kQueryBlock, lane);
        else
            id = nearest_hit<MathFast, 8>(sc, org, dir, dis);
        if (busy) {
            D3 term;
            bool cont = path_shade_spec(shade_sc, id, dis, P.mode, P.max_bounces, org, dir, depth, rng, term, pc, push, ShadeLds(trig, unit_tab));
            if (cont && stack.overflow) {  // records exhausted: this path is truncated; the stream's sticky flag says so
                cont = false;
                term = d3(0, 0, 0);
                depth = 0;
                overflowed = true;
                stack.overflow = false;  // (the lane's next sample starts with its on-chip levels, and its pool slot if it has one)
            }
            if (!cont) {
                const bool deep = depth > kRadianceLdsLevels;
                const D3 L = (__builtin_amdgcn_ballot_w64(deep) == 0)
                                 ? path_fold_blocked(shade_sc, term, depth, [&](int dd) { return (int)rec[dd * kQueryBlock + lane]; })
                                 : path_fold(shade_sc, term, depth, pop);
                const D3 t = L / A.dS;                       // :240 at superSamples == 1
                acc = acc + (A.clamp ? clamp01_d3(t) : t);   // :241-242
                ++s;
                if (s < A.samples) {
                    org = o;
                    dir = d;
                    depth = 0;
                    rng = rng_open(key, s);
                } else {
                    busy = false;
                }
            }
        }
    }
    if (A.overflow && overflowed) atomicOr(A.overflow, 1ull);
    if (i >= A.n_rays) return;
    if (A.radiance) {
        A.radiance[(size_t)i * 3] = acc.x;
        A.radiance[(size_t)i * 3 + 1] = acc.y;
        A.radiance[(size_t)i * 3 + 2] = acc.z;
    }
    if (A.casts) A.casts[i] = pc.casts;
    if (A.draws) A.draws[i] = pc.draws;
}

}  // namespace rtm
#endif
