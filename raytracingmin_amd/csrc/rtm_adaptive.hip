// rtm_adaptive.hip — rtm_render_adaptive / rtm_adaptive_work_bytes (include/rtm.h): the pass schedule of tile-adaptive
// sampling over rtm_render_scene_tiles, the work buffer's layout and the launches of rtm_adaptive_kernel.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "rtm_adaptive_kernel.h"
#include "rtm_host.h"

namespace rtm {

namespace {
constexpr size_t kAlign = 256;
size_t round_up(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

// The work buffer: [snapshot: 24 bytes per pixel of the call's rows][list A][list B][flags][counts], each part 256-aligned.
struct Work {
    double* snap;
    unsigned* list[2];
    unsigned* flags;
    unsigned* count;
};
Work carve(void* base, size_t pixels, size_t tiles) {
    unsigned char* p = static_cast<unsigned char*>(base);
    Work w;
    w.snap = reinterpret_cast<double*>(p);
    p += round_up(pixels * 3 * sizeof(double));
    for (auto& l : w.list) {
        l = reinterpret_cast<unsigned*>(p);
        p += round_up(tiles * sizeof(unsigned));
    }
    w.flags = reinterpret_cast<unsigned*>(p);
    p += round_up(tiles * sizeof(unsigned));
    w.count = reinterpret_cast<unsigned*>(p);
    return w;
}

void add_stats(rtm_stats* total, const rtm_stats& s) {
    total->samples += s.samples;
    total->casts += s.casts;
    total->bounces += s.bounces;
    total->draws += s.draws;
    total->object_tests += s.object_tests;
    total->kernel_ms += s.kernel_ms;
    total->variant = s.variant;
    total->split = s.split;
}
}  // namespace

size_t adaptive_work_bytes(const rtm_settings* st, const rtm_options* opt) {
    if (!st || !opt || st->width <= 0) return 0;
    const int rows = output_rows(opt);
    if (rows <= 0) return 0;
    const size_t tiles = (size_t)((st->width + 7) / 8) * (size_t)((rows + 7) / 8);
    return round_up((size_t)st->width * (size_t)rows * 3 * sizeof(double)) + 3 * round_up(tiles * sizeof(unsigned)) + kAlign;
}

int render_adaptive(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, const rtm_adaptive_params* prm,
                    double* accum, float* out32, uint8_t* out8, uint32_t* tile_samples, void* work, void* stream_v,
                    rtm_stats* stats) {
    if (!prm) return invalid("params: null");
    if (!accum) return invalid("accum_f64_dev: the pixel accumulator is null");
    if (!work) return invalid("work_dev: null");
    if (prm->min_samples == 0u) return invalid("params.min_samples is 0");
    if (!std::isfinite(prm->threshold)) return invalid("params.threshold is NaN or infinite");
    if (!aligned256(work)) return invalid("work_dev is not 256-byte aligned");
    if (!st || !opt) return invalid("null settings or options");
    if (!scene) return invalid("null scene");
    const uint64_t ss = st->super_samples > 0 ? (uint64_t)st->super_samples : 0u, s1 = st->samples > 0 ? (uint64_t)st->samples : 0u;
    const uint64_t total = ss * ss * s1;  // N (0: the render below reports the bad settings)
    const uint32_t b0 = (uint32_t)(prm->min_samples < total ? prm->min_samples : total);
    if (stats) std::memset(stats, 0, sizeof *stats);
    const int rows = output_rows(opt);
    if (rows <= 0 || total == 0 || st->width <= 0)  // nothing to trace, or settings the render rejects: its answer
        return render_scene_samples(st, scene, opt, 0u, b0, accum, out32, out8, stream_v, stats);
    const unsigned tiles_x = (unsigned)((st->width + 7) / 8);
    const unsigned n_tiles = tiles_x * (unsigned)((rows + 7) / 8);
    const size_t pixels = (size_t)st->width * (size_t)rows;
    const Work w = carve(work, pixels, n_tiles);
    const hipStream_t stream = (hipStream_t)stream_v;
    RTM_HIP_CHECK(hipSetDevice(opt->device));

    // pass 0: [0, b_0) of every tile, through the list path.  Only the work buffer is written before it: a variant that
    // refuses lists refuses there, before any of the caller's outputs (tile_samples included) is touched.
    const unsigned begin_blocks = (n_tiles + 255u) / 256u;
    adaptive_begin_kernel<<<begin_blocks, 256, 0, stream>>>(w.list[0], nullptr, n_tiles, b0);
    RTM_HIP_CHECK(hipGetLastError());
    rtm_stats s;
    int rc = render_scene_tiles(st, scene, opt, 0u, b0, w.list[0], n_tiles, accum, out32, out8, stream_v, stats ? &s : nullptr);
    if (rc != RTM_OK) return rc;
    if (stats) add_stats(stats, s);
    if (tile_samples) {
        adaptive_begin_kernel<<<begin_blocks, 256, 0, stream>>>(w.list[0], tile_samples, n_tiles, b0);
        RTM_HIP_CHECK(hipGetLastError());
    }
    if ((uint64_t)b0 == total) return RTM_OK;
    RTM_HIP_CHECK(hipMemcpyAsync(w.snap, accum, pixels * 3 * sizeof(double), hipMemcpyDeviceToDevice, stream));

    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Events {
        hipEvent_t* e;
        ~Events() {
            for (int k = 0; k < 2; ++k)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } guard{ev};
    if (stats)
        for (auto& e : ev) RTM_HIP_CHECK(hipEventCreate(&e));

    unsigned n_active = n_tiles, cur = 0;
    uint64_t a = b0;
    while (n_active != 0u && a < total) {
        const uint64_t b = 2 * a < total ? 2 * a : total;  // b_i = min(2^i m, N) = min(2 b_{i-1}, N)
        rc = render_scene_tiles(st, scene, opt, (uint32_t)a, (uint32_t)b, w.list[cur], n_active, accum, out32, out8, stream_v,
                                stats ? &s : nullptr);
        if (rc != RTM_OK) return rc;
        if (stats) {
            add_stats(stats, s);
            RTM_HIP_CHECK(hipEventRecord(ev[0], stream));
        }
        AdaptiveCheck A;
        A.acc = accum;
        A.snap = w.snap;
        A.list = w.list[cur];
        A.flags = w.flags;
        A.tile_samples = tile_samples;
        A.W = st->width;
        A.rows = rows;
        A.tiles_x = (int)tiles_x;
        A.frame_tiles = n_tiles;
        A.b = (unsigned)b;
        A.last = b == total ? 1u : 0u;
        A.sb = (double)total / (double)b;
        A.sa = (double)total / (double)a;
        A.threshold = (double)prm->threshold;
        adaptive_check_kernel<<<n_active, 64, 0, stream>>>(A);
        adaptive_compact_kernel<<<1, kCompactThreads, 0, stream>>>(w.flags, w.list[cur], n_active, w.list[cur ^ 1u], w.count);
        RTM_HIP_CHECK(hipGetLastError());
        if (stats) RTM_HIP_CHECK(hipEventRecord(ev[1], stream));
        unsigned next = 0;
        RTM_HIP_CHECK(hipMemcpyAsync(&next, w.count, sizeof next, hipMemcpyDeviceToHost, stream));
        RTM_HIP_CHECK(hipStreamSynchronize(stream));
        if (stats) {
            float ms = 0.f;
            RTM_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
            stats->kernel_ms += ms;
        }
        n_active = next;
        cur ^= 1u;
        a = b;
    }
    return RTM_OK;
}

}  // namespace rtm
