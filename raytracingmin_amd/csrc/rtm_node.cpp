// rtm_node.cpp — one-process, N-GPU rendering for the host program: the image is dealt out in
// interleaved 8-row bands (band b goes to GPU b mod N: every GPU gets the same mix of cheap and costly
// rows), every GPU of the node renders its bands through the C ABI (rtm_render_scene with
// band_count/band_index, one host thread per device), and the band stacks are collected on device 0
// with ONE grouped RCCL exchange over xGMI (ncclSend from every device, matching ncclRecv on device 0),
// where the bands are put back in image order.  What travels is the float3 accumulation buffer
// (north_star) with the 8-bit view of the same rows behind it in the same message — the 8-bit image has
// to be quantised from the fp64 value (src/Renderer.cpp:253), which only the rendering GPU has.
// The reference has no multi-device code; this is the north_star's "image tiled across the 8 GPUs of
// one node with a single RCCL gather".  Linked into rtm_cli only — librtm_hip.so itself stays free of
// RCCL so that it can share a process with PyTorch's bundled copy.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtm.h"
#include "rtm_node.h"

namespace {
#define NODE_HIP(expr)                                                                      \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess) {                                                            \
            err = std::string(#expr) + ": " + hipGetErrorString(e__);                       \
            return RTM_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)
#define NODE_NCCL(expr)                                                                     \
    do {                                                                                    \
        ncclResult_t r__ = (expr);                                                          \
        if (r__ != ncclSuccess) {                                                           \
            err = std::string(#expr) + ": " + ncclGetErrorString(r__);                      \
            return RTM_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

// Everything one part owns; released on every return path.
struct Part {
    int dev = 0;
    rtm_options opt{};
    size_t rows = 0;
    hipStream_t stream = nullptr;
    unsigned char* strip = nullptr;  // [rows*W*3 floats][rows*W*3 bytes]
    rtm_scene* scene = nullptr;
    rtm_stats stats{};
    int rc = RTM_OK;
    std::string detail;
    ~Part() {
        (void)hipSetDevice(dev);
        if (scene) (void)rtm_scene_destroy(scene);
        if (strip) (void)hipFree(strip);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
struct RootBuffers {
    int dev = 0;
    unsigned char* stage = nullptr;
    float* full32 = nullptr;
    uint8_t* full8 = nullptr;
    ~RootBuffers() {
        (void)hipSetDevice(dev);
        if (stage) (void)hipFree(stage);
        if (full32) (void)hipFree(full32);
        if (full8) (void)hipFree(full8);
    }
};
struct Comms {
    std::vector<ncclComm_t> c;
    ~Comms() {
        for (auto v : c)
            if (v) (void)ncclCommDestroy(v);
    }
};

// Every step of the multi-GPU path announces itself on stderr (one write per line, never buffered), and a watchdog
// thread ends the process — a fresh non-zero exit, code 3, naming the stage — when a stage does not finish within its
// bound.  A run that stalls (a communicator that never comes up, a send/recv pair that never matches, a kernel that
// never drains) therefore says WHERE it stalled instead of dying silently at its caller's limit.
// Bounds: RTM_NODE_STAGE_TIMEOUT seconds for the set-up / RCCL / assembly stages (default 60), RTM_NODE_RENDER_TIMEOUT
// for the render stage (default 0 = unbounded: a frame may legitimately take minutes); RTM_NODE_QUIET=1 drops the lines
// (never the watchdog's).
class Stages {
  public:
    Stages() {
        stage_limit_ = env_seconds("RTM_NODE_STAGE_TIMEOUT", 60);
        render_limit_ = env_seconds("RTM_NODE_RENDER_TIMEOUT", 0);
        const char* q = std::getenv("RTM_NODE_QUIET");
        quiet_ = q && q[0] == '1';
        dog_ = std::thread([this] { watch(); });
    }
    ~Stages() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        dog_.join();
    }
    void enter(bool render_stage, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        char buf[256];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        {
            std::lock_guard<std::mutex> g(m_);
            name_ = buf;
            since_ = std::chrono::steady_clock::now();
            limit_ = render_stage ? render_limit_ : stage_limit_;
        }
        say("stage: ", buf);
        // test hook: RTM_NODE_DEBUG_STALL=<text> parks the calling thread in the first stage whose name contains
        // <text>, which is how tests/test_cli_gpu.py shows that a stalled stage ends in exit code 3 with its name
        const char* stall = std::getenv("RTM_NODE_DEBUG_STALL");
        if (stall && *stall && std::strstr(buf, stall))
            for (;;) ::pause();
    }
    void note(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char buf[256];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        say("", buf);
    }

  private:
    static int env_seconds(const char* name, int dflt) {
        const char* v = std::getenv(name);
        return v && *v ? std::atoi(v) : dflt;
    }
    void say(const char* prefix, const char* text) const {
        if (quiet_) return;
        char line[320];
        int n = std::snprintf(line, sizeof line - 1, "rtm_node: %s%s", prefix, text);
        if (n > (int)sizeof line - 2) n = (int)sizeof line - 2;
        line[n++] = '\n';
        (void)!::write(2, line, (size_t)n);  // one write(2) per line: nothing to flush, nothing to interleave
    }
    void watch() {
        std::unique_lock<std::mutex> g(m_);
        while (!stop_) {
            cv_.wait_for(g, std::chrono::milliseconds(500));
            if (stop_ || limit_ <= 0 || name_.empty()) continue;
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - since_).count();
            if (waited > limit_) {
                char line[400];
                const int n = std::snprintf(line, sizeof line,
                                            "rtm_node: WATCHDOG: stage '%s' has not finished after %d s; exiting with code 3\n",
                                            name_.c_str(), limit_);
                (void)!::write(2, line, (size_t)n);
                ::_exit(3);
            }
        }
    }
    std::mutex m_;
    std::condition_variable cv_;
    std::string name_;
    std::chrono::steady_clock::time_point since_{};
    int limit_ = 0, stage_limit_ = 60, render_limit_ = 0;
    bool stop_ = false, quiet_ = false;
    std::thread dog_;
};
}  // namespace

int rtm_node_render(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* base,
                    int n_devices, int virtual_strips, int force_rccl, float* out_f32_host, uint8_t* out_u8_host,
                    rtm_stats* total, std::string& err) {
    if (!st || !base || (!out_u8_host && !out_f32_host) || n_devices < 1) return RTM_ERR_INVALID_ARGUMENT;
    const int W = st->width, H = st->height;
    const size_t px_bytes = 3 * sizeof(float) + 3;  // float3 + rgb8 per pixel
    // virtual_strips > 0: that many parts, all on base->device (exercises the tiling on one GPU)
    const int parts = virtual_strips > 0 ? virtual_strips : n_devices;
    Stages stages;  // first, so that it outlives (and watches) the release of everything below
    std::vector<Part> part(parts);
    std::vector<size_t> stage_off(parts + 1, 0);
    for (int r = 0; r < parts; ++r) {
        Part& p = part[r];
        p.dev = virtual_strips > 0 ? base->device : r;
        p.opt = *base;
        p.opt.device = p.dev;
        p.opt.row_begin = 0;
        p.opt.row_end = H;
        p.opt.band_count = parts;
        p.opt.band_index = r;
        p.rows = (size_t)rtm_output_rows(&p.opt);
        stage_off[r + 1] = (stage_off[r] + p.rows * W * px_bytes + 15) & ~(size_t)15;
    }
    const int root = part[0].dev;
    for (int r = 0; r < parts; ++r) {
        Part& p = part[r];
        stages.enter(false, "set-up of part %d of %d on device %d (stream, band stack, scene upload)", r, parts, p.dev);
        NODE_HIP(hipSetDevice(p.dev));
        NODE_HIP(hipStreamCreate(&p.stream));
        if (p.rows) NODE_HIP(hipMalloc((void**)&p.strip, p.rows * W * px_bytes));
        const int rc = rtm_scene_create_objects(objects, n, p.dev, &p.scene);
        if (rc != RTM_OK) {
            err = std::string("rtm_scene_create_objects: ") + rtm_last_error_detail();
            return rc;
        }
    }
    // one host thread per part: the renders of different GPUs run concurrently
    auto work = [&](int r) {
        Part& p = part[r];
        float* f32 = reinterpret_cast<float*>(p.strip);
        uint8_t* u8 = p.strip ? p.strip + p.rows * W * 3 * sizeof(float) : nullptr;
        p.rc = rtm_render_scene(st, p.scene, &p.opt, nullptr, f32, u8, p.stream, &p.stats);
        if (p.rc != RTM_OK) p.detail = rtm_last_error_detail();
        stages.note("part %d rendered on device %d: rc %d, %.3f ms of kernels", r, p.dev, p.rc, p.stats.kernel_ms);
    };
    stages.enter(true, "render of %d part(s): %dx%d, %zu row(s) in the largest", parts, W, H, part[0].rows);
    if (virtual_strips > 0) {
        for (int r = 0; r < parts; ++r) work(r);
    } else {
        std::vector<std::thread> th;
        for (int r = 0; r < parts; ++r) th.emplace_back(work, r);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < parts; ++r)
        if (part[r].rc != RTM_OK) {
            err = "part " + std::to_string(r) + ": " + part[r].detail;
            return part[r].rc;
        }

    // gather on the root device: the band stacks land side by side in a staging buffer ...
    RootBuffers rb;
    rb.dev = root;
    stages.enter(false, "frame buffers on the root device %d", root);
    NODE_HIP(hipSetDevice(root));
    NODE_HIP(hipMalloc((void**)&rb.full32, (size_t)W * H * 3 * sizeof(float)));
    NODE_HIP(hipMalloc((void**)&rb.full8, (size_t)W * H * 3));
    std::vector<const unsigned char*> src(parts);
    const bool use_rccl = virtual_strips <= 0 && (n_devices > 1 || force_rccl);
    if (!use_rccl) {
        for (int r = 0; r < parts; ++r) src[r] = part[r].strip;
    } else {
        NODE_HIP(hipMalloc((void**)&rb.stage, stage_off[parts] ? stage_off[parts] : 1));
        // one process, one node: RCCL's bootstrap needs no more than the loopback interface (a container's veth is
        // not always usable for it); rtm_cli's main() sets NCCL_SOCKET_IFNAME=lo before anything else runs unless the
        // user has set one — here, with HIP threads alive, the environment is only read
        const char* ifname = std::getenv("NCCL_SOCKET_IFNAME");
        Comms comms;
        comms.c.assign(parts, nullptr);
        std::vector<int> devs(parts);
        for (int r = 0; r < parts; ++r) devs[r] = part[r].dev;
        stages.enter(false, "ncclCommInitAll over %d device(s), bootstrap interface %s", parts, ifname ? ifname : "(RCCL's choice)");
        NODE_NCCL(ncclCommInitAll(comms.c.data(), parts, devs.data()));
        stages.enter(false, "grouped ncclSend/ncclRecv of %zu bytes into device %d", stage_off[parts], root);
        NODE_NCCL(ncclGroupStart());
        for (int r = 0; r < parts; ++r) {
            src[r] = rb.stage + stage_off[r];
            const size_t bytes = part[r].rows * W * px_bytes;
            if (!bytes) continue;
            NODE_NCCL(ncclSend(part[r].strip, bytes, ncclUint8, 0, comms.c[r], part[r].stream));
            NODE_NCCL(ncclRecv(rb.stage + stage_off[r], bytes, ncclUint8, r, comms.c[0], part[0].stream));
        }
        NODE_NCCL(ncclGroupEnd());
        for (int r = 0; r < parts; ++r) {
            stages.enter(false, "stream synchronise after the exchange, part %d on device %d", r, part[r].dev);
            NODE_HIP(hipSetDevice(part[r].dev));
            NODE_HIP(hipStreamSynchronize(part[r].stream));
        }
        NODE_HIP(hipSetDevice(root));
        stages.enter(false, "ncclCommDestroy of %d communicator(s)", parts);
    }
    // ... and band b of the image is band b / parts of part b % parts
    const int bands = (H + 7) / 8;
    stages.enter(false, "de-interleave of %d band(s) on the root device + copy to the host", bands);
    for (int b = 0; b < bands; ++b) {
        const int rows = (H - b * 8 < 8) ? H - b * 8 : 8;
        const Part& p = part[b % parts];
        const unsigned char* s32 = src[b % parts] + (size_t)(b / parts) * 8 * W * 3 * sizeof(float);
        const unsigned char* s8 = src[b % parts] + p.rows * W * 3 * sizeof(float) + (size_t)(b / parts) * 8 * W * 3;
        NODE_HIP(hipMemcpyAsync(rb.full32 + (size_t)b * 8 * W * 3, s32, (size_t)rows * W * 3 * sizeof(float),
                                hipMemcpyDeviceToDevice, part[0].stream));
        NODE_HIP(hipMemcpyAsync(rb.full8 + (size_t)b * 8 * W * 3, s8, (size_t)rows * W * 3, hipMemcpyDeviceToDevice,
                                part[0].stream));
    }
    NODE_HIP(hipStreamSynchronize(part[0].stream));
    if (out_f32_host) NODE_HIP(hipMemcpy(out_f32_host, rb.full32, (size_t)W * H * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_u8_host) NODE_HIP(hipMemcpy(out_u8_host, rb.full8, (size_t)W * H * 3, hipMemcpyDeviceToHost));
    if (total) {
        std::memset(total, 0, sizeof *total);
        for (int r = 0; r < parts; ++r) {
            const rtm_stats& s = part[r].stats;
            total->samples += s.samples;
            total->casts += s.casts;
            total->bounces += s.bounces;
            total->draws += s.draws;
            // parts on different GPUs overlap in time: the frame's kernel time is the longest part;
            // virtual parts on one GPU run back to back
            total->kernel_ms = virtual_strips > 0 ? total->kernel_ms + s.kernel_ms
                                                  : (s.kernel_ms > total->kernel_ms ? s.kernel_ms : total->kernel_ms);
            total->variant = s.variant;
            total->split = s.split;
        }
    }
    stages.enter(false, "release of the parts' scenes, buffers and streams");
    return RTM_OK;
}

// --passes (rtm_node.h): the frame as `passes` contiguous, near-equal sample ranges through rtm_render_scene_samples on one
// device, a progress line per pass; the outputs of the last pass are the frame.  Stats are summed over the passes.
int rtm_node_render_passes(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt, int passes,
                           float* out_f32_host, uint8_t* out_u8_host, rtm_stats* total, std::string& err) {
    const unsigned N = (unsigned)st->super_samples * (unsigned)st->super_samples * (unsigned)st->samples;
    if (passes < 1 || (unsigned)passes > N) {
        err = "--passes " + std::to_string(passes) + ": must be in [1, " + std::to_string(N) + "] (the frame's samples per pixel)";
        return RTM_ERR_INVALID_ARGUMENT;
    }
    if (hipSetDevice(opt->device) != hipSuccess) {
        err = "no HIP device " + std::to_string(opt->device);
        return RTM_ERR_NO_DEVICE;
    }
    rtm_scene* scene = nullptr;
    int rc = rtm_scene_create_objects(objects, n, opt->device, &scene);
    if (rc != RTM_OK) {
        err = std::string("scene: ") + rtm_last_error_detail();
        return rc;
    }
    const size_t vals = (size_t)st->width * st->height * 3;
    double* accum = nullptr;
    float* d32 = nullptr;
    uint8_t* d8 = nullptr;
    if (hipMalloc((void**)&accum, vals * sizeof(double)) != hipSuccess ||
        (out_f32_host && hipMalloc((void**)&d32, vals * sizeof(float)) != hipSuccess) ||
        (out_u8_host && hipMalloc((void**)&d8, vals) != hipSuccess)) {
        err = "no device memory for the frame";
        rc = RTM_ERR_HIP;
    }
    std::memset(total, 0, sizeof *total);
    const unsigned q = N / (unsigned)passes, r = N % (unsigned)passes;
    unsigned a = 0;
    for (int i = 0; rc == RTM_OK && i < passes; ++i) {
        const unsigned b = a + q + ((unsigned)i < r ? 1u : 0u);
        rtm_stats s;
        rc = rtm_render_scene_samples(st, scene, opt, a, b, accum, d32, d8, nullptr, &s);
        if (rc != RTM_OK) {
            err = rtm_last_error_detail();
            break;
        }
        std::printf("pass %d/%d: samples [%u, %u) %.3f ms\n", i + 1, passes, a, b, s.kernel_ms);
        total->samples += s.samples;
        total->casts += s.casts;
        total->bounces += s.bounces;
        total->draws += s.draws;
        total->kernel_ms += s.kernel_ms;
        total->variant = s.variant;
        a = b;
    }
    if (rc == RTM_OK && ((out_u8_host && hipMemcpy(out_u8_host, d8, vals, hipMemcpyDeviceToHost) != hipSuccess) ||
                         (out_f32_host && hipMemcpy(out_f32_host, d32, vals * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess))) {
        err = "copying the frame back failed";
        rc = RTM_ERR_HIP;
    }
    (void)hipFree(accum);
    (void)hipFree(d32);
    (void)hipFree(d8);
    (void)rtm_scene_destroy(scene);
    return rc;
}

// --adaptive (rtm_node.h): rtm_render_adaptive of the whole frame on the default stream, outputs and sample map copied back.
int rtm_node_render_adaptive(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                             const rtm_adaptive_params* prm, float* out_f32_host, uint8_t* out_u8_host,
                             std::vector<uint32_t>& tile_samples, rtm_stats* total, std::string& err) {
    if (hipSetDevice(opt->device) != hipSuccess) {
        err = "no HIP device " + std::to_string(opt->device);
        return RTM_ERR_NO_DEVICE;
    }
    rtm_scene* scene = nullptr;
    int rc = rtm_scene_create_objects(objects, n, opt->device, &scene);
    if (rc != RTM_OK) {
        err = std::string("scene: ") + rtm_last_error_detail();
        return rc;
    }
    const size_t vals = (size_t)st->width * st->height * 3;
    const size_t tiles = (size_t)((st->width + 7) / 8) * (size_t)((st->height + 7) / 8);
    tile_samples.assign(tiles, 0u);
    double* accum = nullptr;
    float* d32 = nullptr;
    uint8_t* d8 = nullptr;
    uint32_t* dts = nullptr;
    void* work = nullptr;
    if (hipMalloc((void**)&accum, vals * sizeof(double)) != hipSuccess ||
        (out_f32_host && hipMalloc((void**)&d32, vals * sizeof(float)) != hipSuccess) ||
        (out_u8_host && hipMalloc((void**)&d8, vals) != hipSuccess) ||
        hipMalloc((void**)&dts, tiles * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&work, rtm_adaptive_work_bytes(st, opt)) != hipSuccess) {
        err = "no device memory for the frame";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        rc = rtm_render_adaptive(st, scene, opt, prm, accum, d32, d8, dts, work, nullptr, total);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc == RTM_OK && ((out_u8_host && hipMemcpy(out_u8_host, d8, vals, hipMemcpyDeviceToHost) != hipSuccess) ||
                         (out_f32_host && hipMemcpy(out_f32_host, d32, vals * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) ||
                         hipMemcpy(tile_samples.data(), dts, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)) {
        err = "copying the frame back failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        double sum = 0.0;
        for (size_t t = 0; t < tiles; ++t) {
            const int tx = (int)(t % (size_t)((st->width + 7) / 8)), ty = (int)(t / (size_t)((st->width + 7) / 8));
            sum += (double)tile_samples[t] * std::min(8, st->width - 8 * tx) * std::min(8, st->height - 8 * ty);
        }
        std::printf("adaptive: threshold %g, min_samples %u: mean %.2f samples per pixel of %d\n", (double)prm->threshold,
                    prm->min_samples, sum / ((double)st->width * st->height), st->super_samples * st->super_samples * st->samples);
    }
    (void)hipFree(accum);
    (void)hipFree(d32);
    (void)hipFree(d8);
    (void)hipFree(dts);
    (void)hipFree(work);
    (void)rtm_scene_destroy(scene);
    return rc;
}

// --aov (rtm_node.h): one rtm_render_aov of the frame on the default stream, then the five files.
int rtm_node_write_aov(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                       const std::string& stem, std::string& err) {
    if (hipSetDevice(opt->device) != hipSuccess) {
        err = "no HIP device " + std::to_string(opt->device);
        return RTM_ERR_NO_DEVICE;
    }
    rtm_scene* scene = nullptr;
    int rc = rtm_scene_create_objects(objects, n, opt->device, &scene);
    if (rc != RTM_OK) {
        err = std::string("scene: ") + rtm_last_error_detail();
        return rc;
    }
    const size_t pix = (size_t)st->width * st->height;
    rtm_aov_buffers dev;
    std::memset(&dev, 0, sizeof dev);
    if (hipMalloc((void**)&dev.depth, pix * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.normal, pix * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.albedo, pix * 3 * sizeof(float)) != hipSuccess) {
        err = "no device memory for the AOV planes";
        rc = RTM_ERR_HIP;
    }
    std::vector<float> depth(pix), normal(pix * 3), albedo(pix * 3);
    if (rc == RTM_OK) {
        rc = rtm_render_aov(st, scene, opt, &dev, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc == RTM_OK && (hipMemcpy(depth.data(), dev.depth, pix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(normal.data(), dev.normal, pix * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(albedo.data(), dev.albedo, pix * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) {
        err = "copying the AOV planes back failed";
        rc = RTM_ERR_HIP;
    }
    (void)hipFree(dev.depth);
    (void)hipFree(dev.normal);
    (void)hipFree(dev.albedo);
    (void)rtm_scene_destroy(scene);
    if (rc != RTM_OK) return rc;
    const int w = st->width, h = st->height;
    bool ok = rtm_write_pfm((stem + "_depth.pfm").c_str(), w, h, 1, depth.data()) == 1 &&
              rtm_write_pfm((stem + "_normal.pfm").c_str(), w, h, 3, normal.data()) == 1 &&
              rtm_write_pfm((stem + "_albedo.pfm").c_str(), w, h, 3, albedo.data()) == 1;
    std::vector<double> v(pix * 3);
    std::vector<uint8_t> rgb8(pix * 3);
    for (size_t i = 0; i < v.size(); ++i) v[i] = 0.5 * (double)normal[i] + 0.5;
    ok = ok && rtm_quantise(v.data(), v.size(), rgb8.data()) == RTM_OK &&
         rtm_write_bmp((stem + "_normal.bmp").c_str(), w, h, 3, rgb8.data()) == 1;
    for (size_t i = 0; i < v.size(); ++i) v[i] = (double)albedo[i];
    ok = ok && rtm_quantise(v.data(), v.size(), rgb8.data()) == RTM_OK &&
         rtm_write_bmp((stem + "_albedo.bmp").c_str(), w, h, 3, rgb8.data()) == 1;
    if (!ok) {
        err = "cannot write the AOV files of " + stem;
        return RTM_ERR_IO;
    }
    return RTM_OK;
}

// --alpha / --matte / --background (rtm_node.h): one rtm_render_mattes of the frame on the default stream (the layers only
// when a matte is asked for), then rtm_matte and rtm_composite behind it, then the files.
int rtm_node_write_mattes(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt, bool want_alpha,
                          int layers, const std::vector<int32_t>& ids, const rtm_composite_params* background,
                          const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* over_out) {
    if (hipSetDevice(opt->device) != hipSuccess) {
        err = "no HIP device " + std::to_string(opt->device);
        return RTM_ERR_NO_DEVICE;
    }
    rtm_scene* scene = nullptr;
    int rc = rtm_scene_create_objects(objects, n, opt->device, &scene);
    if (rc != RTM_OK) {
        err = std::string("scene: ") + rtm_last_error_detail();
        return rc;
    }
    const size_t pix = (size_t)st->width * st->height;
    const bool want_matte = !ids.empty();
    rtm_matte_buffers dev;
    std::memset(&dev, 0, sizeof dev);
    int32_t* sel = nullptr;
    float* matte = nullptr;
    float* color = nullptr;  // the frame, composited in place
    uint8_t* over8 = nullptr;
    if (hipMalloc((void**)&dev.alpha, pix * sizeof(float)) != hipSuccess ||
        (want_matte && (hipMalloc((void**)&dev.id, pix * layers * sizeof(int32_t)) != hipSuccess ||
                        hipMalloc((void**)&dev.coverage, pix * layers * sizeof(float)) != hipSuccess ||
                        hipMalloc((void**)&sel, ids.size() * sizeof(int32_t)) != hipSuccess ||
                        hipMalloc((void**)&matte, pix * sizeof(float)) != hipSuccess)) ||
        (background && (hipMalloc((void**)&color, pix * 3 * sizeof(float)) != hipSuccess ||
                        hipMalloc((void**)&over8, pix * 3) != hipSuccess))) {
        err = "no device memory for the coverage planes";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && ((want_matte && hipMemcpy(sel, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) ||
                         (background && hipMemcpy(color, f32_host, pix * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))) {
        err = "copying the id list or the frame to the device failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) rc = rtm_render_mattes(st, scene, opt, layers, &dev, nullptr);
    if (rc == RTM_OK && want_matte)
        rc = rtm_matte(st->width, st->height, layers, opt->device, dev.id, dev.coverage, sel, (int32_t)ids.size(), matte, nullptr);
    if (rc == RTM_OK && background)
        rc = rtm_composite(background, st->width, st->height, opt->device, color, dev.alpha, nullptr, color, over8, nullptr);
    if (rc != RTM_OK && err.empty()) err = rtm_last_error_detail();
    std::vector<float> alpha_h(pix), matte_h(want_matte ? pix : 0), over_h(background && over_out ? pix * 3 : 0);
    std::vector<uint8_t> over8_h(background ? pix * 3 : 0);
    if (rc == RTM_OK &&
        (hipMemcpy(alpha_h.data(), dev.alpha, pix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
         (want_matte && hipMemcpy(matte_h.data(), matte, pix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) ||
         (background && hipMemcpy(over8_h.data(), over8, pix * 3, hipMemcpyDeviceToHost) != hipSuccess) ||
         (!over_h.empty() && hipMemcpy(over_h.data(), color, pix * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess))) {
        err = "copying the coverage planes back failed";
        rc = RTM_ERR_HIP;
    }
    (void)hipFree(dev.alpha);
    (void)hipFree(dev.id);
    (void)hipFree(dev.coverage);
    (void)hipFree(sel);
    (void)hipFree(matte);
    (void)hipFree(color);
    (void)hipFree(over8);
    (void)rtm_scene_destroy(scene);
    if (rc != RTM_OK) return rc;
    const int w = st->width, h = st->height;
    bool ok = !want_alpha || rtm_write_pfm((stem + "_alpha.pfm").c_str(), w, h, 1, alpha_h.data()) == 1;
    if (want_matte) {
        std::vector<double> v(pix * 3);
        std::vector<uint8_t> grey(pix * 3);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (double)matte_h[i / 3];
        ok = ok && rtm_write_pfm((stem + "_matte.pfm").c_str(), w, h, 1, matte_h.data()) == 1 &&
             rtm_quantise(v.data(), v.size(), grey.data()) == RTM_OK && rtm_write_bmp((stem + "_matte.bmp").c_str(), w, h, 3, grey.data()) == 1;
    }
    if (background)
        ok = ok && rtm_write_bmp((stem + "_over.bmp").c_str(), w, h, 3, over8_h.data()) == 1 &&
             rtm_write_jpg((stem + "_over.jpg").c_str(), w, h, 3, over8_h.data(), 60) == 1;
    if (!ok) {
        err = "cannot write the matte files of " + stem;
        return RTM_ERR_IO;
    }
    if (over_out) *over_out = std::move(over_h);
    return RTM_OK;
}

// --denoise (rtm_node.h): the frame's AOVs (rtm_render_aov), then rtm_denoise of its f32 at the default parameters on the
// default stream, then the two files.
int rtm_node_write_denoised(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                            const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* f32_out) {
    if (hipSetDevice(opt->device) != hipSuccess) {
        err = "no HIP device " + std::to_string(opt->device);
        return RTM_ERR_NO_DEVICE;
    }
    rtm_scene* scene = nullptr;
    int rc = rtm_scene_create_objects(objects, n, opt->device, &scene);
    if (rc != RTM_OK) {
        err = std::string("scene: ") + rtm_last_error_detail();
        return rc;
    }
    const size_t pix = (size_t)st->width * st->height;
    const size_t work_bytes = rtm_denoise_work_bytes(st->width, st->height);
    rtm_aov_buffers dev;
    std::memset(&dev, 0, sizeof dev);
    float *color = nullptr, *out32 = nullptr;
    uint8_t* out8 = nullptr;
    void* work = nullptr;
    if (hipMalloc((void**)&dev.depth, pix * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.normal, pix * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.albedo, pix * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.object, pix * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&color, pix * 3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&out8, pix * 3) != hipSuccess ||
        (f32_out && hipMalloc((void**)&out32, pix * 3 * sizeof(float)) != hipSuccess) || hipMalloc(&work, work_bytes) != hipSuccess) {
        err = "no device memory for the denoiser's buffers";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && hipMemcpy(color, f32_host, pix * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        err = "copying the frame to the device failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        rc = rtm_render_aov(st, scene, opt, &dev, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc == RTM_OK) {
        const rtm_denoise_params prm = RTM_DENOISE_DEFAULTS;
        rc = rtm_denoise(&prm, st->width, st->height, opt->device, color, &dev, work, out32, out8, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    std::vector<uint8_t> rgb8(pix * 3);
    if (rc == RTM_OK && hipMemcpy(rgb8.data(), out8, pix * 3, hipMemcpyDeviceToHost) != hipSuccess) {
        err = "copying the denoised frame back failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && f32_out) {
        f32_out->resize(pix * 3);
        if (hipMemcpy(f32_out->data(), out32, pix * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            err = "copying the denoised frame back failed";
            rc = RTM_ERR_HIP;
        }
    }
    (void)hipFree(dev.depth);
    (void)hipFree(dev.normal);
    (void)hipFree(dev.albedo);
    (void)hipFree(dev.object);
    (void)hipFree(color);
    (void)hipFree(out32);
    (void)hipFree(out8);
    (void)hipFree(work);
    (void)rtm_scene_destroy(scene);
    if (rc != RTM_OK) return rc;
    const bool ok = rtm_write_jpg((stem + "_denoised.jpg").c_str(), st->width, st->height, 3, rgb8.data(), 60) == 1 &&
                    rtm_write_bmp((stem + "_denoised.bmp").c_str(), st->width, st->height, 3, rgb8.data()) == 1;
    if (!ok) {
        err = "cannot write the denoised files of " + stem;
        return RTM_ERR_IO;
    }
    return RTM_OK;
}

// --denoise-variance (rtm_node.h): as rtm_node_write_denoised with rtm_denoise_variance, plus the variance plane.
int rtm_node_write_denoised_variance(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                                     const float* f32_host, const std::string& stem, std::string& err,
                                     std::vector<float>* f32_out) {
    if (hipSetDevice(opt->device) != hipSuccess) {
        err = "no HIP device " + std::to_string(opt->device);
        return RTM_ERR_NO_DEVICE;
    }
    rtm_scene* scene = nullptr;
    int rc = rtm_scene_create_objects(objects, n, opt->device, &scene);
    if (rc != RTM_OK) {
        err = std::string("scene: ") + rtm_last_error_detail();
        return rc;
    }
    const size_t pix = (size_t)st->width * st->height;
    const size_t work_bytes = rtm_denoise_variance_work_bytes(st->width, st->height);
    rtm_aov_buffers dev;
    std::memset(&dev, 0, sizeof dev);
    float *color = nullptr, *var = nullptr, *out32 = nullptr;
    uint8_t* out8 = nullptr;
    void* work = nullptr;
    if (hipMalloc((void**)&dev.depth, pix * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.normal, pix * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.albedo, pix * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&dev.object, pix * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&color, pix * 3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&out8, pix * 3) != hipSuccess ||
        hipMalloc((void**)&var, pix * sizeof(float)) != hipSuccess ||
        (f32_out && hipMalloc((void**)&out32, pix * 3 * sizeof(float)) != hipSuccess) || hipMalloc(&work, work_bytes) != hipSuccess) {
        err = "no device memory for the denoiser's buffers";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && hipMemcpy(color, f32_host, pix * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        err = "copying the frame to the device failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        rc = rtm_render_aov(st, scene, opt, &dev, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc == RTM_OK) {
        const rtm_denoise_var_params prm = RTM_DENOISE_VAR_DEFAULTS;
        rc = rtm_denoise_variance(&prm, st->width, st->height, opt->device, color, &dev, work, out32, out8, var, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    std::vector<uint8_t> rgb8(pix * 3);
    std::vector<float> variance(pix);
    if (rc == RTM_OK && (hipMemcpy(rgb8.data(), out8, pix * 3, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(variance.data(), var, pix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) {
        err = "copying the denoised frame back failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && f32_out) {
        f32_out->resize(pix * 3);
        if (hipMemcpy(f32_out->data(), out32, pix * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            err = "copying the denoised frame back failed";
            rc = RTM_ERR_HIP;
        }
    }
    (void)hipFree(dev.depth);
    (void)hipFree(dev.normal);
    (void)hipFree(dev.albedo);
    (void)hipFree(dev.object);
    (void)hipFree(color);
    (void)hipFree(out32);
    (void)hipFree(out8);
    (void)hipFree(var);
    (void)hipFree(work);
    (void)rtm_scene_destroy(scene);
    if (rc != RTM_OK) return rc;
    const bool ok = rtm_write_jpg((stem + "_denoised_var.jpg").c_str(), st->width, st->height, 3, rgb8.data(), 60) == 1 &&
                    rtm_write_bmp((stem + "_denoised_var.bmp").c_str(), st->width, st->height, 3, rgb8.data()) == 1 &&
                    rtm_write_pfm((stem + "_variance.pfm").c_str(), st->width, st->height, 1, variance.data()) == 1;
    if (!ok) {
        err = "cannot write the variance-guided denoised files of " + stem;
        return RTM_ERR_IO;
    }
    return RTM_OK;
}

// --display (rtm_node.h): rtm_tonemap of the frame on the default stream, then the two files.
int rtm_node_write_display(const rtm_settings* st, int device, const rtm_tonemap_params* prm, const float* f32_host,
                           const std::string& stem, rtm_tonemap_stats* stats, std::string& err, std::vector<float>* f32_out) {
    if (hipSetDevice(device) != hipSuccess) {
        err = "no HIP device " + std::to_string(device);
        return RTM_ERR_NO_DEVICE;
    }
    const size_t pix = (size_t)st->width * st->height;
    const size_t work_bytes = rtm_tonemap_work_bytes(st->width, st->height);
    float* color = nullptr;
    float* out32 = nullptr;  // only when f32_out is asked for
    uint8_t* out8 = nullptr;
    void* work = nullptr;  // hipMalloc's alignment is 256 bytes or more, what rtm_tonemap asks of work_dev
    rtm_tonemap_stats* stats_dev = nullptr;
    int rc = RTM_OK;
    if (hipMalloc((void**)&color, pix * 3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&out8, pix * 3) != hipSuccess ||
        (f32_out && hipMalloc((void**)&out32, pix * 3 * sizeof(float)) != hipSuccess) ||
        hipMalloc(&work, work_bytes) != hipSuccess || hipMalloc((void**)&stats_dev, sizeof(rtm_tonemap_stats)) != hipSuccess) {
        err = "no device memory for the display transform's buffers";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && hipMemcpy(color, f32_host, pix * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        err = "copying the frame to the device failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        rc = rtm_tonemap(prm, st->width, st->height, device, color, work, out32, out8, stats_dev, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    std::vector<uint8_t> rgb8(pix * 3);
    rtm_tonemap_stats got;
    std::memset(&got, 0, sizeof got);
    if (rc == RTM_OK && (hipMemcpy(rgb8.data(), out8, pix * 3, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(&got, stats_dev, sizeof got, hipMemcpyDeviceToHost) != hipSuccess)) {
        err = "copying the display frame back failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && f32_out) {
        f32_out->resize(pix * 3);
        if (hipMemcpy(f32_out->data(), out32, pix * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            err = "copying the display frame back failed";
            rc = RTM_ERR_HIP;
        }
    }
    (void)hipFree(color);
    (void)hipFree(out32);
    (void)hipFree(out8);
    (void)hipFree(work);
    (void)hipFree(stats_dev);
    if (rc != RTM_OK) return rc;
    if (stats) *stats = got;
    const bool ok = rtm_write_jpg((stem + "_display.jpg").c_str(), st->width, st->height, 3, rgb8.data(), 60) == 1 &&
                    rtm_write_bmp((stem + "_display.bmp").c_str(), st->width, st->height, 3, rgb8.data()) == 1;
    if (!ok) {
        err = "cannot write the display files of " + stem;
        return RTM_ERR_IO;
    }
    return RTM_OK;
}

// --bloom (rtm_node.h): rtm_bloom of the frame, in place, on the default stream.
int rtm_node_bloom(const rtm_settings* st, int device, const rtm_bloom_params* prm, const float* f32_host,
                   std::vector<float>* f32_out, std::string& err) {
    if (hipSetDevice(device) != hipSuccess) {
        err = "no HIP device " + std::to_string(device);
        return RTM_ERR_NO_DEVICE;
    }
    const size_t bytes = (size_t)st->width * st->height * 3 * sizeof(float);
    const size_t work_bytes = rtm_bloom_work_bytes(st->width, st->height, prm->levels);
    float* color = nullptr;
    void* work = nullptr;  // hipMalloc's alignment is 256 bytes or more, what rtm_bloom asks of work_dev
    int rc = RTM_OK;
    if (work_bytes == 0 || work_bytes == SIZE_MAX) {
        err = "bloom's frame size or levels are out of range";
        rc = RTM_ERR_INVALID_ARGUMENT;
    } else if (hipMalloc((void**)&color, bytes) != hipSuccess || hipMalloc(&work, work_bytes) != hipSuccess) {
        err = "no device memory for bloom's buffers";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && hipMemcpy(color, f32_host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        err = "copying the frame to the device failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        rc = rtm_bloom(prm, st->width, st->height, device, color, work, color, nullptr, nullptr, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc == RTM_OK) {
        f32_out->resize(bytes / sizeof(float));
        if (hipMemcpy(f32_out->data(), color, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
            err = "copying the bloomed frame back failed";
            rc = RTM_ERR_HIP;
        }
    }
    (void)hipFree(color);
    (void)hipFree(work);
    return rc;
}

// --compare (rtm_node.h): rtm_compare of the two frames on the default stream.
int rtm_node_compare(const rtm_settings* st, int device, const float* frame_host, const float* reference_host,
                     rtm_compare_result* result, std::string& err) {
    if (hipSetDevice(device) != hipSuccess) {
        err = "no HIP device " + std::to_string(device);
        return RTM_ERR_NO_DEVICE;
    }
    const size_t bytes = (size_t)st->width * st->height * 3 * sizeof(float);
    const size_t work_bytes = rtm_compare_work_bytes(st->width, st->height);
    float *a = nullptr, *b = nullptr;
    void* work = nullptr;  // hipMalloc's alignment is 256 bytes or more, what rtm_compare asks of work_dev
    rtm_compare_result* result_dev = nullptr;
    int rc = RTM_OK;
    if (hipMalloc((void**)&a, bytes) != hipSuccess || hipMalloc((void**)&b, bytes) != hipSuccess ||
        hipMalloc(&work, work_bytes) != hipSuccess || hipMalloc((void**)&result_dev, sizeof(rtm_compare_result)) != hipSuccess) {
        err = "no device memory for the comparison's buffers";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && (hipMemcpy(a, frame_host, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                         hipMemcpy(b, reference_host, bytes, hipMemcpyHostToDevice) != hipSuccess)) {
        err = "copying the frames to the device failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        const rtm_compare_params prm = RTM_COMPARE_DEFAULTS;
        rc = rtm_compare(&prm, st->width, st->height, device, a, b, work, result_dev, nullptr, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc == RTM_OK && hipMemcpy(result, result_dev, sizeof *result, hipMemcpyDeviceToHost) != hipSuccess) {
        err = "copying the comparison's record back failed";
        rc = RTM_ERR_HIP;
    }
    (void)hipFree(a);
    (void)hipFree(b);
    (void)hipFree(work);
    (void)hipFree(result_dev);
    return rc;
}

// --flip (rtm_node.h): rtm_flip of the two frames on the default stream.
int rtm_node_flip(const rtm_settings* st, int device, const rtm_flip_params* prm, const float* frame_host,
                  const float* reference_host, rtm_flip_result* result, std::vector<float>* map_out, std::string& err) {
    if (hipSetDevice(device) != hipSuccess) {
        err = "no HIP device " + std::to_string(device);
        return RTM_ERR_NO_DEVICE;
    }
    const size_t pix = (size_t)st->width * st->height;
    const size_t bytes = pix * 3 * sizeof(float);
    const size_t work_bytes = rtm_flip_work_bytes(st->width, st->height);
    float *a = nullptr, *b = nullptr, *map_dev = nullptr;
    void* work = nullptr;  // hipMalloc's alignment is 256 bytes or more, what rtm_flip asks of work_dev
    rtm_flip_result* result_dev = nullptr;
    int rc = RTM_OK;
    if (work_bytes == SIZE_MAX || hipMalloc((void**)&a, bytes) != hipSuccess || hipMalloc((void**)&b, bytes) != hipSuccess ||
        hipMalloc(&work, work_bytes) != hipSuccess || hipMalloc((void**)&result_dev, sizeof(rtm_flip_result)) != hipSuccess ||
        (map_out && hipMalloc((void**)&map_dev, pix * sizeof(float)) != hipSuccess)) {
        err = "no device memory for the perceptual difference's buffers";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && (hipMemcpy(a, frame_host, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                         hipMemcpy(b, reference_host, bytes, hipMemcpyHostToDevice) != hipSuccess)) {
        err = "copying the frames to the device failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        rc = rtm_flip(prm, st->width, st->height, device, a, b, work, result_dev, map_dev, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc == RTM_OK && hipMemcpy(result, result_dev, sizeof *result, hipMemcpyDeviceToHost) != hipSuccess) {
        err = "copying the perceptual difference's record back failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && map_out) {
        map_out->resize(pix);
        if (hipMemcpy(map_out->data(), map_dev, pix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            err = "copying the perceptual difference's map back failed";
            rc = RTM_ERR_HIP;
        }
    }
    (void)hipFree(a);
    (void)hipFree(b);
    (void)hipFree(map_dev);
    (void)hipFree(work);
    (void)hipFree(result_dev);
    return rc;
}

// --preview (rtm_node.h): the low render, its AOVs and rtm_denoise, the full AOVs, rtm_upsample, all on the default stream,
// then the two files.
int rtm_node_write_preview(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt, int factor,
                           const std::string& stem, std::string& err, std::vector<float>* f32_out, rtm_stats* stats) {
    if (factor < 2 || factor > 8 || st->width % factor != 0 || st->height % factor != 0) {
        err = "--preview " + std::to_string(factor) + ": a factor in 2..8 that divides the width and the height";
        return RTM_ERR_INVALID_ARGUMENT;
    }
    if (hipSetDevice(opt->device) != hipSuccess) {
        err = "no HIP device " + std::to_string(opt->device);
        return RTM_ERR_NO_DEVICE;
    }
    rtm_scene* scene = nullptr;
    int rc = rtm_scene_create_objects(objects, n, opt->device, &scene);
    if (rc != RTM_OK) {
        err = std::string("scene: ") + rtm_last_error_detail();
        return rc;
    }
    rtm_settings lo_st = *st;
    lo_st.width = st->width / factor;
    lo_st.height = st->height / factor;
    rtm_options lo_opt = *opt;
    lo_opt.row_begin = 0;
    lo_opt.row_end = lo_st.height;
    const size_t lo_pix = (size_t)lo_st.width * lo_st.height, pix = (size_t)st->width * st->height;
    rtm_aov_buffers lo, hi;
    std::memset(&lo, 0, sizeof lo);
    std::memset(&hi, 0, sizeof hi);
    float *color = nullptr, *den = nullptr, *out32 = nullptr;
    uint8_t* out8 = nullptr;
    void *dn_work = nullptr, *up_work = nullptr;
    auto planes = [](rtm_aov_buffers& b, size_t p) {
        return hipMalloc((void**)&b.depth, p * sizeof(float)) == hipSuccess && hipMalloc((void**)&b.normal, p * 3 * sizeof(float)) == hipSuccess &&
               hipMalloc((void**)&b.albedo, p * 3 * sizeof(float)) == hipSuccess && hipMalloc((void**)&b.object, p * sizeof(int32_t)) == hipSuccess;
    };
    if (!planes(lo, lo_pix) || !planes(hi, pix) || hipMalloc((void**)&color, lo_pix * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&den, lo_pix * 3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&out8, pix * 3) != hipSuccess ||
        (f32_out && hipMalloc((void**)&out32, pix * 3 * sizeof(float)) != hipSuccess) ||
        hipMalloc(&dn_work, rtm_denoise_work_bytes(lo_st.width, lo_st.height)) != hipSuccess ||
        hipMalloc(&up_work, rtm_upsample_work_bytes(lo_st.width, lo_st.height)) != hipSuccess) {
        err = "no device memory for the preview's buffers";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK) {
        rc = rtm_render_scene(&lo_st, scene, &lo_opt, nullptr, color, nullptr, nullptr, stats);
        if (rc == RTM_OK) rc = rtm_render_aov(&lo_st, scene, &lo_opt, &lo, nullptr);
        if (rc == RTM_OK) {
            const rtm_denoise_params prm = RTM_DENOISE_DEFAULTS;
            rc = rtm_denoise(&prm, lo_st.width, lo_st.height, opt->device, color, &lo, dn_work, den, nullptr, nullptr);
        }
        if (rc == RTM_OK) rc = rtm_render_aov(st, scene, opt, &hi, nullptr);
        if (rc == RTM_OK) {
            rtm_upsample_params prm = RTM_UPSAMPLE_DEFAULTS;
            prm.factor = factor;
            rc = rtm_upsample(&prm, lo_st.width, lo_st.height, opt->device, den, &lo, &hi, up_work, out32, out8, nullptr);
        }
        if (rc == RTM_OK) rc = rtm_stream_status(opt->device, nullptr);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    std::vector<uint8_t> rgb8(pix * 3);
    if (rc == RTM_OK && hipMemcpy(rgb8.data(), out8, pix * 3, hipMemcpyDeviceToHost) != hipSuccess) {
        err = "copying the preview back failed";
        rc = RTM_ERR_HIP;
    }
    if (rc == RTM_OK && f32_out) {
        f32_out->resize(pix * 3);
        if (hipMemcpy(f32_out->data(), out32, pix * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            err = "copying the preview back failed";
            rc = RTM_ERR_HIP;
        }
    }
    for (rtm_aov_buffers* b : {&lo, &hi}) {
        (void)hipFree(b->depth);
        (void)hipFree(b->normal);
        (void)hipFree(b->albedo);
        (void)hipFree(b->object);
    }
    (void)hipFree(color);
    (void)hipFree(den);
    (void)hipFree(out32);
    (void)hipFree(out8);
    (void)hipFree(dn_work);
    (void)hipFree(up_work);
    (void)rtm_scene_destroy(scene);
    if (rc != RTM_OK) return rc;
    const bool ok = rtm_write_jpg((stem + "_preview.jpg").c_str(), st->width, st->height, 3, rgb8.data(), 60) == 1 &&
                    rtm_write_bmp((stem + "_preview.bmp").c_str(), st->width, st->height, 3, rgb8.data()) == 1;
    if (!ok) {
        err = "cannot write the preview files of " + stem;
        return RTM_ERR_IO;
    }
    return RTM_OK;
}
