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
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
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

// What the one-GPU stages below (--passes, --adaptive and every stage that follows the render) share.  Their device
// arrays and scenes are owned, so a stage returns at its first failure and everything it holds is released.

// A device array of `count` T (bytes for void), freed with its owner.  Until alloc succeeds with a count above zero it
// holds null, which is what the library calls take for an output that is not asked for.
template <class T>
struct DevBuf {
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p_) (void)hipFree(p_);
    }
    // wanted == false: not asked for, nothing is allocated and that is no failure
    bool alloc(size_t count, bool wanted = true) { return !wanted || hipMalloc((void**)&p_, count * kSize) == hipSuccess; }
    bool upload(const T* host, size_t count) { return hipMemcpy(p_, host, count * kSize, hipMemcpyHostToDevice) == hipSuccess; }
    bool download(T* host, size_t count) const { return hipMemcpy(host, p_, count * kSize, hipMemcpyDeviceToHost) == hipSuccess; }
    T* get() const { return p_; }

  private:
    static constexpr size_t kSize = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    T* p_ = nullptr;
};

// A scene handle, destroyed with its owner.
struct Scene {
    Scene() = default;
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    ~Scene() {
        if (s_) (void)rtm_scene_destroy(s_);
    }
    int create(const rtm_object* objects, size_t n, int device) { return rtm_scene_create_objects(objects, n, device, &s_); }
    rtm_scene* get() const { return s_; }

  private:
    rtm_scene* s_ = nullptr;
};

// The first-hit feature planes of `pix` pixels; the object ids only where the stage reads them.
struct AovPlanes {
    DevBuf<float> depth, normal, albedo;
    DevBuf<int32_t> object;
    bool alloc(size_t pix, bool with_object) {
        return depth.alloc(pix) && normal.alloc(pix * 3) && albedo.alloc(pix * 3) && object.alloc(pix, with_object);
    }
    rtm_aov_buffers view() const { return rtm_aov_buffers{depth.get(), normal.get(), albedo.get(), object.get()}; }
};

int fail(std::string& err, int rc, const std::string& text) {
    err = text;
    return rc;
}
int open_device(int device, std::string& err) {
    if (hipSetDevice(device) != hipSuccess) return fail(err, RTM_ERR_NO_DEVICE, "no HIP device " + std::to_string(device));
    return RTM_OK;
}
int open_scene(const rtm_object* objects, size_t n, int device, Scene& scene, std::string& err) {
    if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
    const int rc = scene.create(objects, n, device);
    return rc == RTM_OK ? rc : fail(err, rc, std::string("scene: ") + rtm_last_error_detail());
}

// the counters of one part or pass into the frame's; kernel_ms is the caller's (parts overlap in time, passes do not)
void add_counts(rtm_stats* total, const rtm_stats& s) {
    total->samples += s.samples;
    total->casts += s.casts;
    total->bounces += s.bounces;
    total->draws += s.draws;
    total->variant = s.variant;
}
// the u8 frame back, and the f32 frame when asked; a null host pointer: not asked for
bool frame_back(const DevBuf<uint8_t>& d8, uint8_t* u8_host, const DevBuf<float>& d32, float* f32_host, size_t vals) {
    return (!u8_host || d8.download(u8_host, vals)) && (!f32_host || d32.download(f32_host, vals));
}
// a nullable output vector at its size: where frame_back copies to
float* sized(std::vector<float>* v, size_t count) {
    if (!v) return nullptr;
    v->resize(count);
    return v->data();
}
// <name>.jpg at the reference's quality 60 and <name>.bmp
bool write_jpg_bmp(const std::string& name, const rtm_settings* st, const uint8_t* rgb8) {
    return rtm_write_jpg((name + ".jpg").c_str(), st->width, st->height, 3, rgb8, 60) == 1 &&
           rtm_write_bmp((name + ".bmp").c_str(), st->width, st->height, 3, rgb8) == 1;
}
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
            add_counts(total, s);
            // parts on different GPUs overlap in time: the frame's kernel time is the longest part;
            // virtual parts on one GPU run back to back
            total->kernel_ms = virtual_strips > 0 ? total->kernel_ms + s.kernel_ms
                                                  : (s.kernel_ms > total->kernel_ms ? s.kernel_ms : total->kernel_ms);
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
    if (passes < 1 || (unsigned)passes > N)
        return fail(err, RTM_ERR_INVALID_ARGUMENT,
                    "--passes " + std::to_string(passes) + ": must be in [1, " + std::to_string(N) + "] (the frame's samples per pixel)");
    Scene scene;
    if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
    const size_t vals = (size_t)st->width * st->height * 3;
    DevBuf<double> accum;
    DevBuf<float> d32;
    DevBuf<uint8_t> d8;
    if (!accum.alloc(vals) || !d32.alloc(vals, out_f32_host != nullptr) || !d8.alloc(vals, out_u8_host != nullptr))
        return fail(err, RTM_ERR_HIP, "no device memory for the frame");
    std::memset(total, 0, sizeof *total);
    const unsigned q = N / (unsigned)passes, r = N % (unsigned)passes;
    unsigned a = 0;
    for (int i = 0; i < passes; ++i) {
        const unsigned b = a + q + ((unsigned)i < r ? 1u : 0u);
        rtm_stats s;
        const int rc = rtm_render_scene_samples(st, scene.get(), opt, a, b, accum.get(), d32.get(), d8.get(), nullptr, &s);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        std::printf("pass %d/%d: samples [%u, %u) %.3f ms\n", i + 1, passes, a, b, s.kernel_ms);
        add_counts(total, s);
        total->kernel_ms += s.kernel_ms;
        a = b;
    }
    if (!frame_back(d8, out_u8_host, d32, out_f32_host, vals)) return fail(err, RTM_ERR_HIP, "copying the frame back failed");
    return RTM_OK;
}

// --adaptive (rtm_node.h): rtm_render_adaptive of the whole frame on the default stream, outputs and sample map copied back.
int rtm_node_render_adaptive(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                             const rtm_adaptive_params* prm, float* out_f32_host, uint8_t* out_u8_host,
                             std::vector<uint32_t>& tile_samples, rtm_stats* total, std::string& err) {
    Scene scene;
    if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
    const size_t vals = (size_t)st->width * st->height * 3;
    const size_t tiles = (size_t)((st->width + 7) / 8) * (size_t)((st->height + 7) / 8);
    tile_samples.assign(tiles, 0u);
    DevBuf<double> accum;
    DevBuf<float> d32;
    DevBuf<uint8_t> d8;
    DevBuf<uint32_t> dts;
    DevBuf<void> work;
    if (!accum.alloc(vals) || !d32.alloc(vals, out_f32_host != nullptr) || !d8.alloc(vals, out_u8_host != nullptr) ||
        !dts.alloc(tiles) || !work.alloc(rtm_adaptive_work_bytes(st, opt)))
        return fail(err, RTM_ERR_HIP, "no device memory for the frame");
    const int rc = rtm_render_adaptive(st, scene.get(), opt, prm, accum.get(), d32.get(), d8.get(), dts.get(), work.get(), nullptr, total);
    if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
    if (!frame_back(d8, out_u8_host, d32, out_f32_host, vals) || !dts.download(tile_samples.data(), tiles))
        return fail(err, RTM_ERR_HIP, "copying the frame back failed");
    double sum = 0.0;
    for (size_t t = 0; t < tiles; ++t) {
        const int tx = (int)(t % (size_t)((st->width + 7) / 8)), ty = (int)(t / (size_t)((st->width + 7) / 8));
        sum += (double)tile_samples[t] * std::min(8, st->width - 8 * tx) * std::min(8, st->height - 8 * ty);
    }
    std::printf("adaptive: threshold %g, min_samples %u: mean %.2f samples per pixel of %d\n", (double)prm->threshold,
                prm->min_samples, sum / ((double)st->width * st->height), st->super_samples * st->super_samples * st->samples);
    return RTM_OK;
}

// --aov (rtm_node.h): one rtm_render_aov of the frame on the default stream, then the five files.
int rtm_node_write_aov(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                       const std::string& stem, std::string& err) {
    const size_t pix = (size_t)st->width * st->height;
    std::vector<float> depth(pix), normal(pix * 3), albedo(pix * 3);
    {  // the device's part; what it holds is released before the files are written
        Scene scene;
        if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
        AovPlanes planes;
        if (!planes.alloc(pix, false)) return fail(err, RTM_ERR_HIP, "no device memory for the AOV planes");
        const rtm_aov_buffers dev = planes.view();
        const int rc = rtm_render_aov(st, scene.get(), opt, &dev, nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!planes.depth.download(depth.data(), pix) || !planes.normal.download(normal.data(), pix * 3) ||
            !planes.albedo.download(albedo.data(), pix * 3))
            return fail(err, RTM_ERR_HIP, "copying the AOV planes back failed");
    }
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
    if (!ok) return fail(err, RTM_ERR_IO, "cannot write the AOV files of " + stem);
    return RTM_OK;
}

// --alpha / --matte / --background (rtm_node.h): one rtm_render_mattes of the frame on the default stream (the layers only
// when a matte is asked for), then rtm_matte and rtm_composite behind it, then the files.
int rtm_node_write_mattes(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt, bool want_alpha,
                          int layers, const std::vector<int32_t>& ids, const rtm_composite_params* background,
                          const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* over_out) {
    const size_t pix = (size_t)st->width * st->height;
    const bool want_matte = !ids.empty(), want_over = background != nullptr;
    std::vector<float> alpha_h(pix), matte_h(want_matte ? pix : 0), over_h(want_over && over_out ? pix * 3 : 0);
    std::vector<uint8_t> over8_h(want_over ? pix * 3 : 0);
    {  // the device's part; what it holds is released before the files are written
        Scene scene;
        if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
        DevBuf<float> alpha;
        DevBuf<int32_t> id;
        DevBuf<float> coverage;
        DevBuf<int32_t> sel;
        DevBuf<float> matte;
        DevBuf<float> color;  // the frame, composited in place
        DevBuf<uint8_t> over8;
        if (!alpha.alloc(pix) || !id.alloc(pix * layers, want_matte) || !coverage.alloc(pix * layers, want_matte) ||
            !sel.alloc(ids.size(), want_matte) || !matte.alloc(pix, want_matte) || !color.alloc(pix * 3, want_over) ||
            !over8.alloc(pix * 3, want_over))
            return fail(err, RTM_ERR_HIP, "no device memory for the coverage planes");
        if ((want_matte && !sel.upload(ids.data(), ids.size())) || (want_over && !color.upload(f32_host, pix * 3)))
            return fail(err, RTM_ERR_HIP, "copying the id list or the frame to the device failed");
        const rtm_matte_buffers dev = {id.get(), coverage.get(), alpha.get()};
        int rc = rtm_render_mattes(st, scene.get(), opt, layers, &dev, nullptr);
        if (rc == RTM_OK && want_matte)
            rc = rtm_matte(st->width, st->height, layers, opt->device, dev.id, dev.coverage, sel.get(), (int32_t)ids.size(), matte.get(),
                           nullptr);
        if (rc == RTM_OK && want_over)
            rc = rtm_composite(background, st->width, st->height, opt->device, color.get(), dev.alpha, nullptr, color.get(), over8.get(),
                               nullptr);
        if (rc != RTM_OK) return err.empty() ? fail(err, rc, rtm_last_error_detail()) : rc;
        if (!alpha.download(alpha_h.data(), pix) || (want_matte && !matte.download(matte_h.data(), pix)) ||
            (want_over && !over8.download(over8_h.data(), pix * 3)) || (!over_h.empty() && !color.download(over_h.data(), pix * 3)))
            return fail(err, RTM_ERR_HIP, "copying the coverage planes back failed");
    }
    const int w = st->width, h = st->height;
    bool ok = !want_alpha || rtm_write_pfm((stem + "_alpha.pfm").c_str(), w, h, 1, alpha_h.data()) == 1;
    if (want_matte) {
        std::vector<double> v(pix * 3);
        std::vector<uint8_t> grey(pix * 3);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (double)matte_h[i / 3];
        ok = ok && rtm_write_pfm((stem + "_matte.pfm").c_str(), w, h, 1, matte_h.data()) == 1 &&
             rtm_quantise(v.data(), v.size(), grey.data()) == RTM_OK && rtm_write_bmp((stem + "_matte.bmp").c_str(), w, h, 3, grey.data()) == 1;
    }
    if (want_over)
        ok = ok && rtm_write_bmp((stem + "_over.bmp").c_str(), w, h, 3, over8_h.data()) == 1 &&
             rtm_write_jpg((stem + "_over.jpg").c_str(), w, h, 3, over8_h.data(), 60) == 1;
    if (!ok) return fail(err, RTM_ERR_IO, "cannot write the matte files of " + stem);
    if (over_out) *over_out = std::move(over_h);
    return RTM_OK;
}

namespace {
// --denoise and --denoise-variance: the frame's AOVs (rtm_render_aov), then rtm_denoise or rtm_denoise_variance of its f32
// at the default parameters on the default stream, then the files.  The variance-guided one has a variance plane more, its
// own work size, "_var" in its file names and <stem>_variance.pfm.
int write_denoised(bool variance, const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                   const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* f32_out) {
    const int w = st->width, h = st->height;
    const size_t pix = (size_t)w * h;
    std::vector<uint8_t> rgb8(pix * 3);
    std::vector<float> variance_h(variance ? pix : 0);
    {  // the device's part; what it holds is released before the files are written
        Scene scene;
        if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
        const size_t work_bytes = variance ? rtm_denoise_variance_work_bytes(w, h) : rtm_denoise_work_bytes(w, h);
        AovPlanes planes;
        DevBuf<float> color;
        DevBuf<uint8_t> out8;
        DevBuf<float> var, out32;
        DevBuf<void> work;
        if (!planes.alloc(pix, true) || !color.alloc(pix * 3) || !out8.alloc(pix * 3) || !var.alloc(pix, variance) ||
            !out32.alloc(pix * 3, f32_out != nullptr) || !work.alloc(work_bytes))
            return fail(err, RTM_ERR_HIP, "no device memory for the denoiser's buffers");
        if (!color.upload(f32_host, pix * 3)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
        const rtm_aov_buffers dev = planes.view();
        int rc = rtm_render_aov(st, scene.get(), opt, &dev, nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (variance) {
            const rtm_denoise_var_params prm = RTM_DENOISE_VAR_DEFAULTS;
            rc = rtm_denoise_variance(&prm, w, h, opt->device, color.get(), &dev, work.get(), out32.get(), out8.get(), var.get(), nullptr);
        } else {
            const rtm_denoise_params prm = RTM_DENOISE_DEFAULTS;
            rc = rtm_denoise(&prm, w, h, opt->device, color.get(), &dev, work.get(), out32.get(), out8.get(), nullptr);
        }
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!frame_back(out8, rgb8.data(), out32, sized(f32_out, pix * 3), pix * 3) || (variance && !var.download(variance_h.data(), pix)))
            return fail(err, RTM_ERR_HIP, "copying the denoised frame back failed");
    }
    const bool ok = write_jpg_bmp(stem + (variance ? "_denoised_var" : "_denoised"), st, rgb8.data()) &&
                    (!variance || rtm_write_pfm((stem + "_variance.pfm").c_str(), w, h, 1, variance_h.data()) == 1);
    if (!ok)
        return fail(err, RTM_ERR_IO, std::string("cannot write the ") + (variance ? "variance-guided " : "") + "denoised files of " + stem);
    return RTM_OK;
}
}  // namespace

// --denoise (rtm_node.h)
int rtm_node_write_denoised(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                            const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* f32_out) {
    return write_denoised(false, st, objects, n, opt, f32_host, stem, err, f32_out);
}

// --denoise-variance (rtm_node.h)
int rtm_node_write_denoised_variance(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                                     const float* f32_host, const std::string& stem, std::string& err,
                                     std::vector<float>* f32_out) {
    return write_denoised(true, st, objects, n, opt, f32_host, stem, err, f32_out);
}

// --display (rtm_node.h): rtm_tonemap of the frame on the default stream, with --lut the look and the second rtm_tonemap
// behind it, then the two files.  --display local: a statistics-only rtm_tonemap, rtm_tonemap_local in place, and an
// rtm_tonemap that only clamps, encodes and stores in the curve's stead.
int rtm_node_write_display(const rtm_settings* st, int device, const rtm_tonemap_params* prm, const float* f32_host,
                           const std::string& stem, rtm_tonemap_stats* stats, std::string& err, std::vector<float>* f32_out,
                           const rtm_node_lut* lut, const rtm_tonemap_local_params* local) {
    const size_t pix = (size_t)st->width * st->height;
    std::vector<uint8_t> rgb8(pix * 3);
    rtm_tonemap_stats got;
    std::memset(&got, 0, sizeof got);
    {  // the device's part; what it holds is released before the files are written
        if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
        const size_t work_bytes = rtm_tonemap_work_bytes(st->width, st->height);
        DevBuf<float> color;
        DevBuf<uint8_t> out8;
        DevBuf<float> out32;  // only when f32_out is asked for, or the look takes it
        DevBuf<float> table;  // only with a look
        DevBuf<void> work;    // hipMalloc's alignment is 256 bytes or more, what rtm_tonemap asks of work_dev
        DevBuf<rtm_tonemap_stats> stats_dev;
        DevBuf<void> pyramid;  // only with the local operator at levels > 0
        const size_t pyramid_bytes = local ? rtm_tonemap_local_work_bytes(st->width, st->height, local->levels) : 0;
        if (pyramid_bytes == SIZE_MAX) return fail(err, RTM_ERR_INVALID_ARGUMENT, "the local tone operator's frame size is out of range");
        if (!color.alloc(pix * 3) || !out8.alloc(pix * 3) || !out32.alloc(pix * 3, f32_out != nullptr || lut != nullptr) ||
            !table.alloc(lut ? lut->table.size() : 0, lut != nullptr) || !work.alloc(work_bytes) || !stats_dev.alloc(1) ||
            !pyramid.alloc(pyramid_bytes, pyramid_bytes != 0))
            return fail(err, RTM_ERR_HIP, "no device memory for the display transform's buffers");
        if (!color.upload(f32_host, pix * 3)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
        if (lut && !table.upload(lut->table.data(), lut->table.size())) return fail(err, RTM_ERR_HIP, "copying the LUT to the device failed");
        int rc;
        if (local) {
            // the statistics of the shown curve's key (and the line rtm_cli prints), then the operator in place with that
            // call's E by stream order, or with 2^ev in the anchor; the curve left to rtm_tonemap is the clamp
            rtm_tonemap_local_params fuse = *local;
            fuse.anchor = prm->auto_exposure ? 1.0f : exp2f(prm->ev);
            rtm_tonemap_params store = *prm;
            store.op = RTM_TONEMAP_CLAMP;
            store.auto_exposure = 0;
            store.ev = 0.0f;
            rc = rtm_tonemap(prm, st->width, st->height, device, color.get(), work.get(), nullptr, nullptr, stats_dev.get(), nullptr);
            if (rc == RTM_OK)
                rc = rtm_tonemap_local(&fuse, st->width, st->height, device, color.get(), prm->auto_exposure ? stats_dev.get() : nullptr,
                                       pyramid.get(), color.get(), nullptr, nullptr, nullptr);
            if (rc == RTM_OK)
                rc = rtm_tonemap(&store, st->width, st->height, device, color.get(), work.get(), out32.get(), lut ? nullptr : out8.get(),
                                 nullptr, nullptr);
        } else {
            rc = rtm_tonemap(prm, st->width, st->height, device, color.get(), work.get(), out32.get(), lut ? nullptr : out8.get(),
                             stats_dev.get(), nullptr);
        }
        if (rc == RTM_OK && lut) {
            rtm_tonemap_params store = RTM_TONEMAP_DEFAULTS;  // the look's frame to 8 bits: clamp and dither, nothing else
            store.op = RTM_TONEMAP_CLAMP;
            store.transfer = RTM_TRANSFER_LINEAR;
            store.auto_exposure = 0;
            store.ev = 0.0f;
            store.dither = prm->dither;
            rc = rtm_grade(&lut->params, st->width, st->height, device, out32.get(), table.get(), out32.get(), nullptr, nullptr);
            if (rc == RTM_OK)
                rc = rtm_tonemap(&store, st->width, st->height, device, out32.get(), work.get(), out32.get(), out8.get(), nullptr, nullptr);
        }
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!frame_back(out8, rgb8.data(), out32, sized(f32_out, pix * 3), pix * 3) || !stats_dev.download(&got, 1))
            return fail(err, RTM_ERR_HIP, "copying the display frame back failed");
    }
    if (stats) *stats = got;
    if (!write_jpg_bmp(stem + "_display", st, rgb8.data())) return fail(err, RTM_ERR_IO, "cannot write the display files of " + stem);
    return RTM_OK;
}

// --grade-... (rtm_node.h): rtm_grade of the frame, in place, on the default stream.
int rtm_node_grade(const rtm_settings* st, int device, const rtm_grade_params* prm, const float* f32_host,
                   std::vector<float>* f32_out, std::string& err) {
    if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
    const size_t vals = (size_t)st->width * st->height * 3;
    DevBuf<float> color;
    if (!color.alloc(vals)) return fail(err, RTM_ERR_HIP, "no device memory for the grade's buffer");
    if (!color.upload(f32_host, vals)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
    const int rc = rtm_grade(prm, st->width, st->height, device, color.get(), nullptr, color.get(), nullptr, nullptr);
    if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
    if (!color.download(sized(f32_out, vals), vals)) return fail(err, RTM_ERR_HIP, "copying the graded frame back failed");
    return RTM_OK;
}

// --bloom (rtm_node.h): rtm_bloom of the frame, in place, on the default stream.
int rtm_node_bloom(const rtm_settings* st, int device, const rtm_bloom_params* prm, const float* f32_host,
                   std::vector<float>* f32_out, std::string& err) {
    if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
    const size_t vals = (size_t)st->width * st->height * 3;
    const size_t work_bytes = rtm_bloom_work_bytes(st->width, st->height, prm->levels);
    DevBuf<float> color;
    DevBuf<void> work;  // hipMalloc's alignment is 256 bytes or more, what rtm_bloom asks of work_dev
    if (work_bytes == 0 || work_bytes == SIZE_MAX)
        return fail(err, RTM_ERR_INVALID_ARGUMENT, "bloom's frame size or levels are out of range");
    if (!color.alloc(vals) || !work.alloc(work_bytes)) return fail(err, RTM_ERR_HIP, "no device memory for bloom's buffers");
    if (!color.upload(f32_host, vals)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
    const int rc = rtm_bloom(prm, st->width, st->height, device, color.get(), work.get(), color.get(), nullptr, nullptr, nullptr);
    if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
    if (!color.download(sized(f32_out, vals), vals)) return fail(err, RTM_ERR_HIP, "copying the bloomed frame back failed");
    return RTM_OK;
}

// --firefly (rtm_node.h): rtm_firefly of the frame on the default stream, the mask counted on the host, then the two files.
int rtm_node_write_firefly(const rtm_settings* st, int device, const rtm_firefly_params* prm, const float* f32_host,
                           const std::string& stem, std::string& err, std::vector<float>* f32_out, size_t* clamped,
                           size_t* repaired) {
    const size_t pix = (size_t)st->width * st->height, vals = pix * 3;
    std::vector<uint8_t> rgb8(vals), mask(pix);
    {  // the device's part; what it holds is released before the files are written
        if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
        DevBuf<float> color, out32;
        DevBuf<uint8_t> out8, mask_dev;
        if (!color.alloc(vals) || !out32.alloc(vals) || !out8.alloc(vals) || !mask_dev.alloc(pix))
            return fail(err, RTM_ERR_HIP, "no device memory for firefly's buffers");
        if (!color.upload(f32_host, vals)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
        const int rc = rtm_firefly(prm, st->width, st->height, device, color.get(), out32.get(), out8.get(), mask_dev.get(), nullptr,
                                   nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!frame_back(out8, rgb8.data(), out32, sized(f32_out, vals), vals) || !mask_dev.download(mask.data(), pix))
            return fail(err, RTM_ERR_HIP, "copying the cleaned frame back failed");
    }
    size_t ones = 0, twos = 0;
    for (const uint8_t m : mask) {
        ones += m == 1;
        twos += m == 2;
    }
    if (clamped) *clamped = ones;
    if (repaired) *repaired = twos;
    if (!write_jpg_bmp(stem + "_firefly", st, rgb8.data())) return fail(err, RTM_ERR_IO, "cannot write the firefly files of " + stem);
    return RTM_OK;
}

// --scopes (rtm_node.h): rtm_scopes of the frame on the default stream, and rtm_scope_draw of its waveform.
int rtm_node_scopes(const rtm_settings* st, int device, const rtm_scope_params* prm, const float* f32_host,
                    rtm_scope_histogram* hist, int layout, uint32_t gain, std::vector<uint8_t>* picture, std::string& err) {
    const size_t vals = (size_t)st->width * st->height * 3;
    if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
    const size_t words = picture ? (size_t)4 * 256 * (size_t)(prm->columns > 0 ? prm->columns : 0) : 0;
    const size_t bytes = picture ? (size_t)256 * 3 * (size_t)prm->columns * (layout == RTM_SCOPE_PARADE ? 3 : 1) : 0;
    DevBuf<float> color;
    DevBuf<rtm_scope_histogram> hist_dev;
    DevBuf<uint32_t> wave;
    DevBuf<uint8_t> drawn;
    if (!color.alloc(vals) || !hist_dev.alloc(1) || !wave.alloc(words, picture != nullptr) || !drawn.alloc(bytes, picture != nullptr))
        return fail(err, RTM_ERR_HIP, "no device memory for the scopes' buffers");
    if (!color.upload(f32_host, vals)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
    int rc = rtm_scopes(prm, st->width, st->height, device, color.get(), hist_dev.get(), picture ? wave.get() : nullptr, nullptr);
    if (rc == RTM_OK && picture) rc = rtm_scope_draw(prm->columns, layout, gain, device, wave.get(), drawn.get(), nullptr);
    if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
    if (picture) picture->resize(bytes);
    if (!hist_dev.download(hist, 1) || (picture && !drawn.download(picture->data(), bytes)))
        return fail(err, RTM_ERR_HIP, "copying the scopes back failed");
    return RTM_OK;
}

// --dof (rtm_node.h): the depth plane and rtm_defocus of the frame behind it on the default stream, then the two files.
int rtm_node_write_dof(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                       const rtm_defocus_params* prm, const float* f32_host, const std::string& stem, std::string& err,
                       std::vector<float>* f32_out) {
    const int w = st->width, h = st->height;
    const size_t pix = (size_t)w * h;
    std::vector<uint8_t> rgb8(pix * 3);
    {  // the device's part; what it holds is released before the files are written
        Scene scene;
        if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
        DevBuf<float> color, depth, out32;
        DevBuf<uint8_t> out8;
        if (!color.alloc(pix * 3) || !depth.alloc(pix) || !out32.alloc(pix * 3) || !out8.alloc(pix * 3))
            return fail(err, RTM_ERR_HIP, "no device memory for the depth of field's buffers");
        if (!color.upload(f32_host, pix * 3)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
        const rtm_aov_buffers dev = {depth.get(), nullptr, nullptr, nullptr};
        int rc = rtm_render_aov(st, scene.get(), opt, &dev, nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        rc = rtm_defocus(prm, w, h, opt->device, color.get(), depth.get(), out32.get(), out8.get(), nullptr, nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!frame_back(out8, rgb8.data(), out32, sized(f32_out, pix * 3), pix * 3))
            return fail(err, RTM_ERR_HIP, "copying the defocused frame back failed");
    }
    if (!write_jpg_bmp(stem + "_dof", st, rgb8.data())) return fail(err, RTM_ERR_IO, "cannot write the depth of field files of " + stem);
    return RTM_OK;
}

// --lens (rtm_node.h): rtm_lens of the frame on the default stream, then the two files.
int rtm_node_write_lens(const rtm_settings* st, int device, const rtm_lens_params* prm, const float* f32_host, const std::string& stem,
                        std::string& err, std::vector<float>* f32_out) {
    if (prm->channels != 3) return fail(err, RTM_ERR_INVALID_ARGUMENT, "lens of a frame takes channels = 3");
    const size_t vals = (size_t)st->width * st->height * 3;
    std::vector<uint8_t> rgb8(vals);
    {  // the device's part; what it holds is released before the files are written
        if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
        DevBuf<float> color, out32;
        DevBuf<uint8_t> out8;
        if (!color.alloc(vals) || !out32.alloc(vals) || !out8.alloc(vals))
            return fail(err, RTM_ERR_HIP, "no device memory for lens's buffers");
        if (!color.upload(f32_host, vals)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
        const int rc = rtm_lens(prm, st->width, st->height, device, color.get(), out32.get(), out8.get(), nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!frame_back(out8, rgb8.data(), out32, sized(f32_out, vals), vals))
            return fail(err, RTM_ERR_HIP, "copying the lens frame back failed");
    }
    if (!write_jpg_bmp(stem + "_lens", st, rgb8.data())) return fail(err, RTM_ERR_IO, "cannot write the lens files of " + stem);
    return RTM_OK;
}

// --resize (rtm_node.h): rtm_resize of the frame on the default stream, then the two files at the new size.
int rtm_node_write_resized(const rtm_settings* st, int device, const rtm_resize_params* prm, int dst_width, int dst_height,
                           const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* f32_out) {
    const size_t src_vals = (size_t)st->width * st->height * 3, dst_vals = (size_t)dst_width * dst_height * 3;
    rtm_settings dst = *st;  // the size the files are written at
    dst.width = dst_width;
    dst.height = dst_height;
    // known before anything is allocated: a size the library will refuse must not size a host vector first
    const size_t work_bytes = rtm_resize_work_bytes(st->width, st->height, dst_width, dst_height, prm->filter, prm->channels);
    if (prm->channels != 3 || work_bytes == 0 || work_bytes == SIZE_MAX || dst_vals / 3 > 0x7FFFFFFFu)
        return fail(err, RTM_ERR_INVALID_ARGUMENT, "resize's sizes or filter are out of range");
    std::vector<uint8_t> rgb8(dst_vals);
    {  // the device's part; what it holds is released before the files are written
        if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
        DevBuf<float> color, out32;
        DevBuf<uint8_t> out8;
        DevBuf<void> work;  // hipMalloc's alignment is 256 bytes or more, what rtm_resize asks of work_dev
        if (!color.alloc(src_vals) || !out32.alloc(dst_vals) || !out8.alloc(dst_vals) || !work.alloc(work_bytes))
            return fail(err, RTM_ERR_HIP, "no device memory for resize's buffers");
        if (!color.upload(f32_host, src_vals)) return fail(err, RTM_ERR_HIP, "copying the frame to the device failed");
        const int rc = rtm_resize(prm, st->width, st->height, dst_width, dst_height, device, color.get(), work.get(), out32.get(),
                                  out8.get(), nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!frame_back(out8, rgb8.data(), out32, sized(f32_out, dst_vals), dst_vals))
            return fail(err, RTM_ERR_HIP, "copying the resized frame back failed");
    }
    if (!write_jpg_bmp(stem + "_resized", &dst, rgb8.data())) return fail(err, RTM_ERR_IO, "cannot write the resized files of " + stem);
    return RTM_OK;
}

// --focus-pixel (rtm_node.h): the depth plane of the pixel's row alone
int rtm_node_depth_at(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt, int x, int y,
                      float* depth_out, std::string& err) {
    if (x < 0 || x >= st->width || y < 0 || y >= st->height)
        return fail(err, RTM_ERR_INVALID_ARGUMENT, "the pixel is outside the frame");
    Scene scene;
    if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
    DevBuf<float> depth;
    if (!depth.alloc((size_t)st->width)) return fail(err, RTM_ERR_HIP, "no device memory for a row of the depth plane");
    rtm_options row = *opt;
    row.row_begin = y;
    row.row_end = y + 1;
    const rtm_aov_buffers dev = {depth.get(), nullptr, nullptr, nullptr};
    const int rc = rtm_render_aov(st, scene.get(), &row, &dev, nullptr);
    if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
    std::vector<float> host((size_t)st->width);
    if (!depth.download(host.data(), host.size())) return fail(err, RTM_ERR_HIP, "copying the depth row back failed");
    *depth_out = host[(size_t)x];
    return RTM_OK;
}

namespace {
// --compare and --flip: the two frames up, the work buffer, `call` on the default stream, the record back and, when
// map_out is given, the height x width plane back.  `what` names the stage in the messages.  A work size of SIZE_MAX
// (a frame the stage does not serve) is no device memory, as an allocation of it would be.
template <class Result, class Call>
int frame_pair(const rtm_settings* st, const float* frame_host, const float* reference_host, size_t work_bytes, Result* result,
               std::vector<float>* map_out, const std::string& what, std::string& err, Call call) {
    const size_t pix = (size_t)st->width * st->height;
    DevBuf<float> a, b;
    DevBuf<void> work;  // hipMalloc's alignment is 256 bytes or more, what rtm_compare and rtm_flip ask of work_dev
    DevBuf<Result> result_dev;
    DevBuf<float> map_dev;
    if (work_bytes == SIZE_MAX || !a.alloc(pix * 3) || !b.alloc(pix * 3) || !work.alloc(work_bytes) || !result_dev.alloc(1) ||
        !map_dev.alloc(pix, map_out != nullptr))
        return fail(err, RTM_ERR_HIP, "no device memory for the " + what + "'s buffers");
    if (!a.upload(frame_host, pix * 3) || !b.upload(reference_host, pix * 3))
        return fail(err, RTM_ERR_HIP, "copying the frames to the device failed");
    const int rc = call(a.get(), b.get(), work.get(), result_dev.get(), map_dev.get());
    if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
    if (!result_dev.download(result, 1)) return fail(err, RTM_ERR_HIP, "copying the " + what + "'s record back failed");
    if (map_out && !map_dev.download(sized(map_out, pix), pix)) return fail(err, RTM_ERR_HIP, "copying the " + what + "'s map back failed");
    return RTM_OK;
}
}  // namespace

// --compare (rtm_node.h): rtm_compare of the two frames on the default stream.
int rtm_node_compare(const rtm_settings* st, int device, const float* frame_host, const float* reference_host,
                     rtm_compare_result* result, std::string& err) {
    if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
    const rtm_compare_params prm = RTM_COMPARE_DEFAULTS;
    return frame_pair(st, frame_host, reference_host, rtm_compare_work_bytes(st->width, st->height), result, nullptr, "comparison", err,
                      [&](const float* a, const float* b, void* work, rtm_compare_result* result_dev, float*) {
                          return rtm_compare(&prm, st->width, st->height, device, a, b, work, result_dev, nullptr, nullptr);
                      });
}

// --flip (rtm_node.h): rtm_flip of the two frames on the default stream.
int rtm_node_flip(const rtm_settings* st, int device, const rtm_flip_params* prm, const float* frame_host,
                  const float* reference_host, rtm_flip_result* result, std::vector<float>* map_out, std::string& err) {
    if (const int rc = open_device(device, err); rc != RTM_OK) return rc;
    return frame_pair(st, frame_host, reference_host, rtm_flip_work_bytes(st->width, st->height), result, map_out, "perceptual difference",
                      err, [&](const float* a, const float* b, void* work, rtm_flip_result* result_dev, float* map_dev) {
                          return rtm_flip(prm, st->width, st->height, device, a, b, work, result_dev, map_dev, nullptr);
                      });
}

// --preview (rtm_node.h): the low render, its AOVs and rtm_denoise, the full AOVs, rtm_upsample, all on the default stream,
// then the two files.
int rtm_node_write_preview(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt, int factor,
                           const std::string& stem, std::string& err, std::vector<float>* f32_out, rtm_stats* stats) {
    if (factor < 2 || factor > 8 || st->width % factor != 0 || st->height % factor != 0)
        return fail(err, RTM_ERR_INVALID_ARGUMENT,
                    "--preview " + std::to_string(factor) + ": a factor in 2..8 that divides the width and the height");
    const size_t pix = (size_t)st->width * st->height;
    std::vector<uint8_t> rgb8(pix * 3);
    {  // the device's part; what it holds is released before the files are written
        Scene scene;
        if (const int rc = open_scene(objects, n, opt->device, scene, err); rc != RTM_OK) return rc;
        rtm_settings lo_st = *st;
        lo_st.width = st->width / factor;
        lo_st.height = st->height / factor;
        rtm_options lo_opt = *opt;
        lo_opt.row_begin = 0;
        lo_opt.row_end = lo_st.height;
        const size_t lo_pix = (size_t)lo_st.width * lo_st.height;
        AovPlanes lo_planes, hi_planes;
        DevBuf<float> color, den;
        DevBuf<uint8_t> out8;
        DevBuf<float> out32;
        DevBuf<void> dn_work, up_work;
        if (!lo_planes.alloc(lo_pix, true) || !hi_planes.alloc(pix, true) || !color.alloc(lo_pix * 3) || !den.alloc(lo_pix * 3) ||
            !out8.alloc(pix * 3) || !out32.alloc(pix * 3, f32_out != nullptr) ||
            !dn_work.alloc(rtm_denoise_work_bytes(lo_st.width, lo_st.height)) ||
            !up_work.alloc(rtm_upsample_work_bytes(lo_st.width, lo_st.height)))
            return fail(err, RTM_ERR_HIP, "no device memory for the preview's buffers");
        const rtm_aov_buffers lo = lo_planes.view(), hi = hi_planes.view();
        int rc = rtm_render_scene(&lo_st, scene.get(), &lo_opt, nullptr, color.get(), nullptr, nullptr, stats);
        if (rc == RTM_OK) rc = rtm_render_aov(&lo_st, scene.get(), &lo_opt, &lo, nullptr);
        if (rc == RTM_OK) {
            const rtm_denoise_params prm = RTM_DENOISE_DEFAULTS;
            rc = rtm_denoise(&prm, lo_st.width, lo_st.height, opt->device, color.get(), &lo, dn_work.get(), den.get(), nullptr, nullptr);
        }
        if (rc == RTM_OK) rc = rtm_render_aov(st, scene.get(), opt, &hi, nullptr);
        if (rc == RTM_OK) {
            rtm_upsample_params prm = RTM_UPSAMPLE_DEFAULTS;
            prm.factor = factor;
            rc = rtm_upsample(&prm, lo_st.width, lo_st.height, opt->device, den.get(), &lo, &hi, up_work.get(), out32.get(), out8.get(),
                              nullptr);
        }
        if (rc == RTM_OK) rc = rtm_stream_status(opt->device, nullptr);
        if (rc != RTM_OK) return fail(err, rc, rtm_last_error_detail());
        if (!frame_back(out8, rgb8.data(), out32, sized(f32_out, pix * 3), pix * 3))
            return fail(err, RTM_ERR_HIP, "copying the preview back failed");
    }
    if (!write_jpg_bmp(stem + "_preview", st, rgb8.data())) return fail(err, RTM_ERR_IO, "cannot write the preview files of " + stem);
    return RTM_OK;
}
