// rtm_bloom.hip — rtm_bloom / rtm_bloom_work_bytes (include/rtm.h): argument checks, the work buffer's layout and the
// launches of rtm_bloom_kernel.h.  The call keeps no state: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_bloom_kernel.h"
#include "rtm_host.h"

namespace rtm {

namespace {
constexpr size_t kBlAlign = 256;      // work_dev's alignment and that of every level's plane
constexpr size_t kBlPixelBytes = 12;  // the frame: three floats a pixel
constexpr size_t kBlRecord = 16;      // a level's record
constexpr int kBlMaxLevels = 8;

int half_up(int n) { return (n + 1) / 2; }  // a side that has reached 1 stays 1
unsigned tiles_of(int n, int tile) { return (unsigned)((n + tile - 1) / tile); }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
}  // namespace

// the planes of levels 1..L, each rounded up to 256 bytes, in that order
size_t bloom_work_bytes(int32_t width, int32_t height, int32_t levels) {
    if (width <= 0 || height <= 0 || levels < 1 || levels > kBlMaxLevels) return 0;
    if ((size_t)width * (size_t)height > SIZE_MAX / kBlPixelBytes) return SIZE_MAX;
    size_t sum = 0;
    int w = width, h = height;
    for (int l = 1; l <= levels; ++l) {
        w = half_up(w);
        h = half_up(h);
        const size_t records = (size_t)w * (size_t)h;
        if (records > (SIZE_MAX - kBlAlign) / kBlRecord) return SIZE_MAX;
        const size_t plane = (records * kBlRecord + kBlAlign - 1) / kBlAlign * kBlAlign;
        if (plane > SIZE_MAX - sum) return SIZE_MAX;
        sum += plane;
    }
    return sum;
}

int bloom(const rtm_bloom_params* prm, int32_t width, int32_t height, int device, const float* color, void* work, float* out32,
          uint8_t* out8, float* bloom_out, void* stream_v) {
    if (!prm || !color || !work) return invalid("null params, color_dev or work_dev");
    if (!out32 && !out8 && !bloom_out) return invalid("every output is null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (!std::isfinite(prm->threshold) || !std::isfinite(prm->knee) || !std::isfinite(prm->intensity) || !std::isfinite(prm->scatter))
        return invalid("threshold, knee, intensity or scatter is NaN or infinite");
    if (prm->threshold < 0.0f) return invalid("threshold < 0");
    if (prm->knee < 0.0f || prm->knee > 1.0f) return invalid("knee outside [0, 1]");
    if (prm->intensity < 0.0f) return invalid("intensity < 0");
    if (prm->scatter < 0.0f || prm->scatter > 1.0f) return invalid("scatter outside [0, 1]");
    if (prm->levels < 1 || prm->levels > kBlMaxLevels) return invalid("levels outside 1..8");
    if (!aligned4(color) || !aligned4(out32) || !aligned4(bloom_out)) return invalid("a float buffer is not 4-byte aligned");
    if (!aligned256(work)) return invalid("work_dev is not 256-byte aligned");
    if (work == (const void*)color || work == (void*)out32 || work == (void*)out8 || work == (void*)bloom_out)
        return invalid("work_dev aliases another buffer");
    if (bloom_out && ((const void*)bloom_out == (const void*)color || bloom_out == out32))
        return invalid("bloom_out_dev aliases color_dev or out_f32_dev");
    if (out8 && (const void*)out8 == (const void*)color) return invalid("out_u8_dev aliases color_dev");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFu) return unsupported("frame too large for one launch of bloom");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    const int L = prm->levels;
    int w[kBlMaxLevels + 1], h[kBlMaxLevels + 1];
    float4* plane[kBlMaxLevels + 1];
    w[0] = width;
    h[0] = height;
    plane[0] = nullptr;
    size_t at = 0;
    for (int l = 1; l <= L; ++l) {
        w[l] = half_up(w[l - 1]);
        h[l] = half_up(h[l - 1]);
        plane[l] = (float4*)((char*)work + at);
        at += ((size_t)w[l] * (size_t)h[l] * kBlRecord + kBlAlign - 1) / kBlAlign * kBlAlign;
    }
    const auto down_grid = [&](int l, unsigned& tiles_x) {
        tiles_x = tiles_of(w[l], kBlTileX);
        return tiles_x * tiles_of(h[l], kBlTileY);
    };
    const auto pixel_grid = [&](int l, unsigned& tiles_x) {
        tiles_x = tiles_of(w[l], kBlPixTileX);
        return tiles_x * tiles_of(h[l], kBlPixTileY);
    };
    unsigned tx = 0, grid = down_grid(1, tx);
    const float knee_t = prm->knee * prm->threshold;
    if (((uintptr_t)color & 15) == 0)
        bloom_bright_down_kernel<true><<<grid, kBlBlock, 0, stream>>>(width, height, w[1], h[1], (int)tx, color, prm->threshold, knee_t, plane[1]);
    else
        bloom_bright_down_kernel<false><<<grid, kBlBlock, 0, stream>>>(width, height, w[1], h[1], (int)tx, color, prm->threshold, knee_t, plane[1]);
    for (int l = 2; l <= L; ++l) {
        grid = down_grid(l, tx);
        bloom_down_kernel<<<grid, kBlBlock, 0, stream>>>(w[l - 1], h[l - 1], w[l], h[l], (int)tx, plane[l - 1], plane[l]);
    }
    for (int l = L - 1; l >= 1; --l) {
        grid = pixel_grid(l, tx);
        bloom_up_kernel<<<grid, kBlPixTileX * kBlPixTileY, 0, stream>>>(w[l], h[l], w[l + 1], h[l + 1], (int)tx, plane[l + 1], prm->scatter, plane[l]);
    }
    grid = pixel_grid(0, tx);
    bloom_combine_kernel<<<grid, kBlPixTileX * kBlPixTileY, 0, stream>>>(width, height, w[1], h[1], (int)tx, color, plane[1], prm->intensity, out32, out8, bloom_out);
    return launched("bloom");
}

}  // namespace rtm
