// rtm_resize.hip — rtm_resize / rtm_resize_work_bytes (include/rtm.h): argument checks, the work buffer's layout and the
// three launches of rtm_resize_kernel.h.  The call keeps no state: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtm_host.h"
#include "rtm_resize_kernel.h"

namespace rtm {

namespace {
constexpr size_t kRsAlign = 256;          // work_dev's alignment and that of every part of it
constexpr size_t kRsMaxBlocks = 1 << 20;  // a pass's grid: its blocks stride over the tiles beyond it

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
int twice_radius(int filter) { return filter == RTM_RESIZE_BOX ? 1 : filter == RTM_RESIZE_TRIANGLE ? 2 : filter == RTM_RESIZE_MITCHELL ? 4 : 6; }
// T = ceil(q M / N), M = max(n, N)
uint64_t taps(int q, int32_t n, int32_t N) {
    const uint64_t M = (uint64_t)(n > N ? n : N);
    return ((uint64_t)q * M + (uint64_t)N - 1) / (uint64_t)N;
}
// a * b * c rounded up to 256, or false when it does not fit a size_t
bool part(uint64_t a, uint64_t b, uint64_t c, size_t& bytes) {
    const unsigned __int128 v = (unsigned __int128)a * b * c;  // a, b < 2^31 and c < 2^35: no overflow here
    if (v > (unsigned __int128)(SIZE_MAX - (kRsAlign - 1))) return false;
    bytes = ((size_t)v + kRsAlign - 1) / kRsAlign * kRsAlign;
    return true;
}
struct Layout {
    size_t records, tab_x, tab_y, j0, total;
};
// the records, the two tables, the two j0 arrays, each rounded up to 256 bytes, in that order
bool layout(int32_t w, int32_t h, int32_t W, int32_t H, int32_t filter, int32_t channels, Layout& l) {
    const int q = twice_radius(filter);
    if (!part(channels == 3 ? 16 : 8, (uint64_t)W, (uint64_t)h, l.records)) return false;
    if (!part(4, (uint64_t)W, taps(q, w, W), l.tab_x)) return false;
    if (!part(4, (uint64_t)H, taps(q, h, H), l.tab_y)) return false;
    if (!part(4, (uint64_t)W + (uint64_t)H, 1, l.j0)) return false;
    l.total = l.records;
    for (const size_t p : {l.tab_x, l.tab_y, l.j0}) {
        if (p > SIZE_MAX - l.total) return false;
        l.total += p;
    }
    return true;
}
}  // namespace

size_t resize_work_bytes(int32_t w, int32_t h, int32_t W, int32_t H, int32_t filter, int32_t channels) {
    if (w <= 0 || h <= 0 || W <= 0 || H <= 0 || filter < RTM_RESIZE_BOX || filter > RTM_RESIZE_LANCZOS3 || (channels != 1 && channels != 3))
        return 0;
    Layout l;
    return layout(w, h, W, H, filter, channels, l) ? l.total : SIZE_MAX;
}

int resize(const rtm_resize_params* prm, int32_t w, int32_t h, int32_t W, int32_t H, int device, const float* src, void* work,
           float* out32, uint8_t* out8, void* stream_v) {
    if (!prm || !src || !work) return invalid("null params, src_dev or work_dev");
    if (!out32 && !out8) return invalid("every output is null: out_f32_dev and out_u8_dev");
    if (w <= 0 || h <= 0) return invalid("non-positive source size (src_width, src_height)");
    if (W <= 0 || H <= 0) return invalid("non-positive destination size (dst_width, dst_height)");
    if (prm->filter < RTM_RESIZE_BOX || prm->filter > RTM_RESIZE_LANCZOS3) return invalid("filter outside 0..3");
    if (prm->channels != 1 && prm->channels != 3) return invalid("channels is not 1 or 3");
    if (!aligned4(src) || !aligned4(out32)) return invalid("a float buffer (src_dev, out_f32_dev) is not 4-byte aligned");
    if (!aligned256(work)) return invalid("work_dev is not 256-byte aligned");
    if (work == (const void*)src || work == (void*)out32 || work == (void*)out8) return invalid("work_dev aliases another buffer");
    if ((out32 && (const void*)out32 == (const void*)src) || (out8 && (const void*)out8 == (const void*)src))
        return invalid("out_f32_dev or out_u8_dev aliases src_dev: the gather cannot run in place");
    const uint64_t lim = (uint64_t)1 << 31;
    if ((uint64_t)w * (uint64_t)h >= lim) return unsupported("source frame too large for resize: 2^31 pixels or more");
    if ((uint64_t)W * (uint64_t)H >= lim) return unsupported("destination frame too large for resize: 2^31 pixels or more");
    if ((uint64_t)W * (uint64_t)h >= lim) return unsupported("intermediate frame (dst_width x src_height) too large for resize: 2^31 records or more");
    const int q = twice_radius(prm->filter);
    // the first tap and the tap count are 32-bit: |j0| <= q M / 2 + 1 and T <= q M
    if ((uint64_t)q * (uint64_t)(w > W ? w : W) >= lim || (uint64_t)q * (uint64_t)(h > H ? h : H) >= lim)
        return unsupported("side too large for resize's filter: 2 r max(src, dst) is 2^31 or more on an axis");
    if (device < 0) return invalid("negative device");
    Layout l;
    if (!layout(w, h, W, H, prm->filter, prm->channels, l)) return unsupported("resize's work buffer does not fit a size_t");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    const int Tx = (int)taps(q, w, W), Ty = (int)taps(q, h, H);
    char* const base = (char*)work;
    float* const tab_x = (float*)(base + l.records);
    float* const tab_y = (float*)(base + l.records + l.tab_x);
    int* const j0_x = (int*)(base + l.records + l.tab_x + l.tab_y);
    int* const j0_y = j0_x + W;
    const unsigned table_grid = (unsigned)(((uint64_t)W + (uint64_t)H + kRsTableBlock - 1) / kRsTableBlock);
    resize_tables_kernel<<<table_grid, kRsTableBlock, 0, stream>>>(w, h, W, H, prm->filter, q, Tx, Ty, tab_x, tab_y, j0_x, j0_y);
    const unsigned tiles_x = (unsigned)(((uint64_t)W + kRsTileX - 1) / kRsTileX);
    const size_t h_tiles = (size_t)tiles_x * (((size_t)h + kRsTileY - 1) / kRsTileY);
    const size_t v_tiles = (size_t)tiles_x * (((size_t)H + kRsTileY - 1) / kRsTileY);
    const unsigned h_grid = (unsigned)(h_tiles < kRsMaxBlocks ? h_tiles : kRsMaxBlocks);
    const unsigned v_grid = (unsigned)(v_tiles < kRsMaxBlocks ? v_tiles : kRsMaxBlocks);
    if (prm->channels == 3) {
        resize_horizontal_kernel<3><<<h_grid, kRsBlock, 0, stream>>>(w, h, W, Tx, tiles_x, h_tiles, src, tab_x, j0_x, (float4*)base);
        resize_vertical_kernel<3><<<v_grid, kRsBlock, 0, stream>>>(h, W, H, Ty, tiles_x, v_tiles, (const float4*)base, tab_y, j0_y, out32, out8);
    } else {
        resize_horizontal_kernel<1><<<h_grid, kRsBlock, 0, stream>>>(w, h, W, Tx, tiles_x, h_tiles, src, tab_x, j0_x, (float2*)base);
        resize_vertical_kernel<1><<<v_grid, kRsBlock, 0, stream>>>(h, W, H, Ty, tiles_x, v_tiles, (const float2*)base, tab_y, j0_y, out32, out8);
    }
    return launched("resize");
}

}  // namespace rtm
