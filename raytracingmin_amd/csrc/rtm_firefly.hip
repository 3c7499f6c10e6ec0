// rtm_firefly.hip — rtm_firefly (include/rtm.h): argument checks and the one launch of rtm_firefly_kernel.h.  The call keeps
// no state and needs no work buffer: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rtm_firefly_kernel.h"
#include "rtm_host.h"

namespace rtm {

namespace {
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

using ff_kernel = void (*)(int, int, int, float, float, int, const float*, float*, uint8_t*, uint8_t*, float*);

// the instantiation of a radius and a rank, both checked by the caller
template <int R>
ff_kernel ff_of_rank(int rank) {
    switch (rank) {
        case 1: return firefly_kernel<R, 1>;
        case 2: return firefly_kernel<R, 2>;
        case 3: return firefly_kernel<R, 3>;
        case 4: return firefly_kernel<R, 4>;
        case 5: return firefly_kernel<R, 5>;
        case 6: return firefly_kernel<R, 6>;
        case 7: return firefly_kernel<R, 7>;
        default: return firefly_kernel<R, 8>;
    }
}
ff_kernel ff_pick(int radius, int rank) {
    return radius == 1 ? ff_of_rank<1>(rank) : radius == 2 ? ff_of_rank<2>(rank) : ff_of_rank<3>(rank);
}
}  // namespace

int firefly(const rtm_firefly_params* prm, int32_t width, int32_t height, int device, const float* color, float* out32,
            uint8_t* out8, uint8_t* mask_out, float* thr_out, void* stream_v) {
    if (!prm || !color) return invalid("null params or color_dev");
    if (!out32 && !out8 && !mask_out && !thr_out) return invalid("every output is null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (prm->radius < 1 || prm->radius > kFfMaxRadius) return invalid("radius outside 1..3");
    if (prm->rank < 1 || prm->rank > kFfMaxRank) return invalid("rank outside 1..8");
    if (!std::isfinite(prm->k) || prm->k < 1.0f) return invalid("k is NaN, infinite or below 1");
    if (!std::isfinite(prm->floor) || prm->floor < 0.0f || std::signbit(prm->floor))
        return invalid("floor is NaN, infinite, negative or -0.0");
    if (prm->repair != 0 && prm->repair != 1) return invalid("repair outside {0, 1}");
    if (!aligned4(color) || !aligned4(out32) || !aligned4(thr_out)) return invalid("a float buffer is not 4-byte aligned");
    const void* const outs[4] = {out32, out8, mask_out, thr_out};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i]) continue;
        if (outs[i] == (const void*)color) return invalid("an output aliases color_dev: the gather cannot run in place");
        for (int j = i + 1; j < 4; ++j)
            if (outs[i] == outs[j]) return invalid("two outputs alias each other");
    }
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFu) return unsupported("frame too large for one launch of firefly");
    // one 512-lane block a tile: a frame thinner than a tile has far more lanes than pixels, and a launch holds fewer than 2^32
    const size_t tiles = (size_t)((width + kFfTileX - 1) / kFfTileX) * (size_t)((height + kFfTileY - 1) / kFfTileY);
    if (tiles >= ((size_t)1 << 32) / kFfBlock) return unsupported("frame too large for one launch of firefly: 2^23 tiles or more");
    if (device < 0) return invalid("negative device");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    const unsigned tiles_x = (unsigned)((width + kFfTileX - 1) / kFfTileX);
    const unsigned grid = tiles_x * (unsigned)((height + kFfTileY - 1) / kFfTileY);
    ff_pick(prm->radius, prm->rank)<<<grid, kFfBlock, 0, stream>>>(width, height, (int)tiles_x, prm->k, prm->floor, prm->repair,
                                                                    color, out32, out8, mask_out, thr_out);
    return launched("firefly");
}

}  // namespace rtm
