// rtm_lens.hip — rtm_lens / rtm_lens_fit_zoom (include/rtm.h): argument checks, the fold-over check, the host's search for
// the zoom that hides the border, and the one launch of rtm_lens_kernel.h.  The call keeps no state and needs no work
// buffer: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "rtm_host.h"
#include "rtm_lens_kernel.h"

namespace rtm {

namespace {
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
bool within(float v, float lo, float hi) { return v >= lo && v <= hi; }  // false for a NaN

// rtm.h's fold-over check of the radial map at zoom `zoom`, in double
bool folds_over(const rtm_lens_params& p, float zoom) {
    const double k1 = (double)p.k1, k2 = (double)p.k2, iz = 1.0 / (double)zoom;
    const double a = 3.0 * k1, b = 5.0 * k2;
    const double T = p.mode == RTM_LENS_INVERSE ? 4.0 * (iz * iz) : iz * iz;
    if (!(1.0 + T * (a + T * b) >= 0.25)) return true;
    if (b != 0.0) {
        const double tv = -a / (2.0 * b);
        if (tv > 0.0 && tv < T && !(1.0 + tv * (a + tv * b) >= 0.25)) return true;
    }
    return p.mode == RTM_LENS_INVERSE && !(1.0 + T * (k1 + T * k2) >= 0.5);
}

// what both entry points refuse of the parameters, but for zoom and the fold-over check: the refusal's text, or null
const char* bad_params(const rtm_lens_params& p) {
    if (!within(p.k1, -0.5f, 0.5f)) return "k1 is NaN or outside [-0.5, 0.5]";
    if (!within(p.k2, -0.25f, 0.25f)) return "k2 is NaN or outside [-0.25, 0.25]";
    if (!within(p.chroma, -0.05f, 0.05f)) return "chroma is NaN or outside [-0.05, 0.05]";
    if (!within(p.vignette, 0.0f, 1.0f)) return "vignette is NaN or outside [0, 1]";
    if (!within(p.falloff, 0.0f, 4.0f)) return "falloff is NaN or outside [0, 4]";
    if (p.mode != RTM_LENS_DIRECT && p.mode != RTM_LENS_INVERSE) return "mode outside 0..1";
    if (p.filter < RTM_LENS_NEAREST || p.filter > RTM_LENS_BICUBIC) return "filter outside 0..2";
    if (p.channels != 1 && p.channels != 3) return "channels is not 1 or 3";
    if (p.filter != RTM_LENS_NEAREST && !(std::isfinite(p.border[0]) && std::isfinite(p.border[1]) && std::isfinite(p.border[2])))
        return "border is not finite (only the NEAREST filter, which copies words, takes such a border)";
    if (p.chroma != 0.0f && p.channels == 1) return "chroma is not 0 with channels = 1: a plane has no colours to separate";
    if (p.filter == RTM_LENS_NEAREST && (p.chroma != 0.0f || p.vignette != 0.0f))
        return "the NEAREST filter copies words: chroma and vignette must be 0";
    return nullptr;
}

// P(z) of rtm.h: no fold-over at zoom z, and every channel of every pixel of the outermost rows and columns inside
bool hides_border(const rtm_lens_params& p, float z, int32_t w, int32_t h) {
    if (folds_over(p, z)) return false;
    const LnMap m = ln_map(p, z, w, h);
    const int nc = p.chroma != 0.0f ? 3 : 1;  // chroma = 0: every channel has the one position
    const auto pixel = [&](int X, int Y) {
        const double dx = ((double)X + 0.5) - m.cx, dy = ((double)Y + 0.5) - m.cy;
        const double F = ln_factor(m, dx, dy);
        for (int c = 0; c < nc; ++c) {
            double u, v;
            if (!ln_position(m, dx, dy, nc == 3 ? F * ln_channel_scale(m, c) : F, w, h, u, v)) return false;
        }
        return true;
    };
    for (int X = 0; X < w; ++X)
        if (!pixel(X, 0) || !pixel(X, h - 1)) return false;
    for (int Y = 0; Y < h; ++Y)
        if (!pixel(0, Y) || !pixel(w - 1, Y)) return false;
    return true;
}

template <int FILTER, int C, bool CHROMA>
void ln_launch(unsigned grid, hipStream_t stream, const LnArgs& a, const float* src, float* out32, uint8_t* out8) {
    lens_kernel<FILTER, C, CHROMA><<<grid, kLnBlock, 0, stream>>>(a, src, out32, out8);
}
}  // namespace

int lens_fit_zoom(const rtm_lens_params* prm, int32_t width, int32_t height, float* zoom_out) {
    if (!prm || !zoom_out) return invalid("null params or zoom_out");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size (width, height)");
    // only what the positions read, and no ranges: a lens that rtm_lens refuses at every zoom has no fit (unsupported, below)
    if (!(std::isfinite(prm->k1) && std::isfinite(prm->k2) && std::isfinite(prm->chroma))) return invalid("k1, k2 or chroma is NaN or infinite");
    if (prm->mode != RTM_LENS_DIRECT && prm->mode != RTM_LENS_INVERSE) return invalid("mode outside 0..1");
    if (prm->channels != 1 && prm->channels != 3) return invalid("channels is not 1 or 3");
    if (prm->chroma != 0.0f && prm->channels == 1) return invalid("chroma is not 0 with channels = 1: a plane has no colours to separate");
    if ((uint64_t)width * (uint64_t)height >= ((uint64_t)1 << 31)) return unsupported("frame too large for lens: 2^31 pixels or more");
    float lo = 0.25f, hi = 4.0f;
    if (hides_border(*prm, lo, width, height)) {
        *zoom_out = lo;
        return RTM_OK;
    }
    if (!hides_border(*prm, hi, width, height)) return unsupported("no zoom in [0.25, 4] hides the border of this lens");
    for (int i = 0; i < 24; ++i) {
        const float mid = (lo + hi) * 0.5f;
        if (hides_border(*prm, mid, width, height))
            hi = mid;
        else
            lo = mid;
    }
    *zoom_out = hi;
    return RTM_OK;
}

int lens(const rtm_lens_params* prm, int32_t width, int32_t height, int device, const float* src, float* out32, uint8_t* out8,
         void* stream_v) {
    if (!prm || !src) return invalid("null params or src_dev");
    if (!out32 && !out8) return invalid("every output is null: out_f32_dev and out_u8_dev");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size (width, height)");
    if (const char* why = bad_params(*prm)) return invalid(why);
    if (!within(prm->zoom, 0.25f, 4.0f)) return invalid("zoom is NaN or outside [0.25, 4]");
    if (folds_over(*prm, prm->zoom))
        return invalid("the radial map folds over: with these k1, k2 and zoom its derivative falls under 0.25 inside the frame");
    if (!aligned4(src) || !aligned4(out32)) return invalid("a float buffer (src_dev, out_f32_dev) is not 4-byte aligned");
    if ((out32 && (const void*)out32 == (const void*)src) || (out8 && (const void*)out8 == (const void*)src))
        return invalid("out_f32_dev or out_u8_dev aliases src_dev: the gather cannot run in place");
    if ((uint64_t)width * (uint64_t)height >= ((uint64_t)1 << 31)) return unsupported("frame too large for lens: 2^31 pixels or more");
    // one 256-lane block a tile: a frame thinner than a tile has far more lanes than pixels, and a launch holds fewer than 2^32
    const size_t tiles_x = ((size_t)width + kLnTileX - 1) / kLnTileX;
    const size_t tiles = tiles_x * (((size_t)height + kLnTileY - 1) / kLnTileY);
    if (tiles >= ((size_t)1 << 32) / kLnBlock) return unsupported("frame too large for one launch of lens: 2^24 tiles or more");
    if (device < 0) return invalid("negative device");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    LnArgs a;
    a.map = ln_map(*prm, prm->zoom, width, height);
    a.w = width;
    a.h = height;
    a.tiles_x = (int)tiles_x;
    a.vignette = prm->vignette;
    a.falloff2 = prm->falloff * prm->falloff;
    std::memcpy(a.border, prm->border, sizeof a.border);
    const unsigned grid = (unsigned)tiles;
    const bool chroma = prm->chroma != 0.0f;  // (then channels = 3 and the filter weighs: checked above)
    if (prm->filter == RTM_LENS_NEAREST) {
        if (prm->channels == 3) ln_launch<RTM_LENS_NEAREST, 3, false>(grid, stream, a, src, out32, out8);
        else ln_launch<RTM_LENS_NEAREST, 1, false>(grid, stream, a, src, out32, out8);
    } else if (prm->filter == RTM_LENS_BILINEAR) {
        if (chroma) ln_launch<RTM_LENS_BILINEAR, 3, true>(grid, stream, a, src, out32, out8);
        else if (prm->channels == 3) ln_launch<RTM_LENS_BILINEAR, 3, false>(grid, stream, a, src, out32, out8);
        else ln_launch<RTM_LENS_BILINEAR, 1, false>(grid, stream, a, src, out32, out8);
    } else {
        if (chroma) ln_launch<RTM_LENS_BICUBIC, 3, true>(grid, stream, a, src, out32, out8);
        else if (prm->channels == 3) ln_launch<RTM_LENS_BICUBIC, 3, false>(grid, stream, a, src, out32, out8);
        else ln_launch<RTM_LENS_BICUBIC, 1, false>(grid, stream, a, src, out32, out8);
    }
    return launched("lens");
}

}  // namespace rtm
