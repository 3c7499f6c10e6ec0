// rtm_scope.hip — the frame scopes (include/rtm.h): rtm_scopes' and rtm_scope_draw's argument checks and launches
// (rtm_scope_kernel.h), and the host-only readers of a histogram: bin ranges, percentiles, the exposure suggestion.  The
// device calls keep no state and need no work buffer: they zero their own outputs and only enqueue on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rtm_host.h"
#include "rtm_scope_kernel.h"

namespace rtm {

namespace {
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// step 4's bin of a value in [0, 1]
int code_bin(float v) { return (int)(255.0 * (double)v); }

// the smallest float whose CODE bin is `bin` (1..255): bin / 255 rounded to float, then stepped onto the edge
float code_lower_edge(int bin) {
    float lo = (float)((double)bin / 255.0);
    while (code_bin(lo) < bin) lo = std::nextafterf(lo, 2.0f);
    while (code_bin(std::nextafterf(lo, 0.0f)) >= bin) lo = std::nextafterf(lo, 0.0f);
    return lo;
}

void bin_range(int mode, int bin, float* lo, float* hi) {
    if (mode == RTM_SCOPE_LOG2) {
        const auto edge = [](int b) { return std::ldexp(1.0f + (float)(b & 7) / 8.0f, (b >> 3) - 16); };
        *lo = edge(bin);
        *hi = edge(bin + 1);  // (bin 256 is 2^16)
    } else {
        *lo = bin == 0 ? 0.0f : code_lower_edge(bin);
        *hi = bin == 255 ? 1.0f : code_lower_edge(bin + 1);
    }
}
}  // namespace

int scope_bin_range(int32_t mode, int32_t bin, float* lo, float* hi) {
    if (!lo || !hi) return invalid("null lo or hi");
    if (mode != RTM_SCOPE_LOG2 && mode != RTM_SCOPE_CODE) return invalid("mode out of range");
    if (bin < 0 || bin > 255) return invalid("bin outside 0..255");
    bin_range(mode, bin, lo, hi);
    return RTM_OK;
}

int scope_percentile(const rtm_scope_histogram* h, int32_t mode, int32_t channel, double percent, float* value_out,
                     int32_t* bin_out) {
    if (!h || (!value_out && !bin_out)) return invalid("null histogram, or both outputs null");
    if (mode != RTM_SCOPE_LOG2 && mode != RTM_SCOPE_CODE) return invalid("mode out of range");
    if (channel < 0 || channel > 3) return invalid("channel outside 0..3");
    if (!(percent >= 0.0 && percent <= 100.0)) return invalid("percent is NaN or outside [0, 100]");
    float value = 1.0f;
    int32_t bin = -2;
    if (h->pixels != 0) {
        const double t = percent / 100.0 * (double)h->pixels;
        double cum = (double)h->below[channel];
        if (t <= cum) {
            value = 0.0f;
            bin = -1;
        } else {
            value = mode == RTM_SCOPE_LOG2 ? 65536.0f : 1.0f;
            bin = 256;
            for (int b = 0; b < 256; ++b) {
                const double n = (double)h->bins[channel][b];
                if (n > 0.0 && cum + n >= t) {
                    float lo, hi;
                    bin_range(mode, b, &lo, &hi);
                    value = (float)((double)lo + (t - cum) / n * ((double)hi - (double)lo));
                    bin = b;
                    break;
                }
                cum += n;
            }
        }
    }
    if (value_out) *value_out = value;
    if (bin_out) *bin_out = bin;
    return RTM_OK;
}

int scope_exposure(const rtm_scope_histogram* h, double percent, double target, float* ev_out) {
    if (!h || !ev_out) return invalid("null histogram or ev_out");
    if (!(percent >= 0.0 && percent <= 100.0)) return invalid("percent is NaN or outside [0, 100]");
    if (!(std::isfinite(target) && target > 0.0)) return invalid("target is not positive and finite");
    float value = 0.0f;
    if (const int rc = scope_percentile(h, RTM_SCOPE_LOG2, 0, percent, &value, nullptr); rc != RTM_OK) return rc;
    double ev = 0.0;
    if (value > 0.0f) {
        ev = std::log2(target / (double)value);
        ev = ev < -32.0 ? -32.0 : ev > 32.0 ? 32.0 : ev;
    }
    *ev_out = (float)ev;
    return RTM_OK;
}

int scopes(const rtm_scope_params* prm, int32_t width, int32_t height, int device, const float* color,
           rtm_scope_histogram* hist_out, uint32_t* wave_out, void* stream_v) {
    if (!prm || !color) return invalid("null params or color_dev");
    if (!hist_out && !wave_out) return invalid("both outputs are null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (prm->mode != RTM_SCOPE_LOG2 && prm->mode != RTM_SCOPE_CODE) return invalid("mode out of range");
    if (wave_out && (prm->columns < 1 || prm->columns > width)) return invalid("columns outside 1..width");
    if (!aligned4(color) || !aligned4(hist_out) || !aligned4(wave_out)) return invalid("a buffer is not 4-byte aligned");
    if ((const void*)hist_out == (const void*)color || (const void*)wave_out == (const void*)color)
        return invalid("an output aliases color_dev");
    if (hist_out && (const void*)hist_out == (const void*)wave_out) return invalid("the two outputs alias each other");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFu) return unsupported("frame too large for scopes: 2^31 pixels or more");
    if (device < 0) return invalid("negative device");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    uint32_t* const hist = (uint32_t*)hist_out;
    if (hist) RTM_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(rtm_scope_histogram), stream));
    if (!wave_out) {
        // a grid stride over at most kScHistGrid blocks: each ends with one global add per slot it used, and the adds of all
        // blocks to one word are served one after the other
        const size_t blocks = (pix + kScHistBlock - 1) / kScHistBlock;
        const unsigned grid = (unsigned)(blocks < (size_t)kScHistGrid ? blocks : (size_t)kScHistGrid);
        scope_hist_kernel<<<grid, kScHistBlock, 0, stream>>>((uint32_t)pix, prm->mode, color, hist);
        return launched("scopes");
    }
    const int columns = prm->columns;
    RTM_HIP_CHECK(hipMemsetAsync(wave_out, 0, (size_t)4 * 256 * (size_t)columns * sizeof(uint32_t), stream));
    // strips of output columns across, bands of rows down: about 1024 blocks, none with fewer than 4096 pixels where the
    // frame allows (a block zeroes and folds 8192 words of LDS whatever it counted)
    const size_t strips = ((size_t)columns + kScStrip - 1) / kScStrip;
    size_t bands = (1024 + strips - 1) / strips;
    const size_t by_pixels = pix / strips / 4096;
    if (bands > by_pixels) bands = by_pixels;
    if (bands > (size_t)height) bands = (size_t)height;
    if (bands > 65535) bands = 65535;
    if (bands < 1) bands = 1;
    const int band = (int)(((size_t)height + bands - 1) / bands);
    const dim3 grid((unsigned)strips, (unsigned)((height + band - 1) / band));
    if (hist)
        scope_wave_kernel<true><<<grid, kScBlock, 0, stream>>>(width, height, columns, prm->mode, band, color, hist, wave_out);
    else
        scope_wave_kernel<false><<<grid, kScBlock, 0, stream>>>(width, height, columns, prm->mode, band, color, nullptr, wave_out);
    return launched("scopes");
}

int scope_draw(int32_t columns, int32_t layout, uint32_t gain, int device, const uint32_t* wave, uint8_t* out, void* stream_v) {
    if (!wave || !out) return invalid("null waveform_dev or out_u8_dev");
    if (columns < 1) return invalid("columns below 1");
    if (layout != RTM_SCOPE_LUMA && layout != RTM_SCOPE_OVERLAY && layout != RTM_SCOPE_PARADE) return invalid("layout out of range");
    if (gain == 0) return invalid("gain is 0");
    if (!aligned4(wave)) return invalid("waveform_dev is not 4-byte aligned");
    if ((const void*)wave == (const void*)out) return invalid("out_u8_dev aliases waveform_dev");
    if (columns >= (1 << 21)) return unsupported("too many columns for one launch of scope_draw: 2^21 or more");
    if (device < 0) return invalid("negative device");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const uint32_t out_w = (uint32_t)columns * (layout == RTM_SCOPE_PARADE ? 3u : 1u);
    const unsigned grid = (256u * out_w + kScBlock - 1) / kScBlock;
    scope_draw_kernel<<<grid, kScBlock, 0, (hipStream_t)stream_v>>>((uint32_t)columns, out_w, layout, gain, wave, out);
    return launched("scope_draw");
}

}  // namespace rtm
