// rtm_flip.hip — rtm_flip / rtm_flip_work_bytes (include/rtm.h): argument checks, the filter tables and colour constants
// (computed here in double, on the host), the work buffer's layout and the launches of rtm_flip_kernel.h.  The call keeps no
// state: it only enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "rtm_host.h"
#include "rtm_flip_kernel.h"

namespace rtm {

namespace {
constexpr size_t kFlipAlign = 256;  // work_dev's alignment and the granule of its parts
constexpr double kPi = 3.14159265358979323846;

size_t round_up(size_t v) { return (v + kFlipAlign - 1) / kFlipAlign * kFlipAlign; }
size_t flip_tiles_x(int32_t width) { return ((size_t)width + kFlipTileW - 1) / kFlipTileW; }
size_t flip_tiles(int32_t width, int32_t height) { return flip_tiles_x(width) * (((size_t)height + kFlipTileH - 1) / kFlipTileH); }
constexpr size_t kPlaneBytesPerPixel = 2 * kFlipPlanes * sizeof(double);  // 112

int csf_radius(double ppd) { return (int)std::ceil(3.0 * std::sqrt(0.04 / (2.0 * kPi * kPi)) * ppd); }
int feature_radius(double ppd) { return (int)std::ceil(3.0 * (0.5 * 0.082 * ppd)); }

// e_b(k), k = -r..r, into out[k + r]; returns the sum
double csf_gauss(double b, double ppd, int r, double* out) {
    double s = 0.0;
    for (int k = -r; k <= r; ++k) {
        const double u = (double)k / ppd;
        out[k + r] = std::exp(-(kPi * kPi) * (u * u) / b);
        s += out[k + r];
    }
    return s;
}

void hunt_lab(const FlipArgs& a, const double rgb[3], double out[3]) {
    double f[3];
    for (int i = 0; i < 3; ++i) {
        const double t = ((a.m[i][0] * rgb[0] + a.m[i][1] * rgb[1]) + a.m[i][2] * rgb[2]) / a.white[i];
        f[i] = t > (6.0 / 29.0) * (6.0 / 29.0) * (6.0 / 29.0) ? std::cbrt(t) : t / (3.0 * ((6.0 / 29.0) * (6.0 / 29.0))) + 4.0 / 29.0;
    }
    const double L = 116.0 * f[1] - 16.0;
    out[0] = L;
    out[1] = 0.01 * L * (500.0 * (f[0] - f[1]));
    out[2] = 0.01 * L * (200.0 * (f[1] - f[2]));
}

// everything of FlipArgs that depends on pixels_per_degree and the transfer alone
void flip_constants(double ppd, int transfer, FlipArgs& a) {
    const double num[3][3] = {{10135552.0, 8788810.0, 4435075.0}, {2613072.0, 8788810.0, 887015.0}, {1425312.0, 8788810.0, 70074185.0}};
    const double den[3] = {24577794.0, 12288897.0, 73733382.0};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) a.m[i][j] = num[i][j] / den[i];
        a.white[i] = (a.m[i][0] + a.m[i][1]) + a.m[i][2];
    }
    const double(*m)[3] = a.m;  // the inverse by cofactors
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
            a.m_inv[i][j] = (m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0]) / det;
        }
    const double green[3] = {0.0, 1.0, 0.0}, blue[3] = {0.0, 0.0, 1.0};
    double lg[3], lb[3];
    hunt_lab(a, green, lg);
    hunt_lab(a, blue, lb);
    const double da = lg[1] - lb[1], db = lg[2] - lb[2];
    a.cmax = std::pow(std::fabs(lg[0] - lb[0]) + std::sqrt(da * da + db * db), 0.7);

    const int r = csf_radius(ppd), rf = feature_radius(ppd);
    a.r = r;
    a.rf = rf;
    a.srgb = transfer == RTM_TRANSFER_SRGB;
    const double sy = csf_gauss(0.0047, ppd, r, a.csf_y), sx = csf_gauss(0.0053, ppd, r, a.csf_cx);
    const double s1 = csf_gauss(0.04, ppd, r, a.csf_cz1), s2 = csf_gauss(0.025, ppd, r, a.csf_cz2);
    const double a1 = 34.1 * std::sqrt(kPi / 0.04), a2 = 13.5 * std::sqrt(kPi / 0.025);
    const double s = a1 * (s1 * s1) + a2 * (s2 * s2);  // the sum of the 2-D Cz filter over its grid
    const double c1 = std::sqrt(a1 / s), c2 = std::sqrt(a2 / s);
    for (int i = 0; i <= 2 * r; ++i) {
        a.csf_y[i] /= sy;
        a.csf_cx[i] /= sx;
        a.csf_cz1[i] *= c1;
        a.csf_cz2[i] *= c2;
    }
    const double sigma = 0.5 * 0.082 * ppd;
    double sg = 0.0, d_pos = 0.0, p_pos = 0.0, p_neg = 0.0;
    for (int k = -rf; k <= rf; ++k) {
        const double g = std::exp(-(double)(k * k) / (2.0 * sigma * sigma));
        const double d = -(double)k * g, p = ((double)(k * k) / (sigma * sigma) - 1.0) * g;
        a.feat_g[k + rf] = g;
        a.feat_d[k + rf] = d;
        a.feat_p[k + rf] = p;
        sg += g;
        if (d > 0.0) d_pos += d;
        if (p > 0.0) p_pos += p;
        if (p < 0.0) p_neg -= p;
    }
    for (int i = 0; i <= 2 * rf; ++i) {
        a.feat_g[i] /= sg;
        a.feat_d[i] /= d_pos;  // d is odd: the negative weights sum to -d_pos
        a.feat_p[i] = a.feat_p[i] > 0.0 ? a.feat_p[i] / p_pos : a.feat_p[i] / p_neg;
    }
}
}  // namespace

static_assert(sizeof(FlipPartial) == 32, "one 32-byte partial per tile");
static_assert(sizeof(rtm_flip_params) == 16 && sizeof(rtm_flip_result) == 1072, "include/rtm.h states these sizes");
static_assert(sizeof(FlipArgs) <= 4096, "the arguments travel by value");

// [0, round256(112 pixels)) the fourteen planes, then round256(32 tiles) of partials, then the histogram's 1024 bytes
size_t flip_work_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > (SIZE_MAX - 4 * kFlipAlign - kFlipBins * sizeof(uint32_t)) / (kPlaneBytesPerPixel + sizeof(FlipPartial))) return SIZE_MAX;
    return round_up(pix * kPlaneBytesPerPixel) + round_up(flip_tiles(width, height) * sizeof(FlipPartial)) +
           kFlipBins * sizeof(uint32_t);
}

int flip(const rtm_flip_params* prm, int32_t width, int32_t height, int device, const float* a, const float* b, void* work,
         rtm_flip_result* result_out, float* map_out, void* stream_v) {
    if (!prm || !a || !b || !work) return invalid("null params, a_dev, b_dev or work_dev");
    if (!result_out && !map_out) return invalid("both outputs are null");
    if (width <= 0 || height <= 0) return invalid("non-positive frame size");
    if (prm->transfer != RTM_TRANSFER_LINEAR && prm->transfer != RTM_TRANSFER_SRGB) return invalid("transfer is not an RTM_TRANSFER_* value");
    if (!std::isfinite(prm->pixels_per_degree) || prm->pixels_per_degree < 8.0 || prm->pixels_per_degree > 128.0)
        return invalid("pixels_per_degree is NaN, infinite or outside [8, 128]");
    if (((uintptr_t)a & 3) != 0 || ((uintptr_t)b & 3) != 0) return invalid("a frame pointer is not aligned to its element");
    if (!aligned256(work)) return invalid("work_dev is not 256-byte aligned");
    if (((uintptr_t)result_out & 7) != 0 || ((uintptr_t)map_out & 3) != 0) return invalid("an output pointer is not aligned to its element");
    if (work == (const void*)a || work == (const void*)b || (const void*)result_out == (const void*)a ||
        (const void*)result_out == (const void*)b || (map_out && (map_out == a || map_out == b)))
        return invalid("work_dev or an output aliases a_dev or b_dev");
    if (map_out && ((void*)map_out == work || (void*)map_out == (void*)result_out))
        return invalid("map_out_dev aliases work_dev or result_out_dev");
    if ((void*)result_out == work) return invalid("result_out_dev aliases work_dev");
    if (device < 0) return invalid("negative device");
    const size_t pix = (size_t)width * (size_t)height;
    if (pix > 0x7FFFFFFFu || flip_work_bytes(width, height) == SIZE_MAX)  // the partials index pixels in 32 bits
        return unsupported("frame too large for one launch of the perceptual difference");
    if (const int rc = use_device(device); rc != RTM_OK) return rc;
    const hipStream_t stream = (hipStream_t)stream_v;
    FlipArgs args;
    flip_constants(prm->pixels_per_degree, prm->transfer, args);
    args.width = width;
    args.height = height;
    args.tiles_x = (int32_t)flip_tiles_x(width);
    const size_t tiles = flip_tiles(width, height);
    double* planes = (double*)work;
    FlipPartial* partials = (FlipPartial*)((char*)work + round_up(pix * kPlaneBytesPerPixel));
    uint32_t* hist = (uint32_t*)((char*)partials + round_up(tiles * sizeof(FlipPartial)));
    const size_t strips = ((size_t)width + kFlipStrip - 1) / kFlipStrip;
    flip_rows_kernel<<<(unsigned)(strips * (size_t)height), kFlipBlock, 0, stream>>>(args, a, b, planes, result_out ? hist : nullptr);
    if (result_out && map_out)
        flip_cols_kernel<true, true><<<(unsigned)tiles, kFlipBlock, 0, stream>>>(args, a, b, planes, partials, hist, map_out);
    else if (result_out)
        flip_cols_kernel<true, false><<<(unsigned)tiles, kFlipBlock, 0, stream>>>(args, a, b, planes, partials, hist, nullptr);
    else
        flip_cols_kernel<false, true><<<(unsigned)tiles, kFlipBlock, 0, stream>>>(args, a, b, planes, nullptr, nullptr, map_out);
    if (result_out) flip_final_kernel<<<1, kFlipBlock, 0, stream>>>(args, partials, (uint32_t)tiles, hist, result_out);
    return launched("flip");
}

}  // namespace rtm
