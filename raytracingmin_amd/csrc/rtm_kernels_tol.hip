// rtm_kernels_tol.hip — the fp64 TOLERANCE row (rtm_options.variant 18), a separately labelled variant of the hot kernel.
//
// north_star's bar for the image is a per-pixel delta of 1e-4 against the CPU renderer; the default kernels meet it with 0
// (bit equality) by keeping every IEEE operation of the reference: no FMA contraction (the reference's x86-64 build has
// none) and correctly rounded division / square-root sequences.  This translation unit compiles THE SAME kernel source
// (rtm_device.h, rtm_path.h, rtm_render_kernel.h: same loop nest, same counter RNG and Russian-roulette thresholds, the
// float islands of src/Ray.h:67-72, src/SettingData.h:14-16 and src/SettingData.cpp:200,208, the same order of the
// additions into Renderer::image) a second time, into namespace rtm_tol, with
//   * FMA contraction allowed (-ffp-contract=fast-honor-pragmas), and
//   * division and square root to about one ulp (RTM_TOL: rtm_path.h, seq_rcp / seq_quot / seq_sqrt), sin / cos as the
//     device evaluates them (within one ulp of the host libm's; RTM_MODE_HOST_TRIG has no effect on this row);
//   * the fold L = colorKD * L + emission (src/Renderer.cpp:109) kept unfused (rtm_device.h: fold_step), so that a
//     sample's value stays a function of its path's hit ids alone: the image differs from the exact kernel's only where
//     a last-bit difference in a distance or a direction changes WHICH sphere a ray hits.
// What is instantiated: the default kernels of scenes up to 24 spheres — with a depth cap of at most 8 the LDS tables, chunked
// search, packed records, deferred fold and in-wave sample stealing (kTolCapped: kLdsTab | kPark | kPack8 | kDefer | kSteal);
// for any other depth (the reference's own unlimited recursion) the same with records packed by position and the pooled
// stack, no stealing (kTolAny: kPackL in place of kPack8 | kSteal); each with and without the sample split of a launch's
// last tiles (kSplit) — the class of every BASELINE Cornell configuration.  Never what rtm_options.variant 0 chooses: a caller
// asks for it by number.  bench.py's headline figure IS this row (bench.py --exact: the bit-exact kernel), labelled as such,
// with its own roofline fraction and the count of pixels that differ from the exact frame (tests/test_tolerance_gpu.py).
#define RTM_NS rtm_tol
#define RTM_TOL 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rtm_internal.h"
#include "rtm_render_kernel.h"

namespace rtm_tol {

// The axis-signature instantiations of this unit take the search's roots without their residual step (rtm_path.h:
// seq_sqrt_batch, LIGHT): for compact scenes seen by a camera that is within the same extent — anything else runs the plain
// exact-n kernels with the full roots.
static bool compact_launch(const RenderParams& P) {
    const double cam = std::sqrt(P.cam_org.x * P.cam_org.x + P.cam_org.y * P.cam_org.y + P.cam_org.z * P.cam_org.z);
    return (P.scene.fold_flags & kSceneCompact) != 0u && cam <= kCompactExtent;
}

// The row's two shapes: a depth cap of at most 8 (kTolCapped: packed records, in-wave stealing) and any other depth (kTolAny:
// records packed by position and the pooled stack from level 16, rtm_render_kernel.h; no stealing, a whole tile stores its
// own pixels); both with the LDS tables and the deferred fold, and kSplit where the launch splits its last tiles
constexpr unsigned kTolCapped = kLdsTab | kPark | kPack8 | kDefer | kSteal;
constexpr unsigned kTolAny = kLdsTab | kPark | kDefer | kPackL;
constexpr int kTolWavesPerSimd = 4;  // launch bound of both (the depth-capped kernel's: profiles/r4/tol_wpe_ab.txt)

// The kernel of shape F for the scene: an axis signature (kTolAny: the shipped Cornell box only) where its roots may skip the
// residual step and the launch holds the near-unit Normalize table (a compile-time fact for them), else with kTolCapped the
// shipped scenes' exact sphere counts, else the generic kernel for n < 8 or any n
template <unsigned F>
static void launch_n(const RenderParams& P, unsigned grid, size_t lds_pad, hipStream_t stream) {
    constexpr int LDS_D = (F & kPackL) != 0 ? 0 : 16;
    unsigned unit_tab;
    render_lds_bytes<F, uint8_t, LDS_D>(P.scene.n, lds_pad, &unit_tab);
    const bool axis = P.mode == RTM_MODE_REPAIRED && unit_tab == 1u && compact_launch(P);  // rtm_path.h: sphere_disc
#define RTM_AXIS_CASE(k, sig)                                                                                    \
    if (P.scene.n == k && P.scene.axis_pat == sig && axis) {                                                     \
        launch_tiles<MathFast, F, axis_unroll(k, sig), uint8_t, LDS_D, kTolWavesPerSimd>(P, grid, lds_pad, stream); \
        return;                                                                                                  \
    }
    if constexpr ((F & kPackL) != 0) {
        RTM_AXIS_CASE(7, kAxisSigCornell7)
    } else {
        RTM_AXIS_SIGNATURES(RTM_AXIS_CASE)
        switch (P.scene.n) {
            case 3: launch_tiles<MathFast, F, -103, uint8_t, LDS_D, kTolWavesPerSimd>(P, grid, lds_pad, stream); return;
            case 5: launch_tiles<MathFast, F, -105, uint8_t, LDS_D, kTolWavesPerSimd>(P, grid, lds_pad, stream); return;
            case 7: launch_tiles<MathFast, F, -107, uint8_t, LDS_D, kTolWavesPerSimd>(P, grid, lds_pad, stream); return;
            default: break;
        }
    }
#undef RTM_AXIS_CASE
    if (P.scene.n < 8) launch_tiles<MathFast, F, -8, uint8_t, LDS_D, kTolWavesPerSimd>(P, grid, lds_pad, stream);
    else launch_tiles<MathFast, F, 8, uint8_t, LDS_D, kTolWavesPerSimd>(P, grid, lds_pad, stream);
}

// A render of shape F: the sample split where the caller planned one, steal_finalize_kernel behind a stealing one
template <unsigned F>
static void launch_row(const RenderParams& P, unsigned grid, size_t lds_pad, hipStream_t stream) {
    if (P.split > 1) {
        launch_n<F | kSplit>(P, P.split_first + P.n_tiles * P.split, lds_pad, stream);
        launch_split_finalize(P, stream);
    } else {
        launch_n<F>(P, grid, lds_pad, stream);
    }
    if constexpr ((F & kSteal) != 0) launch_steal_finalize(P, grid, stream);
}

// rtm_debug_math_probe ops 32..: this translation unit's arithmetic on caller data (tests/test_tolerance_gpu.py measures the
// distance to the correctly rounded results in ulps).  32 the unscaled square root, 33 x / y by reciprocal, 34 the
// reciprocal alone, 35 x * y + 1.0 (contracted here: the other translation unit's op 7 must not be), 36 / 37 sin / cos of the
// branch-free sincos as compiled here, 38 one level of the fold (x * y + 0.25: must NOT be contracted), 39 / 40 sin / cos of
// 2 pi (x 2^-24) by the quadrant-exact sequence the shading block uses (x: a draw's 24-bit integer), 41 the search's light root
__global__ void tol_math_probe_kernel(int op, const double* __restrict__ a, const double* __restrict__ b, size_t n,
                                      double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b ? b[i] : 0.0;
    double r = 0.0, s, c;
    switch (op) {
        case 32: r = seq_sqrt(x); break;
        case 33: r = seq_quot(x, y, seq_rcp(y)); break;
        case 34: r = seq_rcp(x); break;
        case 35: r = x * y + 1.0; break;
        case 36: sincos_small(x, s, c); r = s; break;
        case 37: sincos_small(x, s, c); r = c; break;
        case 38: r = fold_step(d3(x, x, x), d3(y, y, y), d3(0.25, 0.25, 0.25)).y; break;
        case 39: sincos_turn24_k(TrigFromRegs{}, x, s, c); r = s; break;
        case 40: sincos_turn24_k(TrigFromRegs{}, x, s, c); r = c; break;
        case 41: {  // the search's light root (seq_sqrt_batch<K, true>)
            const double in[1] = {x};
            double out1[1];
            seq_sqrt_batch<1, true>(in, out1);
            r = out1[0];
            break;
        }
        default: break;
    }
    out[i] = r;
}

}  // namespace rtm_tol

namespace rtm {

int tol_math_probe(int op, const double* a_dev, const double* b_dev, size_t n, double* out_dev) {
    rtm_tol::tol_math_probe_kernel<<<(unsigned)((n + 255) / 256), 256>>>(op, a_dev, b_dev, n, out_dev);
    return hipGetLastError() == hipSuccess ? RTM_OK : RTM_ERR_HIP;
}

// `params`: the caller's rtm::RenderParams (the same struct, compiled from the same header into the other namespace),
// planned exactly as for the default kernel: split_first / n_tiles / split* for the sample split, steal_ws / steal_rows /
// steal_depth for the whole tiles (steal_ws must be there: the whole tiles' pixels are stored by steal_finalize_kernel).
int launch_tol(const void* params, size_t params_bytes, unsigned grid, size_t lds_pad, void* stream_v) {
    rtm_tol::RenderParams P;
    if (params_bytes != sizeof P) {
        set_last_error("tolerance row: RenderParams layout mismatch between the two translation units");
        return RTM_ERR_INVALID_ARGUMENT;
    }
    std::memcpy(&P, params, sizeof P);
    // RTM_MODE_HOST_TRIG turns the device's sin / cos into the host libm's, one ulp apart on 3 % of the arguments: a
    // distinction this unit's own arithmetic does not keep anywhere else.  The row takes the device's (one table gather and
    // ten instructions per bounce less); the flag is accepted and has no effect here.
    P.scene.trig_fix = nullptr;
    hipStream_t stream = (hipStream_t)stream_v;
    const bool any_depth = P.max_bounces < 0 || P.max_bounces > 8;
    if ((!any_depth && P.steal_ws == nullptr) || P.scene.n < 1 || P.scene.n > 24 || P.scene.plane != nullptr ||
        P.sample_end >= 65536u) {
        set_last_error("variant 18 (fp64 tolerance row) serves all-sphere scenes of 1..24 spheres with fewer than 65 536 samples per pixel");
        return RTM_ERR_UNSUPPORTED;
    }
    if (P.prim_masks == nullptr) {
        set_last_error("tolerance row: no primary-ray mask buffer");
        return RTM_ERR_INVALID_ARGUMENT;
    }
    // tiles of the launch: the whole ones and, behind them, the split ones (each once)
    const unsigned n_tiles_all = P.split > 1 ? P.split_first + P.n_tiles : grid;
    static const bool no_masks = [] {
        const char* e = std::getenv("RTM_DEBUG_TOL_PRIMFIX");  // A/B knob: 0 = no primary ray is flagged (NOT within tolerance on the Cornell diagonals)
        return e && e[0] == '0';
    }();
    if (no_masks) P.prim_dirs = nullptr;
    if (no_masks)
        (void)hipMemsetAsync(const_cast<unsigned long long*>(P.prim_masks), 0, (size_t)n_tiles_all * 64 * sizeof(unsigned long long), stream);
    else
        rtm_tol::prim_prepass_kernel<<<n_tiles_all, 64, 0, stream>>>(P, const_cast<unsigned long long*>(P.prim_masks),
                                                                 const_cast<double*>(P.prim_dirs));
    if (any_depth) rtm_tol::launch_row<rtm_tol::kTolAny>(P, grid, lds_pad, stream);
    else rtm_tol::launch_row<rtm_tol::kTolCapped>(P, grid, lds_pad, stream);
    if (hipGetLastError() != hipSuccess) {
        set_last_error("tolerance row: launch failed");
        return RTM_ERR_HIP;
    }
    return RTM_OK;
}

}  // namespace rtm
