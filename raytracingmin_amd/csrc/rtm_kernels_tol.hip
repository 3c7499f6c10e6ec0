// rtm_kernels_tol.hip — the fp64 TOLERANCE row (rtm_options.variant 18), a separately labelled variant of the hot kernel.
//
// north_star's bar for the image is a per-pixel delta of 1e-4 against the CPU renderer; the default kernels meet it with 0
// (bit equality) by keeping every IEEE operation of the reference: no FMA contraction (the reference's x86-64 build has
// none) and correctly rounded division / square-root sequences.  This translation unit compiles THE SAME kernel source
// (rtm_device.h, rtm_path.h, rtm_render_kernel.h: same loop nest, same counter RNG and Russian-roulette thresholds, the
// float islands of src/Ray.h:67-72, src/SettingData.h:14-16 and src/SettingData.cpp:200,208, the same order of the
// additions into Renderer::image) a second time, into namespace rtm_tol, with
//   * FMA contraction allowed (-ffp-contract=fast-honor-pragmas), and
//   * division and square root to about one ulp (RTM_TOL: rtm_path.h, seq_rcp / seq_quot / seq_sqrt; the shading block's two
//     unit-range roots and, in compact scenes, the search's without the residual step: 2^-45), the sine and cosine of a
//     draw's angle 2 pi m 2^-24 from a table of 16 384 points (host long double, rounded once) and two series terms,
//     within 3e-16 of the true values (rtm_device.h: sincos_turn24_tab_load; RTM_MODE_HOST_TRIG has no effect on this row);
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
#include <map>
#include <mutex>
#include <vector>

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
// ... and they take the discriminants of axis spheres in the expanded form (rtm_path.h: sphere_disc), whose rounding error grows
// with (|c| + r)^2 and |o|^2, not with r^2: only for a scene the host has proven inside that form's envelope
// (kSceneAxisReachShift: no sphere can hit itself, distances stay a sixteenth under the smallest threshold) seen by a camera
// within the same reach.  A small sphere far out on an axis fails it; the scene then runs the plain exact-n kernels.
static bool expanded_form_launch(const RenderParams& P) {
    const unsigned e = (P.scene.fold_flags >> kSceneAxisReachShift) & kSceneAxisReachMask;
    const double cam = std::sqrt(P.cam_org.x * P.cam_org.x + P.cam_org.y * P.cam_org.y + P.cam_org.z * P.cam_org.z);
    return e != 0u && cam <= std::ldexp(1.0, (int)e - 128);
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
    render_lds_bytes<F, uint8_t, LDS_D>(P.scene.n, lds_rows_for(-1000), lds_pad, &unit_tab);  // (the axis kernels' layout: `axis` below is what this answer is for)
    const bool axis = P.mode == RTM_MODE_REPAIRED && unit_tab == 1u && compact_launch(P) && expanded_form_launch(P);  // rtm_path.h: sphere_disc
    // (axis_pat holds the signature's low 16 bits, fold_flags' bits 8..15 what goes above them: the spheres that share one K)
    const unsigned shared_k = (P.scene.fold_flags >> kSceneSharedKShift) & kSceneSharedKMask;
    // ... and kSceneWallPairs the bit above those: the group's members are opposite pairs (rtm_path.h: kAxisPairsBit).  Not for
    // the any-depth kernel with the sample split: there the second code path costs 28 bytes of scratch that its twin does not
    // have (-Rpass-analysis=kernel-resource-usage; profiles/r10/wall_pairs.md), so that shape keeps the seven-sphere block.
    constexpr bool kPairsShape = (F & (kPackL | kSplit)) != (kPackL | kSplit);
    const unsigned pairs = kPairsShape && (P.scene.fold_flags & kSceneWallPairs) != 0u ? kAxisPairsBit : 0u;
#define RTM_AXIS_CASE(k, sig)                                                                                    \
    if (P.scene.n == k && P.scene.axis_pat == ((sig) & 0xFFFFu) && ((shared_k << kAxisSharedKShift) | pairs) == ((sig) & ~0xFFFFu) && axis) { \
        launch_tiles<MathFast, F, axis_unroll(k, sig), uint8_t, LDS_D, kTolWavesPerSimd>(P, grid, lds_pad, stream); \
        return;                                                                                                  \
    }
    if constexpr (kPairsShape) {
        RTM_AXIS_CASE(7, kAxisSigCornell7Pairs)  // the shipped box: its six walls share one K and are three opposite pairs
    }
    RTM_AXIS_CASE(7, kAxisSigCornell7Walls)  // ... without being opposite pairs, and the shape left out above
#undef RTM_AXIS_CASE
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
// 2 pi (x 2^-24) by the quadrant-exact sequence the shading block ran until round 7 (x: a draw's 24-bit integer), 41 the search's
// light root, 42 / 43 sin / cos of 2 pi (x 2^-24) as the shading block takes them now — table point and two series terms
// (rtm_device.h: sincos_turn24_tab_load / _apply; `tab`: the device's table) —, 44 the shading block's unit-range root
// (MathSpecT::sqrt64_unit: the light sequence), 45 the light root with its half by a multiply (the form op 41 ran until round 8:
// its reference), 46 / 47 ops 42 / 43 with the angle split made in doubles (until round 8: their reference), 48 op 32 with its
// half by a multiply (the full root's reference), 49 / 50 / 51 the normal table's row for a sphere with r * r = x: the length, its
// refined reciprocal and the float r * r, NaN where the reciprocal is (fill_norm_row, as the render kernels' prologue calls it),
// 52 / 53 an axis sphere's discriminant stage on caller-given rays, in records of 8 doubles: a = (ox, oy, oz, dx, dy, dz, -, -),
// b = (pattern 1 / 2 / 3, c, r * r, -2 c, K, -, -, -), out = (b, D4, 0 ..) — 52 the form of rounds 4 to 8 from (c, r * r)
// (rtm_path.h: sphere_disc_ref, the reference), 53 the expanded form from the axis row (c, -2 c, K) as the search runs it now,
// 54 the same for a sphere of the signature's shared-K group (oo + K formed first),
// 55 / 56 the whole nearest-hit search of a seven-sphere scene with the Cornell box's signature on caller-given rays (records as
// above; b: the scene's 7 geometry rows and, behind them, its 7 axis rows, 56 doubles, as a scene object keeps them): 55 with the
// opposite wall pairs (kAxisSigCornell7Pairs), out = (distance, hit id, 1 where the ray's wave took the seven-sphere block, 0 ..),
// 56 the seven-sphere block itself (kAxisSigCornell7Walls), out = (distance, hit id, 0 ..),
// 57 / 58 the words a lane leaves the roulette with, in records of 8 doubles, ONE LANE per record (lane i: record i), a = (p0, p1,
// ctr, k1, n', ended, -, -) with the 32-bit words as doubles; the stream (ctr, k1) makes the roulette's draw first; out = (m of the
// bounce's first draw, m of its second, ctr, k1 of the stream the lane goes on with, 0 ..) — a continuing lane's two draws and
// its stream three draws on, an ended lane's (0, 0, rng_open((p0, p1), n')): 57 through rng_merged_mix (one mix32 pair for both
// kinds of lane, as the render loops run it), 58 through rng_next_mi / rng_next / rng_open (its reference),
// 59 / 60 a bounce direction before its Normalize, records and lanes as 57 / 58, a = (w.x, w.y, w.z, m1, m2, -, -, -) with w the
// turned normal (no zero component) and m1, m2 the odd integers of the bounce's two draws, out = (nd.x, nd.y, nd.z, 1 where the
// lane set `bad`, 0 ..): 59 from one reciprocal root, without the basis (rtm_path.h: bounce_nd_fused, as the shading block runs
// it), 60 with the basis built (bounce_nd_basis: the form of rounds 2 to 13, its reference),
// 61 / 62 op 55's search on op 55's records, out = (distance, hit id, 1 where the ray's wave took the general acceptance chain,
// 1 where it took the seven-sphere block, 1 where it asked the far-root question a second time, 0 ..): 61 as the render kernels
// run it — a pair's wall forms no t2 (rtm_path.h: accept_batch_lane's WALLS) —, 62 with t2 formed for every candidate (the form
// of rounds 10 to 14, its reference)
__global__ void tol_math_probe_kernel(int op, const double* __restrict__ a, const double* __restrict__ b, size_t n,
                                      double* __restrict__ out, const double2* __restrict__ tab) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op >= 52 && op <= 54) {  // records of 8 doubles: every thread of a record computes it, each stores its own slot
        const size_t j = i & ~(size_t)7;
        double bb = 0.0, D4 = 0.0;
        if (b && j + 7 < n) {
            const D3 org = d3(a[j], a[j + 1], a[j + 2]), dir = d3(a[j + 3], a[j + 4], a[j + 5]);
            const unsigned pat = (unsigned)b[j];
            const double c = b[j + 1];
            if (pat >= 1u && pat <= 3u) {
                if (op == 52) {
                    const double4 g = double4{pat == 1u ? c : 0.0, pat == 2u ? c : 0.0, pat == 3u ? c : 0.0, b[j + 2]};
                    sphere_disc_ref(g, pat, org, dir, AxisSharedRef(org, dir), bb, D4);
                } else {
                    const AxisShared A(org, dir);
                    sphere_disc(double4{}, AxisRow{c, b[j + 3], b[j + 4]}, pat, op == 54, A.oo + b[j + 4], org, dir, A, bb, D4);
                }
            }
        }
        out[i] = (i & 7) == 0 ? bb : (i & 7) == 1 ? D4 : 0.0;
        return;
    }
    if (op == 55 || op == 56 || op == 61 || op == 62) {  // (as above: every thread of a record computes it; a wave holds 8 rays)
        const size_t j = i & ~(size_t)7;
        double dis = DBL_MAX;
        int hit = -1;
        bool fell_back = false, general = false, again = false;
        if (b && n >= 56 && j + 7 < n) {
            const D3 org = d3(a[j], a[j + 1], a[j + 2]), dir = d3(a[j + 3], a[j + 4], a[j + 5]);
            SceneGlobal sc{};
            sc.v.geom = reinterpret_cast<const double4*>(b);
            sc.v.n = 7;
            if (op == 55) sphere_chunk<MathFast, 7, SceneGlobal, false, kAxisSigCornell7Pairs>(sc, 0, org, dir, dis, hit, &fell_back);
            else if (op == 61) sphere_chunk<MathFast, 7, SceneGlobal, false, kAxisSigCornell7Pairs>(sc, 0, org, dir, dis, hit, &fell_back, &general, &again);
            else if (op == 62) sphere_chunk<MathFast, 7, SceneGlobal, false, kAxisSigCornell7Pairs, true>(sc, 0, org, dir, dis, hit, &fell_back, &general, &again);
            else sphere_chunk<MathFast, 7, SceneGlobal, false, kAxisSigCornell7Walls>(sc, 0, org, dir, dis, hit);
        }
        const bool f2 = op >= 61 ? general : fell_back, f3 = op >= 61 && fell_back;
        const unsigned s = (unsigned)(i & 7);
        out[i] = s == 0u ? dis : s == 1u ? (double)hit : s == 2u ? (f2 ? 1.0 : 0.0) : s == 3u ? (f3 ? 1.0 : 0.0) : s == 4u ? (again ? 1.0 : 0.0) : 0.0;
        return;
    }
    if (op == 57 || op == 58) {  // ONE lane per record (a wave holds 64 records: the caller mixes the two kinds of lane in it)
        if (i * 8 + 7 >= n) return;
        const double* q = a + i * 8;
        const RngPixelKey pk{(uint32_t)q[0], (uint32_t)q[1]};
        RngStream st{(uint32_t)q[2], (uint32_t)q[3]};
        const uint32_t n_next = (uint32_t)q[4];
        const bool ended = q[5] != 0.0;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        (void)rng_next_mi(st);  // the roulette's draw
        if (op == 57) {
            const RngStream m = rng_merged_mix(ended, pk, n_next, st);
            if (ended) {
                w[2] = m.ctr;
                w[3] = m.k1;
            } else {
                w[0] = rng_bits_to_mi(m.ctr);
                w[1] = (uint32_t)(rng_bits_to_u01(m.k1) * 16777216.0);
                w[2] = st.ctr + 2u * 0x9E3779B9u;
                w[3] = st.k1;
            }
        } else if (ended) {
            st = rng_open(pk, n_next);
            w[2] = st.ctr;
            w[3] = st.k1;
        } else {
            w[0] = rng_next_mi(st);
            w[1] = (uint32_t)(rng_next(st) * 16777216.0);
            w[2] = st.ctr;
            w[3] = st.k1;
        }
        for (int k = 0; k < 8; ++k) out[i * 8 + k] = k < 4 ? (double)w[k] : 0.0;
        return;
    }
    if (op == 59 || op == 60) {  // ONE lane per record, as above; `tab`: the device's sin / cos table
        if (i * 8 + 7 >= n) return;
        const double* q = a + i * 8;
        const D3 w = d3(q[0], q[1], q[2]);
        const uint32_t m1 = (uint32_t)q[3];
        const double r2 = (double)(uint32_t)q[4] * (1.0 / 16777216.0);  // rng_bits_to_u01's value for the draw's integer
        MathSpec m;
        m.trig_tab = tab;
        const MathSpec::TrigAhead ahead = m.sincos_draw_issue(m1);
        const D3 nd = op == 59 ? bounce_nd_fused(m, w, r2, ahead) : bounce_nd_basis(m, w, r2, ahead);
        const double res[4] = {nd.x, nd.y, nd.z, m.bad ? 1.0 : 0.0};
        for (int k = 0; k < 8; ++k) out[i * 8 + k] = k < 4 ? res[k] : 0.0;
        return;
    }
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
        case 42: sincos_turn24_tab_apply(sincos_turn24_tab_load(tab, (uint32_t)x), s, c); r = s; break;
        case 43: sincos_turn24_tab_apply(sincos_turn24_tab_load(tab, (uint32_t)x), s, c); r = c; break;
        case 44: { MathSpec m; r = m.sqrt64_unit(x); } break;
        case 45: {  // op 41 with h0 = 0.5 * y by the multiply (rtm_path.h: half_of_rsq_ref)
            const double in[1] = {x};
            double out1[1];
            seq_sqrt_batch<1, true, true>(in, out1);
            r = out1[0];
            break;
        }
        case 48: {  // op 32 with h0 = 0.5 * y by the multiply: the full root's reference form
            const double in[1] = {x};
            double out1[1];
            seq_sqrt_batch<1, false, true>(in, out1);
            r = out1[0];
            break;
        }
        case 49: case 50: case 51: {  // a sphere's row of the normal table for r * r = x (rtm_path.h: fill_norm_row): ms, rinv, r2f
            double row[3];
            fill_norm_row(row, x);
            r = op == 51 ? (double)reinterpret_cast<const float*>(row + 2)[0] : row[op - 49];
            break;
        }
        case 46: sincos_turn24_tab_ref(tab, x, s, c); r = s; break;
        case 47: sincos_turn24_tab_ref(tab, x, s, c); r = c; break;
        default: break;
    }
    out[i] = r;
}

}  // namespace rtm_tol

namespace rtm {

// The shading block's sin / cos table (rtm_device.h: sincos_turn24_tab_load): entry i = (sin, cos) of i 2 pi / entries, each
// evaluated in long double and rounded to double once.  HOST only; rtm_debug_trig_table hands it to the tests.
int trig_table_host(int entries, double* out) {
    if (!out || entries < 1 || entries > (1 << 20)) return RTM_ERR_INVALID_ARGUMENT;
    const long double step = 6.283185307179586476925286766559L / (long double)entries;
    for (int i = 0; i < entries; ++i) {
        const long double a = (long double)i * step;
        out[2 * i] = (double)sinl(a);
        out[2 * i + 1] = (double)cosl(a);
    }
    return RTM_OK;
}

// ... a variable of the device code (rtm_device.h: g_trig_tab), filled once per device: a constant of the build — nothing of a
// scene or a frame enters it —, read-only and shared by every stream's launches
namespace {
std::mutex g_trig_tab_mu;
std::map<int, const double2*> g_trig_tab_filled;  // device -> the variable's address there
}  // namespace

static int ensure_trig_tab(const double2** out) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return RTM_ERR_HIP;
    std::lock_guard<std::mutex> lock(g_trig_tab_mu);
    const auto it = g_trig_tab_filled.find(device);
    if (it != g_trig_tab_filled.end()) {
        *out = it->second;
        return RTM_OK;
    }
    constexpr size_t kBytes = (size_t)rtm_tol::kTrigTabEntries * sizeof(double2);
    std::vector<double> host(2 * (size_t)rtm_tol::kTrigTabEntries);
    const int rc = trig_table_host(rtm_tol::kTrigTabEntries, host.data());
    if (rc != RTM_OK) return rc;
    void* dev = nullptr;
    // (a blocking copy and the null stream drained: whatever stream launches next finds the table written)
    if (hipGetSymbolAddress(&dev, HIP_SYMBOL(rtm_tol::g_trig_tab)) != hipSuccess || dev == nullptr ||
        hipMemcpy(dev, host.data(), kBytes, hipMemcpyHostToDevice) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
        (void)hipGetLastError();
        return RTM_ERR_HIP;
    }
    g_trig_tab_filled[device] = static_cast<const double2*>(dev);
    *out = static_cast<const double2*>(dev);
    return RTM_OK;
}

// release_scratch's share: nothing — the table lives in the code object, not in memory this library allocated, and stays filled
void release_trig_tab(int device) { (void)device; }

// rtm_debug_tol_lds_bytes: what launch_tiles asks for, per shape of the row (HOST only; tests/test_trip_slots_host.py)
int tol_lds_bytes(int n, int any_depth, int split, int rows, uint64_t* out) {
    using namespace rtm_tol;
    if (!out || n < 1 || n > 24) return RTM_ERR_INVALID_ARGUMENT;
    unsigned unit = 0u;
    const bool r = rows != 0;
    size_t b;
    if (any_depth) b = split ? render_lds_bytes<kTolAny | kSplit, uint8_t, 0>(n, r, 0, &unit) : render_lds_bytes<kTolAny, uint8_t, 0>(n, r, 0, &unit);
    else b = split ? render_lds_bytes<kTolCapped | kSplit, uint8_t, 16>(n, r, 0, &unit) : render_lds_bytes<kTolCapped, uint8_t, 16>(n, r, 0, &unit);
    out[0] = (uint64_t)b;
    out[1] = unit;
    return RTM_OK;
}

int tol_math_probe(int op, const double* a_dev, const double* b_dev, size_t n, double* out_dev) {
    const double2* tab = nullptr;
    if (op == 42 || op == 43 || op == 46 || op == 47 || op == 59 || op == 60) {
        if (ensure_trig_tab(&tab) != RTM_OK) {
            set_last_error("tolerance row: the sin / cos table could not be written on the device");
            return RTM_ERR_HIP;
        }
    }
    rtm_tol::tol_math_probe_kernel<<<(unsigned)((n + 255) / 256), 256>>>(op, a_dev, b_dev, n, out_dev, tab);
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
    // ... by table point and two series terms: the table is the device's, filled at the first launch (the kernels name it)
    const double2* trig_tab = nullptr;
    if (ensure_trig_tab(&trig_tab) != RTM_OK) {
        set_last_error("tolerance row: the sin / cos table could not be written on the device");
        return RTM_ERR_HIP;
    }
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
