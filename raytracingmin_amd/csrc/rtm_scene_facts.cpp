// rtm_scene_facts.cpp — the host-only half of making a scene (rtm_scene_facts.h): flattening, the proofs that gate the
// kernels' shortcuts, the axis rows, the host grid builder, and the test hooks that show each of them without a device.
// Every proof here is the only gate in front of a kernel path that is wrong outside its envelope.  Plain C++ (-x c++,
// -ffp-contract=off like the kernels): links with rtm_scene.cpp alone, which is how scene_facts_selftest.cpp runs it under
// sanitizers.
#include "rtm_scene_facts.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace rtm {

// Flatten rtm_sphere[] to the kernel layout.  kd and colorKD are hoisted: the same
// IEEE operations the reference redoes per bounce (src/SettingData.h:11-16).
void flatten_scene(const rtm_sphere* sp, size_t n, std::vector<double>& geom, std::vector<double>& mat,
                   std::vector<double>* surf) {
    if (surf) {  // png::SurfaeSample's extras: the raw colour and the radius as the float it is (rtm_surface.h)
        surf->resize((n ? n : 1) * 4);
        for (size_t i = 0; i < n; ++i) {
            for (int k = 0; k < 3; ++k) (*surf)[i * 4 + k] = sp[i].color[k];
            (*surf)[i * 4 + 3] = (double)sp[i].radius;
        }
    }
    geom.resize(n * 4);
    mat.assign((n + 1) * 8, 0.0);
    mat[n * 8 + 0] = mat[n * 8 + 1] = mat[n * 8 + 2] = 1.0;  // identity row for path_fold_blocked
    for (size_t i = 0; i < n; ++i) {
        const float r2 = sp[i].radius * sp[i].radius;  // float product, src/SettingData.cpp:200
        geom[i * 4 + 0] = sp[i].center[0];
        geom[i * 4 + 1] = sp[i].center[1];
        geom[i * 4 + 2] = sp[i].center[2];
        geom[i * 4 + 3] = (double)r2;
        double m = sp[i].color[0] < sp[i].color[1] ? sp[i].color[1] : sp[i].color[0];
        m = m < sp[i].color[2] ? sp[i].color[2] : m;
        const double kd = (double)(float)m;  // kd() returns float
        mat[i * 8 + 0] = sp[i].color[0] / kd;
        mat[i * 8 + 1] = sp[i].color[1] / kd;
        mat[i * 8 + 2] = sp[i].color[2] / kd;
        mat[i * 8 + 3] = sp[i].emission[0];
        mat[i * 8 + 4] = sp[i].emission[1];
        mat[i * 8 + 5] = sp[i].emission[2];
        mat[i * 8 + 6] = kd;
        mat[i * 8 + 7] = kd * 16777216.0;  // kd * 2^24 (exact): the RR test compares it with the draw's integer
    }
}

// SceneView::axis_pat from flattened geometry rows (cx, cy, cz, r*r): 1 / 2 / 3 where x / y / z is the centre's only
// coordinate that is not +-0 (all finite), else 0; a plane's row (negative "r*r") is 0.
static uint64_t axis_pattern(const double* geom, size_t n) {
    uint64_t pat = 0;
    for (size_t i = 0; i < n && i < 32; ++i) {
        const double* g = geom + i * 4;
        if (!(std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2])) || !(g[3] >= 0.0)) continue;
        const bool zx = g[0] == 0.0, zy = g[1] == 0.0, zz = g[2] == 0.0;
        const uint64_t a = (!zx && zy && zz) ? 1u : (zx && !zy && zz) ? 2u : (zx && zy && !zz) ? 3u : 0u;
        pat |= a << (2 * i);
    }
    return pat;
}
// The tolerance unit's AXIS ROWS (rtm_path.h: sphere_disc under RTM_TOL), one of 32 bytes per sphere of a scene of at most 32,
// kept behind the n geometry rows of an rtm_scene (row n + i belongs to sphere i): for a sphere with pattern a != 0 and centre
// coordinate c on that axis (c, -2 c, K = c c - r*r, e), for pattern 0 zeros (unused).  K from the row's own c and its stored
// r*r (geom.w, the float product widened) as one fused long-double operation: TWO roundings, one to 64 bits and one to double —
// exact for the shipped scenes, the Cornell walls' 200100 among them.  e (not read by the kernels; rtm_debug_axis_rows shows
// it): the reach 2^k of the expanded form's envelope where the host has proven the SCENE inside it (axis_reach_bits), else 0.  Derived data of the geometry rows: nothing
// new enters a scene's cache key.  (kAxisRowsMax: rtm_scene_flags.h; axis_row_count: rtm_scene_facts.h)
// rtm_scene_flags.h, kSceneAxisReachShift: the bound on the expanded q's rounding error for origins within `reach` of the origin
static double axis_q_err(double own_reach, double reach) {
    const double m = own_reach > reach ? own_reach : reach;
    return std::ldexp(m * m, -49);
}
static bool axis_self_hit_safe(double c, double r2) {  // test (A)
    const double r = std::sqrt(r2), own = std::fabs(c) + r;
    return r > 0.0 && std::isfinite(own) && axis_q_err(own, 0.0) / (2.0 * r) <= std::ldexp((double)1e-5f, -17);
}
// SceneView::fold_flags' bits 16..23 (kSceneAxisReachShift): 128 + k where every axis sphere passes (A), and (B) for origins
// within 2^k, and the whole scene lies within 2^k; 0 where that is not proven (no axis sphere, more than 32 spheres, a sphere
// outside the envelope)
static unsigned axis_reach_bits(const double* geom, size_t n, uint64_t pat) {
    if (axis_row_count(n) == 0 || pat == 0) return 0u;
    double extent = 0.0, reach = kCompactExtent;
    for (size_t i = 0; i < n; ++i) {
        const double* g = geom + i * 4;
        const double own = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) + std::sqrt(std::fabs(g[3]));
        if (!std::isfinite(own)) return 0u;
        extent = own > extent ? own : extent;
        const unsigned a = (unsigned)(pat >> (2 * i)) & 3u;
        if (a == 0u) continue;
        if (!axis_self_hit_safe(g[a - 1u], g[3])) return 0u;
        // (B): err(rho) / (2 r) <= 2^-4 x 1e-5f  <=>  rho^2 <= 2^46 x 1e-5f x r
        const double rho = std::sqrt(std::ldexp((double)1e-5f * std::sqrt(g[3]), 46));
        reach = rho < reach ? rho : reach;
    }
    const int k = std::ilogb(reach);  // 2^k <= reach
    if (!(reach >= 1.0) || !(extent <= std::ldexp(1.0, k))) return 0u;
    return (unsigned)(128 + k) << kSceneAxisReachShift;
}
static void axis_rows(const double* geom, size_t n, uint64_t pat, double* rows) {
    const unsigned e = (axis_reach_bits(geom, n, pat) >> kSceneAxisReachShift) & kSceneAxisReachMask;
    const double reach = e ? std::ldexp(1.0, (int)e - 128) : 0.0;
    for (size_t i = 0; i < axis_row_count(n); ++i) {
        const unsigned a = (unsigned)(pat >> (2 * i)) & 3u;
        double* row = rows + i * 4;
        row[0] = row[1] = row[2] = row[3] = 0.0;
        if (a == 0u) continue;
        const double c = geom[i * 4 + (a - 1u)];
        row[0] = c;
        row[1] = -2.0 * c;
        row[2] = (double)fmal((long double)c, (long double)c, -(long double)geom[i * 4 + 3]);
        row[3] = reach;
    }
}
// SceneView::fold_flags' bits 8..15 (kSceneSharedKShift): among the first 8 spheres, the largest group of axis spheres whose
// axis rows hold one K bit for bit (the lowest group on a tie); 0 where no two do
static unsigned shared_k_bits(const double* geom, size_t n, uint64_t pat) {
    if (axis_row_count(n) == 0) return 0u;
    std::vector<double> rows(n * 4);
    axis_rows(geom, n, pat, rows.data());
    unsigned best = 0u, best_count = 1u;
    for (size_t i = 0; i < n && i < 8; ++i) {
        if (((pat >> (2 * i)) & 3u) == 0u) continue;
        unsigned mask = 0u, count = 0u;
        for (size_t j = i; j < n && j < 8; ++j)
            if (((pat >> (2 * j)) & 3u) != 0u && std::memcmp(&rows[j * 4 + 2], &rows[i * 4 + 2], sizeof(double)) == 0) {
                mask |= 1u << j;
                ++count;
            }
        if (count > best_count) {
            best = mask;
            best_count = count;
        }
    }
    return best << kSceneSharedKShift;
}
// kSceneCompact from flattened geometry rows (cx, cy, cz, r*r): every sphere within kCompactExtent of the origin
static unsigned compact_flag_of(const double* geom, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const double* g = geom + i * 4;
        const double reach = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) + std::sqrt(std::fabs(g[3]));
        if (!(reach <= kCompactExtent)) return 0u;  // (NaN fails too)
    }
    return kSceneCompact;
}
// SceneView::fold_flags' kSceneWallPairs (rtm_path.h: kAxisPairsBit, the tolerance unit's one root and one acceptance per
// opposite wall pair): set where the members of the shared-K group, taken two by two in index order, are opposite pairs —
// both on one axis, the lower index at +c and the other at -c bit for bit, one r*r — AND the scene is compact and inside the
// expanded form's envelope AND the proof's constants hold for it: gamma / (2 beta) + reach 2^-44 < 1e-5f / 2 (what a skipped
// wall's far root can reach stays under half of Intersect's threshold) and r 2^-17 >= 2 beta for every paired sphere (a bounce
// ray leaving its own wall at the envelope's smallest cosine passes the proof).  *lower (optional): bit i = sphere i is the
// lower member of a pair that passes the per-pair tests, whether or not the scene as a whole is granted the extension.
static unsigned wall_pairs_flag(const double* geom, size_t n, uint64_t pat, unsigned* lower = nullptr) {
    if (lower) *lower = 0u;
    const unsigned group = (shared_k_bits(geom, n, pat) >> kSceneSharedKShift) & kSceneSharedKMask;
    const unsigned e = (axis_reach_bits(geom, n, pat) >> kSceneAxisReachShift) & kSceneAxisReachMask;
    if (group == 0u || e == 0u || compact_flag_of(geom, n) == 0u) return 0u;
    const double reach = std::ldexp(1.0, (int)e - 128);
    const bool far_root_ok = kPairGamma / (2.0 * kPairBeta) + std::ldexp(reach, -44) < 0.5 * (double)1e-5f;
    int members[8], count = 0;
    for (int i = 0; i < 8; ++i)
        if ((group >> i) & 1u) members[count++] = i;
    bool all = far_root_ok && count % 2 == 0;
    unsigned low = 0u;
    for (int m = 0; m + 1 < count; m += 2) {
        const int i = members[m], j = members[m + 1];
        const unsigned a = (unsigned)(pat >> (2 * i)) & 3u;
        const double ci = geom[i * 4 + (a - 1u)], cj = geom[j * 4 + (a - 1u)], mci = -ci;
        const bool ok = a == ((unsigned)(pat >> (2 * j)) & 3u) && ci > 0.0 && std::memcmp(&mci, &cj, sizeof(double)) == 0 &&
                        std::memcmp(&geom[i * 4 + 3], &geom[j * 4 + 3], sizeof(double)) == 0 &&
                        std::ldexp(std::sqrt(geom[i * 4 + 3]), -17) >= 2.0 * kPairBeta;
        if (ok) low |= 1u << i;
        all = all && ok;
    }
    if (lower) *lower = low;
    return all && count >= 2 ? kSceneWallPairs : 0u;
}

// SceneView::fold_flags from flattened material rows (colorKD[3], emission[3], kd, kd * 2^24): see kFoldNoLevelEmission
static unsigned fold_flags_of(const double* mat, size_t n) {
    auto plain = [](double v) { return !std::signbit(v) && !std::isnan(v); };  // +0 or positive (or +inf)
    for (size_t i = 0; i < n; ++i) {
        const double* m = mat + i * 8;
        if (!(plain(m[3]) && plain(m[4]) && plain(m[5]))) return 0u;  // a path may END on any object: L starts as its emission
        if (m[6] > 0.0) {  // a path can bounce off this one (the roulette passes only for a draw <= kd, and draws are > 0)
            if (!(m[3] == 0.0 && m[4] == 0.0 && m[5] == 0.0)) return 0u;
            if (!(plain(m[0]) && plain(m[1]) && plain(m[2]))) return 0u;
        }
    }
    return kFoldNoLevelEmission;
}
// ... and kFoldZeroTermSkippable with SceneView::emit_mask, from the same rows: on top of kFoldNoLevelEmission every colorKD of
// an object a path can bounce off is finite (0 x inf is NaN, not +0) and there are at most 63 objects, so that each — and the
// identity row, which never emits — has a bit of the mask.  *emit_mask: bit i = object i's emission row is not (+0, +0, +0);
// all ones where the flag is not proven (every path end is then queued and folded, as before).
static unsigned zero_term_flags_of(const double* mat, size_t n, uint64_t* emit_mask) {
    *emit_mask = ~(uint64_t)0;
    if (n > 63 || fold_flags_of(mat, n) == 0u) return 0u;
    uint64_t mask = 0;
    for (size_t i = 0; i < n; ++i) {
        const double* m = mat + i * 8;
        if (m[6] > 0.0 && !(std::isfinite(m[0]) && std::isfinite(m[1]) && std::isfinite(m[2]))) return 0u;
        // (kFoldNoLevelEmission: no emission is NaN or carries a sign bit, so "not +0" is "> 0")
        if (m[3] > 0.0 || m[4] > 0.0 || m[5] > 0.0) mask |= (uint64_t)1 << i;
    }
    *emit_mask = mask;
    return kFoldZeroTermSkippable;
}

// The facts of a scene, put together (rtm_scene_facts.h: SceneFacts)
SceneFacts scene_facts(const double* geom, const double* mat, size_t n, double* axis_rows_out) {
    SceneFacts f;
    f.axis_pat = axis_pattern(geom, n);
    f.fold_flags = fold_flags_of(mat, n) | compact_flag_of(geom, n) | zero_term_flags_of(mat, n, &f.emit_mask) |
                   shared_k_bits(geom, n, f.axis_pat) | axis_reach_bits(geom, n, f.axis_pat) |
                   wall_pairs_flag(geom, n, f.axis_pat);
    axis_rows(geom, n, f.axis_pat, axis_rows_out);
    return f;
}

// png::PlaneObject's constructor (src/SettingData.cpp:235-242) on the host, in the reference's operation order;
// `upv` and the two squared half-extents are this build's completion (include/rtm.h).
void plane_row(const rtm_object& o, double row[16]) {
    using namespace host;
    const H3 pos = {o.position[0], o.position[1], o.position[2]};
    const H3 nrm = normalize(sub(H3{o.target[0], o.target[1], o.target[2]}, pos));  // :240
    const H3 rn = normalize(cross(nrm, H3{o.up[0], o.up[1], o.up[2]}));             // :241 Normalize(Cross(..))
    const H3 right = {rn.x * 0.5 * o.width, rn.y * 0.5 * o.width, rn.z * 0.5 * o.width};  // (v * 0.5) * width
    const H3 upv = cross(right, nrm);
    const double v[16] = {pos.x, pos.y, pos.z, nrm.x, nrm.y, nrm.z, right.x, right.y, right.z, upv.x, upv.y, upv.z,
                          right.x * right.x + right.y * right.y + right.z * right.z,
                          upv.x * upv.x + upv.y * upv.y + upv.z * upv.z, 0.0, 0.0};
    std::memcpy(row, v, sizeof v);
}

// ---- uniform grid of a large scene (rtm_grid_header.h: GridHeader; rtm_path.h: GridWalk, where the pads are derived) ------------------
// Built on the host from the flattened geometry rows (cx, cy, cz, float r*r) when a scene OBJECT is created: 25 ms for
// 100 000 spheres on one core, once per scene.  ~2 cells per sphere (RTM_DEBUG_GRID_CELLS); a sphere whose padded box
// covers more than kGridBigCells cells goes to the list every ray tests.  No grid (the other kernels serve the scene)
// for fewer than kGridMinSpheres gridded spheres (below that the packed-record kernels are as fast or faster:
// profiles/r3/grid_crossover.txt), non-finite geometry, more than kGridMaxBig big spheres or planes.
double grid_cells_per_sphere() {
    static const double v = [] {
        const char* e = std::getenv("RTM_DEBUG_GRID_CELLS");  // tuning knob: cells per sphere; 0 = build no grid
        return e ? std::strtod(e, nullptr) : 1.5;  // (round 4, with the next-cell fill: flat between 1.35 and 1.65, 2.0 is 2.3 % slower — profiles/r4/grid_cells.txt)
    }();
    return v;
}
// The scalar arithmetic of a build, host code for the host builder below and for the device build (rtm_grid_build.hip) alike.
// A classification round's cell edge and pad horizon from the box of the spheres that are not big: the edge from the box's
// volume, the pads from its diagonal.  false: no grid.
bool grid_round_scalars(const double lo[3], const double hi[3], size_t n_small, double lambda, double& h, double& t_ok) {
    double ext[3], diag2 = 0.0, vol = 1.0, longest = 0.0;
    for (int k = 0; k < 3; ++k) {
        ext[k] = hi[k] - lo[k];
        diag2 += ext[k] * ext[k];
        longest = std::max(longest, ext[k]);
    }
    if (!(longest > 0.0) || !std::isfinite(diag2)) return false;
    for (int k = 0; k < 3; ++k) vol *= std::max(ext[k], longest * 1e-3);  // (a flat scene still gets cells of a sane size)
    h = std::cbrt(vol / (lambda * (double)n_small));
    h = std::max(h, longest / (double)(kGridMaxDim - 2));
    t_ok = 2.5 * std::sqrt(diag2);
    return true;
}
// The header from the small spheres' padded box (lo, hi: changed), *cells = the number of cells.  false: no grid.
bool grid_header_from_box(double lo[3], const double hi[3], double h, double t_ok, size_t n, size_t n_big, GridHeader& H,
                          size_t* cells_out) {
    std::memset(&H, 0, sizeof H);
    size_t cells = 1;
    for (int k = 0; k < 3; ++k) {
        lo[k] -= 0.01 * h;
        int d = (int)std::ceil((hi[k] + 0.01 * h - lo[k]) / h);
        d = d < 1 ? 1 : d;
        if (d > kGridMaxDim) return false;
        H.lo[k] = lo[k];
        H.hi[k] = lo[k] + (double)d * h;
        H.dim[k] = d;
        cells *= (size_t)d;
    }
    if (cells > 64 * n + 4096) return false;  // (cannot happen with cells of the volume's size; a guard for the host's memory)
    H.h = h;
    H.inv_h = 1.0 / h;
    H.t_ok = t_ok;
    double half2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        H.cb[k] = 0.5 * (H.lo[k] + H.hi[k]);
        half2 += 0.25 * (H.hi[k] - H.lo[k]) * (H.hi[k] - H.lo[k]);
    }
    const double reach = t_ok / 1.001 - std::sqrt(half2);  // (t_ok = 2.5 diagonals of the unpadded box: about two of them)
    if (!(reach > 0.0)) return false;
    H.reach2 = reach * reach;
    H.dd_tol = kGridDdTol;
    H.n_big = (int)n_big;
    *cells_out = cells;
    return true;
}
GridBuildDims grid_build_dims(const GridHeader& H) {
    GridBuildDims D;
    for (int k = 0; k < 3; ++k) {
        D.lo[k] = H.lo[k];
        D.dim[k] = H.dim[k];
    }
    D.h = H.h;
    return D;
}
bool make_grid(const double* g, size_t n, GridBuild& out, double* pads_out) {
    const double lambda = grid_cells_per_sphere();
    if (n < kGridMinSpheres || n >= (1u << 29) || !(lambda > 0.0)) return false;
    std::vector<double> R(n), pad(n);
    std::vector<char> is_big(n, 0);
    std::vector<char> is_plane(n, 0);  // a png::PlaneObject's geometry row is (position, negative "r*r"): tested by every ray
    for (size_t i = 0; i < n; ++i) {
        const double* r = g + i * 4;
        if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) && std::isfinite(r[3]))) return false;
        R[i] = grid_sphere_R(r[3]);
        if (r[3] < 0.0) {
            is_plane[i] = is_big[i] = 1;
            continue;
        }
        unsigned long long wbits;
        std::memcpy(&wbits, &r[3], sizeof wbits);
        if (wbits & 0x1FFFFFFFull) return false;  // (never: r*r is a float widened to double — the records keep the index there)
    }
    double lo[3], hi[3], h = 0.0, t_ok = 0.0;
    size_t n_small = 0;
    for (size_t i = 0; i < n; ++i) n_small += !is_plane[i];
    if (n_small < kGridMinSpheres) return false;
    for (int round = 0; round < 4; ++round) {
        // box of the small spheres (unpadded), cell edge from its volume, pads from its diagonal
        for (int k = 0; k < 3; ++k) {
            lo[k] = HUGE_VAL;
            hi[k] = -HUGE_VAL;
        }
        for (size_t i = 0; i < n; ++i) {
            if (is_big[i]) continue;
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], g[i * 4 + k] - R[i]);
                hi[k] = std::max(hi[k], g[i * 4 + k] + R[i]);
            }
        }
        if (!grid_round_scalars(lo, hi, n_small, lambda, h, t_ok)) return false;
        size_t changed = 0;
        n_small = 0;
        for (size_t i = 0; i < n; ++i) {
            pad[i] = grid_sphere_pad(R[i], h, t_ok);
            const char b = is_plane[i] || grid_sphere_is_big(R[i], pad[i], h);
            changed += b != is_big[i];
            is_big[i] = b;
            n_small += !b;
        }
        if (n_small < kGridMinSpheres) return false;
        if (!changed && round > 0) break;
    }
    out.big.clear();
    for (size_t i = 0; i < n; ++i)
        if (is_big[i]) out.big.push_back((int)i);
    if (out.big.size() > (size_t)kGridMaxBig) return false;
    // the grid's box: the small spheres' padded boxes
    for (int k = 0; k < 3; ++k) {
        lo[k] = HUGE_VAL;
        hi[k] = -HUGE_VAL;
    }
    for (size_t i = 0; i < n; ++i) {
        if (is_big[i]) continue;
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], g[i * 4 + k] - R[i] - pad[i]);
            hi[k] = std::max(hi[k], g[i * 4 + k] + R[i] + pad[i]);
        }
    }
    if (pads_out) std::memcpy(pads_out, pad.data(), n * sizeof(double));
    GridHeader& H = out.hdr;
    size_t cells = 0;
    if (!grid_header_from_box(lo, hi, h, t_ok, n, out.big.size(), H, &cells)) return false;
    const GridBuildDims D = grid_build_dims(H);
    // counting sort of (cell, sphere) pairs; spheres are visited in index order, so every cell's list ascends
    out.cell_start.assign(cells + 1, 0u);
    size_t refs = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t i = 0; i < n; ++i) {
            if (is_big[i]) continue;
            grid_sphere_cells(g + i * 4, pad[i], D, [&](size_t c) {
                if (pass == 0) {
                    ++out.cell_start[c + 1];
                    ++refs;
                } else {
                    out.items[out.cell_start[c]++] = (unsigned)i;
                }
            });
        }
        if (pass == 0) {
            if (refs > 0xFFFFFF00ull) return false;
            for (size_t c = 0; c < cells; ++c) out.cell_start[c + 1] += out.cell_start[c];
            out.items.assign(refs ? refs : 1, 0u);
            out.refs = refs;
        } else {  // the fill advanced every start to its end: shift back
            for (size_t c = cells; c > 0; --c) out.cell_start[c] = out.cell_start[c - 1];
            out.cell_start[0] = 0u;
        }
    }
    return true;
}
// rtm_debug_grid_build: the builder alone, on the HOST (no device is touched) — what tests/test_host_io.py checks the
// lists' invariants on.  info[12] = {cells, records, big, dim x, y, z} then, as doubles' bit patterns, {lo x, y, z, h, reach,
// t_ok}; pads: n doubles (a big sphere's is its pad too); with buffers, ranges: 2 x cells unsigned, items: `records` sphere
// indices, big: `big` sphere indices.  RTM_ERR_UNSUPPORTED when the scene gets no grid, RTM_ERR_CAPACITY when a buffer is short.
int grid_build_host(const rtm_sphere* sp, size_t n, uint64_t* info, double* pads, uint32_t* ranges, size_t ranges_cap,
                    uint32_t* items, size_t items_cap, int32_t* big, size_t big_cap) {
    if (!sp || !n || !info) return RTM_ERR_INVALID_ARGUMENT;
    std::vector<double> hg, hm;
    flatten_scene(sp, n, hg, hm);
    GridBuild B;
    if (!make_grid(hg.data(), n, B, pads)) return unsupported("this scene gets no grid");
    const size_t cells = B.cell_start.size() - 1;
    info[0] = cells;
    info[1] = B.refs;
    info[2] = B.big.size();
    for (int k = 0; k < 3; ++k) info[3 + k] = (uint64_t)B.hdr.dim[k];
    const double d[6] = {B.hdr.lo[0], B.hdr.lo[1], B.hdr.lo[2], B.hdr.h, std::sqrt(B.hdr.reach2), B.hdr.t_ok};
    std::memcpy(info + 6, d, sizeof d);
    if ((ranges && ranges_cap < cells * 2) || (items && items_cap < B.refs) || (big && big_cap < B.big.size())) return RTM_ERR_CAPACITY;
    if (ranges)
        for (size_t c = 0; c < cells; ++c) {
            ranges[c * 2] = B.cell_start[c];
            ranges[c * 2 + 1] = B.cell_start[c + 1];
        }
    if (items) std::memcpy(items, B.items.data(), B.refs * sizeof(unsigned));
    if (big && !B.big.empty()) std::memcpy(big, B.big.data(), B.big.size() * sizeof(int));
    return RTM_OK;
}

// rtm_debug_scene_facts: axis_pattern and fold_flags_of on the HOST, from the caller's spheres (tests/test_host_io.py)
int scene_facts_host(const rtm_sphere* sp, size_t n, uint64_t* facts) {
    if ((!sp && n) || !facts) return RTM_ERR_INVALID_ARGUMENT;
    std::vector<double> hg, hm;
    flatten_scene(sp, n, hg, hm);
    facts[0] = axis_pattern(hg.data(), n);
    facts[1] = fold_flags_of(hm.data(), n) | compact_flag_of(hg.data(), n);
    return RTM_OK;
}
// rtm_debug_zero_term_facts: zero_term_flags_of on the HOST — facts[0] 1 where kFoldZeroTermSkippable is proven, facts[1] the
// emit mask (tests/test_zero_term_host.py)
int zero_term_facts_host(const rtm_sphere* sp, size_t n, uint64_t* facts) {
    if ((!sp && n) || !facts) return RTM_ERR_INVALID_ARGUMENT;
    std::vector<double> hg, hm;
    flatten_scene(sp, n, hg, hm);
    facts[0] = zero_term_flags_of(hm.data(), n, &facts[1]) != 0u ? 1u : 0u;
    return RTM_OK;
}
// rtm_debug_axis_rows: axis_rows on the HOST, as a scene object of these spheres gets them (tests/test_axis_disc_host.py)
int axis_rows_host(const rtm_sphere* sp, size_t n, double* rows) {
    if ((!sp && n) || !rows || n > kAxisRowsMax) return RTM_ERR_INVALID_ARGUMENT;
    std::vector<double> hg, hm;
    flatten_scene(sp, n, hg, hm);
    axis_rows(hg.data(), n, axis_pattern(hg.data(), n), rows);
    return RTM_OK;
}
// rtm_debug_wall_pairs: wall_pairs_flag on the HOST (tests/test_wall_pairs_host.py)
int wall_pairs_host(const rtm_sphere* sp, size_t n, uint64_t* facts) {
    if ((!sp && n) || !facts || n > kAxisRowsMax) return RTM_ERR_INVALID_ARGUMENT;
    std::vector<double> hg, hm;
    flatten_scene(sp, n, hg, hm);
    unsigned lower = 0u;
    facts[0] = wall_pairs_flag(hg.data(), n, axis_pattern(hg.data(), n), &lower) != 0u ? 1u : 0u;
    facts[1] = lower;
    return RTM_OK;
}

GridLayout grid_layout(size_t n_cells, size_t n_recs, size_t n_big) {
    GridLayout L;
    L.off_cs = (sizeof(GridHeader) + 255) & ~(size_t)255;
    L.off_items = L.off_cs + ((n_cells * 2 * sizeof(unsigned) + 255) & ~(size_t)255);
    L.off_big = L.off_items + ((n_recs * 4 * sizeof(double) + 255) & ~(size_t)255);
    L.bytes = L.off_big + (n_big + 1) * sizeof(int);
    return L;
}

}  // namespace rtm
