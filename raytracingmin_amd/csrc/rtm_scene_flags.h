// rtm_scene_flags.h — the facts a host proves about a scene and the kernels' launchers read: SceneView::fold_flags' bits,
// the constants of the proofs behind them, the limits of the axis rows and of the grid builder.  Plain C++, nothing of HIP:
// included by rtm_path.h (the kernels, in both of its namespaces) and by rtm_scene_facts.cpp (the proofs, host only).
#pragma once
#include <stddef.h>

// (rtm_device.h: the kernel headers are compiled into namespace rtm and, by the tolerance unit, into rtm_tol)
#ifndef RTM_NS
#define RTM_NS rtm
#endif

namespace RTM_NS {

// SceneView::fold_flags (rtm_path.h), bit 0: see SceneView::fold_flags
constexpr unsigned kFoldNoLevelEmission = 1u;
// ... bit 2, kFoldZeroTermSkippable: kFoldNoLevelEmission holds, every colorKD of an object a path can bounce off is finite
// (no 0 x inf) and the scene has at most 63 objects (SceneView::emit_mask has a bit for each)
constexpr unsigned kFoldZeroTermSkippable = 4u;
// ... and bit 1, kSceneCompact: every |centre| + radius is finite and at most 1e7 (the launcher adds the camera): what the
// tolerance unit's light search roots ask for (seq_sqrt_batch)
constexpr unsigned kSceneCompact = 2u;
// ... and bits 8..15 (set by the host where it holds the geometry, else 0): the spheres among the first 8 that form the largest
// group of axis spheres whose axis rows hold ONE K = c c - r*r, bit for bit — at least two, the lowest group on a tie; the six
// walls of the Cornell box: 0x7E.  The tolerance unit's launcher extends the axis signature with it (kAxisSharedKShift).
constexpr unsigned kSceneSharedKShift = 8u, kSceneSharedKMask = 0xFFu;
// ... and bits 16..23 (likewise): the ENVELOPE of the tolerance unit's expanded axis discriminant (sphere_disc), 0 = not proven,
// else 128 + k: every axis sphere passes the two tests below for origins within 2^k of the scene's origin, and every sphere
// of the scene lies within that reach (the launcher adds the camera).  The expanded q = (-2 c) o_a + o.o + K sums three terms
// of up to (|c| + r)^2 or |o|^2 where the form of rounds 4 to 8 squared the EXACT difference c - o_a: its rounding error is
// bounded by err(o) = 2^-49 max(|c| + r, |o|)^2 (three roundings of partial sums below 4 max^2), not by a multiple of r^2.
//   (A) a bounce ray leaving sphere i (|o| <= |c| + r) has q = 0 in real arithmetic and the far root t2 = err / (2 r cos theta)
//       with it; it must stay under Intersect's 1e-5f down to cos theta = 2^-17 (a cosine-weighted bounce is flatter than that
//       once in 2^34): err(|c| + r) / (2 r) <= 2^-17 x 1e-5f.  A Cornell wall: 3.6e-11 against 7.6e-11; a sphere of radius 100
//       at 1e6 fails by seven orders and WOULD hit itself (tests/test_axis_disc_host.py shows it in numpy).
//   (B) from any origin within the reach a distance to sphere i is off by err(reach) / (2 r) at normal incidence: at most a
//       sixteenth of 1e-5f, the smallest threshold a distance is compared with.
// A scene outside the envelope takes the plain exact-n kernels (p_o formed as the reference does).
constexpr unsigned kSceneAxisReachShift = 16u, kSceneAxisReachMask = 0xFFu;
constexpr double kCompactExtent = 1e7;

// ... and bit 24, kSceneWallPairs (the host's proof, rtm_scene_facts.cpp: wall_pairs_flag; rtm_path.h: kAxisPairsBit)
constexpr unsigned kSceneWallPairs = 1u << 24;  // SceneView::fold_flags
// The proof.  The wall a ray does NOT head for has b_u = -|c| |d_a| - o.d and
// q_u = 2 |c| (o_a sgn d_a) + o.o + K, the very numbers sphere_disc forms for it.  Where b_u <= -beta and q_u >= 2 tau b_u
// (tau = gamma / (2 beta) = 2^-21; b_u is negative, so this admits a q_u down to -2 tau |b_u|) its near root b_u - s is negative
// and its far root b_u + s = -q_u / (|b_u| + s) is at most tau = 4.8e-7, plus the light root's 2^-44 |b_u|: under half of
// Intersect's 1e-5f within any reach the host admits (gamma / (2 beta) + reach 2^-44 < 1e-5f / 2), so nothing of that wall can be
// accepted.  The bound on q_u scales with |b_u| because a bounce ray's q for the wall it LEAVES is not 0 but t^2 (d.d - 1), up to
// 2e-4 either way — the direction's length comes from a float root, 1.2e-7 off —: a constant -gamma would fail half of all bounce
// rays, -2 tau |b_u| = -2 tau r cos fails the ones flatter than cos = 2e-3.  beta keeps b_u's own rounding out of it and is
// small enough for every bounce ray down to cos = 2^-17 (the host asks r 2^-17 >= 2 beta of a paired sphere).  NaN operands
// compare false: not proven.
constexpr double kPairBeta = 0.03125, kPairGamma = 2.98023223876953125e-8;  // 2^-5, 2^-25
constexpr double kPairTau = kPairGamma / (2.0 * kPairBeta);                    // 2^-21

// the axis rows (rtm_scene_facts.cpp: axis_rows): a scene of more spheres has none
constexpr size_t kAxisRowsMax = 32;

// the uniform grid of a large scene (rtm_scene_facts.cpp: make_grid; rtm_grid_build.hip: the same on the device)
constexpr size_t kGridMinSpheres = 64;  // gridded spheres a scene needs to get a grid (profiles/r3/grid_crossover.txt)
constexpr int kGridMaxBig = 1024, kGridMaxDim = 1024;  // (kGridBigCells, kGridDdTol: rtm_grid_exprs.h, with the per-sphere expressions)

}  // namespace RTM_NS
