/*
 * rtm_debug.h — test and diagnostic hooks exported by librtm_hip.so next to the C ABI of rtm.h.
 *
 * NOT part of the drop-in boundary: nothing here replaces a seam of the reference; they expose
 * building blocks of the device path (device math, the exhaustive self-checks, the large-scene
 * nearest-hit kernels, isolated loop timings) to tests/ and profiles/.  Host buffers throughout;
 * same status codes as rtm.h.  May change without an ABI version bump.
 */
#ifndef RTM_DEBUG_H
#define RTM_DEBUG_H

#include "rtm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device sqrt / sqrtf / division / sin / cos and the exact-fast forms on caller data; `op` as in
 * math_probe_kernel (csrc/rtm_seam_kernels.h); ops 32..47: the tolerance row's arithmetic — one-ulp square root, division and
 * reciprocal, a contracted multiply-add, its sin / cos, the unfused fold step; 45..47: the reference forms of 41..43; 48: of 32;
 * 49..51: a sphere's row of the normal table for r * r = a[i] (csrc/rtm_kernels_tol.hip).  Ops 39, 40, 42, 43, 46, 47 take a draw's
 * integer: a[i] must be an ODD integer below 2^24 (42 / 43 convert it to an integer, the others round it: other operands differ).
 * Ops 52 .. 54: the discriminant stage of the tolerance row's search for a sphere whose centre is on a coordinate axis, on
 * caller-given rays.  Records of 8 doubles, n a multiple of 8: a = (origin x, y, z, direction x, y, z, unused, unused),
 * b = (axis 1 / 2 / 3 for x / y / z, the centre's coordinate c on it, r * r, -2 c, K = c c - r * r, unused x 3; the last two as
 * rtm_debug_axis_rows returns them), out = (b, D4, 0 x 6) with t = b -+ sqrt(D4).  52: the form of rounds 4 to 8, p = c - o_a
 * with the shared sums of the foreign products (reads c and r * r) — the reference of 53; 53: the expanded form the search
 * runs, b = c d_a - o.d, D4 = b b - ((-2 c) o_a + o.o + K) (reads c, -2 c and K); 54: the same for a sphere of a signature's
 * shared-K group, D4 = b b - ((-2 c) o_a + (o.o + K)).  Any other axis value gives (0, 0).
 * Ops 55 / 56: the tolerance row's whole nearest-hit search of a seven-sphere scene with the Cornell box's signature (the light on
 * y, walls on +x, -x, +y, -y, +z, -z sharing one K) on caller-given rays.  a: records as above; b: the scene's table in its first
 * 56 doubles — 7 geometry rows (cx, cy, cz, r * r), then 7 axis rows as rtm_debug_axis_rows returns them —, n >= 56.  55: the search
 * with opposite wall pairs, out = (distance, hit id or -1, 1 where the ray's wave took the seven-sphere block instead, 0 x 5);
 * 56: the seven-sphere block, out = (distance, hit id or -1, 0 x 6).  A wave holds the 8 rays of 64 consecutive doubles.
 * Ops 57 / 58: the words a lane of the tolerance row's render loops leaves the Russian roulette with.  Records of 8 doubles, n a
 * multiple of 8, ONE LANE per record (lane i computes record i, so a wave holds 64 records and the caller decides which of its
 * lanes continue): a = (p0, p1 of a pixel key, ctr, k1 of a stream, the sample index n' to restart with, ended != 0, unused x 2),
 * the 32-bit words as doubles, b unused; the stream makes the roulette's draw first.  out = (the integer m of the bounce's first
 * draw, of its second, ctr, k1 of the stream the lane goes on with, 0 x 4): for a continuing lane its two draws and the stream
 * three draws on, for an ended lane (0, 0, the stream of sample n').  57: through the one mix32 pair both kinds of lane share
 * (csrc/rtm_device.h: rng_merged_mix); 58: through rng_next_mi, rng_next and rng_open — the reference of 57.
 * Ops 59 / 60: a bounce direction of the tolerance row's shading block BEFORE its final Normalize (src/Renderer.cpp:96-107).
 * Records and lanes as for 57 / 58: a = (w.x, w.y, w.z of the turned normal, the odd integers m1 and m2 < 2^24 of the bounce's
 * two draws — the angle 2 pi m1 2^-24 and r2 = m2 2^-24 —, unused x 3), b unused, out = (nd.x, nd.y, nd.z, 1 where the lane set
 * the block's `bad` flag, 0 x 4).  No component of w may be zero (such a lane is another branch's in the render loops).
 * 59: from one reciprocal root, k = sqrt(r2) / y, without the orthonormal basis (csrc/rtm_path.h: bounce_nd_fused), as the block
 * runs it; 60: with the basis built, a refined reciprocal and a root (bounce_nd_basis) — the reference of 59.
 * Ops 61 / 62: op 55's search on op 55's records (a, b, n and the waves as there), out = (distance, hit id or -1, 1 where the
 * ray's wave took the acceptance's general chain, 1 where it took the seven-sphere block instead of the pairs, 1 where it asked
 * the far-root question a second time, 0 x 3).  61: as the render kernels run it, no far-root sum for a pair's wall
 * (csrc/rtm_path.h: accept_batch_lane's WALLS); 62: the sum formed for every candidate — the reference of 61. */
int rtm_debug_math_probe(int op, const double* a, const double* b, size_t n, double* out);
/* The tolerance row's sin / cos table as the HOST builds it for every device (no device is touched; runs in the CPU test
 * suite): out[2 i], out[2 i + 1] = sin, cos of i 2 pi / entries, evaluated in long double and rounded to double once.  The
 * row itself uses entries = 16384 (ops 42 / 43 of rtm_debug_math_probe run its sequence; 44: the shading block's unit root). */
int rtm_debug_trig_table(int entries, double* out);
/* exhaustive device self-checks; *mismatches = number of failing inputs (kind 0: fast sqrtf) */
int rtm_debug_selfcheck(int kind, unsigned long long* mismatches);
/* nearest hit for caller-given rays: kind 1 the reference's loop as written (src/Renderer.cpp:58-73, the compiler's
 * math, nothing in front of it), kind 3 the large-scene kernel (packed-fp32 rejection test + per-lane candidate lists
 * in front of the same arithmetic); any other kind is RTM_ERR_INVALID_ARGUMENT */
int rtm_debug_wf_nearest(int kind, const rtm_sphere* spheres, size_t n, const double* org, const double* dir,
                         size_t n_rays, int32_t* out_id, double* out_t);
/* the fp64 vector peak of the current device by wall clock: a chip-filling v_fma_f64 kernel (`waves_per_simd` waves on
 * every SIMD, 8 independent accumulators per lane) timed with HIP events over a launch of at least `min_ms`;
 * *tflops counts an FMA as 2 flops.  bench.py puts it beside the datasheet figure ("verify by
 * microbenchmark"); profiles/ubench/fp64_peak.hip is the stand-alone form with the per-instruction price list. */
int rtm_debug_fp64_peak(int waves_per_simd, double min_ms, double* tflops, double* kernel_ms);
/* The uniform-grid nearest-hit search of variant 17 (csrc/rtm_path.h: nearest_hit_grid) on caller-supplied rays
 * (org, dir: n_rays x 3 doubles, HOST): hit object (-1: none) and distance per ray as the reference loop
 * (src/Renderer.cpp:58-73) finds them — kind 1 of rtm_debug_wf_nearest is that loop — plus, where the pointers are not
 * NULL, the sphere tests and cell steps each ray took and info[6] = {cells, cell-list entries, spheres tested by every
 * ray, dim x, dim y, dim z}.  RTM_ERR_UNSUPPORTED when the scene gets no grid. */
int rtm_debug_grid_nearest(const rtm_sphere* spheres, size_t n, const double* org, const double* dir, size_t n_rays,
                           int32_t* out_id, double* out_t, uint32_t* out_tests, uint32_t* out_steps, uint64_t* info);
/* The grid's builder alone, on the HOST (no device is touched; runs in the CPU test suite): info[12] = {cells, list
 * entries, spheres tested by every ray, dim x, y, z} followed by the bit patterns of six doubles {box lo x, y, z, cell edge,
 * reach of origins from the box's centre, largest hit parameter the pads cover}; pads[n]: every sphere's pad; and, where the
 * pointers are not NULL, ranges[2 x cells] (first, one past last entry of each cell's list; x fastest), items[entries]
 * (sphere indices, ascending within a cell) and big[...].  RTM_ERR_UNSUPPORTED: no grid; RTM_ERR_CAPACITY: a buffer is short
 * (info is filled: call once without buffers for the sizes). */
int rtm_debug_grid_build(const rtm_sphere* spheres, size_t n, uint64_t* info, double* pads, uint32_t* ranges, size_t ranges_cap,
                         uint32_t* items, size_t items_cap, int32_t* big, size_t big_cap);
/* A scene object's grid as the DEVICE holds it, read back in rtm_debug_grid_build's format — for a scene built by
 * rtm_scene_create (host builder, uploaded) as for one built by rtm_scene_create_device (device kernels): info[12] as above;
 * ranges[2 x cells]; items[entries] = the low 29 bits of each record's fourth double (the sphere's index); big[...];
 * extra[0] = the number of records (the one dummy record of a grid without entries included) whose four doubles are not the
 * scene's geometry row of that index with the index OR-ed into the fourth, extra[1] = 1 where a diffuse sphere encloses the
 * gridded ones from beyond the pads' reach (variant 0 then leaves the grid alone).  Any buffer and `extra` may be NULL.
 * RTM_ERR_UNSUPPORTED: the scene has no grid; RTM_ERR_CAPACITY: a buffer is short (info and extra[1] are filled).  Waits for
 * the scene's device. */
int rtm_debug_scene_grid(const rtm_scene* scene, uint64_t* info, uint32_t* ranges, size_t ranges_cap, uint32_t* items,
                         size_t items_cap, int32_t* big, size_t big_cap, uint64_t extra[2]);
/* rtm_scene_nearest's (any = 0) or rtm_scene_occluded's (any = 1) search of a scene that has a grid, through the grid walk's
 * counting instantiation (csrc/rtm_path.h: GridWalk's COUNT): the sphere tests and the cell steps each ray took, so that a test
 * can see the occlusion walk's early exit.  DEVICE buffers and the contract of those calls: only enqueues on `stream`, same
 * refusals (every output null counts as one).  Outputs, each n_rays long and nullable: any = 0: object and t as
 * rtm_scene_nearest writes them, occluded = t < tmax as rtm_scene_occluded defines it; any = 1: occluded as
 * rtm_scene_occluded writes it, object and t = the hit that decided it (not necessarily the nearest; -1 and +infinity where
 * nothing occludes).  RTM_ERR_UNSUPPORTED: the scene has no grid. */
int rtm_debug_scene_query(const rtm_scene* scene, int any, const double* org_dev, const double* dir_dev, const double* tmax_dev,
                          size_t n_rays, int32_t* out_object_dev, double* out_t_dev, uint8_t* out_occluded_dev,
                          uint32_t* out_tests_dev, uint32_t* out_steps_dev, void* stream);
/* What the host finds in a sphere array when it flattens it into the kernels' tables, on the HOST (no device is touched; runs in
 * the CPU test suite): facts[0] = two bits per sphere for the first 32 — 1 / 2 / 3: the centre's only coordinate that is not
 * +-0 is x / y / z (the axis-signature instantiations of the exact-n kernels, csrc/rtm_path.h: sphere_disc) —, facts[1] bit 0:
 * every object a path can bounce off (kd > 0) emits (+0, +0, +0) and no colorKD or emission carries a sign bit (the packed
 * folds then leave a bounce level's "+ emission" out: SceneView::fold_flags), bit 1: every |centre| + radius is at most 1e7 (a
 * compact scene: the tolerance row's search may take its square roots without the residual step). */
int rtm_debug_scene_facts(const rtm_sphere* spheres, size_t n, uint64_t facts[2]);
/* Two more such facts, also on the HOST (rtm_debug_scene_facts' two words are compared whole by its callers, so these have an
 * entry of their own): facts[0] = 1 where a path end whose terminal object does not emit provably adds (+0, +0, +0) — bit 0 of
 * rtm_debug_scene_facts' facts[1] holds, every colorKD of an object a path can bounce off is finite and there are at most 63
 * objects —, so that the deferred-fold kernels neither queue nor fold nor store it (SceneView::emit_mask), else 0; facts[1] =
 * the mask those kernels get: bit i = object i's emission is not (+0, +0, +0), all ones where facts[0] is 0.  (RTM_DEBUG_ZERO_SKIP=0
 * in the environment of a render call makes it queue and fold every path end whatever these facts say.) */
int rtm_debug_zero_term_facts(const rtm_sphere* spheres, size_t n, uint64_t facts[2]);
/* The axis rows a scene object of these spheres keeps behind its geometry rows for the tolerance row's search, on the HOST (no
 * device is touched; n <= 32): rows[4 i .. 4 i + 3] = (c, -2 c, K, e) for a sphere that rtm_debug_scene_facts gives an axis, c its
 * centre's coordinate on that axis and K = c c - r * r from the float product r * r as the geometry row stores it, formed in
 * long double (one fused operation) and rounded to double; zeros for any other sphere.  e, the same in every axis row and not
 * read by the kernels: the reach 2^k within which the host has proven the expanded form safe for this scene — no axis sphere can
 * hit itself, distances stay a sixteenth under the smallest threshold, every sphere lies within it (csrc/rtm_path.h:
 * kSceneAxisReachShift) —, 0 where it has not: such a scene, or a camera beyond the reach, takes the plain kernels. */
int rtm_debug_axis_rows(const rtm_sphere* spheres, size_t n, double* rows);
/* Whether a scene object of these spheres gets the tolerance row's opposite-wall-pair search (one root and one acceptance per
 * pair, csrc/rtm_path.h: kAxisPairsBit), on the HOST (no device is touched; n <= 32): facts[0] = 1 where the members of the
 * shared-K group are, two by two in index order, spheres of one radius on one axis at +c and -c bit for bit, the scene is
 * compact and inside the expanded form's envelope, and the proof's constants hold (gamma / (2 beta) + reach 2^-44 < 1e-5f / 2,
 * r 2^-17 >= 2 beta; beta = 2^-5, gamma = 2^-25), else 0; facts[1]: bit i = sphere i is the lower member of a pair that passes
 * the per-pair tests.  (Ops 55 / 56 of rtm_debug_math_probe run that search and the seven-sphere block it replaces on caller
 * rays: csrc/rtm_kernels_tol.hip.) */
int rtm_debug_wall_pairs(const rtm_sphere* spheres, size_t n, uint64_t facts[2]);
/* The dynamic LDS bytes of a tolerance-row launch for a scene of n spheres (1 .. 24), on the HOST (no device is touched;
 * csrc/rtm_render_kernel.h: render_lds_bytes): any_depth 0 the depth-capped shape, 1 the any-depth one; split: with the sample
 * split; rows 1: the scene tables with one 64-byte row per sphere (SceneLdsRows: the axis-signature kernels), 0: three tables.
 * out[0] = bytes per workgroup (one wave), out[1] = 1 where they include the near-unit Normalize table. */
int rtm_debug_tol_lds_bytes(int n, int any_depth, int split, int rows, uint64_t out[2]);
/* isolated nearest-hit / shading loops timed with s_memtime (profiles/component_bench.py) */
int rtm_debug_component_bench(int which, const rtm_sphere* spheres, size_t n, int reps, int blocks, int lds_pad,
                              double* cycles_per_rep);
/* One form of rtm_denoise_variance's variance kernel alone (profiles/denoise_variance_pass.py, and the tests that hold the
 * forms against each other): form 0 takes every tap from L2, 1 / 2 stage a tile of 64 x 4 / 64 x 8 pixels and its halo in
 * LDS; the call ships one of them.  DEVICE buffers, unlike the hooks above: work_dev holds the records that a
 * rtm_denoise_variance call with K = 0 and a variance output left there for the same frame, guides and sigmas (only the
 * null-ness of the guide pointers is read); variance_out_dev receives v0.  Only enqueues on `stream`. */
int rtm_debug_denoise_variance_kernel(int form, const rtm_denoise_var_params* params, int32_t width, int32_t height, int device,
                                      const rtm_aov_buffers* guide_dev, void* work_dev, float* variance_out_dev, void* stream);
/* rtm_defocus with one form of its kernel (profiles/defocus_pass.py, and the test that holds the forms against each other):
 * form 0 is the call as shipped, form 1 runs every block over all (2R+1)^2 taps, without the per-tile window bound and the
 * pass-through of sharp tiles.  Arguments, refusals and bits are rtm_defocus's.  Only enqueues on `stream`. */
int rtm_debug_defocus_form(int form, const rtm_defocus_params* params, int32_t width, int32_t height, int device,
                           const float* color_dev, const float* depth_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                           float* coc_out_dev, void* stream);
/* rtm_render_mattes' ranking alone (csrc/rtm_matte_kernel.h: matte_rank) on caller-given id lists, so that ties, truncation
 * and lists of 64 distinct ids can be pinned without rays.  DEVICE buffers: ids_dev holds n_pixels lists of SS^2 ids each
 * (pixel-major), any negative id is a miss; a small kernel loads 64 pixels' lists into the render kernel's LDS layout and calls
 * the same function.  Outputs are planar, layers x n_pixels (id, coverage) and n_pixels (alpha); each may be null, not all.
 * Only enqueues on `stream`; n_pixels == 0 enqueues nothing.  layers outside 1..8, a non-positive super_samples, null ids_dev,
 * every output null, a misaligned pointer, a negative device: RTM_ERR_INVALID_ARGUMENT; super_samples > 8:
 * RTM_ERR_UNSUPPORTED; both before any device call. */
int rtm_debug_matte_rank(int32_t super_samples, int32_t layers, int device, const int32_t* ids_dev, size_t n_pixels,
                         int32_t* id_out_dev, float* coverage_out_dev, float* alpha_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTM_DEBUG_H */
