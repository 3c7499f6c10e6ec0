/*
 * rtm.h — C ABI of the MI355X-native path-tracing hot path for RaytracingMin scenes.
 *
 * This is the drop-in boundary.  The reference has no FFI; the seams this ABI
 * replaces are (paths relative to the reference checkout):
 *
 *   png::Renderer::Renderer(SettingData&)              src/Renderer.h:11, src/Renderer.cpp:20-23
 *   void png::Renderer::Render(std::string fileName)   src/Renderer.h:13, src/Renderer.cpp:200-258
 *   png::vec3 png::PathTracing(Ray, SettingData&, fn)  src/Renderer.cpp:57-117
 *   bool png::SphereObject::Intersect(...)             src/SettingData.cpp:197-226
 *   png::LoadData::LoadData(std::string)               src/SettingData.cpp:6-12,129-186
 *   stbi_write_bmp / stbi_write_jpg call sites         src/Renderer.cpp:251-257
 *
 * Conventions: plain C types only; the caller owns every buffer; nothing allocated inside is
 * handed out; every entry point returns RTM_OK (0) or a negative rtm_status, never throws.
 * "Device" pointers are HIP device pointers on the GPU selected in rtm_options.device; streams are
 * hipStream_t passed as void*.
 *
 * Threading: every entry point may be called from any host thread.  Renders on DIFFERENT
 * (device, stream) pairs run concurrently and share nothing; calls that name the SAME (device, stream)
 * are serialised by the library for the time it takes to enqueue them (the work itself is ordered by
 * the stream), so the work buffers the library keeps per (device, stream) are never handed to two
 * calls at once.  rtm_release_scratch waits for the renders it affects.  rtm_last_error_detail is
 * per thread.  Diagnostic hooks (rtm_debug_*) are declared in rtm_debug.h, not here.
 */
#ifndef RTM_H
#define RTM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTM_ABI_VERSION 5

typedef enum rtm_status {
    RTM_OK = 0,
    RTM_ERR_INVALID_ARGUMENT = -1, /* null pointer, non-positive size, bad enum value          */
    RTM_ERR_INVALID_SCENE = -2,    /* unsupported objectType, malformed numbers                 */
    RTM_ERR_IO = -3,               /* file cannot be opened / written                           */
    RTM_ERR_PARSE = -4,            /* JSON syntax or type error (reference: nlohmann exception) */
    RTM_ERR_NO_DEVICE = -5,        /* no HIP device / HIP runtime failure at init               */
    RTM_ERR_HIP = -6,              /* a HIP call failed; see rtm_last_error_detail()            */
    RTM_ERR_CAPACITY = -7,         /* caller buffer too small                                   */
    RTM_ERR_UNSUPPORTED = -8       /* valid request this build cannot serve                     */
} rtm_status;

/* png::Camera — src/SettingData.h:43-46.  fov is a float and is a tangent scale, not degrees
 * (src/Renderer.cpp:207-208). */
typedef struct rtm_camera {
    double origin[3];
    double target[3];
    double up[3];
    float fov;
    float _pad;
} rtm_camera;

/* png::SphereObject + png::Material flattened — src/SettingData.h:8-17,25-32.
 * radius is a float exactly like SphereObject::m_size. */
typedef struct rtm_sphere {
    double center[3];
    double color[3];
    double emission[3];
    float radius;
    float _pad;
} rtm_sphere;

/* Any object of png::SettingData::object — src/SettingData.h:18-42 — for scenes that are not all spheres.
 * type 1: png::SphereObject (position = centre, size = radius as a float, like m_size).
 * type 2: png::PlaneObject(position, up, target, width, mat) — src/SettingData.cpp:235-242.  The reference
 *   constructs m_normal = Normalize(target - position) and m_right = Normalize(Cross(m_normal, up)) * 0.5 * width
 *   but leaves Intersect unfinished (it falls off its end, :243-246) and never builds one (the loader only
 *   knows type 1).  This build completes it as the finite square the constructor describes — centre
 *   `position`, side `width`, spanned by m_right and Cross(m_right, m_normal):
 *       dn = Dot(m_normal, dir);           if |dn| < FLT_EPSILON: no hit            (the reference's own line, :244)
 *       t  = Dot(m_normal, position - org) / dn;      if !(t > 0.001): no hit       (the sphere's near threshold)
 *       d  = org + dir * t - position;     if |Dot(d, m_right)| > Dot(m_right, m_right)
 *                                          or |Dot(d, m_upv)|   > Dot(m_upv, m_upv): no hit
 *       out_dis = t; out_normal = m_normal  (the caller orients it against the ray, src/Renderer.cpp:82-83)
 *   A BUILD-DEFINED semantics: the reference has none to match; oracle and device agree bit for bit. */
enum { RTM_OBJECT_SPHERE = 1, RTM_OBJECT_PLANE = 2 };
typedef struct rtm_object {
    int32_t type;        /* RTM_OBJECT_*                                                       */
    float size;          /* sphere radius (float, SphereObject::m_size); unused for planes     */
    double position[3];  /* sphere centre / plane centre                                        */
    double color[3];
    double emission[3];
    double up[3];        /* plane only                                                          */
    double target[3];    /* plane only: the normal points from position towards target          */
    double width;        /* plane only: side of the square (a double, like the constructor's)   */
} rtm_object;

/* png::SettingData minus the object vector — src/SettingData.h:47-51. */
typedef struct rtm_settings {
    int32_t width, height, samples, super_samples;
    rtm_camera camera;
} rtm_settings;

enum { RTM_MODE_LITERAL = 0,  /* L0: HEAD as shipped (normal lost, recursion gets ::rand)       */
       RTM_MODE_REPAIRED = 1, /* L1: the three one-line defects fixed    */
       /* flag, OR-ed into mode: sin/cos of src/Renderer.cpp:93-94 return exactly what the HOST's
        * libm returns.  The argument takes 2^23 values, so on first use the library evaluates them
        * all on both sides (a fraction of a second, once per device) and keeps the one-ulp
        * differences in a 4 MB table.  Costs ~2 % of a frame; makes GPU and CPU-libm renders agree
        * bit for bit even where one-ulp differences are amplified over many bounces.            */
       RTM_MODE_HOST_TRIG = 0x100,
       /* flag, OR-ed into mode (diagnostic): a render WITH rtm_stats also counts the Intersect evaluations it makes
        * (rtm_stats.object_tests).  The exhaustive kernels make n_objects per cast by construction; the uniform-grid kernel
        * (variant 17) runs a counting instantiation that is a few per cent slower, so time a frame without the flag.     */
       RTM_MODE_COUNT_TESTS = 0x200,
       /* flag, OR-ed into mode: the INTEGRATOR is png::SurfaeSample (src/Renderer.cpp:119-198 with
        * SphereObject::ComputeSurfacePoint, src/SettingData.cpp:227-233) instead of png::PathTracing — the branch
        * src/Renderer.cpp:234-236 takes when a U[0,1) draw is >= 1.0, i.e. never in the reference; the function is defined,
        * has external linkage and takes the same injectable generator, so it is restated (oracle first) and served by a
        * general per-object kernel, not by the tuned ones.  max_bounces >= 0: an invocation at depth > max_bounces returns
        * 0 without drawing (the reference has no bound); records for up to 16 + 960 levels, beyond which the call fails
        * with RTM_ERR_UNSUPPORTED like a PathTracing render does. */
       RTM_MODE_SURFACE_SAMPLE = 0x400 };

typedef struct rtm_options {
    int32_t mode;         /* RTM_MODE_*                                                        */
    int32_t max_bounces;  /* <0: unlimited (reference recursion); k>=0: cast k+1 returns
                             emission on hit without drawing (build extension)     */
    uint64_t seed;        /* RNG seed (build-defined counter RNG, rtm_rng_u01 below)           */
    int32_t row_begin;    /* first image row of this tile                                      */
    int32_t row_end;      /* one past the last row; full image = [0, height)                   */
    int32_t device;       /* HIP device ordinal                                                */
    int32_t variant;      /* kernel variant, 0 = default (see rtm_variant_name)                */
    int32_t band_count;   /* interleaved bands for multi-GPU load balance: when > 1 the call
                             renders only the 8-row bands b = band_index, band_index + band_count,
                             ... of [row_begin,row_end) (band b = rows row_begin + 8b ..) and
                             stores them back to back; 0 or 1 = every band                     */
    int32_t band_index;   /* 0 <= band_index < band_count                                       */
} rtm_options;

/* Per-render counters (sum over the rendered tile); filled when the pointer is non-null. */
typedef struct rtm_stats {
    uint64_t samples;     /* primary samples traced = output rows*width*SS*SS*S                */
    uint64_t casts;       /* PathTracing invocations (ray casts)                               */
    uint64_t bounces;     /* casts that continued (RR passed)                                  */
    uint64_t draws;       /* RNG draws consumed                                                */
    double kernel_ms;     /* device time of the render kernel(s), HIP events on the stream     */
    int32_t variant;      /* the kernel variant that ran (rtm_options.variant resolved; see
                             rtm_variant_name), and                                              */
    int32_t split;        /* waves per 8x8 tile of the sample split (1 = not split)            */
    uint64_t object_tests; /* Object::Intersect evaluations (src/Renderer.cpp:66): casts x n_objects for the
                             exhaustive kernels; for the uniform-grid kernel the count of RTM_MODE_COUNT_TESTS, else 0 */
} rtm_stats;

/* A scene flattened to the kernels' layout and resident on one device (opaque).  Created once,
 * used by any number of renders on any stream of that device, destroyed by the caller after the
 * last render that uses it has been ENQUEUED: rtm_scene_destroy does not wait for that work.  When the
 * renders that named the scene have all finished, its device memory is freed in the call; otherwise the
 * scene is parked and freed by a later library call (any render, create or destroy) that finds them
 * finished, or by rtm_release_scratch, which waits.  Other streams of the device are never waited for. */
typedef struct rtm_scene rtm_scene;

/* ---- library ---- */
int rtm_abi_version(void);
const char* rtm_strerror(int status);
const char* rtm_last_error_detail(void);   /* thread-local text of the last failure            */
int rtm_device_count(int* count);          /* RTM_ERR_NO_DEVICE if the HIP runtime has none    */
int rtm_num_variants(void);
const char* rtm_variant_name(int variant);

/* Rows a call with these options renders and stores (row_end - row_begin unless banded). */
int rtm_output_rows(const rtm_options* options);
/* The library keeps its large work buffers (per device and stream, grown on demand), the scene cache
 * of rtm_render_device and the RTM_MODE_HOST_TRIG tables between calls; this frees them for one
 * device, or for all with device < 0.  Waits for the device to go idle.  Scenes made by
 * rtm_scene_create are the caller's and stay.
 * What "large" means: the sample split of a launch's last tiles keeps 2 KiB per (split tile, deferred sample) —
 * 1.6 GB for the headline frame, capped at 24 GiB per stream (a launch whose terms would not fit splits fewer
 * tiles, or none), and in-wave sample stealing 1.8 KiB x (2 sqrt(spp) + 5) per whole tile (3.8 GB for the headline
 * frame; without room the launch runs without it); unlimited-depth renders keep two pooled record stacks per lane
 * (5.5 GB for a 1080p frame); the large-scene grid kernel 32 B per sample of a launch (17.0 GB for a 1080p frame at
 * 256 spp: above the 16 GiB budget, so that frame is rendered in two launches — beyond the budget, or what the device
 * gives, a frame is cut into several launches of as many tiles as fit); the exhaustive
 * large-scene pipeline ~300 B per pixel plus 4 B per pixel and record level. */
int rtm_release_scratch(int device);
/* What a render with these arguments will ask of those work buffers, in bytes, before anything is allocated:
 * out_bytes[0] the total, [1] per-sample terms (sample split of a launch's last tiles / the grid kernel's term buffer:
 * one launch's worth, at most the 16 GiB budget), [2] pooled hit records (unlimited depth or a cap of 16 and more),
 * [3] the exhaustive large-scene pipeline's path state, [4] the rows of in-wave sample stealing, [5] the table of primary
 * directions a pre-pass leaves for the default kernels (1.5 KiB per tile and sub-pixel, at most 4 GiB).  The buffers are per
 * (device, stream), grown on demand and kept until rtm_release_scratch / rtm_stream_release; a stream that has rendered
 * larger frames already holds more.  Where the device cannot give an OPTIONAL buffer (terms, stolen rows) the render
 * runs without the feature or in more launches — same image.  The figure for a whole frame is an upper bound for any pass of it
 * (rtm_render_scene_samples). */
int rtm_scratch_bytes(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                      uint64_t out_bytes[6]);
/* The same for ONE stream: waits for that stream's queued work (and, like rtm_release_scratch, for every render call
 * that is being enqueued at that moment), frees the buffers and the sticky status word the
 * library keeps for (device, stream) and forgets the pair.  Call it before destroying a stream that has rendered
 * (a later stream may be given the same handle and would inherit the context otherwise).  An overflow that was
 * never reported is returned here (RTM_ERR_UNSUPPORTED), like rtm_stream_status would. */
int rtm_stream_release(int device, void* stream);

/* ---- scene lifetime: png::SettingData::object (src/SettingData.h:47-51) on the device ----
 * rtm_scene_create flattens `spheres` (HOST pointer, or a DEVICE pointer on `device` when
 * spheres_on_device != 0) and uploads the tables; it returns when they are resident, so the caller's
 * array may be freed at once.  A scene belongs to one device.
 * For an all-sphere scene of 64 spheres or more (not counting those that span the scene, like the Cornell walls) the
 * call also builds, on the host (~25 ms per 100 000 spheres plus the upload; rtm_scene_create_device builds the same grid on
 * the device), a uniform grid over the spheres (~32 B x 6 per sphere +
 * 8 B per cell, ~2 cells per sphere): renders then find the reference loop's nearest hit (src/Renderer.cpp:58-73:
 * same object, same distance, same image) through the grid instead of testing every sphere for every cast
 * (rtm_options.variant 17; variant 0 picks it when the camera is within about two scene diagonals of the scene and no
 * diffuse sphere encloses the scene from farther away than that — its bounces would start where the grid cannot serve them;
 * variants 3 / 14 and, from 512 spheres, 12 are the exhaustive kernels). */
int rtm_scene_create(const rtm_sphere* spheres, size_t n_spheres, int spheres_on_device, int device,
                     rtm_scene** out_scene);
/* The same for a list of objects of any type (spheres and planes in the reference's vector order, which
 * decides ties: the lowest index wins).  Scenes that contain a plane are rendered by the default chunked kernel
 * up to 255 objects (rtm_options.variant 0, 2 or 9) and by the general per-object kernel beyond (variant 1, which
 * may also be asked for); the other variants know spheres only and refuse them.  HOST pointer. */
int rtm_scene_create_objects(const rtm_object* objects, size_t n_objects, int device, rtm_scene** out_scene);
/* A scene from a DEVICE sphere array, built entirely on the device: for spheres that are produced there (a tensor, a particle
 * step, an animation of a large scene).  The result is what rtm_scene_create(spheres_dev, n_spheres, 1, device, &s) returns for
 * the same array in every observable way — the grid is the host builder's bit for bit (the same cells, lists in the same
 * order, the same spheres tested by every ray), so renders, AOVs and mattes, their counters, variant 0's choice, the decision
 * about an enclosing diffuse sphere, rtm_scene_size and every "no grid" outcome are the same — and differs in three:
 *   - All device work is enqueued on `stream` (rtm_scene_create uses the device's null stream), so it is ordered after
 *     whatever produced the array there.  The call returns once the tables are resident, after waiting for `stream`; the
 *     array may be overwritten or freed at once.  Temporaries come from and return to the device's memory pool on `stream`.
 *   - Per-sphere data never travels to the host (rtm_scene_create on a device array brings every geometry and material row
 *     back for the host's grid builder and uploads the grid).  What crosses: 120 bytes down and two doubles up per
 *     classification round (at most five), the cell-list entry count, the indices and rows of the spheres every ray tests
 *     (at most 1024 of 44 bytes), the header up; and, for n_spheres <= 32, the rows the small-scene facts are read from, as
 *     in rtm_scene_create.
 *   - The arguments are checked before any device call: a null out_scene, null spheres_dev with n_spheres > 0, n_spheres >
 *     0x7FFFFFFF or a negative device give RTM_ERR_INVALID_ARGUMENT.
 * rtm_scene_destroy, its deferred release and the use records work as for any scene.
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbol up. */
int rtm_scene_create_device(const rtm_sphere* spheres_dev, size_t n_spheres, int device, void* stream,
                            rtm_scene** out_scene);
int rtm_scene_destroy(rtm_scene* scene);
size_t rtm_scene_size(const rtm_scene* scene);

/* ---- ray queries on a scene: "what does this ray hit?" and "is this segment blocked?" for rays of the caller's ----
 * Rays live on the scene's device: org_dev and dir_dev hold n_rays x 3 doubles, a row per ray (rtm_path_trace_batch's layout;
 * a contiguous (n, 3) float64 tensor).
 * rtm_scene_nearest: for ray i, object and t are exactly what the loop of src/Renderer.cpp:58-73 leaves in hitObject and dis
 * over the scene's objects in index order — Intersect in the reference's arithmetic (src/SettingData.cpp:197-226; the
 * build-defined square for a plane), accepted when tmp_dis < dis && tmp_dis > 0, so the lowest index wins ties — bit for bit,
 * for every ray: directions of any length, origins anywhere; a ray with a non-finite component hits nothing.  normal is what
 * Intersect reports for the winning object in RTM_MODE_REPAIRED: Normalize((org + dir t) - centre) with the reference's
 * float-length Normalize for a sphere, m_normal for a plane.  It is NOT turned towards the ray, and there is no mode argument.
 * rtm_scene_occluded: out[i] = 1 exactly when that t satisfies t < tmax[i] (strictly; a miss never does), else 0.  A tmax that
 * is NaN, zero or negative is never occluded; a null tmax_dev stands for +infinity everywhere: any hit occludes.  An object's
 * accepted t does not depend on the other objects, so this is "some object's Intersect reports a hit with 0 < t < tmax", and
 * where the scene has a grid the search stops at the first such hit instead of looking for the nearest.
 * The scene has no other effect on the answers: one with a grid, one without, one built by rtm_scene_create_device give the
 * same bits for the same objects.  What it decides is the cost.  A scene with a grid (see rtm_scene_create) serves through it
 * every ray with |d.d - 1| <= 4e-7 — any direction normalised in double precision; normalising is the caller's business — and
 * an origin within the grid's reach, about two scene diagonals from the scene.  Any other ray makes its whole wave (the 64
 * consecutive rays it is among) run the loop over all objects: correct, and slow for a large scene.
 * Both calls only ENQUEUE one kernel on `stream` on the scene's device: no allocation, no copy, no host synchronisation.
 * They are serialised with the other calls on that (device, stream) and recorded as a use of the scene (rtm_scene_destroy
 * right after the call is safe).  The outputs must not overlap the ray buffers or each other (not checked).
 * n_rays == 0: RTM_OK, nothing is enqueued.  A null scene, org_dev, dir_dev or out_dev, an out_dev whose planes are all null,
 * a pointer that is not aligned to its element (8 bytes for doubles, 4 for object), n_rays > 0x7FFFFFFF:
 * RTM_ERR_INVALID_ARGUMENT with a text in rtm_last_error_detail, before any device call.
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
typedef struct rtm_hit_buffers { /* DEVICE pointers on the scene's device; any may be null, not all */
    int32_t* object; /* n_rays: index of the hit object in the scene's order, -1 on a miss             */
    double* t;       /* n_rays: the loop's dis; +infinity on a miss                                     */
    double* normal;  /* n_rays x 3: Intersect's out_normal of the hit object; +0 on a miss              */
} rtm_hit_buffers;
int rtm_scene_nearest(const rtm_scene* scene, const double* org_dev, const double* dir_dev, size_t n_rays,
                      const rtm_hit_buffers* out_dev, void* stream);
int rtm_scene_occluded(const rtm_scene* scene, const double* org_dev, const double* dir_dev,
                       const double* tmax_dev /* n_rays, nullable: +infinity */, size_t n_rays,
                       uint8_t* out_dev /* n_rays: 1 occluded, 0 not */, void* stream);

/* ---- radiance queries on a scene: "how much light arrives along this ray?" for rays of the caller's ----
 * Rays as for the ray queries above: org_dev and dir_dev hold n_rays x 3 doubles on the scene's device, a row per ray.
 * For ray i and s = 0 .. S-1 (S = params->samples), L_s is png::PathTracing (src/Renderer.cpp:57-117) on (org_i, dir_i) with
 * the generator stream (seed, pixel = key_base + i, sample = s) — exactly what rtm_path_trace_batch computes for that key,
 * bit for bit, max_bounces, the mode and RTM_MODE_HOST_TRIG included.  radiance_i is the sum over s ascending, from +0.0, of
 * t_s = L_s / (double)S per component; with RTM_RADIANCE_CLAMP each t_s first goes through the clamp of src/Renderer.cpp:241
 * (std::min<double>(std::max<double>(v, 0), 1.0f)).  Every multiply, add and divide is separately rounded.
 * That is the reference's own accumulation of a pixel's samples (src/Renderer.cpp:240-242) at superSamples == 1: with the
 * clamp, key_base = 0 and the rays of a camera's pixels in row-major order, radiance is rtm_render_scene's out_f64 for the
 * same settings, bit for bit.  Without the clamp it is the plain mean of the samples, for probes and baking.
 * casts_i and draws_i count the nearest-hit loops run and the generator calls made for ray i over all its samples, modulo 2^32.
 * Directions of any length, origins anywhere; a ray with a non-finite component hits nothing and returns +0 (one cast per
 * sample, no draw).  The scene decides only the cost, as for the ray queries: one with a grid, one without, one built by
 * rtm_scene_create_device give the same bits; a ray the grid cannot serve (see above) sends its wave, for that cast, through
 * the loop over all objects.
 * Parallelism is over RAYS only: one GPU lane per ray traces that ray's S samples one after the other (which is what keeps
 * the sum in sample order).  A call with few rays and many samples leaves the device idle; repeat the rays instead, each copy
 * under its own key (key_base + its row), and combine the copies' means.
 * The contract is the ray queries', with one addition.  Every argument is checked before any device call, and a refusal
 * leaves a text in rtm_last_error_detail: a null scene, org_dev, dir_dev, params or out_dev, an out_dev whose planes are all
 * null, a pointer that is not aligned to its element (8 bytes for doubles, 4 for casts and draws), n_rays > 0x7FFFFFFF,
 * key_base + n_rays > 2^32, samples == 0, max_bounces < -1, flag bits other than RTM_RADIANCE_CLAMP, a nonzero reserved, a mode
 * that is neither RTM_MODE_LITERAL nor RTM_MODE_REPAIRED with or without RTM_MODE_HOST_TRIG: RTM_ERR_INVALID_ARGUMENT;
 * RTM_MODE_SURFACE_SAMPLE: RTM_ERR_UNSUPPORTED.  n_rays == 0: RTM_OK, nothing is enqueued.  Otherwise the call only ENQUEUES on
 * `stream` on the scene's device, is serialised with the other calls on that (device, stream) and recorded as a use of the
 * scene.  The outputs must not overlap the ray buffers or each other (not checked).
 * The addition: hit records.  The kernel keeps 16 levels per path on chip; a call with 0 <= max_bounces <= 16 needs no more
 * and touches no work buffer.  Any other call takes the deeper levels from the record pool the library keeps for (device,
 * stream), exactly as a render does (see rtm_render_scene): the first call on the pair that needs the pool — and, with
 * RTM_MODE_HOST_TRIG, the first on the device that needs the trig table — sets it up, which may allocate and wait once;
 * steady-state calls do neither.  A lane takes one pool slot of 960 levels the first time one of its paths needs it and keeps it
 * for all its samples, so the pool is sized to the call: one slot (3 840 bytes) per ray, rounded up to 64 rays, for at most
 * 262 144 rays (960 MiB); a call with more rays runs as launches of 262 144, one behind the other on the stream.  The number
 * of rays therefore never exhausts the pool.  What remains is the depth of ONE path, the render's 976 bounces: max_bounces >
 * 976 is refused with RTM_ERR_UNSUPPORTED like a render's, and with max_bounces = -1 a path that reaches level 976 is
 * truncated there (that sample contributes 0, its casts and draws up to there are counted, the ray's other samples are
 * traced normally) and raises the stream's sticky overflow flag, which rtm_stream_status reports and clears.
 * rtm_release_scratch / rtm_stream_release free the pool.
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbol up. */
#define RTM_RADIANCE_CLAMP 1u
typedef struct rtm_radiance_params { /* 32 bytes */
    int32_t mode;        /* RTM_MODE_REPAIRED or RTM_MODE_LITERAL, optionally | RTM_MODE_HOST_TRIG               */
    int32_t max_bounces; /* -1: the reference's unlimited recursion; >= 0: the build's depth cap (rtm_options)   */
    uint64_t seed;
    uint32_t samples;    /* S >= 1                                                                               */
    uint32_t key_base;   /* ray i draws sample s from the stream (seed, pixel = key_base + i, sample = s)        */
    uint32_t flags;      /* RTM_RADIANCE_CLAMP or 0                                                              */
    uint32_t reserved;   /* 0                                                                                    */
} rtm_radiance_params;
typedef struct rtm_radiance_buffers { /* DEVICE pointers on the scene's device; any may be null, not all; 24 bytes */
    double* radiance;    /* n_rays x 3                                                                            */
    uint32_t* casts;     /* n_rays: nearest-hit loops run for the ray, all samples, modulo 2^32                   */
    uint32_t* draws;     /* n_rays: generator calls, likewise                                                     */
} rtm_radiance_buffers;
int rtm_scene_radiance(const rtm_scene* scene, const double* org_dev, const double* dir_dev, size_t n_rays,
                       const rtm_radiance_params* params, const rtm_radiance_buffers* out_dev, void* stream);

/* ---- the hot path: Renderer::Render's pixel/sample loop (src/Renderer.cpp:215-250) ----
 * Renders rows [row_begin,row_end) of the image into caller-owned DEVICE buffers; any of the
 * three outputs may be null.  Layout is the reference's: row-major, row 0 first, RGB interleaved
 * (src/Renderer.cpp:246-248).  out_f64 holds Renderer::image bit-for-bit semantics (double);
 * out_f32 is the same value rounded to float (the float3 accumulation buffer); out_u8 is the
 * reference's 8-bit quantisation (src/Renderer.cpp:251-254).
 *
 * rtm_render_scene with stats == NULL only ENQUEUES work on `stream` and returns: no copy from pageable
 * memory and no wait — except that the FIRST call on a (device, stream) pair sets up its context, and a call
 * that needs a larger work buffer than the pair has (see rtm_release_scratch) grows it, which allocates and
 * waits for that stream's queued work once; steady-state calls do neither.  Scenes that have a grid
 * (rtm_scene_create) are two launches per frame like any other; scenes of 512 spheres or more without one — rtm_render_device on a device
 * array, scenes the grid declines (planes, non-finite geometry), a far-away camera, variant 12 by name — they run a
 * pipeline of two launches per ray cast of the slowest pixel: with a depth cap such that samples x superSamples^2 x
 * (max_bounces + 1) <= 16 384 every trip that could be needed is enqueued at once (those after the last active pixel
 * has finished fall through) and the call returns like any other; with unlimited depth or a longer budget the host
 * follows the device-resident active-pixel count one batch of trips behind and the call returns when it has seen the
 * count at zero, i.e. it blocks for about the duration of the render.
 * With stats != NULL the call synchronises the stream to read the counters and the timing.
 *
 * Hit records of paths deeper than the on-chip levels spill to a pooled buffer (capacity: 976
 * bounces per path); exceeding it truncates that path and raises the stream's sticky overflow flag:
 *   - with stats != NULL the call itself returns RTM_ERR_UNSUPPORTED;
 *   - with stats == NULL it is reported by rtm_stream_status(device, stream) — call it after
 *     synchronising the stream — and by the NEXT render enqueued on that stream once the flag has
 *     reached the host (RTM_ERR_UNSUPPORTED, nothing enqueued).  The flag is cleared by the call
 *     that reports it. */
int rtm_render_scene(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                     double* out_f64_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream,
                     rtm_stats* stats);
/* Progressive rendering: samples [sample_begin, sample_end) of every pixel of the call's rows.  The sample index is
 * k = ((sx-1)*SS + (sy-1))*S + s, in the order of src/Renderer.cpp:223-225, with N = SS*SS*S.
 * accum_f64_dev (DEVICE, required, layout of out_f64) is the pixel accumulator:
 *   sample_begin == 0 : write-only; the fold starts at +0 exactly like rtm_render_scene
 *   sample_begin  > 0 : must hold what the call that ended at sample_begin left; the fold continues from it
 * After the pass that ends at N, accum / out_f32 / out_u8 are rtm_render_scene's out_f64 / out_f32 / out_u8 bit for bit
 * (the accumulator goes +0 -> +t0 -> ... and never holds -0, so continuing the fold from the stored value is exact).
 * Before that, out_f32 / out_u8 are a PREVIEW: the accumulator times N / sample_end, rounded or quantised like a final
 * frame.  The caller passes the same settings, scene and options (mode, seed, rows, bands, variant, max_bounces) to every
 * pass of a frame.
 * A null accumulator, sample_begin > sample_end or sample_end > N: RTM_ERR_INVALID_ARGUMENT, checked before the scene
 * pointer is looked at.  sample_begin == sample_end: RTM_OK, nothing enqueued.  Enqueueing, stats (rtm_stats.samples counts
 * the pass's rows x width x (sample_end - sample_begin)) and the sticky overflow flag are rtm_render_scene's.  Every variant
 * variant 0 resolves to serves any range, and so does variant 18; variants 7, 15 and 16 render [0, N) only and return
 * RTM_ERR_UNSUPPORTED for any other range without writing anything.  rtm_scratch_bytes' figure for the whole frame bounds
 * what any pass of it asks for.
 * Added after RTM_ABI_VERSION 5 without changing it: callers detect the entry point by looking the symbol up. */
int rtm_render_scene_samples(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                             uint32_t sample_begin, uint32_t sample_end, double* accum_f64_dev, float* out_f32_dev,
                             uint8_t* out_u8_dev, void* stream, rtm_stats* stats);
/* rtm_render_scene_samples restricted to a DEVICE list of tiles.  A tile is an 8x8 block of the call's output rows:
 * tiles_x = ceil(width / 8), tiles_y = ceil(output rows / 8); tile t covers columns 8 (t % tiles_x) .. +7 and the call's
 * local row block t / tiles_x, whose rows map to image rows as for a render (row range, interleaved bands).
 * Listed tiles get exactly the accumulator, f32 and u8 values of rtm_render_scene_samples over the same range (preview rule
 * included); pixels of tiles that are not listed are neither read nor written in any of the three buffers.  List order
 * changes no value.  An entry of tiles_x * tiles_y or more makes its blocks return before any load or store; duplicate entries
 * give unspecified pixels of those tiles but stay in bounds.  n_tiles == 0: RTM_OK, nothing enqueued; a null list with
 * n_tiles > 0: RTM_ERR_INVALID_ARGUMENT.  Range and accumulator errors are rtm_render_scene_samples'.  rtm_stats.samples
 * counts the in-frame pixels of the listed tiles x (sample_end - sample_begin) (a call with stats reads the list back).
 * Every variant that serves partial ranges serves lists (variant 0's choices, 1 and 18) except the wavefront pipeline:
 * variant 12, and variant 0 where it resolves to 12 (512 spheres or more without a grid), returns RTM_ERR_UNSUPPORTED before
 * writing anything, as do variants 7, 15 and 16.  rtm_scratch_bytes' figure for the whole frame bounds a call whose list has
 * at most tiles_x * tiles_y entries.
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbol up. */
int rtm_render_scene_tiles(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                           uint32_t sample_begin, uint32_t sample_end, const uint32_t* tiles_dev, uint32_t n_tiles,
                           double* accum_f64_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream, rtm_stats* stats);
/* ---- tile-adaptive sampling on top of rtm_render_scene_tiles ----
 * N = SS*SS*S, m = min_samples.  Pass ends b_0 = min(m, N), b_i = min(2^i m, N).  Pass 0 traces [0, b_0) of every tile and
 * snapshots the accumulator; pass i >= 1 traces [b_{i-1}, b_i) of the tiles still active, then each of them is checked:
 *   sb = (double)N / b_i, sa = (double)N / b_{i-1};  I_c = acc_c * sb, J_c = snap_c * sa  (c = R, G, B)
 *   d = (|I_R - J_R| + |I_G - J_G|) + |I_B - J_B|;   e_p = d / (1e-3 + sqrt((I_R + I_G) + I_B))
 *   E = max of e_p over the tile's in-frame pixels (a NaN e_p makes E NaN)
 * in double, without contraction, sqrt correctly rounded.  (I - J is half the difference of the means of samples [0, a) and
 * [a, b): a relative noise estimate weighted towards dark pixels.)  The tile stays active iff b_i < N && !(E <= threshold):
 * a negative threshold stops nothing, a NaN E keeps the tile.  An active tile copies acc -> snapshot; every checked tile
 * records b_i.  The active tiles form the next list in ascending order (a deterministic scan, no atomics).
 * Result, tile by tile, with k = tile_samples[t]: the accumulator is rtm_render_scene_samples' over [0, k) bit for bit, f32
 * and u8 that pass's preview; tiles that ran to N hold rtm_render_scene's bytes.
 * tile_samples_dev (nullable, DEVICE): tiles_y x tiles_x words.  work_dev (DEVICE, 256-byte aligned): at least
 * rtm_adaptive_work_bytes = round256(24 x width x rows) (the snapshot) + 3 x round256(4 x tiles) (two lists, the flags) + 256
 * (the counts); 0 for a call without rows.
 * The call BLOCKS: after each checkpoint it copies the 4-byte active count to the host and waits for the stream.  It stops
 * when no tile is active or b_i = N.  It allocates nothing beyond the per-stream render scratch.  With stats: the passes'
 * counters summed, kernel_ms including the checkpoints, variant the resolved one.
 * A null params, accumulator or work buffer, min_samples == 0, a NaN or infinite threshold or a misaligned work_dev:
 * RTM_ERR_INVALID_ARGUMENT before any device call (a null scene too).  A variant that refuses tile lists (7, 15, 16, the
 * wavefront pipeline 12 and variant 0 where it resolves to 12) returns RTM_ERR_UNSUPPORTED having written only work_dev: the
 * accumulator, the views and tile_samples are untouched.  Rows and bands as for a render; one device (no adaptive multi-GPU).
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
typedef struct rtm_adaptive_params {
    uint32_t min_samples; /* m >= 1; m >= N renders the frame in one pass */
    float threshold;      /* finite; < 0: no tile stops (the full frame) */
} rtm_adaptive_params;
size_t rtm_adaptive_work_bytes(const rtm_settings* settings, const rtm_options* options);
int rtm_render_adaptive(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                        const rtm_adaptive_params* params, double* accum_f64_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                        uint32_t* tile_samples_dev, void* work_dev, void* stream, rtm_stats* stats);
/* ---- first-hit feature buffers (AOVs) of a frame: what a preview's denoiser, compositor or object picker needs ----
 * Primary rays have no jitter (src/Renderer.cpp:224-232), so every value below is a deterministic function of the scene
 * and the camera.  Sub-pixels are visited in the reference's loop order, sx = 1..SS outer, sy = 1..SS inner; for each:
 *   ray     org = camera.origin, dir = the primary direction of src/Renderer.cpp:227-232 (the render kernels' bits)
 *   hit     the nearest-hit loop of :58-73 in the reference's own arithmetic (hit needs t < dis && t > 0, the lowest index
 *           wins ties; spheres through SphereObject::Intersect, planes through the build-defined square above)
 *   n       the orienting normal PathTracing holds at that hit (:80-83): Dot(normal, dir) < 0.0 ? normal : normal * -1.0,
 *           where normal is what Intersect reports for the mode: RTM_MODE_REPAIRED Normalize(hitPoint - centre) (float-sqrtf
 *           magnitude; a plane's m_normal); RTM_MODE_LITERAL vec3(), lost as in the reference, so n = (-0, -0, -0)
 *   albedo  the hit object's raw material colour (rtm_sphere.color / rtm_object.color, not colorKD)
 * Per pixel, in float (any plane pointer may be null; only the non-null ones are written):
 *   depth   1 float      the CENTRE sub-pixel's dis rounded to float, +inf on a miss
 *   object  1 int32      the centre sub-pixel's object index, -1 on a miss
 *   normal  3 floats     sum of n over the SS^2 sub-pixels, divided by (double)(SS*SS), rounded to float (RGB-interleaved
 *                        like out_f32); literal mode gives +0 everywhere (the sum starts at +0.0)
 *   albedo  3 floats     the same reduction over the albedo
 * The centre sub-pixel is c = (SS + 1) / 2 (integer division) in both axes: the one nearest the pixel centre, the first
 * in loop order on ties.  Sums are taken in double from +0.0 in loop order; a miss adds +0. */
typedef struct rtm_aov_buffers {
    float* depth;     /* DEVICE, rows x width          */
    float* normal;    /* DEVICE, rows x width x 3      */
    float* albedo;    /* DEVICE, rows x width x 3      */
    int32_t* object;  /* DEVICE, rows x width          */
} rtm_aov_buffers;
/* The AOVs of the rows [row_begin, row_end) (bands as for a render; rows stored back to back, rtm_output_rows of them).
 * Only ENQUEUES one kernel on `stream` and allocates nothing; serialised per (device, stream) like a render, and recorded
 * as a use of the scene (rtm_scene_destroy right after the call is safe).  Variant 0: the scene's uniform grid where a
 * render would take it (see rtm_scene_create), else the chunked exhaustive loop; 1: the general per-object
 * loop; 17: the grid (RTM_ERR_UNSUPPORTED for a scene without one); any other variant: RTM_ERR_UNSUPPORTED.  seed,
 * max_bounces and the mode flags (RTM_MODE_HOST_TRIG, _COUNT_TESTS, _SURFACE_SAMPLE) are ignored: there are no draws and
 * no trigonometry.  Null settings, options, out_dev or scene, bad rows or bands, a bad mode: RTM_ERR_INVALID_ARGUMENT,
 * before any device call.  Added after RTM_ABI_VERSION 5 without changing it: callers look the symbol up. */
int rtm_render_aov(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                   const rtm_aov_buffers* out_dev, void* stream);

/* ---- coverage AOVs of a frame: alpha, ranked id / coverage layers (Cryptomatte-style), a matte, "over" a background ----
 * rtm_render_aov's object plane is one hard choice per pixel; these planes say which objects cover a pixel and by how much.
 * Sub-pixels, rays and hits are exactly rtm_render_aov's: sx = 1..SS outer, sy = 1..SS inner, the primary direction of
 * src/Renderer.cpp:227-232 (the render kernels' bits), the nearest-hit loop of :58-73 (hit needs t < dis && t > 0, the lowest
 * index wins ties; spheres and the build-defined plane).  Nothing is random, so every value is exact.  Per pixel:
 *   counts    c_i = the number of the SS^2 sub-pixels whose first hit is object i;  m = the number that miss
 *   alpha     (float)((double)(SS^2 - m) / (double)SS^2)
 *   ranking   the objects with c_i > 0 by c_i descending, ties by i ascending; misses are never ranked
 *   layer l   (0-based) of a pixel with D distinct objects: id = i_l, coverage = (float)((double)c_{i_l} / (double)SS^2) for
 *             l < D;  id = -1, coverage = +0.0f for l >= D
 * Objects beyond `layers` are dropped: alpha - (sum of the coverages) tells how much.  Layers are PLANAR: plane l of id and of
 * coverage is rank l of every pixel.  Any plane pointer may be null; only the non-null ones are written. */
typedef struct rtm_matte_buffers {
    int32_t* id;       /* DEVICE, layers x rows x width (planar: plane l is rank l) */
    float*   coverage; /* DEVICE, layers x rows x width                             */
    float*   alpha;    /* DEVICE, rows x width                                      */
} rtm_matte_buffers;
/* The coverage AOVs of the rows [row_begin, row_end): rows, bands, variants (0, 1 and 17 as rtm_render_aov serves them; any
 * other: RTM_ERR_UNSUPPORTED), the serialisation per (device, stream) and the recording of the scene's use are
 * rtm_render_aov's.  Only ENQUEUES one kernel on `stream`, allocates nothing and needs no work buffer; seed, max_bounces and
 * the mode flags are ignored.  layers outside 1..8, all three planes null, null settings, options or out_dev, bad rows or
 * bands, a bad mode: RTM_ERR_INVALID_ARGUMENT.  super_samples > 8: RTM_ERR_UNSUPPORTED (a block keeps the SS^2 ids of its 64
 * pixels in LDS: 8^2 ids x 64 lanes x 4 B = 16 KiB is the limit).  Both are checked before the scene pointer is looked at; a
 * null scene is RTM_ERR_INVALID_ARGUMENT after that; all before any device call.
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
int rtm_render_mattes(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options, int32_t layers,
                      const rtm_matte_buffers* out_dev, void* stream);
#define RTM_MATTE_DEFAULT_LAYERS 4 /* what rtm_cli --matte-layers and the Python package default to */
/* The antialiased matte of a set of objects from a frame's layers (width x height pixels, rows = height, no bands):
 *   matte_p = (float)min(1.0, sum over the layers l ascending with id_{l,p} >= 0 in the list of (double)coverage_{l,p})
 * the sum taken in double from +0.0: exact given the layers.  ids_dev: a DEVICE list of n_ids ids, unsorted; duplicates are
 * harmless, a negative entry selects nothing.  Keeps no state, allocates nothing, ENQUEUES one launch on `stream` of `device`.
 * layers outside 1..8, n_ids outside 1..64, a null pointer, a non-positive size, a pointer that is not 4-byte aligned,
 * matte_out_dev equal to an input, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A frame of 2^31
 * pixels or more: RTM_ERR_UNSUPPORTED. */
int rtm_matte(int32_t width, int32_t height, int32_t layers, int device, const int32_t* layer_id_dev,
              const float* layer_coverage_dev, const int32_t* ids_dev, int32_t n_ids, float* matte_out_dev, void* stream);
/* A traced frame "over" a background, premultiplied: the frame already holds zero for the fraction of a pixel that missed
 * (a primary ray that misses returns vec3(), src/Renderer.cpp:116).  color (DEVICE, height x width x 3 floats, RGB-interleaved
 * like out_f32), alpha (height x width, as rtm_render_mattes writes it), background_dev (nullable, height x width x 3).  Per
 * channel, in float, without contraction:
 *   t = 1.0f - alpha_p;   out = color + t * B      B = the background pixel where background_dev is given, else
 *                                                      params->background
 * out_u8 (if non-null) is rtm_quantise of (double)out_f32, bit for bit.  out_f32_dev == color_dev is allowed.  Keeps no
 * state, allocates nothing, ENQUEUES one launch.  Null params, color_dev or alpha_dev, both outputs null, a NaN or infinite
 * constant background, a non-positive size, a float pointer that is not 4-byte aligned, an output equal to alpha_dev or
 * background_dev, out_u8_dev equal to color_dev, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A
 * frame of 2^31 pixels or more: RTM_ERR_UNSUPPORTED, as rtm_tonemap. */
typedef struct rtm_composite_params {
    float background[3]; /* finite; used where background_dev is null */
} rtm_composite_params;
int rtm_composite(const rtm_composite_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                  const float* alpha_dev, const float* background_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream);

/* ---- firefly: a rank-order outlier clamp and the repair of non-finite pixels — what a path tracer leaves at low sample
 * counts: isolated pixels far brighter than everything around them, and now and then a NaN.  Opt-in, right after the render
 * and before every other stage: the denoisers spread a firefly into a blob and a NaN over the frame, rtm_tonemap's L_max takes
 * a firefly for the white point, rtm_bloom makes a glare star of it.  Every other stage and its defaults stay.
 * Input: color (DEVICE, height x width x 3 floats, RGB-interleaved like out_f32; 4-byte alignment is enough).  Arithmetic in
 * float, without contraction, in exactly this order, so that a float32 restatement reproduces every decision bit for bit.
 *   1 counting   a pixel COUNTS iff its three components are finite.  l = (0.2126f c_R + 0.7152f c_G) + 0.0722f c_B
 *                (rtm_tonemap's lum), Y = l > 0 ? l : +0.0f.  (No l of a counting pixel is NaN; one that overflows is +inf.)
 *   2 neighbours q = p + (dx, dy), dx and dy in -radius..radius, q != p.  Taps outside the frame or not counting are skipped,
 *                not clamped (the library's rule).  n is the number of taps left.
 *   3 statistic  S is the rank-th largest Y_q over those taps, counted with multiplicity (sorted descending, index rank - 1).
 *                A selection: exact, and ties cannot matter.  With n < rank the pixel has no statistic.
 *   4 threshold  T = (k S) + floor, two roundings.  An overflow to +inf is kept as the float it is: nothing exceeds it.
 *   5 decision   a counting pixel with a statistic is a FIREFLY iff Y_p > T.  Its out_f32 is c_p (T / Y_p) per channel: the
 *                chroma is kept, the luminance is brought down to the threshold.  Y_p > T >= 0, so the divisor is positive;
 *                the output is continuous in c_p across the threshold, so the division may be the device's fast form.  Every
 *                other counting pixel's out_f32 is its input, bit for bit.
 *   6 the rest   a pixel that does not count: with repair = 0 its out_f32 is its input's words; with repair = 1 it is the
 *                per-channel mean of the counting taps' colours (the sum in float, dy outer and dx inner, then one division
 *                by (float)n; a sum that overflows is kept as the float it is), and (+0, +0, +0) when n = 0.  Either way it
 *                contributes to no other pixel's window.
 *   7 outputs    mask_out_dev (nullable, height x width bytes): 0 unchanged, 1 clamped, 2 repaired (a pixel that does not
 *                count keeps 0 with repair = 0).  threshold_out_dev (nullable, height x width floats): T, or +inf for a pixel
 *                without a statistic or one that does not count.  out_u8 (nullable) is rtm_quantise of (double)out_f32, out
 *                of range (NaN included) -> 0, as in the other stages.
 * It follows that a frame in which no pixel exceeds its threshold and every pixel counts is copied bit for bit; that a
 * constant frame is copied bit for bit (k >= 1, floor >= 0); and that the luminance of an output pixel never exceeds its
 * input's.  With the defaults (radius 1, rank 3) every pixel of a uniformly bright axis-aligned rectangle of at least 2 x 2
 * pixels keeps its words, however dark the surround: a convex corner pixel has three neighbours inside the rectangle.  That
 * is why the default rank is 3: a light seen directly must not be eaten at its rim.  With the defaults a cluster of up to
 * three fireflies is still caught (each has at most two bright neighbours).  A one-pixel-wide bright line is clamped at rank
 * 3 and kept at rank 2 (an inner pixel of it has two bright neighbours; its two end pixels have one, and go at rank 2 too).
 * Against a float64 evaluation of c_p (T / Y_p) from the float T and Y_p, and of the repair mean, every changed component is
 * within 1e-4 max(1, |ref|); mask_out and threshold_out are exact; out_u8 is exact given the call's own out_f32.
 * No atomics, no state, no work buffer: the call allocates nothing and only ENQUEUES one launch on `stream`; the same inputs
 * give the same bits on every call, on any stream, at any 4-byte alignment.  Null params or color_dev, all four outputs
 * null, a non-positive size, radius outside 1..3, rank outside 1..8, k NaN, infinite or below 1, floor NaN, infinite, negative
 * or -0.0, repair outside {0, 1}, a float pointer that is not 4-byte aligned, any output equal to color_dev (a gather cannot
 * run in place), two outputs equal to each other, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A
 * frame of 2^31 pixels or more, or one of 2^23 or more tiles of 32 x 16 pixels (ceil(width / 32) ceil(height / 16): a launch
 * has one 512-lane block a tile): RTM_ERR_UNSUPPORTED, as rtm_defocus.
 * Defaults: RTM_FIREFLY_DEFAULTS below (what Renderer.Render(firefly=True) and rtm_cli --firefly use).  Added after
 * RTM_ABI_VERSION 5 without changing it: callers look the symbol up. */
typedef struct rtm_firefly_params { /* 20 bytes */
    int32_t radius; /* 1..3: the window is (2 radius + 1)^2, the centre excluded                                          */
    int32_t rank;   /* 1..8: the neighbour statistic is the rank-th LARGEST luminance (1 = the maximum)                   */
    float k;        /* finite, >= 1: how far above that statistic a pixel may be                                          */
    float floor;    /* finite, >= 0 (not -0.0): added to the threshold, so that dark regions keep faint detail            */
    int32_t repair; /* 0 / 1: replace a pixel that does not count by the mean of its counting neighbours                  */
} rtm_firefly_params;
#define RTM_FIREFLY_DEFAULTS {1, 3, 4.0f, 0.01f, 1} /* of rtm_firefly_params */
int rtm_firefly(const rtm_firefly_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                float* out_f32_dev, uint8_t* out_u8_dev, uint8_t* mask_out_dev, float* threshold_out_dev, void* stream);

/* ---- denoiser: an edge-avoiding à-trous wavelet filter (Dammertz et al. 2010) guided by the AOVs above, with the albedo
 * demodulated (SVGF-style) and no temporal part ----
 * Inputs: a frame of width x height pixels; color (DEVICE, height x width x 3 floats, RGB-interleaved like out_f32); the
 * guide planes in the rtm_aov_buffers layout of the whole frame (rows = height, no bands).  guide_dev itself and any of its
 * four pointers may be null: a null plane switches its term off.  Depths are positive or +inf, as rtm_render_aov writes
 * them.  Arithmetic in float:
 *   1 demodulate  a_p,k = albedo_p,k > 1e-3f ? albedo_p,k : 1.0f (1.0f without an albedo plane); e0_p = c_p / a_p per
 *                 channel (the Cornell light has albedo 0: it is filtered as its own emission)
 *   2 iterate     for i = 0 .. K-1, step s = 2^i:  e(i+1)_p = sum_q w_i(p,q) e(i)_q / sum_q w_i(p,q), over the taps
 *                 q = (x + s dx, y + s dy), dx, dy in -2..2; taps outside the frame are skipped (not clamped); the sums run
 *                 dy outer, dx inner.  w_i(p,q) = h[dx] h[dy] g(p,q) w_c, h = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *                 g(p,q), the geometry weight:
 *                   q == p: 1 (so sum w >= h[2]^2 = (3/8)^2 > 0: never a division by zero)
 *                   else, object given and obj_p != obj_q: 0
 *                   else, depth given: both depths +inf (two misses): 1, the terms below skipped; exactly one +inf: 0;
 *                         otherwise w_z = sigma_depth > 0 ? exp(-|z_p - z_q| / (sigma_depth s max(z_p, z_q))) : 1
 *                   w_n = (normal given && sigma_normal > 0) ? max(0, n_p . n_q)^sigma_normal : 1;  g = w_z w_n
 *                 w_c = sigma_color > 0 ? exp(-|e(i)_p - e(i)_q|^2 4^i / sigma_color^2) : 1 (Dammertz's sigma halved
 *                 at each level)
 *   3 remodulate  out_p = e(K)_p a_p
 *   K = 0 copies color to out_f32 bit for bit.  out_u8 (if non-null) is rtm_quantise of (double)out_f32, bit for bit.
 * exp and pow may be the device's fast forms: against a float64 evaluation of the steps above every output component is
 * within 1e-4 max(1, |ref|).  No atomics: the same inputs give the same bits on every call, on any stream.
 * Defaults: RTM_DENOISE_DEFAULTS below (what Renderer.Render(denoise=True) and rtm_cli --denoise use, chosen on the Cornell
 * box): iterations 4, sigma_color 16, sigma_normal 64, sigma_depth 0.05. */
typedef struct rtm_denoise_params {
    int32_t iterations; /* K, 0..10 */
    float sigma_color;  /* >= 0, finite; 0 switches the term off */
    float sigma_normal; /* >= 0, finite: an exponent; 0 switches the term off */
    float sigma_depth;  /* >= 0, finite: relative depth; 0 switches w_z off (the +inf rules stay) */
} rtm_denoise_params;
#define RTM_DENOISE_DEFAULTS {4, 16.0f, 64.0f, 0.05f} /* an initializer of rtm_denoise_params */
/* Bytes of the work buffer rtm_denoise needs for a frame: 48 per pixel (two ping-pong planes and the packed guides, one
 * 16-byte record per pixel each); 0 for a non-positive size. */
size_t rtm_denoise_work_bytes(int32_t width, int32_t height);
/* Filters `color_dev` into out_f32_dev and / or out_u8_dev (DEVICE, height x width x 3; either may be null, not both).
 * The caller owns every buffer; work_dev (DEVICE, 16-byte aligned, rtm_denoise_work_bytes bytes) holds the intermediate
 * planes, so the call allocates nothing and only ENQUEUES its launches (K + 1, or one for K = 0) on `stream` of `device`.
 * It keeps no per-(device, stream) state and needs no serialisation: calls on different streams with different work
 * buffers run side by side.  Null params, color_dev or work_dev, both outputs null, a non-positive size, iterations outside
 * 0..10, a negative, NaN or infinite sigma, color_dev equal to out_f32_dev or to work_dev, a misaligned work_dev, a negative
 * device: RTM_ERR_INVALID_ARGUMENT, before any device call.  Added after RTM_ABI_VERSION 5 without changing it: callers
 * look the symbols up. */
int rtm_denoise(const rtm_denoise_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                const rtm_aov_buffers* guide_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream);

/* ---- variance-guided denoiser: the spatial part of SVGF (Schied et al. 2017) on top of the filter above, for frames whose
 * noise is uneven (adaptive frames, late progressive previews).  The colour weight of rtm_denoise, one global sigma_color,
 * becomes a luminance weight relative to each pixel's own standard deviation, estimated from the frame itself and carried
 * through the levels, so that converged pixels keep their shading.  Inputs as rtm_denoise.  Arithmetic in float; g_s(p,q)
 * is rtm_denoise's geometry weight g(p,q) at step s (the object test, the +inf miss rules, w_z with sigma_depth s, w_n,
 * g = 1 for q == p), h = {1/16, 1/4, 3/8, 1/4, 1/16}, lum(e) = 0.2126 e_R + 0.7152 e_G + 0.0722 e_B:
 *   1 demodulate  as rtm_denoise: a_p, e0_p = c_p / a_p
 *   2 variance    l = lum(e0); over the taps q = (x + dx, y + dy), dx, dy in -3..3 (unstepped), taps outside the frame
 *                 skipped, the sums dy outer, dx inner: u = g_1(p,q), d_q = l_q - l_p, U = sum u (>= 1: the centre tap has
 *                 u = 1, d = 0), m1 = sum u d_q / U, m2 = sum u d_q^2 / U, v0_p = max(0, m2 - m1 m1).  The shift by l_p is
 *                 part of the contract: it keeps the subtraction from cancelling in float.  variance_out_dev (if non-null)
 *                 receives v0, for K = 0 too.
 *   3 iterate     for i = 0 .. K-1, step s = 2^i, l = lum(e(i)):
 *                 v~_p = sum k[dx] k[dy] v(i)_q / sum k[dx] k[dy] over dx, dy in -1..1 (unstepped), in-frame taps only,
 *                 k = {1/4, 1/2, 1/4}, no geometry weight;
 *                 w_l(p,q) = sigma_lum > 0 ? exp(-|l_p - l_q| / (sigma_lum sqrt(v~_p) + 1e-4f)) : 1 (only v~_p enters, never
 *                 v~_q); w(p,q) = h[dx] h[dy] g_s(p,q) w_l(p,q), w(p,p) = h[2]^2, over q = p + s (dx, dy), dx, dy in -2..2,
 *                 taps outside the frame skipped, dy outer;
 *                 e(i+1)_p = sum w e(i)_q / sum w;  v(i+1)_p = sum w^2 v(i)_q / (sum w)^2
 *   4 remodulate  out_p = e(K)_p a_p
 *   K = 0 copies color to out_f32 bit for bit.  out_u8 (if non-null) is rtm_quantise of (double)out_f32, bit for bit.
 * exp, sqrt and the divisions may be the device's fast forms: against a float64 evaluation of the steps above every output
 * component is within 1e-4 max(1, |ref|), and so is variance_out.  No atomics: the same inputs give the same bits on every
 * call, on any stream.
 * Defaults: RTM_DENOISE_VAR_DEFAULTS below (what Renderer.Render(denoise="variance") and rtm_cli --denoise-variance use;
 * SVGF's sigma_lum and K with rtm_denoise's sigma_normal and sigma_depth): iterations 5, sigma_lum 4,
 * sigma_normal 64, sigma_depth 0.05. */
typedef struct rtm_denoise_var_params {
    int32_t iterations; /* K, 0..10 */
    float sigma_lum;    /* >= 0, finite; 0 switches the luminance term off */
    float sigma_normal; /* as rtm_denoise_params */
    float sigma_depth;  /* as rtm_denoise_params */
} rtm_denoise_var_params;
#define RTM_DENOISE_VAR_DEFAULTS {5, 4.0f, 64.0f, 0.05f} /* an initializer of rtm_denoise_var_params */
/* Bytes of the work buffer rtm_denoise_variance needs for a frame: 56 per pixel (rtm_denoise's three planes of 16-byte
 * records and two variance planes of one float); 0 for a non-positive size, SIZE_MAX when the size does not fit a size_t. */
size_t rtm_denoise_variance_work_bytes(int32_t width, int32_t height);
/* Filters `color_dev` into out_f32_dev and / or out_u8_dev and writes v0 to variance_out_dev (DEVICE, height x width
 * floats); any of the three may be null, not all: with both colour outputs null the call only estimates the variance.  The
 * caller owns every buffer; work_dev (DEVICE, 16-byte aligned, rtm_denoise_variance_work_bytes bytes) holds the intermediate
 * planes, so the call allocates nothing and only ENQUEUES its launches (K + 2; for K = 0 one, or three with a variance
 * output) on `stream` of `device`.  It keeps no per-(device, stream) state and needs no serialisation.  Everything
 * rtm_denoise refuses (with "both outputs null" read as "all three outputs null"), and variance_out_dev equal to color_dev,
 * to work_dev or to out_f32_dev: RTM_ERR_INVALID_ARGUMENT, before any device call.  Added after RTM_ABI_VERSION 5 without
 * changing it: callers look the symbols up. */
int rtm_denoise_variance(const rtm_denoise_var_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                         const rtm_aov_buffers* guide_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                         float* variance_out_dev, void* stream);

/* ---- display transform: the last stage before an 8-bit file — exposure (fixed, or Reinhard's log-average key), a tone
 * curve, the sRGB transfer function and an ordered-dither store.  Opt-in: rtm_quantise and the out_u8 of the renders and
 * the denoisers stay the reference's bytes.
 * Input: color (DEVICE, height x width x 3 floats, RGB-interleaved like out_f32; 4-byte alignment is enough).  Arithmetic in
 * float unless stated, without contraction.  lum(c) = (0.2126 c_R + 0.7152 c_G) + 0.0722 c_B (the denoiser's weights).
 *   1 statistics  over the whole frame.  A pixel COUNTS iff its three components are finite; Y_p = max(lum(c_p), 0); n the
 *                 number of counting pixels; L_avg = exp((sum log(1e-4f + Y_p)) / n) (the logarithms float, their sum
 *                 carried in DOUBLE in an order fixed by the frame size alone); L_max = max Y_p; n == 0: L_avg = L_max = 1.
 *                 E = exp2(ev) (auto_exposure ? key / L_avg : 1).  stats_out_dev (nullable, DEVICE, one rtm_tonemap_stats)
 *                 receives {L_avg, L_max, E, n}.  The statistics are skipped when nothing needs them: no auto exposure,
 *                 not (REINHARD with white == 0) and no stats_out_dev.
 *   2 map         per pixel, x = max(c E, 0) per channel, then
 *                   CLAMP     t = x
 *                   REINHARD  (extended, on luminance, chroma kept) Yx = lum(x), W = white > 0 ? white : E L_max;
 *                             t = x ((1 + Yx / W^2) / (1 + Yx)) when Yx > 0 && W > 0, else t = x
 *                   ACES      (Narkowicz's fit) per channel t = x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14)
 *                 then t = min(max(t, 0), 1)
 *   3 transfer    SRGB: t <= 0.0031308f ? 12.92f t : 1.055f t^(1/2.4) - 0.055f;  LINEAR: unchanged
 *   4 non-finite  a pixel that does not count is (0, 0, 0) in both outputs
 *   5 outputs     out_f32 = t.  out_u8 without dither is rtm_quantise of (double)out_f32, bit for bit; with dither it is
 *                 (uint8_t)min(255.0f, floorf(255.0f t + (B(x & 7, y & 7) + 0.5f) / 64.0f)), B the 8 x 8 Bayer index
 *                   B(x, y) = sum over i = 0..2 of (((x>>i) ^ (y>>i)) & 1) << (2(2-i)+1) | ((y>>i) & 1) << (2(2-i))
 *                 (a permutation of 0..63 whose 2 x 2 core is [[0, 2], [3, 1]]): the reference's truncation becomes a store
 *                 whose mean over an aligned 8 x 8 block is 255 t.
 *   {CLAMP, LINEAR, auto_exposure 0, dither 0, ev 0} gives the u8 bytes rtm_quantise gives for the (finite) input.
 * exp, log, exp2, pow and the divisions may be the device's fast forms: against a float64 evaluation of the steps above
 * every out_f32 component and the three float statistics are within 1e-4 max(1, |ref|); pixels is exact; out_u8 is exact
 * given the call's own out_f32.  No atomics: the same inputs give the same bits on every call, on any stream.
 * work_dev: DEVICE, 256-byte aligned, rtm_tonemap_work_bytes = round256(16 ceil(width height / 4096)) + 256 bytes (one
 * partial per 4096 pixels and the final statistics); 0 for a non-positive size, SIZE_MAX when the frame itself (12 bytes a
 * pixel) does not fit a size_t.  Required even when the statistics are skipped.  The call allocates nothing, keeps no
 * per-(device, stream) state, needs no serialisation and only ENQUEUES: three launches, one when the statistics are
 * skipped, two when stats_out_dev is the only output.  out_f32_dev == color_dev (in place) is allowed: the statistics are
 * read before the map, in stream order.  Null params, color_dev or work_dev, all three outputs null, a non-positive size,
 * op or transfer out of range, auto_exposure or dither not 0 or 1, a NaN or infinite ev, key or white, |ev| > 32, key <= 0,
 * white < 0, a misaligned work_dev, work_dev equal to any other buffer, stats_out_dev equal to color_dev or out_f32_dev, a
 * negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.
 * Defaults: RTM_TONEMAP_DEFAULTS below (what Renderer.Render(tonemap=True) and rtm_cli --display use).
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
enum { RTM_TONEMAP_CLAMP = 0, RTM_TONEMAP_REINHARD = 1, RTM_TONEMAP_ACES = 2 };
enum { RTM_TRANSFER_LINEAR = 0, RTM_TRANSFER_SRGB = 1 };
typedef struct rtm_tonemap_params {
    int32_t op;            /* RTM_TONEMAP_*                                                       */
    int32_t transfer;      /* RTM_TRANSFER_*                                                      */
    int32_t auto_exposure; /* 0: E = 2^ev;  1: E = 2^ev * key / L_avg                             */
    int32_t dither;        /* 0: u8 = rtm_quantise;  1: ordered 8x8 dither (above)                */
    float ev;              /* finite, |ev| <= 32                                                  */
    float key;             /* finite, > 0 (0.18: middle grey)                                     */
    float white;           /* REINHARD only: finite, >= 0; 0 = the exposed frame maximum E*L_max  */
} rtm_tonemap_params;
#define RTM_TONEMAP_DEFAULTS {RTM_TONEMAP_ACES, RTM_TRANSFER_SRGB, 1, 1, 0.0f, 0.18f, 0.0f} /* of rtm_tonemap_params */
typedef struct rtm_tonemap_stats {
    float log_average;   /* L_avg */
    float max_luminance; /* L_max */
    float exposure;      /* E */
    uint32_t pixels;     /* n */
} rtm_tonemap_stats;
size_t rtm_tonemap_work_bytes(int32_t width, int32_t height);
int rtm_tonemap(const rtm_tonemap_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, rtm_tonemap_stats* stats_out_dev, void* stream);

/* ---- bloom (glare): the light a bright part of an HDR frame scatters into its surround, added in linear space before the
 * display transform — a bright pass, a pyramid of 4-tap down filters, an up pass that blends each coarser level into the
 * finer, and the add-back.  Opt-in: every other stage and its defaults stay.
 * Input: color (DEVICE, height x width x 3 floats, RGB-interleaved like out_f32; 4-byte alignment is enough).  Arithmetic in
 * float, without contraction.  lum(c) = (0.2126 c_R + 0.7152 c_G) + 0.0722 c_B (rtm_tonemap's).
 *   1 counting    a pixel COUNTS iff its three components are finite.  A pixel that does not count is (0, 0, 0) for steps
 *                 2-5: it contributes no light.
 *   2 bright pass per full-resolution pixel, never stored: x = max(c, 0) per channel, Y = lum(x), T = threshold,
 *                 K = knee T,
 *                   soft = min(max(Y - T + K, 0), 2K);  soft = soft soft / (4K + 1e-5f)
 *                   g = max(soft, Y - T) / max(Y, 1e-5f);  b0 = x g
 *                 g is continuous in Y.  threshold = 0 passes everything (g = Y / max(Y, 1e-5f)).  A frame whose every Y is at
 *                 or below T - K (with knee = 0: at or below the threshold) gives a bloom of exactly +0.
 *   3 down        level 0 is b0 at W_0 x H_0 = width x height; level l = 1..L has W_l = ceil(W_{l-1} / 2), H_l likewise (a
 *                 side that has reached 1 stays 1), and
 *                   d_l(X, Y) = sum over dy, dx in {-1, 0, 1, 2} of k[dx] k[dy] d_{l-1}(2X + dx, 2Y + dy) / (K_x K_y),
 *                 d_0 = b0, k = {1/8, 3/8, 3/8, 1/8}.  Taps outside level l-1's frame are skipped (not clamped); K_x is the sum
 *                 of k over the dx in the frame, K_y likewise: the library's skip-and-renormalise rule, and separable.  The
 *                 horizontal pass comes first.  The tap 2X is always in the frame; the filter is centred on 2X + 0.5, the
 *                 centre of the coarse pixel.
 *   4 up          u_L = d_L; for l = L-1 .. 1: u_l = (1 - scatter) d_l + scatter up_l(u_{l+1}).  up_l resamples level l+1 to
 *                 W_l x H_l: for the fine column x, X0 = floor((x - 1) / 2) (floor division: x = 0 gives -1), the taps are X0
 *                 and X0 + 1 with the weights (1/4, 3/4) for even x and (3/4, 1/4) for odd x (the fine pixel's centre is at
 *                 x / 2 - 1/4 in coarse coordinates); rows alike.  Taps outside the frame are skipped and the rest
 *                 renormalised; the 3/4 tap is always in the frame.  up is the exact counterpart of step 3's alignment.
 *   5 combine     B = up_0(u_1) at full resolution.  A pixel that counts: out_f32 = c + intensity B per channel (c, not x).
 *                 A pixel that does not count: out_f32 is its input, bit for bit — bloom adds light, it does not repair, and
 *                 rtm_tonemap downstream still sees the pixel as not counting.  bloom_out_dev (nullable, height x width x 3
 *                 floats) receives B at every pixel.  out_u8 (nullable) is the denoisers' store of the call's own out_f32:
 *                 rtm_quantise of (double)out_f32, out of range (NaN included) -> 0.
 * It follows that a constant frame c >= 0 with threshold 0 gives B = c at every level, and that intensity = 0 leaves every
 * counting pixel equal to its input.
 * The divisions may be the device's fast forms: against a float64 evaluation of the steps above every out_f32 component of a
 * counting pixel and every bloom_out component is within 1e-4 max(1, |ref|); out_u8 is exact given the call's own out_f32.
 * No atomics: the same inputs give the same bits on every call, on any stream, at any alignment of color.
 * work_dev: DEVICE, 256-byte aligned, rtm_bloom_work_bytes = the sum over l = 1..L of round256(16 W_l H_l) bytes: one plane
 * of 16-byte records per level (u_l overwrites d_l in place: the up pass reads d_l only at the pixel it writes); the plane of
 * level 1 is about 4 bytes per full-resolution pixel.  0 for a non-positive size or levels outside 1..8, SIZE_MAX when the
 * frame (12 bytes a pixel) or the sum does not fit a size_t.  The call allocates nothing, keeps no per-(device, stream)
 * state, needs no serialisation and only ENQUEUES 2L launches on `stream`.  out_f32_dev == color_dev (in place) is allowed:
 * the pyramid is read from color before the combine, in stream order.  Null params, color_dev or work_dev, all three outputs
 * null, a non-positive size, a NaN, infinite or out-of-range parameter, levels outside 1..8, a frame or bloom_out pointer
 * that is not 4-byte aligned, a misaligned work_dev, work_dev equal to any other buffer, bloom_out_dev equal to color_dev or
 * out_f32_dev, out_u8_dev equal to color_dev, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A frame
 * of 2^31 pixels or more: RTM_ERR_UNSUPPORTED, as rtm_tonemap.
 * Defaults: RTM_BLOOM_DEFAULTS below, the customary ones of this filter (what Renderer.Render(bloom=True) and rtm_cli --bloom
 * use).  Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
typedef struct rtm_bloom_params { /* 20 bytes */
    float threshold;   /* finite, >= 0: luminance above which a pixel blooms           */
    float knee;        /* in [0, 1]: the soft knee, as a fraction of the threshold     */
    float intensity;   /* finite, >= 0                                                  */
    float scatter;     /* in [0, 1]: how much of each coarser level reaches the finer  */
    int32_t levels;    /* L, 1..8                                                       */
} rtm_bloom_params;
#define RTM_BLOOM_DEFAULTS {1.0f, 0.5f, 0.2f, 0.7f, 6} /* of rtm_bloom_params */
size_t rtm_bloom_work_bytes(int32_t width, int32_t height, int32_t levels);
int rtm_bloom(const rtm_bloom_params* params, int32_t width, int32_t height, int device, const float* color_dev,
              void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, float* bloom_out_dev, void* stream);

/* ---- local tone operator: exposure fusion (Mertens et al.) on luminance — three synthetic exposures of the one frame, blended
 * per pixel by how well each is exposed, through a Laplacian pyramid so that the blend follows the frame's regions and not its
 * pixels.  Chroma is kept.  It REPLACES rtm_tonemap's curve: the output is display-linear, nominally in [0, 1], and rtm_tonemap
 * then runs as {CLAMP, transfer, auto_exposure 0, dither, ev 0} (one launch) for the transfer function and the store.  Opt-in:
 * every other stage and its defaults stay.
 * Input: color (DEVICE, height x width x 3 floats, RGB-interleaved like out_f32; 4-byte alignment is enough).  Arithmetic in
 * float, without contraction.  lum(c) = (0.2126 c_R + 0.7152 c_G) + 0.0722 c_B (rtm_tonemap's).
 *   1 counting    a pixel COUNTS iff its three components are finite.  A pixel that does not count is (0, 0, 0) for steps
 *                 2-6 and (0, 0, 0) in out_f32 and out_u8, as in rtm_tonemap: it is black for the pyramid and it is not
 *                 repaired (rtm_firefly upstream is the repair).
 *   2 exposed     xc = max(c, 0) per channel, Y = lum(xc), A = anchor (stats_dev ? stats_dev->exposure : 1),
 *     luminance   x = min(A Y, 1e6f).  stats_dev is a nullable DEVICE rtm_tonemap_stats that the kernels read: no host sync.
 *                 Filled by an earlier rtm_tonemap call on the same stream, it makes the anchor that call's own E.
 *   3 exposures   e_0 = exp2(shadows), e_1 = 1, e_2 = exp2(-highlights); I_k = (e_k x) / (1 + e_k x): simple Reinhard,
 *                 display-linear, in [0, 1).
 *   4 well-       v_k = sqrt(I_k), w_k = exp(-(v_k - 0.5)^2 / (2 sigma^2)), w^_k = w_k / (w_0 + w_1 + w_2).  With
 *     exposedness sigma >= 0.1 the exponent is >= -12.5: no w_k underflows and the sum is positive.
 *   5 pyramids    levels l = 0..L with rtm_bloom's sizes (W_l = ceil(W_{l-1} / 2), H_l likewise; a side that has reached 1
 *                 stays 1).  GI_0 = I and GW_0 = w^, three channels each; GI_l and GW_l are rtm_bloom's down filter (step 3
 *                 there) of level l-1: k = {1, 3, 3, 1} / 8 over the taps 2X-1 .. 2X+2, taps outside skipped and the rest
 *                 renormalised, the horizontal pass first.  up_l is rtm_bloom's up filter (step 4 there) from level l+1 to
 *                 W_l x H_l: the (1/4, 3/4) pair, skip and renormalise.
 *   6 blend and   R_L = sum_k GW_L,k GI_L,k; for l = L-1 .. 0: R_l = sum_k GW_l,k (GI_l,k - up_l(GI_{l+1,k})) + up_l(R_{l+1});
 *     collapse    F = min(max(R_0, 0), 1).  L = 0 is the pointwise blend F = sum_k w^_k I_k.
 *   7 apply       r = F / max(x, 1e-4f); out_f32 = xc (A r) per channel.  The luminance of a counting pixel with
 *                 1e-4 <= A Y <= 1e6 is F.  Above 1e6 the pixel is brighter than F, and the display transform's clamp takes it
 *                 to white.  An overflow is kept as the float it is.
 *   8 outputs     out_f32; out_u8 (nullable) is rtm_quantise of (double)out_f32, out of range (NaN included) -> 0, as in the
 *                 other stages; fused_out_dev (nullable, height x width floats) receives F at every pixel (at a pixel that
 *                 does not count: the F of a black pixel there).
 * It follows that (a) shadows = highlights = 0 gives F = x / (1 + x) at every L, within the tolerance: the three pyramids are
 * equal and the weights sum to one; (b) a constant frame gives, at every L, what L = 0 gives; (c) L = 0 is a pointwise
 * function of the pixel; (d) there are no atomics and no state: the same inputs give the same bits on every call, on any
 * stream, at any 4-byte alignment of color.
 * exp, sqrt, exp2 and the divisions may be the device's fast forms: against a float64 evaluation of the steps above every
 * out_f32 component and every fused_out value is within 1e-4 max(1, |ref|); out_u8 is exact given the call's own out_f32.
 * work_dev: DEVICE, 256-byte aligned, rtm_tonemap_local_work_bytes = the sum over l = 1..L of 2 round256(16 W_l H_l) bytes:
 * two planes of 16-byte records per level, (GI_0, GI_1, GI_2, R) and (GW_0, GW_1, GW_2, unused); level 0 is never stored.  0 for
 * a non-positive size, levels outside 0..8 and levels 0, SIZE_MAX when the frame (12 bytes a pixel) or the sum does not fit a
 * size_t.  levels 0 needs no work buffer and accepts a null work_dev.  The call allocates nothing, keeps no per-(device,
 * stream) state, needs no serialisation and only ENQUEUES 2L launches on `stream`, one for L = 0.  out_f32_dev == color_dev
 * (in place) is allowed: the apply kernel reads its pixel before it writes it, and the pyramid is read from color earlier, in
 * stream order.  Null params or color_dev, a null work_dev with levels > 0, all three outputs null, a non-positive size, a
 * NaN, infinite or out-of-range parameter, a float or stats pointer that is not 4-byte aligned, a work_dev that is not 256-byte
 * aligned, work_dev equal to any other buffer, fused_out_dev or stats_dev equal to color_dev or out_f32_dev, out_u8_dev equal
 * to color_dev, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A frame of 2^31 pixels or more:
 * RTM_ERR_UNSUPPORTED, as rtm_tonemap.
 * Defaults: RTM_TONEMAP_LOCAL_DEFAULTS below, the customary ones of this operator (what Renderer.Render(local=True) and
 * rtm_cli --display local use).  Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
typedef struct rtm_tonemap_local_params { /* 20 bytes */
    float anchor;      /* finite, > 0: the exposure in front of the operator                  */
    float shadows;     /* finite, in [0, 8]: stops the shadow exposure is opened by           */
    float highlights;  /* finite, in [0, 8]: stops the highlight exposure is closed by        */
    float sigma;       /* in [0.1, 1]: width of the well-exposedness weight about 0.5         */
    int32_t levels;    /* L, 0..8; 0 = the pointwise blend                                     */
} rtm_tonemap_local_params;
#define RTM_TONEMAP_LOCAL_DEFAULTS {1.0f, 2.0f, 2.0f, 0.25f, 5} /* of rtm_tonemap_local_params */
size_t rtm_tonemap_local_work_bytes(int32_t width, int32_t height, int32_t levels);
int rtm_tonemap_local(const rtm_tonemap_local_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                      const rtm_tonemap_stats* stats_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                      float* fused_out_dev, void* stream);

/* ---- grade: the colour decision — white balance (or any change of primaries) as a 3x3 matrix, exposure, contrast about a
 * pivot, the ASC CDL's slope / offset / power, saturation, and an optional 3D look LUT gathered on the device.  Opt-in, a
 * per-pixel transform of a device float frame: every other stage and its defaults stay.  The parametric steps are meant for
 * linear light, after rtm_bloom (glare is light, so it is added before the colour decision) and before rtm_tonemap; a look
 * LUT from a .cube file is display-referred and is meant for rtm_tonemap's float frame.  One call serves either or both.
 * Input: color (DEVICE, h x w x 3 floats, interleaved like out_f32; 4-byte alignment is enough).  lut (DEVICE, 3 N^3 floats
 * in .cube order, N = lut_size: entry (r, g, b) is the three floats at 3 (r + N (g + N b)), red fastest; the caller owns it;
 * null iff lut_size = 0).  The arithmetic is float, without contraction, in the order written; pow, exp2, log2 and the
 * divisions may be the device's fast forms.
 * A pixel COUNTS iff its three components are finite.  A pixel that does not count is copied to out_f32 word for word: the
 * stage does not repair, and rtm_tonemap downstream still sees the pixel as not counting.
 * A step whose parameters all equal their defaults exactly (float ==, so -0 equals 0) is SKIPPED; the host decides this
 * before the launch.  So RTM_GRADE_DEFAULTS copies every word of the frame bit for bit, -0 and NaN payloads included, and a
 * skipped step rounds nothing.  For a counting pixel (r, g, b), in this order:
 *   1 matrix      y_i = (m[3i] r + m[3i+1] g) + m[3i+2] b, m = matrix, row-major.  Default: the identity.
 *   2 exposure    y = y G, G = (float)exp2((double)exposure), computed on the host.  Default: 0 stops.
 *   3 contrast    y = pivot pow(max(y, 0) / pivot, contrast) per channel: a power curve through (pivot, pivot); it clips
 *                 negative components to 0.  Defaults: contrast 1 at pivot 0.18 (both are the step's parameters: contrast 1
 *                 at another pivot is a live step, which only clips).
 *   4 CDL         per channel c: v = max(y slope_c + offset_c, 0), the product rounded, then the sum; y = v when
 *                 power_c == 1, else pow(v, power_c), with pow(0, p) = 0.  Defaults: slope 1, offset 0, power 1.
 *   5 saturation  L = (0.2126 y_R + 0.7152 y_G) + 0.0722 y_B (the library's luminance); y = L + saturation (y - L).
 *                 Default: 1.  0 gives r = g = b = L.
 *   6 LUT         (lut_size = N > 0) per channel c: s = (y - lo_c) inv_c with lo = lut_min, hi = lut_max and
 *                 inv_c = (float)((double)(N - 1) / ((double)hi_c - (double)lo_c)) computed on the host;
 *                 s = (s > 0) ? min(s, N - 1) : 0, so a NaN lands on 0 and +inf on N - 1; i = min((int)s, N - 2),
 *                 f = s - i, in [0, 1].  With c_abc the entry at (i_R + a, i_G + b, i_B + c):
 *                 TRILINEAR   the eight corners, blended along r, then g, then b, each blend as a + f (b - a).
 *                 TETRAHEDRAL the three fractions in descending order f1 >= f2 >= f3, a tie taking the earlier channel
 *                             first; c_1 is c000 moved one step along the first channel, c_2 along the first two;
 *                             out = (((1 - f1) c000 + (f1 - f2) c_1) + (f2 - f3) c_2) + f3 c111.
 *                 Both interpolants are continuous across cells and tetrahedra, both return a lattice point's entry at the
 *                 lattice point, and both reproduce an affine table.
 *   7 outputs     out_f32 is the result; out_u8 (nullable) is rtm_quantise of (double)out_f32, out of range (NaN included)
 *                 -> 0, as in the other stages.
 * Memory safety is part of the contract: for ANY input words and any accepted parameters, every read of lut lies inside its
 * 3 N^3 floats; that is what the clamp of step 6 is written for.  An intermediate overflow (an infinity, or the NaN of
 * inf - inf in step 5) gives IEEE's result without a LUT and a table entry with one.
 * Against a float64 evaluation of the steps with the float-rounded G, inv_c and parameters, every out_f32 component of a
 * counting pixel is within 1e-4 max(1, |ref|); pixels that do not count and the all-defaults copy are exact; out_u8 is exact
 * given the call's own out_f32.  The call is stateless: no work buffer, no allocation, no per-(device, stream) state, no
 * serialisation, no atomics; it only ENQUEUES one launch on `stream` of `device`, and the same inputs give the same bits on
 * every call, on any stream, at any 4-byte alignment of color and out_f32.  out_f32_dev == color_dev grades in place, with
 * the same bits as out of place.
 * Null params or color_dev, both outputs null, a non-positive size, a parameter that is NaN, infinite or outside its range
 * (|exposure| <= 32, contrast in [0.25, 4], pivot > 0, slope >= 0, power in [0.1, 10], saturation in [0, 4]; matrix, offset,
 * lut_min and lut_max finite), lut_size neither 0 nor in 2..256, lut_interp out of range, lut_max_c <= lut_min_c, lut_dev
 * null with lut_size > 0 or non-null with lut_size = 0, a float pointer that is not 4-byte aligned, lut_dev equal to an
 * output, out_u8_dev == color_dev, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A frame of 2^31
 * pixels or more: RTM_ERR_UNSUPPORTED.
 * rtm_grade_white_balance (HOST only, no device call) gives the matrix for step 1 that takes a scene lit by a black body at
 * `kelvin` to D65: the Bradford adaptation from that white to D65 (0.3127, 0.3290), expressed in linear Rec.709 / sRGB
 * primaries, computed in double and rounded to float; the source white's linear RGB maps to three equal components.  The
 * source white is Kang et al.'s (2002) cubic approximation of the Planckian locus, T = kelvin:
 *   T <= 4000: x = -0.2661239e9 / T^3 - 0.2343589e6 / T^2 + 0.8776956e3 / T + 0.179910, otherwise
 *              x = -3.0258469e9 / T^3 + 2.1070379e6 / T^2 + 0.2226347e3 / T + 0.240390;
 *   T <= 2222: y = -1.1063814 x^3 - 1.34811020 x^2 + 2.18555832 x - 0.20219683,
 *   T <= 4000: y = -0.9549476 x^3 - 1.37418593 x^2 + 2.09137015 x - 0.16748867, otherwise
 *              y =  3.0817580 x^3 - 5.87338670 x^2 + 3.75112997 x - 0.37001483.
 * `tint` is added to v in CIE 1960 (u, v): u = 4x / (-2x + 12y + 3), v = 6y / (-2x + 12y + 3) + tint, and back
 * x = 3u / (2u - 8v + 4), y = 2v / (2u - 8v + 4); a positive tint is a greener source.  The RGB <-> XYZ matrices are derived
 * from the Rec.709 primaries and D65; the cone response matrix is Bradford's.  kelvin in [1667, 25000], tint in
 * [-0.05, 0.05]; a value out of range or not finite, or a null pointer: RTM_ERR_INVALID_ARGUMENT.
 * rtm_lut_parse_cube / rtm_lut_load_cube (HOST only) read a 3D LUT in the Adobe / Resolve .cube text format, shaped like
 * the scene loaders: `size` receives N, domain_min / domain_max the input domain per channel, `table` (capacity in floats)
 * the 3 N^3 floats in the file's order, which is rtm_grade's; a null table with capacity 0 asks for the size and checks the
 * whole text all the same.  Lines end in LF or CR LF; blank lines and lines that begin with # are skipped; TITLE "..." is
 * ignored; LUT_3D_SIZE N; DOMAIN_MIN and DOMAIN_MAX with three numbers each (defaults 0 and 1); LUT_3D_INPUT_RANGE lo hi
 * sets all three channels; then exactly N^3 rows of three numbers, each a decimal number that is finite as a float.
 * RTM_ERR_PARSE, with "line K: ..." in rtm_last_error_detail(): an unknown keyword, a keyword after the first row, a size
 * that is not a whole number in 2..256 or is given twice, a row before the size, a token that is no such number, a line with
 * too few or too many numbers, more than N^3 rows, fewer (K is then the last line), no size at all, a domain with
 * max <= min (K is the last domain line).  LUT_1D_SIZE or LUT_1D_INPUT_RANGE: RTM_ERR_UNSUPPORTED.  A file that cannot be
 * opened: RTM_ERR_IO.  A table with capacity < 3 N^3: RTM_ERR_CAPACITY (size and the domain are set).  A null text with a
 * length, a null path, size or domain pointer, a null table with a capacity: RTM_ERR_INVALID_ARGUMENT.
 * Defaults: RTM_GRADE_DEFAULTS below.  Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
enum { RTM_GRADE_TRILINEAR = 0, RTM_GRADE_TETRAHEDRAL = 1 }; /* lut_interp */
typedef struct rtm_grade_params { /* 120 bytes */
    float matrix[9];    /* row-major 3x3, finite: white balance, any change of primaries                  */
    float exposure;     /* stops, finite, |ev| <= 32                                                      */
    float contrast;     /* in [0.25, 4]                                                                   */
    float pivot;        /* finite, > 0: the value the contrast curve leaves where it is                   */
    float slope[3];     /* ASC CDL: finite, >= 0                                                          */
    float offset[3];    /* finite                                                                         */
    float power[3];     /* in [0.1, 10]                                                                   */
    float saturation;   /* in [0, 4]                                                                      */
    int32_t lut_size;   /* 0: no LUT; else N in 2..256                                                    */
    int32_t lut_interp; /* RTM_GRADE_*                                                                    */
    float lut_min[3];   /* the LUT's input domain per channel, finite                                     */
    float lut_max[3];   /* ... max > min                                                                  */
} rtm_grade_params;
#define RTM_GRADE_DEFAULTS                                                                                               \
    {{1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, 0.0f, 1.0f, 0.18f, {1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f},     \
     {1.0f, 1.0f, 1.0f}, 1.0f, 0, RTM_GRADE_TETRAHEDRAL, {0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}}
int rtm_grade(const rtm_grade_params* params, int32_t width, int32_t height, int device, const float* color_dev,
              const float* lut_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream);
int rtm_grade_white_balance(float kelvin, float tint, float matrix_out[9]); /* host only */
int rtm_lut_parse_cube(const char* text, size_t len, int32_t* size, float domain_min[3], float domain_max[3], float* table,
                       size_t capacity); /* host only */
int rtm_lut_load_cube(const char* path, int32_t* size, float domain_min[3], float domain_max[3], float* table,
                      size_t capacity); /* host only */

/* ---- depth of field (defocus): a focus distance and an aperture applied to a finished frame by its depth plane — a
 * depth-aware gather blur (scatter-as-gather) whose per-pixel circle of confusion follows the thin-lens law.  A focused
 * foreground stays sharp against a blurred background; a blurred foreground spills over what is behind it.  Opt-in, after the
 * denoisers and before rtm_bloom (glare forms behind the lens) and rtm_tonemap: every other stage and its defaults stay.
 * Inputs: color (DEVICE, height x width x 3 floats, RGB-interleaved like out_f32; 4-byte alignment is enough) and depth
 * (DEVICE, height x width floats, as rtm_render_aov writes it: positive, +inf on a miss).  Depth is the distance along the
 * primary ray, so the surface in focus is a sphere around the camera's origin, not a plane: build-defined, the reference has
 * no lens.  Arithmetic in float, without contraction.  zf = focus_distance, A = aperture, R = max_radius, pi_f = (float)pi.
 *   1 counting   a pixel COUNTS iff its three colour components are finite and its depth is > 0 (+inf counts; NaN, 0 and
 *                negative do not).  A pixel that does not count contributes to no other pixel; its out_f32 is its input, bit
 *                for bit, its coc_out is +0 and its out_u8 the usual store of its own out_f32.
 *   2 circle     s = A max(1 - zf / z, -FLT_MAX); for z = +inf the quotient is +0, so s = A; a quotient that overflows (a
 *                depth tiny against zf) counts as the largest float, so that A = 0 gives -0 and never NaN.  s is clamped to
 *                [-R, R]: negative in front of the focus, positive behind it.  r = |s|, m = max(r, 0.5f), ia = 1 / ((pi_f m) m): the reciprocal area of
 *                the pixel's disc; the floor of half a pixel makes a sharp pixel a disc of one pixel.
 *   3 taps       q = p + (dx, dy), dx and dy in -R..R.  Taps outside the frame or not counting are skipped, not clamped (the
 *                library's skip-and-renormalise rule).  d = sqrtf((float)(dx dx + dy dy)).
 *   4 which disc behind = z_q > z_p, as the floats they are (+inf > finite is true, inf > inf is false);
 *                (r_e, ia_e) = (behind && r_p < r_q) ? (r_p, ia_p) : (r_q, ia_q).  A tap in front of p spreads over p with its
 *                own disc; a tap behind p spreads no further than p's own blur, so a focused foreground does not take on its
 *                background.
 *   5 weight     w = min(max(r_e + 0.5f - d, 0), 1) ia_e: a disc with a one-pixel linear edge, continuous in every input.
 *                The centre tap always has w > 0.
 *   6 combine    out = (sum of w c_q) / (sum of w) per channel.  If no tap other than the centre has w > 0, out is the input,
 *                bit for bit.  Taps whose weight is +0 may be skipped: adding +0 changes no sum.  The order of the sums is
 *                the implementation's (rows, then columns), but fixed: the same inputs give the same bits on every call, on
 *                any stream, at any alignment of color.  No atomics.
 *   7 outputs    coc_out_dev (nullable, height x width floats) receives s.  out_u8 (nullable) is rtm_quantise of
 *                (double)out_f32, out of range (NaN included) -> 0, as in the other stages.
 * It follows that aperture = 0 returns every pixel bit for bit (every r is 0, and every non-centre weight +0); that a frame
 * of one constant colour over any depths stays that colour, within the tolerance; and that a pixel with r_p = 0 whose nearer
 * neighbours all have r = 0 keeps its words, however blurred what lies behind it.
 * The divisions and the reciprocal may be the device's fast forms: against a float64 evaluation of the steps above every
 * out_f32 component of a counting pixel and every coc_out value is within 1e-4 max(1, |ref|); out_u8 is exact given the
 * call's own out_f32.
 * The call keeps no state, allocates nothing, needs no work buffer and no serialisation, and only ENQUEUES one launch on
 * `stream`.  Null params, color_dev or depth_dev, all three outputs null, a non-positive size, a focus_distance that is NaN,
 * infinite or not positive, an aperture that is NaN, infinite or negative, max_radius outside 1..16, a float pointer that is
 * not 4-byte aligned, any output equal to color_dev or depth_dev (a gather cannot run in place), coc_out_dev equal to
 * out_f32_dev, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A frame of 2^31 pixels or more, or
 * one of 2^23 or more tiles of 32 x 16 pixels (ceil(width / 32) ceil(height / 16): a launch has one 512-lane block a tile,
 * so a frame thinner than a tile reaches the launch's limit of 2^32 lanes first): RTM_ERR_UNSUPPORTED, as rtm_tonemap.
 * Defaults: RTM_DEFOCUS_DEFAULTS below (what Renderer.Render(dof=True) and rtm_cli --dof use, with the focus at the camera's
 * target distance).  Added after RTM_ABI_VERSION 5 without changing it: callers look the symbol up. */
typedef struct rtm_defocus_params { /* 12 bytes */
    float focus_distance; /* zf: finite, > 0, in depth's units.  No default: 0 is refused                                */
    float aperture;       /* A: finite, >= 0: the blur radius, in pixels, of a point at infinity.  The thin lens's       */
                          /* f^2 / (N (zf - f)) and the pixel pitch are folded into it                                   */
    int32_t max_radius;   /* R: 1..16, in pixels: radii are clamped to it and the window is (2R+1)^2                     */
} rtm_defocus_params;
#define RTM_DEFOCUS_DEFAULTS {0.0f, 4.0f, 8} /* of rtm_defocus_params; the caller sets focus_distance */
int rtm_defocus(const rtm_defocus_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                const float* depth_dev, float* out_f32_dev, uint8_t* out_u8_dev, float* coc_out_dev, void* stream);

/* ---- lens: radial distortion, lateral chromatic aberration and vignetting of a frame or a single-channel plane — a traced
 * frame given the distortion of a plate's lens (DIRECT), a plate's distortion taken out (INVERSE), the AOV planes (depth,
 * ids, mattes, alpha) warped consistently with the frame (NEAREST).  Opt-in, after rtm_defocus and before rtm_resize,
 * rtm_bloom and rtm_tonemap, in linear light: every other stage and its defaults stay.  The one stage that resamples at
 * per-pixel positions; input and output have the same size.
 * Input: src (DEVICE, h x w x C floats, C = channels in {1, 3}, interleaved like out_f32; 4-byte alignment is enough).
 *   1 positions  in double, in the order written, without contraction, so that a float64 restatement reproduces every
 *                position bit for bit; k1, k2, zoom and chroma are widened from float first.  For destination pixel (X, Y):
 *                cx = w / 2, cy = h / 2; dx = (X + 0.5) - cx, dy = (Y + 0.5) - cy; R2 = cx cx + cy cy; iz = 1.0 / zoom;
 *                r2 = ((dx dx + dy dy) / R2) (iz iz), the squared radius normalised to the half diagonal, after the zoom.
 *                DIRECT:  F = (1 + r2 (k1 + r2 k2)) iz.
 *                INVERSE: r = sqrt(r2); rho solves rho g(rho^2) = r, g(t) = 1 + t (k1 + t k2), by exactly 12 Newton steps
 *                from rho = r, each t = rho rho; rho = rho - (rho (1 + t (k1 + t k2)) - r) / (1 + t (3 k1 + t (5 k2)));
 *                F = (r > 0 ? rho / r : 1.0) iz.
 *                Channel c has m_c = 1 + chroma (1 - c) for C = 3 (R is scaled by 1 + chroma, G by 1, B by 1 - chroma) and
 *                m = 1 for C = 1; F_c = F m_c; u = cx + dx F_c - 0.5, v = cy + dy F_c - 0.5: source pixel coordinates.
 *                With the defaults F_c = 1.0 and u = X exactly.  DIRECT shows, at p, the source at p g(|p|^2); INVERSE the
 *                source at D^-1(p): DIRECT and then INVERSE with the same k1, k2 (zoom 1, chroma 0) is the identity map.
 *   2 border     a channel is INSIDE iff -0.5 <= u < w - 0.5 and -0.5 <= v < h - 0.5 (a NaN position is outside).  Otherwise
 *                its output is border[c]'s word, bit for bit, and nothing else touches it (no vignette).
 *   3 taps       a source pixel COUNTS iff all its C components are finite.  A tap outside the frame or one that does not
 *                count is skipped, not clamped: the library's skip-and-renormalise rule.  fx = floor(u), t = u - fx, rows
 *                alike.  BILINEAR: taps fx, fx + 1 with weights (1 - t, t).  BICUBIC (Catmull-Rom, which interpolates, so the
 *                identity is exact): taps fx - 1 .. fx + 2 with w0 = (((2 - t) t - 1) t) / 2, w1 = (((3 t - 5) t) t + 2) / 2,
 *                w2 = (((4 - 3 t) t + 1) t) / 2, w3 = (((t - 1) t) t) / 2.  The weights are evaluated in double and rounded
 *                to float.  Then in float, without contraction, rows outer, columns inner, ascending: w = w^x_i w^y_j,
 *                N = sum w c_q, D = sum w over the contributing taps; out = N / D when D >= 0.0625f, otherwise a quiet NaN:
 *                the stage does not repair, and rtm_tonemap downstream still sees the pixel as not counting.  A frame whose
 *                pixels all count never meets the threshold: every per-axis sum is 0.5 or more.
 *   4 nearest    NEAREST copies the word of source pixel (floor(u + 0.5), floor(v + 0.5)) bit for bit, with no counting test
 *                (an index that the rounding of u + 0.5 brings to w or h is w - 1 or h - 1): an int32 id plane viewed as
 *                floats, a depth plane with +inf and a NaN all pass through.  border[] is not checked for finiteness with
 *                NEAREST, so an id plane can take the word of -1.
 *   5 vignette   after resampling, inside channels only, in float: rv = (float)((dx dx + dy dy) / R2) (the division in
 *                double), q = 1 + (falloff falloff) rv, c4 = 1 / (q q), gain = 1 - vignette (1 - c4), out = out gain: the
 *                cos^4 law of a lens whose half field angle at the frame's corner has the tangent `falloff`.  vignette = 0
 *                gives gain = 1 exactly.  (NEAREST takes no vignette: it copies words.)
 *   6 outputs    out_u8 (nullable) is rtm_quantise of (double)out_f32, out of range (NaN included) -> 0, as in the other
 *                stages.
 * It follows that the defaults, in either mode and with any filter, return every counting pixel == its input, and every
 * word with NEAREST; and that a constant frame stays that constant at every inside pixel, within the tolerance, for any
 * parameters with vignette = 0.
 * The division N / D may be the device's fast form: against a float64 evaluation with the float-rounded weights every inside
 * out_f32 component is within 1e-4 max(1, |ref|); NEAREST, which channels are inside and the border words are exact; where
 * the output is NaN is exact for inputs whose reference D stays 1e-3 away from 1/16; out_u8 is exact given the call's own
 * out_f32.  The call is stateless: no work buffer, no allocation, no per-(device, stream) state, no serialisation, no
 * atomics; it only ENQUEUES one launch on `stream` of `device`, and the same inputs give the same bits on every call, on any
 * stream, at any 4-byte alignment of src and out_f32.
 * Null params or src_dev, both outputs null, a non-positive size, a parameter that is NaN, infinite or outside its range
 * (|k1| <= 0.5, |k2| <= 0.25, zoom in [0.25, 4], chroma in [-0.05, 0.05], vignette in [0, 1], falloff in [0, 4]), a
 * non-finite border with a filter other than NEAREST, mode, filter or channels out of range, chroma != 0 with channels = 1,
 * NEAREST with chroma != 0 or vignette != 0, a float pointer that is not 4-byte aligned, an output equal to src_dev (a gather
 * cannot run in place), a negative device, a radial map that folds over: RTM_ERR_INVALID_ARGUMENT, before any device call.
 * The fold-over check, in double on the host: a = 3 k1, b = 5 k2, T = iz iz for DIRECT and 4 (iz iz) for INVERSE (the
 * solve may look as far as rho = 2 iz); d(t) = 1 + t (a + t b), the derivative of rho g(rho^2) at t = rho^2, must be 0.25
 * or more at t = T and, when b != 0 and tv = -a / (2 b) lies in 0 < tv < T, at tv (d(0) = 1); INVERSE also needs
 * 1 + T (k1 + T k2) >= 0.5, so that a root exists in [0, 2 iz].
 * A frame of 2^31 pixels or more, or of 2^24 tiles of 64 x 4 or more (a launch holds fewer than 2^32 lanes):
 * RTM_ERR_UNSUPPORTED.
 * rtm_lens_fit_zoom (HOST only, no device call) gives the zoom that hides the border: P(z) is true iff the parameters with
 * zoom = z pass the fold-over check and every pixel of the frame's outermost rows and columns has all its channels inside,
 * by the arithmetic of step 1.  lo = 0.25f, hi = 4.0f; if P(lo) the result is lo; if not P(hi): RTM_ERR_UNSUPPORTED;
 * otherwise 24 times mid = (lo + hi) 0.5f in float, hi = mid if P(mid), else lo = mid, and the result is hi.  P is monotone
 * in z, because the radial map is increasing wherever the check passes.  It reads k1, k2, chroma, mode and channels only
 * (params->zoom is ignored) and holds k1, k2 and chroma to no range: a lens that no zoom in [0.25, 4] serves has no fit and
 * gives RTM_ERR_UNSUPPORTED (no parameters that rtm_lens accepts get there: P(4) holds for all of them).  Null params or
 * zoom_out, a non-positive size, a NaN or infinite k1, k2 or chroma, mode or channels out of range, chroma != 0 with
 * channels = 1: RTM_ERR_INVALID_ARGUMENT; a frame of 2^31 pixels or more: RTM_ERR_UNSUPPORTED.
 * Defaults: RTM_LENS_DEFAULTS below.  Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
enum { RTM_LENS_NEAREST = 0, RTM_LENS_BILINEAR = 1, RTM_LENS_BICUBIC = 2 }; /* filter */
enum { RTM_LENS_DIRECT = 0, RTM_LENS_INVERSE = 1 };                         /* mode   */
typedef struct rtm_lens_params { /* 48 bytes */
    float k1, k2;     /* radial polynomial g(t) = 1 + t (k1 + t k2), t = squared normalised radius; |k1| <= 0.5, |k2| <= 0.25 */
    float zoom;       /* in [0.25, 4]: magnification about the centre, applied before the polynomial                        */
    float chroma;     /* in [-0.05, 0.05]: lateral chromatic aberration; R is scaled by 1 + chroma, G by 1, B by 1 - chroma  */
    float vignette;   /* amount in [0, 1]                                                                                    */
    float falloff;    /* in [0, 4]: tan of the half field angle at the frame's corner (cos^4 law)                            */
    float border[3];  /* written, bit for bit, where a channel's source position lies outside the frame                      */
    int32_t mode;     /* RTM_LENS_DIRECT / RTM_LENS_INVERSE                                                                  */
    int32_t filter;   /* RTM_LENS_*                                                                                          */
    int32_t channels; /* C: 1 (a plane) or 3 (a frame)                                                                       */
} rtm_lens_params;
#define RTM_LENS_DEFAULTS {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, {0.0f, 0.0f, 0.0f}, RTM_LENS_DIRECT, RTM_LENS_BICUBIC, 3}
int rtm_lens(const rtm_lens_params* params, int32_t width, int32_t height, int device, const float* src_dev,
             float* out_f32_dev, uint8_t* out_u8_dev, void* stream);
int rtm_lens_fit_zoom(const rtm_lens_params* params, int32_t width, int32_t height, float* zoom_out); /* host only */

/* ---- resize: a frame or a single-channel plane brought to another size by a separable filter — thumbnails, a 4K trace
 * filtered down to 1080p, a plane (alpha, matte, variance, spp map) brought beside a frame of another size.  Opt-in, after
 * rtm_defocus and before rtm_bloom and rtm_tonemap, in linear light: every other stage and its defaults stay.  It is for
 * radiance-like and coverage-like planes: depth, object ids and normals must not be averaged.
 * Input: src (DEVICE, h x w x C floats, C = channels in {1, 3}, interleaved like out_f32; 4-byte alignment is enough).
 * Output: H x W x C.  Any W, H >= 1; the axes are independent (an enlargement in x with a reduction in y is legal).
 *   1 kernels    k(t) with half-width r.  BOX: r = 1/2, k = 1 on -1/2 < t <= 1/2.  TRIANGLE: r = 1, k = max(0, 1 - |t|).
 *                MITCHELL (B = C = 1/3): r = 2, k = (7|t|^3 - 12|t|^2 + 16/3) / 6 for |t| < 1 and
 *                (-7/3 |t|^3 + 12|t|^2 - 20|t| + 32/3) / 6 for 1 <= |t| < 2.  LANCZOS3: r = 3, k(0) = 1, otherwise
 *                k = sinc(pi t) sinc(pi t / 3) for |t| < 3, sinc(x) = sin x / x.  Every kernel is 0 outside its support.
 *   2 taps       per axis, all positions in integers.  n is the source length, N the destination length, M = max(n, N),
 *                q = 2r in {1, 2, 4, 6}.  When reducing, the kernel is stretched by M / N (the antialiasing); when enlarging
 *                it is not.  T = ceil(q M / N) taps per destination index.  For destination index X:
 *                b = (2X + 1) n - N (the centre is u = b / 2N in source pixel coordinates: (X + 1/2) n/N = u + 1/2);
 *                j0 = floor((b - q M) / (2N)) + 1, floor toward minus infinity; tap i = 0..T-1 is source index j = j0 + i;
 *                a = 2N j - b in 64-bit integers; t = a / (2M), one double division.  BOX is decided in integers: k = 1
 *                iff -M < a <= M.  These T taps are exactly the integers in (u - rM/N, u + rM/N], and the raw weights of
 *                every X have a positive sum.
 *   3 tables     w^[X][i] = k(t_i) / (sum over all T taps, in the frame or not, of k(t)), evaluated in double and rounded
 *                to float, by a device kernel (its double sin) into the work buffer.
 *   4 counting   a source pixel COUNTS iff all its C components are finite: m = 1, else m = 0.  A pixel that does not
 *                count contributes nothing (it is selected out, not multiplied by zero); a tap outside the frame is skipped.
 *   5 horizontal arithmetic in float, without contraction, taps ascending: for every source row y and destination column
 *                X the record (sum_i w^x[X][i] m c_k for each channel k, sum_i w^x[X][i] m): 16 bytes for C = 3, 8 for C = 1.
 *   6 vertical   Nk = sum_i w^y[Y][i] rec_k(j0y + i, X), taps ascending, and D likewise from the records' last field, over
 *                the rows inside the frame.  out_k = Nk / D when D >= 0.0625f; otherwise every channel of the pixel is a
 *                quiet NaN: resize does not repair, and rtm_tonemap downstream still sees the pixel as not counting.  This
 *                is skip-and-renormalise written as a normalised convolution, which keeps it separable around holes.  A
 *                frame whose pixels all count never meets the threshold (every per-axis sum is above 0.5).
 *   7 outputs    out_u8 (nullable) is rtm_quantise of (double)out_f32, out of range (NaN included) -> 0, as in the other
 *                stages.  MITCHELL and LANCZOS3 have negative lobes: an output may undershoot 0 next to a bright edge (or
 *                overshoot); nothing here clamps, the stages downstream (rtm_tonemap, rtm_quantise) already do.
 * It follows that W = w, H = h with BOX or TRIANGLE returns every counting pixel == its input (the tables are exactly
 * {0, 1}; MITCHELL at equal size is a blur by design, LANCZOS3 the input within the tolerance); that a constant frame stays
 * that constant at any size pair and filter, also around holes wherever D >= 1/16; and that BOX at w = fW, h = fH is the
 * mean of each f x f block.
 * The divisions may be the device's fast forms: against a float64 evaluation with the float-rounded tables every out_f32
 * component is within 1e-4 max(1, |ref|); where the output is NaN is exact for inputs whose reference D stays 1e-3 away
 * from 1/16; out_u8 is exact given the call's own out_f32.  No atomics: the same inputs give the same bits on every call,
 * on any stream, at any 4-byte alignment of src and out_f32.
 * work_dev (DEVICE, 256-byte aligned) holds rtm_resize_work_bytes = round256(rec W h) + round256(4 W Tx) + round256(4 H Ty)
 * + round256(4 (W + H)) bytes: the records (rec = 16 for C = 3, 8 for C = 1), the two tables and the two j0 arrays.  It
 * returns 0 for a non-positive size or a filter or channels out of range, SIZE_MAX when a term or the sum does not fit a
 * size_t.  The call allocates nothing, keeps no per-(device, stream) state, needs no serialisation and only ENQUEUES three
 * launches on `stream` of `device`: tables, horizontal, vertical.
 * Null params, src_dev or work_dev, both outputs null, a non-positive size, filter outside 0..3, channels not 1 or 3, a
 * float pointer that is not 4-byte aligned, a work_dev that is not 256-byte aligned or equal to any other buffer,
 * out_f32_dev or out_u8_dev equal to src_dev (a gather cannot run in place), a negative device: RTM_ERR_INVALID_ARGUMENT,
 * before any device call.  w h, W H or W h (the intermediate) of 2^31 or more: RTM_ERR_UNSUPPORTED, as rtm_tonemap; so is
 * an axis with q max(n, N) of 2^31 or more (a side of 3.5e8 pixels for LANCZOS3), whose first tap or tap count would leave 32 bits.
 * Defaults: RTM_RESIZE_DEFAULTS below.  Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
enum { RTM_RESIZE_BOX = 0, RTM_RESIZE_TRIANGLE = 1, RTM_RESIZE_MITCHELL = 2, RTM_RESIZE_LANCZOS3 = 3 };
typedef struct rtm_resize_params { /* 8 bytes */
    int32_t filter;   /* RTM_RESIZE_*                                                                                     */
    int32_t channels; /* C: 1 (a plane) or 3 (a frame)                                                                    */
} rtm_resize_params;
#define RTM_RESIZE_DEFAULTS {RTM_RESIZE_MITCHELL, 3}
size_t rtm_resize_work_bytes(int32_t src_width, int32_t src_height, int32_t dst_width, int32_t dst_height, int32_t filter,
                             int32_t channels);
int rtm_resize(const rtm_resize_params* params, int32_t src_width, int32_t src_height, int32_t dst_width, int32_t dst_height,
               int device, const float* src_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream);

/* ---- AOV-guided upsampling: a frame traced at 1/f of the resolution in each axis, brought to full size by a joint
 * bilateral upsample (Kopf et al. 2007) steered by the full-resolution first-hit planes, with the albedo demodulated so that
 * material colour comes back at full resolution.  The AOVs have no random draws and cost one cheap kernel at any size; the
 * path-traced colour needs f^2 fewer paths.
 * Inputs: the low frame is w x h, the output W x H with W = f w, H = f h.  color_low (DEVICE, h x w x 3 floats,
 * RGB-interleaved like out_f32); guide_low in the rtm_aov_buffers layout at w x h and guide_high in the same layout at W x H
 * (rows = the frame's height, no bands).  A plane (depth, normal, albedo, object) is GIVEN iff it is non-null in both guide
 * structs; either struct pointer may be null (no planes at all), and then both must be.  Depths are positive or +inf, as
 * rtm_render_aov writes them.  Arithmetic in float:
 *   1 taps        in integers.  For the output column x: num = 2x + 1 - f, X0 = floor(num / 2f) (floor division: a negative
 *                 num rounds down), r = num - 2f X0 in [0, 2f), t_x = r / (2f); rows alike.  (X0 + t_x is the pixel centre
 *                 (x + 0.5) / f - 0.5 in low-resolution pixel coordinates.)  The taps are the low pixels
 *                 q = (X0 + dx, Y0 + dy), dx, dy in -1..2; taps outside the low frame are skipped (not clamped); the sums run
 *                 dy outer, dx inner.  The tap nearest to the pixel centre is always inside the frame.
 *   2 spatial     h_x[dx] = exp(-(dx - t_x)^2 / (2 sigma_spatial^2)); it depends only on x mod f, so there are 4f values
 *                 per axis: computed in double on the host, rounded to float, one table for both axes.
 *                 h(p,q) = h_x[dx] h_y[dy].
 *   3 geometry    g(p,q), rtm_denoise's weight with step s = f; p the full-resolution pixel with the high guides, q the
 *                 low tap with the low guides:
 *                   object given and obj_p != obj_q: 0
 *                   else, depth given: both depths +inf (two misses): 1, the terms below skipped; exactly one +inf: 0;
 *                         otherwise w_z = sigma_depth > 0 ? exp(-|z_p - z_q| / (sigma_depth f max(z_p, z_q))) : 1
 *                   w_n = (normal given && sigma_normal > 0) ? max(0, n_p . n_q)^sigma_normal : 1;  g = w_z w_n
 *                 There is no centre-tap case: no tap coincides with p.
 *   4 combine     w(p,q) = h(p,q) (g(p,q) + 1e-6f): a continuous fallback, no threshold.  a_q,k = albedo_q,k > 1e-3f ?
 *                 albedo_q,k : 1.0f from the LOW albedo (1.0f when albedo is not given), e_q = c_q / a_q per channel;
 *                 e^_p = sum_q w e_q / sum_q w;  out_p = e^_p A_p, A built the same way from the HIGH albedo.
 *                 A full-resolution pixel whose object no tap saw (a thin feature) gets the spatial average of its taps;
 *                 a pixel whose nearest tap carries its object with g = 1 takes, at the default sigma_spatial, under 1e-5
 *                 of its value from across an edge (DESIGN.md has the bound).  sum w > 0 always: never a division by zero.
 *   out_u8 (if non-null) is rtm_quantise of (double)out_f32, bit for bit.
 * exp, pow and the divisions may be the device's fast forms: against a float64 evaluation of the steps above every output
 * component is within 1e-4 max(1, |ref|).  No atomics: the same inputs give the same bits on every call, on any stream.
 * Defaults: RTM_UPSAMPLE_DEFAULTS below (what Renderer.preview and rtm_cli --preview use; the sigma_spatial sweep on the
 * Cornell box: DESIGN.md): factor 2, sigma_spatial 0.5, sigma_normal 64, sigma_depth 0.05. */
typedef struct rtm_upsample_params {
    int32_t factor;       /* f, 2..8: the full frame is (f w) x (f h) */
    float sigma_spatial;  /* finite, 0.25..4, in low-resolution pixels */
    float sigma_normal;   /* as rtm_denoise_params */
    float sigma_depth;    /* as rtm_denoise_params */
} rtm_upsample_params;
#define RTM_UPSAMPLE_DEFAULTS {2, 0.5f, 64.0f, 0.05f} /* an initializer of rtm_upsample_params */
/* Bytes of the work buffer rtm_upsample needs for a low frame: 32 per low pixel (two 16-byte records, (e.xyz, object bits)
 * and (n.xyz, z), packed by a prepass like the denoiser's); 0 for a non-positive size, SIZE_MAX when the full frame at
 * f = 8 (12 x 64 bytes per low pixel) does not fit a size_t. */
size_t rtm_upsample_work_bytes(int32_t low_width, int32_t low_height);
/* Upsamples `color_low_dev` into out_f32_dev and / or out_u8_dev (DEVICE, (f h) x (f w) x 3; either may be null, not
 * both).  The caller owns every buffer; work_dev (DEVICE, 16-byte aligned, rtm_upsample_work_bytes bytes) holds the packed
 * low records, so the call allocates nothing and only ENQUEUES its two launches (the low-resolution prepass and the
 * upsample) on `stream` of `device`.  It keeps no per-(device, stream) state and needs no serialisation: calls on different
 * streams with different work buffers run side by side.  Null params, color_low_dev or work_dev, both outputs null, a
 * non-positive size, factor outside 2..8, sigma_spatial outside [0.25, 4] or not finite, a negative, NaN or infinite
 * sigma_normal or sigma_depth, a plane (or a guide struct) given at one resolution only, a misaligned work_dev, work_dev or
 * color_low_dev equal to an output, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device call.  Added after
 * RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
int rtm_upsample(const rtm_upsample_params* params, int32_t low_width, int32_t low_height, int device,
                 const float* color_low_dev, const rtm_aov_buffers* guide_low_dev, const rtm_aov_buffers* guide_high_dev,
                 void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream);

/* ---- frame comparison: how far a frame is from a reference, measured where both frames are — maximum error, the count of
 * pixels outside a tolerance, MSE / PSNR, relative MSE, SSIM and a per-pixel error map, in one pass with nothing copied to
 * the host.
 * Inputs: `a` is the frame under test, `b` the reference: DEVICE buffers of height x width x 3, RGB-interleaved like out_f32
 * (RTM_COMPARE_F32) or out_f64 (RTM_COMPARE_F64), both of the params' dtype; alignment is only the element's own, 4 or 8
 * bytes.  Every input value is widened to double exactly and all arithmetic is in double (one ulp at 1.0 between two out_f64
 * frames is seen and counted).  FMA contraction is allowed; the exact fields below do not depend on it.
 *   1 counting    a pixel COUNTS iff its six components (three of a, three of b) are finite.  pixels = n, the number of
 *                 counting pixels; nonfinite = width height - n; nonfinite_mismatch = the non-counting pixels that have a
 *                 component c where neither (a_c and b_c are both NaN) nor (a_c == b_c) holds: two frames with "the same
 *                 NaNs" (and the same infinities) report 0.
 *   2 error       per counting pixel d_c = |a_c - b_c|, D_p = max(max(d_R, d_G), d_B).  max_abs = max D_p (0 when n = 0);
 *                 (argmax_x, argmax_y) = the lowest row-major pixel index that attains max_abs ((-1, -1) when n = 0);
 *                 outside = #{p : D_p > tolerance}, a strict inequality: with tolerance 0 the number of differing pixels.
 *   3 mse         mse = sum_p ((d_R^2 + d_G^2) + d_B^2) / (3 n) (0 when n = 0); psnr = 10 log10(peak^2 / mse) when mse > 0,
 *                 else +inf.
 *   4 rel_mse     rel_mse = sum_p sum_c d_c^2 / (b_c^2 + rel_epsilon) / (3 n) (0 when n = 0): not symmetric in a and b.
 *   5 ssim        (Wang et al. 2004, on luminance) l = (0.2126 R + 0.7152 G) + 0.0722 B for a counting pixel and 0 IN BOTH
 *                 IMAGES at a non-counting one (the display transform's rule).  Window g[k] = exp(-k^2 / 4.5), k = -5..5
 *                 (sigma 1.5 over 11 x 11); only in-frame taps are used, renormalised: the tap (dx, dy) of pixel (x, y) has
 *                 weight g[dx] g[dy] / (G_x G_y), G_x the sum of g over the in-frame dx and G_y likewise — separable at the
 *                 border too, and defined for every frame size including 1 x 1.  With E[.] that weighted mean:
 *                 mu_a = E[l_a], mu_b = E[l_b], var_a = E[l_a^2] - mu_a^2, var_b likewise, cov = E[l_a l_b] - mu_a mu_b;
 *                 C1 = (0.01 peak)^2, C2 = (0.03 peak)^2;
 *                 S_p = ((2 mu_a mu_b + C1)(2 cov + C2)) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2));
 *                 ssim = the mean of S_p over all width height pixels.
 *   6 map         map_out_dev (nullable, DEVICE, height x width floats): RTM_COMPARE_MAP_ABS (float)D_p, NaN at a
 *                 non-counting pixel; RTM_COMPARE_MAP_SSIM (float)S_p.
 * Sums are taken in an order fixed by the frame size alone; no atomics: the same inputs give the same bits on every call, on
 * any stream, and at any alignment of the frames.  Against a float64 evaluation of the steps above: pixels, outside,
 * nonfinite, nonfinite_mismatch, max_abs, argmax_x, argmax_y and the MAP_ABS map are exact; mse, rel_mse and psnr are within
 * 1e-9 relative (psnr: both +inf, or within 1e-9 relative); ssim within 1e-9 absolute; the MAP_SSIM map within 1e-7 absolute
 * (1e-9 plus the float rounding).
 * work_dev: DEVICE, 256-byte aligned, rtm_compare_work_bytes = round256(48 tiles) + 256 bytes, tiles = ceil(width / 32)
 * ceil(height / 32): one 48-byte partial per 32 x 32 tile of pixels and the final record, nothing else (SSIM's moments stay on
 * the chip).  That is at most 256 bytes per 1024 pixels plus 512 for every frame whose sides are both 32 or more and for
 * every frame of one tile; a frame thinner than a tile pays its 48 bytes per started tile.  0 for a non-positive size,
 * SIZE_MAX when the frame itself (24 bytes a pixel) does not fit a size_t.
 * The call allocates nothing, keeps no per-(device, stream) state, needs no serialisation and only ENQUEUES two launches on
 * `stream` of `device`: one block per tile, then a one-block fold of the partials that writes the record; one launch when
 * result_out_dev is null (a map alone needs no fold, and the ABS map alone no window).  a_dev == b_dev is allowed.
 * Null params, a_dev, b_dev or work_dev, both outputs null, a non-positive size, dtype or map out of range, a negative, NaN or
 * infinite tolerance, peak or rel_epsilon not finite and > 0, a frame pointer, an output or work_dev misaligned (the
 * element's 4 or 8 bytes, 8 for the record, 4 for the map, 256 for work_dev), work_dev or either output equal to a_dev or
 * b_dev, map_out_dev equal to work_dev or to result_out_dev, result_out_dev equal to work_dev, a negative device:
 * RTM_ERR_INVALID_ARGUMENT, before any device call.  A frame too large for one launch (2^31 pixels or more):
 * RTM_ERR_UNSUPPORTED, as rtm_tonemap.
 * Defaults: RTM_COMPARE_DEFAULTS below (the headline's tolerance 1e-4, peak 1, rel_epsilon 1e-2; what rtm_cli --compare uses).
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
enum { RTM_COMPARE_F32 = 0, RTM_COMPARE_F64 = 1 };
enum { RTM_COMPARE_MAP_ABS = 0, RTM_COMPARE_MAP_SSIM = 1 };
typedef struct rtm_compare_params {
    int32_t dtype;       /* RTM_COMPARE_F*: the element type of BOTH frames                     */
    int32_t map;         /* RTM_COMPARE_MAP_*: what map_out_dev receives                        */
    double tolerance;    /* >= 0, finite: outside counts D_p > tolerance                        */
    double peak;         /* > 0, finite: PSNR's peak and SSIM's dynamic range L                 */
    double rel_epsilon;  /* > 0, finite: rel_mse's denominator offset                           */
} rtm_compare_params;
#define RTM_COMPARE_DEFAULTS {RTM_COMPARE_F32, RTM_COMPARE_MAP_ABS, 1e-4, 1.0, 1e-2} /* an initializer of rtm_compare_params */
typedef struct rtm_compare_result { /* 80 bytes, no padding */
    double max_abs, mse, psnr, rel_mse, ssim;
    uint64_t pixels, outside, nonfinite, nonfinite_mismatch;
    int32_t argmax_x, argmax_y;
} rtm_compare_result;
size_t rtm_compare_work_bytes(int32_t width, int32_t height);
int rtm_compare(const rtm_compare_params* params, int32_t width, int32_t height, int device, const void* a_dev,
                const void* b_dev, void* work_dev, rtm_compare_result* result_out_dev, float* map_out_dev, void* stream);

/* ---- perceptual frame difference (LDR FLIP, Andersson et al. 2020, "A Difference Evaluator for Alternating Images"): which
 * of two wrong frames LOOKS closer to a reference, where rtm_compare answers whether two frames are the same.  Contrast
 * sensitivity filtering in an opponent colour space, a perceptually uniform colour distance and an edge / point feature term
 * give one error map in [0, 1] and pooled statistics, on the device.  This text is the definition; its constants are the
 * paper's and its published program's as known here, and no figure has been compared with that program.
 * Inputs: `a` is the frame under test, `b` the reference: DEVICE buffers of height x width x 3 floats, RGB-interleaved like
 * out_f32, 4-byte aligned, DISPLAY-REFERRED: params.transfer says how they are encoded, RTM_TRANSFER_SRGB as rtm_tonemap
 * writes them by default, RTM_TRANSFER_LINEAR already linear.  Every value is widened to double exactly and all arithmetic
 * is in double; FMA contraction is allowed.  ppd = params.pixels_per_degree, finite, in [8, 128]; the default is a 0.7 m wide
 * 3840-pixel monitor viewed from 0.7 m, 0.7 * 3840 / 0.7 * pi / 180 = 67.02...
 *   1 counting    a pixel COUNTS iff its six components are finite.  A non-counting pixel is (0, 0, 0) in BOTH frames for
 *                 everything below (its neighbours see black), its map value is NaN and it is excluded from the pooled
 *                 statistics.  pixels = n, the number of counting pixels; nonfinite = width height - n.
 *   2 to linear   each component clamped to [0, 1]; for SRGB then c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4).
 *   3 opponent    XYZ = M rgb, M's rows (10135552, 8788810, 4435075) / 24577794, (2613072, 8788810, 887015) / 12288897,
 *                 (1425312, 8788810, 70074185) / 73733382, each entry one double division, a row applied as
 *                 (m0 r + m1 g) + m2 b; (Xn, Yn, Zn) = M (1, 1, 1) = (m0 + m1) + m2 per row.  With x = X / Xn, y = Y / Yn,
 *                 z = Z / Zn:  Y = 116 y - 16,  Cx = 500 (x - y),  Cz = 200 (y - z).
 *   4 CSF         e_b(k) = exp(-pi^2 (k / ppd)^2 / b), k = -r..r, r = ceil(3 sqrt(0.04 / (2 pi^2)) ppd) (10 at the default,
 *                 2..18 over the range).  Y is filtered with e_0.0047(dx) e_0.0047(dy), Cx with e_0.0053(dx) e_0.0053(dy), Cz
 *                 with A1 e_0.04(dx) e_0.04(dy) + A2 e_0.025(dx) e_0.025(dy), A1 = 34.1 sqrt(pi / 0.04), A2 = 13.5 sqrt(pi /
 *                 0.025); each 2-D filter is divided by its own sum over the (2r+1)^2 grid.  As 1-D tables used in both axes:
 *                 t_Y(k) = e_0.0047(k) / sum e_0.0047, t_Cx likewise, and for Cz the two parts t_1(k) = sqrt(A1 / S) e_0.04(k),
 *                 t_2(k) = sqrt(A2 / S) e_0.025(k) with S = A1 (sum e_0.04)^2 + A2 (sum e_0.025)^2, filtered Cz = the sum of
 *                 the two separable results.  A tap outside the frame takes the NEAREST IN-FRAME pixel (coordinates clamped:
 *                 replicate padding).  That is the published definition and it DIFFERS from the skip-and-renormalise rule of
 *                 this library's other filters (rtm_compare's SSIM window, the denoisers).  A separable filter is evaluated
 *                 horizontal pass first, taps in ascending offset; the tables are computed in double on the host.
 *   5 colour      filtered (Y, Cx, Cz) back to linear RGB: y = (Y + 16) / 116, x = Cx / 500 + y, z = y - Cz / 200, times
 *                 (Xn, Yn, Zn), then M^-1 (inverted in double on the host), clamped to [0, 1]; to CIELAB with the same white:
 *                 f(t) = t > (6/29)^3 ? cbrt(t) : t / (3 (6/29)^2) + 4/29 on M rgb / white, L = 116 f(y) - 16,
 *                 a = 500 (f(x) - f(y)), b = 200 (f(y) - f(z)); Hunt adjustment (L, 0.01 L a, 0.01 L b); HyAB distance
 *                 |dL| + sqrt(da^2 + db^2) between the two frames; c = HyAB^0.7; cmax = the same power of the HyAB distance
 *                 between the Hunt-adjusted Lab of linear (0, 1, 0) and of linear (0, 0, 1), computed on the host (41.276...);
 *                 dEc = c < 0.4 cmax ? (0.95 / (0.4 cmax)) c : 0.95 + (c - 0.4 cmax) / (cmax - 0.4 cmax) 0.05.
 *   6 feature     on the UNFILTERED y = (Y + 16) / 116 of each frame: sigma = 0.5 0.082 ppd, rf = ceil(3 sigma) (9 at the
 *                 default, 1..16 over the range), g(k) = exp(-k^2 / (2 sigma^2)), d(k) = -k g(k) (edge), p(k) = (k^2 / sigma^2
 *                 - 1) g(k) (point).  Of each 2-D filter d(dx) g(dy) and p(dx) g(dy) the positive weights are divided by their
 *                 sum and the negative ones by the magnitude of theirs; the sign depends on dx alone, so as 1-D tables:
 *                 g'(k) = g(k) / sum g;  d'(k) = d(k) / sum_{k<0} d(k) (d is odd: one divisor serves both signs);
 *                 p'(k) = p(k) / sum_{p>0} p where p(k) > 0, p(k) / |sum_{p<0} p| where p(k) < 0.  ex = d'(dx) g'(dy),
 *                 ey = g'(dx) d'(dy), px = p'(dx) g'(dy), py = g'(dx) p'(dy), replicate padding, horizontal pass first.  Per
 *                 frame |edge| = sqrt(ex^2 + ey^2), |point| = sqrt(px^2 + py^2);
 *                 dEf = sqrt(max(| |edge_b| - |edge_a| |, | |point_b| - |point_a| |) / sqrt(2)).
 *   7 combine     dE_p = dEc^(1 - dEf), with pow(0, .) = 0.  map_out_dev (nullable, DEVICE, height x width floats) receives
 *                 (float)dE_p, NaN at a non-counting pixel.  Identical inputs give dE_p = +0 exactly at every counting pixel.
 *   8 pooled      rtm_flip_result (1072 bytes, no padding): mean = the mean of dE_p over the counting pixels (0 when n = 0);
 *                 max, with (argmax_x, argmax_y) the lowest row-major pixel index that attains it (0 and (-1, -1) when n = 0);
 *                 min (0 when n = 0); pixels, nonfinite as in step 1; hist[256] = counts of counting pixels, bin =
 *                 min(255, (int)(m * 256.0f)) with m the pixel's FLOAT map value: exact given the call's own map, the way
 *                 rtm_tonemap's out_u8 is exact given its own out_f32, and computed whether or not the map is stored.
 * Sums are taken in an order fixed by the frame size alone and the only atomics add integers (the histogram): the same inputs
 * give the same bits on every call, on any stream.  Against a float64 evaluation of the steps above: pixels, nonfinite and
 * where the map is NaN are exact; mean, min and max are within 1e-9 absolute, the map within 1e-9 plus its float rounding
 * (2^-25 = 3e-8); argmax is the evaluation's wherever its two largest values differ by more than 2e-9.  (The bound is max(1e-9,
 * 100 D), D = 9.3e-14 the largest disagreement of two float64 evaluation orders, separable and direct 2-D: DESIGN.md.)
 * work_dev: DEVICE, 256-byte aligned, rtm_flip_work_bytes = round256(112 width height) + round256(32 tiles) + 1024 bytes,
 * tiles = ceil(width / 64) ceil(height / 16): the seven horizontally filtered planes of each frame as doubles (they do not
 * fit the chip: a tile with the halo of the largest tables would need 3.2 times a CU's LDS), one 32-byte partial per tile
 * and the histogram.  0 for a non-positive size, SIZE_MAX when that sum does not fit a size_t.
 * The call allocates nothing, keeps no per-(device, stream) state, needs no serialisation and only ENQUEUES three launches on
 * `stream` of `device`: the horizontal pass (one block per 256 pixels of a row), the vertical pass with steps 5-8 (one block
 * per tile) and a one-block fold that writes the record; two launches when result_out_dev is null.  a_dev == b_dev is
 * allowed.  Null params, a_dev, b_dev or work_dev, both outputs null, a non-positive size, transfer out of range,
 * pixels_per_degree NaN, infinite or outside [8, 128], a frame pointer, an output or work_dev misaligned (4 bytes for the
 * frames and the map, 8 for the record, 256 for work_dev), work_dev or either output equal to a_dev or b_dev, map_out_dev
 * equal to work_dev or to result_out_dev, result_out_dev equal to work_dev, a negative device: RTM_ERR_INVALID_ARGUMENT,
 * before any device call.  A frame of 2^31 pixels or more: RTM_ERR_UNSUPPORTED.
 * Defaults: RTM_FLIP_DEFAULTS below (what rtm_cli --flip uses).
 * Added after RTM_ABI_VERSION 5 without changing it: callers look the symbols up. */
typedef struct rtm_flip_params { /* 16 bytes */
    int32_t transfer;         /* RTM_TRANSFER_*: how BOTH frames are encoded                    */
    double pixels_per_degree; /* finite, in [8, 128]                                            */
} rtm_flip_params;
#define RTM_FLIP_DEFAULT_PPD (0.7 * 3840.0 / 0.7 * 3.14159265358979323846 / 180.0)
#define RTM_FLIP_DEFAULTS {RTM_TRANSFER_SRGB, RTM_FLIP_DEFAULT_PPD} /* an initializer of rtm_flip_params */
typedef struct rtm_flip_result { /* 1072 bytes, no padding */
    double mean, max, min;
    uint64_t pixels, nonfinite;
    int32_t argmax_x, argmax_y;
    uint32_t hist[256];
} rtm_flip_result;
size_t rtm_flip_work_bytes(int32_t width, int32_t height);
int rtm_flip(const rtm_flip_params* params, int32_t width, int32_t height, int device, const float* a_dev,
             const float* b_dev, void* work_dev, rtm_flip_result* result_out_dev, float* map_out_dev, void* stream);

/* ---- scopes: what ONE frame holds — per-channel histograms, a per-column waveform / RGB parade, and from the histogram, on
 * the host, percentiles and an exposure suggestion.  rtm_compare and rtm_flip measure a pair of frames; rtm_tonemap knows a
 * frame's log-average and L_max only.  Opt-in; no other stage and no default changes.
 * Input: color (DEVICE, height x width x 3 floats, RGB-interleaved like out_f32; 4-byte alignment is enough).  Every count is
 * an integer and every bin is taken from a float's 32-bit word or from one stated double product, so a float32 restatement
 * reproduces every word of both outputs.
 *   1 counting   a pixel COUNTS iff its three components are finite (the library's rule).  `pixels` counts those that do,
 *                `not_counting` those that do not; a pixel that does not count enters nothing else.
 *   2 channels   channel 0 is Y, 1 is R, 2 is G, 3 is B.  R, G and B are the components' own words.
 *                l = (0.2126f c_R + 0.7152f c_G) + 0.0722f c_B in float, without contraction (rtm_tonemap's lum), and
 *                Y = l > 0 ? l : +0.0f.  An l that overflowed to +inf is a value like any other: it lands in `above`.
 *   3 LOG2 bins  (mode RTM_SCOPE_LOG2, for a scene-referred frame) 8 bins a stop from 2^-16 up to, not including, 2^16,
 *                read from the value's bit pattern: no logarithm is evaluated and no bin edge depends on a fast-math form.
 *                With u the value's 32-bit word: the value is BELOW when the sign bit is set or (u >> 20) < 888 (that is
 *                +-0, denormals and everything under 2^-16, so it does not matter whether the device flushes denormals);
 *                otherwise b = (u >> 20) - 888, and the value is ABOVE when b > 255, else it is in bins[c][b].  Bin b holds
 *                [2^e (1 + j/8), the next bin's lower edge) with e = (b >> 3) - 16 and j = b & 7; bin 128 starts at 1.0,
 *                0.18 is in bin 107, and 65536 is the first value above.
 *   4 CODE bins  (mode RTM_SCOPE_CODE, for a display-referred frame in [0, 1]) v < 0 is BELOW, v > 1 is ABOVE, otherwise
 *                the bin is (int)(255.0 * (double)v): the byte rtm_quantise stores.  -0.0f is bin 0 and 1.0 is bin 255.
 *   5 histogram  hist_out_dev (nullable): bins[c][b], below[c] and above[c] over the counting pixels, pixels, not_counting,
 *                reserved = 0.
 *   6 waveform   waveform_out_dev (nullable, [4][256][columns] words): frame column x belongs to output column
 *                (int64)x * columns / width, and waveform[c][b][oc] counts the counting pixels of those columns whose channel
 *                c is in bin b; BELOW is counted in row 0 and ABOVE in row 255: clipped values pile up at the scope's edges.
 * It follows that, for every c, below[c] + sum_b bins[c][b] + above[c] == pixels; that pixels + not_counting == width height;
 * and that sum_oc waveform[c][b][oc] == bins[c][b] for 0 < b < 255, == bins[c][0] + below[c] for b = 0 and
 * == bins[c][255] + above[c] for b = 255.
 * The counts are exact and order-free, so this stage uses INTEGER ATOMICS ONLY (on LDS and on the outputs' words): the same
 * inputs give the same words on every call, on any stream, at any 4-byte alignment.  No state, no work buffer: the call
 * zeroes its own outputs on `stream`, allocates nothing and only ENQUEUES (the zeroing and one launch).  Null params or
 * color_dev, both outputs null, a non-positive size, mode out of range, columns outside 1..width when a waveform is asked for
 * (ignored without one), a pointer that is not 4-byte aligned, an output equal to color_dev or to the other output, a negative
 * device: RTM_ERR_INVALID_ARGUMENT, before any device call.  A frame of 2^31 pixels or more: RTM_ERR_UNSUPPORTED.
 *
 * rtm_scope_draw turns a waveform into a picture (DEVICE, 256 rows of RGB bytes, bin 255 on top): a value is
 * min(255, (uint64)count * gain).  RTM_SCOPE_LUMA: columns wide, plane 0 in all three bytes.  RTM_SCOPE_OVERLAY: columns wide,
 * byte k from plane 1 + k.  RTM_SCOPE_PARADE: 3 columns wide, the panels R, G, B side by side, each in its own byte with the
 * other two bytes 0.  One launch on `stream`, no atomics.  Null pointers, columns < 1, layout out of range, gain 0, a
 * misaligned waveform_dev, out_u8_dev equal to waveform_dev, a negative device: RTM_ERR_INVALID_ARGUMENT, before any device
 * call; columns of 2^21 or more: RTM_ERR_UNSUPPORTED.
 *
 * The rest is HOST ONLY (a histogram copied to the host; no device call), in double:
 * rtm_scope_bin_range: the range [lo, hi) of bin 0..255 as floats.  LOG2: step 3's edges (hi of bin 255 is 65536).  CODE: lo
 *   is the smallest float whose bin is `bin` (0 for bin 0) and hi the next bin's lo; bin 255 holds 1.0 alone: lo = hi = 1.
 * rtm_scope_percentile of channel c: N = pixels.  N == 0: value 1, bin -2 (rtm_tonemap's n == 0 rule).  t = percent / 100 N,
 *   cum = below[c].  t <= cum: value 0, bin -1.  Otherwise the first bin b with n_b > 0 and cum + n_b >= t (cum running over
 *   the bins before it): value = lo_b + (t - cum) / n_b (hi_b - lo_b), rounded to float, bin b.  Past the last bin: the
 *   range's upper end (65536 or 1) and bin 256.  value_out and bin_out are each nullable, not both.
 * rtm_scope_exposure: ev = log2(target / value), value being channel Y's LOG2 percentile, clamped to rtm_tonemap's +-32 and
 *   rounded to float; value <= 0 gives ev = 0.  rtm_tonemap with auto_exposure = 0 and this ev puts that percentile at target.
 * Null pointers, mode out of range, a bin or a channel out of range, a percent outside [0, 100] or NaN, a target that is not
 * positive and finite: RTM_ERR_INVALID_ARGUMENT.
 * Defaults: RTM_SCOPE_DEFAULTS below (what rtm_cli --scopes uses for the linear frame).  Added after RTM_ABI_VERSION 5 without
 * changing it: callers look the symbols up. */
enum { RTM_SCOPE_LOG2 = 0, RTM_SCOPE_CODE = 1 };
enum { RTM_SCOPE_LUMA = 0, RTM_SCOPE_OVERLAY = 1, RTM_SCOPE_PARADE = 2 };
typedef struct rtm_scope_params { /* 8 bytes */
    int32_t mode;    /* RTM_SCOPE_LOG2 or RTM_SCOPE_CODE                                      */
    int32_t columns; /* waveform columns, 1..width; ignored without a waveform                */
} rtm_scope_params;
#define RTM_SCOPE_DEFAULTS {RTM_SCOPE_LOG2, 256} /* an initializer of rtm_scope_params */
typedef struct rtm_scope_histogram { /* 4144 bytes, no padding */
    uint32_t bins[4][256]; /* channel 0 = Y, 1 = R, 2 = G, 3 = B */
    uint32_t below[4], above[4];
    uint32_t pixels, not_counting, reserved[2]; /* reserved = 0 */
} rtm_scope_histogram;
int rtm_scopes(const rtm_scope_params* params, int32_t width, int32_t height, int device, const float* color_dev,
               rtm_scope_histogram* hist_out_dev, uint32_t* waveform_out_dev, void* stream);
int rtm_scope_draw(int32_t columns, int32_t layout, uint32_t gain, int device, const uint32_t* waveform_dev,
                   uint8_t* out_u8_dev, void* stream);
int rtm_scope_bin_range(int32_t mode, int32_t bin, float* lo, float* hi);
int rtm_scope_percentile(const rtm_scope_histogram* hist_host, int32_t mode, int32_t channel, double percent,
                         float* value_out, int32_t* bin_out);
int rtm_scope_exposure(const rtm_scope_histogram* hist_host, double percent, double target, float* ev_out);

/* RTM_OK, or RTM_ERR_UNSUPPORTED when a render enqueued on (device, stream) since the last report
 * overflowed its hit records.  Waits for the stream's queued work (hipStreamSynchronize). */
int rtm_stream_status(int device, void* stream);

/* The same render from a sphere ARRAY.  spheres is a HOST pointer (tiny for shipped scenes) unless
 * spheres_on_device != 0.  Host arrays are looked up in a small per-device cache keyed by their
 * content, so repeated calls with an unchanged scene behave like rtm_render_scene (the first call
 * with new content uploads it and waits for the upload); device arrays are flattened on the stream
 * per call. */
int rtm_render_device(const rtm_settings* settings, const rtm_sphere* spheres, size_t n_spheres,
                      int spheres_on_device, const rtm_options* options, double* out_f64_dev,
                      float* out_f32_dev, uint8_t* out_u8_dev, void* stream, rtm_stats* stats);

/* Blocking convenience: same render, HOST output buffers (any may be null). */
int rtm_render(const rtm_settings* settings, const rtm_sphere* spheres, size_t n_spheres,
               const rtm_options* options, double* out_f64, float* out_f32, uint8_t* out_u8,
               rtm_stats* stats);

/* The blocking render for a list of objects of any type (rtm_object: spheres and planes), HOST buffers. */
int rtm_render_objects(const rtm_settings* settings, const rtm_object* objects, size_t n_objects,
                       const rtm_options* options, double* out_f64, float* out_f32, uint8_t* out_u8,
                       rtm_stats* stats);

/* ---- per-ray seam: png::PathTracing (src/Renderer.cpp:57-117) for a batch of rays on device.
 * Ray i uses the RNG stream keyed (seed, pixel = i, sample = 0).  Host buffers.
 * org/dir: n*3 doubles; out_radiance: n*3; out_draws/out_casts: n (nullable). */
int rtm_path_trace_batch(const rtm_sphere* spheres, size_t n_spheres, const rtm_options* options,
                         const double* org, const double* dir, size_t n_rays,
                         double* out_radiance, uint32_t* out_draws, uint32_t* out_casts);

/* ---- per-ray seam of the reference's second integrator: png::SurfaeSample (src/Renderer.cpp:119-198, entered at depth 0)
 * for a batch of rays on device, like rtm_path_trace_batch: ray i uses the RNG stream keyed (seed, pixel = i, sample = 0);
 * host buffers; out_draws = generator calls, out_casts = nearest-hit loops.  options->max_bounces >= 0 bounds the recursion
 * (RTM_MODE_SURFACE_SAMPLE above); unbounded, a recursion deeper than 1 024 levels fails with RTM_ERR_UNSUPPORTED. */
int rtm_surface_sample_batch(const rtm_sphere* spheres, size_t n_spheres, const rtm_options* options,
                             const double* org, const double* dir, size_t n_rays,
                             double* out_radiance, uint32_t* out_draws, uint32_t* out_casts);

/* ---- per-call seam: SphereObject::Intersect (src/SettingData.cpp:197-226) on device.
 * Pair i tests ray i against sphere i.  Host buffers.  out_t/out_normal are left untouched
 * (caller-initialised) where out_hit[i]==0; in RTM_MODE_LITERAL out_normal is never written. */
int rtm_intersect_batch(const rtm_sphere* spheres, const double* org, const double* dir,
                        size_t n, int mode, int32_t* out_hit, double* out_t, double* out_normal);

/* The same seam for objects of any type (rtm_object): pair i tests ray i against object i. */
int rtm_intersect_objects_batch(const rtm_object* objects, const double* org, const double* dir, size_t n, int mode,
                                int32_t* out_hit, double* out_t, double* out_normal);

/* ---- the build-defined RNG (reference seeds std::mt19937 from random_device:
 * src/Renderer.cpp:210-213, so there is no reference stream to match).  Host-side evaluation of
 * draw `index` of stream (seed, pixel, sample); device side must agree (rtm_rng_batch). */
double rtm_rng_u01(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t index);
int rtm_rng_batch(uint64_t seed, uint32_t pixel0, uint32_t n_pixels, uint32_t sample,
                  uint32_t n_draws, double* out /* n_pixels*n_draws, host, computed on device */);

/* ---- host side: scene loading (png::LoadData, src/SettingData.cpp:6-12,129-186) ----
 * Reads the reference's JSON schema.  literal_loader != 0 reproduces HEAD's position bug
 * (src/SettingData.cpp:165-167: centre = (json_z, 0, 0)).  Shipped files load unchanged:
 * missing "00 objectType" => sphere, objects without "00 position" skipped, "00 sample" accepted
 * for "00 samples", missing samples/superSamples => 10 / 1.
 * spheres may be NULL with capacity 0 to query *n_spheres. */
int rtm_scene_load_json(const char* path, int literal_loader, rtm_settings* settings,
                        rtm_sphere* spheres, size_t capacity, size_t* n_spheres);
int rtm_scene_parse_json(const char* text, size_t len, int literal_loader, rtm_settings* settings,
                         rtm_sphere* spheres, size_t capacity, size_t* n_spheres);
/* The same loaders for files that may hold planes ("00 objectType": 2 with "00 position", "01 size" = width,
 * "03 up", "04 target", "02 material" — a build-defined extension of the schema; the sphere-only loaders
 * above reject such a file with RTM_ERR_INVALID_SCENE). */
int rtm_scene_load_json_objects(const char* path, int literal_loader, rtm_settings* settings,
                                rtm_object* objects, size_t capacity, size_t* n_objects);
int rtm_scene_parse_json_objects(const char* text, size_t len, int literal_loader, rtm_settings* settings,
                                 rtm_object* objects, size_t capacity, size_t* n_objects);
/* LoadData::SaveSampleJson (src/SettingData.cpp:14-24,100-127): 960x540, samples 10, SS 4. */
int rtm_scene_save_sample_json(const char* path);
/* Stress scene of BASELINE config 5: SplitMix64(seed), n spheres. */
int rtm_scene_make_stress(uint64_t seed, size_t n, rtm_settings* settings, rtm_sphere* spheres);

/* ---- host side: image output (src/Renderer.cpp:251-257) ----
 * rtm_quantise: u8 = (unsigned char)(255 * min(v, 1.0)) per component. */
int rtm_quantise(const double* image, size_t n_values, uint8_t* out);
/* stb_image_write-compatible signatures (w, h, comp = 3, RGB rows top-down). Return 1 on success
 * like stb (0 on failure) so real stb can replace them. */
int rtm_write_bmp(const char* filename, int w, int h, int comp, const void* data);
int rtm_write_jpg(const char* filename, int w, int h, int comp, const void* data, int quality);
/* Portable float map (the AOV planes): "PF" (comp 3) or "Pf" (comp 1), "w h", scale -1.0 (little-endian), rows
 * bottom-up; data is HOST, rows top-down like the writers above.  1 on success, 0 on failure.  Added after
 * RTM_ABI_VERSION 5 (callers look the symbol up). */
int rtm_write_pfm(const char* filename, int w, int h, int comp /* 1 or 3 */, const float* data);
/* Reads a file rtm_write_pfm wrote, bit for bit: *w, *h and *comp (1 or 3) receive the header's values; data (HOST,
 * nullable) receives the rows top-down, as the writer was given them, when capacity (in floats) is at least w h comp.  A
 * null data with capacity 0 only queries the size (the samples are still checked to be all there).  Only little-endian
 * files (a negative scale) are read.  1 on success; 0, with nothing promised about data, for a file that cannot be opened, a
 * malformed header (magic, a non-positive or overflowing size, a scale that is no number or 0), a big-endian file, a
 * truncated file or a capacity that is too small.  Added after RTM_ABI_VERSION 5 (callers look the symbol up). */
int rtm_read_pfm(const char* filename, int* w, int* h, int* comp, float* data, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* RTM_H */
