// rtm_internal.h — C++ entry points behind the C ABI (include/rtm.h).  Not installed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/rtm.h"

namespace rtm {

// rtm_last_error's message (rtm_scene.cpp)
void set_last_error(const std::string& s);
const char* last_error();
// records `message` for rtm_last_error and hands `code` back: `return fail(...)`
inline int fail(int code, const std::string& message) {
    set_last_error(message);
    return code;
}
inline int invalid(const std::string& what) { return fail(RTM_ERR_INVALID_ARGUMENT, what); }
inline int unsupported(const std::string& what) { return fail(RTM_ERR_UNSUPPORTED, what); }

// device path (rtm_kernels.hip)
int device_count(int* count);
int num_variants();
int output_rows(const rtm_options* opt);
int release_scratch(int device);
int stream_release(int device, void* stream);
int wf_nearest_probe(int kind, const rtm_sphere* sp, size_t n, const double* org, const double* dir, size_t n_rays,
                     int32_t* out_id, double* out_t);
const char* variant_name(int v);
int scene_create(const rtm_sphere* sp, size_t n, int on_device, int device, rtm_scene** out);
int scene_create_device(const rtm_sphere* sp_dev, size_t n, int device, void* stream, rtm_scene** out);  // rtm_grid_build.hip
int scene_create_objects(const rtm_object* objs, size_t n, int device, rtm_scene** out);
int intersect_objects_batch(const rtm_object* objs, const double* org, const double* dir, size_t n, int mode,
                            int32_t* out_hit, double* out_t, double* out_normal);
// ray queries on a scene object (rtm_query.hip); the probe runs the grid walk's counting instantiations (rtm_debug_scene_query)
int scene_nearest(const rtm_scene* scene, const double* org, const double* dir, size_t n_rays, const rtm_hit_buffers* out,
                  void* stream);
int scene_occluded(const rtm_scene* scene, const double* org, const double* dir, const double* tmax, size_t n_rays, uint8_t* out,
                   void* stream);
int scene_query_probe(const rtm_scene* scene, int any, const double* org, const double* dir, const double* tmax, size_t n_rays,
                      int32_t* out_object, double* out_t, uint8_t* out_occluded, uint32_t* out_tests, uint32_t* out_steps,
                      void* stream);
// radiance queries on a scene object (rtm_radiance.hip)
int scene_radiance(const rtm_scene* scene, const double* org, const double* dir, size_t n_rays, const rtm_radiance_params* params,
                   const rtm_radiance_buffers* out, void* stream);
int scene_destroy(rtm_scene* sc);
size_t scene_size(const rtm_scene* sc);
int stream_status(int device, void* stream);
int scratch_bytes(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, uint64_t out[6]);
int render_scene(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, double* out64, float* out32,
                 uint8_t* out8, void* stream, rtm_stats* stats);
int render_scene_samples(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, uint32_t sample_begin,
                         uint32_t sample_end, double* accum, float* out32, uint8_t* out8, void* stream, rtm_stats* stats);
int render_scene_tiles(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, uint32_t sample_begin,
                       uint32_t sample_end, const uint32_t* tiles, uint32_t n_tiles, double* accum, float* out32, uint8_t* out8,
                       void* stream, rtm_stats* stats);
// tile-adaptive sampling (rtm_adaptive.hip)
size_t adaptive_work_bytes(const rtm_settings* st, const rtm_options* opt);
int render_adaptive(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, const rtm_adaptive_params* prm,
                    double* accum, float* out32, uint8_t* out8, uint32_t* tile_samples, void* work, void* stream,
                    rtm_stats* stats);
int render_aov(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, const rtm_aov_buffers* out,
               void* stream);
int render_mattes(const rtm_settings* st, const rtm_scene* scene, const rtm_options* opt, int32_t layers,
                  const rtm_matte_buffers* out, void* stream);
// coverage AOVs (rtm_matte.hip): the ranking hook; the matte of a set of ids; "over" a background
int matte_rank_probe(int32_t super_samples, int32_t layers, int device, const int32_t* ids, size_t n_pixels, int32_t* id_out,
                     float* coverage_out, float* alpha_out, void* stream);
int matte(int32_t width, int32_t height, int32_t layers, int device, const int32_t* layer_id, const float* layer_coverage,
          const int32_t* ids, int32_t n_ids, float* matte_out, void* stream);
int composite(const rtm_composite_params* params, int32_t width, int32_t height, int device, const float* color,
              const float* alpha, const float* background, float* out32, uint8_t* out8, void* stream);
// denoiser (rtm_denoise.hip)
size_t denoise_work_bytes(int32_t width, int32_t height);
int denoise(const rtm_denoise_params* params, int32_t width, int32_t height, int device, const float* color,
            const rtm_aov_buffers* guide, void* work, float* out32, uint8_t* out8, void* stream);
size_t denoise_variance_work_bytes(int32_t width, int32_t height);
int denoise_variance(const rtm_denoise_var_params* params, int32_t width, int32_t height, int device, const float* color,
                     const rtm_aov_buffers* guide, void* work, float* out32, uint8_t* out8, float* var_out, void* stream);
int denoise_variance_kernel_probe(int form, const rtm_denoise_var_params* params, int32_t width, int32_t height, int device,
                                  const rtm_aov_buffers* guide, void* work, float* var_out, void* stream);
// display transform (rtm_tonemap.hip)
size_t tonemap_work_bytes(int32_t width, int32_t height);
int tonemap(const rtm_tonemap_params* params, int32_t width, int32_t height, int device, const float* color, void* work,
            float* out32, uint8_t* out8, rtm_tonemap_stats* stats_out, void* stream);
// bloom (rtm_bloom.hip)
size_t bloom_work_bytes(int32_t width, int32_t height, int32_t levels);
int bloom(const rtm_bloom_params* params, int32_t width, int32_t height, int device, const float* color, void* work, float* out32,
          uint8_t* out8, float* bloom_out, void* stream);
// the local tone operator (rtm_tonemap_local.hip)
size_t tonemap_local_work_bytes(int32_t width, int32_t height, int32_t levels);
int tonemap_local(const rtm_tonemap_local_params* params, int32_t width, int32_t height, int device, const float* color,
                  const rtm_tonemap_stats* stats, void* work, float* out32, uint8_t* out8, float* fused_out, void* stream);
// colour grade (rtm_grade.hip), and its host-only helpers: the white balance matrix and the .cube reader (rtm_lut.cpp)
int grade(const rtm_grade_params* params, int32_t width, int32_t height, int device, const float* color, const float* lut,
          float* out32, uint8_t* out8, void* stream);
int grade_white_balance(float kelvin, float tint, float* matrix_out);
int lut_parse_cube(const char* text, size_t len, int32_t* size, float* domain_min, float* domain_max, float* table,
                   size_t capacity);
int lut_load_cube(const char* path, int32_t* size, float* domain_min, float* domain_max, float* table, size_t capacity);
// the firefly clamp and the repair of non-finite pixels (rtm_firefly.hip)
int firefly(const rtm_firefly_params* params, int32_t width, int32_t height, int device, const float* color, float* out32,
            uint8_t* out8, uint8_t* mask_out, float* threshold_out, void* stream);
// the frame scopes (rtm_scope.hip): histograms and the waveform on the device, the picture of a waveform, and the host-only
// readers of a histogram
int scopes(const rtm_scope_params* params, int32_t width, int32_t height, int device, const float* color,
           rtm_scope_histogram* hist_out, uint32_t* waveform_out, void* stream);
int scope_draw(int32_t columns, int32_t layout, uint32_t gain, int device, const uint32_t* waveform, uint8_t* out8, void* stream);
int scope_bin_range(int32_t mode, int32_t bin, float* lo, float* hi);
int scope_percentile(const rtm_scope_histogram* hist, int32_t mode, int32_t channel, double percent, float* value_out,
                     int32_t* bin_out);
int scope_exposure(const rtm_scope_histogram* hist, double percent, double target, float* ev_out);
// depth of field (rtm_defocus.hip); the probe runs one form of the kernel (rtm_debug_defocus_form)
int defocus(const rtm_defocus_params* params, int32_t width, int32_t height, int device, const float* color, const float* depth,
            float* out32, uint8_t* out8, float* coc_out, void* stream);
int defocus_form_probe(int form, const rtm_defocus_params* params, int32_t width, int32_t height, int device, const float* color,
                       const float* depth, float* out32, uint8_t* out8, float* coc_out, void* stream);
// lens distortion, chromatic aberration, vignette (rtm_lens.hip)
int lens(const rtm_lens_params* params, int32_t width, int32_t height, int device, const float* src, float* out32, uint8_t* out8,
         void* stream);
int lens_fit_zoom(const rtm_lens_params* params, int32_t width, int32_t height, float* zoom_out);
// filtered resampling (rtm_resize.hip)
size_t resize_work_bytes(int32_t src_width, int32_t src_height, int32_t dst_width, int32_t dst_height, int32_t filter,
                         int32_t channels);
int resize(const rtm_resize_params* params, int32_t src_width, int32_t src_height, int32_t dst_width, int32_t dst_height, int device,
           const float* src, void* work, float* out32, uint8_t* out8, void* stream);
// AOV-guided upsampling (rtm_upsample.hip)
size_t upsample_work_bytes(int32_t low_width, int32_t low_height);
int upsample(const rtm_upsample_params* params, int32_t low_width, int32_t low_height, int device, const float* color_low,
             const rtm_aov_buffers* guide_low, const rtm_aov_buffers* guide_high, void* work, float* out32, uint8_t* out8,
             void* stream);
// frame comparison (rtm_compare.hip)
size_t compare_work_bytes(int32_t width, int32_t height);
int compare(const rtm_compare_params* params, int32_t width, int32_t height, int device, const void* a, const void* b, void* work,
            rtm_compare_result* result_out, float* map_out, void* stream);
// perceptual frame difference (rtm_flip.hip)
size_t flip_work_bytes(int32_t width, int32_t height);
int flip(const rtm_flip_params* params, int32_t width, int32_t height, int device, const float* a, const float* b, void* work,
         rtm_flip_result* result_out, float* map_out, void* stream);
int render_device(const rtm_settings* st, const rtm_sphere* sp, size_t n, int spheres_on_device,
                  const rtm_options* opt, double* out64, float* out32, uint8_t* out8, void* stream,
                  rtm_stats* stats);
int render_host(const rtm_settings* st, const rtm_sphere* sp, size_t n, const rtm_options* opt,
                double* out64, float* out32, uint8_t* out8, rtm_stats* stats);
int render_host_objects(const rtm_settings* st, const rtm_object* objs, size_t n, const rtm_options* opt,
                        double* out64, float* out32, uint8_t* out8, rtm_stats* stats);
int path_trace_batch(const rtm_sphere* sp, size_t n, const rtm_options* opt, const double* org,
                     const double* dir, size_t n_rays, double* out, uint32_t* out_draws,
                     uint32_t* out_casts);
int surface_sample_batch(const rtm_sphere* sp, size_t n, const rtm_options* opt, const double* org, const double* dir,
                         size_t n_rays, double* out, uint32_t* out_draws, uint32_t* out_casts);
int intersect_batch(const rtm_sphere* sp, const double* org, const double* dir, size_t n, int mode,
                    int32_t* out_hit, double* out_t, double* out_normal);
int rng_batch(uint64_t seed, uint32_t pixel0, uint32_t n_pixels, uint32_t sample, uint32_t n_draws,
              double* out);
double rng_u01_host(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t index);
int component_bench(int which, const rtm_sphere* sp, size_t n, int reps, int blocks, int lds_pad,
                    double* cycles_per_rep);
int selfcheck(int kind, unsigned long long* mismatches);
int grid_nearest_probe(const rtm_sphere* sp, size_t n, const double* org, const double* dir, size_t n_rays, int32_t* out_id,
                       double* out_t, uint32_t* out_tests, uint32_t* out_steps, uint64_t* info);
int scene_grid_probe(const rtm_scene* sc, uint64_t* info, uint32_t* ranges, size_t ranges_cap, uint32_t* items, size_t items_cap,
                     int32_t* big, size_t big_cap, uint64_t* extra);  // rtm_grid_build.hip
int fp64_peak(int waves_per_simd, double min_ms, double* tflops, double* kernel_ms);
int math_probe(int op, const double* a, const double* b, size_t n, double* out);
// the host-only test hooks of the scene proofs and the host grid builder (rtm_scene_facts.cpp): no device is touched
int scene_facts_host(const rtm_sphere* sp, size_t n, uint64_t* facts);
int zero_term_facts_host(const rtm_sphere* sp, size_t n, uint64_t* facts);
int axis_rows_host(const rtm_sphere* sp, size_t n, double* rows);
int wall_pairs_host(const rtm_sphere* sp, size_t n, uint64_t* facts);
int grid_build_host(const rtm_sphere* sp, size_t n, uint64_t* info, double* pads, uint32_t* ranges, size_t ranges_cap,
                    uint32_t* items, size_t items_cap, int32_t* big, size_t big_cap);
// the labelled tolerance row (rtm_kernels_tol.hip): launches for a planned rtm::RenderParams passed by bytes
int launch_tol(const void* render_params, size_t params_bytes, unsigned grid, size_t lds_pad, void* stream);
int tol_math_probe(int op, const double* a_dev, const double* b_dev, size_t n, double* out_dev);  // ops 32.. of math_probe
int tol_lds_bytes(int n, int any_depth, int split, int rows, uint64_t* out);  // rtm_debug_tol_lds_bytes (rtm_kernels_tol.hip)
int trig_table_host(int entries, double* out);  // the row's sin / cos table as the host builds it (rtm_debug_trig_table)
void release_trig_tab(int device);              // ... and the devices' copies, dropped by release_scratch

// host side: scene input and image output (rtm_scene.cpp, rtm_image.cpp)
int scene_parse_json(const char* text, size_t len, int literal_loader, rtm_settings* st,
                     rtm_sphere* spheres, size_t capacity, size_t* n_spheres);
int scene_parse_json_objects(const char* text, size_t len, int literal_loader, rtm_settings* st,
                             rtm_object* objects, size_t capacity, size_t* n_objects);
int scene_load_json_objects(const char* path, int literal_loader, rtm_settings* st, rtm_object* objects,
                            size_t capacity, size_t* n_objects);
int scene_load_json(const char* path, int literal_loader, rtm_settings* st, rtm_sphere* spheres,
                    size_t capacity, size_t* n_spheres);
int scene_save_sample_json(const char* path);
int scene_make_stress(uint64_t seed, size_t n, rtm_settings* st, rtm_sphere* spheres);
int quantise(const double* image, size_t n_values, uint8_t* out);
int write_bmp(const char* filename, int w, int h, int comp, const void* data);
int write_jpg(const char* filename, int w, int h, int comp, const void* data, int quality);
int write_pfm(const char* filename, int w, int h, int comp, const float* data);
int read_pfm(const char* filename, int* w, int* h, int* comp, float* data, size_t capacity);

}  // namespace rtm
