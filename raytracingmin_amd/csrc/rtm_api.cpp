// rtm_api.cpp — the extern "C" surface of include/rtm.h.  Thin: argument checks live with the
// implementations; no exception crosses the ABI.
#include <exception>

#include "../../include/rtm_debug.h"
#include "rtm_internal.h"

#define RTM_GUARD(call)                                  \
    try {                                                \
        return (call);                                   \
    } catch (const std::exception& e) {                  \
        rtm::set_last_error(e.what());                   \
        return RTM_ERR_INVALID_ARGUMENT;                 \
    } catch (...) {                                      \
        rtm::set_last_error("unknown exception");        \
        return RTM_ERR_INVALID_ARGUMENT;                 \
    }

extern "C" {

int rtm_abi_version(void) { return RTM_ABI_VERSION; }

const char* rtm_strerror(int status) {
    switch (status) {
        case RTM_OK: return "ok";
        case RTM_ERR_INVALID_ARGUMENT: return "invalid argument";
        case RTM_ERR_INVALID_SCENE: return "invalid scene";
        case RTM_ERR_IO: return "i/o error";
        case RTM_ERR_PARSE: return "json parse error";
        case RTM_ERR_NO_DEVICE: return "no HIP device";
        case RTM_ERR_HIP: return "HIP runtime error";
        case RTM_ERR_CAPACITY: return "buffer too small";
        case RTM_ERR_UNSUPPORTED: return "unsupported";
    }
    return "unknown status";
}
const char* rtm_last_error_detail(void) { return rtm::last_error(); }
int rtm_device_count(int* count) { RTM_GUARD(rtm::device_count(count)) }
int rtm_num_variants(void) { return rtm::num_variants(); }
int rtm_output_rows(const rtm_options* options) { return options ? rtm::output_rows(options) : 0; }
int rtm_release_scratch(int device) { RTM_GUARD(rtm::release_scratch(device)) }
int rtm_stream_release(int device, void* stream) { RTM_GUARD(rtm::stream_release(device, stream)) }
int rtm_scratch_bytes(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options, uint64_t out_bytes[6]) {
    RTM_GUARD(rtm::scratch_bytes(settings, scene, options, out_bytes))
}
const char* rtm_variant_name(int variant) { return rtm::variant_name(variant); }

int rtm_scene_create(const rtm_sphere* spheres, size_t n_spheres, int spheres_on_device, int device,
                     rtm_scene** out_scene) {
    RTM_GUARD(rtm::scene_create(spheres, n_spheres, spheres_on_device, device, out_scene))
}
int rtm_scene_create_device(const rtm_sphere* spheres_dev, size_t n_spheres, int device, void* stream, rtm_scene** out_scene) {
    RTM_GUARD(rtm::scene_create_device(spheres_dev, n_spheres, device, stream, out_scene))
}
int rtm_scene_create_objects(const rtm_object* objects, size_t n_objects, int device, rtm_scene** out_scene) {
    RTM_GUARD(rtm::scene_create_objects(objects, n_objects, device, out_scene))
}
int rtm_intersect_objects_batch(const rtm_object* objects, const double* org, const double* dir, size_t n, int mode,
                                int32_t* out_hit, double* out_t, double* out_normal) {
    RTM_GUARD(rtm::intersect_objects_batch(objects, org, dir, n, mode, out_hit, out_t, out_normal))
}
int rtm_scene_load_json_objects(const char* path, int literal_loader, rtm_settings* settings,
                                rtm_object* objects, size_t capacity, size_t* n_objects) {
    RTM_GUARD(rtm::scene_load_json_objects(path, literal_loader, settings, objects, capacity, n_objects))
}
int rtm_scene_parse_json_objects(const char* text, size_t len, int literal_loader, rtm_settings* settings,
                                 rtm_object* objects, size_t capacity, size_t* n_objects) {
    RTM_GUARD(rtm::scene_parse_json_objects(text, len, literal_loader, settings, objects, capacity, n_objects))
}
int rtm_scene_nearest(const rtm_scene* scene, const double* org_dev, const double* dir_dev, size_t n_rays,
                      const rtm_hit_buffers* out_dev, void* stream) {
    RTM_GUARD(rtm::scene_nearest(scene, org_dev, dir_dev, n_rays, out_dev, stream))
}
int rtm_scene_occluded(const rtm_scene* scene, const double* org_dev, const double* dir_dev, const double* tmax_dev, size_t n_rays,
                       uint8_t* out_dev, void* stream) {
    RTM_GUARD(rtm::scene_occluded(scene, org_dev, dir_dev, tmax_dev, n_rays, out_dev, stream))
}
int rtm_scene_radiance(const rtm_scene* scene, const double* org_dev, const double* dir_dev, size_t n_rays,
                       const rtm_radiance_params* params, const rtm_radiance_buffers* out_dev, void* stream) {
    RTM_GUARD(rtm::scene_radiance(scene, org_dev, dir_dev, n_rays, params, out_dev, stream))
}
int rtm_scene_destroy(rtm_scene* scene) { RTM_GUARD(rtm::scene_destroy(scene)) }
size_t rtm_scene_size(const rtm_scene* scene) { return rtm::scene_size(scene); }
int rtm_stream_status(int device, void* stream) { RTM_GUARD(rtm::stream_status(device, stream)) }
int rtm_render_scene(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                     double* out_f64_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream,
                     rtm_stats* stats) {
    RTM_GUARD(rtm::render_scene(settings, scene, options, out_f64_dev, out_f32_dev, out_u8_dev, stream, stats))
}
int rtm_render_scene_samples(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                             uint32_t sample_begin, uint32_t sample_end, double* accum_f64_dev, float* out_f32_dev,
                             uint8_t* out_u8_dev, void* stream, rtm_stats* stats) {
    RTM_GUARD(rtm::render_scene_samples(settings, scene, options, sample_begin, sample_end, accum_f64_dev, out_f32_dev,
                                        out_u8_dev, stream, stats))
}
int rtm_render_scene_tiles(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                           uint32_t sample_begin, uint32_t sample_end, const uint32_t* tiles_dev, uint32_t n_tiles,
                           double* accum_f64_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream, rtm_stats* stats) {
    RTM_GUARD(rtm::render_scene_tiles(settings, scene, options, sample_begin, sample_end, tiles_dev, n_tiles, accum_f64_dev,
                                      out_f32_dev, out_u8_dev, stream, stats))
}
size_t rtm_adaptive_work_bytes(const rtm_settings* settings, const rtm_options* options) {
    return rtm::adaptive_work_bytes(settings, options);
}
int rtm_render_adaptive(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                        const rtm_adaptive_params* params, double* accum_f64_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                        uint32_t* tile_samples_dev, void* work_dev, void* stream, rtm_stats* stats) {
    RTM_GUARD(rtm::render_adaptive(settings, scene, options, params, accum_f64_dev, out_f32_dev, out_u8_dev, tile_samples_dev,
                                   work_dev, stream, stats))
}
int rtm_render_aov(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options,
                   const rtm_aov_buffers* out_dev, void* stream) {
    RTM_GUARD(rtm::render_aov(settings, scene, options, out_dev, stream))
}
int rtm_render_mattes(const rtm_settings* settings, const rtm_scene* scene, const rtm_options* options, int32_t layers,
                      const rtm_matte_buffers* out_dev, void* stream) {
    RTM_GUARD(rtm::render_mattes(settings, scene, options, layers, out_dev, stream))
}
int rtm_matte(int32_t width, int32_t height, int32_t layers, int device, const int32_t* layer_id_dev,
              const float* layer_coverage_dev, const int32_t* ids_dev, int32_t n_ids, float* matte_out_dev, void* stream) {
    RTM_GUARD(rtm::matte(width, height, layers, device, layer_id_dev, layer_coverage_dev, ids_dev, n_ids, matte_out_dev, stream))
}
int rtm_composite(const rtm_composite_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                  const float* alpha_dev, const float* background_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream) {
    RTM_GUARD(rtm::composite(params, width, height, device, color_dev, alpha_dev, background_dev, out_f32_dev, out_u8_dev, stream))
}
size_t rtm_denoise_work_bytes(int32_t width, int32_t height) { return rtm::denoise_work_bytes(width, height); }
int rtm_denoise(const rtm_denoise_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                const rtm_aov_buffers* guide_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream) {
    RTM_GUARD(rtm::denoise(params, width, height, device, color_dev, guide_dev, work_dev, out_f32_dev, out_u8_dev, stream))
}
size_t rtm_denoise_variance_work_bytes(int32_t width, int32_t height) { return rtm::denoise_variance_work_bytes(width, height); }
int rtm_denoise_variance(const rtm_denoise_var_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                         const rtm_aov_buffers* guide_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                         float* variance_out_dev, void* stream) {
    RTM_GUARD(rtm::denoise_variance(params, width, height, device, color_dev, guide_dev, work_dev, out_f32_dev, out_u8_dev,
                                    variance_out_dev, stream))
}
size_t rtm_tonemap_work_bytes(int32_t width, int32_t height) { return rtm::tonemap_work_bytes(width, height); }
int rtm_tonemap(const rtm_tonemap_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, rtm_tonemap_stats* stats_out_dev, void* stream) {
    RTM_GUARD(rtm::tonemap(params, width, height, device, color_dev, work_dev, out_f32_dev, out_u8_dev, stats_out_dev, stream))
}
size_t rtm_bloom_work_bytes(int32_t width, int32_t height, int32_t levels) { return rtm::bloom_work_bytes(width, height, levels); }
int rtm_bloom(const rtm_bloom_params* params, int32_t width, int32_t height, int device, const float* color_dev, void* work_dev,
              float* out_f32_dev, uint8_t* out_u8_dev, float* bloom_out_dev, void* stream) {
    RTM_GUARD(rtm::bloom(params, width, height, device, color_dev, work_dev, out_f32_dev, out_u8_dev, bloom_out_dev, stream))
}
size_t rtm_tonemap_local_work_bytes(int32_t width, int32_t height, int32_t levels) {
    return rtm::tonemap_local_work_bytes(width, height, levels);
}
int rtm_tonemap_local(const rtm_tonemap_local_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                      const rtm_tonemap_stats* stats_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                      float* fused_out_dev, void* stream) {
    RTM_GUARD(rtm::tonemap_local(params, width, height, device, color_dev, stats_dev, work_dev, out_f32_dev, out_u8_dev,
                                 fused_out_dev, stream))
}
int rtm_grade(const rtm_grade_params* params, int32_t width, int32_t height, int device, const float* color_dev,
              const float* lut_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream) {
    RTM_GUARD(rtm::grade(params, width, height, device, color_dev, lut_dev, out_f32_dev, out_u8_dev, stream))
}
int rtm_grade_white_balance(float kelvin, float tint, float matrix_out[9]) {
    RTM_GUARD(rtm::grade_white_balance(kelvin, tint, matrix_out))
}
int rtm_lut_parse_cube(const char* text, size_t len, int32_t* size, float domain_min[3], float domain_max[3], float* table,
                       size_t capacity) {
    RTM_GUARD(rtm::lut_parse_cube(text, len, size, domain_min, domain_max, table, capacity))
}
int rtm_lut_load_cube(const char* path, int32_t* size, float domain_min[3], float domain_max[3], float* table, size_t capacity) {
    RTM_GUARD(rtm::lut_load_cube(path, size, domain_min, domain_max, table, capacity))
}
int rtm_firefly(const rtm_firefly_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                float* out_f32_dev, uint8_t* out_u8_dev, uint8_t* mask_out_dev, float* threshold_out_dev, void* stream) {
    RTM_GUARD(rtm::firefly(params, width, height, device, color_dev, out_f32_dev, out_u8_dev, mask_out_dev, threshold_out_dev, stream))
}
int rtm_scopes(const rtm_scope_params* params, int32_t width, int32_t height, int device, const float* color_dev,
               rtm_scope_histogram* hist_out_dev, uint32_t* waveform_out_dev, void* stream) {
    RTM_GUARD(rtm::scopes(params, width, height, device, color_dev, hist_out_dev, waveform_out_dev, stream))
}
int rtm_scope_draw(int32_t columns, int32_t layout, uint32_t gain, int device, const uint32_t* waveform_dev, uint8_t* out_u8_dev,
                   void* stream) {
    RTM_GUARD(rtm::scope_draw(columns, layout, gain, device, waveform_dev, out_u8_dev, stream))
}
int rtm_scope_bin_range(int32_t mode, int32_t bin, float* lo, float* hi) { RTM_GUARD(rtm::scope_bin_range(mode, bin, lo, hi)) }
int rtm_scope_percentile(const rtm_scope_histogram* hist_host, int32_t mode, int32_t channel, double percent, float* value_out,
                         int32_t* bin_out) {
    RTM_GUARD(rtm::scope_percentile(hist_host, mode, channel, percent, value_out, bin_out))
}
int rtm_scope_exposure(const rtm_scope_histogram* hist_host, double percent, double target, float* ev_out) {
    RTM_GUARD(rtm::scope_exposure(hist_host, percent, target, ev_out))
}
int rtm_defocus(const rtm_defocus_params* params, int32_t width, int32_t height, int device, const float* color_dev,
                const float* depth_dev, float* out_f32_dev, uint8_t* out_u8_dev, float* coc_out_dev, void* stream) {
    RTM_GUARD(rtm::defocus(params, width, height, device, color_dev, depth_dev, out_f32_dev, out_u8_dev, coc_out_dev, stream))
}
int rtm_lens(const rtm_lens_params* params, int32_t width, int32_t height, int device, const float* src_dev, float* out_f32_dev,
             uint8_t* out_u8_dev, void* stream) {
    RTM_GUARD(rtm::lens(params, width, height, device, src_dev, out_f32_dev, out_u8_dev, stream))
}
int rtm_lens_fit_zoom(const rtm_lens_params* params, int32_t width, int32_t height, float* zoom_out) {
    RTM_GUARD(rtm::lens_fit_zoom(params, width, height, zoom_out))
}
size_t rtm_resize_work_bytes(int32_t src_width, int32_t src_height, int32_t dst_width, int32_t dst_height, int32_t filter,
                             int32_t channels) {
    return rtm::resize_work_bytes(src_width, src_height, dst_width, dst_height, filter, channels);
}
int rtm_resize(const rtm_resize_params* params, int32_t src_width, int32_t src_height, int32_t dst_width, int32_t dst_height,
               int device, const float* src_dev, void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream) {
    RTM_GUARD(rtm::resize(params, src_width, src_height, dst_width, dst_height, device, src_dev, work_dev, out_f32_dev, out_u8_dev,
                          stream))
}
size_t rtm_upsample_work_bytes(int32_t low_width, int32_t low_height) { return rtm::upsample_work_bytes(low_width, low_height); }
int rtm_upsample(const rtm_upsample_params* params, int32_t low_width, int32_t low_height, int device,
                 const float* color_low_dev, const rtm_aov_buffers* guide_low_dev, const rtm_aov_buffers* guide_high_dev,
                 void* work_dev, float* out_f32_dev, uint8_t* out_u8_dev, void* stream) {
    RTM_GUARD(rtm::upsample(params, low_width, low_height, device, color_low_dev, guide_low_dev, guide_high_dev, work_dev,
                            out_f32_dev, out_u8_dev, stream))
}
size_t rtm_compare_work_bytes(int32_t width, int32_t height) { return rtm::compare_work_bytes(width, height); }
int rtm_compare(const rtm_compare_params* params, int32_t width, int32_t height, int device, const void* a_dev,
                const void* b_dev, void* work_dev, rtm_compare_result* result_out_dev, float* map_out_dev, void* stream) {
    RTM_GUARD(rtm::compare(params, width, height, device, a_dev, b_dev, work_dev, result_out_dev, map_out_dev, stream))
}
size_t rtm_flip_work_bytes(int32_t width, int32_t height) { return rtm::flip_work_bytes(width, height); }
int rtm_flip(const rtm_flip_params* params, int32_t width, int32_t height, int device, const float* a_dev, const float* b_dev,
             void* work_dev, rtm_flip_result* result_out_dev, float* map_out_dev, void* stream) {
    RTM_GUARD(rtm::flip(params, width, height, device, a_dev, b_dev, work_dev, result_out_dev, map_out_dev, stream))
}
int rtm_render_device(const rtm_settings* settings, const rtm_sphere* spheres, size_t n_spheres,
                      int spheres_on_device, const rtm_options* options, double* out_f64_dev,
                      float* out_f32_dev, uint8_t* out_u8_dev, void* stream, rtm_stats* stats) {
    RTM_GUARD(rtm::render_device(settings, spheres, n_spheres, spheres_on_device, options,
                                 out_f64_dev, out_f32_dev, out_u8_dev, stream, stats))
}
int rtm_render(const rtm_settings* settings, const rtm_sphere* spheres, size_t n_spheres,
               const rtm_options* options, double* out_f64, float* out_f32, uint8_t* out_u8,
               rtm_stats* stats) {
    RTM_GUARD(rtm::render_host(settings, spheres, n_spheres, options, out_f64, out_f32, out_u8, stats))
}
int rtm_render_objects(const rtm_settings* settings, const rtm_object* objects, size_t n_objects,
                       const rtm_options* options, double* out_f64, float* out_f32, uint8_t* out_u8,
                       rtm_stats* stats) {
    RTM_GUARD(rtm::render_host_objects(settings, objects, n_objects, options, out_f64, out_f32, out_u8, stats))
}
int rtm_path_trace_batch(const rtm_sphere* spheres, size_t n_spheres, const rtm_options* options,
                         const double* org, const double* dir, size_t n_rays, double* out_radiance,
                         uint32_t* out_draws, uint32_t* out_casts) {
    RTM_GUARD(rtm::path_trace_batch(spheres, n_spheres, options, org, dir, n_rays, out_radiance,
                                    out_draws, out_casts))
}
int rtm_surface_sample_batch(const rtm_sphere* spheres, size_t n_spheres, const rtm_options* options, const double* org,
                             const double* dir, size_t n_rays, double* out_radiance, uint32_t* out_draws, uint32_t* out_casts) {
    RTM_GUARD(rtm::surface_sample_batch(spheres, n_spheres, options, org, dir, n_rays, out_radiance, out_draws, out_casts))
}
int rtm_intersect_batch(const rtm_sphere* spheres, const double* org, const double* dir, size_t n,
                        int mode, int32_t* out_hit, double* out_t, double* out_normal) {
    RTM_GUARD(rtm::intersect_batch(spheres, org, dir, n, mode, out_hit, out_t, out_normal))
}
double rtm_rng_u01(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t index) {
    return rtm::rng_u01_host(seed, pixel, sample, index);
}
int rtm_rng_batch(uint64_t seed, uint32_t pixel0, uint32_t n_pixels, uint32_t sample,
                  uint32_t n_draws, double* out) {
    RTM_GUARD(rtm::rng_batch(seed, pixel0, n_pixels, sample, n_draws, out))
}
/* ---- test and diagnostic hooks: declared in include/rtm_debug.h, not part of the drop-in boundary ---- */
int rtm_debug_math_probe(int op, const double* a, const double* b, size_t n, double* out) {
    RTM_GUARD(rtm::math_probe(op, a, b, n, out))
}

int rtm_debug_component_bench(int which, const rtm_sphere* sp, size_t n, int reps, int blocks, int lds_pad,
                              double* cycles_per_rep) {
    RTM_GUARD(rtm::component_bench(which, sp, n, reps, blocks, lds_pad, cycles_per_rep))
}

int rtm_debug_wf_nearest(int kind, const rtm_sphere* sp, size_t n, const double* org, const double* dir, size_t n_rays,
                         int32_t* out_id, double* out_t) {
    RTM_GUARD(rtm::wf_nearest_probe(kind, sp, n, org, dir, n_rays, out_id, out_t))
}
int rtm_debug_denoise_variance_kernel(int form, const rtm_denoise_var_params* params, int32_t width, int32_t height, int device,
                                      const rtm_aov_buffers* guide_dev, void* work_dev, float* variance_out_dev, void* stream) {
    RTM_GUARD(rtm::denoise_variance_kernel_probe(form, params, width, height, device, guide_dev, work_dev, variance_out_dev, stream))
}
int rtm_debug_defocus_form(int form, const rtm_defocus_params* params, int32_t width, int32_t height, int device,
                           const float* color_dev, const float* depth_dev, float* out_f32_dev, uint8_t* out_u8_dev,
                           float* coc_out_dev, void* stream) {
    RTM_GUARD(rtm::defocus_form_probe(form, params, width, height, device, color_dev, depth_dev, out_f32_dev, out_u8_dev, coc_out_dev,
                                      stream))
}
int rtm_debug_matte_rank(int32_t super_samples, int32_t layers, int device, const int32_t* ids_dev, size_t n_pixels,
                         int32_t* id_out_dev, float* coverage_out_dev, float* alpha_out_dev, void* stream) {
    RTM_GUARD(rtm::matte_rank_probe(super_samples, layers, device, ids_dev, n_pixels, id_out_dev, coverage_out_dev, alpha_out_dev,
                                    stream))
}
int rtm_debug_trig_table(int entries, double* out) { RTM_GUARD(rtm::trig_table_host(entries, out)) }
int rtm_debug_selfcheck(int kind, unsigned long long* mismatches) { RTM_GUARD(rtm::selfcheck(kind, mismatches)) }
int rtm_debug_grid_nearest(const rtm_sphere* sp, size_t n, const double* org, const double* dir, size_t n_rays,
                           int32_t* out_id, double* out_t, uint32_t* out_tests, uint32_t* out_steps, uint64_t* info) {
    RTM_GUARD(rtm::grid_nearest_probe(sp, n, org, dir, n_rays, out_id, out_t, out_tests, out_steps, info))
}
int rtm_debug_grid_build(const rtm_sphere* sp, size_t n, uint64_t* info, double* pads, uint32_t* ranges, size_t ranges_cap,
                         uint32_t* items, size_t items_cap, int32_t* big, size_t big_cap) {
    RTM_GUARD(rtm::grid_build_host(sp, n, info, pads, ranges, ranges_cap, items, items_cap, big, big_cap))
}
int rtm_debug_scene_grid(const rtm_scene* scene, uint64_t* info, uint32_t* ranges, size_t ranges_cap, uint32_t* items,
                         size_t items_cap, int32_t* big, size_t big_cap, uint64_t extra[2]) {
    RTM_GUARD(rtm::scene_grid_probe(scene, info, ranges, ranges_cap, items, items_cap, big, big_cap, extra))
}
int rtm_debug_scene_query(const rtm_scene* scene, int any, const double* org_dev, const double* dir_dev, const double* tmax_dev,
                          size_t n_rays, int32_t* out_object_dev, double* out_t_dev, uint8_t* out_occluded_dev,
                          uint32_t* out_tests_dev, uint32_t* out_steps_dev, void* stream) {
    RTM_GUARD(rtm::scene_query_probe(scene, any, org_dev, dir_dev, tmax_dev, n_rays, out_object_dev, out_t_dev, out_occluded_dev,
                                     out_tests_dev, out_steps_dev, stream))
}
int rtm_debug_scene_facts(const rtm_sphere* sp, size_t n, uint64_t facts[2]) { RTM_GUARD(rtm::scene_facts_host(sp, n, facts)) }
int rtm_debug_zero_term_facts(const rtm_sphere* sp, size_t n, uint64_t facts[2]) { RTM_GUARD(rtm::zero_term_facts_host(sp, n, facts)) }
int rtm_debug_axis_rows(const rtm_sphere* sp, size_t n, double* rows) { RTM_GUARD(rtm::axis_rows_host(sp, n, rows)) }
int rtm_debug_wall_pairs(const rtm_sphere* sp, size_t n, uint64_t facts[2]) { RTM_GUARD(rtm::wall_pairs_host(sp, n, facts)) }
int rtm_debug_tol_lds_bytes(int n, int any_depth, int split, int rows, uint64_t out[2]) { RTM_GUARD(rtm::tol_lds_bytes(n, any_depth, split, rows, out)) }
int rtm_debug_fp64_peak(int waves_per_simd, double min_ms, double* tflops, double* kernel_ms) {
    RTM_GUARD(rtm::fp64_peak(waves_per_simd, min_ms, tflops, kernel_ms))
}

int rtm_scene_load_json(const char* path, int literal_loader, rtm_settings* settings,
                        rtm_sphere* spheres, size_t capacity, size_t* n_spheres) {
    RTM_GUARD(rtm::scene_load_json(path, literal_loader, settings, spheres, capacity, n_spheres))
}
int rtm_scene_parse_json(const char* text, size_t len, int literal_loader, rtm_settings* settings,
                         rtm_sphere* spheres, size_t capacity, size_t* n_spheres) {
    RTM_GUARD(rtm::scene_parse_json(text, len, literal_loader, settings, spheres, capacity, n_spheres))
}
int rtm_scene_save_sample_json(const char* path) { RTM_GUARD(rtm::scene_save_sample_json(path)) }
int rtm_scene_make_stress(uint64_t seed, size_t n, rtm_settings* settings, rtm_sphere* spheres) {
    RTM_GUARD(rtm::scene_make_stress(seed, n, settings, spheres))
}
int rtm_quantise(const double* image, size_t n_values, uint8_t* out) {
    RTM_GUARD(rtm::quantise(image, n_values, out))
}
int rtm_write_bmp(const char* filename, int w, int h, int comp, const void* data) {
    try {
        return rtm::write_bmp(filename, w, h, comp, data);
    } catch (...) {
        return 0;
    }
}
int rtm_write_jpg(const char* filename, int w, int h, int comp, const void* data, int quality) {
    try {
        return rtm::write_jpg(filename, w, h, comp, data, quality);
    } catch (...) {
        return 0;
    }
}
int rtm_write_pfm(const char* filename, int w, int h, int comp, const float* data) {
    try {
        return rtm::write_pfm(filename, w, h, comp, data);
    } catch (...) {
        return 0;
    }
}
int rtm_read_pfm(const char* filename, int* w, int* h, int* comp, float* data, size_t capacity) {
    try {
        return rtm::read_pfm(filename, w, h, comp, data, capacity);
    } catch (...) {
        return 0;
    }
}

}  // extern "C"
