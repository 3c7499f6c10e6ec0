// rtm_node.h — what rtm_cli runs on the device (rtm_node.cpp): the single-process multi-GPU render with its RCCL gather, and
// the one-GPU stages of a run, each a host wrapper around one library stage that copies in, calls, copies back and writes files.
#pragma once
#include <string>
#include <vector>

#include "../../include/rtm.h"

// Renders the full frame as `n_devices` parts of interleaved 8-row bands (device r renders bands r,
// r + n_devices, ...) and gathers the float3 image and its 8-bit view on device 0 with one grouped
// ncclSend/ncclRecv exchange (taken for n_devices > 1, and for n_devices == 1 when force_rccl is set:
// communicator init + a grouped self send/recv); virtual_strips > 0 instead renders that many parts one
// after another on options->device (same partition and assembly, no RCCL).  Either output may be null.
int rtm_node_render(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* base,
                    int n_devices, int virtual_strips, int force_rccl, float* out_f32_host, uint8_t* out_u8_host,
                    rtm_stats* total, std::string& err);
// The frame's samples in `passes` contiguous, near-equal ranges on options->device (rtm_render_scene_samples, rtm_cli
// --passes), printing "pass i/N: samples [a, b) <ms> ms" per pass.  The outputs are rtm_render_scene's frame.
int rtm_node_render_passes(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* options, int passes,
                           float* out_f32_host, uint8_t* out_u8_host, rtm_stats* total, std::string& err);
// The frame rendered tile-adaptively on options->device (rtm_render_adaptive, rtm_cli --adaptive), printing the mean
// samples per pixel.  tile_samples receives the per-tile sample map (tiles_y x tiles_x).  Outputs as rtm_node_render_passes.
int rtm_node_render_adaptive(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* options,
                             const rtm_adaptive_params* params, float* out_f32_host, uint8_t* out_u8_host,
                             std::vector<uint32_t>& tile_samples, rtm_stats* total, std::string& err);
// The first-hit feature buffers of the whole frame on options->device (rtm_render_aov, rtm_cli --aov), written next to the
// image: <stem>_depth.pfm, <stem>_normal.pfm, <stem>_albedo.pfm (the exact float planes), <stem>_normal.bmp (the quantised
// 0.5 n + 0.5) and <stem>_albedo.bmp (the quantised albedo).
int rtm_node_write_aov(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* options,
                       const std::string& stem, std::string& err);
// The coverage AOVs of the whole frame on options->device (rtm_render_mattes, rtm_cli --alpha / --matte / --background),
// written next to the image: with want_alpha <stem>_alpha.pfm; with ids (1..64 of them) <stem>_matte.pfm, rtm_matte of those
// objects over `layers` ranked layers, and a grey <stem>_matte.bmp; with background, <stem>_over.bmp and <stem>_over.jpg
// (quality 60), rtm_composite of f32_host (HOST, height x width x 3: the frame of the last stage) over that colour, and in
// *over_out (nullable) its float frame.
int rtm_node_write_mattes(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* options, bool want_alpha,
                          int layers, const std::vector<int32_t>& ids, const rtm_composite_params* background,
                          const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* over_out);
// The frame's f32 (HOST, height x width x 3) denoised on options->device at the default parameters (rtm_denoise guided by
// the frame's rtm_render_aov planes, rtm_cli --denoise) and written next to the image: <stem>_denoised.jpg (quality 60)
// and <stem>_denoised.bmp.  f32_out (nullable) receives the filtered float frame, for a stage that follows (--display).
int rtm_node_write_denoised(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* options,
                            const float* f32_host, const std::string& stem, std::string& err,
                            std::vector<float>* f32_out = nullptr);
// The same frame through the variance-guided filter (rtm_denoise_variance at its default parameters, rtm_cli
// --denoise-variance): <stem>_denoised_var.jpg (quality 60), <stem>_denoised_var.bmp and <stem>_variance.pfm, the per-pixel
// variance estimate v0.  f32_out as rtm_node_write_denoised's.
int rtm_node_write_denoised_variance(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* options,
                                     const float* f32_host, const std::string& stem, std::string& err,
                                     std::vector<float>* f32_out = nullptr);
// The display transform (rtm_tonemap, rtm_cli --display) of a float frame (HOST, height x width x 3) on device `device`,
// written next to the image: <stem>_display.jpg (quality 60) and <stem>_display.bmp.  stats (nullable) receives the frame
// statistics and the exposure that was applied; f32_out (nullable) the transform's float frame (rtm_tonemap's out_f32), for a
// stage that follows (--flip, --display-pfm).
// lut (nullable, rtm_cli --lut): a display-referred look.  The table is copied to the device, rtm_grade applies it in place
// to the transform's float frame, and the 8-bit files and f32_out are made from that frame by a second rtm_tonemap call
// that only clamps and dithers: {CLAMP, LINEAR, no auto exposure, ev 0, params->dither}.
// local (nullable, rtm_cli --display local): the local tone operator (rtm_tonemap_local) in the tone curve's stead.  A
// statistics-only rtm_tonemap call with params' key fills stats; the operator runs in place on the frame's device copy with
// anchor 1 and those statistics (automatic exposure) or with anchor 2^ev and none; then rtm_tonemap runs as {CLAMP,
// params->transfer, no auto exposure, ev 0, params->dither}, and the look, if any, follows as above.  local->anchor is ignored.
struct rtm_node_lut {
    rtm_grade_params params;   // RTM_GRADE_DEFAULTS but for lut_size, lut_interp, lut_min, lut_max
    std::vector<float> table;  // 3 lut_size^3 floats in .cube order
};
int rtm_node_write_display(const rtm_settings* st, int device, const rtm_tonemap_params* params, const float* f32_host,
                           const std::string& stem, rtm_tonemap_stats* stats, std::string& err,
                           std::vector<float>* f32_out = nullptr, const rtm_node_lut* lut = nullptr,
                           const rtm_tonemap_local_params* local = nullptr);
// The parametric colour grade (rtm_grade without a LUT, rtm_cli --grade-...) of a float frame (HOST, height x width x 3) on
// device `device`: the frame is copied to the device, graded in place by one call on the default stream and copied back
// into f32_out, for the display transform that follows.
int rtm_node_grade(const rtm_settings* st, int device, const rtm_grade_params* params, const float* f32_host,
                   std::vector<float>* f32_out, std::string& err);
// Bloom (rtm_bloom, rtm_cli --bloom) of a float frame (HOST, height x width x 3) on device `device`: the frame is copied to the
// device, bloomed in place by one call on the default stream and copied back into f32_out, for the display transform that
// follows.
int rtm_node_bloom(const rtm_settings* st, int device, const rtm_bloom_params* params, const float* f32_host,
                   std::vector<float>* f32_out, std::string& err);
// The firefly clamp (rtm_firefly, rtm_cli --firefly) of a float frame (HOST, height x width x 3) on device `device`: the frame
// is copied to the device, one rtm_firefly call on the default stream, the frame and the mask are copied back, then
// <stem>_firefly.bmp and <stem>_firefly.jpg (quality 60).  clamped and repaired receive the counts of the mask's 1s and 2s,
// taken on the host; the cleaned float frame comes back in f32_out, for the stages that follow.
int rtm_node_write_firefly(const rtm_settings* st, int device, const rtm_firefly_params* params, const float* f32_host,
                           const std::string& stem, std::string& err, std::vector<float>* f32_out, size_t* clamped,
                           size_t* repaired);
// The frame scopes (rtm_scopes, rtm_cli --scopes and --expose-percentile) of a float frame (HOST, height x width x 3) on device
// `device`: the frame is copied to the device, one rtm_scopes call on the default stream, and the histogram is copied back.
// With `picture` the call also takes the waveform (params->columns wide), draws it with rtm_scope_draw (layout, gain) and copies
// the picture back: 256 rows of params->columns RGB pixels, of 3 params->columns for the parade.
int rtm_node_scopes(const rtm_settings* st, int device, const rtm_scope_params* params, const float* f32_host,
                    rtm_scope_histogram* hist, int layout, uint32_t gain, std::vector<uint8_t>* picture, std::string& err);
// Depth of field (rtm_defocus, rtm_cli --dof) of a float frame (HOST, height x width x 3) on device opt->device: the frame's depth
// plane (rtm_render_aov), one rtm_defocus call behind it on the default stream, then <stem>_dof.bmp and <stem>_dof.jpg
// (quality 60); the defocused float frame comes back in f32_out, for the stages that follow.
int rtm_node_write_dof(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt,
                       const rtm_defocus_params* params, const float* f32_host, const std::string& stem, std::string& err,
                       std::vector<float>* f32_out);
// Lens distortion, chromatic aberration and vignette (rtm_lens, rtm_cli --lens ...) of a float frame (HOST, height x width x 3)
// on device `device`: one rtm_lens call on the default stream, then <stem>_lens.bmp and <stem>_lens.jpg (quality 60); the
// float frame comes back in f32_out, for the stages that follow.
int rtm_node_write_lens(const rtm_settings* st, int device, const rtm_lens_params* params, const float* f32_host,
                        const std::string& stem, std::string& err, std::vector<float>* f32_out);
// Resize (rtm_resize, rtm_cli --resize) of a float frame (HOST, height x width x 3) on device `device` to dst_width x dst_height:
// one rtm_resize call on the default stream, then <stem>_resized.bmp and <stem>_resized.jpg (quality 60) at the new size; the
// resized float frame comes back in f32_out, for the stages that follow.
int rtm_node_write_resized(const rtm_settings* st, int device, const rtm_resize_params* params, int dst_width, int dst_height,
                           const float* f32_host, const std::string& stem, std::string& err, std::vector<float>* f32_out);
// The depth AOV at pixel (x, y) of the frame, which must lie inside it (rtm_cli --focus-pixel): +inf on a miss.
int rtm_node_depth_at(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* opt, int x, int y,
                      float* depth, std::string& err);
// Two float frames (HOST, height x width x 3; `frame` under test, `reference`) compared on device `device` (rtm_compare at its
// default parameters, rtm_cli --compare): both are copied to the device, one call on the default stream, the record copied back.
int rtm_node_compare(const rtm_settings* st, int device, const float* frame_host, const float* reference_host,
                     rtm_compare_result* result, std::string& err);
// The perceptual difference of two display-referred float frames (HOST, height x width x 3; `frame` under test, `reference`)
// on device `device` (rtm_flip, rtm_cli --flip): both are copied to the device, one call on the default stream, the record
// copied back; map_out (nullable) receives the height x width error map.
int rtm_node_flip(const rtm_settings* st, int device, const rtm_flip_params* params, const float* frame_host,
                  const float* reference_host, rtm_flip_result* result, std::vector<float>* map_out, std::string& err);
// The preview of the frame on options->device (rtm_cli --preview F): the scene traced at (width / factor) x (height / factor)
// with the same camera, samples, seed and mode, denoised there at the default parameters (rtm_denoise guided by the low
// rtm_render_aov planes) and brought to full size by rtm_upsample at its default sigmas, guided by the AOVs at both
// resolutions; written next to the image: <stem>_preview.jpg (quality 60) and <stem>_preview.bmp.  factor must divide the
// width and the height.  f32_out (nullable) receives the float frame, for a stage that follows (--display); stats
// (nullable) the low render's.
int rtm_node_write_preview(const rtm_settings* st, const rtm_object* objects, size_t n, const rtm_options* options, int factor,
                           const std::string& stem, std::string& err, std::vector<float>* f32_out = nullptr,
                           rtm_stats* stats = nullptr);
