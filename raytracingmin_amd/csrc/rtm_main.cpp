// rtm_main.cpp — host program: the reference's main() (src/main.cpp:8-46) on top of the C ABI.
//
//   rtm_cli [-?] [-json <file>] [-sampleJson]            (the reference's flags, same defaults)
//           [--width N] [--height N] [--samples N] [--superSamples N] [--spp N]
//           [--mode literal|repaired] [--max-bounces N] [--seed N] [--device N] [--out STEM] [--device-trig]
//           [--gpus N] [--virtual-strips N] [--force-rccl]   (interleaved 8-row bands over N GPUs + one RCCL gather)
//           [--dump-f32 FILE]                    (the gathered float3 buffer, raw little-endian floats)
//           [--adaptive T [--adaptive-min M]]   (tile-adaptive sampling on one GPU, + STEM_spp.pfm)
//           [--passes N]                         (progressive: the frame's samples in N passes on one GPU, same image)
//           [--aov]                              (first-hit feature buffers next to the image: STEM_depth/_normal/_albedo.pfm, .bmp)
//           [--firefly [K]] [--firefly-rank N] [--firefly-radius R] [--firefly-floor F] [--firefly-keep-nonfinite]
//                                                (the firefly clamp of the frame, before every stage below: STEM_firefly.bmp, .jpg)
//           [--scopes [--scopes-columns N] [--scopes-layout luma|overlay|parade]]
//                                                (histograms, percentiles and the waveform of the last frame and of the display
//                                                 frame: one line scopes: {...}, STEM_scopes.json, STEM_waveform.bmp)
//           [--expose-percentile P[,TARGET]]     (with --display: the exposure that puts luminance percentile P at TARGET)
//           [--denoise]                          (the à-trous denoiser next to the image: STEM_denoised.bmp, .jpg)
//           [--denoise-variance]                 (the variance-guided one: STEM_denoised_var.bmp, .jpg, STEM_variance.pfm)
//           [--display [clamp|reinhard|aces|local]] [--exposure auto|EV] [--linear] [--no-dither]
//                                                (the display transform of the last stage: STEM_display.bmp, .jpg)
//           [--local-shadows S] [--local-highlights S] [--local-sigma V] [--local-levels N]
//                                                (with --display local: the local tone operator's parameters)
//           [--bloom [INTENSITY]] [--bloom-threshold T] [--bloom-levels L]
//                                                (with --display: bloom the frame before the display transform)
//           [--grade-temperature K] [--grade-tint T] [--grade-exposure EV] [--grade-contrast C[,PIVOT]]
//           [--grade-slope R,G,B|S] [--grade-offset R,G,B|S] [--grade-power R,G,B|S] [--grade-saturation S]
//                                                (with --display: the colour grade of the frame, in linear light after --bloom
//                                                and before the display transform)
//           [--lut FILE.cube] [--lut-interp trilinear|tetrahedral]
//                                                (with --display: a look LUT applied to the display transform's float frame)
//           [--dof [APERTURE]] [--focus DISTANCE | --focus-pixel X,Y] [--dof-radius R]
//                                                (depth of field of the last stage by the depth plane: STEM_dof.bmp, .jpg; the
//                                                defocused frame then is the last stage's for what follows)
//           [--lens K1[,K2]] [--lens-inverse] [--lens-ca X] [--lens-vignette A[,F]] [--lens-zoom Z|auto]
//           [--lens-filter nearest|bilinear|bicubic]
//                                                (radial distortion, chromatic aberration and vignette of the last stage:
//                                                STEM_lens.bmp, .jpg; that frame then is the last stage's for what follows)
//           [--resize WxH [--resize-filter box|triangle|mitchell|lanczos3]]
//                                                (the last stage's float frame resized on the device: STEM_resized.bmp, .jpg; the
//                                                resized frame then is the last stage's for --display, --pfm, --display-pfm)
//           [--preview F [--preview-only]]       (the frame traced at 1/F of the resolution per axis, denoised there and upsampled
//                                                by the first-hit feature buffers: STEM_preview.bmp, .jpg; -only: no full render)
//           [--pfm]                              (the float frame of the last stage: STEM.pfm)
//           [--compare REF.pfm]                  (that frame against a reference on the device: one line "compare: {...}")
//           [--display-pfm]                      (with --display: the display transform's float frame, STEM_display.pfm)
//           [--flip REF.pfm [--flip-ppd X] [--flip-map]]
//                                                (the perceptual difference of the display frame, or without --display of the
//                                                last stage's frame taken as linear, from a reference of the same kind: one
//                                                line "flip: {...}"; -map: STEM_flip.pfm)
//           [--alpha] [--matte ID[,ID...] [--matte-layers K]] [--background R,G,B]
//                                                (coverage AOVs on one GPU: STEM_alpha.pfm; the antialiased matte of the listed
//                                                objects, STEM_matte.pfm, .bmp; the last stage's frame over a constant
//                                                background, STEM_over.bmp, .jpg, with --display also STEM_over_display.*)
//
// Flow of the reference: pick the JSON (default settingData.json), create the sample JSON when it
// does not exist, load, render, write <stem>.jpg (quality 60) and <stem>.bmp with stem "result".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtm.h"
#include "rtm_node.h"

static bool file_exists(const std::string& p) {
    FILE* f = std::fopen(p.c_str(), "rb");
    if (f) std::fclose(f);
    return f != nullptr;
}

// a double as JSON: the shortest text that reads back to the same bits; Infinity / NaN as Python's json module writes them
static std::string json_number(double v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// a number, all of it: false for an empty text and for one with anything behind the number
static bool parse_number(const std::string& text, double& v) {
    char* end = nullptr;
    v = std::strtod(text.c_str(), &end);
    return !text.empty() && end == text.c_str() + text.size();
}

// the line of a stage that failed, and the exit status
static int fail(const char* stage, int rc, const std::string& detail) {
    std::fprintf(stderr, "%s failed: %s (%s)\n", stage, rtm_strerror(rc), detail.c_str());
    return 1;
}

// the reference frame of --compare or --flip (`flag`): a three-channel float map of the frame's size
static bool read_reference(const char* flag, const std::string& path, const rtm_settings& st, std::vector<float>& out) {
    int rw = 0, rh = 0, rcomp = 0;
    bool ok = rtm_read_pfm(path.c_str(), &rw, &rh, &rcomp, nullptr, 0) == 1;
    if (ok && (rw != st.width || rh != st.height || rcomp != 3)) {
        std::fprintf(stderr, "%s: %s is %d x %d x %d, the frame is %d x %d x 3\n", flag, path.c_str(), rw, rh, rcomp, st.width,
                     st.height);
        return false;
    }
    if (ok) {
        out.resize((size_t)rw * rh * 3);
        ok = rtm_read_pfm(path.c_str(), &rw, &rh, &rcomp, out.data(), out.size()) == 1;
    }
    if (!ok) std::fprintf(stderr, "%s: cannot read %s as a little-endian float map\n", flag, path.c_str());
    return ok;
}

static void usage() {
    std::printf(
        "Usage: rtm_cli [OPTION]...\n\n"
        "-sampleJson : save the sample scene json file as settingData.json\n"
        "-json <file> : scene json file; settingData.json when not given\n"
        "--width/--height/--samples/--superSamples N : override the file's values\n"
        "--spp N : samples = N / superSamples^2\n"
        "--mode literal|repaired (default repaired), --max-bounces N (default -1 = unlimited)\n"
        "--seed N, --device N, --out STEM (default result)\n"
        "--device-trig : the device's own sin/cos instead of this host's libm values (default: host values, bit-identical\n"
        "              to a CPU run of the reference even where deep paths amplify one-ulp differences; device-trig is ~2 %% faster)\n"
        "--gpus N : interleaved 8-row bands over N GPUs of this node, one RCCL gather of the float3 buffer;\n"
        "--force-rccl : take the RCCL exchange with --gpus 1 too; --virtual-strips N : N parts on one GPU, no RCCL\n"
        "--dump-f32 FILE : write the float3 accumulation buffer (raw floats, row-major RGB)\n"
        "--passes N : render the frame's samples in N near-equal passes on one GPU (rtm_render_scene_samples), printing\n"
        "             each pass's sample range and time; the image is the one-pass image bit for bit\n"
        "--aov : also write the first-hit feature buffers on one GPU (rtm_render_aov): STEM_depth.pfm, STEM_normal.pfm,\n"
        "        STEM_albedo.pfm and the quantised STEM_normal.bmp (0.5 n + 0.5), STEM_albedo.bmp\n"
        "--adaptive T [--adaptive-min M] : tile-adaptive sampling on one GPU (rtm_render_adaptive, threshold T, first pass\n"
        "             M samples, default 16); also writes STEM_spp.pfm, the samples each pixel traced\n"
        "--firefly [K] [--firefly-rank N] [--firefly-radius R] [--firefly-floor F] [--firefly-keep-nonfinite] : also write the frame\n"
        "            with its fireflies clamped on one GPU (rtm_firefly): STEM_firefly.bmp and STEM_firefly.jpg.  A pixel whose\n"
        "            luminance exceeds K (default 4, at least 1) times the N-th largest luminance (1..8, default 3) among its\n"
        "            (2R+1)^2 - 1 neighbours (R in 1..3, default 1), plus F (default 0.01, not negative), is scaled down to that\n"
        "            threshold; a pixel with a non-finite component becomes the mean of its finite neighbours, unless\n"
        "            --firefly-keep-nonfinite is given.  Prints one line 'firefly: {...}', the counts of clamped and repaired pixels\n"
        "            as JSON.  The cleaned frame then is the frame every later stage takes: --denoise, --denoise-variance, --dof,\n"
        "            --lens, --resize, --display (with --bloom), --pfm, --compare, --flip and --background\n"
        "--scopes [--scopes-columns N] [--scopes-layout luma|overlay|parade] : measure the last linear float frame (the frame --pfm\n"
        "            would write) on one GPU (rtm_scopes): per-channel histograms of Y, R, G, B at 8 bins a stop from 2^-16 to 2^16,\n"
        "            and, with --display, the display frame's at the 256 8-bit code values.  Prints one line 'scopes: {...}' as\n"
        "            JSON: the pixels that count and that do not, the luminance percentiles 1, 50, 99 and 99.9, the share of\n"
        "            pixels below and above the bins per channel, the same under \"display\" for the display frame; writes\n"
        "            STEM_scopes.json (that object plus the full histograms) and STEM_waveform.bmp, the waveform (rtm_scope_draw)\n"
        "            of the display frame when there is one, else of the linear frame: N columns (default min(256, width)), 256\n"
        "            rows, layout luma (default), overlay or parade (three panels), gain max(1, 2040 / height) per count\n"
        "--expose-percentile P[,TARGET] : with --display and a global curve, run the display transform at the exposure that puts\n"
        "            the luminance percentile P (0..100) of the frame it takes at TARGET (default 0.18): rtm_scope_exposure of that\n"
        "            frame's histogram, in --exposure's stead; the stops chosen are printed, in the scopes: line with --scopes\n"
        "--denoise : also write the frame denoised on one GPU (rtm_denoise at its default parameters, guided by the\n"
        "            frame's first-hit feature buffers): STEM_denoised.bmp and STEM_denoised.jpg\n"
        "--denoise-variance : also write the frame through the variance-guided denoiser on one GPU (rtm_denoise_variance at\n"
        "            its default parameters; for frames whose noise is uneven, such as --adaptive's): STEM_denoised_var.bmp,\n"
        "            STEM_denoised_var.jpg and STEM_variance.pfm, the per-pixel variance estimate\n"
        "--display [clamp|reinhard|aces|local] : also write the display transform (rtm_tonemap; default aces) of the last stage\n"
        "            asked for on one GPU (the --denoise-variance frame, else the --denoise frame, else the frame itself):\n"
        "            STEM_display.bmp and STEM_display.jpg.  --exposure auto|EV : Reinhard's log-average key 0.18 (default) or\n"
        "            a fixed number of stops; --linear : no sRGB transfer function; --no-dither : the truncating 8-bit store\n"
        "            local : the local tone operator in the curve's stead (rtm_tonemap_local: exposure fusion on luminance at\n"
        "            that exposure, after --bloom and --grade-..., then the clamp, the transfer function and the store).\n"
        "            --local-shadows S --local-highlights S : the stops, 0..8, the shadow exposure is opened and the highlight\n"
        "            exposure closed by (default 2 and 2); --local-sigma V : the width of the well-exposedness weight, 0.1..1\n"
        "            (default 0.25); --local-levels N : the depth of the pyramid, 0..8 (default 5; 0 blends per pixel)\n"
        "--bloom [INTENSITY] [--bloom-threshold T] [--bloom-levels L] : with --display, bloom every frame the display transform\n"
        "            is given (rtm_bloom: a bright pass above luminance T, default 1, a pyramid of L levels, 1..8, default 6, and\n"
        "            INTENSITY, default 0.2, times the result added back in linear space): STEM_display.*, STEM_preview_display.*,\n"
        "            STEM_over_display.*, --display-pfm and what --flip sees are those of the bloomed frame\n"
        "--grade-temperature K [--grade-tint T] --grade-exposure EV --grade-contrast C[,PIVOT] --grade-slope R,G,B|S\n"
        "            --grade-offset R,G,B|S --grade-power R,G,B|S --grade-saturation S : with --display, grade every frame the\n"
        "            display transform is given (rtm_grade, in linear light after --bloom): white balance from a source at K kelvin\n"
        "            (1667..25000, tint T in [-0.05, 0.05], rtm_grade_white_balance) to D65, exposure in stops (|EV| <= 32), contrast\n"
        "            C in [0.25, 4] about PIVOT (default 0.18), the ASC CDL's slope (>= 0), offset and power ([0.1, 10]), one number\n"
        "            or three, saturation in [0, 4]; what is not given stays at its default and is skipped\n"
        "--lut FILE.cube [--lut-interp trilinear|tetrahedral] : with --display, a display-referred look: the 3D LUT of the .cube\n"
        "            file (rtm_lut_load_cube) applied to the display transform's float frame (rtm_grade; default tetrahedral); the\n"
        "            8-bit files are then made from its result by a second rtm_tonemap that only clamps and dithers.\n"
        "            STEM_display.*, STEM_preview_display.*, STEM_over_display.*, --display-pfm and what --flip sees are those\n"
        "            of the graded frame\n"
        "--dof [APERTURE] [--focus DISTANCE | --focus-pixel X,Y] [--dof-radius R] : also write the depth of field (rtm_defocus) of\n"
        "            the last stage asked for on one GPU, by the frame's depth plane: STEM_dof.bmp and STEM_dof.jpg.  APERTURE: the\n"
        "            blur radius, in pixels, of a point at infinity (default 4); --dof-radius R : the largest radius, 1..16 (default\n"
        "            8); the focus is at the camera's target distance, at --focus DISTANCE, or at what pixel X,Y shows.  The\n"
        "            defocused frame then is the frame of the last stage for --pfm, --compare, --flip, --background and --display\n"
        "            (with --bloom: the glare of the defocused frame)\n"
        "--lens K1[,K2] [--lens-inverse] [--lens-ca X] [--lens-vignette A[,F]] [--lens-zoom Z|auto]\n"
        "            [--lens-filter nearest|bilinear|bicubic] : also write the last stage asked for (render, denoiser or --dof) through\n"
        "            a lens on one GPU (rtm_lens, in linear light): STEM_lens.bmp and STEM_lens.jpg.  Any of --lens, --lens-ca,\n"
        "            --lens-vignette, --lens-zoom switches the stage on.  K1, K2: the radial polynomial 1 + K1 r^2 + K2 r^4, r = 1 at\n"
        "            the frame's corner (|K1| <= 0.5, |K2| <= 0.25; K1 < 0 is a barrel); --lens-inverse : take that distortion out\n"
        "            instead of putting it in; --lens-ca X : lateral chromatic aberration, red scaled by 1 + X and blue by 1 - X\n"
        "            (|X| <= 0.05); --lens-vignette A[,F] : cos^4 vignetting, amount A in [0, 1], F in [0, 4] the tangent of the\n"
        "            half field angle at the corner (default 1); --lens-zoom Z : magnification in [0.25, 4] (default 1), auto : the\n"
        "            smallest that hides the border (rtm_lens_fit_zoom); --lens-filter : default bicubic.  Where the source lies\n"
        "            outside the frame the result is black.  The lens frame then is the frame of the last stage for --resize,\n"
        "            --display (with --bloom), --pfm, --compare and --flip; it does not combine with --alpha, --matte or --background\n"
        "--resize WxH [--resize-filter box|triangle|mitchell|lanczos3] : also write the last stage asked for (render, denoiser or\n"
        "            --dof) resized to W x H on one GPU (rtm_resize, in linear light; default filter mitchell; antialiased when it\n"
        "            shrinks): STEM_resized.bmp and STEM_resized.jpg.  The resized frame then is the frame of the last stage for\n"
        "            --display (with --bloom), --pfm and --display-pfm; it does not combine with --compare, --flip, --alpha, --matte\n"
        "            or --background, which work at the render's size\n"
        "--preview F [--preview-only] : also write a fast preview on one GPU: the scene traced at width / F x height / F (F in\n"
        "            2..8, dividing both; F^2 fewer paths), denoised there (rtm_denoise at its defaults) and brought to full size\n"
        "            by rtm_upsample, guided by the first-hit feature buffers at both resolutions: STEM_preview.bmp and\n"
        "            STEM_preview.jpg (with --display also STEM_preview_display.bmp, .jpg).  --preview-only : skip the full\n"
        "            render; STEM.bmp and STEM.jpg are not written\n"
        "--pfm : also write STEM.pfm, the float frame of the last stage asked for (the --denoise-variance frame, else the\n"
        "        --denoise frame, else the frame itself), bit for bit\n"
        "--compare REF.pfm : compare that same frame with the 3-channel float map REF.pfm (the reference) on the device\n"
        "        (rtm_compare at its default parameters: tolerance 1e-4, peak 1, rel_epsilon 1e-2) and print one line\n"
        "        'compare: {...}', the record's fields as JSON; a file that cannot be read or has another size: exit status 1\n"
        "--display-pfm : with --display, also write STEM_display.pfm, the display transform's float frame (sRGB-encoded, or\n"
        "        linear with --linear), bit for bit: what --display --flip takes as its reference\n"
        "--flip REF.pfm [--flip-ppd X] [--flip-map] : the perceptual difference (rtm_flip, LDR FLIP) between the frame and the\n"
        "        3-channel float map REF.pfm (the reference) on the device.  With --display the frame is the display transform's\n"
        "        float frame (sRGB, or linear with --linear) and REF.pfm a --display-pfm file; without it the float frame of the\n"
        "        last stage, taken as linear and clamped to [0, 1], and REF.pfm a --pfm file.  --flip-ppd X : pixels per degree\n"
        "        in [8, 128] (default 67.02: a 0.7 m wide 4K monitor at 0.7 m).  Prints one line 'flip: {...}', the record\n"
        "        without its histogram plus the weighted median, as JSON; --flip-map : also write STEM_flip.pfm, the error map\n"
        "        in [0, 1]; a file that cannot be read or has another size: exit status 1\n"
        "--alpha : also write STEM_alpha.pfm on one GPU (rtm_render_mattes): per pixel the fraction of its superSamples^2\n"
        "        sub-pixels whose primary ray hits anything (superSamples up to 8)\n"
        "--matte ID[,ID...] [--matte-layers K] : also write the antialiased matte of the listed objects (1..64 indices into the\n"
        "        scene's object list; rtm_matte over K ranked id / coverage layers, K in 1..8, default 4): STEM_matte.pfm and a\n"
        "        grey STEM_matte.bmp\n"
        "--background R,G,B : also write the frame of the last stage asked for over that constant colour (rtm_composite with\n"
        "        the alpha plane: frame + (1 - alpha) * colour): STEM_over.bmp and STEM_over.jpg; with --display also its display\n"
        "        transform, STEM_over_display.bmp and STEM_over_display.jpg\n"
        "        These three need the full render (not with --preview-only) and superSamples up to 8; --matte-layers requires\n"
        "        --matte\n");
}

int main(int argc, char* argv[]) {
    // progress lines reach a pipe as they are printed (a caller that has to kill a stalled run still sees how far it got)
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    // N GPUs of ONE node in ONE process: RCCL's bootstrap needs no more than the loopback interface, and a
    // container's veth is not always connectable to itself.  Set before any thread exists; a user's value is kept.
    (void)setenv("NCCL_SOCKET_IFNAME", "lo", 0);
    std::string json_file = "settingData.json", stem = "result";
    int width = 0, height = 0, samples = 0, super_samples = 0, spp = 0;
    int mode = RTM_MODE_REPAIRED, max_bounces = -1, device = 0, gpus = 1, virtual_strips = 0, host_trig = 1, force_rccl = 0;
    int passes = 0, aov = 0, denoise = 0, denoise_variance = 0, adaptive = 0, adaptive_min = 16;
    float adaptive_threshold = 0.f;
    int display = 0, preview = 0, preview_only = 0;
    rtm_tonemap_params display_prm = RTM_TONEMAP_DEFAULTS;
    int bloom = 0;
    rtm_bloom_params bloom_prm = RTM_BLOOM_DEFAULTS;
    int local = 0, local_flag_given = 0;
    rtm_tonemap_local_params local_prm = RTM_TONEMAP_LOCAL_DEFAULTS;
    int grade = 0, grade_temperature_given = 0, grade_tint_given = 0, lut_interp_given = 0;
    float grade_kelvin = 6504.0f, grade_tint = 0.0f;
    rtm_grade_params grade_prm = RTM_GRADE_DEFAULTS;
    std::string lut_file;
    rtm_node_lut look = {RTM_GRADE_DEFAULTS, {}};
    int firefly = 0, firefly_rank_given = 0, firefly_radius_given = 0, firefly_floor_given = 0, firefly_keep_given = 0;
    rtm_firefly_params firefly_prm = RTM_FIREFLY_DEFAULTS;
    int dof = 0, focus_given = 0, focus_pixel_given = 0, dof_radius_given = 0, focus_x = 0, focus_y = 0;
    rtm_defocus_params dof_prm = RTM_DEFOCUS_DEFAULTS;
    int lens = 0, lens_inverse = 0, lens_filter_given = 0, lens_zoom_auto = 0;
    rtm_lens_params lens_prm = RTM_LENS_DEFAULTS;
    int resize = 0, resize_filter_given = 0, resize_w = 0, resize_h = 0;
    rtm_resize_params resize_prm = RTM_RESIZE_DEFAULTS;
    int scopes = 0, scopes_columns = 0, scopes_columns_given = 0, scopes_layout = RTM_SCOPE_LUMA, scopes_layout_given = 0;
    int expose = 0, exposure_given = 0;
    double expose_percent = 0.0, expose_target = 0.18;
    int pfm = 0;
    std::string dump_f32, compare_ref, flip_ref;
    int display_pfm = 0, flip_map = 0, flip_ppd_given = 0;
    rtm_flip_params flip_prm = RTM_FLIP_DEFAULTS;
    int alpha = 0, matte_layers = RTM_MATTE_DEFAULT_LAYERS, matte_layers_given = 0, background = 0;
    std::vector<int32_t> matte_ids;
    rtm_composite_params composite_prm = {{0.0f, 0.0f, 0.0f}};
    unsigned long long seed = 0x5EED;
    for (int i = 1; i < argc; ++i) {
        const std::string c = argv[i];
        auto next_int = [&](int& dst) {
            if (i + 1 < argc) dst = std::atoi(argv[++i]);
        };
        if (c == "-?") {
            usage();
            return 0;
        } else if (c == "-json") {  // src/main.cpp:18-28: falls back when the value is missing or a flag
            if (argc <= i + 1 || argv[i + 1][0] == '-')
                json_file = "settingData.json";
            else
                json_file = argv[++i];
        } else if (c == "-sampleJson") {  // src/main.cpp:29-33
            std::printf("saving the sample scene json file: settingData.json\n");
            return rtm_scene_save_sample_json("settingData.json") == RTM_OK ? 0 : 1;
        } else if (c == "--width") next_int(width);
        else if (c == "--height") next_int(height);
        else if (c == "--samples") next_int(samples);
        else if (c == "--superSamples") next_int(super_samples);
        else if (c == "--spp") next_int(spp);
        else if (c == "--max-bounces") next_int(max_bounces);
        else if (c == "--device") next_int(device);
        else if (c == "--gpus") next_int(gpus);
        else if (c == "--virtual-strips") next_int(virtual_strips);
        else if (c == "--passes") next_int(passes);
        else if (c == "--adaptive" && i + 1 < argc) {
            adaptive = 1;
            adaptive_threshold = (float)std::strtod(argv[++i], nullptr);  // (double first, as Python's float() then C float)
        } else if (c == "--adaptive-min") next_int(adaptive_min);
        else if (c == "--host-trig") host_trig = 1;
        else if (c == "--device-trig") host_trig = 0;
        else if (c == "--force-rccl") force_rccl = 1;
        else if (c == "--aov") aov = 1;
        else if (c == "--preview") next_int(preview);
        else if (c == "--preview-only") preview_only = 1;
        else if (c == "--denoise") denoise = 1;
        else if (c == "--denoise-variance") denoise_variance = 1;
        else if (c == "--display") {
            display = 1;
            const std::string m = i + 1 < argc ? argv[i + 1] : "";
            if (m == "clamp") display_prm.op = RTM_TONEMAP_CLAMP;
            else if (m == "reinhard") display_prm.op = RTM_TONEMAP_REINHARD;
            else if (m == "aces") display_prm.op = RTM_TONEMAP_ACES;
            else if (m == "local") local = 1;
            if (m == "clamp" || m == "reinhard" || m == "aces" || m == "local") ++i;  // anything else is the next option: the default curve
        } else if (c == "--local-shadows" || c == "--local-highlights" || c == "--local-sigma" || c == "--local-levels") {
            // a number, all of it, in range once rounded to float
            const std::string m = i + 1 < argc ? argv[i + 1] : "";
            double v = 0.0;
            bool ok = parse_number(m, v);
            if (ok) ++i;
            local_flag_given = 1;
            const float f = (float)v;
            if (c == "--local-levels") {
                ok = ok && v == std::floor(v) && v >= 0.0 && v <= 8.0;
                if (ok) local_prm.levels = (int)v;
            } else if (c == "--local-sigma") {
                ok = ok && std::isfinite(f) && f >= 0.1f && f <= 1.0f;
                local_prm.sigma = f;
            } else {
                ok = ok && std::isfinite(f) && f >= 0.0f && f <= 8.0f;
                (c == "--local-shadows" ? local_prm.shadows : local_prm.highlights) = f;
            }
            if (!ok) {
                std::fprintf(stderr, "%s takes %s, got %s\n", c.c_str(),
                             c == "--local-levels" ? "a number of levels in 0..8"
                             : c == "--local-sigma" ? "a number in 0.1..1" : "a number of stops in 0..8", m.c_str());
                return 2;
            }
        } else if (c == "--exposure" && i + 1 < argc) {
            const std::string m = argv[++i];
            double ev = 0.0;
            exposure_given = 1;
            if (m == "auto") {
                display_prm.auto_exposure = 1;
                display_prm.ev = 0.0f;
            } else if (parse_number(m, ev)) {
                display_prm.auto_exposure = 0;
                display_prm.ev = (float)ev;  // (double first, as Python's float() then C float)
            } else {
                std::fprintf(stderr, "--exposure takes auto or a number of stops, got %s\n", m.c_str());
                return 2;
            }
        } else if (c == "--linear") display_prm.transfer = RTM_TRANSFER_LINEAR;
        else if (c == "--no-dither") display_prm.dither = 0;
        else if (c == "--bloom" || c == "--bloom-threshold" || c == "--bloom-levels") {
            // a number, all of it; --bloom alone may stand without one (anything that is not a number is the next option)
            const std::string m = i + 1 < argc ? argv[i + 1] : "";
            double v = 0.0;
            const bool number = parse_number(m, v);
            bool ok = number || c == "--bloom";
            if (number) ++i;
            if (c == "--bloom") {
                bloom = 1;
                if (number) ok = std::isfinite(bloom_prm.intensity = (float)v) && v >= 0.0;
            } else if (c == "--bloom-threshold") {
                if (number) ok = std::isfinite(bloom_prm.threshold = (float)v) && v >= 0.0;
            } else if (number) {
                ok = v == std::floor(v) && v >= 1.0 && v <= 8.0;
                if (ok) bloom_prm.levels = (int)v;
            }
            if (!ok) {
                std::fprintf(stderr, "%s takes %s, got %s\n", c.c_str(),
                             c == "--bloom-levels" ? "a number of levels in 1..8" : "a finite number that is not negative", m.c_str());
                return 2;
            }
        }
        else if (c.rfind("--grade-", 0) == 0) {
            // one number, or for the CDL's three one or three (R,G,B), or C[,PIVOT]: all of the text, in range once rounded to float
            const std::string m = i + 1 < argc ? argv[++i] : "";
            float v[3] = {0.0f, 0.0f, 0.0f};
            int count = 0;
            bool ok = true;
            for (size_t b = 0; ok && b <= m.size();) {
                const size_t e = std::min(m.find(',', b), m.size());
                double d = 0.0;
                ok = count < 3 && parse_number(m.substr(b, e - b), d) && std::isfinite(v[count] = (float)d);  // (double first)
                ++count;
                b = e + 1;
            }
            const auto three = [&](float* dst, float lo, float hi) {
                ok = ok && (count == 1 || count == 3);
                for (int k = 0; ok && k < 3; ++k) {
                    dst[k] = v[count == 1 ? 0 : k];
                    ok = dst[k] >= lo && dst[k] <= hi;
                }
            };
            const char* takes = "a finite number";
            if (c == "--grade-temperature") {
                takes = "a number of kelvin in [1667, 25000]";
                ok = ok && count == 1 && v[0] >= 1667.0f && v[0] <= 25000.0f;
                grade_kelvin = v[0];
                grade_temperature_given = 1;
            } else if (c == "--grade-tint") {
                takes = "a number in [-0.05, 0.05]";
                ok = ok && count == 1 && v[0] >= -0.05f && v[0] <= 0.05f;
                grade_tint = v[0];
                grade_tint_given = 1;
            } else if (c == "--grade-exposure") {
                takes = "a number of stops in [-32, 32]";
                ok = ok && count == 1 && v[0] >= -32.0f && v[0] <= 32.0f;
                grade_prm.exposure = v[0];
            } else if (c == "--grade-contrast") {
                takes = "C[,PIVOT] with C in [0.25, 4] and PIVOT positive";
                ok = ok && count <= 2 && v[0] >= 0.25f && v[0] <= 4.0f && (count == 1 || v[1] > 0.0f);
                grade_prm.contrast = v[0];
                if (count == 2) grade_prm.pivot = v[1];
            } else if (c == "--grade-slope") {
                takes = "one number or R,G,B, none negative";
                three(grade_prm.slope, 0.0f, INFINITY);
            } else if (c == "--grade-offset") {
                takes = "one finite number or R,G,B";
                three(grade_prm.offset, -INFINITY, INFINITY);
            } else if (c == "--grade-power") {
                takes = "one number or R,G,B in [0.1, 10]";
                three(grade_prm.power, 0.1f, 10.0f);
            } else if (c == "--grade-saturation") {
                takes = "a number in [0, 4]";
                ok = ok && count == 1 && v[0] >= 0.0f && v[0] <= 4.0f;
                grade_prm.saturation = v[0];
            } else {
                std::fprintf(stderr, "unknown option %s\n", c.c_str());
                return 2;
            }
            if (!ok) {
                std::fprintf(stderr, "%s takes %s, got %s\n", c.c_str(), takes, m.c_str());
                return 2;
            }
            grade = 1;
        } else if (c == "--lut" && i + 1 < argc) {
            lut_file = argv[++i];
        } else if (c == "--lut-interp") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m != "trilinear" && m != "tetrahedral") {
                std::fprintf(stderr, "--lut-interp takes trilinear or tetrahedral, got %s\n", m.c_str());
                return 2;
            }
            lut_interp_given = 1;
            look.params.lut_interp = m == "trilinear" ? RTM_GRADE_TRILINEAR : RTM_GRADE_TETRAHEDRAL;
        }
        else if (c == "--firefly" || c == "--firefly-rank" || c == "--firefly-radius" || c == "--firefly-floor") {
            // a number, all of it; --firefly alone may stand without one (anything that is not a number is the next option)
            const std::string m = i + 1 < argc ? argv[i + 1] : "";
            double v = 0.0;
            const bool number = parse_number(m, v);
            bool ok = number || c == "--firefly";
            if (number) ++i;
            const float f = (float)v;  // (double first, as Python's float() then C float)
            if (c == "--firefly") {
                firefly = 1;
                if (number) ok = std::isfinite(firefly_prm.k = f) && f >= 1.0f;
            } else if (c == "--firefly-floor") {
                firefly_floor_given = 1;
                if (number) ok = std::isfinite(firefly_prm.floor = f) && f >= 0.0f && !std::signbit(f);
            } else {
                const bool is_rank = c == "--firefly-rank";
                (is_rank ? firefly_rank_given : firefly_radius_given) = 1;
                ok = number && v == std::floor(v) && v >= 1.0 && v <= (is_rank ? 8.0 : 3.0);
                if (ok) (is_rank ? firefly_prm.rank : firefly_prm.radius) = (int)v;
            }
            if (!ok) {
                std::fprintf(stderr, "%s takes %s, got %s\n", c.c_str(),
                             c == "--firefly"          ? "a finite number that is at least 1"
                             : c == "--firefly-floor"  ? "a finite number that is not negative (nor -0.0)"
                             : c == "--firefly-rank"   ? "an integer in 1..8"
                                                       : "an integer in 1..3",
                             m.c_str());
                return 2;
            }
        } else if (c == "--firefly-keep-nonfinite") {
            firefly_keep_given = 1;
            firefly_prm.repair = 0;
        }
        else if (c == "--dof" || c == "--focus" || c == "--dof-radius") {
            // a number, all of it; --dof alone may stand without one (anything that is not a number is the next option)
            const std::string m = i + 1 < argc ? argv[i + 1] : "";
            double v = 0.0;
            const bool number = parse_number(m, v);
            bool ok = number || c == "--dof";
            if (number) ++i;
            if (c == "--dof") {
                dof = 1;
                if (number) ok = std::isfinite(dof_prm.aperture = (float)v) && v >= 0.0;
            } else if (c == "--focus") {
                focus_given = 1;
                if (number) ok = std::isfinite(dof_prm.focus_distance = (float)v) && dof_prm.focus_distance > 0.0f;
            } else {
                dof_radius_given = 1;
                ok = number && v == std::floor(v) && v >= 1.0 && v <= 16.0;
                if (ok) dof_prm.max_radius = (int)v;
            }
            if (!ok) {
                std::fprintf(stderr, "%s takes %s, got %s\n", c.c_str(),
                             c == "--dof"     ? "a finite aperture that is not negative"
                             : c == "--focus" ? "a finite distance above zero"
                                              : "a radius in 1..16",
                             m.c_str());
                return 2;
            }
        } else if (c == "--focus-pixel") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            const size_t comma = m.find(',');
            double x = 0.0, y = 0.0;
            const bool ok = comma != std::string::npos && parse_number(m.substr(0, comma), x) && parse_number(m.substr(comma + 1), y) &&
                            x == std::floor(x) && y == std::floor(y) && x >= 0.0 && y >= 0.0 && x <= 2147483647.0 && y <= 2147483647.0;
            if (!ok) {
                std::fprintf(stderr, "--focus-pixel takes a pixel X,Y, two whole numbers from 0, got %s\n", m.c_str());
                return 2;
            }
            focus_pixel_given = 1;
            focus_x = (int)x;
            focus_y = (int)y;
        }
        else if (c == "--lens" || c == "--lens-ca" || c == "--lens-vignette") {
            // one or two comma-separated numbers, all of the text, each in its range once rounded to float
            const std::string m = i + 1 < argc ? argv[++i] : "";
            const size_t comma = m.find(',');
            double v0 = 0.0, v1 = 0.0;
            const bool two = comma != std::string::npos;
            bool ok = parse_number(two ? m.substr(0, comma) : m, v0);
            if (two) ok = ok && c != "--lens-ca" && parse_number(m.substr(comma + 1), v1);  // (--lens-ca takes one number)
            const float f0 = (float)v0, f1 = (float)v1;  // (double first, as Python's float() then C float)
            if (c == "--lens") {
                ok = ok && f0 >= -0.5f && f0 <= 0.5f && (!two || (f1 >= -0.25f && f1 <= 0.25f));
                lens_prm.k1 = f0;
                if (two) lens_prm.k2 = f1;
            } else if (c == "--lens-ca") {
                ok = ok && f0 >= -0.05f && f0 <= 0.05f;
                lens_prm.chroma = f0;
            } else {
                ok = ok && f0 >= 0.0f && f0 <= 1.0f && (!two || (f1 >= 0.0f && f1 <= 4.0f));
                lens_prm.vignette = f0;
                if (two) lens_prm.falloff = f1;
            }
            if (!ok) {
                std::fprintf(stderr, "%s takes %s, got %s\n", c.c_str(),
                             c == "--lens"      ? "K1[,K2] with |K1| <= 0.5 and |K2| <= 0.25"
                             : c == "--lens-ca" ? "a number in [-0.05, 0.05]"
                                                : "A[,F] with A in [0, 1] and F in [0, 4]",
                             m.c_str());
                return 2;
            }
            lens = 1;
        } else if (c == "--lens-zoom") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            double v = 0.0;
            if (m == "auto")
                lens_zoom_auto = 1;
            else if (parse_number(m, v) && (float)v >= 0.25f && (float)v <= 4.0f) {
                lens_zoom_auto = 0;
                lens_prm.zoom = (float)v;
            } else {
                std::fprintf(stderr, "--lens-zoom takes auto or a number in [0.25, 4], got %s\n", m.c_str());
                return 2;
            }
            lens = 1;
        } else if (c == "--lens-inverse") {
            lens_inverse = 1;
            lens_prm.mode = RTM_LENS_INVERSE;
        } else if (c == "--lens-filter") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            static const char* const names[] = {"nearest", "bilinear", "bicubic"};  // RTM_LENS_*, in the enum's order
            int which = -1;
            for (int k = 0; k < 3; ++k)
                if (m == names[k]) which = k;
            if (which < 0) {
                std::fprintf(stderr, "--lens-filter takes nearest, bilinear or bicubic, got %s\n", m.c_str());
                return 2;
            }
            lens_filter_given = 1;
            lens_prm.filter = which;
        }
        else if (c == "--resize") {
            // WxH: two whole numbers from 1, all of the text
            const std::string m = i + 1 < argc ? argv[++i] : "";
            const size_t x = m.find('x');
            double vw = 0.0, vh = 0.0;
            const bool ok = x != std::string::npos && parse_number(m.substr(0, x), vw) && parse_number(m.substr(x + 1), vh) &&
                            vw == std::floor(vw) && vh == std::floor(vh) && vw >= 1.0 && vh >= 1.0 && vw <= 2147483647.0 &&
                            vh <= 2147483647.0;
            if (!ok) {
                std::fprintf(stderr, "--resize takes a size WxH, two whole numbers from 1, got %s\n", m.c_str());
                return 2;
            }
            resize = 1;
            resize_w = (int)vw;
            resize_h = (int)vh;
        } else if (c == "--resize-filter") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            static const char* const names[] = {"box", "triangle", "mitchell", "lanczos3"};  // RTM_RESIZE_*, in the enum's order
            int which = -1;
            for (int k = 0; k < 4; ++k)
                if (m == names[k]) which = k;
            if (which < 0) {
                std::fprintf(stderr, "--resize-filter takes box, triangle, mitchell or lanczos3, got %s\n", m.c_str());
                return 2;
            }
            resize_filter_given = 1;
            resize_prm.filter = which;
        }
        else if (c == "--scopes") scopes = 1;
        else if (c == "--scopes-columns") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            double v = 0.0;
            scopes_columns_given = 1;
            if (!parse_number(m, v) || v != std::floor(v) || v < 1.0 || v > 2147483647.0) {
                std::fprintf(stderr, "--scopes-columns takes a whole number of columns from 1, got %s\n", m.c_str());
                return 2;
            }
            scopes_columns = (int)v;
        } else if (c == "--scopes-layout") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            scopes_layout_given = 1;
            if (m == "luma") scopes_layout = RTM_SCOPE_LUMA;
            else if (m == "overlay") scopes_layout = RTM_SCOPE_OVERLAY;
            else if (m == "parade") scopes_layout = RTM_SCOPE_PARADE;
            else {
                std::fprintf(stderr, "--scopes-layout takes luma, overlay or parade, got %s\n", m.c_str());
                return 2;
            }
        } else if (c == "--expose-percentile") {
            // P or P,TARGET: a percent in [0, 100] and a positive finite target
            const std::string m = i + 1 < argc ? argv[++i] : "";
            const size_t comma = m.find(',');
            expose = 1;
            bool ok = parse_number(m.substr(0, comma), expose_percent) && expose_percent >= 0.0 && expose_percent <= 100.0;
            if (ok && comma != std::string::npos)
                ok = parse_number(m.substr(comma + 1), expose_target) && std::isfinite(expose_target) && expose_target > 0.0;
            if (!ok) {
                std::fprintf(stderr, "--expose-percentile takes P or P,TARGET, a percent in 0..100 and a positive target, got %s\n",
                             m.c_str());
                return 2;
            }
        }
        else if (c == "--pfm") pfm = 1;
        else if (c == "--compare" && i + 1 < argc) compare_ref = argv[++i];
        else if (c == "--display-pfm") display_pfm = 1;
        else if (c == "--flip" && i + 1 < argc) flip_ref = argv[++i];
        else if (c == "--flip-map") flip_map = 1;
        else if (c == "--flip-ppd" && i + 1 < argc) {
            const std::string m = argv[++i];
            flip_ppd_given = 1;
            double& ppd = flip_prm.pixels_per_degree;
            if (!parse_number(m, ppd) || !(ppd >= 8.0 && ppd <= 128.0)) {
                std::fprintf(stderr, "--flip-ppd takes a number of pixels per degree in [8, 128], got %s\n", m.c_str());
                return 2;
            }
        } else if (c == "--alpha") alpha = 1;
        else if (c == "--matte" || c == "--background" || c == "--matte-layers") {
            // a comma-separated list of numbers, all of it: 1..64 object indices, three finite colour components, or K in 1..8
            const std::string m = i + 1 < argc ? argv[++i] : "";
            std::vector<double> v;
            bool ok = !m.empty();
            for (size_t at = 0; ok && at <= m.size();) {
                const size_t comma = std::min(m.find(',', at), m.size());
                double d = 0.0;
                ok = parse_number(m.substr(at, comma - at), d) && std::isfinite(d);
                v.push_back(d);
                at = comma + 1;
            }
            if (c == "--matte") {
                ok = ok && v.size() <= 64;
                for (size_t k = 0; ok && k < v.size(); ++k) ok = v[k] == std::floor(v[k]) && v[k] >= -2147483648.0 && v[k] <= 2147483647.0;
                if (ok) matte_ids.assign(v.begin(), v.end());
            } else if (c == "--background") {
                ok = ok && v.size() == 3;
                for (size_t k = 0; ok && k < 3; ++k) ok = std::isfinite(composite_prm.background[k] = (float)v[k]);
                background = 1;
            } else {
                ok = ok && v.size() == 1 && v[0] == std::floor(v[0]) && v[0] >= 1.0 && v[0] <= 8.0;
                if (ok) matte_layers = (int)v[0];
                matte_layers_given = 1;
            }
            if (!ok) {
                std::fprintf(stderr, "%s takes %s, got %s\n", c.c_str(),
                             c == "--matte" ? "1..64 comma-separated object indices" : c == "--background" ? "three finite numbers R,G,B"
                                                                                                         : "a number of layers in 1..8",
                             m.c_str());
                return 2;
            }
        } else if (c == "--dump-f32" && i + 1 < argc) dump_f32 = argv[++i];
        else if (c == "--seed" && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 0);
        else if (c == "--out" && i + 1 < argc) stem = argv[++i];
        else if (c == "--mode" && i + 1 < argc) {
            const std::string m = argv[++i];
            if (m == "literal") mode = RTM_MODE_LITERAL;
            else if (m == "repaired") mode = RTM_MODE_REPAIRED;
            else {
                std::fprintf(stderr, "unknown mode %s\n", m.c_str());
                return 2;
            }
        }
    }
    // What does not combine, in the order it is looked at: the first refusal that applies is the one that is printed.
    const bool many = gpus > 1 || virtual_strips > 0 || force_rccl;  // anything but the plain one-GPU render
    const bool mattes = alpha || !matte_ids.empty() || background;
    const std::string bad_preview = "--preview takes a factor in 2..8, got " + std::to_string(preview);
    const struct {
        bool applies;
        const char* text;
    } refusals[] = {
        {passes > 0 && many,
         "--passes renders on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {adaptive && (passes > 0 || many),
         "--adaptive renders on one GPU: it does not combine with --passes, --gpus > 1, --virtual-strips or --force-rccl"},
        {aov && many, "--aov renders on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {denoise && many, "--denoise runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {denoise_variance && many,
         "--denoise-variance runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {(grade || !lut_file.empty()) && many,
         "--grade-... and --lut run on one GPU: they do not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {display && many, "--display runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {preview_only && preview == 0, "--preview-only requires --preview F"},
        {preview != 0 && (preview < 2 || preview > 8), bad_preview.c_str()},
        {preview && many, "--preview runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {preview_only && (adaptive || passes > 0),
         "--preview-only skips the full render: it does not combine with --adaptive or --passes"},
        {preview_only && (denoise || denoise_variance || !dump_f32.empty()),
         "--preview-only skips the full render: it does not combine with --denoise, --denoise-variance or --dump-f32"},
        {preview_only && (pfm || !compare_ref.empty()),
         "--preview-only skips the full render: it does not combine with --pfm or --compare"},
        {preview_only && !flip_ref.empty(), "--preview-only skips the full render: it does not combine with --flip"},
        {display_pfm && (!display || preview_only),
         "--display-pfm writes the display transform's float frame of the full render: it requires --display and does not combine "
         "with --preview-only"},
        {local_flag_given && !local,
         "--local-shadows, --local-highlights, --local-sigma and --local-levels set the local tone operator: they require "
         "--display local"},
        {bloom && !display, "--bloom blooms the frame the display transform shows: it requires --display"},
        {grade && !display, "--grade-... grades the frame the display transform shows: it requires --display"},
        {!lut_file.empty() && !display, "--lut is a look on the display transform's frame: it requires --display"},
        {lut_interp_given && lut_file.empty(), "--lut-interp requires --lut FILE.cube"},
        {grade_tint_given && !grade_temperature_given, "--grade-tint shifts the white of a temperature: it requires --grade-temperature K"},
        {(firefly_rank_given || firefly_radius_given || firefly_floor_given || firefly_keep_given) && !firefly,
         "--firefly-rank, --firefly-radius, --firefly-floor and --firefly-keep-nonfinite require --firefly"},
        {firefly && many, "--firefly runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {firefly && preview_only, "--preview-only skips the full render: it does not combine with --firefly"},
        {(scopes_columns_given || scopes_layout_given) && !scopes, "--scopes-columns and --scopes-layout require --scopes"},
        {scopes && many, "--scopes runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {scopes && preview_only, "--preview-only skips the full render: it does not combine with --scopes"},
        {expose && many,
         "--expose-percentile runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {expose && preview_only, "--preview-only skips the full render: it does not combine with --expose-percentile"},
        {expose && !display, "--expose-percentile sets the display transform's exposure: it requires --display"},
        {expose && exposure_given, "--expose-percentile chooses the exposure: it does not combine with --exposure"},
        {expose && local,
         "--expose-percentile needs a global curve: it does not combine with --display local, which takes its own exposures"},
        {(focus_given || focus_pixel_given || dof_radius_given) && !dof, "--focus, --focus-pixel and --dof-radius require --dof"},
        {focus_given && focus_pixel_given, "--dof focuses at --focus DISTANCE or at --focus-pixel X,Y, not at both"},
        {dof && many, "--dof runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {dof && preview_only, "--preview-only skips the full render: it does not combine with --dof"},
        {(lens_inverse || lens_filter_given) && !lens,
         "--lens-inverse and --lens-filter require the lens stage: --lens, --lens-ca, --lens-vignette or --lens-zoom"},
        {lens && many, "--lens runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {lens && preview_only, "--preview-only skips the full render: it does not combine with --lens"},
        {lens && mattes,
         "--lens does not combine with --alpha, --matte or --background: the coverage planes are not warped with the frame"},
        {lens && lens_prm.filter == RTM_LENS_NEAREST && (lens_prm.chroma != 0.0f || lens_prm.vignette != 0.0f),
         "--lens-filter nearest copies words: it does not combine with --lens-ca or --lens-vignette"},
        {resize_filter_given && !resize, "--resize-filter requires --resize WxH"},
        {resize && many, "--resize runs on one GPU: it does not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {resize && preview_only, "--preview-only skips the full render: it does not combine with --resize"},
        {resize && (!compare_ref.empty() || !flip_ref.empty()),
         "--resize does not combine with --compare or --flip: their references are checked against the render's size"},
        {resize && mattes, "--resize does not combine with --alpha, --matte or --background: the composite runs at the render's size"},
        {(flip_map || flip_ppd_given) && flip_ref.empty(), "--flip-map and --flip-ppd require --flip REF.pfm"},
        {mattes && many,
         "--alpha, --matte and --background run on one GPU: they do not combine with --gpus > 1, --virtual-strips or --force-rccl"},
        {mattes && preview_only,
         "--preview-only skips the full render: it does not combine with --alpha, --matte or --background"},
        {matte_layers_given && matte_ids.empty(), "--matte-layers requires --matte ID[,ID...]"},
    };
    for (const auto& r : refusals)
        if (r.applies) {
            std::fprintf(stderr, "%s\n", r.text);
            return 2;
        }
    if (!file_exists(json_file)) {  // src/main.cpp:36-39
        std::printf("saving the sample scene json file: %s\n", json_file.c_str());
        if (rtm_scene_save_sample_json(json_file.c_str()) != RTM_OK) return 1;
    }
    std::printf("loading %s and starting the render\n", json_file.c_str());  // src/main.cpp:40

    rtm_settings st;
    size_t n = 0;
    const int literal = (mode == RTM_MODE_LITERAL);
    // the any-type object list: the shipped files hold spheres only; objectType 2 (png::PlaneObject) loads too
    int rc = rtm_scene_load_json_objects(json_file.c_str(), literal, &st, nullptr, 0, &n);
    if (rc != RTM_OK) {
        std::fprintf(stderr, "%s: %s (%s)\n", json_file.c_str(), rtm_strerror(rc), rtm_last_error_detail());
        return 1;
    }
    std::vector<rtm_object> spheres(n ? n : 1);
    rc = rtm_scene_load_json_objects(json_file.c_str(), literal, &st, spheres.data(), n, &n);
    if (rc != RTM_OK) {
        std::fprintf(stderr, "%s: %s (%s)\n", json_file.c_str(), rtm_strerror(rc), rtm_last_error_detail());
        return 1;
    }
    if (width > 0) st.width = width;
    if (height > 0) st.height = height;
    if (super_samples > 0) st.super_samples = super_samples;
    if (samples > 0) st.samples = samples;
    if (spp > 0) st.samples = spp / (st.super_samples * st.super_samples) > 0 ? spp / (st.super_samples * st.super_samples) : 1;

    rtm_options opt;
    std::memset(&opt, 0, sizeof opt);
    opt.mode = mode | (host_trig ? RTM_MODE_HOST_TRIG : 0);
    opt.max_bounces = max_bounces;
    opt.seed = seed;
    opt.row_begin = 0;
    opt.row_end = st.height;
    opt.device = device;

    if (mattes && st.super_samples > 8) {  // rtm_render_mattes' limit, known before anything is rendered
        std::fprintf(stderr, "--alpha, --matte and --background serve superSamples up to 8, got %d\n", st.super_samples);
        return 2;
    }
    if (preview && (st.width % preview != 0 || st.height % preview != 0)) {
        std::fprintf(stderr, "--preview %d does not divide the %d x %d frame\n", preview, st.width, st.height);
        return 2;
    }
    // --compare and --flip: read before anything is rendered, so that a bad file costs no render
    std::vector<float> reference, flip_reference;
    if (!compare_ref.empty() && !read_reference("--compare", compare_ref, st, reference)) return 1;
    if (!flip_ref.empty() && !read_reference("--flip", flip_ref, st, flip_reference)) return 1;
    // --lut: read before anything is rendered, like the references; --grade-temperature: the matrix (host only)
    if (!lut_file.empty()) {
        int32_t n3 = 0;
        rc = rtm_lut_load_cube(lut_file.c_str(), &n3, look.params.lut_min, look.params.lut_max, nullptr, 0);
        if (rc == RTM_OK) {
            look.table.resize((size_t)3 * n3 * n3 * n3);
            rc = rtm_lut_load_cube(lut_file.c_str(), &n3, look.params.lut_min, look.params.lut_max, look.table.data(), look.table.size());
        }
        if (rc != RTM_OK) {
            std::fprintf(stderr, "--lut: %s: %s (%s)\n", lut_file.c_str(), rtm_strerror(rc), rtm_last_error_detail());
            return 1;
        }
        look.params.lut_size = n3;
    }
    if (grade_temperature_given) {
        rc = rtm_grade_white_balance(grade_kelvin, grade_tint, grade_prm.matrix);
        if (rc != RTM_OK) {
            std::fprintf(stderr, "--grade-temperature: %s (%s)\n", rtm_strerror(rc), rtm_last_error_detail());
            return 2;
        }
    }
    // a later stage takes the float frame of the last one
    const bool want_last = scopes || display || pfm || !compare_ref.empty() || !flip_ref.empty() || background || dof || lens || resize;
    if (dof) {  // the focus, known before anything is rendered: --focus, what --focus-pixel shows, else the camera's target
        if (focus_pixel_given) {
            if (focus_x >= st.width || focus_y >= st.height) {
                std::fprintf(stderr, "--focus-pixel %d,%d is outside the %d x %d frame\n", focus_x, focus_y, st.width, st.height);
                return 2;
            }
            std::string ferr;
            rc = rtm_node_depth_at(&st, spheres.data(), n, &opt, focus_x, focus_y, &dof_prm.focus_distance, ferr);
            if (rc != RTM_OK) return fail("focus-pixel", rc, ferr);
            if (!(std::isfinite(dof_prm.focus_distance) && dof_prm.focus_distance > 0.0f)) {
                std::fprintf(stderr, "--focus-pixel %d,%d is a miss: its primary ray hits nothing\n", focus_x, focus_y);
                return 2;
            }
        } else if (!focus_given) {
            double d2 = 0.0;
            for (int k = 0; k < 3; ++k) d2 += (st.camera.target[k] - st.camera.origin[k]) * (st.camera.target[k] - st.camera.origin[k]);
            dof_prm.focus_distance = (float)std::sqrt(d2);
            if (!(std::isfinite(dof_prm.focus_distance) && dof_prm.focus_distance > 0.0f)) {
                std::fprintf(stderr, "--dof: the camera's target is its origin, there is no target distance: give --focus DISTANCE\n");
                return 2;
            }
        }
        std::printf("dof: focus %.6g, aperture %.6g, max radius %d\n", (double)dof_prm.focus_distance, (double)dof_prm.aperture,
                    dof_prm.max_radius);
    }
    if (lens && lens_zoom_auto) {  // the zoom that hides the border, known before anything is rendered (host only)
        rc = rtm_lens_fit_zoom(&lens_prm, st.width, st.height, &lens_prm.zoom);
        if (rc != RTM_OK) {
            std::fprintf(stderr, "--lens-zoom auto: %s (%s)\n", rtm_strerror(rc), rtm_last_error_detail());
            return 2;
        }
    }
    if (bloom)
        std::printf("bloom: threshold %.6g, knee %.6g, intensity %.6g, scatter %.6g, levels %d\n", (double)bloom_prm.threshold,
                    (double)bloom_prm.knee, (double)bloom_prm.intensity, (double)bloom_prm.scatter, bloom_prm.levels);
    if (local)
        std::printf("local: shadows %.6g, highlights %.6g, sigma %.6g, levels %d\n", (double)local_prm.shadows,
                    (double)local_prm.highlights, (double)local_prm.sigma, local_prm.levels);
    if (grade) {
        std::printf("grade:");
        if (grade_temperature_given) std::printf(" temperature %.9g, tint %.9g,", (double)grade_kelvin, (double)grade_tint);
        std::printf(" exposure %.9g, contrast %.9g at pivot %.9g, slope %.9g %.9g %.9g, offset %.9g %.9g %.9g, power %.9g %.9g %.9g, "
                    "saturation %.9g\n",
                    (double)grade_prm.exposure, (double)grade_prm.contrast, (double)grade_prm.pivot, (double)grade_prm.slope[0],
                    (double)grade_prm.slope[1], (double)grade_prm.slope[2], (double)grade_prm.offset[0], (double)grade_prm.offset[1],
                    (double)grade_prm.offset[2], (double)grade_prm.power[0], (double)grade_prm.power[1], (double)grade_prm.power[2],
                    (double)grade_prm.saturation);
    }
    if (!lut_file.empty())
        std::printf("lut: %s, size %d, %s, domain %.9g %.9g %.9g to %.9g %.9g %.9g\n", lut_file.c_str(), look.params.lut_size,
                    look.params.lut_interp == RTM_GRADE_TRILINEAR ? "trilinear" : "tetrahedral", (double)look.params.lut_min[0],
                    (double)look.params.lut_min[1], (double)look.params.lut_min[2], (double)look.params.lut_max[0],
                    (double)look.params.lut_max[1], (double)look.params.lut_max[2]);
    // --display of one frame: bloomed first with --bloom, graded with --grade-..., then STEM<suffix>_display.bmp / .jpg and their line, which gives
    // the statistics for the frame itself (no suffix); the exit status, 0 when all went well
    float chosen_ev = 0.0f;  // --expose-percentile's stops for the frame itself
    const auto show = [&](const rtm_settings& fs, const float* frame, const std::string& suffix, std::vector<float>* f32_out) {
        std::string err;
        std::vector<float> bloomed;
        if (bloom) {
            const int brc = rtm_node_bloom(&fs, opt.device, &bloom_prm, frame, &bloomed, err);
            if (brc != RTM_OK) return fail("bloom", brc, err);
            frame = bloomed.data();
        }
        std::vector<float> graded;
        if (grade) {
            const int grc = rtm_node_grade(&fs, opt.device, &grade_prm, frame, &graded, err);
            if (grc != RTM_OK) return fail("grade", grc, err);
            frame = graded.data();
        }
        rtm_tonemap_params shown_prm = display_prm;
        if (expose) {  // the exposure from the histogram of the frame the transform is about to take
            const rtm_scope_params sp = RTM_SCOPE_DEFAULTS;
            rtm_scope_histogram hist;
            int erc = rtm_node_scopes(&fs, opt.device, &sp, frame, &hist, RTM_SCOPE_LUMA, 1, nullptr, err);
            if (erc != RTM_OK) return fail("expose-percentile", erc, err);
            shown_prm.auto_exposure = 0;
            erc = rtm_scope_exposure(&hist, expose_percent, expose_target, &shown_prm.ev);
            if (erc != RTM_OK) return fail("expose-percentile", erc, rtm_last_error_detail());
            if (suffix.empty()) chosen_ev = shown_prm.ev;
            std::printf("expose-percentile: %s%s at %s percent to %s, exposure %s\n", stem.c_str(), suffix.c_str(),
                        json_number(expose_percent).c_str(), json_number(expose_target).c_str(),
                        json_number((double)shown_prm.ev).c_str());
        }
        rtm_tonemap_stats ts;
        const std::string name = stem + suffix;
        const int drc = rtm_node_write_display(&fs, opt.device, &shown_prm, frame, name, &ts, err, f32_out,
                                               lut_file.empty() ? nullptr : &look, local ? &local_prm : nullptr);
        if (drc != RTM_OK) return fail("display", drc, err);
        if (suffix.empty())
            std::printf("display: %s_display.bmp, %s_display.jpg (log-average %.6g, max luminance %.6g, exposure %.6g, %u pixels)\n",
                        name.c_str(), name.c_str(), (double)ts.log_average, (double)ts.max_luminance, (double)ts.exposure, ts.pixels);
        else
            std::printf("display: %s_display.bmp, %s_display.jpg\n", name.c_str(), name.c_str());
        return 0;
    };
    std::string err;  // a stage's account of its failure: main returns at the first one
    if (preview) {  // STEM_preview.bmp / .jpg, and their display transform
        std::vector<float> shown;
        rtm_stats ps;
        rc = rtm_node_write_preview(&st, spheres.data(), n, &opt, preview, stem, err, display ? &shown : nullptr, &ps);
        if (rc != RTM_OK) return fail("preview", rc, err);
        std::printf("preview: %s_preview.bmp, %s_preview.jpg (%d x %d traced, %llu samples, kernel %.3f ms)\n", stem.c_str(),
                    stem.c_str(), st.width / preview, st.height / preview, (unsigned long long)ps.samples, ps.kernel_ms);
        if (display && show(st, shown.data(), "_preview", nullptr) != 0) return 1;
        if (preview_only) {
            if (aov) {
                rc = rtm_node_write_aov(&st, spheres.data(), n, &opt, stem, err);
                if (rc != RTM_OK) return fail("aov", rc, err);
            }
            return 0;
        }
    }

    const size_t vals = (size_t)st.width * st.height * 3;
    std::vector<uint8_t> rgb8(vals);
    std::vector<float> rgb32(dump_f32.empty() && !firefly && !denoise && !denoise_variance && !want_last ? 0 : vals);
    float* const out32 = rgb32.empty() ? nullptr : rgb32.data();
    rtm_stats stats;
    std::vector<uint32_t> tile_samples;
    if (adaptive) {
        rtm_adaptive_params prm;
        prm.min_samples = adaptive_min > 0 ? (uint32_t)adaptive_min : 0u;
        prm.threshold = adaptive_threshold;
        rc = rtm_node_render_adaptive(&st, spheres.data(), n, &opt, &prm, out32, rgb8.data(), tile_samples, &stats, err);
    } else if (passes > 0) {
        rc = rtm_node_render_passes(&st, spheres.data(), n, &opt, passes, out32, rgb8.data(), &stats, err);
    } else if (many) {
        int have = 0;
        if (rtm_device_count(&have) != RTM_OK || have < gpus) {
            std::fprintf(stderr, "--gpus %d requested, %d HIP device(s) present\n", gpus, have);
            return 1;
        }
        rc = rtm_node_render(&st, spheres.data(), n, &opt, gpus, virtual_strips, force_rccl, out32, rgb8.data(), &stats, err);
    } else {
        rc = rtm_render_objects(&st, spheres.data(), n, &opt, nullptr, out32, rgb8.data(), &stats);
        if (rc != RTM_OK) err = rtm_last_error_detail();
    }
    if (rc != RTM_OK) return fail("render", rc, err);
    if (!dump_f32.empty()) {
        FILE* f = std::fopen(dump_f32.c_str(), "wb");
        if (!f || std::fwrite(rgb32.data(), sizeof(float), vals, f) != vals) {
            std::fprintf(stderr, "cannot write %s\n", dump_f32.c_str());
            return 1;
        }
        std::fclose(f);
    }
    std::printf("%d x %d, %llu samples, %.3f casts/sample, kernel %.3f ms, %.1f Msamples/s\n", st.width,
                st.height, (unsigned long long)stats.samples,
                stats.samples ? (double)stats.casts / (double)stats.samples : 0.0, stats.kernel_ms,
                stats.kernel_ms > 0 ? (double)stats.samples / stats.kernel_ms * 1e-3 : 0.0);
    // src/Renderer.cpp:256-257
    const int ok_jpg = rtm_write_jpg((stem + ".jpg").c_str(), st.width, st.height, 3, rgb8.data(), 60);
    const int ok_bmp = rtm_write_bmp((stem + ".bmp").c_str(), st.width, st.height, 3, rgb8.data());
    if (!(ok_jpg && ok_bmp)) return 1;
    if (adaptive) {  // <stem>_spp.pfm: every pixel's sample count
        const int tiles_x = (st.width + 7) / 8;
        std::vector<float> spp((size_t)st.width * st.height);
        for (int y = 0; y < st.height; ++y)
            for (int x = 0; x < st.width; ++x) spp[(size_t)y * st.width + x] = (float)tile_samples[(size_t)(y / 8) * tiles_x + x / 8];
        if (rtm_write_pfm((stem + "_spp.pfm").c_str(), st.width, st.height, 1, spp.data()) != 1) return 1;
    }
    if (aov) {
        rc = rtm_node_write_aov(&st, spheres.data(), n, &opt, stem, err);
        if (rc != RTM_OK) return fail("aov", rc, err);
        std::printf("aov: %s_depth.pfm, %s_normal.pfm, %s_albedo.pfm, %s_normal.bmp, %s_albedo.bmp\n", stem.c_str(), stem.c_str(),
                    stem.c_str(), stem.c_str(), stem.c_str());
    }
    std::vector<float> cleaned;  // --firefly's frame: what every stage below takes for the render's
    if (firefly) {
        size_t clamped = 0, repaired = 0;
        rc = rtm_node_write_firefly(&st, opt.device, &firefly_prm, rgb32.data(), stem, err, &cleaned, &clamped, &repaired);
        if (rc != RTM_OK) return fail("firefly", rc, err);
        std::printf("firefly: {\"clamped\": %llu, \"repaired\": %llu, \"pixels\": %llu}\n", (unsigned long long)clamped,
                    (unsigned long long)repaired, (unsigned long long)st.width * (unsigned long long)st.height);
    }
    const float* const frame32 = firefly ? cleaned.data() : rgb32.data();
    std::vector<float> shown;  // the float frame of the last stage, when --display, --pfm or --compare follows a denoiser
    if (denoise) {
        rc = rtm_node_write_denoised(&st, spheres.data(), n, &opt, frame32, stem, err,
                                     want_last && !denoise_variance ? &shown : nullptr);
        if (rc != RTM_OK) return fail("denoise", rc, err);
        std::printf("denoise: %s_denoised.bmp, %s_denoised.jpg\n", stem.c_str(), stem.c_str());
    }
    if (denoise_variance) {
        rc = rtm_node_write_denoised_variance(&st, spheres.data(), n, &opt, frame32, stem, err, want_last ? &shown : nullptr);
        if (rc != RTM_OK) return fail("denoise-variance", rc, err);
        std::printf("denoise-variance: %s_denoised_var.bmp, %s_denoised_var.jpg, %s_variance.pfm\n", stem.c_str(), stem.c_str(),
                    stem.c_str());
    }
    if (dof) {  // of the last stage so far; its frame then is the last stage's
        std::vector<float> defocused;
        rc = rtm_node_write_dof(&st, spheres.data(), n, &opt, &dof_prm, shown.empty() ? frame32 : shown.data(), stem, err, &defocused);
        if (rc != RTM_OK) return fail("dof", rc, err);
        shown.swap(defocused);
    }
    if (lens) {  // of the last stage so far, in linear light; its frame then is the last stage's
        std::vector<float> through;
        rc = rtm_node_write_lens(&st, opt.device, &lens_prm, shown.empty() ? frame32 : shown.data(), stem, err, &through);
        if (rc != RTM_OK) return fail("lens", rc, err);
        shown.swap(through);
        std::printf("lens: %s_lens.bmp, %s_lens.jpg (zoom %.9g)\n", stem.c_str(), stem.c_str(), (double)lens_prm.zoom);
    }
    rtm_settings last_st = st;  // the last stage's size: the render's, unless --resize follows
    if (resize) {  // of the last stage so far, in linear light; its frame then is the last stage's
        std::vector<float> resized;
        rc = rtm_node_write_resized(&st, opt.device, &resize_prm, resize_w, resize_h, shown.empty() ? frame32 : shown.data(), stem,
                                    err, &resized);
        if (rc != RTM_OK) return fail("resize", rc, err);
        shown.swap(resized);
        last_st.width = resize_w;
        last_st.height = resize_h;
        std::printf("resize: %s_resized.bmp, %s_resized.jpg (%d x %d)\n", stem.c_str(), stem.c_str(), resize_w, resize_h);
    }
    const float* last = shown.empty() ? frame32 : shown.data();
    std::vector<float> displayed;  // the display transform's float frame, when --display-pfm or --flip follows --display
    if (display && show(last_st, last, "", display_pfm || scopes || !flip_ref.empty() ? &displayed : nullptr) != 0) return 1;
    if (display_pfm) {
        if (rtm_write_pfm((stem + "_display.pfm").c_str(), last_st.width, last_st.height, 3, displayed.data()) != 1) {
            std::fprintf(stderr, "cannot write %s_display.pfm\n", stem.c_str());
            return 1;
        }
        std::printf("display-pfm: %s_display.pfm\n", stem.c_str());
    }
    if (pfm) {
        if (rtm_write_pfm((stem + ".pfm").c_str(), last_st.width, last_st.height, 3, last) != 1) {
            std::fprintf(stderr, "cannot write %s.pfm\n", stem.c_str());
            return 1;
        }
        std::printf("pfm: %s.pfm\n", stem.c_str());
    }
    if (scopes) {  // the last linear frame in stops, the display frame in code values, the waveform of the one that is shown
        rtm_scope_params sp = RTM_SCOPE_DEFAULTS;
        sp.columns = scopes_columns_given ? scopes_columns : std::min(sp.columns, last_st.width);
        if (sp.columns > last_st.width) {
            std::fprintf(stderr, "--scopes-columns %d exceeds the frame's width %d\n", sp.columns, last_st.width);
            return 2;
        }
        const uint32_t gain = (uint32_t)std::max(1, 2040 / last_st.height);
        // one frame's object: the line's fields, and with `full` the counts
        const auto describe = [](const rtm_scope_histogram& h, int mode, bool full) {
            std::string s = std::string("{\"mode\": \"") + (mode == RTM_SCOPE_LOG2 ? "log2" : "code") + "\", \"pixels\": " +
                            std::to_string(h.pixels) + ", \"not_counting\": " + std::to_string(h.not_counting) + ", \"percentiles\": {";
            const double percents[4] = {1.0, 50.0, 99.0, 99.9};
            const char* const keys[4] = {"1", "50", "99", "99.9"};
            for (int k = 0; k < 4; ++k) {
                float v = 0.0f;
                (void)rtm_scope_percentile(&h, mode, 0, percents[k], &v, nullptr);
                s += std::string(k ? ", \"" : "\"") + keys[k] + "\": " + json_number((double)v);
            }
            s += "}";
            const auto list = [&](const char* name, const uint32_t* v, int count, bool share) {
                s += std::string(", \"") + name + "\": [";
                for (int k = 0; k < count; ++k)
                    s += std::string(k ? ", " : "") +
                         (share ? json_number(h.pixels ? (double)v[k] / (double)h.pixels : 0.0) : std::to_string(v[k]));
                s += "]";
            };
            list("below", h.below, 4, true);
            list("above", h.above, 4, true);
            if (full) {
                s += ", \"histogram\": {\"bins\": [";
                for (int c = 0; c < 4; ++c) {
                    s += c ? ", [" : "[";
                    for (int b = 0; b < 256; ++b) s += std::string(b ? ", " : "") + std::to_string(h.bins[c][b]);
                    s += "]";
                }
                s += "]";
                list("below", h.below, 4, false);
                list("above", h.above, 4, false);
                s += "}";
            }
            return s + "}";
        };
        rtm_scope_histogram lin, disp;
        std::vector<uint8_t> picture;
        rc = rtm_node_scopes(&last_st, opt.device, &sp, last, &lin, scopes_layout, gain, display ? nullptr : &picture, err);
        if (rc != RTM_OK) return fail("scopes", rc, err);
        if (display) {
            sp.mode = RTM_SCOPE_CODE;
            rc = rtm_node_scopes(&last_st, opt.device, &sp, displayed.data(), &disp, scopes_layout, gain, &picture, err);
            if (rc != RTM_OK) return fail("scopes", rc, err);
        }
        std::string line, doc;
        for (int full = 0; full < 2; ++full) {
            std::string s = describe(lin, RTM_SCOPE_LOG2, full != 0);
            s.pop_back();  // the frame's object stays open for what belongs to the run
            if (display) s += ", \"display\": " + describe(disp, RTM_SCOPE_CODE, full != 0);
            if (expose) s += ", \"exposure\": " + json_number((double)chosen_ev);
            s += "}";
            (full ? doc : line) = s;
        }
        std::printf("scopes: %s\n", line.c_str());
        FILE* f = std::fopen((stem + "_scopes.json").c_str(), "wb");
        const bool wrote = f && std::fwrite(doc.data(), 1, doc.size(), f) == doc.size();
        if (f) std::fclose(f);
        const int picture_w = sp.columns * (scopes_layout == RTM_SCOPE_PARADE ? 3 : 1);
        if (!wrote || rtm_write_bmp((stem + "_waveform.bmp").c_str(), picture_w, 256, 3, picture.data()) != 1) {
            std::fprintf(stderr, "cannot write %s_scopes.json or %s_waveform.bmp\n", stem.c_str(), stem.c_str());
            return 1;
        }
        std::printf("waveform: %s_waveform.bmp (%d x 256, gain %u), %s_scopes.json\n", stem.c_str(), picture_w, gain, stem.c_str());
    }
    if (!compare_ref.empty()) {
        rtm_compare_result cr;
        rc = rtm_node_compare(&st, opt.device, last, reference.data(), &cr, err);
        if (rc != RTM_OK) return fail("compare", rc, err);
        std::printf("compare: {\"max_abs\": %s, \"mse\": %s, \"psnr\": %s, \"rel_mse\": %s, \"ssim\": %s, \"pixels\": %llu, "
                    "\"outside\": %llu, \"nonfinite\": %llu, \"nonfinite_mismatch\": %llu, \"argmax_x\": %d, \"argmax_y\": %d}\n",
                    json_number(cr.max_abs).c_str(), json_number(cr.mse).c_str(), json_number(cr.psnr).c_str(),
                    json_number(cr.rel_mse).c_str(), json_number(cr.ssim).c_str(), (unsigned long long)cr.pixels,
                    (unsigned long long)cr.outside, (unsigned long long)cr.nonfinite, (unsigned long long)cr.nonfinite_mismatch,
                    cr.argmax_x, cr.argmax_y);
    }
    if (mattes) {
        std::vector<float> over;
        rc = rtm_node_write_mattes(&st, spheres.data(), n, &opt, alpha != 0, matte_layers, matte_ids, background ? &composite_prm : nullptr,
                                   background ? last : nullptr, stem, err, background && display ? &over : nullptr);
        if (rc != RTM_OK) return fail("mattes", rc, err);
        if (alpha) std::printf("alpha: %s_alpha.pfm\n", stem.c_str());
        if (!matte_ids.empty())
            std::printf("matte: %s_matte.pfm, %s_matte.bmp (%d ids, %d layers)\n", stem.c_str(), stem.c_str(), (int)matte_ids.size(), matte_layers);
        if (background) std::printf("background: %s_over.bmp, %s_over.jpg\n", stem.c_str(), stem.c_str());
        if (background && display && show(st, over.data(), "_over", nullptr) != 0) return 1;
    }
    if (!flip_ref.empty()) {
        rtm_flip_result fr;
        std::vector<float> fmap;
        if (display)
            flip_prm.transfer = display_prm.transfer;  // the display frame's own encoding
        else
            flip_prm.transfer = RTM_TRANSFER_LINEAR;  // the last stage's frame, taken as linear
        rc = rtm_node_flip(&st, opt.device, &flip_prm, display ? displayed.data() : last, flip_reference.data(), &fr,
                           flip_map ? &fmap : nullptr, err);
        if (rc != RTM_OK) return fail("flip", rc, err);
        // the weighted median as the published tool pools it: bin i weighs its count times its centre (i + 0.5) / 256; the
        // centre of the first bin at which the running weight reaches half of the total (bin resolution, 1/256)
        double run[256], total = 0.0, median = 0.0;
        for (int i = 0; i < 256; ++i) run[i] = total += (double)fr.hist[i] * (((double)i + 0.5) / 256.0);
        if (total > 0.0)
            for (int i = 0; i < 256; ++i)
                if (run[i] >= 0.5 * total) {
                    median = ((double)i + 0.5) / 256.0;
                    break;
                }
        std::printf("flip: {\"mean\": %s, \"max\": %s, \"min\": %s, \"pixels\": %llu, \"nonfinite\": %llu, \"argmax_x\": %d, "
                    "\"argmax_y\": %d, \"weighted_median\": %s}\n",
                    json_number(fr.mean).c_str(), json_number(fr.max).c_str(), json_number(fr.min).c_str(),
                    (unsigned long long)fr.pixels, (unsigned long long)fr.nonfinite, fr.argmax_x, fr.argmax_y,
                    json_number(median).c_str());
        if (flip_map) {
            if (rtm_write_pfm((stem + "_flip.pfm").c_str(), st.width, st.height, 1, fmap.data()) != 1) {
                std::fprintf(stderr, "cannot write %s_flip.pfm\n", stem.c_str());
                return 1;
            }
            std::printf("flip-map: %s_flip.pfm\n", stem.c_str());
        }
    }
    return 0;
}
