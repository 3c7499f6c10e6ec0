"""ctypes binding of the C ABI in include/rtm.h (librtm_hip.so, built by csrc/Makefile).

The HIP library is the product path: importing fails loudly when it has not been built, and
nothing here falls back to a CPU implementation.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTM_LIB_OVERRIDE") or os.path.join(_HERE, "librtm_hip.so")  # override: A/B of builds

RTM_OK = 0
MODE_LITERAL, MODE_REPAIRED = 0, 1
MODE_HOST_TRIG = 0x100  # flag: sin/cos exactly as the host libm returns them (include/rtm.h)
MODE_COUNT_TESTS = 0x200  # flag: count Intersect evaluations into rtm_stats.object_tests (diagnostic)
MODE_SURFACE_SAMPLE = 0x400  # flag: the integrator is png::SurfaeSample instead of png::PathTracing
MODES = {"literal": MODE_LITERAL, "repaired": MODE_REPAIRED, 0: 0, 1: 1}


class RtmError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: {detail}" if detail else what)


class rtm_camera(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("target", C.c_double * 3), ("up", C.c_double * 3),
                ("fov", C.c_float), ("_pad", C.c_float)]


class rtm_sphere(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("color", C.c_double * 3),
                ("emission", C.c_double * 3), ("radius", C.c_float), ("_pad", C.c_float)]


class rtm_object(C.Structure):
    _fields_ = [("type", C.c_int32), ("size", C.c_float), ("position", C.c_double * 3),
                ("color", C.c_double * 3), ("emission", C.c_double * 3), ("up", C.c_double * 3),
                ("target", C.c_double * 3), ("width", C.c_double)]


OBJECT_SPHERE, OBJECT_PLANE = 1, 2


class rtm_settings(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32),
                ("super_samples", C.c_int32), ("camera", rtm_camera)]


class rtm_options(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_bounces", C.c_int32), ("seed", C.c_uint64),
                ("row_begin", C.c_int32), ("row_end", C.c_int32), ("device", C.c_int32),
                ("variant", C.c_int32), ("band_count", C.c_int32), ("band_index", C.c_int32)]


class rtm_stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("casts", C.c_uint64), ("bounces", C.c_uint64),
                ("draws", C.c_uint64), ("kernel_ms", C.c_double), ("variant", C.c_int32),
                ("split", C.c_int32), ("object_tests", C.c_uint64)]

    def as_dict(self):
        return {"samples": int(self.samples), "casts": int(self.casts),
                "bounces": int(self.bounces), "draws": int(self.draws),
                "kernel_ms": float(self.kernel_ms), "variant": int(self.variant),
                "split": int(self.split), "object_tests": int(self.object_tests)}


class rtm_aov_buffers(C.Structure):  # DEVICE pointers, any may be null (include/rtm.h: rtm_render_aov)
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("object", C.c_void_p)]


class rtm_hit_buffers(C.Structure):  # DEVICE pointers, any may be null but not all (include/rtm.h: rtm_scene_nearest)
    _fields_ = [("object", C.c_void_p), ("t", C.c_void_p), ("normal", C.c_void_p)]


RADIANCE_CLAMP = 1  # RTM_RADIANCE_CLAMP


class rtm_radiance_params(C.Structure):  # include/rtm.h: rtm_scene_radiance; 32 bytes
    _fields_ = [("mode", C.c_int32), ("max_bounces", C.c_int32), ("seed", C.c_uint64), ("samples", C.c_uint32),
                ("key_base", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class rtm_radiance_buffers(C.Structure):  # DEVICE pointers, any may be null but not all (include/rtm.h: rtm_scene_radiance)
    _fields_ = [("radiance", C.c_void_p), ("casts", C.c_void_p), ("draws", C.c_void_p)]


class rtm_matte_buffers(C.Structure):  # DEVICE pointers, any may be null but not all (include/rtm.h: rtm_render_mattes)
    _fields_ = [("id", C.c_void_p), ("coverage", C.c_void_p), ("alpha", C.c_void_p)]


class rtm_composite_params(C.Structure):  # include/rtm.h: rtm_composite
    _fields_ = [("background", C.c_float * 3)]


class rtm_adaptive_params(C.Structure):  # include/rtm.h: rtm_render_adaptive
    _fields_ = [("min_samples", C.c_uint32), ("threshold", C.c_float)]


class rtm_denoise_params(C.Structure):  # include/rtm.h: rtm_denoise
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class rtm_denoise_var_params(C.Structure):  # include/rtm.h: rtm_denoise_variance
    _fields_ = [("iterations", C.c_int32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class rtm_upsample_params(C.Structure):  # include/rtm.h: rtm_upsample
    _fields_ = [("factor", C.c_int32), ("sigma_spatial", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


TONEMAP_OPS = {"clamp": 0, "reinhard": 1, "aces": 2}  # include/rtm.h: RTM_TONEMAP_*
TRANSFERS = {"linear": 0, "srgb": 1}  # RTM_TRANSFER_*


class rtm_tonemap_params(C.Structure):  # include/rtm.h: rtm_tonemap
    _fields_ = [("op", C.c_int32), ("transfer", C.c_int32), ("auto_exposure", C.c_int32), ("dither", C.c_int32),
                ("ev", C.c_float), ("key", C.c_float), ("white", C.c_float)]


class rtm_tonemap_stats(C.Structure):  # what rtm_tonemap leaves in stats_out_dev
    _fields_ = [("log_average", C.c_float), ("max_luminance", C.c_float), ("exposure", C.c_float), ("pixels", C.c_uint32)]


class rtm_bloom_params(C.Structure):  # include/rtm.h: rtm_bloom (20 bytes)
    _fields_ = [("threshold", C.c_float), ("knee", C.c_float), ("intensity", C.c_float), ("scatter", C.c_float),
                ("levels", C.c_int32)]


class rtm_tonemap_local_params(C.Structure):  # include/rtm.h: rtm_tonemap_local (20 bytes)
    _fields_ = [("anchor", C.c_float), ("shadows", C.c_float), ("highlights", C.c_float), ("sigma", C.c_float),
                ("levels", C.c_int32)]


class rtm_firefly_params(C.Structure):  # include/rtm.h: rtm_firefly (20 bytes)
    _fields_ = [("radius", C.c_int32), ("rank", C.c_int32), ("k", C.c_float), ("floor", C.c_float), ("repair", C.c_int32)]


FIREFLY_DEFAULTS = {"radius": 1, "rank": 3, "k": 4.0, "floor": 0.01, "repair": True}  # RTM_FIREFLY_DEFAULTS


class rtm_defocus_params(C.Structure):  # include/rtm.h: rtm_defocus (12 bytes)
    _fields_ = [("focus_distance", C.c_float), ("aperture", C.c_float), ("max_radius", C.c_int32)]


DEFOCUS_DEFAULTS = {"aperture": 4.0, "max_radius": 8}  # RTM_DEFOCUS_DEFAULTS; the caller sets focus_distance


class rtm_grade_params(C.Structure):  # include/rtm.h: rtm_grade (120 bytes)
    _fields_ = [("matrix", C.c_float * 9), ("exposure", C.c_float), ("contrast", C.c_float), ("pivot", C.c_float),
                ("slope", C.c_float * 3), ("offset", C.c_float * 3), ("power", C.c_float * 3), ("saturation", C.c_float),
                ("lut_size", C.c_int32), ("lut_interp", C.c_int32), ("lut_min", C.c_float * 3), ("lut_max", C.c_float * 3)]


GRADE_INTERPS = ("trilinear", "tetrahedral")  # RTM_GRADE_TRILINEAR, RTM_GRADE_TETRAHEDRAL
# RTM_GRADE_DEFAULTS; matrix None is the identity
GRADE_DEFAULTS = {"matrix": None, "exposure": 0.0, "contrast": 1.0, "pivot": 0.18, "slope": 1.0, "offset": 0.0, "power": 1.0,
                  "saturation": 1.0}


class rtm_lens_params(C.Structure):  # include/rtm.h: rtm_lens (48 bytes)
    _fields_ = [("k1", C.c_float), ("k2", C.c_float), ("zoom", C.c_float), ("chroma", C.c_float), ("vignette", C.c_float),
                ("falloff", C.c_float), ("border", C.c_float * 3), ("mode", C.c_int32), ("filter", C.c_int32),
                ("channels", C.c_int32)]


LENS_FILTERS = ("nearest", "bilinear", "bicubic")  # RTM_LENS_NEAREST .. RTM_LENS_BICUBIC, in the enum's order
LENS_MODES = ("direct", "inverse")  # RTM_LENS_DIRECT, RTM_LENS_INVERSE
# RTM_LENS_DEFAULTS; channels follows the tensor
LENS_DEFAULTS = {"k1": 0.0, "k2": 0.0, "zoom": 1.0, "chroma": 0.0, "vignette": 0.0, "falloff": 1.0, "border": 0.0,
                 "mode": "direct", "filter": "bicubic"}


class rtm_resize_params(C.Structure):  # include/rtm.h: rtm_resize (8 bytes)
    _fields_ = [("filter", C.c_int32), ("channels", C.c_int32)]


RESIZE_FILTERS = ("box", "triangle", "mitchell", "lanczos3")  # RTM_RESIZE_BOX .. RTM_RESIZE_LANCZOS3, in the enum's order
RESIZE_DEFAULTS = {"filter": "mitchell"}  # RTM_RESIZE_DEFAULTS; channels follows the tensor

COMPARE_DTYPES = {"float32": 0, "float64": 1}  # include/rtm.h: RTM_COMPARE_F32, RTM_COMPARE_F64
COMPARE_MAPS = {"abs": 0, "ssim": 1}  # RTM_COMPARE_MAP_*


class rtm_compare_params(C.Structure):  # include/rtm.h: rtm_compare
    _fields_ = [("dtype", C.c_int32), ("map", C.c_int32), ("tolerance", C.c_double), ("peak", C.c_double),
                ("rel_epsilon", C.c_double)]


class rtm_compare_result(C.Structure):  # what rtm_compare leaves in result_out_dev: 80 bytes, no padding
    _fields_ = [("max_abs", C.c_double), ("mse", C.c_double), ("psnr", C.c_double), ("rel_mse", C.c_double),
                ("ssim", C.c_double), ("pixels", C.c_uint64), ("outside", C.c_uint64), ("nonfinite", C.c_uint64),
                ("nonfinite_mismatch", C.c_uint64), ("argmax_x", C.c_int32), ("argmax_y", C.c_int32)]


class rtm_flip_params(C.Structure):  # include/rtm.h: rtm_flip (16 bytes: four bytes of padding after transfer)
    _fields_ = [("transfer", C.c_int32), ("pixels_per_degree", C.c_double)]


class rtm_flip_result(C.Structure):  # what rtm_flip leaves in result_out_dev: 1072 bytes, no padding
    _fields_ = [("mean", C.c_double), ("max", C.c_double), ("min", C.c_double), ("pixels", C.c_uint64),
                ("nonfinite", C.c_uint64), ("argmax_x", C.c_int32), ("argmax_y", C.c_int32), ("hist", C.c_uint32 * 256)]


SCOPE_MODES = {"log2": 0, "code": 1}  # include/rtm.h: RTM_SCOPE_LOG2, RTM_SCOPE_CODE
SCOPE_LAYOUTS = {"luma": 0, "overlay": 1, "parade": 2}  # RTM_SCOPE_LUMA, RTM_SCOPE_OVERLAY, RTM_SCOPE_PARADE
SCOPE_CHANNELS = ("y", "r", "g", "b")  # the histogram's and the waveform's channel order


class rtm_scope_params(C.Structure):  # include/rtm.h: rtm_scopes (8 bytes)
    _fields_ = [("mode", C.c_int32), ("columns", C.c_int32)]


class rtm_scope_histogram(C.Structure):  # what rtm_scopes leaves in hist_out_dev: 4144 bytes, no padding
    _fields_ = [("bins", (C.c_uint32 * 256) * 4), ("below", C.c_uint32 * 4), ("above", C.c_uint32 * 4), ("pixels", C.c_uint32),
                ("not_counting", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SCOPE_DEFAULTS = {"mode": "log2", "columns": 256}  # RTM_SCOPE_DEFAULTS


# every symbol include/rtm.h declares: name -> (restype, argtypes)
_P = C.POINTER
SIGNATURES = {
    "rtm_abi_version": (C.c_int, []),
    "rtm_strerror": (C.c_char_p, [C.c_int]),
    "rtm_last_error_detail": (C.c_char_p, []),
    "rtm_device_count": (C.c_int, [_P(C.c_int)]),
    "rtm_output_rows": (C.c_int, [_P(rtm_options)]),
    "rtm_release_scratch": (C.c_int, [C.c_int]),
    "rtm_stream_release": (C.c_int, [C.c_int, C.c_void_p]),
    "rtm_scratch_bytes": (C.c_int, [_P(rtm_settings), C.c_void_p, _P(rtm_options), _P(C.c_uint64)]),
    "rtm_num_variants": (C.c_int, []),
    "rtm_variant_name": (C.c_char_p, [C.c_int]),
    "rtm_scene_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, _P(C.c_void_p)]),
    "rtm_scene_create_device": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, _P(C.c_void_p)]),
    "rtm_scene_create_objects": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, _P(C.c_void_p)]),
    "rtm_scene_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _P(rtm_hit_buffers), C.c_void_p]),
    "rtm_scene_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rtm_scene_radiance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _P(rtm_radiance_params),
                                     _P(rtm_radiance_buffers), C.c_void_p]),
    "rtm_scene_destroy": (C.c_int, [C.c_void_p]),
    "rtm_scene_size": (C.c_size_t, [C.c_void_p]),
    "rtm_stream_status": (C.c_int, [C.c_int, C.c_void_p]),
    "rtm_render_scene": (C.c_int, [_P(rtm_settings), C.c_void_p, _P(rtm_options), C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, _P(rtm_stats)]),
    "rtm_render_scene_samples": (C.c_int, [_P(rtm_settings), C.c_void_p, _P(rtm_options), C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(rtm_stats)]),
    "rtm_render_scene_tiles": (C.c_int, [_P(rtm_settings), C.c_void_p, _P(rtm_options), C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         _P(rtm_stats)]),
    "rtm_adaptive_work_bytes": (C.c_size_t, [_P(rtm_settings), _P(rtm_options)]),
    "rtm_render_adaptive": (C.c_int, [_P(rtm_settings), C.c_void_p, _P(rtm_options), _P(rtm_adaptive_params), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(rtm_stats)]),
    "rtm_render_aov": (C.c_int, [_P(rtm_settings), C.c_void_p, _P(rtm_options), _P(rtm_aov_buffers), C.c_void_p]),
    "rtm_render_mattes": (C.c_int, [_P(rtm_settings), C.c_void_p, _P(rtm_options), C.c_int32, _P(rtm_matte_buffers), C.c_void_p]),
    "rtm_matte": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                            C.c_void_p]),
    "rtm_composite": (C.c_int, [_P(rtm_composite_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_denoise_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rtm_denoise": (C.c_int, [_P(rtm_denoise_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, _P(rtm_aov_buffers),
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_denoise_variance_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rtm_denoise_variance": (C.c_int, [_P(rtm_denoise_var_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, _P(rtm_aov_buffers),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_tonemap_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rtm_tonemap": (C.c_int, [_P(rtm_tonemap_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_bloom_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rtm_bloom": (C.c_int, [_P(rtm_bloom_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_tonemap_local_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "rtm_tonemap_local": (C.c_int, [_P(rtm_tonemap_local_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_firefly": (C.c_int, [_P(rtm_firefly_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_defocus": (C.c_int, [_P(rtm_defocus_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_grade": (C.c_int, [_P(rtm_grade_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p]),
    "rtm_grade_white_balance": (C.c_int, [C.c_float, C.c_float, _P(C.c_float)]),
    "rtm_lut_parse_cube": (C.c_int, [C.c_char_p, C.c_size_t, _P(C.c_int32), _P(C.c_float), _P(C.c_float), C.c_void_p, C.c_size_t]),
    "rtm_lut_load_cube": (C.c_int, [C.c_char_p, _P(C.c_int32), _P(C.c_float), _P(C.c_float), C.c_void_p, C.c_size_t]),
    "rtm_lens": (C.c_int, [_P(rtm_lens_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_lens_fit_zoom": (C.c_int, [_P(rtm_lens_params), C.c_int32, C.c_int32, _P(C.c_float)]),
    "rtm_resize_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rtm_resize": (C.c_int, [_P(rtm_resize_params), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_upsample_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rtm_upsample": (C.c_int, [_P(rtm_upsample_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, _P(rtm_aov_buffers),
                               _P(rtm_aov_buffers), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_compare_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rtm_compare": (C.c_int, [_P(rtm_compare_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_flip_work_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "rtm_flip": (C.c_int, [_P(rtm_flip_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_scopes": (C.c_int, [_P(rtm_scope_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_scope_draw": (C.c_int, [C.c_int32, C.c_int32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_scope_bin_range": (C.c_int, [C.c_int32, C.c_int32, _P(C.c_float), _P(C.c_float)]),
    "rtm_scope_percentile": (C.c_int, [_P(rtm_scope_histogram), C.c_int32, C.c_int32, C.c_double, _P(C.c_float), _P(C.c_int32)]),
    "rtm_scope_exposure": (C.c_int, [_P(rtm_scope_histogram), C.c_double, C.c_double, _P(C.c_float)]),
    "rtm_render_device": (C.c_int, [_P(rtm_settings), C.c_void_p, C.c_size_t, C.c_int,
                                    _P(rtm_options), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, _P(rtm_stats)]),
    "rtm_render": (C.c_int, [_P(rtm_settings), C.c_void_p, C.c_size_t, _P(rtm_options),
                             C.c_void_p, C.c_void_p, C.c_void_p, _P(rtm_stats)]),
    "rtm_render_objects": (C.c_int, [_P(rtm_settings), C.c_void_p, C.c_size_t, _P(rtm_options),
                                     C.c_void_p, C.c_void_p, C.c_void_p, _P(rtm_stats)]),
    "rtm_path_trace_batch": (C.c_int, [C.c_void_p, C.c_size_t, _P(rtm_options), C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_surface_sample_batch": (C.c_int, [C.c_void_p, C.c_size_t, _P(rtm_options), C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_intersect_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_intersect_objects_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_rng_u01": (C.c_double, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rtm_rng_batch": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_void_p]),
    "rtm_scene_load_json": (C.c_int, [C.c_char_p, C.c_int, _P(rtm_settings), C.c_void_p,
                                      C.c_size_t, _P(C.c_size_t)]),
    "rtm_scene_parse_json": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, _P(rtm_settings),
                                       C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "rtm_scene_load_json_objects": (C.c_int, [C.c_char_p, C.c_int, _P(rtm_settings), C.c_void_p,
                                              C.c_size_t, _P(C.c_size_t)]),
    "rtm_scene_parse_json_objects": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, _P(rtm_settings),
                                               C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "rtm_scene_save_sample_json": (C.c_int, [C.c_char_p]),
    "rtm_scene_make_stress": (C.c_int, [C.c_uint64, C.c_size_t, _P(rtm_settings), C.c_void_p]),
    "rtm_quantise": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "rtm_write_bmp": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rtm_write_jpg": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rtm_write_pfm": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rtm_read_pfm": (C.c_int, [C.c_char_p, _P(C.c_int), _P(C.c_int), _P(C.c_int), C.c_void_p, C.c_size_t]),
}
# test and diagnostic hooks: include/rtm_debug.h (not part of the drop-in boundary)
DEBUG_SIGNATURES = {
    "rtm_debug_math_probe": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rtm_debug_selfcheck": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "rtm_debug_trig_table": (C.c_int, [C.c_int, C.c_void_p]),
    "rtm_debug_fp64_peak": (C.c_int, [C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rtm_debug_wf_nearest": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_void_p]),
    "rtm_debug_grid_nearest": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_debug_scene_facts": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "rtm_debug_zero_term_facts": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "rtm_debug_axis_rows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "rtm_debug_wall_pairs": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "rtm_debug_tol_lds_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rtm_debug_grid_build": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.c_size_t]),
    "rtm_debug_scene_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    "rtm_debug_scene_query": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_debug_denoise_variance_kernel": (C.c_int, [C.c_int, _P(rtm_denoise_var_params), C.c_int32, C.c_int32, C.c_int,
                                                    _P(rtm_aov_buffers), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_debug_defocus_form": (C.c_int, [C.c_int, _P(rtm_defocus_params), C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtm_debug_matte_rank": (C.c_int, [C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "rtm_debug_component_bench": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_double)]),
}
ABI_VERSION = 5

_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64 (same SONAME as
    /opt/rocm's); two copies in one process leave the second without a device.  Importing torch
    BEFORE librtm_hip.so is loaded makes the dynamic loader resolve our libamdhip64.so.7
    dependency to the copy torch already mapped, so tensors, streams and RCCL buffers torch owns
    are valid in our kernels.  Without torch (rtm_cli, plain C callers) /opt/rocm's is used."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib():
    """The loaded HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` or `make -C raytracingmin_amd/csrc`. There is no CPU fallback.")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **DEBUG_SIGNATURES}.items():
            fn = getattr(L, name)  # AttributeError if the ABI lost a symbol
            fn.restype, fn.argtypes = res, args
        if L.rtm_abi_version() != ABI_VERSION:
            raise ImportError("librtm_hip.so has an unexpected ABI version")
        _lib = L
    return _lib


def check(status, what):
    if status != RTM_OK:
        L = lib()
        raise RtmError(status, f"{what}: {L.rtm_strerror(status).decode()}",
                       (L.rtm_last_error_detail() or b"").decode())
    return status
