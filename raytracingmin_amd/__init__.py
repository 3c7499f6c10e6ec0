"""raytracingmin_amd — MI355X-native hot path for RaytracingMin scenes.

Host-side mirror of the reference interface (png::LoadData, png::Renderer, SettingData) over the
C ABI of include/rtm.h; all rendering happens in hand-written HIP kernels (csrc/).
"""
from ._lib import MODE_LITERAL, MODE_REPAIRED, RtmError, lib  # noqa: F401
from .renderer import (ADAPTIVE_DEFAULTS, BLOOM_DEFAULTS, COMPARE_DEFAULTS, DEFOCUS_DEFAULTS, FIREFLY_DEFAULTS, FLIP_DEFAULTS, GRADE_DEFAULTS, GRADE_INTERPS, LENS_DEFAULTS, LENS_FILTERS, LENS_MODES, MATTE_DEFAULTS, DENOISE_DEFAULTS, DENOISE_VAR_DEFAULTS, RESIZE_DEFAULTS, RESIZE_FILTERS, SCOPE_DEFAULTS, TONEMAP_DEFAULTS, TONEMAP_LOCAL_DEFAULTS, UPSAMPLE_DEFAULTS,  # noqa: F401
                       Renderer, bloom, compare, compare_result, composite, defocus, firefly, flip, flip_result, denoise, grade, lens, lens_fit_zoom, load_cube, matte,
                       denoise_variance, intersect_batch, intersect_objects_batch, pack_spheres, path_tracing_batch, plan_passes,
                       resize, scope_bin_range, scope_draw, scope_exposure, scope_histogram, scope_percentile, scope_summary, scopes,
                       surface_sample_batch, tonemap, tonemap_local, tonemap_stats, upsample, white_balance)
from .settings import (Camera, LoadData, Material, PlaneObject, SettingData, SphereObject,  # noqa: F401
                       make_stress_scene, vec3)

__all__ = ["LoadData", "Renderer", "SettingData", "Camera", "SphereObject", "Material", "vec3",
           "make_stress_scene", "pack_spheres", "plan_passes", "denoise", "DENOISE_DEFAULTS", "denoise_variance", "DENOISE_VAR_DEFAULTS", "tonemap", "tonemap_stats", "TONEMAP_DEFAULTS", "tonemap_local", "TONEMAP_LOCAL_DEFAULTS", "bloom", "BLOOM_DEFAULTS", "defocus", "DEFOCUS_DEFAULTS", "firefly", "FIREFLY_DEFAULTS", "grade", "white_balance", "load_cube", "GRADE_DEFAULTS", "GRADE_INTERPS", "lens", "lens_fit_zoom", "LENS_DEFAULTS", "LENS_FILTERS", "LENS_MODES", "resize", "RESIZE_DEFAULTS", "RESIZE_FILTERS", "upsample", "UPSAMPLE_DEFAULTS", "compare", "compare_result", "COMPARE_DEFAULTS", "flip", "flip_result", "FLIP_DEFAULTS", "scopes", "scope_draw", "scope_histogram", "scope_percentile", "scope_exposure", "scope_bin_range", "scope_summary", "SCOPE_DEFAULTS", "matte", "composite", "MATTE_DEFAULTS", "ADAPTIVE_DEFAULTS", "path_tracing_batch", "surface_sample_batch", "intersect_batch", "intersect_objects_batch", "PlaneObject", "RtmError", "lib",
           "MODE_LITERAL", "MODE_REPAIRED"]
