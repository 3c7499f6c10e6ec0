"""The variance-guided denoiser, the parts that need no GPU: the bindings, rtm_denoise_variance's argument checks (all made
before any device call), rtm_denoise_variance_work_bytes, the CLI's refusal of the multi-GPU flags, and self-checks of the
NumPy reference."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _denoise_ref
import _denoise_var_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = C.c_size_t(-1).value
FIELDS = ("iterations", "sigma_lum", "sigma_normal", "sigma_depth")


def test_denoise_variance_is_bound_and_exported():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_denoise_variance" in _lib.SIGNATURES and "rtm_denoise_variance_work_bytes" in _lib.SIGNATURES
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "rtm_denoise_variance") and hasattr(raw, "rtm_denoise_variance_work_bytes")
    assert C.sizeof(_lib.rtm_denoise_var_params) == 16
    assert tuple(f[0] for f in _lib.rtm_denoise_var_params._fields_) == FIELDS
    assert callable(rtm.denoise_variance) and "denoise_variance" in rtm.__all__ and "DENOISE_VAR_DEFAULTS" in rtm.__all__
    params = inspect.signature(rtm.denoise_variance).parameters
    for k in ("aov",) + FIELDS + ("want", "stream"):
        assert k in params, k
    # the header, the package, the reference: one set of defaults
    assert rtm.DENOISE_VAR_DEFAULTS == _denoise_var_ref.DEFAULTS
    header = open(os.path.join(ROOT, "include", "rtm.h")).read()
    fields = re.search(r"#define RTM_DENOISE_VAR_DEFAULTS \{([^}]*)\}", header).group(1).split(",")
    assert dict(zip(FIELDS, (float(v.strip().rstrip("f")) for v in fields))) == rtm.DENOISE_VAR_DEFAULTS
    assert {k: params[k].default for k in FIELDS} == rtm.DENOISE_VAR_DEFAULTS
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump
    # rtm_denoise's own defaults did not move
    assert rtm.DENOISE_DEFAULTS == _denoise_ref.DEFAULTS == {"iterations": 4, "sigma_color": 16.0, "sigma_normal": 64.0,
                                                              "sigma_depth": 0.05}


def test_denoise_variance_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    prm = _lib.rtm_denoise_var_params(5, 4.0, 64.0, 0.05)
    guides = _lib.rtm_aov_buffers()
    color, work, out32, out8, var = (C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000),
                                     C.c_void_p(0x50000000))
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=C.byref(prm), w=8, h=8, dev=0, c=color, g=C.byref(guides), wk=work, o32=out32, o8=out8, v=var):
        return L.rtm_denoise_variance(p, w, h, dev, c, g, wk, o32, o8, v, None)

    # everything rtm_denoise refuses
    assert call(p=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(c=None) == -1
    assert call(wk=None) == -1
    assert call(o32=None, o8=None, v=None) == -1
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
        assert call(w=w, h=h, v=None) == -1, (w, h)
    for k in (-1, 11, 1 << 30):
        assert call(p=C.byref(_lib.rtm_denoise_var_params(k, 4.0, 64.0, 0.05))) == -1, k
    for field in ("sigma_lum", "sigma_normal", "sigma_depth"):
        for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            bad = _lib.rtm_denoise_var_params.from_buffer_copy(prm)
            setattr(bad, field, v)
            assert call(p=C.byref(bad)) == -1, (field, v)
    assert call(o32=color) == -1
    assert call(wk=color) == -1
    assert b"alias" in L.rtm_last_error_detail()
    assert call(wk=C.c_void_p(0x20008)) == -1  # not 16-byte aligned
    assert call(dev=-1) == -1
    # the variance output's own aliasing rules
    for other in (color, work, out32):
        assert call(v=other) == -1, other
        assert b"variance_out_dev" in L.rtm_last_error_detail()
    # a variance-only call passes the "no output" check: what refuses this one is the device number
    assert call(o32=None, o8=None, dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()


def test_variance_work_bytes_is_zero_for_no_frame_grows_with_it_and_saturates():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    for w, h in ((0, 5), (5, 0), (-4, 5), (5, -4), (0, 0), (-(2**31), -(2**31))):
        assert L.rtm_denoise_variance_work_bytes(w, h) == 0, (w, h)
    last = 0
    for w, h in ((1, 1), (1, 17), (7, 5), (37, 23), (64, 64), (130, 70), (1920, 1080), (1 << 14, 1 << 14)):
        b = L.rtm_denoise_variance_work_bytes(w, h)
        # room for rtm_denoise's planes and two float planes, and the planes after the first stay 16-byte aligned
        assert b > last and b >= L.rtm_denoise_work_bytes(w, h) + 8 * w * h and b != SIZE_MAX, (w, h)
        last = b
    for w in range(1, 40):
        assert (L.rtm_denoise_variance_work_bytes(w, 3) <= L.rtm_denoise_variance_work_bytes(w + 1, 3)
                <= L.rtm_denoise_variance_work_bytes(w + 1, 4))
    for w, h in ((2**31 - 1, 2**31 - 1), (2**31 - 1, 2**30), (2**30, 2**29)):
        assert w * h * 48 > SIZE_MAX // 2  # near or past what a size_t holds
        b = L.rtm_denoise_variance_work_bytes(w, h)
        assert b == SIZE_MAX or b >= 56 * w * h, (w, h)
    assert L.rtm_denoise_variance_work_bytes(2**31 - 1, 2**31 - 1) == SIZE_MAX


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--virtual-strips", "2"], ["--force-rccl"]])
def test_cli_denoise_variance_refuses_multi_gpu_flags_before_any_gpu(tmp_path, flags):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    r = subprocess.run([cli, "-json", scene, "--width", "8", "--height", "8", "--out", "x", "--denoise-variance"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--denoise-variance" in r.stderr
    assert not (tmp_path / "x_denoised_var.bmp").exists() and not (tmp_path / "x.bmp").exists()


def test_cli_usage_mentions_denoise_variance():
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    r = subprocess.run([cli, "-?"], capture_output=True, text=True, timeout=60)
    assert "--denoise-variance" in r.stdout + r.stderr and "_variance.pfm" in r.stdout + r.stderr


def test_render_refuses_an_unknown_denoise_mode():
    import raytracingmin_amd as rtm
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    with pytest.raises(ValueError):
        rtm.Renderer(data).Render("unused", denoise="varience")


# ---- the NumPy reference itself -------------------------------------------------------------------------------------
def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return {"color": rng.uniform(0, 2, (h, w, 3)).astype(np.float32),
            "depth": rng.uniform(1, 3, (h, w)).astype(np.float32),
            "normal": n.astype(np.float32),
            "albedo": rng.uniform(0, 1, (h, w, 3)).astype(np.float32),
            "obj": rng.integers(0, 3, (h, w)).astype(np.int32)}


def test_reference_constant_frame_is_a_fixed_point_without_variance():
    c = np.full((9, 11, 3), 0.25, np.float32)
    for k in (0, 1, 4):
        out, v0 = _denoise_var_ref.denoise_variance_ref(c, iterations=k)
        assert np.allclose(out, 0.25, rtol=1e-14) and np.array_equal(v0, np.zeros((9, 11))), k
    f = _frame(9, 11, 5)  # the same under guides: the geometry weights scale every tap's zero difference
    out, v0 = _denoise_var_ref.denoise_variance_ref(c, f["depth"], f["normal"], None, f["obj"], iterations=3)
    assert np.allclose(out, 0.25, rtol=1e-14) and np.array_equal(v0, np.zeros((9, 11)))


def test_reference_without_the_luminance_term_is_the_plain_filter_without_its_colour_term():
    f = _frame(19, 23, 6)
    f["depth"][3, 4] = f["depth"][10, 11] = np.inf
    for k in (0, 1, 3, 5):
        out, _ = _denoise_var_ref.denoise_variance_ref(f["color"], f["depth"], f["normal"], f["albedo"], f["obj"], iterations=k,
                                                       sigma_lum=0, sigma_normal=8.0, sigma_depth=0.5)
        ref = _denoise_ref.denoise_ref(f["color"], f["depth"], f["normal"], f["albedo"], f["obj"], iterations=k, sigma_color=0,
                                       sigma_normal=8.0, sigma_depth=0.5)
        assert np.max(np.abs(out - ref)) <= 1e-12, k


def test_reference_variance_of_a_checkerboard_is_the_closed_form():
    h, w = 16, 19
    yy, xx = np.mgrid[:h, :w]
    sign = np.where((yy + xx) % 2 == 0, 1.0, -1.0)
    color = np.repeat(sign[..., None], 3, axis=-1).astype(np.float32)  # luminance +-1: the weights sum to 1
    _, v0 = _denoise_var_ref.denoise_variance_ref(color, iterations=0)
    # 49 taps of weight 1: 25 of the centre's sign (d = 0), 24 of the other (d = -+2): m1 = -+48/49, m2 = 96/49
    assert np.allclose(v0[3:-3, 3:-3], 96.0 / 49 - (48.0 / 49) ** 2, rtol=1e-12, atol=0)
    assert abs(96.0 / 49 - (48.0 / 49) ** 2 - 2400.0 / 2401) < 1e-15
    # a corner sees 4 x 4 taps, 8 of each sign: m1 = -+1, m2 = 2
    assert np.isclose(v0[0, 0], 1.0, rtol=1e-12)


def test_reference_variance_ignores_other_objects_and_needs_the_shift_by_the_centre():
    rng = np.random.default_rng(9)
    obj = np.zeros((11, 11), np.int32)
    obj[5, 5] = 7  # alone among other objects: U = 1, every moment 0
    color = rng.uniform(0, 2, (11, 11, 3)).astype(np.float32)
    _, v0 = _denoise_var_ref.denoise_variance_ref(color, obj=obj, iterations=0)
    assert v0[5, 5] == 0.0 and np.all(v0[obj == 0] > 0)
    # a large offset does not change the estimate: it is one of differences
    _, shifted_v0 = _denoise_var_ref.denoise_variance_ref(color.astype(np.float64) + 1024.0, obj=obj, iterations=0)
    assert np.allclose(shifted_v0, v0, rtol=1e-9, atol=1e-12)
