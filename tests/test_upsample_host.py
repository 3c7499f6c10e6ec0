"""The AOV-guided upsampler, the parts that need no GPU: the bindings, rtm_upsample_work_bytes, rtm_upsample's argument checks
(all made before any device call), the integer tap rule against a float64 brute force, properties of the NumPy reference,
Renderer.preview's factor check and the CLI's refusals."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _upsample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")


def test_upsample_is_bound_and_exported():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_upsample" in _lib.SIGNATURES and "rtm_upsample_work_bytes" in _lib.SIGNATURES
    assert C.sizeof(_lib.rtm_upsample_params) == 16
    assert callable(rtm.upsample) and "upsample" in rtm.__all__ and "UPSAMPLE_DEFAULTS" in rtm.__all__
    assert "preview" in inspect.signature(rtm.Renderer.Render).parameters
    params = inspect.signature(rtm.upsample).parameters
    for k in ("color_low", "aov_low", "aov_high", "factor", "sigma_spatial", "sigma_normal", "sigma_depth", "want", "stream"):
        assert k in params, k
    assert rtm.UPSAMPLE_DEFAULTS == _upsample_ref.DEFAULTS
    header = open(os.path.join(ROOT, "include", "rtm.h")).read()
    fields = re.search(r"#define RTM_UPSAMPLE_DEFAULTS \{([^}]*)\}", header).group(1).split(",")
    assert dict(zip(("factor", "sigma_spatial", "sigma_normal", "sigma_depth"),
                    (float(v.strip().rstrip("f")) for v in fields))) == rtm.UPSAMPLE_DEFAULTS
    assert {k: params[k].default for k in rtm.UPSAMPLE_DEFAULTS} == rtm.UPSAMPLE_DEFAULTS
    assert rtm.UPSAMPLE_DEFAULTS["sigma_normal"] == rtm.DENOISE_DEFAULTS["sigma_normal"]
    assert rtm.UPSAMPLE_DEFAULTS["sigma_depth"] == rtm.DENOISE_DEFAULTS["sigma_depth"]
    preview = inspect.signature(rtm.Renderer.preview).parameters
    assert preview["factor"].default == 2 and preview["denoise"].default is True
    assert _lib.lib().rtm_abi_version() == 5


def test_work_bytes():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    assert L.rtm_upsample_work_bytes(0, 5) == 0
    assert L.rtm_upsample_work_bytes(5, 0) == 0
    assert L.rtm_upsample_work_bytes(-4, 5) == 0
    assert L.rtm_upsample_work_bytes(3, 2) == 192
    assert L.rtm_upsample_work_bytes(960, 540) == 32 * 960 * 540
    size_max = C.c_size_t(-1).value
    # 12 bytes x 64 full-resolution pixels per low pixel must fit a size_t
    assert L.rtm_upsample_work_bytes(2**31 - 1, 2**31 - 1) == size_max
    assert L.rtm_upsample_work_bytes(1 << 20, 1 << 20) == 32 << 40


def test_upsample_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    prm = _lib.rtm_upsample_params(2, 0.5, 64.0, 0.05)
    color, work, out32, out8 = C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000)
    # fake device pointers: never dereferenced, every call below fails its checks first

    def guides(**planes):
        g = _lib.rtm_aov_buffers()
        for k, v in planes.items():
            setattr(g, k, v)
        return C.byref(g)

    full = dict(depth=0x5000, normal=0x6000, albedo=0x7000, object=0x8000)

    def call(p=C.byref(prm), w=8, h=8, dev=0, c=color, lo=guides(**full), hi=guides(**full), wk=work, o32=out32, o8=out8):
        return L.rtm_upsample(p, w, h, dev, c, lo, hi, wk, o32, o8, None)

    assert call(p=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(c=None) == -1
    assert call(wk=None) == -1
    assert call(o32=None, o8=None) == -1
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for f in (-1, 0, 1, 9, 1 << 30):
        assert call(p=C.byref(_lib.rtm_upsample_params(f, 0.5, 64.0, 0.05))) == -1, f
    for v in (0.0, 0.2499, 4.001, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(p=C.byref(_lib.rtm_upsample_params(2, v, 64.0, 0.05))) == -1, v
    for field in ("sigma_normal", "sigma_depth"):
        for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            bad = _lib.rtm_upsample_params.from_buffer_copy(prm)
            setattr(bad, field, v)
            assert call(p=C.byref(bad)) == -1, (field, v)
    # the pairing rule: a plane in exactly one struct, or exactly one struct
    for k in full:
        one = dict(full)
        del one[k]
        assert call(lo=guides(**one)) == -1, k
        assert call(hi=guides(**one)) == -1, k
        assert b"one resolution" in L.rtm_last_error_detail()
    assert call(lo=None) == -1
    assert call(hi=None) == -1
    assert call(wk=C.c_void_p(0x20008)) == -1  # not 16-byte aligned
    assert call(o32=work) == -1
    assert call(o8=work) == -1
    assert call(o32=color) == -1
    assert call(o8=color) == -1
    assert b"alias" in L.rtm_last_error_detail()
    assert call(dev=-1) == -1


# ---- the tap rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(2, 9))
def test_tap_rule_matches_the_float64_brute_force(f):
    n = 3 * f + 1
    x0, r = _upsample_ref.tap_base(n, f)
    for x in range(n):
        c = (x + 0.5) / f - 0.5  # the pixel centre in low-resolution pixel coordinates: exact enough in float64
        assert x0[x] == math.floor(c), (f, x)
        assert 0 <= r[x] < 2 * f
        assert abs(r[x] / (2.0 * f) - (c - math.floor(c))) < 1e-12, (f, x)
    assert x0[0] == -1 and np.all(np.diff(x0) >= 0)
    # the nearest tap is inside the frame for every x of a 1-wide low frame
    x0, r = _upsample_ref.tap_base(f, f)
    nearest = x0 + (2 * r >= 2 * f)  # t >= 1/2: the tap dx = 1
    assert np.all(nearest == 0), (f, nearest)
    # the weights depend on x mod f only: 4 f values per axis
    x0, r = _upsample_ref.tap_base(4 * f, f)
    assert np.array_equal(r[:f], r[f:2 * f]) and len(set(r.tolist())) == f


# ---- the NumPy reference itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", (2, 3, 8))
def test_reference_keeps_a_constant_frame(f):
    c = np.full((5, 6, 3), 0.375, np.float32)
    out = _upsample_ref.upsample_ref(c, factor=f)
    assert out.shape == (5 * f, 6 * f, 3)
    assert np.max(np.abs(out - 0.375)) <= 1e-12


@pytest.mark.parametrize("f", (2, 4))
def test_reference_edges_between_objects_are_hard(f):
    """Two constant regions that meet on a low pixel boundary.  Every pixel's nearest tap (at most half a low pixel away in
    each axis) carries its own object with weight h >= exp(-1/4 / (2 sigma^2))^2 = 0.368 at sigma_spatial 0.5, and the taps of
    the other object share 1e-6 of at most (sum of h_x)(sum of h_y) <= 1.27^2: under 4.4e-6 of the step of 1 crosses."""
    h, w = 6, 8
    obj_hi = np.zeros((h * f, w * f), np.int32)
    obj_hi[:, (w // 2) * f:] = 1
    high = {"object": obj_hi}
    low = {"object": _upsample_ref.sample_low(obj_hi, f)}
    color = np.repeat(low["object"].astype(np.float32)[..., None], 3, axis=2)
    out, matched, den = _upsample_ref.upsample_ref(color, low, high, factor=f, return_weights=True)
    assert matched.all() and np.all(den > 0)
    assert np.max(np.abs(out - obj_hi[..., None])) <= 1e-5


def test_reference_thin_feature_falls_back_to_the_spatial_average():
    color, low, high, thin = _upsample_ref.synthetic_case(9, 5, 3, 4)
    lo, hi = {"object": low["object"]}, {"object": high["object"]}
    out, matched, _ = _upsample_ref.upsample_ref(color, lo, hi, factor=3, return_weights=True)
    plain = _upsample_ref.upsample_ref(color, factor=3)
    assert thin.any() and not matched[thin].any()
    assert np.allclose(out[thin], plain[thin], rtol=1e-12, atol=0)
    assert not np.allclose(out[~thin], plain[~thin], rtol=1e-3, atol=0)


# ---- the Python layer and the CLI -----------------------------------------------------------------------------------
def test_preview_refuses_a_factor_that_does_not_divide_the_frame():
    import raytracingmin_amd as rtm
    data = rtm.LoadData(SCENE).data
    data.width, data.height = 64, 48
    r = rtm.Renderer(data)
    for f in (5, 7):
        with pytest.raises(ValueError, match="divide"):
            r.preview(factor=f)
    for f in (0, 1, 9):
        with pytest.raises(ValueError):
            r.preview(factor=f)
    with pytest.raises(ValueError):
        r.Render("never_written", preview=5)
    assert not os.path.exists("never_written.bmp")


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--virtual-strips", "2"], ["--force-rccl"]])
def test_cli_preview_refuses_multi_gpu_flags_before_any_gpu(tmp_path, flags):
    r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x", "--preview", "2"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--preview" in r.stderr
    assert not (tmp_path / "x_preview.bmp").exists() and not (tmp_path / "x.bmp").exists()


@pytest.mark.parametrize("flags,word", [(["--preview-only"], "--preview"),
                                        (["--preview", "2", "--preview-only", "--adaptive", "0.05"], "--adaptive"),
                                        (["--preview", "2", "--preview-only", "--passes", "2"], "--passes"),
                                        (["--preview", "9"], "2..8"), (["--preview", "3"], "divide")])
def test_cli_preview_refusals(tmp_path, flags, word):
    r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert word in r.stderr
    assert not list(tmp_path.glob("x*"))


def test_cli_usage_mentions_preview():
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    assert "--preview F" in r.stdout and "--preview-only" in r.stdout
