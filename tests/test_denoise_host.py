"""The à-trous denoiser, the parts that need no GPU: the bindings, rtm_denoise's argument checks (all made before any device
call), rtm_denoise_work_bytes, the CLI's refusal of the multi-GPU flags, and self-checks of the NumPy reference."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _denoise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_denoise_is_bound_and_exported():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_denoise" in _lib.SIGNATURES and "rtm_denoise_work_bytes" in _lib.SIGNATURES
    assert C.sizeof(_lib.rtm_denoise_params) == 16
    assert callable(rtm.denoise) and "denoise" in rtm.__all__
    assert "denoise" in inspect.signature(rtm.Renderer.Render).parameters
    params = inspect.signature(rtm.denoise).parameters
    for k in ("aov", "iterations", "sigma_color", "sigma_normal", "sigma_depth", "want", "stream"):
        assert k in params, k
    assert rtm.DENOISE_DEFAULTS == _denoise_ref.DEFAULTS
    header = open(os.path.join(ROOT, "include", "rtm.h")).read()
    fields = re.search(r"#define RTM_DENOISE_DEFAULTS \{([^}]*)\}", header).group(1).split(",")
    assert dict(zip(("iterations", "sigma_color", "sigma_normal", "sigma_depth"),
                    (float(v.strip().rstrip("f")) for v in fields))) == rtm.DENOISE_DEFAULTS
    assert {k: params[k].default for k in rtm.DENOISE_DEFAULTS} == rtm.DENOISE_DEFAULTS
    assert _lib.lib().rtm_abi_version() == 5


def test_denoise_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    prm = _lib.rtm_denoise_params(5, 1.0, 64.0, 0.05)
    guides = _lib.rtm_aov_buffers()
    color, work, out32, out8 = C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000)
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=C.byref(prm), w=8, h=8, dev=0, c=color, g=C.byref(guides), wk=work, o32=out32, o8=out8):
        return L.rtm_denoise(p, w, h, dev, c, g, wk, o32, o8, None)

    assert call(p=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(c=None) == -1
    assert call(wk=None) == -1
    assert call(o32=None, o8=None) == -1
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for k in (-1, 11, 1 << 30):
        assert call(p=C.byref(_lib.rtm_denoise_params(k, 1.0, 64.0, 0.05))) == -1, k
    for field in ("sigma_color", "sigma_normal", "sigma_depth"):
        for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            bad = _lib.rtm_denoise_params.from_buffer_copy(prm)
            setattr(bad, field, v)
            assert call(p=C.byref(bad)) == -1, (field, v)
    assert call(o32=color) == -1
    assert call(wk=color) == -1
    assert b"alias" in L.rtm_last_error_detail()
    assert call(wk=C.c_void_p(0x20008)) == -1  # not 16-byte aligned
    assert call(dev=-1) == -1


def test_work_bytes_is_zero_for_no_frame_and_grows_with_it():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    assert L.rtm_denoise_work_bytes(0, 5) == 0
    assert L.rtm_denoise_work_bytes(5, 0) == 0
    assert L.rtm_denoise_work_bytes(-4, 5) == 0
    last = 0
    for w, h in ((1, 1), (1, 17), (37, 23), (64, 64), (130, 70), (1920, 1080), (1 << 20, 1 << 20), (2**31 - 1, 2**31 - 1)):
        b = L.rtm_denoise_work_bytes(w, h)
        assert b >= last and b >= 48 * min(w * h, 2**58), (w, h)
        last = b
    for w in range(1, 40):
        assert L.rtm_denoise_work_bytes(w, 3) <= L.rtm_denoise_work_bytes(w + 1, 3) <= L.rtm_denoise_work_bytes(w + 1, 4)


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--virtual-strips", "2"], ["--force-rccl"]])
def test_cli_denoise_refuses_multi_gpu_flags_before_any_gpu(tmp_path, flags):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    r = subprocess.run([cli, "-json", scene, "--width", "8", "--height", "8", "--out", "x", "--denoise"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--denoise" in r.stderr
    assert not (tmp_path / "x_denoised.bmp").exists() and not (tmp_path / "x.bmp").exists()


def test_cli_usage_mentions_denoise():
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    r = subprocess.run([cli, "-?"], capture_output=True, text=True, timeout=60)
    assert "--denoise" in r.stdout + r.stderr


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


def test_reference_k0_is_the_identity():
    f = _frame(9, 13, 1)
    out = _denoise_ref.denoise_ref(f["color"], f["depth"], f["normal"], f["albedo"], f["obj"], iterations=0)
    assert np.array_equal(out, f["color"].astype(np.float64))


def test_reference_pixel_among_other_objects_keeps_its_colour():
    f = _frame(11, 11, 2)
    obj = np.zeros((11, 11), np.int32)
    obj[5, 5] = 7
    for k in (1, 3, 5):
        out = _denoise_ref.denoise_ref(f["color"], f["depth"], f["normal"], f["albedo"], obj, iterations=k)
        assert np.allclose(out[5, 5], f["color"][5, 5], rtol=1e-12, atol=0), k


def test_reference_constant_frame_is_a_fixed_point_and_weights_switch_off():
    c = np.full((6, 7, 3), 0.25, np.float32)
    assert np.allclose(_denoise_ref.denoise_ref(c, iterations=4), 0.25, rtol=1e-14)
    f = _frame(8, 8, 3)
    # every sigma 0 and no guides: a plain normalised B3-spline blur, the same with or without the zero-sigma planes
    plain = _denoise_ref.denoise_ref(f["color"], iterations=2, sigma_color=0, sigma_normal=0, sigma_depth=0)
    guided = _denoise_ref.denoise_ref(f["color"], depth=f["depth"], normal=f["normal"], iterations=2, sigma_color=0,
                                      sigma_normal=0, sigma_depth=0)
    assert np.array_equal(plain, guided)
