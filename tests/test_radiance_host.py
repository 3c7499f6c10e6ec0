"""Radiance queries on a scene (include/rtm.h: rtm_scene_radiance): the symbol is exported and bound, the structs have the
header's sizes, and every refusal comes with a text before anything touches a device (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -8
REPAIRED, LITERAL, HOST_TRIG, COUNT_TESTS, SURFACE_SAMPLE = 1, 0, 0x100, 0x200, 0x400


@pytest.fixture(scope="module")
def L():
    from raytracingmin_amd import _lib
    return _lib.lib()


def test_radiance_symbol_is_exported_and_bound(L):
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "rtm_scene_radiance") and "rtm_scene_radiance" in _lib.SIGNATURES
    assert C.sizeof(_lib.rtm_radiance_params) == 32 and C.sizeof(_lib.rtm_radiance_buffers) == 24
    assert _lib.rtm_radiance_params.seed.offset == 8 and _lib.rtm_radiance_params.samples.offset == 16
    assert _lib.RADIANCE_CLAMP == 1
    assert L.rtm_abi_version() == 5
    assert callable(rtm.Renderer.radiance)
    assert rtm.Renderer.RADIANCE_PLANES == ("radiance", "casts", "draws")


# A scene pointer that is never looked into: every refusal below comes before the scene is read.
_SCENE = C.c_void_p(0x1000)
_BUF = np.zeros(64, dtype=np.float64)
_P = _BUF.ctypes.data  # 8-byte aligned, never written: every call below is refused


def _bufs(radiance=None, casts=None, draws=None):
    from raytracingmin_amd import _lib
    b = _lib.rtm_radiance_buffers()
    b.radiance, b.casts, b.draws = radiance, casts, draws
    return b


def _prm(mode=REPAIRED | HOST_TRIG, max_bounces=-1, seed=0x5EED, samples=4, key_base=0, flags=0, reserved=0):
    from raytracingmin_amd import _lib
    return _lib.rtm_radiance_params(mode, max_bounces, seed, samples, key_base, flags, reserved)


def _refused(L, status, *words, code=INVALID):
    assert status == code
    text = (L.rtm_last_error_detail() or b"").decode()
    assert text and all(w in text for w in words), text


def test_radiance_refusals_need_no_device(L):
    q = L.rtm_scene_radiance
    ok, prm = _bufs(radiance=_P, casts=_P + 64, draws=_P + 128), _prm()
    _refused(L, q(None, _P, _P, 4, C.byref(prm), C.byref(ok), None), "scene")
    _refused(L, q(_SCENE, None, _P, 4, C.byref(prm), C.byref(ok), None), "org_dev")
    _refused(L, q(_SCENE, _P, None, 4, C.byref(prm), C.byref(ok), None), "dir_dev")
    _refused(L, q(_SCENE, _P, _P, 4, None, C.byref(ok), None), "params")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(prm), None, None), "out_dev")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(prm), C.byref(_bufs()), None), "every plane")
    _refused(L, q(_SCENE, _P + 4, _P, 4, C.byref(prm), C.byref(ok), None), "aligned")
    _refused(L, q(_SCENE, _P, _P + 1, 4, C.byref(prm), C.byref(ok), None), "aligned")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(prm), C.byref(_bufs(radiance=_P + 4)), None), "aligned")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(prm), C.byref(_bufs(casts=_P + 2)), None), "aligned")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(prm), C.byref(_bufs(draws=_P + 6)), None), "aligned")
    _refused(L, q(_SCENE, _P, _P, 0x80000000, C.byref(prm), C.byref(ok), None), "n_rays")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(key_base=0xFFFFFFFD)), C.byref(ok), None), "key_base")
    _refused(L, q(_SCENE, _P, _P, 0x7FFFFFFF, C.byref(_prm(key_base=0x80000002)), C.byref(ok), None), "key_base")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(samples=0)), C.byref(ok), None), "samples")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(max_bounces=-2)), C.byref(ok), None), "max_bounces")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(flags=2)), C.byref(ok), None), "flags")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(flags=0x80000001)), C.byref(ok), None), "flags")
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(reserved=1)), C.byref(ok), None), "reserved")
    for mode in (2, 7, REPAIRED | COUNT_TESTS, REPAIRED | 0x800, -1 & 0x7FFFFBFF):
        _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(mode=mode)), C.byref(ok), None), "mode")
    for mode in (REPAIRED | SURFACE_SAMPLE, LITERAL | HOST_TRIG | SURFACE_SAMPLE):
        _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(mode=mode)), C.byref(ok), None), "SURFACE_SAMPLE", code=UNSUPPORTED)
    _refused(L, q(_SCENE, _P, _P, 4, C.byref(_prm(max_bounces=977)), C.byref(ok), None), "976", code=UNSUPPORTED)
    # casts and draws need 4 bytes only; the last key of the last ray may be 2^32 - 1; no rays: nothing to refuse, nothing to do
    _refused(L, q(None, _P, _P, 4, C.byref(_prm(key_base=0xFFFFFFFC)), C.byref(_bufs(casts=_P + 4, draws=_P + 12)), None), "scene")
    assert q(_SCENE, _P, _P, 0, C.byref(prm), C.byref(ok), None) == 0
