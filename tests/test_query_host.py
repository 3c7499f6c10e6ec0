"""Ray queries on a scene (include/rtm.h: rtm_scene_nearest, rtm_scene_occluded; include/rtm_debug.h: rtm_debug_scene_query):
the symbols are exported and bound, and every refusal comes with a text before anything touches a device (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from raytracingmin_amd import _lib
    return _lib.lib()


def test_query_symbols_are_exported_and_bound(L):
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("rtm_scene_nearest", "rtm_scene_occluded"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert hasattr(raw, "rtm_debug_scene_query") and "rtm_debug_scene_query" in _lib.DEBUG_SIGNATURES
    assert C.sizeof(_lib.rtm_hit_buffers) == 24
    assert L.rtm_abi_version() == 5
    assert callable(rtm.Renderer.nearest) and callable(rtm.Renderer.occluded)
    assert rtm.Renderer.QUERY_PLANES == ("object", "t", "normal")


# A scene pointer that is never looked into: every refusal below comes before the scene is read.
_SCENE = C.c_void_p(0x1000)
_BUF = np.zeros(64, dtype=np.float64)
_P = _BUF.ctypes.data  # 8-byte aligned, never written: every call below is refused


def _hits(obj=None, t=None, normal=None):
    from raytracingmin_amd import _lib
    b = _lib.rtm_hit_buffers()
    b.object, b.t, b.normal = obj, t, normal
    return b


def _refused(L, status, *words):
    assert status == -1
    text = (L.rtm_last_error_detail() or b"").decode()
    assert text and all(w in text for w in words), text


def test_nearest_refusals_need_no_device(L):
    ok = _hits(obj=_P, t=_P + 64, normal=_P + 128)
    _refused(L, L.rtm_scene_nearest(None, _P, _P, 4, C.byref(ok), None), "scene")
    _refused(L, L.rtm_scene_nearest(_SCENE, None, _P, 4, C.byref(ok), None), "org_dev")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, None, 4, C.byref(ok), None), "dir_dev")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, _P, 4, None, None), "out_dev")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, _P, 4, C.byref(_hits()), None), "every plane")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P + 4, _P, 4, C.byref(ok), None), "aligned")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, _P + 1, 4, C.byref(ok), None), "aligned")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, _P, 4, C.byref(_hits(obj=_P + 2)), None), "aligned")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, _P, 4, C.byref(_hits(t=_P + 4)), None), "aligned")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, _P, 4, C.byref(_hits(normal=_P + 4)), None), "aligned")
    _refused(L, L.rtm_scene_nearest(_SCENE, _P, _P, 0x80000000, C.byref(ok), None), "n_rays")
    # an object plane needs 4 bytes only
    _refused(L, L.rtm_scene_nearest(None, _P, _P, 4, C.byref(_hits(obj=_P + 4)), None), "scene")


def test_occluded_refusals_need_no_device(L):
    _refused(L, L.rtm_scene_occluded(None, _P, _P, None, 4, _P, None), "scene")
    _refused(L, L.rtm_scene_occluded(_SCENE, None, _P, None, 4, _P, None), "org_dev")
    _refused(L, L.rtm_scene_occluded(_SCENE, _P, None, None, 4, _P, None), "dir_dev")
    _refused(L, L.rtm_scene_occluded(_SCENE, _P, _P, None, 4, None, None), "out_dev")
    _refused(L, L.rtm_scene_occluded(_SCENE, _P + 4, _P, None, 4, _P, None), "aligned")
    _refused(L, L.rtm_scene_occluded(_SCENE, _P, _P + 4, None, 4, _P, None), "aligned")
    _refused(L, L.rtm_scene_occluded(_SCENE, _P, _P, _P + 4, 4, _P, None), "aligned")
    _refused(L, L.rtm_scene_occluded(_SCENE, _P, _P, _P, 0x80000000, _P, None), "n_rays")
    # bytes have no alignment
    _refused(L, L.rtm_scene_occluded(None, _P, _P, _P, 4, _P + 1, None), "scene")


def test_counting_hook_refusals_need_no_device(L):
    q = L.rtm_debug_scene_query
    _refused(L, q(None, 0, _P, _P, None, 4, _P, _P, _P, _P, _P, None), "scene")
    _refused(L, q(_SCENE, 2, _P, _P, None, 4, _P, _P, _P, _P, _P, None), "any")
    _refused(L, q(_SCENE, 0, None, _P, None, 4, _P, _P, _P, _P, _P, None), "org_dev")
    _refused(L, q(_SCENE, 1, _P, _P, None, 4, None, None, None, None, None, None), "every output")
    _refused(L, q(_SCENE, 1, _P, _P, _P + 4, 4, _P, _P, _P, _P, _P, None), "aligned")
    _refused(L, q(_SCENE, 1, _P, _P, None, 4, _P, _P + 4, _P, _P, _P, None), "aligned")
    _refused(L, q(_SCENE, 1, _P, _P, None, 0x80000000, _P, _P, _P, _P, _P, None), "n_rays")
