"""rtm_scene_create_device and its Python side, as far as they go without a GPU: the symbols, the argument checks that come
before any device call, pack_spheres' byte layout, and the tensors Renderer.set_device_spheres refuses."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd
    return raytracingmin_amd


def test_symbols_are_exported_and_bound(rtm):
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "rtm_scene_create_device") and hasattr(raw, "rtm_debug_scene_grid")
    assert "rtm_scene_create_device" in _lib.SIGNATURES and "rtm_debug_scene_grid" in _lib.DEBUG_SIGNATURES
    assert rtm.lib().rtm_scene_create_device.argtypes is not None


def test_argument_errors_come_before_any_device_call(rtm):
    """A null out_scene, null spheres_dev with n > 0, n > 0x7FFFFFFF and a negative device: RTM_ERR_INVALID_ARGUMENT (-1),
    on a machine without a device too (a device call would give RTM_ERR_HIP or RTM_ERR_NO_DEVICE there)."""
    L = rtm.lib()
    h = C.c_void_p()
    fake = C.c_void_p(0x1000)  # never dereferenced: the checks come first
    assert L.rtm_scene_create_device(fake, 100, 0, None, None) == -1
    assert L.rtm_scene_create_device(None, 100, 0, None, C.byref(h)) == -1
    assert L.rtm_scene_create_device(fake, 0x80000000, 0, None, C.byref(h)) == -1
    assert L.rtm_scene_create_device(fake, 100, -1, None, C.byref(h)) == -1
    assert L.rtm_last_error_detail()
    assert h.value is None
    info = (C.c_uint64 * 12)()
    assert L.rtm_debug_scene_grid(None, info, None, 0, None, 0, None, 0, None) == -1


def _small_scene(rtm):
    data = rtm.make_stress_scene(n=37, seed=5)
    data.object[3].m_size = 0.1  # a radius that is not a float: pack_spheres rounds it as spheres_c does
    data.object[4].m_material.emission = rtm.vec3(1.5, 0.25, 3.0)
    return data


def _columns(data):
    import torch
    c = torch.tensor([list(o.m_position) for o in data.object], dtype=torch.float64)
    r = torch.tensor([o.m_size for o in data.object], dtype=torch.float64)
    col = torch.tensor([list(o.m_material.color) for o in data.object], dtype=torch.float64)
    em = torch.tensor([list(o.m_material.emission) for o in data.object], dtype=torch.float64)
    return c, r, col, em


def test_pack_spheres_is_the_c_layout(rtm):
    import torch
    data = _small_scene(rtm)
    arr, n = data.spheres_c()
    packed = rtm.pack_spheres(*_columns(data))
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (n, 80)
    assert packed.numpy().tobytes() == bytes(arr)[:n * 80]
    assert not packed.numpy()[:, 76:].any()  # the pad bytes
    empty = rtm.pack_spheres(torch.zeros((0, 3), dtype=torch.float64), torch.zeros(0), torch.zeros((0, 3), dtype=torch.float64),
                             torch.zeros((0, 3), dtype=torch.float64))
    assert tuple(empty.shape) == (0, 80)


def test_pack_spheres_refuses_bad_tensors(rtm):
    import torch
    c, r, col, em = _columns(_small_scene(rtm))
    for bad in ((c.float(), r, col, em), (c, r, col[:, :2], em), (c, r[:-1], col, em), (c, r, col, em[:-1]),
                (c.numpy(), r, col, em), (c.reshape(-1), r, col, em)):
        with pytest.raises(ValueError):
            rtm.pack_spheres(*bad)


def test_set_device_spheres_refuses_bad_tensors(rtm):
    import torch
    data = _small_scene(rtm)
    r = rtm.Renderer(data)
    good = rtm.pack_spheres(*_columns(data))
    for bad in (good.numpy(), good.to(torch.int8), good[:, :79], good.reshape(-1), good.view(torch.float64),
                good.t(),   # (80, n): the wrong shape
                good):      # a CPU tensor: the wrong device
        with pytest.raises(ValueError):
            r.set_device_spheres(bad)
    r.set_device_spheres(None)  # nothing to drop: fine
    assert r._device_scene is None
